"""The yardstick of the row sort and the duplicate removal (tests/unique_ref.py) against a second definition, on the CPU: the value
of a row as a Python integer built bit by bit from the definition of include/m4ri_hip_unique.h, the order by sorted() on (value, row)
and the kept rows by a loop over the rows before each row.  No library, no device."""
import numpy as np
import pytest

import gf2util as g
import unique_ref as ur

CASES = [(1, 0, 1), (64, 0, 64), (65, 0, 65), (65, 64, 65), (130, 1, 129), (200, 57, 57), (200, 57, 87), (200, 57, 88), (200, 63, 193),
         (257, 63, 257), (300, 128, 192), (300, 0, 300)]


def big_values(words, ncols, c0, c1):
    bits = g.words_to_bits(words, ncols) if len(words) else np.zeros((0, ncols), dtype=np.uint8)
    return [sum(int(row[c0 + j]) << j for j in range(c1 - c0)) for row in bits]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%d-c%d-%d" % c)
def test_the_yardstick_against_big_integers(case):
    ncols, c0, c1 = case
    rng = np.random.default_rng(ncols + c0)
    for n in (0, 1, 2, 57, 300):
        pool = g.random_words(max(n // 3, 1), ncols, 7 + n)
        words = pool[rng.integers(0, len(pool), n)].copy()                          # classes of several members
        if n >= 57 and c1 - c0 >= 2:
            words[5] = words[40]
            words[5, (c1 - 1) // 64] ^= np.uint64(1 << ((c1 - 1) % 64))               # differ in the most significant column alone
            words[6] = words[41]
            words[6, c0 // 64] ^= np.uint64(1 << (c0 % 64))                           # ... in the least significant one
        if n >= 57 and c0 > 0 and c1 < ncols:
            words[7] = words[42]
            words[7, (c0 - 1) // 64] ^= np.uint64(1 << ((c0 - 1) % 64))               # outside the range: equal
            words[7, c1 // 64] ^= np.uint64(1 << (c1 % 64))
        v = big_values(words, ncols, c0, c1)
        got = ur.everything(words, c0, c1)
        order = sorted(range(n), key=lambda i: (v[i], i))
        assert got.order.tolist() == order and got.order.dtype == np.int32
        head = []
        for s in range(n):
            head.append(s if s == 0 or v[order[s]] != v[order[s - 1]] else head[-1])
        assert got.head.tolist() == head
        rep = [min(j for j in range(i + 1) if v[j] == v[i]) for i in range(n)]
        assert got.rep.tolist() == rep and got.keep.tolist() == [i for i in range(n) if rep[i] == i]
        assert got.count == len(set(v)) == len(got.keep)
        if n >= 57 and c0 > 0 and c1 < ncols:
            assert rep[42] == rep[7] <= 7                                             # bits outside the range do not count
        # the words of the range hold exactly the value
        rw = ur.range_words(words, c0, c1)
        assert [sum(int(x) << (64 * k) for k, x in enumerate(row)) for row in rw] == v
