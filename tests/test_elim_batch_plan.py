"""CPU tests of the batched elimination's host side (elim_batch_host.cpp): gf2_elim_batch_plan over every shape class, and the
argument checks of gf2_echelonize_batch_dev / gf2_inverse_batch_dev, which come before a device is required -- this runs without one."""
import ctypes

import pytest

from elim_batch_cases import INVERSE_SIZES, SHAPES

MAX_ROWS, MAX_COLS, LDS_PER_CU = 512, 1024, 163840
# 1, 63, 64, 65, 127, 128, 129, ..., 1023, 1024: every word boundary and its neighbours
COLS = sorted({c for w in range(1, 17) for c in (64 * w - 1, 64 * w, 64 * w + 1) if c <= MAX_COLS} | {1})


@pytest.fixture(scope="module")
def pkg(built):
    import m4ri_rust_amd as p
    return p


@pytest.fixture(scope="module")
def dev(pkg):
    from m4ri_rust_amd import device
    return device


def plan(pkg, m, ncols, inverse):
    out = (ctypes.c_longlong * 4)(-1, -1, -1, -1)
    return pkg._lib.lib().gf2_elim_batch_plan(m, ncols, inverse, out), list(out)


def test_every_shape_inside_the_limits_has_a_variant(pkg):
    for m in range(1, MAX_ROWS + 1):
        for ncols in COLS:
            v, (threads, mats, lds, held) = plan(pkg, m, ncols, 0)
            w = (ncols + 63) // 64
            assert v >= 0, (m, ncols)
            assert 64 <= threads <= 1024 and threads % 64 == 0 and mats >= 1 and 0 <= lds <= LDS_PER_CU and w <= held <= 16, (m, ncols)
            if m <= 64:  # a wave per matrix: no LDS, the smallest register width of 1, 2, 4, 8, 16 that holds the row
                assert lds == 0 and mats == threads // 64 and held in (1, 2, 4, 8, 16) and held < 2 * w, (m, ncols)
            else:  # a workgroup per matrix: a thread per row, the rows at an odd stride in LDS
                assert mats == 1 and m <= threads < m + 64 and held == w and lds >= m * (w | 1) * 8, (m, ncols)


def test_every_inverse_inside_the_limits_has_a_variant(pkg):
    for n in range(1, MAX_ROWS + 1):
        v, (threads, mats, lds, held) = plan(pkg, n, n, 1)
        w = (n + 63) // 64
        assert v >= 0 and 64 <= threads <= 1024 and 0 <= lds <= LDS_PER_CU and held == 2 * w, n  # [A | I]
        assert (lds == 0) == (n <= 64), n
        for ncols in COLS:
            if ncols != n:  # the inverse is of square blocks
                assert plan(pkg, n, ncols, 1)[0] == -1, (n, ncols)


def test_echelon_and_inverse_variants_are_distinct_kernels(pkg):
    assert not {plan(pkg, m, c, 0)[0] for m in (1, 64, 65, 512) for c in COLS} & {plan(pkg, n, n, 1)[0] for n in (1, 64, 65, 512)}


@pytest.mark.parametrize("m,ncols", [(0, 10), (-1, 10), (513, 10), (10, 0), (10, -5), (10, 1025), (512, 2048), (1 << 20, 1 << 20)])
def test_shapes_outside_the_limits(pkg, m, ncols):
    for inverse in (0, 1):
        v, out = plan(pkg, m, ncols, inverse)
        assert v == -1 and out == [0, 0, 0, 0]
    assert plan(pkg, 513, 513, 1)[0] == -1 and plan(pkg, 0, 0, 1)[0] == -1


def test_the_gpu_suite_reaches_every_variant(pkg):
    """Every kernel of gf2_elim_batch.hip is one variant id, so the shapes of the GPU tests launch all of them (the census test at the
    end of the GPU suite asks for that)."""
    every = {plan(pkg, m, c, 0)[0] for m in range(1, MAX_ROWS + 1) for c in COLS} | {plan(pkg, n, n, 1)[0] for n in range(1, MAX_ROWS + 1)}
    reached = {plan(pkg, m, c, 0)[0] for m, c, _ in SHAPES} | {plan(pkg, n, n, 1)[0] for n, _ in INVERSE_SIZES}
    assert -1 not in reached
    assert reached == every, sorted(every - reached)
    assert len(every) == 8  # rows of 1, 2, 4, 8, 16 words in a wave, the wave inverse, LDS echelon form and LDS inverse


def test_python_plan(dev):
    assert dev.elim_batch_plan(64, 64) == (0, 256, 4, 0, 1)
    assert dev.elim_batch_plan(64, 64, inverse=True)[4] == 2
    assert dev.elim_batch_plan(512, 1024)[1:3] == (512, 1) and dev.elim_batch_plan(512, 1024)[3] <= LDS_PER_CU
    assert dev.elim_batch_plan(513, 64) is None and dev.elim_batch_plan(10, 12, inverse=True) is None


# ---- argument checks: -1 and a message, without a device and without a HIP call ----------------------------------------------------

ALIGNED = 1 << 20  # an address that is never dereferenced: every call below is refused before the first HIP call


def stack(pkg, nrows, ncols, ld=None, data=ALIGNED):
    s = pkg._lib.DMatStruct()
    s.data, s.ld, s.nrows, s.ncols = data, ld if ld is not None else ((ncols + 63) // 64 + 1) & ~1, nrows, ncols
    return s


def refused(pkg, rc, *words):
    msg = pkg._lib.lib().gf2_last_error().decode()
    assert rc == -1, (rc, msg)
    assert all(w in msg for w in words), msg


def ech(pkg, A, m, full=1, limit=0):
    return pkg._lib.lib().gf2_echelonize_batch_dev(ctypes.byref(A) if A is not None else None, m, full, limit, None, None, None)


def inv(pkg, Ainv, A, n):
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    return pkg._lib.lib().gf2_inverse_batch_dev(ref(Ainv), ref(A), n, None, None)


def test_echelonize_batch_argument_errors(pkg):
    refused(pkg, ech(pkg, None, 10), "gf2_echelonize_batch_dev", "null")
    refused(pkg, ech(pkg, stack(pkg, 100, 64), 7), "multiple")                    # A->nrows % m != 0
    refused(pkg, ech(pkg, stack(pkg, 100, 64, data=None), 10), "data is null")
    refused(pkg, ech(pkg, stack(pkg, 100, 130, ld=2), 10), "ld is smaller")        # ld < ceil(ncols / 64)
    refused(pkg, ech(pkg, stack(pkg, 100, 64), -10), "limits")                     # negative m
    refused(pkg, ech(pkg, stack(pkg, 100, 64), 0), "limits")
    refused(pkg, ech(pkg, stack(pkg, 100, 64), 10, limit=-1), "ncols_limit is negative")
    refused(pkg, ech(pkg, stack(pkg, 513 * 2, 64), 513), "limits", "513")          # larger shapes: gf2_echelonize_dev
    refused(pkg, ech(pkg, stack(pkg, 100, 1025), 10), "limits", "1025")
    refused(pkg, ech(pkg, stack(pkg, 100, 0), 10), "limits")
    refused(pkg, ech(pkg, stack(pkg, -10, 64), 10), "negative")
    refused(pkg, ech(pkg, stack(pkg, 100, 130, data=ALIGNED + 4), 10), "8-byte")


def test_inverse_batch_argument_errors(pkg):
    A = stack(pkg, 100, 10)
    far = ALIGNED + (1 << 16)
    refused(pkg, inv(pkg, None, A, 10), "gf2_inverse_batch_dev", "Ainv is null")
    refused(pkg, inv(pkg, stack(pkg, 100, 10, data=far), None, 10), "A is null")
    refused(pkg, inv(pkg, stack(pkg, 90, 10, data=far), A, 10), "shape")           # an Ainv of another shape
    refused(pkg, inv(pkg, stack(pkg, 100, 11, data=far), A, 10), "shape")
    refused(pkg, inv(pkg, stack(pkg, 100, 10, data=far), stack(pkg, 100, 12), 10), "n x n")
    refused(pkg, inv(pkg, stack(pkg, 100, 10, data=far), A, 7), "multiple")
    refused(pkg, inv(pkg, stack(pkg, 100, 10, data=far), A, -10), "limits")
    refused(pkg, inv(pkg, stack(pkg, 100, 10, data=None), A, 10), "Ainv.data is null")
    refused(pkg, inv(pkg, stack(pkg, 100, 10, data=far), stack(pkg, 100, 10, data=None), 10), "A.data is null")
    refused(pkg, inv(pkg, stack(pkg, 100, 10, data=far, ld=0), A, 10), "ld is smaller")
    refused(pkg, inv(pkg, stack(pkg, 1026, 513, data=far), stack(pkg, 1026, 513), 513), "limits")   # n <= 512
    # address ranges that meet: the same stack, a stack that starts inside A, and two views that interleave in one parent
    refused(pkg, inv(pkg, A, A, 10), "overlap")
    refused(pkg, inv(pkg, stack(pkg, 100, 10, data=ALIGNED + 16 * 50), A, 10), "overlap")
    refused(pkg, inv(pkg, stack(pkg, 100, 10, ld=4, data=ALIGNED + 16), stack(pkg, 100, 10, ld=4), 10), "overlap")
    refused(pkg, inv(pkg, stack(pkg, 100, 10, data=ALIGNED - 16 * 99), A, 10), "overlap")   # its last row is A's first


def test_an_empty_stack_is_no_error_and_needs_no_device(pkg):
    assert ech(pkg, stack(pkg, 0, 64, data=None), 10) == 0
    assert inv(pkg, stack(pkg, 0, 10, data=None), stack(pkg, 0, 10, data=None), 10) == 0


def test_a_good_call_without_a_device_says_so(pkg):
    """with a device this call would run, so it is made only where there is none: the refusal then comes from the device check, which
    is the last one"""
    if pkg._lib.lib().gf2_device_count() > 0:
        return
    refused(pkg, ech(pkg, stack(pkg, 100, 64), 10), "no usable HIP device")
    refused(pkg, inv(pkg, stack(pkg, 100, 10, data=ALIGNED + (1 << 16)), stack(pkg, 100, 10), 10), "no usable HIP device")
