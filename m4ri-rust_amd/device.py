"""Device-resident matrices over the C ABI (include/m4ri_hip.h, section 2).

`DMat` owns (or wraps) a dense bit matrix in HBM: row-major 64-bit words, LSB-first, `ld` words
per row.  Used by bench.py, the multi-GPU layer and tests that must not pay PCIe per product.

Output arrays
-------------
The wrappers of the companion headers (include/m4ri_hip_*.h) write int arrays next to their matrices.  Every such argument is
  * a raw device address (e.g. a torch int32 / int64 tensor's data_ptr()): the kernels write there, None is returned in its place;
  * SKIP (0), where the wrapper's docstring allows it: the array is not wanted, the C call gets NULL, None is returned in its place;
  * None (the default): the wrapper allocates the array itself.
What None returns depends on the wrapper, and its docstring says which kind it is:
  * a wrapper that WAITS for `stream` returns the values: a numpy int32 array, or an int / a bool for a single value.  Such a
    wrapper only enqueues on `stream` when none of its arrays is None;
  * a wrapper that only enqueues returns the array as an object with .ptr (its device address, which feeds the next wrapper as it
    is), .read(stream) (numpy; waits for `stream`), .count (the int32s it holds) and .mat (the DMat behind it).  An array of no
    element is None, except where the docstring says that the object is always there.
An input array (`idx`, `weights`, `ranks`, ...) is a raw device address or a list / numpy int array that the wrapper uploads.

Count first: where a wrapper stores one row of D per pair or hit, the capacity is D.nrows, else `cap`, and `count` / `hits` say how
many there are in all, which may be more; the call then only enqueues.  With neither D nor cap a count-only call comes first, the
wrapper WAITS for it and sizes D to exactly that many rows (ValueError for 2^31 rows or more, and for a raw `count` / `hits` address,
which the wrapper cannot read).  store=False: the rows are not stored -- D is passed without data, None is returned in its place and
only the arrays are written (the index-only mode); it takes no D.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import ALGO_AUTO, ALGO_M4RM, ALGO_NAIVE, ALGO_STRASSEN, DMatStruct  # noqa: F401
from .friendly import BinMatrix

ALGOS = {"auto": ALGO_AUTO, "m4rm": ALGO_M4RM, "strassen": ALGO_STRASSEN, "naive": ALGO_NAIVE}


def device_count():
    return _lib.lib().gf2_device_count()


def require_gpu():
    if device_count() <= 0:
        raise _lib.HipError("no usable HIP device: the multiply path has no CPU fallback")


class DMat:
    def __init__(self, nrows, ncols, _wrap=None):
        self.s = DMatStruct()
        self._owned = _wrap is None
        self._keep = None
        self._streams = set()  # streams this matrix has been used on (the device API is asynchronous)
        if _wrap is None:
            _lib.check(_lib.lib().gf2_dmat_alloc(ctypes.byref(self.s), nrows, ncols), "gf2_dmat_alloc")
        else:
            ptr, ld, keep = _wrap
            self.s.data, self.s.ld, self.s.nrows, self.s.ncols = ptr, ld, nrows, ncols
            self._keep = keep

    def __del__(self):
        if getattr(self, "_owned", False) and self.s.data:
            try:
                if len(self._streams) == 1:  # stream-ordered: recycled once that stream has passed this point
                    _lib.lib().gf2_dmat_free_async(ctypes.byref(self.s), next(iter(self._streams)))
                else:  # never used, or used on several streams: hipFree semantics (waits for the device)
                    _lib.lib().gf2_dmat_free(ctypes.byref(self.s))
            except Exception:  # interpreter shutdown: module globals may already be gone
                pass

    def _on(self, stream):
        self._streams.add(stream)
        return ctypes.byref(self.s)

    nrows = property(lambda self: self.s.nrows)
    ncols = property(lambda self: self.s.ncols)
    ld = property(lambda self: self.s.ld)

    @staticmethod
    def wrap(ptr, nrows, ncols, ld, keep=None):
        """Wrap caller-owned device memory (e.g. a torch int64 tensor's data_ptr())."""
        return DMat(nrows, ncols, _wrap=(ptr, ld, keep))

    @staticmethod
    def from_torch(t, ncols):
        """Wrap a 2-D contiguous torch.int64 CUDA tensor of shape (nrows, ld)."""
        assert t.dim() == 2 and t.is_contiguous() and t.element_size() == 8 and t.is_cuda
        assert t.shape[1] * 64 >= ncols
        return DMat.wrap(t.data_ptr(), t.shape[0], ncols, t.shape[1], keep=t)

    @staticmethod
    def random(nrows, ncols, seed, stream=None):
        m = DMat(nrows, ncols)
        m.fill_random(seed, stream)
        return m

    def fill_random(self, seed, stream=None):
        _lib.check(_lib.lib().gf2_dmat_fill_random(self._on(stream), seed, stream), "gf2_dmat_fill_random")

    def bernoulli_(self, thr, seed, accumulate=False, stream=None):
        """In place: every bit (accumulate: ^)= 1 with probability thr / 2^32 (include/m4ri_hip_draw.h) -> self."""
        return bernoulli(self, thr, seed, accumulate=accumulate, stream=stream)

    @staticmethod
    def from_host(bm, stream=None):
        m = DMat(bm.nrows(), bm.ncols())
        _lib.check(_lib.lib().gf2_dmat_upload(m._on(stream), bm.mzd, stream), "gf2_dmat_upload")
        return m

    @staticmethod
    def from_words(arr, ncols, stream=None):
        return DMat.from_host(BinMatrix.from_words(arr, ncols), stream)

    def to_host(self, stream=None):
        bm = BinMatrix.zero(self.nrows, self.ncols)
        _lib.check(_lib.lib().gf2_dmat_download(bm.mzd, self._on(stream), stream), "gf2_dmat_download")
        return bm

    def to_words(self, stream=None):
        return self.to_host(stream).to_words()

    # -- the friendly layer's operators on device-resident operands: same meaning as on
    #    BinMatrix (binary_matrix.rs:434-526), no PCIe traffic; everything runs on the default stream --
    def __mul__(self, other):
        return mul(self, other)

    def __add__(self, other):
        return add(self, other)

    def __eq__(self, other):
        return isinstance(other, DMat) and equal(self, other)

    __hash__ = None

    def transposed(self):
        return transpose(self)

    def clone(self, stream=None):
        zero = add(self, self, stream=stream)  # self ^ self; freed stream-ordered behind the second add
        return add(self, zero, stream=stream)

    def rank(self):
        return echelonize(self.clone(), full=False)[0]

    def kernel(self):
        """Null space basis K (self * K = 0) as a new DMat, or None for full column rank; self is left unchanged."""
        return nullspace(self.clone())[0]

    def inverted(self):
        inv = inverse(self)
        if inv is None:
            raise _lib.HipError("matrix is singular")
        return inv

    # -- binary_matrix.rs: augmented / stacked / get_window / set_window, on the device --
    def augmented(self, other):
        """[self | other] as a new DMat."""
        return concat(self, other)

    def stacked(self, other):
        """[self ; other] as a new DMat."""
        return stack(self, other)

    def get_window(self, start_row, start_col, high_row, high_col):
        """Rows [start_row, high_row) x columns [start_col, high_col) as a new DMat."""
        return submatrix(self, start_row, start_col, high_row, high_col)

    def take_rows(self, idx):
        """The rows idx[0], idx[1], ... of self as a new DMat (numpy's self[idx]; -1: a zero row; duplicates allowed)."""
        return gather_rows(self, idx)[0]

    def take_cols(self, idx):
        """The columns idx[0], idx[1], ... of self as a new DMat (numpy's self[:, idx]; -1: a zero column; duplicates allowed)."""
        return gather_cols(self, idx)[0]

    # -- Hamming weights on the device (include/m4ri_hip_weight.h) --
    def row_weights(self):
        """The Hamming weight of every row as a numpy int32 array."""
        return row_weights(self)

    def col_weights(self):
        """The number of set bits of every column as a numpy int32 array."""
        return col_weights(self)

    def count_ones(self):
        """The number of set bits.  On a vector (one row or one column) this is the reference's BinVector / BinMatrix count_ones
        (binary_matrix.rs:172-189, binary_vector.rs:112); on a matrix it is the total over all rows, where the reference panics."""
        return count_ones(self)

    def lpn_errors(self, c0, k, label_col):
        """For every secret s < 2^k the number of rows whose bits [c0, c0 + k) disagree with bit label_col under s (numpy int32[2^k]):
        tally, Walsh-Hadamard transform, (N - F) / 2 on the device (include/m4ri_hip_wht.h)."""
        return lpn_errors(self, c0, k, label_col)

    def lf1_reduce(self, c0, b, keep_zero=False):
        """One LF1 round of a BKW reduction as a new DMat of exactly the surviving rows: every row but the first of its class (classes
        by the bits [c0, c0 + b)), XORed with that first row, in the order they had (include/m4ri_hip_bkw.h).  keep_zero: the rows
        whose window is zero already all stay, unchanged."""
        return lf1_reduce(self, c0, b, keep_zero=keep_zero, src=SKIP)[0]

    def lf2_reduce(self, c0, b):
        """One LF2 round of a BKW reduction as a new DMat of exactly `count` rows: the XOR of every pair of rows inside a class
        (classes by the bits [c0, c0 + b)), classes by ascending key, the pairs of a class by (higher row, lower row)
        (include/m4ri_hip_lf2.h)."""
        return lf2_reduce(self, c0, b, lo=SKIP, hi=SKIP)[0]

    def join(self, other, c0, b, wcols=None):
        """The join with another pool as a new DMat of exactly `count` rows: the XOR of every pair of a row of self and a row of
        `other` whose bits [c0, c0 + b) are equal, classes by ascending key, the pairs of a class by (row of self, row of other)
        (include/m4ri_hip_join.h).  With wcols = (wc0, wc1) -> (D, wt): wt the ones of every row of D in those columns, on the
        device (.ptr feeds select_weights, .read(stream) gives numpy)."""
        out = join(self, other, c0, b, ia=SKIP, ib=SKIP, wt=SKIP if wcols is None else None, wcols=wcols)
        return out[0] if wcols is None else (out[0], out[4])

    def join_select(self, other, c0, b, wcols, wlo, whi):
        """The hits of the join with another pool as a new DMat of exactly `hits` rows: of the pairs of join(), in its order, those
        whose XOR has between wlo and whi ones in the columns wcols = (wc0, wc1) (include/m4ri_hip_join_select.h) -> (D, ia, ib, wt):
        the rows of self and of `other` and the weight of every hit, on the device (.ptr, .read(stream))."""
        out = join_select(self, other, c0, b, wcols, wlo, whi)
        return (out[0],) + out[3:]

    def near_pairs(self, other, wcols, wlo, whi, flags=0):
        """The pairs of a row of self and a row of `other` whose XOR has between wlo and whi ones in the columns wcols = (wc0, wc1)
        (None: all), as a new DMat of exactly `hits` rows ordered by (row of self, row of other) (include/m4ri_hip_near.h; flags:
        NEAR_OFF_DIAGONAL, NEAR_UPPER) -> (D, ia, ib, wt): the rows and the distance of every hit, on the device (.ptr, .read(stream))."""
        out = near_pairs(self, other, wcols, wlo, whi, flags=flags)
        return (out[0],) + out[2:]

    def nearest(self, other, wcols=None, flags=0):
        """For every row of self the lowest nearest row of `other` on the columns wcols and its distance (-1, -1 where `flags` admit
        none), as two numpy int32 arrays (include/m4ri_hip_near.h)."""
        idx, dist = nearest(self, other, wcols, flags=flags)
        return idx.read(None), dist.read(None)

    def sort_rows(self, c0=0, c1=None):
        """The rows of self sorted by their columns [c0, c1) (None: to the last column), ties in ascending row order, as the device
        array of the row at every sorted position (.ptr feeds gather_rows, .read(stream) gives numpy; include/m4ri_hip_unique.h)."""
        return sort_rows(self, c0, c1, head=SKIP)[0]

    def unique_rows(self, c0=0, c1=None):
        """The rows of self without those that repeat an earlier row on the columns [c0, c1) (None: to the last column), in the order
        they had, as a new DMat (include/m4ri_hip_unique.h).  The count of the kept rows is read back once, to size the result."""
        keep, count, _ = unique_rows(self, c0, c1, cap=self.nrows, rep=SKIP)
        n = int(count.read(None)[0])
        D = DMat(n, self.ncols)
        return gather_rows(self, keep.ptr, D=D)[0] if n else D

    def find_in(self, B, c0=0, c1=None):
        """For every row of self the lowest row of B that equals it on the columns [c0, c1) (None: to the last column of the narrower
        of the two), -1 where there is none, as a device array (.ptr feeds gather_rows, .read(stream) gives numpy;
        include/m4ri_hip_find.h)."""
        return find_rows(self, B, c0, c1, mult=SKIP, count=SKIP)[0]

    def _found_in(self, B, c0, c1, lo, hi):
        """the rows of self whose find_in(B) lies in [lo, hi] (the selection's compare is signed), in their order, as a new DMat"""
        idx = self.find_in(B, c0, c1)
        kptr, own_k = _out(None, self.nrows, always=True)
        n = select_weights(idx.ptr, self.nrows, lo, hi, idx=kptr, cap=self.nrows)[1]
        D = DMat(n, self.ncols)
        return gather_rows(self, kptr, D=D)[0] if n else D

    def difference(self, B, c0=0, c1=None):
        """The rows of self that equal no row of B on the columns [c0, c1) (None: as in find_in), in the order they had, as a new DMat
        (include/m4ri_hip_find.h).  The count of those rows is read back once, to size the result."""
        return self._found_in(B, c0, c1, -1, -1)

    def intersection(self, B, c0=0, c1=None):
        """The rows of self that equal a row of B on the columns [c0, c1) (None: as in find_in), in the order they had, as a new DMat
        (include/m4ri_hip_find.h).  The count of those rows is read back once, to size the result."""
        return self._found_in(B, c0, c1, 0, 2**31 - 1)

    def group_rows(self, c0=0, c1=None):
        """The rows of self grouped by their columns [c0, c1) (None: to the last column): the rows of a class together and ascending,
        the classes by their lowest row, as the device array of the row at every position (.ptr feeds gather_rows, .read(stream)
        gives numpy; include/m4ri_hip_join_rows.h)."""
        return group_rows(self, c0, c1, head=SKIP)[0]

    def join_rows(self, other, c0=0, c1=None, wcols=None):
        """The join with another pool on a column range of any width as a new DMat of exactly `count` rows: the XOR of every pair of a
        row of self and a row of `other` that are equal on the columns [c0, c1) (None: to the last column), ordered by (row of self,
        row of other) (include/m4ri_hip_join_rows.h).  With wcols = (wc0, wc1) -> (D, wt): wt the ones of every row of D in those
        columns, on the device (.ptr feeds select_weights, .read(stream) gives numpy)."""
        out = join_rows(self, other, c0, c1, ia=SKIP, ib=SKIP, wt=SKIP if wcols is None else None, wcols=wcols)
        return out[0] if wcols is None else (out[0], out[4])

    def subset_sums(self, p, base=None):
        """All C(nrows, p) XORs of p rows of self (each ^ base, a 1-row DMat, if given) as a new DMat, in the colexicographic order of
        the subsets: row C(c_1, 1) + ... + C(c_p, p) is the sum of the rows c_1 < ... < c_p (include/m4ri_hip_sums.h)."""
        return subset_sums(self, p, base=base, idx=SKIP, wt=SKIP)[0]

    def cover_reduce(self, c0, segments):
        """The covering-code reduction as a new DMat: the columns from c0 on are cut into blocks as long as the codes of `segments` (a
        list of CoverCode), every block is decoded to its nearest codeword and replaced by the message (include/m4ri_hip_cover.h)."""
        return cover_reduce(self, c0, segments, dist=SKIP)[0]

    def set_window(self, start_row, start_col, other):
        """Overwrite the block of other's shape at (start_row, start_col) with other."""
        copy_block(self, start_row, start_col, other, 0, 0, other.nrows, other.ncols)


def mul(A, B, C=None, accumulate=False, algo="auto", param=0, stream=None):
    """C (+)= A*B on the device; asynchronous on `stream` (int hipStream_t or None).
    Aliasing: A and B are only read -- mul(A, A) squares, and the two may overlap; C may share no word with A or B, with or without
    `accumulate` (HipError, "overlap").  C, A and B may be three disjoint column ranges of one parent."""
    if C is None:
        C = DMat(A.nrows, B.ncols)
    rc = _lib.lib().gf2_mul_dev(C._on(stream), A._on(stream), B._on(stream), int(accumulate), ALGOS[algo], param, stream)
    _lib.check(rc, "gf2_mul_dev")
    return C


def mul_nt(A, Bt, C=None, accumulate=False, stream=None):
    """C (+)= A * Bt^T.  Aliasing as mul(): mul_nt(A, A) is the Gram matrix A A^T; C may share no word with A or Bt."""
    if C is None:
        C = DMat(A.nrows, Bt.nrows)
    _lib.check(_lib.lib().gf2_mul_nt_dev(C._on(stream), A._on(stream), Bt._on(stream), int(accumulate), stream), "gf2_mul_nt_dev")
    return C


def add(A, B, C=None, stream=None):
    """C = A xor B.  Aliasing: C may be A, B or both -- add(A, B, C=A) is A += B in place (mzd_add(A, A, B)) -- and A may be B (zero); a C
    that overlaps an operand in any other way (another row, word or ld of the same buffer) raises HipError ("overlap")."""
    if C is None:
        C = DMat(A.nrows, A.ncols)
    _lib.check(_lib.lib().gf2_add_dev(C._on(stream), A._on(stream), B._on(stream), stream), "gf2_add_dev")
    return C


def transpose(S, D=None, stream=None):
    """D = S^T.  Aliasing: D may share no word with S (no in-place transposition, not for a square matrix either: HipError, "overlap");
    D and S may be disjoint column ranges of one parent."""
    if D is None:
        D = DMat(S.ncols, S.nrows)
    _lib.check(_lib.lib().gf2_transpose_dev(D._on(stream), S._on(stream), stream), "gf2_transpose_dev")
    return D


def copy_block(D, dr, dc, S, sr, sc, nrows, ncols, accumulate=False, stream=None):
    """D[dr+i][dc+j] (^)= S[sr+i][sc+j] for i < nrows, j < ncols, at any bit offsets; only those bits of D change.  S and D may share
    a buffer when the rectangles do not overlap.  Asynchronous on `stream`."""
    _lib.check(_lib.lib().gf2_copy_block_dev(D._on(stream), dr, dc, S._on(stream), sr, sc, nrows, ncols, int(bool(accumulate)),
                                             stream), "gf2_copy_block_dev")
    return D


def submatrix(S, lowr, lowc, highr, highc, D=None, stream=None):
    """D = S[lowr:highr, lowc:highc] (mzd_submatrix)."""
    if D is None:
        D = DMat(highr - lowr, highc - lowc)
    _lib.check(_lib.lib().gf2_submatrix_dev(D._on(stream), S._on(stream), lowr, lowc, highr, highc, stream), "gf2_submatrix_dev")
    return D


def concat(A, B, C=None, stream=None):
    """C = [A | B] (mzd_concat)."""
    if C is None:
        C = DMat(A.nrows, A.ncols + B.ncols)
    _lib.check(_lib.lib().gf2_concat_dev(C._on(stream), A._on(stream), B._on(stream), stream), "gf2_concat_dev")
    return C


def stack(A, B, C=None, stream=None):
    """C = [A ; B] (mzd_stack)."""
    if C is None:
        C = DMat(A.nrows + B.nrows, A.ncols)
    _lib.check(_lib.lib().gf2_stack_dev(C._on(stream), A._on(stream), B._on(stream), stream), "gf2_stack_dev")
    return C


def equal(A, B, stream=None):
    out = ctypes.c_int(0)
    _lib.check(_lib.lib().gf2_equal_dev(A._on(stream), B._on(stream), ctypes.byref(out), stream), "gf2_equal_dev")
    return bool(out.value)


def echelonize(A, full=True, ncols_limit=0, stream=None):
    """In-place (reduced) row echelon form of the first ncols_limit columns (0 = all) -> (rank, pivot columns)."""
    rank = ctypes.c_int(0)
    cap = min(A.nrows, ncols_limit if 0 < ncols_limit < A.ncols else A.ncols)
    piv = (ctypes.c_int * max(cap, 1))()
    _lib.check(_lib.lib().gf2_echelonize_dev(A._on(stream), int(bool(full)), int(ncols_limit), ctypes.byref(rank), piv,
                                             stream), "gf2_echelonize_dev")
    return rank.value, list(piv[:rank.value])


def inverse(A, stream=None):
    """A^-1 as a new DMat, or None if A is singular.  (The C entry gf2_inverse_dev also inverts in place: its Ainv may be A, or overlap
    it in any way, because A is copied into scratch before Ainv is written.)"""
    out = DMat(A.nrows, A.ncols)
    singular = ctypes.c_int(0)
    _lib.check(_lib.lib().gf2_inverse_dev(out._on(stream), A._on(stream), ctypes.byref(singular), stream),
               "gf2_inverse_dev")
    return None if singular.value else out


SKIP = 0  # for an output array that accepts it: do not compute it (the C call gets NULL)


# ---- the one copy of the rules of "Output arrays" (module docstring) ----------------------------------------------------------------

class _Ints:
    """Device ints that a wrapper owns, in a dense DMat of 128 int32 per row: `count` elements of `dtype` (int32 or int64), each a
    tuple of `width` of them if given (read() then has shape (count, width)); or, with `values`, host ints uploaded on `stream` (at
    least one row).  `least`: room for that many int32 even where count is smaller.  .count is in int32s."""

    def __init__(self, count=0, dtype=np.int32, width=None, values=None, least=0, stream=None):
        self.dtype, self.width = dtype, width
        if values is None:
            self.count = count * (width or 1) * (np.dtype(dtype).itemsize // 4)
            self.mat = DMat((max(self.count, least) + 127) // 128, 4096)
        else:
            v = np.ascontiguousarray(np.asarray(values).reshape(-1), dtype=np.int32)
            self.count = len(v)
            rows = max((self.count + 127) // 128, 1)
            full = np.zeros(rows * 128, dtype=np.int32)
            full[:self.count] = v
            self.mat = DMat.from_words(full.view(np.uint64).reshape(rows, 64), 4096, stream)

    @property
    def ptr(self):
        return self.mat.s.data

    def read(self, stream):
        """the values as a numpy array; waits for `stream`"""
        self.mat._streams.add(stream)
        a = np.ascontiguousarray(self.mat.to_words(stream)).reshape(-1).view(np.int32)[:self.count].copy().view(self.dtype)
        return a if self.width is None else a.reshape(-1, self.width)


def _out(given, count, always=False, **kind):
    """An output argument -> (pointer for the C call, the array the wrapper owns or None).  `given`: None, a raw address or SKIP.
    An own array is allocated only for count > 0; always: in any case, with room for one int (an address even for no element)."""
    if given is not None:
        return given or None, None
    if count <= 0 and not always:
        return None, None
    own = _Ints(count, least=int(always), **kind)
    return own.ptr, own


def _outs(givens, count, always=False):
    """_out for several int32 arrays of one length -> (pointers, owned)"""
    pairs = [_out(given, count, always) for given in givens]
    return [p for p, _ in pairs], [own for _, own in pairs]


def _used(stream, *owned):
    """after a call that passed _lib.check: its own arrays are in use on `stream` (and are released in its order)"""
    for own in owned:
        if own:
            own.mat._streams.add(stream)


def _numpy(given, own, stream):
    """what a wrapper that WAITS returns for an output array: None in the place of the caller's own, else the values"""
    if given is not None:
        return None
    return own.read(stream) if own else np.zeros(0, dtype=np.int32)


def _one_array(name, call, given, count, stream, wait, always=False):
    """a wrapper with one int32 output array: call(pointer) -> rc"""
    ptr, own = _out(given, count, always)
    _lib.check(call(ptr), name)
    if wait:
        return _numpy(given, own, stream)
    _used(stream, own)
    return own


def _count_first(name, what, own, count_only, stream, fits=True):
    """The capacity of a D that is sized by a count-only call: count_only() makes it, `own` is the wrapper's array of the count of
    `what` ("pairs": the argument `count`; "hits": `hits`); WAITS for `stream`.  fits: a D of 2^31 rows or more is refused."""
    arg = "hits" if what == "hits" else "count"
    if own is None:
        raise ValueError("%s: a raw %s address needs D or cap (the wrapper cannot read the %s to size D)" % (name, arg, arg))
    count_only()
    cap = int(own.read(stream)[0])
    if fits and cap >= 1 << 31:
        raise ValueError("%s: %d %s do not fit a matrix; give D or cap" % (name, cap, what))
    return cap


def _unstored(nrows, ncols):
    """the D of store=False: rows without data"""
    return DMat.wrap(None, nrows, ncols, max((ncols + 63) // 64, 1))


def _bad_int(bad, stream):
    """the `bad` argument -> (pointer, the zeroed int the wrapper owns or None)"""
    if bad is not None:
        return bad or None, None
    own = _Ints(values=[0], stream=stream)
    return own.ptr, own


def _bad_result(own, stream):
    return bool(own.read(stream)[0]) if own else None


def _plan(fn, args, n, lead=True):
    """a plan query fn(*args, out[n]) -> a tuple of ints, the return value first if `lead`; None for a negative return value"""
    out = (ctypes.c_longlong * n)()
    v = fn(*args, out)
    if v < 0:
        return None
    return ((int(v),) if lead else ()) + tuple(int(x) for x in out)


def _wcols(ncols, wcols):
    return (0, ncols) if wcols is None else wcols


def elim_batch_plan(m, ncols, inverse=False):
    """Which kernel a batch of m x ncols matrices runs on (no device needed) -> (variant id, threads per workgroup, matrices per
    workgroup, LDS bytes per workgroup, words per row held), or None when the shape is outside the limits."""
    return _plan(_lib.lib().gf2_elim_batch_plan, (m, ncols, int(bool(inverse))), 4)


def echelonize_batch(A, m, full=True, ncols_limit=0, ranks=None, pivots=None, stream=None):
    """Every m-row matrix of the stack A (matrix b = rows [b*m, (b+1)*m)) is replaced by its echelon form, each as echelonize() would
    leave it.  -> (ranks, pivots): `ranks` batch int32, `pivots` batch * P int32, P = min(m, limit), padded with -1 (numpy: shape
    (batch, P)).  Either may be SKIP.  WAITS."""
    batch = A.nrows // m if m > 0 else 0
    limit = ncols_limit if 0 < ncols_limit < A.ncols else A.ncols
    P = max(min(m, limit), 0)
    rptr, own_r = _out(ranks, batch)
    pptr, own_p = _out(pivots, batch * P)
    _lib.check(_lib.lib().gf2_echelonize_batch_dev(A._on(stream), m, int(bool(full)), int(ncols_limit), rptr, pptr, stream),
               "gf2_echelonize_batch_dev")
    out_r, out_p = _numpy(ranks, own_r, stream), _numpy(pivots, own_p, stream)
    return out_r, out_p if out_p is None else out_p.reshape(batch, P)


def inverse_batch(A, n, Ainv=None, singular=None, stream=None):
    """Block b of Ainv = (block b of A)^-1 for the n x n blocks of the stack A; blocks without an inverse are flagged in `singular`
    and left as they were in Ainv (a fresh Ainv: undefined).  -> (Ainv, singular): `singular` batch int32, may be SKIP.  WAITS."""
    if Ainv is None:
        Ainv = DMat(A.nrows, A.ncols)
    batch = A.nrows // n if n > 0 else 0
    sptr, own = _out(singular, batch)
    _lib.check(_lib.lib().gf2_inverse_batch_dev(Ainv._on(stream), A._on(stream), n, sptr, stream), "gf2_inverse_batch_dev")
    return Ainv, _numpy(singular, own, stream)


def _device_ints(idx, count, what, stream):
    """idx as (address, owner): an int is a raw device address and only passed on; a list or numpy int array is uploaded"""
    if isinstance(idx, (int, np.integer)):
        return int(idx), None
    arr = np.asarray(idx)
    if arr.size != count:
        raise ValueError("%s: idx holds %d indices, D needs %d" % (what, arr.size, count))
    if count == 0:
        return None, None
    if arr.dtype.kind not in "iu" or arr.min() < -(1 << 31) or arr.max() >= (1 << 31):
        raise ValueError("%s: idx must hold int32 values" % what)
    up = _Ints(values=arr, stream=stream)
    return up.ptr, up


def _gather(name, D, S, ptr, accumulate, bad, stream):
    bptr, own = _bad_int(bad, stream)
    L = _lib.lib()
    if name == "gf2_gather_rows_dev":
        rc = L.gf2_gather_rows_dev(D._on(stream), S._on(stream), ptr, int(bool(accumulate)), bptr, stream)
    else:
        rc = L.gf2_gather_cols_dev(D._on(stream), S._on(stream), ptr, bptr, stream)
    _lib.check(rc, name)
    return D, _bad_result(own, stream)


def gather_rows(S, idx, D=None, accumulate=False, bad=SKIP, stream=None):
    """D[i] (^)= S[idx[i]] for every row i of D (default: a new len(idx) x S.ncols matrix) -> (D, bad).  An index of -1 gives a zero row
    (accumulate: leaves the row), any other value outside S's rows likewise and is reported in `bad`.  `idx`: D.nrows int32, an input
    array.  `bad`: one int32 that a caller who gives its address has zeroed; SKIP is the default; None: the wrapper zeroes an int of its
    own, WAITS and returns a bool.  Duplicates are fine; D may share no word with S (HipError, "overlap")."""
    if D is None:
        if isinstance(idx, (int, np.integer)):
            raise ValueError("gather_rows: a raw idx address needs D (its row count is the number of indices)")
        D = DMat(int(np.asarray(idx).size), S.ncols)
    ptr, keep = _device_ints(idx, D.nrows, "gather_rows", stream)
    return _gather("gf2_gather_rows_dev", D, S, ptr, accumulate, bad, stream)


def gather_cols(S, idx, D=None, bad=SKIP, stream=None):
    """D[r][j] = S[r][idx[j]] for every column j of D (default: a new S.nrows x len(idx) matrix) -> (D, bad); idx and bad as in
    gather_rows(), -1 gives a zero column.  gather_cols_plan() tells which kernel a shape runs on."""
    if D is None:
        if isinstance(idx, (int, np.integer)):
            raise ValueError("gather_cols: a raw idx address needs D (its column count is the number of indices)")
        D = DMat(S.nrows, int(np.asarray(idx).size))
    ptr, keep = _device_ints(idx, D.ncols, "gather_cols", stream)
    return _gather("gf2_gather_cols_dev", D, S, ptr, False, bad, stream)


def gather_cols_plan(nrows, s_ncols, d_ncols):
    """Which path a column gather of this shape takes (no device needed) -> (path, threads per workgroup, LDS bytes per workgroup, rows
    per workgroup, scratch bytes) with path 0 = the fused LDS kernel, 1 = transpose / row gather / transpose; None for a bad shape."""
    return _plan(_lib.lib().gf2_gather_cols_plan, (nrows, s_ncols, d_ncols), 4)


_WEIGHT_WHAT = {"rows": 0, "cols": 1, "columns": 1, "total": 2}


def weights_plan(what, nrows, ncols):
    """Which kernel the weights of an nrows x ncols matrix run on (no device needed); what: "rows", "cols" or "total" (0, 1, 2)
    -> (variant id, threads per workgroup, rows per workgroup and pass, rows a lane takes before it empties its bit-sliced counters
    (columns; else 0), scratch bytes); None for a bad shape.  The variant ids are listed in include/m4ri_hip_weight.h."""
    return _plan(_lib.lib().gf2_weights_plan, (_WEIGHT_WHAT.get(what, what), nrows, ncols), 4)


def row_weights(A, out=None, stream=None):
    """The Hamming weight of every row of A: `out`, A.nrows int32.  WAITS.  Only A's ncols bits count; the array is overwritten, the
    caller zeroes nothing."""
    L = _lib.lib()
    return _one_array("gf2_row_weights_dev", lambda p: L.gf2_row_weights_dev(A._on(stream), p, stream), out, A.nrows, stream, True)


def col_weights(A, out=None, stream=None):
    """The number of rows of A with bit j set, for every column j: `out`, A.ncols int32, as in row_weights().  weights_plan("cols", ...)
    tells how the rows are cut into bands."""
    L = _lib.lib()
    return _one_array("gf2_col_weights_dev", lambda p: L.gf2_col_weights_dev(A._on(stream), p, stream), out, A.ncols, stream, True)


def count_ones(A, stream=None):
    """The number of set bits of A as a Python int (nrows * ncols can pass 2^32); WAITS for `stream`."""
    own = _Ints(2)   # one uint64
    _lib.check(_lib.lib().gf2_count_ones_dev(A._on(stream), own.ptr, stream), "gf2_count_ones_dev")
    return int(own.read(stream).view(np.uint64)[0])


def select_weights(weights, n, lo, hi, idx=None, cap=None, count=None, stream=None):
    """The indices i < n with lo <= weights[i] <= hi, ascending -> (idx, count).  `weights`: n int32, an input array (what row_weights /
    col_weights wrote).  At most `cap` (default: n) indices are stored; `count` is how many there are in all and may exceed cap.
    `idx`: cap int32 (numpy: cut to min(count, cap) when the wrapper owns the count too); `count`: one int32 (an int).  WAITS.
    idx=SKIP is a count-only call.  The device array idx feeds gather_rows / gather_cols as it is."""
    if cap is None:
        cap = n
    if idx is not None and idx == SKIP:
        cap = 0
    wptr, keep = _device_ints(weights, n, "select_weights", stream)
    iptr, own_i = _out(idx, cap)
    cptr, own_c = _out(count, 1)
    _lib.check(_lib.lib().gf2_select_weights_dev(wptr, n, lo, hi, iptr, cap, cptr, stream), "gf2_select_weights_dev")
    out_c = int(own_c.read(stream)[0]) if own_c and (n > 0 or cap > 0) else (0 if own_c else None)
    out_i = _numpy(idx, own_i, stream)
    if out_i is not None and out_c is not None:
        out_i = out_i[:min(out_c, cap)]
    return out_i, out_c


def wht_plan(k):
    """How a Walsh-Hadamard transform of 2^k int32 runs (no device needed) -> (passes, first level of every pass + [k], threads per
    workgroup, LDS bytes, tally variant (0: histogram in LDS, 1: global atomics), scratch bytes of min_weight for n = 2^k); None for a
    k outside 0 .. 30.  Pass p covers the levels [first[p], first[p + 1])."""
    out = (ctypes.c_longlong * 12)()
    passes = _lib.lib().gf2_wht_plan(k, out)
    return None if passes < 0 else (passes, [int(out[p]) for p in range(passes)] + [k], out[8], out[9], out[10], out[11])


def lpn_tally(P, c0, k, label_col=-1, out=None, stream=None):
    """f[v] = (rows of P whose bits [c0, c0 + k) read v and whose bit label_col is 0) - (... is 1), v < 2^k; label_col = -1: the plain
    histogram.  `out`: 2^k int32.  WAITS."""
    L = _lib.lib()
    return _one_array("gf2_lpn_tally_dev", lambda p: L.gf2_lpn_tally_dev(P._on(stream), c0, k, label_col, p, stream), out, 1 << k, stream, True)


def wht(f, k, stream=None):
    """The Walsh-Hadamard transform of 2^k int32, modulo 2^32.  `f` is a raw device address (16-byte aligned when k >= 2): transformed in
    place, the call only enqueues on `stream` and None is returned; or a list / numpy int array that the wrapper uploads: it WAITS for
    `stream` and returns a numpy int32 array."""
    if isinstance(f, (int, np.integer)):
        _lib.check(_lib.lib().gf2_wht_dev(int(f), k, stream), "gf2_wht_dev")
        return None
    ptr, keep = _device_ints(f, 1 << k, "wht", stream)
    _lib.check(_lib.lib().gf2_wht_dev(ptr, k, stream), "gf2_wht_dev")
    return keep.read(stream)


def lpn_errors(P, c0, k, label_col, out=None, stream=None):
    """errors[s] = the rows i of P with <P[i][c0 .. c0 + k), s> != P[i][label_col], for every s < 2^k: what col_weights(P * [S ; 1])
    gives for S = all 2^k vectors.  `out` as in lpn_tally() (16-byte aligned when k >= 2); the array feeds select_weights / min_weight
    as it is."""
    L = _lib.lib()
    return _one_array("gf2_lpn_errors_dev", lambda p: L.gf2_lpn_errors_dev(P._on(stream), c0, k, label_col, p, stream), out, 1 << k, stream, True)


def min_weight(w, n, idx=None, val=None, stream=None):
    """The smallest of w[0 .. n) and the LOWEST index that holds it -> (idx, val).  `w`: n int32, an input array.  `idx`, `val`: one
    int32 each (an int).  WAITS."""
    wptr, keep = _device_ints(w, n, "min_weight", stream)
    iptr, own_i = _out(idx, 1)
    vptr, own_v = _out(val, 1)
    _lib.check(_lib.lib().gf2_min_weight_dev(wptr, n, iptr, vptr, stream), "gf2_min_weight_dev")
    return (int(own_i.read(stream)[0]) if own_i else None), (int(own_v.read(stream)[0]) if own_v else None)


def lf1_plan(nrows, ncols, b):
    """How an LF1 round over nrows x ncols with a window of b bits runs (no device needed) -> (variant of the class-first kernel (0:
    table in LDS, 1: global atomics), its threads per workgroup, its LDS bytes, rows a workgroup of the count / scatter kernels covers,
    lanes per row of the scatter kernel, scratch bytes); None for a bad shape."""
    return _plan(_lib.lib().gf2_lf1_plan, (nrows, ncols, b), 5)


def class_first(P, c0, b, out=None, stream=None):
    """first[v] = the lowest row of P whose bits [c0, c0 + b) read v, -1 where no row does, v < 2^b.  `out`: 2^b int32.  WAITS."""
    L = _lib.lib()
    return _one_array("gf2_class_first_dev", lambda p: L.gf2_class_first_dev(P._on(stream), c0, b, p, stream), out, 1 << b, stream, True)


def lf1_reduce(P, c0, b, keep_zero=False, D=None, cap=None, first=None, count=None, src=None, stream=None):
    """One LF1 round of a BKW reduction (include/m4ri_hip_bkw.h): the rows of P are partitioned by their bits [c0, c0 + b), the first
    row of every class is XORed into the other rows of its class and dropped; with keep_zero the rows of key 0 stay as they are.
    -> (D, count, first, src): D holds the survivors in their order, `count` (one int32) says how many there are in all, first[v] is
    the first row of class v (2^b int32), src[j] the row of P that D[j] came from (D.nrows int32; may be SKIP).  Only enqueues; count
    first.  The arrays feed gather_rows / select_weights as they are."""
    L = _lib.lib()
    flags = _lib.LF1_KEEP_ZERO if keep_zero else 0
    fptr, own_f = _out(first, 1 << b)
    cptr, own_c = _out(count, 1)

    def call(Dm, sptr):
        _lib.check(L.gf2_lf1_reduce_dev(Dm._on(stream), P._on(stream), c0, b, flags, fptr, cptr, sptr, stream), "gf2_lf1_reduce_dev")

    if D is None:
        if cap is None:   # an int32 count always fits a matrix
            cap = _count_first("lf1_reduce", "rows", own_c, lambda: call(DMat.wrap(None, 0, P.ncols, P.ld), None), stream, fits=False)
        D = DMat(cap, P.ncols)
    sptr, own_s = _out(src, D.nrows)
    call(D, sptr)
    _used(stream, own_f, own_c, own_s)
    return D, own_c, own_f, own_s


def lf2_plan(nrows, ncols, b):
    """How the class sort and an LF2 round over nrows x ncols with a window of b bits run (no device needed) -> (sort passes, key bits
    per pass, threads per workgroup, LDS bytes of the sort kernels, rows per sort tile, rows per run of the pair kernels, lanes per
    row of the pair scatter, scratch bytes of class_sort, scratch bytes of lf2_reduce); None for a bad shape."""
    return _plan(_lib.lib().gf2_lf2_plan, (nrows, ncols, b), 8)


def class_sort(P, c0, b, order=None, skeys=None, stream=None):
    """The rows of P sorted by their bits [c0, c0 + b), ties in ascending row order (a stable sort; include/m4ri_hip_lf2.h)
    -> (order, skeys): order[s] the row at sorted position s, skeys[s] its key, P.nrows int32 each; skeys may be SKIP.  Only enqueues;
    the objects are always there (an address even where no row is sorted)."""
    optr, own_o = _out(order, P.nrows, always=True)
    kptr, own_k = _out(skeys, P.nrows, always=True)
    _lib.check(_lib.lib().gf2_class_sort_dev(P._on(stream), c0, b, optr, kptr, stream), "gf2_class_sort_dev")
    _used(stream, own_o, own_k)
    return own_o, own_k


def lf2_reduce(P, c0, b, D=None, cap=None, count=None, lo=None, hi=None, stream=None):
    """One LF2 round of a BKW reduction (include/m4ri_hip_lf2.h): the rows of P are partitioned by their bits [c0, c0 + b) and every
    pair of rows inside a class is XORed.  -> (D, count, lo, hi): D holds the pairs, classes by ascending key and the pairs of a class
    by (higher row, lower row); `count` (one int64) says how many there are in all; lo[j] < hi[j] are the rows of P that D[j] came
    from (D.nrows int32 each; may be SKIP; they feed gather_rows as they are).  Only enqueues; count first."""
    L = _lib.lib()
    cptr, own_c = _out(count, 1, dtype=np.int64)

    def call(Dm, lptr, hptr):
        _lib.check(L.gf2_lf2_reduce_dev(Dm._on(stream), P._on(stream), c0, b, cptr, lptr, hptr, stream), "gf2_lf2_reduce_dev")

    if D is None:
        if cap is None:
            cap = _count_first("lf2_reduce", "pairs", own_c, lambda: call(DMat.wrap(None, 0, P.ncols, P.ld), None, None), stream)
        D = DMat(cap, P.ncols)
    ptrs, owned = _outs((lo, hi), D.nrows)
    call(D, *ptrs)
    _used(stream, own_c, *owned)
    return (D, own_c) + tuple(owned)


def join_plan(nrows_a, nrows_b, ncols, b):
    """How the join of nrows_a x ncols with nrows_b x ncols on a window of b bits runs (no device needed) -> (passes of either sort,
    threads per workgroup, sorted positions of A per run R, lanes per row of the scatter, keys of B a workgroup stages in LDS at the
    most S, LDS bytes, scratch bytes, runs of A, the sorts' share of the scratch bytes); None for a bad shape."""
    return _plan(_lib.lib().gf2_join_plan, (nrows_a, nrows_b, ncols, b), 8)


def join(A, B, c0, b, D=None, cap=None, count=None, ia=None, ib=None, wt=None, wcols=None, stream=None):
    """The join of two pools on a window (include/m4ri_hip_join.h): every pair of a row of A and a row of B whose bits [c0, c0 + b)
    are equal is XORed.  -> (D, count, ia, ib, wt): D holds the pairs, classes by ascending key and the pairs of a class by (row of A,
    row of B); `count` (one int64) says how many there are in all; ia[t] and ib[t] are the rows of A and B that D[t] came from, wt[t]
    the ones of D[t] in the columns wcols = (wc0, wc1) (None: all columns) (D.nrows int32 each; may be SKIP; they feed gather_rows /
    select_weights as they are).  Only enqueues; count first.  A may be B: all ordered pairs of a class, (i, i) included."""
    L = _lib.lib()
    wc0, wc1 = _wcols(A.ncols, wcols)
    cptr, own_c = _out(count, 1, dtype=np.int64)

    def call(Dm, pa, pb, pw):
        rc = L.gf2_join_dev(Dm._on(stream), A._on(stream), B._on(stream), c0, b, cptr, pa, pb, pw, wc0, wc1, stream)
        _lib.check(rc, "gf2_join_dev")

    if D is None:
        if cap is None:
            cap = _count_first("join", "pairs", own_c, lambda: call(DMat.wrap(None, 0, A.ncols, A.ld), None, None, None), stream)
        D = DMat(cap, A.ncols)
    ptrs, owned = _outs((ia, ib, wt), D.nrows)
    call(D, *ptrs)
    _used(stream, own_c, *owned)
    return (D, own_c) + tuple(owned)


def join_select_plan(nrows_a, nrows_b, ncols, b, wcols=None):
    """How the weight-filtered join runs (include/m4ri_hip_join_select.h, no device needed) -> (passes of either sort, threads per
    workgroup, sorted positions of A per run R, lanes per pair of the weigh pass (by the words of the weight range wcols), lanes per
    row of the row store (by the row width), LDS bytes, scratch bytes, runs of A, outputs per round of the scatter G); None for a bad
    shape or range."""
    return _plan(_lib.lib().gf2_join_select_plan, (nrows_a, nrows_b, ncols, b) + tuple(_wcols(ncols, wcols)), 8)


def join_select(A, B, c0, b, wcols, wlo, whi, D=None, cap=None, store=True, count=None, hits=None, ia=None, ib=None, wt=None, stream=None):
    """The weight-filtered join (include/m4ri_hip_join_select.h): of the pairs of join(A, B, c0, b), in its order, only the HITS -- those
    whose XOR has between wlo and whi ones in the columns wcols = (wc0, wc1) (None: all columns) -- are written.  -> (D, count, hits,
    ia, ib, wt): D[h], ia[h], ib[h], wt[h] for the h-th hit (D.nrows int32 each; may be SKIP); `count` (one int64) the number of all
    pairs and `hits` (one int64) the number of all hits, which may exceed the capacity.  Only enqueues; count first, by `hits`;
    store=False."""
    L = _lib.lib()
    wc0, wc1 = _wcols(A.ncols, wcols)
    cptr, own_c = _out(count, 1, dtype=np.int64)
    hptr, own_h = _out(hits, 1, dtype=np.int64)

    def call(Dm, pa, pb, pw):
        rc = L.gf2_join_select_dev(Dm._on(stream), A._on(stream), B._on(stream), c0, b, wc0, wc1, wlo, whi, cptr, hptr, pa, pb, pw, stream)
        _lib.check(rc, "gf2_join_select_dev")

    if D is not None and not store:
        raise ValueError("join_select: store=False takes no D")
    if D is None:
        if cap is None:
            cap = _count_first("join_select", "hits", own_h, lambda: call(DMat.wrap(None, 0, A.ncols, A.ld), None, None, None), stream)
        D = DMat(cap, A.ncols) if store else _unstored(cap, A.ncols)
    ptrs, owned = _outs((ia, ib, wt), D.nrows)
    call(D, *ptrs)
    _used(stream, own_c, own_h, *owned)
    return (D if store else None, own_c, own_h) + tuple(owned)


NEAR_OFF_DIAGONAL = 1  # flags of near_pairs / nearest: pairs with ia == ib are not admitted (A is B: a row is not its own neighbour)
NEAR_UPPER = 2         # only pairs with ia < ib are admitted (A is B: every unordered pair once)


def near_plan(nrows_a, nrows_b, ncols, wcols=None):
    """How the Hamming-distance search runs (include/m4ri_hip_near.h, no device needed) -> (kernel: the words of the range wcols that
    it keeps in registers per row of A, 1, 2, 4, 8 or 16, and 0 for the wide kernel; threads per workgroup; rows of A per workgroup;
    the chunks S that B is cut into; rows of B per chunk; LDS bytes; scratch bytes; the words of a row that hold a column of the
    range); None for a bad shape or range."""
    return _plan(_lib.lib().gf2_near_plan, (nrows_a, nrows_b, ncols) + tuple(_wcols(ncols, wcols)), 8, lead=False)


def near_pairs(A, B, wcols, wlo, whi, flags=0, D=None, cap=None, store=True, hits=None, ia=None, ib=None, wt=None, stream=None):
    """The pairs of a row of A and a row of B that are close (include/m4ri_hip_near.h): of all pairs (ia, ib) that `flags` admits
    (NEAR_OFF_DIAGONAL: not ia == ib; NEAR_UPPER: only ia < ib), ordered by (ia, ib), only the HITS -- those whose XOR has between wlo
    and whi ones in the columns wcols = (wc0, wc1) (None: all columns) -- are written.  -> (D, hits, ia, ib, wt): D[h], ia[h], ib[h],
    wt[h] for the h-th hit (D.nrows int32 each; may be SKIP) and `hits` (one int64), the number of all hits, which may exceed the
    capacity.  Only enqueues; count first, by `hits`; store=False.  A may be B."""
    L = _lib.lib()
    wc0, wc1 = _wcols(A.ncols, wcols)
    hptr, own_h = _out(hits, 1, dtype=np.int64)

    def call(Dm, pa, pb, pw):
        rc = L.gf2_near_pairs_dev(Dm._on(stream), A._on(stream), B._on(stream), wc0, wc1, wlo, whi, flags, hptr, pa, pb, pw, stream)
        _lib.check(rc, "gf2_near_pairs_dev")

    if D is not None and not store:
        raise ValueError("near_pairs: store=False takes no D")
    if D is None:
        if cap is None:
            cap = _count_first("near_pairs", "hits", own_h, lambda: call(DMat.wrap(None, 0, A.ncols, A.ld), None, None, None), stream)
        D = DMat(cap, A.ncols) if store else _unstored(cap, A.ncols)
    ptrs, owned = _outs((ia, ib, wt), D.nrows)
    call(D, *ptrs)
    _used(stream, own_h, *owned)
    return (D if store else None, own_h) + tuple(owned)


def nearest(A, B, wcols=None, flags=0, idx=None, dist=None, stream=None):
    """For every row of A the nearest row of B on the columns wcols = (wc0, wc1) (None: all columns) among those that `flags` admits
    (include/m4ri_hip_near.h) -> (idx, dist): idx[i] the lowest such row, dist[i] its distance, both -1 where no row is admitted;
    A.nrows int32 each; either may be SKIP, not both.  Only enqueues; the objects are always there."""
    wc0, wc1 = _wcols(A.ncols, wcols)
    ptrs, owned = _outs((idx, dist), A.nrows, always=True)
    rc = _lib.lib().gf2_nearest_dev(A._on(stream), B._on(stream), wc0, wc1, flags, ptrs[0], ptrs[1], stream)
    _lib.check(rc, "gf2_nearest_dev")
    _used(stream, *owned)
    return tuple(owned)


def _crange(ncols, c0, c1):
    return c0, ncols if c1 is None else c1


def sort_rows_plan(nrows, ncols, c0=0, c1=None):
    """How the row sort on the columns [c0, c1) (c1 = None: to the last column) and the duplicate removal run
    (include/m4ri_hip_unique.h, no device needed) -> (radix passes, windows, bits per window, radix passes, launches of sort_rows
    without head, launches of unique_rows, scratch bytes of sort_rows, scratch bytes of unique_rows, rows per run of the head kernels);
    None for a bad shape or range."""
    return _plan(_lib.lib().gf2_sort_rows_plan, (nrows, ncols) + _crange(ncols, c0, c1), 8)


def sort_rows(P, c0=0, c1=None, order=None, head=None, stream=None):
    """The rows of P sorted by their columns [c0, c1) (c1 = None: to the last column; column c1 - 1 is the most significant bit), ties
    in ascending row order (a stable sort on a range of any width; include/m4ri_hip_unique.h) -> (order, head): order[s] the row at
    sorted position s, head[s] the first sorted position of the class of s, P.nrows int32 each; head may be SKIP.  Only enqueues; the
    objects are always there (an address even where no row is sorted).  gather_rows by `order` gives the canonical form of a list."""
    c0, c1 = _crange(P.ncols, c0, c1)
    ptrs, owned = _outs((order, head), P.nrows, always=True)
    _lib.check(_lib.lib().gf2_sort_rows_dev(P._on(stream), c0, c1, ptrs[0], ptrs[1], stream), "gf2_sort_rows_dev")
    _used(stream, *owned)
    return tuple(owned)


def unique_rows(P, c0=0, c1=None, keep=None, cap=None, count=None, rep=None, stream=None):
    """The first occurrence of every distinct value of the columns [c0, c1) of P's rows (c1 = None: to the last column;
    include/m4ri_hip_unique.h) -> (keep, count, rep): keep holds the kept rows, ascending (`cap` int32; it feeds gather_rows as it is);
    `count` (one int32) says how many there are in all, which may exceed cap; rep[i] is the lowest row equal to row i on the range
    (P.nrows int32; may be SKIP).  Only enqueues; count first, by `count`: with neither keep nor cap a count-only call (keep=SKIP,
    cap=0) comes first, the wrapper WAITS for it and sizes keep to exactly that many -- the rows are sorted twice; cap=P.nrows always
    suffices and sorts once.  A raw keep address needs cap."""
    L = _lib.lib()
    c0, c1 = _crange(P.ncols, c0, c1)
    cptr, own_c = _out(count, 1)

    def call(kptr, capacity, rptr):
        _lib.check(L.gf2_unique_rows_dev(P._on(stream), c0, c1, kptr, capacity, cptr, rptr, stream), "gf2_unique_rows_dev")

    if keep is not None and keep == SKIP:
        cap = 0
    if cap is None:
        if keep is not None:
            raise ValueError("unique_rows: a raw keep address needs cap (the number of int32 it holds)")
        cap = _count_first("unique_rows", "rows", own_c, lambda: call(None, 0, None), stream, fits=False)
    kptr, own_k = _out(keep, cap)
    rptr, own_r = _out(rep, P.nrows)
    call(kptr, cap, rptr)
    _used(stream, own_k, own_c, own_r)
    return own_k, own_c, own_r


def find_rows_plan(nrows_a, nrows_b, ncols, c0=0, c1=None):
    """How the lookup of nrows_a rows among nrows_b rows on the columns [c0, c1) (c1 = None: to the last column) runs
    (include/m4ri_hip_find.h, no device needed) -> (slots of the table, capped at 2^31 - 1, slots, bytes per slot, scratch bytes,
    launches, rows per workgroup of the build kernel, of the lookup kernel, the form (0: a lane per row, 1: a wave per row), words of a
    row in the range); None for a bad shape or range."""
    return _plan(_lib.lib().gf2_find_rows_plan, (nrows_a, nrows_b, ncols) + _crange(ncols, c0, c1), 8)


def find_rows(A, B, c0=0, c1=None, idx=None, mult=None, count=None, stream=None):
    """Every row of A looked up among the rows of B on the columns [c0, c1) (c1 = None: to the last column of the narrower of the two;
    include/m4ri_hip_find.h) -> (idx, mult, count): idx[i] the lowest row of B equal to row i of A, -1 for none; mult[i] how many rows
    of B are equal to it; A.nrows int32 each; `count` (one int32) the rows of A that were found.  mult and count may be SKIP.  A may
    be B: idx is then the rep of unique_rows and mult the class sizes.  Only enqueues; the objects are always there.  idx cannot be
    skipped (ValueError): with neither idx nor mult wanted there is nothing to look up."""
    if idx is not None and idx == SKIP:
        raise ValueError("find_rows: idx cannot be SKIP (mult and count can)")
    c0, c1 = _crange(min(A.ncols, B.ncols), c0, c1)
    ptrs, owned = _outs((idx, mult), A.nrows, always=True)
    cptr, own_c = _out(count, 1)
    _lib.check(_lib.lib().gf2_find_rows_dev(A._on(stream), B._on(stream), c0, c1, ptrs[0], ptrs[1], cptr, stream), "gf2_find_rows_dev")
    _used(stream, own_c, *owned)
    return owned[0], owned[1], own_c


def join_rows_plan(nrows_a, nrows_b, ncols, c0=0, c1=None):
    """How the grouping of nrows_b rows by class and the join of nrows_a with nrows_b rows on the columns [c0, c1) (c1 = None: to the
    last column) run (include/m4ri_hip_join_rows.h, no device needed) -> (radix passes of the grouping, slots of the table over B, the
    form of its kernels (0: a lane per row, 1: a wave per row), launches of group_rows without head, launches of join_rows with a
    capacity, rows of A per workgroup of the sum and offset kernels, outputs per workgroup of the scatter, scratch bytes of
    group_rows, scratch bytes of join_rows); None for a bad shape or range."""
    return _plan(_lib.lib().gf2_join_rows_plan, (nrows_a, nrows_b, ncols) + _crange(ncols, c0, c1), 8)


def group_rows(P, c0=0, c1=None, order=None, head=None, stream=None):
    """The rows of P grouped by their columns [c0, c1) (c1 = None: to the last column) without sorting by value
    (include/m4ri_hip_join_rows.h) -> (order, head): order[s] the rows ascending by (lowest equal row, row) -- the rows of a class
    together and ascending, the classes by their lowest row --, head[s] the first sorted position of the class of s, P.nrows int32
    each; head may be SKIP.  Only enqueues; the objects are always there (an address even where no row is grouped)."""
    c0, c1 = _crange(P.ncols, c0, c1)
    ptrs, owned = _outs((order, head), P.nrows, always=True)
    _lib.check(_lib.lib().gf2_group_rows_dev(P._on(stream), c0, c1, ptrs[0], ptrs[1], stream), "gf2_group_rows_dev")
    _used(stream, *owned)
    return tuple(owned)


def join_rows(A, B, c0=0, c1=None, D=None, cap=None, store=True, count=None, ia=None, ib=None, wt=None, wcols=None, stream=None):
    """The join of two pools on a column range of any width (include/m4ri_hip_join_rows.h): every pair of a row of A and a row of B
    that are equal on the columns [c0, c1) (c1 = None: to the last column) is XORed.  -> (D, count, ia, ib, wt): D holds the pairs
    ordered by (row of A, row of B); `count` (one int64) says how many there are in all, which may exceed the capacity; ia[t] and
    ib[t] are the rows of A and B that D[t] came from, wt[t] the ones of D[t] in the columns wcols = (wc0, wc1) (None: all columns)
    (D.nrows int32 each; may be SKIP; they feed gather_rows / select_weights as they are).  Only enqueues; count first, by `count`;
    store=False: the rows are not stored (D is None in the result).  A may be B: all ordered pairs of a class, (i, i) included."""
    L = _lib.lib()
    c0, c1 = _crange(A.ncols, c0, c1)
    wc0, wc1 = _wcols(A.ncols, wcols)
    cptr, own_c = _out(count, 1, dtype=np.int64)

    def call(Dm, pa, pb, pw):
        rc = L.gf2_join_rows_dev(Dm._on(stream), A._on(stream), B._on(stream), c0, c1, cptr, pa, pb, pw, wc0, wc1, stream)
        _lib.check(rc, "gf2_join_rows_dev")

    if D is not None and not store:
        raise ValueError("join_rows: store=False takes no D")
    if D is None:
        if cap is None:
            cap = _count_first("join_rows", "pairs", own_c, lambda: call(DMat.wrap(None, 0, A.ncols, A.ld), None, None, None), stream)
        D = DMat(cap, A.ncols) if store else _unstored(cap, A.ncols)
    ptrs, owned = _outs((ia, ib, wt), D.nrows)
    call(D, *ptrs)
    _used(stream, own_c, *owned)
    return (D if store else None, own_c) + tuple(owned)


def subset_count(n, p):
    """C(n, p), the number of subsets that subset_sums(S, p) of n rows enumerates (no device needed); 0 for n < p; None for a p outside
    1 .. 4 or a value past 2^62."""
    v = _lib.lib().gf2_subset_count(n, p)
    return None if v < 0 else int(v)


def subset_sums_plan(n, ncols, p, count):
    """How `count` sums of p of n rows of ncols columns run (include/m4ri_hip_sums.h, no device needed) -> (kernel id: 0 .. 3 S in LDS
    with 1, 2, 8, 64 lanes per row, 4 .. 7 S from global memory likewise; threads per workgroup; ranks per workgroup R; lanes per row;
    LDS bytes; workgroups; scratch bytes); None for a bad shape."""
    return _plan(_lib.lib().gf2_subset_sums_plan, (n, ncols, p, count), 6)


def subset_sums(S, p, base=None, rank0=0, count=None, D=None, idx=None, wt=None, wcols=None, store=True, stream=None):
    """All XORs of p rows of S in rank order (include/m4ri_hip_sums.h): D[t] = base ^ S[c_1] ^ ... ^ S[c_p] for the subset c_1 < ... <
    c_p of rank rank0 + t in the colexicographic order, rank = C(c_1, 1) + ... + C(c_p, p).  -> (D, idx, wt): idx[t] = (c_1 .. c_p)
    (count * p int32; read(): shape (count, p); feeds gather_rows), wt[t] the ones of D[t] in the columns wcols = (wc0, wc1) (None: all
    columns) (count int32; feeds select_weights); either may be SKIP.  base: None or a 1-row DMat (the syndrome).  The window is
    D.nrows rows, else `count`, else (count=None) everything from rank0 up to C(n, p); ValueError when that does not fit a matrix
    (2^31 - 1 rows): there is no count-only call.  store=False: only idx and wt are written (the weights of all candidates of
    Lee-Brickell).  Only enqueues."""
    total = subset_count(S.nrows, p)
    if total is None:
        raise ValueError("subset_sums: p = %d is outside 1 .. 4, or C(%d, %d) passes 2^62" % (p, S.nrows, p))
    if D is not None:
        if not store:
            raise ValueError("subset_sums: store=False takes no D")
        if count is not None and count != D.nrows:
            raise ValueError("subset_sums: count = %d, but D has %d rows" % (count, D.nrows))
        count = D.nrows
    if count is None:
        count = max(total - rank0, 0)
    if count >= 1 << 31:
        raise ValueError("subset_sums: %d sums do not fit a matrix; give count, D or rank0" % count)
    if D is None:
        D = DMat(count, S.ncols) if store else _unstored(count, S.ncols)
    wc0, wc1 = _wcols(S.ncols, wcols)
    iptr, own_i = _out(idx, count, width=p)
    wptr, own_w = _out(wt, count)
    rc = _lib.lib().gf2_subset_sums_dev(D._on(stream), S._on(stream), base._on(stream) if base is not None else None, p, rank0, iptr, wptr,
                                        wc0, wc1, stream)
    _lib.check(rc, "gf2_subset_sums_dev")
    _used(stream, own_i, own_w)
    return (D if store else None), own_i, own_w


def unrank_subsets(ranks, count, p, n, rank0=0, idx=None, bad=None, stream=None):
    """The subsets of the ranks rank0 + ranks[t], t < count, of the order of subset_sums over n rows -> (idx, bad): idx[t] = (c_1 ..
    c_p) (count * p int32; read(): shape (count, p)); a rank of -1 (what select_weights leaves behind its count) gives p times -1, any
    other rank outside [0, C(n, p)) as well and is reported in `bad`.  `ranks`: count int32, an input array (what select_weights wrote,
    or the ia / ib of a join gathered at the hits).  `bad` as in gather_rows(), but None is the default: only enqueues when `bad` is an
    address or SKIP."""
    rptr, keep = _device_ints(ranks, count, "unrank_subsets", stream)
    iptr, own_i = _out(idx, count, width=p)
    bptr, own_b = _bad_int(bad, stream)
    rc = _lib.lib().gf2_unrank_subsets_dev(rptr, count, rank0, p, n, iptr, bptr, stream)
    _lib.check(rc, "gf2_unrank_subsets_dev")
    _used(stream, own_i)
    return own_i, _bad_result(own_b, stream)


def draw_plan(what, count_or_k=0, n=1, thr=0):
    """How a draw runs (include/m4ri_hip_draw.h, no device needed); what: "bernoulli" -> (Philox calls per output word for thr, threads
    per workgroup, lanes of one pass of the grid, 0); "indices" (count, n) -> (Philox calls, threads, draws of one pass of the grid,
    0); "subsets" (k, n) -> (threads, LDS bytes, subsets per workgroup, the rounds of max_rounds=0); "permutation" (n) -> (scratch
    bytes, sort passes, key bits, 0); None for a bad shape."""
    code = {"bernoulli": _lib.DRAW_BERNOULLI, "indices": _lib.DRAW_INDICES, "subsets": _lib.DRAW_SUBSETS,
            "permutation": _lib.DRAW_PERMUTATION}.get(what, what)
    return _plan(_lib.lib().gf2_draw_plan, (code, count_or_k, n, thr), 4, lead=False)


def bernoulli(D, thr, seed, accumulate=False, row0=0, col_word0=0, full_ncols=0, stream=None):
    """Every bit of D (accumulate: ^)= 1 with probability thr / 2^32, by the Philox rule of include/m4ri_hip_draw.h -> D.  With row0,
    col_word0 (in 64-bit words) and full_ncols, D is that rectangle of the noise of a matrix of full_ncols columns.  Asynchronous on
    `stream`."""
    L = _lib.lib()
    if row0 or col_word0 or full_ncols:
        rc = L.gf2_bernoulli_block_dev(D._on(stream), thr, seed, row0, col_word0, full_ncols, int(bool(accumulate)), stream)
        _lib.check(rc, "gf2_bernoulli_block_dev")
    else:
        _lib.check(L.gf2_bernoulli_dev(D._on(stream), thr, seed, int(bool(accumulate)), stream), "gf2_bernoulli_dev")
    return D


def draw_indices(count, n, seed, out=None, stream=None):
    """`count` independent draws from [0, n) (include/m4ri_hip_draw.h): `out`, count int32; they feed gather_rows as the device array
    they are.  Only enqueues; the object is always there (an address even where nothing is drawn)."""
    L = _lib.lib()
    return _one_array("gf2_draw_indices_dev", lambda p: L.gf2_draw_indices_dev(p, count, n, seed, stream), out, count, stream, False, always=True)


def draw_subsets(batch, k, n, seed, max_rounds=0, out=None, unfinished=None, stream=None):
    """`batch` ordered k-tuples of distinct values from [0, n), one per guess of a pooled-Gauss round (include/m4ri_hip_draw.h)
    -> (sub, unfinished): `out` batch * k int32 (the object is always there), `unfinished` one int32, may be SKIP.  A position that has
    not settled after max_rounds rounds (0: 64) reads -1.  Only enqueues."""
    L = _lib.lib()
    uptr, own_u = _out(unfinished, 1)
    own_s = _one_array("gf2_draw_subsets_dev", lambda p: L.gf2_draw_subsets_dev(p, batch, k, n, seed, max_rounds, uptr, stream), out, batch * k,
                       stream, False, always=True)
    _used(stream, own_u)
    return own_s, own_u


def draw_permutation(n, seed, out=None, stream=None):
    """A permutation of 0 .. n - 1: the stable argsort of 30-bit Philox keys (include/m4ri_hip_draw.h); it feeds gather_cols and
    gather_rows as the device array it is.  `out` as in draw_indices()."""
    L = _lib.lib()
    return _one_array("gf2_draw_permutation_dev", lambda p: L.gf2_draw_permutation_dev(p, n, seed, stream), out, n, stream, False, always=True)


def lpn_samples(N, k, secret, thr, seed, stream=None):
    """N samples of an LPN oracle as an N x (k + 1) DMat [A | A s ^ e]: A is the uniform fill of `seed` (gf2_dmat_fill_random), e
    Bernoulli(thr / 2^32) noise of the same seed.  `secret` is a k x 1 DMat or k bits (uploaded).  A chain of existing entries --
    fill, mul, bernoulli(accumulate), concat -- that only enqueues on `stream` when the secret is on the device already."""
    if not isinstance(secret, DMat):
        bits = np.asarray(secret).reshape(-1)
        if len(bits) != k:
            raise ValueError("lpn_samples: the secret holds %d bits, k is %d" % (len(bits), k))
        secret = DMat.from_words((bits != 0).astype(np.uint64).reshape(k, 1), 1, stream)
    A = DMat(N, k)
    A.fill_random(seed, stream)
    y = mul(A, secret, stream=stream)
    bernoulli(y, thr, seed, accumulate=True, stream=stream)
    return concat(A, y, stream=stream)


class CoverCode:
    """A small [n, k] code in systematic form for cover_reduce() (include/m4ri_hip_cover.h): bit t of a block's syndrome is
    parity(block & h[t]), and h[t] >> k == 1 << t.  Made by identity(n), drop(n), repetition(n), hamming(r), golay23() or
    from_rows(n, k, h).  Codes compare equal when n, k, the check rows and the table are equal."""

    def __init__(self, n, k, h=(), table=None):
        self.s = _lib.CoverCodeStruct()
        self.s.n, self.s.k = n, k
        for t, row in enumerate(h):
            self.s.h[t] = row
        self._table = None if table is None else np.ascontiguousarray(table, dtype=np.uint32)
        self._leaders = self._radius = self._dev = None

    n = property(lambda self: self.s.n)
    k = property(lambda self: self.s.k)
    r = property(lambda self: self.s.n - self.s.k)
    h = property(lambda self: tuple(int(x) for x in self.s.h))
    has_table = property(lambda self: 0 < self.s.k < self.s.n)

    @staticmethod
    def _named(kind, param):
        code = CoverCode(0, 0)
        if _lib.lib().gf2_cover_code_named(kind, param, ctypes.byref(code.s)) != 0:
            raise ValueError("CoverCode: no code of kind %d with parameter %r" % (kind, param))
        return code

    @staticmethod
    def identity(n):
        """[n, n], 1 <= n <= 32: the bits pass through"""
        return CoverCode._named(_lib.COVER_IDENTITY, n)

    @staticmethod
    def drop(n):
        """[n, 0], 1 <= n <= 32: the bits are dropped (and counted in dist)"""
        return CoverCode._named(_lib.COVER_DROP, n)

    @staticmethod
    def repetition(n):
        """[n, 1], 2 <= n <= 13: the majority bit (a tie decodes to the pattern that is smaller as an integer)"""
        return CoverCode._named(_lib.COVER_REPETITION, n)

    @staticmethod
    def hamming(r):
        """[2^r - 1, 2^r - 1 - r], 2 <= r <= 5"""
        return CoverCode._named(_lib.COVER_HAMMING, r)

    @staticmethod
    def golay23():
        """the binary Golay code [23, 12], covering radius 3"""
        return CoverCode._named(_lib.COVER_GOLAY23, 0)

    @staticmethod
    def from_rows(n, k, h, table=None):
        """The code with the check rows h[0 .. n - k).  table: 2^(n-k) uint32 that the device reads INSTEAD of the coset leaders (the
        tables are taken as they are).  ValueError for a code outside the limits or a non-systematic h."""
        h = [int(x) for x in h]
        if len(h) > _lib.COVER_MAX_R or len(h) < (n - k if 0 < k < n else 0):
            raise ValueError("CoverCode.from_rows: [%d, %d] with %d check rows is outside the limits" % (n, k, len(h)))
        code = CoverCode(n, k, h, table)
        if _lib.lib().gf2_cover_plan(0, 0, ctypes.byref(code.s), 1, None, 0, None) < 0:
            raise ValueError("CoverCode.from_rows: [%d, %d] breaks the rules of include/m4ri_hip_cover.h" % (n, k))
        if table is not None and (not code.has_table or code._table.shape != (1 << (n - k),)):
            raise ValueError("CoverCode.from_rows: the table must hold 2^(n-k) words, and only a code with 1 <= k < n has one")
        return code

    def _key(self):
        return (self.n, self.k, self.h[:self.r] if self.has_table else (), None if self._table is None else self._table.tobytes())

    def __eq__(self, other):
        return isinstance(other, CoverCode) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "CoverCode[%d, %d]" % (self.n, self.k)

    def leaders(self):
        """The coset leaders as a numpy uint32 array: 2^r entries (none for k == 0), leaders[s] = the pattern of lowest weight with
        syndrome s, among equal weights the smallest integer (gf2_cover_leaders)."""
        if self._leaders is None:
            out = np.zeros(0 if self.k == 0 else 1 << self.r, dtype=np.uint32)
            radius = ctypes.c_int(0)
            if _lib.lib().gf2_cover_leaders(ctypes.byref(self.s), out.ctypes.data, ctypes.byref(radius)) != 0:
                raise ValueError("gf2_cover_leaders refused %r" % self)
            self._leaders, self._radius = out, radius.value
        return self._leaders

    @property
    def radius(self):
        """the largest weight of a coset leader: the covering radius (0 for identity and drop)"""
        self.leaders()
        return self._radius

    def table_ptr(self):
        """Device address of the table that cover_reduce() reads for this code (the coset leaders unless from_rows() was given a
        table), None for a code without one.  The copy is made once, WAITS for the upload, and is kept with the code."""
        if not self.has_table:
            return None
        if self._dev is None:
            self._dev = _Ints(values=(self.leaders() if self._table is None else self._table).view(np.int32))
        return self._dev.ptr


def _cover_args(segments):
    """segments (a list of CoverCode) -> (codes, array of gf2_cover_code, seg_code bytes), the codes deduplicated"""
    codes, index, seg = [], {}, []
    for code in segments:
        if code not in index:
            index[code] = len(codes)
            codes.append(code)
        seg.append(index[code])
    if len(codes) > _lib.COVER_MAX_CODES or len(seg) > _lib.COVER_MAX_SEGS:
        raise ValueError("cover: %d distinct codes in %d segments: at most %d in %d" % (len(codes), len(seg), _lib.COVER_MAX_CODES,
                                                                                         _lib.COVER_MAX_SEGS))
    arr = (_lib.CoverCodeStruct * max(len(codes), 1))()
    for i, code in enumerate(codes):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(code.s), ctypes.sizeof(_lib.CoverCodeStruct))
    return codes, arr, (ctypes.c_ubyte * max(len(seg), 1))(*seg)


def cover_plan(nrows, p_ncols, segments):
    """How a covering-code reduction of nrows x p_ncols by `segments` (a list of CoverCode) runs (no device needed) -> (variant (0: rows
    read from global memory, 1: window words staged in LDS), threads per workgroup, LDS bytes, rows per workgroup and pass, lanes per
    row of the copy, K, bits of the window, table words, workgroups); None for a bad argument."""
    try:
        codes, arr, seg = _cover_args(segments)
    except ValueError:
        return None
    return _plan(_lib.lib().gf2_cover_plan, (nrows, p_ncols, arr, len(codes), seg, len(segments)), 8)


def cover_reduce(P, c0, segments, D=None, dist=None, stream=None):
    """The covering-code reduction (include/m4ri_hip_cover.h): the columns of P from c0 on are cut into blocks, block j as long as
    segments[j] (a CoverCode), every block is decoded to the nearest codeword and replaced by its message -> (D, dist): D (default: a
    new P.nrows x K matrix, K = the sum of the codes' k) holds the messages side by side, dist[i] the number of bits of row i that the
    decoding flipped or dropped (P.nrows int32; may be SKIP).  Only enqueues, except that a code's table is uploaded (and waited for)
    the first time the code is used: table_ptr() does that ahead of a chain."""
    codes, arr, seg = _cover_args(segments)
    tables = (ctypes.c_void_p * max(len(codes), 1))(*[code.table_ptr() for code in codes])
    if D is None:
        D = DMat(P.nrows, sum(code.k for code in segments))
    L = _lib.lib()
    return D, _one_array("gf2_cover_reduce_dev", lambda p: L.gf2_cover_reduce_dev(D._on(stream), P._on(stream), c0, arr, len(codes), seg,
                                                                                   len(segments), tables, p, stream), dist, P.nrows, stream, False)


def nullspace(A, stream=None):
    """A is reduced in place to its reduced row echelon form -> (K or None, rank, pivot columns): K is n x (n - rank) with A K = 0,
    its rows at the free columns the identity (ascending free columns); None when the rank is n.  Synchronous on `stream`."""
    rank = ctypes.c_int(0)
    piv = (ctypes.c_int * max(min(A.nrows, A.ncols), 1))()
    ks = DMatStruct()
    _lib.check(_lib.lib().gf2_nullspace_dev(A._on(stream), ctypes.byref(ks), ctypes.byref(rank), piv, stream), "gf2_nullspace_dev")
    K = None
    if ks.data:
        K = DMat.wrap(ks.data, ks.nrows, ks.ncols, ks.ld)
        K._owned = True  # allocated by the library for the caller: released like a matrix of DMat's own
        K._streams.add(stream)
    return K, rank.value, list(piv[:rank.value])


def prof_enable(on):
    _lib.lib().gf2_prof_enable(int(on))


def prof_read(reset=True):
    n, ms = ctypes.c_int(0), ctypes.c_double(0)
    _lib.check(_lib.lib().gf2_prof_read(ctypes.byref(n), ctypes.byref(ms), int(reset)), "gf2_prof_read")
    return n.value, ms.value


def ple(A, pluq=False, stream=None):
    """In-place PLE (pluq=False) or PLUQ decomposition (layout of mzd_ple / mzd_pluq) -> (rank, P list, Q list)."""
    P = (ctypes.c_int * max(A.nrows, 1))()
    Q = (ctypes.c_int * max(A.ncols, 1))()
    rank = ctypes.c_int(0)
    _lib.check(_lib.lib().gf2_ple_dev(A._on(stream), int(bool(pluq)), P, Q, ctypes.byref(rank), stream), "gf2_ple_dev")
    return rank.value, list(P[:A.nrows]), list(Q[:A.ncols])


def apply_p(A, P, right=False, trans=False, stream=None):
    """mzd_apply_p_left / _left_trans / _right / _right_trans on a device matrix; P: transposition list."""
    arr = (ctypes.c_int * max(len(P), 1))(*P)
    _lib.check(_lib.lib().gf2_apply_p_dev(A._on(stream), arr, len(P), int(bool(right)), int(bool(trans)), stream),
               "gf2_apply_p_dev")
    return A


def pluq_solve_left(A, rank, P, Q, B, check=True, stream=None):
    """Solve A0 X = B in place in B with A as ple(pluq=True) left it -> False if check finds the system inconsistent."""
    pa = (ctypes.c_int * max(len(P), 1))(*P)
    qa = (ctypes.c_int * max(len(Q), 1))(*Q)
    bad = ctypes.c_int(0)
    _lib.check(_lib.lib().gf2_pluq_solve_left_dev(A._on(stream), rank, pa, qa, B._on(stream), int(bool(check)),
                                                  ctypes.byref(bad), stream), "gf2_pluq_solve_left_dev")
    return not bad.value


def solve_left(A, B, check=True, stream=None):
    """Solve A X = B in place (mzd_solve_left's contract): A is left holding its reduced row echelon form, rows 0 .. A.ncols-1 of B hold
    X (free variables 0), further rows are zero -> False if check finds the system inconsistent.  Synchronous on `stream`."""
    bad = ctypes.c_int(0)
    _lib.check(_lib.lib().gf2_solve_left_dev(A._on(stream), B._on(stream), int(bool(check)), ctypes.byref(bad), stream),
               "gf2_solve_left_dev")
    return not bad.value


def trsm(T, B, upper=False, right=False, stream=None):
    """B = T^-1 B (right=False) or B T^-1 (right=True) in place, T unit lower (upper=False) or upper triangular: only its strict
    triangle is read.  Asynchronous on `stream`.  Aliasing: T and B may be views of one buffer, but B may share no word with T (HipError,
    "overlap")."""
    _lib.check(_lib.lib().gf2_trsm_dev(T._on(stream), B._on(stream), int(bool(upper)), int(bool(right)), stream), "gf2_trsm_dev")
    return B


class Mzp:
    """Owner of an mzp_t (mzp_init / mzp_free) for tests and ctypes callers."""

    def __init__(self, length=None, _ptr=None, _window=False):
        self.ptr = _ptr if _ptr is not None else _lib.lib().mzp_init(length)
        self._window = _window

    @staticmethod
    def from_list(values):
        p = Mzp(len(values))
        for i, v in enumerate(values):
            p.ptr.contents.values[i] = v
        return p

    def window(self, begin, end):
        return Mzp(_ptr=_lib.lib().mzp_init_window(self.ptr, begin, end), _window=True)

    def __len__(self):
        return self.ptr.contents.length

    def to_list(self):
        z = self.ptr.contents
        return [z.values[i] for i in range(z.length)]

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                (_lib.lib().mzp_free_window if self._window else _lib.lib().mzp_free)(self.ptr)
            except Exception:
                pass
            self.ptr = None
