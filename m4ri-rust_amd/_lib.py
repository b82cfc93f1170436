"""ctypes binding of libm4ri_hip.so (declarations: include/m4ri_hip.h).

The library is the product: if it is missing or cannot be loaded this module raises -- there is
no Python or CPU stand-in for the multiply path.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libm4ri_hip.so")

c_word_p = ctypes.POINTER(ctypes.c_uint64)


class MzdBlock(ctypes.Structure):
    """mzd_block_t (m4ri-sys/src/mzd.rs:16-21)."""
    _fields_ = [("size", ctypes.c_size_t), ("begin", c_word_p), ("end", c_word_p)]


class Mzd(ctypes.Structure):
    """mzd_t, 64 bytes (m4ri-sys/src/mzd.rs:24-79)."""
    _fields_ = [
        ("nrows", ctypes.c_int),
        ("ncols", ctypes.c_int),
        ("width", ctypes.c_int),
        ("rowstride", ctypes.c_int),
        ("offset_vector", ctypes.c_int),
        ("row_offset", ctypes.c_int),
        ("flags", ctypes.c_uint8),
        ("blockrows_log", ctypes.c_uint8),
        ("padding", ctypes.c_uint8 * 14),
        ("high_bitmask", ctypes.c_uint64),
        ("blocks", ctypes.POINTER(MzdBlock)),
        ("rows", ctypes.POINTER(c_word_p)),
    ]


assert ctypes.sizeof(Mzd) == 64

MzdP = ctypes.POINTER(Mzd)


class DMatStruct(ctypes.Structure):
    """gf2_dmat (include/m4ri_hip.h, section 2)."""
    _fields_ = [("data", ctypes.c_void_p), ("ld", ctypes.c_int64), ("nrows", ctypes.c_int), ("ncols", ctypes.c_int)]


DMatP = ctypes.POINTER(DMatStruct)


class Mzp(ctypes.Structure):
    """mzp_t (include/m4ri_hip.h; m4ri-sys/src/mzp.rs treats it as opaque)."""
    _fields_ = [("values", ctypes.POINTER(ctypes.c_int)), ("length", ctypes.c_int)]


MzpP = ctypes.POINTER(Mzp)

ALGO_AUTO, ALGO_M4RM, ALGO_STRASSEN, ALGO_NAIVE = 0, 1, 2, 3

_I = ctypes.c_int
_PROTOS = {
    # name: (restype, argtypes)
    "mzd_init": (MzdP, [_I, _I]),
    "mzd_free": (None, [MzdP]),
    "mzd_init_window": (MzdP, [MzdP, _I, _I, _I, _I]),
    "mzd_copy": (MzdP, [MzdP, MzdP]),
    "mzd_equal": (_I, [MzdP, MzdP]),
    "mzd_randomize": (None, [MzdP]),
    "mzd_set_ui": (None, [MzdP, ctypes.c_uint]),
    "mzd_transpose": (MzdP, [MzdP, MzdP]),
    "mzd_add": (MzdP, [MzdP, MzdP, MzdP]),
    "mzd_sub": (MzdP, [MzdP, MzdP, MzdP]),
    "mzd_concat": (MzdP, [MzdP, MzdP, MzdP]),
    "mzd_stack": (MzdP, [MzdP, MzdP, MzdP]),
    "mzd_submatrix": (MzdP, [MzdP, MzdP, _I, _I, _I, _I]),
    "mzd_is_zero": (_I, [MzdP]),
    "mzd_row_swap": (None, [MzdP, _I, _I]),
    "mzd_copy_row": (None, [MzdP, _I, MzdP, _I]),
    "mzd_col_swap": (None, [MzdP, _I, _I]),
    "mzd_row_clear_offset": (None, [MzdP, _I, _I]),
    "mzd_invert_naive": (MzdP, [MzdP, MzdP, MzdP]),
    "m4ri_opt_k": (_I, [_I, _I, _I]),
    "mzd_make_table": (None, [MzdP, _I, _I, _I, MzdP, ctypes.POINTER(_I)]),
    "mzd_echelonize": (_I, [MzdP, _I]),
    "mzd_echelonize_m4ri": (_I, [MzdP, _I, _I]),
    "mzd_echelonize_pluq": (_I, [MzdP, _I]),
    "mzd_inv_m4ri": (MzdP, [MzdP, MzdP, _I]),
    "mzd_solve_left": (_I, [MzdP, MzdP, _I, _I]),
    "mzp_init": (MzpP, [_I]),
    "mzp_free": (None, [MzpP]),
    "mzp_init_window": (MzpP, [MzpP, _I, _I]),
    "mzp_free_window": (None, [MzpP]),
    "Mzp_free_window": (None, [MzpP]),
    "mzp_copy": (MzpP, [MzpP, MzpP]),
    "mzp_set_ui": (None, [MzpP, ctypes.c_uint]),
    "mzp_print": (None, [MzpP]),
    "mzd_apply_p_left": (None, [MzdP, MzpP]),
    "mzd_apply_p_left_trans": (None, [MzdP, MzpP]),
    "mzd_apply_p_right": (None, [MzdP, MzpP]),
    "mzd_apply_p_right_trans": (None, [MzdP, MzpP]),
    "mzd_ple": (_I, [MzdP, MzpP, MzpP, _I]),
    "mzd_pluq": (_I, [MzdP, MzpP, MzpP, _I]),
    "mzd_pluq_solve_left": (_I, [MzdP, _I, MzpP, MzpP, MzdP, _I, _I]),
    "mzd_trsm_lower_left": (None, [MzdP, MzdP, _I]),
    "mzd_trsm_upper_left": (None, [MzdP, MzdP, _I]),
    "mzd_trsm_lower_right": (None, [MzdP, MzdP, _I]),
    "mzd_trsm_upper_right": (None, [MzdP, MzdP, _I]),
    "mzd_kernel_left_pluq": (MzdP, [MzdP, _I]),
    "mzd_mul_m4rm": (MzdP, [MzdP, MzdP, MzdP, _I]),
    "mzd_addmul_m4rm": (MzdP, [MzdP, MzdP, MzdP, _I]),
    "mzd_mul": (MzdP, [MzdP, MzdP, MzdP, _I]),
    "mzd_addmul": (MzdP, [MzdP, MzdP, MzdP, _I]),
    "mzd_mul_naive": (MzdP, [MzdP, MzdP, MzdP]),
    "mzd_addmul_naive": (MzdP, [MzdP, MzdP, MzdP]),
    "_mzd_mul_naive": (MzdP, [MzdP, MzdP, MzdP, _I]),
    "_mzd_mul_va": (MzdP, [MzdP, MzdP, MzdP, _I]),
    "gf2_device_count": (_I, []),
    "gf2_last_error": (ctypes.c_char_p, []),
    "gf2_dmat_alloc": (_I, [DMatP, _I, _I]),
    "gf2_dmat_free": (None, [DMatP]),
    "gf2_dmat_free_async": (_I, [DMatP, ctypes.c_void_p]),
    "gf2_dmat_upload": (_I, [DMatP, MzdP, ctypes.c_void_p]),
    "gf2_dmat_download": (_I, [MzdP, DMatP, ctypes.c_void_p]),
    "gf2_dmat_fill_random": (_I, [DMatP, ctypes.c_uint64, ctypes.c_void_p]),
    "gf2_dmat_fill_random_rows": (_I, [DMatP, ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p]),
    "gf2_dmat_fill_random_block": (_I, [DMatP, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, _I, ctypes.c_void_p]),
    "gf2_strassen_levels": (_I, [_I, _I, _I, _I, _I]),
    "gf2_strassen_pass_bytes": (ctypes.c_double, [_I, _I, _I, _I]),
    "gf2_mul_plan": (_I, [_I, _I, _I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "gf2_model_time": (ctypes.c_double, [_I, _I, _I, _I]),
    "gf2_tile_plan": (ctypes.c_double, [_I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
    "gf2_tile_plan_band": (None, [_I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
    "gf2_mul_dev": (_I, [DMatP, DMatP, DMatP, _I, _I, _I, ctypes.c_void_p]),
    "gf2_mul_nt_dev": (_I, [DMatP, DMatP, DMatP, _I, ctypes.c_void_p]),
    "gf2_add_dev": (_I, [DMatP, DMatP, DMatP, ctypes.c_void_p]),
    "gf2_transpose_dev": (_I, [DMatP, DMatP, ctypes.c_void_p]),
    "gf2_equal_dev": (_I, [DMatP, DMatP, ctypes.POINTER(_I), ctypes.c_void_p]),
    "gf2_copy_block_dev": (_I, [DMatP, _I, _I, DMatP, _I, _I, _I, _I, _I, ctypes.c_void_p]),
    "gf2_submatrix_dev": (_I, [DMatP, DMatP, _I, _I, _I, _I, ctypes.c_void_p]),
    "gf2_concat_dev": (_I, [DMatP, DMatP, DMatP, ctypes.c_void_p]),
    "gf2_stack_dev": (_I, [DMatP, DMatP, DMatP, ctypes.c_void_p]),
    "gf2_solve_left_dev": (_I, [DMatP, DMatP, _I, ctypes.POINTER(_I), ctypes.c_void_p]),
    "gf2_echelonize_dev": (_I, [DMatP, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.c_void_p]),
    "gf2_inverse_dev": (_I, [DMatP, DMatP, ctypes.POINTER(_I), ctypes.c_void_p]),
    "gf2_echelonize_batch_dev": (_I, [DMatP, _I, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_inverse_batch_dev": (_I, [DMatP, DMatP, _I, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_elim_batch_plan": (_I, [_I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
    "gf2_ple_dev": (_I, [DMatP, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.c_void_p]),
    "gf2_apply_p_dev": (_I, [DMatP, ctypes.POINTER(_I), _I, _I, _I, ctypes.c_void_p]),
    "gf2_pluq_solve_left_dev": (_I, [DMatP, _I, ctypes.POINTER(_I), ctypes.POINTER(_I), DMatP, _I, ctypes.POINTER(_I),
                                     ctypes.c_void_p]),
    "gf2_trsm_dev": (_I, [DMatP, DMatP, _I, _I, ctypes.c_void_p]),
    "gf2_nullspace_dev": (_I, [DMatP, DMatP, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.c_void_p]),
    "gf2_nullspace_last_assembly_ms": (ctypes.c_double, []),
    "gf2_mul_workspace_bytes": (ctypes.c_size_t, [_I, _I, _I, _I, _I]),
    "gf2_mul_multi": (MzdP, [MzdP, MzdP, MzdP, _I, _I, ctypes.POINTER(_I), _I]),
    "gf2_mzd_cache_on_device": (_I, [MzdP]),
    "gf2_mzd_uncache": (None, [MzdP]),
    "gf2_set_result_side_cols": (_I, [_I]),
    "gf2_mzd_prewarm": (_I, [_I, _I, _I]),
    "gf2_trim": (_I, []),
    "gf2_mul_host_small": (_I, [MzdP, MzdP, MzdP, _I]),
    "gf2_mul_nt_host_small": (_I, [MzdP, MzdP, MzdP, _I]),
    "gf2_echelonize_host_small": (_I, [MzdP, _I]),
    "gf2_ple_host_small": (_I, [MzdP, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "gf2_trsm_host_small": (_I, [MzdP, MzdP, _I, _I]),
    "gf2_nullspace_host_small": (_I, [MzdP, ctypes.POINTER(MzdP)]),
    "gf2_host_small_calls": (ctypes.c_longlong, []),
    "gf2_mzd_save": (_I, [ctypes.c_char_p, MzdP]),
    "gf2_mzd_load": (MzdP, [ctypes.c_char_p]),
    "gf2_prof_enable": (None, [_I]),
    "gf2_prof_read": (_I, [ctypes.POINTER(_I), ctypes.POINTER(ctypes.c_double), _I]),
    "gf2_kernel_census": (ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]),
    "gf2_dev_alloc_counts": (None, [ctypes.POINTER(ctypes.c_longlong)]),
    "gf2_host_plan_model": (_I, [_I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_double)]),
}

# every symbol include/m4ri_hip.h declares; tests check the library exports all of them (the mzp_* names are declared for
# ctypes but are not part of the header check's mzd_* / gf2_* pattern)
DECLARED_SYMBOLS = tuple(k for k in _PROTOS if not k.lower().startswith("mzp_"))

# header under include/ -> its table.  lib() binds every table in here and the *_SYMBOLS tuples are read from here, so a table cannot
# exist without being bound.
_TABLES = {"m4ri_hip.h": _PROTOS}

# what the companion header include/m4ri_hip_gather.h declares: a table of its own, so that DECLARED_SYMBOLS stays the list of
# m4ri_hip.h (tests/test_gather_contract.py checks this header against the library)
_TABLES["m4ri_hip_gather.h"] = {
    "gf2_gather_rows_dev": (_I, [DMatP, DMatP, ctypes.c_void_p, _I, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_gather_cols_dev": (_I, [DMatP, DMatP, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_gather_cols_plan": (_I, [_I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
}
GATHER_SYMBOLS = tuple(_TABLES["m4ri_hip_gather.h"])

# ... and include/m4ri_hip_weight.h (tests/test_weight_contract.py)
_TABLES["m4ri_hip_weight.h"] = {
    "gf2_row_weights_dev": (_I, [DMatP, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_col_weights_dev": (_I, [DMatP, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_count_ones_dev": (_I, [DMatP, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_select_weights_dev": (_I, [ctypes.c_void_p, _I, _I, _I, ctypes.c_void_p, _I, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_weights_plan": (_I, [_I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
}
WEIGHT_SYMBOLS = tuple(_TABLES["m4ri_hip_weight.h"])

# ... and include/m4ri_hip_wht.h (tests/test_wht_contract.py)
_TABLES["m4ri_hip_wht.h"] = {
    "gf2_lpn_tally_dev": (_I, [DMatP, _I, _I, _I, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_wht_dev": (_I, [ctypes.c_void_p, _I, ctypes.c_void_p]),
    "gf2_lpn_errors_dev": (_I, [DMatP, _I, _I, _I, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_min_weight_dev": (_I, [ctypes.c_void_p, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_wht_plan": (_I, [_I, ctypes.POINTER(ctypes.c_longlong)]),
}
WHT_SYMBOLS = tuple(_TABLES["m4ri_hip_wht.h"])

# ... and include/m4ri_hip_bkw.h (tests/test_bkw_contract.py)
LF1_KEEP_ZERO = 1
_TABLES["m4ri_hip_bkw.h"] = {
    "gf2_class_first_dev": (_I, [DMatP, _I, _I, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_lf1_reduce_dev": (_I, [DMatP, DMatP, _I, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_lf1_plan": (_I, [_I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
}
BKW_SYMBOLS = tuple(_TABLES["m4ri_hip_bkw.h"])

# ... and include/m4ri_hip_cover.h (tests/test_cover_contract.py)
COVER_MAX_N, COVER_MAX_R, COVER_MAX_CODES, COVER_MAX_SEGS, COVER_MAX_LEADERS = 32, 12, 16, 256, 16384
COVER_IDENTITY, COVER_DROP, COVER_REPETITION, COVER_HAMMING, COVER_GOLAY23 = range(5)


class CoverCodeStruct(ctypes.Structure):
    """gf2_cover_code (include/m4ri_hip_cover.h), 56 bytes."""
    _fields_ = [("n", ctypes.c_int), ("k", ctypes.c_int), ("h", ctypes.c_uint32 * COVER_MAX_R)]


assert ctypes.sizeof(CoverCodeStruct) == 56

CoverCodeP = ctypes.POINTER(CoverCodeStruct)
_TABLES["m4ri_hip_cover.h"] = {
    "gf2_cover_code_named": (_I, [_I, _I, CoverCodeP]),
    "gf2_cover_leaders": (_I, [CoverCodeP, ctypes.c_void_p, ctypes.POINTER(_I)]),
    "gf2_cover_reduce_dev": (_I, [DMatP, DMatP, _I, CoverCodeP, _I, ctypes.c_void_p, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_cover_plan": (_I, [_I, _I, CoverCodeP, _I, ctypes.c_void_p, _I, ctypes.POINTER(ctypes.c_longlong)]),
}
COVER_SYMBOLS = tuple(_TABLES["m4ri_hip_cover.h"])

# ... and include/m4ri_hip_lf2.h (tests/test_lf2_contract.py)
_TABLES["m4ri_hip_lf2.h"] = {
    "gf2_class_sort_dev": (_I, [DMatP, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_lf2_reduce_dev": (_I, [DMatP, DMatP, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_lf2_plan": (_I, [_I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
}
LF2_SYMBOLS = tuple(_TABLES["m4ri_hip_lf2.h"])

# ... and include/m4ri_hip_draw.h (tests/test_draw_contract.py)
DRAW_BERNOULLI, DRAW_INDICES, DRAW_SUBSETS, DRAW_PERMUTATION = 1, 2, 3, 4
_TABLES["m4ri_hip_draw.h"] = {
    "gf2_bernoulli_dev": (_I, [DMatP, ctypes.c_uint32, ctypes.c_uint64, _I, ctypes.c_void_p]),
    "gf2_bernoulli_block_dev": (_I, [DMatP, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, _I, _I, ctypes.c_void_p]),
    "gf2_draw_indices_dev": (_I, [ctypes.c_void_p, ctypes.c_longlong, _I, ctypes.c_uint64, ctypes.c_void_p]),
    "gf2_draw_subsets_dev": (_I, [ctypes.c_void_p, _I, _I, _I, ctypes.c_uint64, _I, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_draw_permutation_dev": (_I, [ctypes.c_void_p, _I, ctypes.c_uint64, ctypes.c_void_p]),
    "gf2_draw_plan": (_I, [_I, ctypes.c_longlong, _I, ctypes.c_uint32, ctypes.POINTER(ctypes.c_longlong)]),
}
DRAW_SYMBOLS = tuple(_TABLES["m4ri_hip_draw.h"])

# ... and include/m4ri_hip_join.h (tests/test_join_contract.py)
_TABLES["m4ri_hip_join.h"] = {
    "gf2_join_dev": (_I, [DMatP, DMatP, DMatP, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _I, _I,
                          ctypes.c_void_p]),
    "gf2_join_plan": (_I, [_I, _I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
}
JOIN_SYMBOLS = tuple(_TABLES["m4ri_hip_join.h"])

# ... and include/m4ri_hip_sums.h (tests/test_sums_contract.py)
_TABLES["m4ri_hip_sums.h"] = {
    "gf2_subset_sums_dev": (_I, [DMatP, DMatP, DMatP, _I, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_void_p, _I, _I, ctypes.c_void_p]),
    "gf2_unrank_subsets_dev": (_I, [ctypes.c_void_p, _I, ctypes.c_longlong, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_subset_count": (ctypes.c_longlong, [_I, _I]),
    "gf2_subset_rank": (ctypes.c_longlong, [ctypes.POINTER(_I), _I]),
    "gf2_subset_unrank": (_I, [ctypes.c_longlong, _I, ctypes.POINTER(_I)]),
    "gf2_subset_sums_plan": (_I, [_I, _I, _I, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]),
}
SUMS_SYMBOLS = tuple(_TABLES["m4ri_hip_sums.h"])

# ... and include/m4ri_hip_join_select.h (tests/test_join_select_contract.py)
_TABLES["m4ri_hip_join_select.h"] = {
    "gf2_join_select_dev": (_I, [DMatP, DMatP, DMatP, _I, _I, _I, _I, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_join_select_plan": (_I, [_I, _I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
}
JOIN_SELECT_SYMBOLS = tuple(_TABLES["m4ri_hip_join_select.h"])

# ... and include/m4ri_hip_near.h (tests/test_near_contract.py)
_TABLES["m4ri_hip_near.h"] = {
    "gf2_near_pairs_dev": (_I, [DMatP, DMatP, DMatP, _I, _I, _I, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_void_p]),
    "gf2_nearest_dev": (_I, [DMatP, DMatP, _I, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_near_plan": (_I, [_I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
}
NEAR_SYMBOLS = tuple(_TABLES["m4ri_hip_near.h"])

# ... and include/m4ri_hip_unique.h (tests/test_unique_contract.py)
_TABLES["m4ri_hip_unique.h"] = {
    "gf2_sort_rows_dev": (_I, [DMatP, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_unique_rows_dev": (_I, [DMatP, _I, _I, ctypes.c_void_p, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_sort_rows_plan": (_I, [_I, _I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
}
UNIQUE_SYMBOLS = tuple(_TABLES["m4ri_hip_unique.h"])

# ... and include/m4ri_hip_find.h (tests/test_find_contract.py)
_TABLES["m4ri_hip_find.h"] = {
    "gf2_find_rows_dev": (_I, [DMatP, DMatP, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_find_rows_plan": (_I, [_I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
}
FIND_SYMBOLS = tuple(_TABLES["m4ri_hip_find.h"])

# ... and include/m4ri_hip_join_rows.h (tests/test_join_rows_contract.py)
_TABLES["m4ri_hip_join_rows.h"] = {
    "gf2_group_rows_dev": (_I, [DMatP, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "gf2_join_rows_dev": (_I, [DMatP, DMatP, DMatP, _I, _I, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _I, _I,
                               ctypes.c_void_p]),
    "gf2_join_rows_plan": (_I, [_I, _I, _I, _I, _I, ctypes.POINTER(ctypes.c_longlong)]),
}
JOIN_ROWS_SYMBOLS = tuple(_TABLES["m4ri_hip_join_rows.h"])

_lib = None


def lib():
    """Load libm4ri_hip.so (once). Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C m4ri-rust_amd/csrc`). There is no fallback for the HIP multiply path.")
        handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in [item for table in _TABLES.values() for item in table.items()]:
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


class HipError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        msg = lib().gf2_last_error()
        raise HipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
