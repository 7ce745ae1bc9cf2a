"""ctypes binding of libirec_hip.so (include/irec.h).  Fails loudly when the library has not been built."""
import ctypes
import os

from .errors import IrecLibraryError  # noqa: F401  (re-exported: irec._lib.IrecLibraryError)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "csrc", "libirec_hip.so")   # the product library; no environment variable is read

IREC_OK = 0
IREC_E_INVALID = -1
IREC_E_HIP = -2
IREC_E_NO_DEVICE = -3
IREC_E_WORKSPACE = -4
IREC_FLAG_FORCE_GENERIC = 1
IREC_FLAG_FUSED_PHILOX = 2
IREC_FLAG_ONE_TABLE = 4
IREC_FLAG_TEAM = 8
IREC_FLAG_NO_SPLIT = 16
IREC_FLAG_TEST_SPLIT_ORPHAN = 32   # test hook: the partner workgroups / teams of a shared block leave at once
IREC_FLAG_LISTED_ORDER = 262144     # team encoder: deal the rows of a mid-size call as listed, not by cost (diagnostics)
IREC_FLAG_MARGINS = 524288           # irec_beam_encode_ex: the call reports its top-B margins (out_margin)
IREC_FLAG_NO_TEN = 1048576            # diagnostics: plain calls of at most ten beams stay on encode_team_kernel<10,..> (not encode_ten_kernel)
IREC_FLAG_LANE_SWAPS = 2097152        # diagnostics: search lane-swap masks also for calls of fewer blocks than team slots
IREC_FLAG_LANE_SWAPS_ONES = 4194304   # diagnostics: every lane-swap mask all ones
# layout of the workspace head that the tests of the lane swaps read back (csrc/irec_kernels.h: WS_COUNTER_BYTES, WS_XCH_BYTES, WS_COST_BYTES)
WS_SWAP_MASKS_OFFSET = 2560 + 2 * 384 * 1024 * 8   # uint32 [4 table slots][SWAP_STEPS][4 dim groups], in the row costs' words
WS_HEAD_BYTES = WS_SWAP_MASKS_OFFSET + 4096          # the proposal tables start here
SWAP_STEPS = 64
IREC_FLAG_TABLES_PRESENT = 65536     # the previous call on this workspace / stream was this call's twin: no table launches
IREC_FLAG_REUSE_TABLES = 64        # keep a proposal table whose stamp in the workspace head matches the call's key
IREC_FLAG_SHAPE_SHIFT = 8          # diagnostic workgroup shapes of the team encoder (include/irec.h)
IREC_FLAG_SHAPE = {"default": 0, "2": 2 << 8, "3": 3 << 8, "1x2": 5 << 8, "team": 6 << 8}
IREC_TABLE_STEPS_DEFAULT = 32
IREC_TABLE_STEPS_MAX = 4096
IREC_NORMAL_TABLE_PAD = 16
BIG_PRIME = 10007
MAX_BEAMS = 256
MAX_PARTITIONS = 65536
IREC_ROWS_OK, IREC_ROWS_E_K_RANGE, IREC_ROWS_E_INDEX_RANGE, IREC_ROWS_E_RATIO_TABLE = 0, 1, 2, 3   # irec_rows_status
IREC_REC_E_MAX_K = 18            # irec_rec_status: a block with more partitions than max_K
IREC_REC_E_STRUCTURE = 17        # irec_rec_status: a file whose R or block counts differ from the call's
REC_RAGGED_MAX_RES = 64          # IREC_REC_RAGGED_MAX_RES
IREC_REC_E_COUNT_FILES = 5       # irec_rec_status: a file that uses count tables the call did not bring
IREC_REC_E_TABLE = 19            # irec_rec_status: a symbol table whose entries cannot be coded under
REC_TABLE_LDS_SYMBOLS = 4096     # IREC_REC_TABLE_LDS_SYMBOLS
IREC_REC_E_SEG_MAGIC, IREC_REC_E_SEG_DIRECTORY, IREC_REC_E_SEG_BLOCKS = 20, 21, 22   # irec_rec_status: the segmented reader's own causes
REC_SEG_MAGIC = b"IRSG"          # the first four bytes of a segmented file (NAME.recs)
INT32_MAX = 2 ** 31 - 1
INT64_MAX = 2 ** 63 - 1
SEED_MAX = INT64_MAX - (MAX_PARTITIONS + 2)   # IREC_SEED_MAX: the largest coding seed (seed + step must fit int64; the library checks it)
HEADER_SEED_MAX = 2 ** 32 - 1                 # the seed field of a .rec / .recs header is a uint32


class IrecParams(ctypes.Structure):
    _fields_ = [("kl_per_partition", ctypes.c_float), ("n_samples", ctypes.c_int32), ("n_beams", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("table_dims", ctypes.c_int32 * 4), ("table_steps", ctypes.c_int32)]


class IrecTables(ctypes.Structure):
    """irec_tables of include/irec.h: the caller-supplied tables of a context (irec_create_with)."""
    _fields_ = [("lut10007", ctypes.c_void_p), ("aux_ratios", ctypes.c_void_p), ("n_aux_ratios", ctypes.c_int32)]


class IrecNormalTables(ctypes.Structure):
    """irec_normal_tables of include/irec.h: the device tables of one call of the sequential importance coder."""
    _fields_ = [("table", ctypes.c_void_p * 4), ("dim", ctypes.c_int32 * 4), ("n_samples", ctypes.c_int32), ("steps", ctypes.c_int32)]


class IrecGumbelTable(ctypes.Structure):
    """irec_gumbel_table of include/irec.h: the device table of Gumbel perturbations of one call at finite alpha."""
    _fields_ = [("table", ctypes.c_void_p), ("n_samples", ctypes.c_int32), ("steps", ctypes.c_int32), ("alpha", ctypes.c_float)]


class IrecFitParams(ctypes.Structure):
    """irec_fit_params of include/irec.h: the ratio fitter's parameters."""
    _fields_ = [("kl_per_partition", ctypes.c_float), ("relative_tolerance", ctypes.c_double), ("learning_rate", ctypes.c_double),
                ("max_iters", ctypes.c_int32)]


class IrecQualityParams(ctypes.Structure):
    """irec_quality_params of include/irec.h: the pixel transform of both images and the SSIM constants."""
    _fields_ = [("mul_a", ctypes.c_float), ("add_a", ctypes.c_float), ("mul_b", ctypes.c_float), ("add_b", ctypes.c_float),
                ("clip_a", ctypes.c_int32), ("clip_b", ctypes.c_int32), ("max_val", ctypes.c_float), ("k1", ctypes.c_float),
                ("k2", ctypes.c_float)]


class IrecPlanInfo(ctypes.Structure):
    """irec_plan_info of include/irec.h."""
    _fields_ = [("kernel", ctypes.c_char * 64), ("table_kernel", ctypes.c_char * 32), ("grid", ctypes.c_int32),
                ("waves_per_wg", ctypes.c_int32), ("teams_per_wg", ctypes.c_int32), ("lds_bytes", ctypes.c_int32),
                ("table_steps", ctypes.c_int32), ("n_tables", ctypes.c_int32), ("split", ctypes.c_int32), ("n_cu", ctypes.c_int32),
                ("clock_mhz", ctypes.c_int32), ("split_beams", ctypes.c_int32), ("table_bytes", ctypes.c_int64), ("workspace_bytes", ctypes.c_int64)]

    def as_dict(self):
        return {name: (getattr(self, name).decode() if isinstance(getattr(self, name), bytes) else int(getattr(self, name)))
                for name, _ in self._fields_}


class IrecPlanDetail(ctypes.Structure):
    """irec_plan_detail of csrc/irec_internal.h (test hooks irec_test_plan, irec_test_plan_ws)."""
    _fields_ = [("kind", ctypes.c_int32), ("grid", ctypes.c_int32), ("teams_per_wg", ctypes.c_int32), ("coop_width", ctypes.c_int32),
                ("coop_beams", ctypes.c_int32), ("gang_chunks", ctypes.c_int32), ("placed", ctypes.c_int32), ("split_blocks", ctypes.c_int32),
                ("share_first", ctypes.c_int64), ("n_slots", ctypes.c_int64), ("slabs_in_workspace", ctypes.c_int64),
                ("slab_bytes", ctypes.c_int64), ("fixed_bytes", ctypes.c_int64), ("exchange_rows", ctypes.c_int32), ("exchange_keys", ctypes.c_int32)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


def seed_int(seed):
    """`seed` as a Python int of any size: an integer type (numpy's included), or anything else that int() takes without changing its
    value (a 0-d array, an integral float); ValueError for the rest."""
    if hasattr(seed, "__index__"):
        return seed.__index__()
    try:
        value = None if isinstance(seed, (str, bytes)) else int(seed)
    except (TypeError, ValueError, OverflowError):
        value = None
    if value is None or value != seed:
        raise ValueError(f"seed must be an integer, got {seed!r}")
    return value


def seed64(seed, coding=False):
    """`seed` as the Python int a C entry point takes for an int64 seed, or ValueError: ctypes wraps an int that does not fit the C type
    silently (c_int64(2 ** 63).value == -2 ** 63).  The bound IREC_SEED_MAX of a coding seed is the library's own check; coding=True
    makes it here, for the callers that form seed + step themselves (the host path of the sequential coder)."""
    seed = seed_int(seed)
    if not -INT64_MAX - 1 <= seed <= (SEED_MAX if coding else INT64_MAX):
        raise ValueError(f"seed {seed} is out of range: a coding seed is an int64 of at most IREC_SEED_MAX = {SEED_MAX} "
                         "(INT64_MAX - MAX_PARTITIONS - 2: seed + step must fit int64)")
    return seed


class Seed64:
    """The argument type of every int64 `seed` of include/irec.h: seed64 for whoever calls the library without it (ctypes reports the
    ValueError as a ctypes.ArgumentError)."""

    @classmethod
    def from_param(cls, seed):
        return ctypes.c_int64(seed64(seed))


_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_seed = Seed64
_i32 = ctypes.c_int32
_PP = ctypes.POINTER(IrecParams)

# The argument runs that the batched .rec entries of include/irec.h (and their irec_rec_test_core_* hooks) are put together from
_REC_HEADER = [ctypes.c_uint32] * 6         # seed, block_size, max_index, height, width, channels
_REC_ROWS = [_vp, _i64, _vp, _i64]          # K, k_stride, idx, idx_stride
_REC_TABLES = [_vp, _i32, _vp, _vp, _i64]   # index_cum, n_index_symbols, count_cum, count_first, n_count_cum
_REC_WORKSPACE = [_vp, ctypes.c_size_t, _vp]   # workspace, workspace_bytes, hip_stream


def _rec_batched():
    """irec_rec_{encode,decode}_files[_device | (hook) test_core][ | _ragged | _tables]: eighteen entries, one set of fragments;
    and the seven of the segmented container."""
    rows = {}
    for suffix, blocks_per_res, tables in (("", _i32, False), ("_ragged", _vp, False), ("_tables", _vp, True)):
        tb = _REC_TABLES if tables else []
        enc = _REC_HEADER + [_i32, _i32, blocks_per_res, _i32]       # ..., n_images, n_res_blocks, blocks_per_res, max_K
        dec = [_vp, _vp, _i32, _i32, blocks_per_res, _i32] + tb       # bytes, offsets, n_images, n_res_blocks, blocks_per_res, max_K
        files = [_vp, _i64, _vp, _vp]                                 # out, cap, offsets, status
        outputs = [_vp, _vp, _vp, _vp]                                # headers, K, idx, status
        rows[f"irec_rec_encode_files_device{suffix}"] = (ctypes.c_int, enc + _REC_ROWS + tb + files + _REC_WORKSPACE)
        rows[f"irec_rec_decode_files_device{suffix}"] = (ctypes.c_int, dec + outputs + _REC_WORKSPACE)
        rows[f"irec_rec_test_core_encode_files{suffix}"] = (ctypes.c_int, enc + _REC_ROWS + tb + files)
        rows[f"irec_rec_test_core_decode_files{suffix}"] = (ctypes.c_int, dec + outputs)
        # the host forms: packed rows, a thread count; a status per image only under tables (the others name the file in their error)
        rows[f"irec_rec_encode_files{suffix}"] = (_i64, enc + [_vp, _vp] + tb + files[:3 + tables] + [_i32])
        rows[f"irec_rec_decode_files{suffix}"] = (ctypes.c_int, dec + outputs[:3 + tables] + [_i32])
    # the segmented container (csrc/irec_rec_seg.hip): the ragged layout and segment_blocks, a status per image in every form
    enc = _REC_HEADER + [_i32, _i32, _vp, _i32, _i32]                 # ..., n_images, n_res_blocks, blocks_per_res, segment_blocks, max_K
    dec = [_vp, _vp, _i32, _i32, _vp, _i32, _i32]                     # bytes, offsets, n_images, n_res_blocks, blocks_per_res, segment_blocks, max_K
    rows["irec_rec_encode_files_device_segmented"] = (ctypes.c_int, enc + _REC_ROWS + files + _REC_WORKSPACE)
    rows["irec_rec_decode_files_device_segmented"] = (ctypes.c_int, dec + outputs + _REC_WORKSPACE)
    rows["irec_rec_test_core_encode_files_segmented"] = (ctypes.c_int, enc + _REC_ROWS + files)
    rows["irec_rec_test_core_decode_files_segmented"] = (ctypes.c_int, dec + outputs)
    rows["irec_rec_encode_files_segmented"] = (_i64, enc + [_vp, _vp] + files + [_i32])
    rows["irec_rec_decode_files_segmented"] = (ctypes.c_int, dec + outputs + [_i32])
    rows["irec_rec_seg_workspace_bytes"] = (ctypes.c_size_t, [_i32, _i32, _vp, _i32])
    return rows


# name -> (restype, argtypes); every symbol declared in include/irec.h
SIGNATURES = {
    "irec_last_error": (ctypes.c_char_p, []),
    "irec_version": (ctypes.c_char_p, []),
    "irec_n_samples": (_i32, [ctypes.c_double, ctypes.c_double]),
    "irec_codelength": (ctypes.c_double, [_i64, _i32]),
    "irec_build_lut": (ctypes.c_int, [_vp]),
    "irec_tf_shuffle_perm": (ctypes.c_int, [_seed, _i64, _vp]),
    "irec_philox_uniform_int": (ctypes.c_int, [_seed, _i64, _vp]),
    "irec_importance_encode": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, ctypes.c_double, ctypes.c_double, _seed,
                                              ctypes.POINTER(_i64), _vp]),
    "irec_tf_stateless_normal": (ctypes.c_int, [_seed, _seed, _i64, _vp]),
    "irec_tf_stateless_gumbel": (ctypes.c_int, [_seed, _i64, _vp]),
    "irec_importance_decode": (ctypes.c_int, [_vp, _vp, _i64, _i64, _seed, _vp]),
    "irec_importance_n_samples": (_i64, [ctypes.c_double]),
    "irec_tf_random_normal": (ctypes.c_int, [_seed, _i64, _vp]),
    "irec_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "irec_create_ex": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "irec_create_with": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(IrecTables), ctypes.POINTER(_vp)]),
    "irec_max_partitions": (_i32, [_vp]),
    "irec_destroy": (None, [_vp]),
    "irec_encode_workspace_bytes": (ctypes.c_size_t, [_vp, _PP, _i32, _i32]),
    "irec_encode_workspace_bytes_for": (ctypes.c_size_t, [_vp, _PP, _i64, _i32, _i32]),
    "irec_test_plan": (ctypes.c_int, [_i32, _i32, _PP, _i64, _i32, _i32, _vp, _vp]),
    "irec_test_plan_ws": (ctypes.c_int, [_i32, _i32, _PP, _i64, _i32, _i32, _i64, _vp, _vp]),
    "irec_encode_plan": (ctypes.c_int, [_vp, _PP, _i64, _i32, _i32, ctypes.POINTER(IrecPlanInfo)]),
    "irec_block_kl": (ctypes.c_int, [_vp, _PP, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "irec_beam_encode": (ctypes.c_int, [_vp, _PP, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _seed, _i32,
                                        _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "irec_beam_encode_ex": (ctypes.c_int, [_vp, _PP, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _seed, _i32,
                                           _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "irec_beam_decode": (ctypes.c_int, [_vp, _PP, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _seed, _i32, _vp, _vp, _vp, _vp]),
    "irec_decode_workspace_bytes": (ctypes.c_size_t, [_vp, _PP, _i32]),
    "irec_beam_decode_ws": (ctypes.c_int, [_vp, _PP, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _seed, _i32, _vp, _vp, _vp, _vp,
                                           ctypes.c_size_t, _vp]),
    "irec_decode_tensors_supported": (_i32, [_PP, _i32, _i32]),
    "irec_beam_decode_tensors": (ctypes.c_int, [_vp, _PP, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _seed, _i32, _vp, _vp, _vp, _vp,
                                                ctypes.c_size_t, _vp]),
    "irec_normal_table_floats": (ctypes.c_size_t, [_i32, _i32, _i32]),
    "irec_normal_table_build": (ctypes.c_int, [_seed, _i32, _i32, _i32, _vp, _i32]),
    "irec_gc_importance_encode": (ctypes.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(IrecNormalTables),
                                                 ctypes.c_float, _i32, _vp, _vp, _vp, _vp]),
    "irec_gc_encode_workspace_bytes": (ctypes.c_size_t, [_vp, _i64, _i32]),
    "irec_gc_importance_encode_ws": (ctypes.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(IrecNormalTables),
                                                    ctypes.c_float, _i32, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "irec_gumbel_table_floats": (ctypes.c_size_t, [_i32, _i32]),
    "irec_gumbel_table_build": (ctypes.c_int, [_seed, _i32, _i32, _vp, _i32]),
    "irec_gc_importance_encode_gumbel": (ctypes.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(IrecNormalTables),
                                                        ctypes.c_float, _i32, _vp, _vp, _vp, _vp, ctypes.c_size_t,
                                                        ctypes.POINTER(IrecGumbelTable), _vp]),
    "irec_gc_importance_decode": (ctypes.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.POINTER(IrecNormalTables), _i32,
                                                 _vp, _vp, _vp, _vp]),
    "irec_fit_workspace_bytes": (ctypes.c_size_t, [_i64, _i32]),
    "irec_fit_partitions": (ctypes.c_int, [_vp, ctypes.c_float, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "irec_fit_partitions_host": (ctypes.c_int, [ctypes.c_float, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
    "irec_fit_aux_ratios": (ctypes.c_int, [_vp, ctypes.POINTER(IrecFitParams), _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32,
                                           ctypes.POINTER(_i32), _vp, _vp, ctypes.c_size_t, _vp]),
    "irec_fit_aux_ratios_host": (ctypes.c_int, [ctypes.POINTER(IrecFitParams), _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i32,
                                                ctypes.POINTER(_i32), _vp, _vp, ctypes.c_size_t, _i32]),
    "irec_test_fit_chunk": (_i32, [_i32]),
    "irec_test_det_exp": (ctypes.c_int, [_vp, _i64, _vp]),
    "irec_io_last_error": (ctypes.c_char_p, []),
    "irec_ac_encode": (ctypes.c_int, [_vp, _i32, _vp, _i64, _i32, _vp, _i64, ctypes.POINTER(_i64)]),
    "irec_ac_decode": (ctypes.c_int, [_vp, _i32, _vp, _i64, _i32, _vp, _i64, ctypes.POINTER(_i64)]),
    "irec_rec_pack_bits": (_i64, [_vp, _i64, _vp, _i64]),
    "irec_rec_unpack_bits": (_i64, [_vp, _i64, _vp, _i64]),
    "irec_rec_encode_file": (_i64, [ctypes.c_uint32] * 6 + [_i32, _vp, _vp, _vp, _vp, _i64]),
    "irec_rec_decode_file": (ctypes.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64]),
    "irec_rec_device_workspace_bytes": (ctypes.c_size_t, [_i32, _i32]),
    **_rec_batched(),
    "irec_rec_tables_build": (ctypes.c_int, [_vp, _i32, _vp]),
    "irec_rec_hist_rows": (ctypes.c_int, [_i32, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "irec_rec_hist_rows_device": (ctypes.c_int, [_i32, _i32, _vp, _i32, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "irec_res_device_workspace_bytes": (ctypes.c_size_t, [_i32, _i64]),
    "irec_res_encode_files_device": (ctypes.c_int, [_vp, _vp, ctypes.c_float, _i32] + [ctypes.c_uint32] * 4 + [_vp, _i64, _vp, _vp, _vp,
                                                    ctypes.c_size_t, _vp]),
    "irec_res_decode_files_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_float, _i32] + [ctypes.c_uint32] * 4 + [_vp, _vp, _vp,
                                                    ctypes.c_size_t, _vp]),
    "irec_res_encode_files": (ctypes.c_int, [_vp, _vp, ctypes.c_float, _i32] + [ctypes.c_uint32] * 4 + [_vp, _i64, _vp, _vp, _i32]),
    "irec_res_decode_files": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_float, _i32] + [ctypes.c_uint32] * 4 + [_vp, _vp, _i32]),
    "irec_res_encode_files_device_scales": (ctypes.c_int, [_vp, _vp, _vp, _i32] + [ctypes.c_uint32] * 4 + [_vp, _i64, _vp, _vp, _vp,
                                                           ctypes.c_size_t, _vp]),
    "irec_res_decode_files_device_scales": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32] + [ctypes.c_uint32] * 4 + [_vp, _vp, _vp,
                                                           ctypes.c_size_t, _vp]),
    "irec_res_encode_files_scales": (ctypes.c_int, [_vp, _vp, _vp, _i32] + [ctypes.c_uint32] * 4 + [_vp, _i64, _vp, _vp, _i32]),
    "irec_res_decode_files_scales": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32] + [ctypes.c_uint32] * 4 + [_vp, _vp, _i32]),
    "irec_res_cost_table": (ctypes.c_int, [_vp]),
    "irec_res_scale_bits_workspace_bytes": (ctypes.c_size_t, [_i32] + [ctypes.c_uint32] * 3 + [_i32]),
    "irec_res_scale_bits_device": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32] + [ctypes.c_uint32] * 3 + [_i32, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "irec_res_scale_bits": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32] + [ctypes.c_uint32] * 3 + [_i32, _vp, _vp, _i32]),
    "irec_res_model_counts": (ctypes.c_int, [_i32, ctypes.c_float, _vp]),
    "irec_res_symbol_counts": (ctypes.c_int, [_vp, _vp, ctypes.c_float, _i64, _vp]),
    "irec_quality_workspace_bytes": (ctypes.c_size_t, [_i32] * 5),
    "irec_quality_device": (ctypes.c_int, [_vp, _vp] + [_i32] * 5 + [ctypes.POINTER(IrecQualityParams), _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "irec_quality_host": (ctypes.c_int, [_vp, _vp] + [_i32] * 5 + [ctypes.POINTER(IrecQualityParams), _vp, _vp, _i32]),
    "irec_ideal_workspace_bytes": (ctypes.c_size_t, [_i32, _i64]),
    "irec_posterior_draw_device": (ctypes.c_int, [_vp] * 4 + [_i32, _i64, _seed, ctypes.c_uint32, _i64, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    "irec_posterior_draw_host": (ctypes.c_int, [_vp] * 4 + [_i32, _i64, _seed, ctypes.c_uint32, _i64, _vp, _vp, _i32]),
    "irec_loglik_device": (ctypes.c_int, [_vp] * 3 + [_i32, _i32, _i32, _i64, ctypes.c_double, _vp, _vp, ctypes.c_size_t, _vp]),
    "irec_loglik_host": (ctypes.c_int, [_vp] * 3 + [_i32, _i32, _i32, _i64, ctypes.c_double, _vp, _i32]),
    "irec_resize_bilinear_device": (ctypes.c_int, [_vp] + [_i32] * 8 + [_vp, _vp]),
    "irec_resize_bilinear_host": (ctypes.c_int, [_vp] + [_i32] * 8 + [_vp, _i32]),
    "irec_decode_rows_status": (ctypes.c_int, [_i64, _i32, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp]),
    "irec_test_rows_status_host": (ctypes.c_int, [_i64, _i32, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp]),
    "irec_device_uniform_int": (ctypes.c_int, [_vp, _seed, _i64, _vp, _vp]),
    "irec_shim_stats": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "irec_shim_cat_elu": (ctypes.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "irec_shim_residual_elu": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_float, _vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "irec_test_decoder_sqrt": (ctypes.c_int, [_vp, _vp, _vp]),
    "irec_test_reduce_scatter": (ctypes.c_int, [_vp, _vp, _vp, _i32, _vp]),
    "irec_test_select": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "irec_test_select_quick": (ctypes.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "irec_test_proposal_table": (ctypes.c_int, [_vp, _seed, _i32, _i32, _i32, _vp, _vp]),
    "irec_device_tables": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                          ctypes.POINTER(_vp)]),
}

_lib = None


_lib_path = None


def load(path=None):
    """Load libirec_hip.so.  No fallback of any kind: a missing library is an error.

    `path`: a diagnostic build (csrc/variants/*.so) to load INSTEAD of the product library -- an explicit argument of the
    A/B tooling (scripts/with_lib.py), which must make this call before anything else loads the library; the product
    itself never passes it and no environment variable can redirect the loader."""
    global _lib, _lib_path
    if _lib is not None:
        if path is not None and os.path.abspath(path) != _lib_path:
            raise IrecLibraryError(f"irec._lib.load({path!r}): {_lib_path} is loaded already")
        return _lib
    variant = path is not None
    path = os.path.abspath(path) if variant else LIB_PATH
    if not os.path.exists(path):
        raise IrecLibraryError(
            f"{path} not found: build it with `make -C relative-entropy-coding_amd/csrc` "
            "(or `python -c 'import __graft_entry__ as g; g.build()'`).  irec has no CPU fallback.")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if variant and not hasattr(lib, name):
            continue             # a diagnostic build of older sources (same-box A/B against an earlier round) may lack newer entries
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib, _lib_path = lib, path
    return _lib


def check(status, what=""):
    if status != IREC_OK:
        msg = load().irec_last_error().decode("utf-8", "replace")
        raise IrecLibraryError(f"{what}: irec_status {status}: {msg}")
