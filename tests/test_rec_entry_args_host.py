"""CPU test of what the fourteen .rec entry points of csrc/irec_rec.hip refuse before they run anything: the six device entries
(irec_rec_{encode,decode}_files_device[_ragged|_tables]), their six host hooks (irec_rec_test_core_*) and the two host forms under
tables (irec_rec_{encode,decode}_files_tables).  Every call below has at least one fault, so no entry gets as far as a launch and no
GPU is needed.  The expected return codes and irec_last_error texts are literals, recorded from the library as it was when every entry
still spelled its checks out by hand; the faults in pairs pin the ORDER of the checks (layout, tables, "bad arguments", workspace).
A refused call must leave every output as it found it."""
import ctypes

import numpy as np
import pytest

N, R, BPT, MAX_K = 2, 2, 3, 2
T = R * BPT

# name -> (direction, layout, tables, kind): kind "device" has a workspace and a stream, "core" neither, "host" a thread count
ENTRIES = {}
for _dir in ("encode", "decode"):
    for _suffix, _layout, _tables in (("", "uniform", False), ("_ragged", "ragged", False), ("_tables", "ragged", True)):
        ENTRIES[f"irec_rec_{_dir}_files_device{_suffix}"] = (_dir, _layout, _tables, "device")
        ENTRIES[f"irec_rec_test_core_{_dir}_files{_suffix}"] = (_dir, _layout, _tables, "core")
    ENTRIES[f"irec_rec_{_dir}_files_tables"] = (_dir, "ragged", True, "host")
assert len(ENTRIES) == 14

ALL = lambda e: True
UNIFORM = lambda e: e[1] == "uniform"
RAGGED = lambda e: e[1] == "ragged"
TABLES = lambda e: e[2]
DEVICE = lambda e: e[3] == "device"
STRIDED = lambda e: e[0] == "encode" and e[3] != "host"

INVALID, WORKSPACE = -1, -4
BAD = "bad arguments"
WS = "workspace too small (irec_rec_device_workspace_bytes) or not 8-byte aligned"
R_RANGE = "n_res_blocks outside [1, IREC_REC_RAGGED_MAX_RES]"
BPR_NULL = "blocks_per_res is null"
BPR_ZERO = "an entry of blocks_per_res is below 1"
INDEX_TABLE = "an index table of fewer than 2 symbols"
COUNT_TABLE = "count tables without count_first, or a negative n_count_cum"

# (faults, the entries they can be put to, (return code, what irec_last_error says after "<entry>: "))
TABLE = [
    (("null_K",), ALL, (INVALID, BAD)),
    (("R0",), UNIFORM, (INVALID, BAD)),
    (("R0",), RAGGED, (INVALID, R_RANGE)),
    (("R65",), RAGGED, (INVALID, R_RANGE)),
    (("bpr_null",), RAGGED, (INVALID, BPR_NULL)),
    (("bpr_zero",), UNIFORM, (INVALID, BAD)),
    (("bpr_zero",), RAGGED, (INVALID, BPR_ZERO)),
    (("idx_stride",), STRIDED, (INVALID, BAD)),
    (("index_one_symbol",), TABLES, (INVALID, INDEX_TABLE)),
    (("count_without_first",), TABLES, (INVALID, COUNT_TABLE)),
    (("ws_null",), DEVICE, (WORKSPACE, WS)),
    (("ws_misaligned",), DEVICE, (WORKSPACE, WS)),
    (("ws_short",), DEVICE, (WORKSPACE, WS)),
    # two at once: the earlier check speaks
    (("bpr_zero", "index_one_symbol"), TABLES, (INVALID, BPR_ZERO)),
    (("bpr_zero", "count_without_first"), TABLES, (INVALID, BPR_ZERO)),
    (("index_one_symbol", "count_without_first"), TABLES, (INVALID, INDEX_TABLE)),
    (("index_one_symbol", "null_K"), TABLES, (INVALID, INDEX_TABLE)),
    (("count_without_first", "idx_stride"), lambda e: TABLES(e) and STRIDED(e), (INVALID, COUNT_TABLE)),
    (("bpr_zero", "null_K"), UNIFORM, (INVALID, BAD)),
    (("bpr_zero", "null_K"), RAGGED, (INVALID, BPR_ZERO)),
    (("R65", "ws_null"), lambda e: RAGGED(e) and DEVICE(e), (INVALID, R_RANGE)),
    (("null_K", "ws_null"), DEVICE, (INVALID, BAD)),
    (("idx_stride", "ws_short"), lambda e: STRIDED(e) and DEVICE(e), (INVALID, BAD)),
    (("index_one_symbol", "ws_misaligned"), lambda e: TABLES(e) and DEVICE(e), (INVALID, INDEX_TABLE)),
]
PARAMS = [pytest.param(name, faults, want, id=f"{name}-{'+'.join(faults)}")
          for faults, applies, want in TABLE for name, e in ENTRIES.items() if applies(e)]


def _ptr(a):
    return None if a is None else a.ctypes.data


def _call(lib, name, faults):
    """One refused call: (return code, irec_last_error, whether every output still holds its fill)."""
    direction, layout, tables, kind = ENTRIES[name]
    n_res = 0 if "R0" in faults else 65 if "R65" in faults else R
    bpr = np.full(max(n_res, R), BPT, dtype=np.int32)
    if "bpr_zero" in faults:
        bpr[1] = 0
    if layout == "uniform":
        lay = 0 if "bpr_zero" in faults else BPT
    else:
        lay = None if "bpr_null" in faults else _ptr(bpr)
    index_cum = np.arange(22, dtype=np.uint32)                          # 21 symbols of count 1
    count_cum = np.tile(np.arange(MAX_K + 3, dtype=np.uint32), R)       # per residual block: terminator and K = 0 .. MAX_K
    count_first = (np.arange(R + 1) * (MAX_K + 3)).astype(np.int32)
    tb = [_ptr(index_cum), 1 if "index_one_symbol" in faults else 21, _ptr(count_cum),
          None if "count_without_first" in faults else _ptr(count_first), count_cum.size] if tables else []
    ws_bytes = lib.irec_rec_device_workspace_bytes(N, R)
    ws = np.zeros(ws_bytes + 16, dtype=np.uint8)
    ws_at = (ws.ctypes.data + 7) & ~7
    tail = {"device": [None if "ws_null" in faults else ws_at + 1 if "ws_misaligned" in faults else ws_at,
                       ws_bytes - 1 if "ws_short" in faults else ws_bytes, None],
            "core": [], "host": [1]}[kind]
    if direction == "encode":
        K = np.ones((N, T), dtype=np.int32)
        idx = np.zeros((N, T, MAX_K), dtype=np.int32)
        outputs = [np.full(4096, 0xAB, dtype=np.uint8), np.full(N + 1, -7, dtype=np.int64), np.full(N, -7, dtype=np.int32)]
        fills = [0xAB, -7, -7]
        out, offsets, status = outputs
        rows = [None if "null_K" in faults else _ptr(K)] + ([1] if kind != "host" else []) + [_ptr(idx)] + \
               ([MAX_K - 1 if "idx_stride" in faults else MAX_K] if kind != "host" else [])
        args = [1, 2, 20, 32, 32, 3, N, n_res, lay, MAX_K] + rows + tb + [_ptr(out), out.size, _ptr(offsets), _ptr(status)] + tail
    else:
        blob = np.zeros(64, dtype=np.uint8)
        offsets = np.zeros(N + 1, dtype=np.int64)
        outputs = [np.full((N, 9), 7, dtype=np.uint32), np.full((N, T), -7, dtype=np.int32), np.full((N, T, MAX_K), -7, dtype=np.int32),
                   np.full(N, -7, dtype=np.int32)]
        fills = [7, -7, -7, -7]
        hdr, K, idx, status = outputs
        args = [_ptr(blob), _ptr(offsets), N, n_res, lay, MAX_K] + tb + \
               [_ptr(hdr), None if "null_K" in faults else _ptr(K), _ptr(idx), _ptr(status)] + tail
    rc = getattr(lib, name)(*args)
    text = lib.irec_last_error().decode()
    return int(rc), text, all((o == f).all() for o, f in zip(outputs, fills))


@pytest.mark.parametrize("name, faults, want", PARAMS)
def test_a_refused_call_says_what_it_said_before(name, faults, want):
    from irec import _lib
    lib = _lib.load()
    rc, text, untouched = _call(lib, name, faults)
    assert (rc, text) == (want[0], f"{name}: {want[1]}")
    assert untouched


def test_every_entry_is_bound_with_the_arguments_the_calls_above_pass():
    from irec import _lib
    lib = _lib.load()
    for name, (direction, layout, tables, kind) in ENTRIES.items():
        n_args = (10 if direction == "encode" else 6) + (0 if direction == "decode" else 2 if kind == "host" else 4) + 4 + \
                 5 * tables + {"device": 3, "core": 0, "host": 1}[kind]
        assert len(getattr(lib, name).argtypes) == n_args, name
        assert getattr(lib, name).restype is (ctypes.c_int64 if name == "irec_rec_encode_files_tables" else ctypes.c_int), name
