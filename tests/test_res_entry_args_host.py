"""CPU test of what the twelve entry points of csrc/irec_res.hip, csrc/irec_res_fit.hip and csrc/irec_quality.hip refuse before they
run anything: irec_res_{encode,decode}_files[_device][_scales], irec_res_scale_bits[_device] and irec_quality_{device,host}.  Every
call below has at least one fault, so no entry gets as far as a launch and no GPU is needed.  The expected return codes and
irec_last_error texts are literals, recorded from the library as it was when every entry still spelled its checks out by hand; the
faults in pairs pin the ORDER of the checks (arguments, then workspace).  A refused call must leave every output, and the workspace,
as it found it."""
import ctypes

import numpy as np
import pytest

N, H, W, C, STREAM_LEN, N_CAND = 2, 2, 3, 3, 4, 3
N_STREAMS = -(-H * W * C // STREAM_LEN)
QH = QW = 11                                                            # the smallest planes a quality call takes (one scale)
MAX_STREAM_LEN = 4096

# name -> (unit, direction, one scale per channel, kind): kind "device" has a workspace and a stream, "host" a thread count
ENTRIES = {}
for _dir in ("encode", "decode"):
    for _kind, _k in (("host", ""), ("device", "_device")):
        for _scales, _s in ((False, ""), (True, "_scales")):
            ENTRIES[f"irec_res_{_dir}_files{_k}{_s}"] = ("res", _dir, _scales, _kind)
ENTRIES["irec_res_scale_bits"] = ("fit", None, True, "host")
ENTRIES["irec_res_scale_bits_device"] = ("fit", None, True, "device")
ENTRIES["irec_quality_host"] = ("quality", None, False, "host")
ENTRIES["irec_quality_device"] = ("quality", None, False, "device")
assert len(ENTRIES) == 12

ALL = lambda e: True
RES = lambda e: e[0] == "res"
FIT = lambda e: e[0] == "fit"
QUALITY = lambda e: e[0] == "quality"
SCALES = lambda e: e[2]
DEVICE = lambda e: e[3] == "device"


def both(*conds):
    return lambda e: all(c(e) for c in conds)


INVALID, WORKSPACE = -1, -4
BAD = "bad arguments"
BAD_FIT = "bad arguments (1 .. 64 candidates)"
NULL_Q = "null pointer"
SHAPE_Q = "shape out of range (n, c, h, w >= 1, h and w at most 32768, n c at most 65535, n c h w below 2^31)"
SCALES_Q = "n_scales must be 1 .. 5"
SMALL_Q = "image too small: height or width below 11 at one of the scales"
WS = "workspace too small (%s) or not 8-byte aligned"
WS_RES = WS % "irec_res_device_workspace_bytes"
WS_FIT = WS % "irec_res_scale_bits_workspace_bytes"
WS_Q = WS % "irec_quality_workspace_bytes"

# (faults, the entries they can be put to, (return code, what irec_last_error says after "<entry>: "))
TABLE = [
    (("null_pointer",), RES, (INVALID, BAD)),
    (("null_pointer",), FIT, (INVALID, BAD_FIT)),
    (("null_pointer",), QUALITY, (INVALID, NULL_Q)),
    (("null_output",), RES, (INVALID, BAD)),
    (("null_output",), FIT, (INVALID, BAD_FIT)),
    (("null_output",), QUALITY, (INVALID, NULL_Q)),
    (("height0",), RES, (INVALID, BAD)),
    (("height0",), FIT, (INVALID, BAD_FIT)),
    (("height0",), QUALITY, (INVALID, SHAPE_Q)),
    (("channels65536",), RES, (INVALID, BAD)),
    (("channels65536",), FIT, (INVALID, BAD_FIT)),
    (("channels65536",), QUALITY, (INVALID, SHAPE_Q)),
    (("stream_len0",), RES, (INVALID, BAD)),
    (("stream_len_over",), RES, (INVALID, BAD)),
    (("scales_null",), both(RES, SCALES), (INVALID, BAD)),
    (("scales_null",), FIT, (INVALID, BAD_FIT)),
    (("candidates0",), FIT, (INVALID, BAD_FIT)),
    (("candidates65",), FIT, (INVALID, BAD_FIT)),
    (("n_scales6",), QUALITY, (INVALID, SCALES_Q)),
    (("height10",), QUALITY, (INVALID, SMALL_Q)),
    (("ws_null",), both(RES, DEVICE), (WORKSPACE, WS_RES)),
    (("ws_misaligned",), both(RES, DEVICE), (WORKSPACE, WS_RES)),
    (("ws_short",), both(RES, DEVICE), (WORKSPACE, WS_RES)),
    (("ws_null",), both(FIT, DEVICE), (WORKSPACE, WS_FIT)),
    (("ws_misaligned",), both(FIT, DEVICE), (WORKSPACE, WS_FIT)),
    (("ws_short",), both(FIT, DEVICE), (WORKSPACE, WS_FIT)),
    (("ws_null",), both(QUALITY, DEVICE), (WORKSPACE, WS_Q)),
    (("ws_misaligned",), both(QUALITY, DEVICE), (WORKSPACE, WS_Q)),
    (("ws_short",), both(QUALITY, DEVICE), (WORKSPACE, WS_Q)),
    # two at once: the argument speaks, not the workspace
    (("null_pointer", "ws_null"), both(RES, DEVICE), (INVALID, BAD)),
    (("null_pointer", "ws_null"), both(FIT, DEVICE), (INVALID, BAD_FIT)),
    (("null_pointer", "ws_null"), both(QUALITY, DEVICE), (INVALID, NULL_Q)),
    (("height0", "ws_null"), both(RES, DEVICE), (INVALID, BAD)),
    (("candidates65", "ws_null"), both(FIT, DEVICE), (INVALID, BAD_FIT)),
    (("n_scales6", "ws_null"), both(QUALITY, DEVICE), (INVALID, SCALES_Q)),
    (("stream_len0", "ws_short"), both(RES, DEVICE), (INVALID, BAD)),
    (("scales_null", "ws_misaligned"), both(RES, SCALES, DEVICE), (INVALID, BAD)),
    (("scales_null", "height0"), both(RES, SCALES), (INVALID, BAD)),
    (("scales_null", "height0"), FIT, (INVALID, BAD_FIT)),
    (("scales_null", "stream_len_over"), both(RES, SCALES), (INVALID, BAD)),
    # in a quality call the null pointers come before the shape, and the number of scales before the planes
    (("null_pointer", "height0"), QUALITY, (INVALID, NULL_Q)),
    (("n_scales6", "height0"), QUALITY, (INVALID, SCALES_Q)),
]
PARAMS = [pytest.param(name, faults, want, id=f"{name}-{'+'.join(faults)}")
          for faults, applies, want in TABLE for name, e in ENTRIES.items() if applies(e)]


def _ptr(a):
    return None if a is None else a.ctypes.data


def _tail(kind, faults, ws_bytes):
    """The last arguments of an entry (and the workspace, an output like any other: a refused call writes nothing into it)."""
    if kind == "host":
        return [1], []
    ws = np.full(ws_bytes + 16, 0x5C, dtype=np.uint8)
    ws_at = (ws.ctypes.data + 7) & ~7
    return [None if "ws_null" in faults else ws_at + 4 if "ws_misaligned" in faults else ws_at,
            ws_bytes - 1 if "ws_short" in faults else ws_bytes, None], [(ws, 0x5C)]


def _call(lib, name, faults):
    """One refused call: (return code, irec_last_error, whether every output still holds its fill)."""
    unit, direction, scales, kind = ENTRIES[name]
    h = 0 if "height0" in faults else 10 if "height10" in faults else QH if unit == "quality" else H
    c = 65536 if "channels65536" in faults else C
    if unit == "quality":
        from irec import _lib
        a, b = np.zeros((2, N, C, QH, QW), dtype=np.float32)
        n_scales = 6 if "n_scales6" in faults else 1
        params = _lib.IrecQualityParams(1.0, 0.0, 1.0, 0.0, 0, 0, 1.0, 0.01, 0.03)
        outputs = [(np.full((2, N, C, 5), -7, dtype=np.float32), -7), (np.full(N, -7, dtype=np.float32), -7)]
        tail, ws = _tail(kind, faults, lib.irec_quality_workspace_bytes(N, C, QH, QW, 1))
        args = [None if "null_pointer" in faults else _ptr(a), _ptr(b), N, c, h, QW, n_scales, ctypes.byref(params),
                _ptr(outputs[0][0]), None if "null_output" in faults else _ptr(outputs[1][0])] + tail
    else:
        pixels = np.zeros((N, H, W, C), dtype=np.uint8)
        loc = np.zeros((N, H, W, C), dtype=np.float32)
        loc_arg = None if "null_pointer" in faults else _ptr(loc)
        if unit == "fit":
            cand = np.ones((C, 65), dtype=np.float32)
            cost = np.zeros(1 << 16, dtype=np.uint32)
            n_cand = 0 if "candidates0" in faults else 65 if "candidates65" in faults else N_CAND
            outputs = [(np.full((N, C, 65), -7, dtype=np.int64), -7), (np.full((N, C), -7, dtype=np.int64), -7)]
            tail, ws = _tail(kind, faults, lib.irec_res_scale_bits_workspace_bytes(N, H, W, C, N_CAND))
            args = [_ptr(pixels), loc_arg, None if "scales_null" in faults else _ptr(cand), _ptr(cost), N, h, W, c, n_cand,
                    _ptr(outputs[0][0]), None if "null_output" in faults else _ptr(outputs[1][0])] + tail
        else:
            per_channel = np.ones(C, dtype=np.float32)
            scale = (None if "scales_null" in faults else _ptr(per_channel)) if scales else 1.0
            stream_len = 0 if "stream_len0" in faults else MAX_STREAM_LEN + 1 if "stream_len_over" in faults else STREAM_LEN
            shape = [N, h, W, c, stream_len]
            tail, ws = _tail(kind, faults, lib.irec_res_device_workspace_bytes(N, N_STREAMS))
            status = np.full(N, -7, dtype=np.int32)
            status_arg = None if "null_output" in faults else _ptr(status)
            if direction == "encode":
                out, offsets = np.full(4096, 0xAB, dtype=np.uint8), np.full(N + 1, -7, dtype=np.int64)
                outputs = [(out, 0xAB), (offsets, -7), (status, -7)]
                args = [_ptr(pixels), loc_arg, scale] + shape + [_ptr(out), out.size, _ptr(offsets), status_arg] + tail
            else:
                blob, offsets = np.zeros(256, dtype=np.uint8), np.zeros(N + 1, dtype=np.int64)
                pixels_out = np.full((N, H, W, C), 0xAB, dtype=np.uint8)
                outputs = [(pixels_out, 0xAB), (status, -7)]
                args = [_ptr(blob), _ptr(offsets), loc_arg, scale] + shape + [_ptr(pixels_out), status_arg] + tail
    rc = getattr(lib, name)(*args)
    text = lib.irec_last_error().decode()
    return int(rc), text, all((o == f).all() for o, f in outputs + ws)


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
    for name, (unit, direction, scales, kind) in ENTRIES.items():
        n_args = {"res": 12 if direction == "encode" else 11, "fit": 11, "quality": 10}[unit] + {"device": 3, "host": 1}[kind]
        assert len(getattr(lib, name).argtypes) == n_args, name
        assert getattr(lib, name).restype is ctypes.c_int, name
