"""CPU tests of the device decompress path's host-side parts: the row check's core (csrc/irec_rows_core.h through its host twin
irec_test_rows_status_host) against a numpy referee on the cases of tests/rows_status_cases.py, the header grouping of
harness.decompress_images on the golden containers, and the signatures of the new methods.  The same cases run over exactly-sized
heap buffers under AddressSanitizer / UBSan in scripts/rows_core_check.cpp (profiles/decompress/sanitizer_rows_core.log)."""
import inspect
import io
import os

import numpy as np
import pytest

import rows_status_cases as C

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def referee(case):
    """The twelve lines the core must agree with: per group the first cause of its lowest failing block, a preset status kept."""
    out = case["status0"].copy()
    for g in range(case["n_groups"]):
        for j in range(case["bpg"] if not out[g] else 0):
            at = g * case["bpg"] + j
            b = at if case["block_row"] is None else case["block_row"][at]
            k = int(case["K"][b])
            row = case["idx"][b, :max(0, min(k, case["max_K"]))]
            out[g] = (C.K_RANGE if k < case["min_K"] or k > case["max_K"] else C.RATIO_TABLE if k > case["k_limit"] else
                      C.INDEX_RANGE if ((row < 0) | (row >= C.S)).any() else C.OK)
            if out[g]:
                break
    return out


def test_host_twin_gives_every_plant_its_cause():
    """What the host twin answers for each kind of planted row, over the whole case list (which this also holds to its promise:
    every plant occurs, with the causes it is there for)."""
    import irec
    lib = irec._lib.load()
    cases = C.cases()
    assert len(cases) == 3 * 3 * 3 * 2 * 2 * 2
    want = [C.host_status(lib, c) for c in cases]
    seen = {}                                                  # plant -> statuses it produced anywhere
    for c, w in zip(cases, want):
        for g, name in enumerate(c["plants"]):
            seen.setdefault(name, set()).add(int(w[g]))
    assert set(seen) == set(C.PLANTS)
    assert seen["none"] == {0} and seen["K=max_K"] == {0} and seen["K=0"] == {0, C.K_RANGE}          # K = 0: by min_K
    for name in ("K=max_K+1", "K=-1", "K=int32max"):
        assert seen[name] == {C.K_RANGE}, name
    for v in C.BAD_INDEX:
        assert seen[f"idx{v}@0"] == {C.INDEX_RANGE} and seen[f"idx{v}@K-1"] == {C.INDEX_RANGE}
        assert C.INDEX_RANGE not in seen[f"idx{v}@K"]          # past the row's end: never counts (K_RANGE only where K = 0 < min_K)
    assert seen["two:index-then-K"] >= {C.INDEX_RANGE} and seen["two:K-then-index"] >= {C.K_RANGE}    # the lowest block's cause
    assert seen["preset"] == {7} and C.RATIO_TABLE in seen["K>k_limit"]


@pytest.mark.parametrize("which", range(0, len(C.cases()), 8))
def test_host_twin_equals_the_numpy_referee(which):
    import irec
    lib = irec._lib.load()
    for case in C.cases()[which:which + 8]:
        got = C.host_status(lib, case)
        assert np.array_equal(got, referee(case)), (case["name"], case["plants"], got.tolist(), referee(case).tolist())


def test_bad_arguments_are_refused():
    import irec
    lib = irec._lib.load()
    K, idx, st = np.zeros(4, np.int32), np.zeros((4, 2), np.int32), np.zeros(2, np.int32)
    args = lambda **kw: [kw.get(k, v) for k, v in (("n", 2), ("bpg", 2), ("br", None), ("K", K.ctypes.data), ("ks", 1), ("idx", idx.ctypes.data),
                                                 ("ist", 2), ("max_K", 2), ("min_K", 0), ("lim", C.INT32_MAX), ("S", C.S), ("st", st.ctypes.data))]
    assert lib.irec_test_rows_status_host(*args()) == 0 and not st.any()
    for bad in ({"n": -1}, {"bpg": 0}, {"K": None}, {"idx": None}, {"ks": 0}, {"ist": 1}, {"max_K": -1}, {"S": 0}, {"st": None}):
        assert lib.irec_test_rows_status_host(*args(**bad)) == irec._lib.IREC_E_INVALID, bad
        assert lib.irec_decode_rows_status(*args(**bad), None) == irec._lib.IREC_E_INVALID, bad     # (refused before any launch)
    assert lib.irec_test_rows_status_host(*args(n=0, st=None)) == 0


def test_header_grouping_on_the_golden_containers():
    from irec import harness
    from irec.io.utils import RecHeader
    g = np.load(os.path.join(GOLDEN_DIR, "rec_files.npz"))
    datas = [g[f"{name}_bytes"].tobytes() for name in g["names"]]
    infos, groups = harness.rec_file_groups(datas + [datas[0], datas[0][:27], datas[0][:40]])
    for data, info in zip(datas, infos):
        h = RecHeader.read(io.BytesIO(data))
        assert (info["seed"], info["image_shape"], info["block_size"], info["max_index"]) == (h.seed, tuple(h.image_shape), h.block_size, h.max_index)
        assert (info["R"], info["bpt"], info["max_partitions"]) == (len(h.blocks_per_res_block), h.blocks_per_res_block, h.max_partitions)
    assert infos[2] == infos[0] and infos[3] is None and infos[4] is None            # shorter than the static / the dynamic header
    assert len(groups) == 2 and sorted(groups.values()) == [[0, 2], [1]]             # two shapes: two groups, in the order given
    assert {k[1] for k in groups} == {(32, 32, 3), (512, 768, 3)}
    # equal-count files get the count itself as bpt: what decompress_rec takes
    import irec
    blob, off = irec.io.encode_files(7, (64, 64, 3), 1000, np.ones((2, 3, 9), np.int32), np.zeros((2, 3, 9, 4), np.int32), 36)
    infos, groups = harness.rec_file_groups([blob[off[0]:off[1]].tobytes(), blob[off[1]:off[2]].tobytes()])
    assert groups == {(7, (64, 64, 3), 3, 9): [0, 1]} and infos[0]["max_partitions"] == [1, 1, 1]
    assert irec.io.rec_files_max_K(blob, off) == 1


def test_signatures_of_the_device_decompress_surface():
    import irec
    from irec import harness
    from irec.models import BidirectionalResNetVAE, GraphedDecompress
    want = ["self", "p_loc", "p_scale", "K", "idx", "seed", "block_size", "rows", "status"]
    for cls in (irec.BeamSearchCoder, irec.GaussianCoder):
        sig = inspect.signature(cls.decode_tensors_device)
        assert list(sig.parameters) == want and sig.parameters["rows"].default is None and sig.parameters["status"].default is None
    M = BidirectionalResNetVAE
    assert list(inspect.signature(M._decompress_device).parameters) == ["self", "K", "idx", "seed", "image_shape", "status"]
    assert list(inspect.signature(M.decompress_packed).parameters) == ["self", "K", "idx", "seed", "image_shape", "strict"]
    sig = inspect.signature(M.decompress_rec)
    assert list(sig.parameters) == ["self", "blob", "offsets", "seed", "image_shape", "max_K", "strict"]
    assert sig.parameters["max_K"].default is None and sig.parameters["strict"].default is True
    assert list(inspect.signature(GraphedDecompress.__init__).parameters) == ["self", "model", "image_shape", "seed", "R", "bpt", "max_K", "blob_bytes"]
    sig = inspect.signature(harness.decompress_images)
    assert list(sig.parameters) == ["model", "paths", "batch", "strict"] and sig.parameters["strict"].default is True
    assert list(inspect.signature(M.decompress).parameters) == ["self", "block_indices", "seed", "image_shape"]     # the list path stays
