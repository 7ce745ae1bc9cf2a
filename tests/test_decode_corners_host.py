"""The decoder's corner cases (tests/decode_cases.py), host side: every compiled decode_* build is reached by a case, every build's
cases contain the rows and blocks at which it can go wrong, the restated dispatch agrees with the library, and the reference itself
stays within the project's float64 decode bound on these rows (a condition on the reference alone).  The device side is
tests/test_decode_corners_gpu.py."""
import ctypes
import functools

import numpy as np
import pytest

import decode_cases as dc
import f64_referee as R
import kernel_names as kn

N_CU = (256, 64, 304)             # the full device, and two partitions of other sizes: the dispatch names the same builds


def _routes(n_cu):
    """build -> [(case, mode, table_steps, K_tab)] over every call tests/test_decode_corners_gpu.py makes."""
    out = {}
    for case in dc.all_cases(n_cu):
        for mode, ts, name, kt in case.routes(n_cu):
            out.setdefault(name, []).append((case, mode, ts, kt))
    return out


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
def test_every_compiled_decoder_build_is_named():
    compiled = {k for k in kn.compiled_kernels() if k.startswith("decode_")}
    assert len(compiled) == 8, sorted(compiled)
    for n_cu in N_CU:
        named = set(_routes(n_cu))
        assert not compiled - named, f"compiled, but no case reaches them on {n_cu} CUs: {sorted(compiled - named)}"
        assert not named - compiled, f"named by the restated dispatch, but not in the library: {sorted(named - compiled)}"


def _live_K(case):
    return [int(k) for b, k in enumerate(case.K) if b not in case.bad]


@pytest.mark.parametrize("n_cu", N_CU)
def test_every_corner_is_reached_in_every_build(n_cu):
    routes = _routes(n_cu)
    assert len(routes) == 8
    for name, calls in sorted(routes.items()):
        table = "<true" in name and name != "decode_kernel<true>"
        assert any(k > 64 for c, *_ in calls for k in _live_K(c)), f"{name}: no row takes a second lane vector"
        dims = {d for c, *_ in calls for d in c.lay.block_dims}
        assert any(d % 4 for d in dims), f"{name}: no block with a partial last quad"
        assert any(d < 4 for d in dims), f"{name}: no block of fewer dims than a lane quad"
        if table:
            assert all(kt > 0 for *_, kt in calls)
            # the window's edge inside one call: K = K_tab streams table rows to the end, K = K_tab + 1 draws in the kernel
            assert any(kt in _live_K(c) and kt + 1 in _live_K(c) for c, _, _, kt in calls), f"{name}: no call with K_tab and K_tab + 1"
            # table rows in a second lane vector, with one to three steps in it (the prefetch clamp) and a full one
            for k in (65, 66, 67, 127, 128):
                assert any(kt >= k and k in _live_K(c) for c, _, _, kt in calls), f"{name}: no table call with K = {k}"
        else:
            assert all(kt == 0 for *_, kt in calls)
        assert any(c.bad for c, *_ in calls), f"{name}: no row that is not decodable"
    # the wrapping hash sum: two blocks share too few rows for tables, so it runs where the draw is fused into the kernel
    assert {n for n, calls in routes.items() if any(c.name == "wrap" for c, *_ in calls)} == \
        {"decode_wave_kernel<false>", "decode_tensor_kernel<false,3>", "decode_kernel<false>"}
    # the staged kernel's layouts take the builds and staging passes they are there for
    for (n, bs), (slots, rmax, vec) in dc.STAGED_LAYOUTS.items():
        lay = dc.Lay(3, n, bs)
        assert dc.tensors_supported(n, bs) and lay.bpt * -(-lay.bs // 256) == slots and dc.staged_rmax(n, bs) == rmax and (n % 4 == 0) == vec, (n, bs)
        for table in (True, False):
            assert (dc.tensor_waves(n, lay.bs, table)[0] < 12) == (slots < 12)
    assert dc.tensor_waves(1, 1, True)[0] == 1 and not dc.tensors_supported(*dc.STAGED_UNSUPPORTED)
    # the tensor loop: three passes for some workgroups, two for the others; every wave count below twelve occurs too
    loop = dc.loop_case(n_cu)
    for table in (True, False):
        grid = dc.staged_grid(n_cu, loop.lay, table)
        passes = {len(range(w, loop.lay.n_tensors, grid)) for w in range(grid)}
        assert passes == {2, 3}, (table, grid, passes)
    assert dc.tensor_waves(70, 7, True)[0] == 10
    # the large grids: the LDS-table build of the legacy kernel, and only there
    for case in (dc.grid_case(n_cu), dc.grid_case(n_cu, True)):
        assert dc.dispatch(n_cu, "legacy", case.lay, case.S, case.max_K)[0] == "decode_kernel<true>"
        assert case.lay.n_blocks - 16 * n_cu in range(0, 8)
    assert all(c.lay.n_blocks < 16 * n_cu for c, *_ in routes["decode_kernel<false>"])


def test_rows_are_what_the_cases_say():
    for case in dc.all_cases(256):
        lay = case.lay
        assert case.K.shape == (lay.n_blocks,) and case.idx.shape == (lay.n_blocks, case.max_K) and case.idx.dtype == np.int32
        for b in range(lay.n_blocks):
            k = int(case.K[b])
            if b in case.bad:
                continue
            assert 0 <= k <= case.max_K and (case.idx[b, k:] == dc.PAD).all()
            assert ((case.idx[b, :k] >= 0) & (case.idx[b, :k] < case.S)).all(), (case, b)
            if case.name != "wrap" and k > 2:
                assert case.idx[b, 1] == case.S - 1 and case.idx[b, 2] == 0
    bad = dc.bad_case(261, 256)
    planted = sorted(bad.bad)
    assert [int(bad.K[b]) for b in planted] == [129] * 6 + [-1, dc.MAX_K + 1]
    assert [(t, int(bad.idx[b, t])) for b, (t, _) in zip(planted, dc.BAD_PLANTS)] == [(0, 36), (63, 36), (64, 36), (128, 36), (70, -1), (3, dc.PAD)]
    assert set(dc.ladder_Ks(dc.Lay(dc.N_LADDER, 7, 4))) == set(dc.K_LADDER) and max(dc.K_LADDER) < dc.MAX_K
    assert dc.wrap_case().idx[:, :6].tolist() == [[(1 << 24) - 1] * 6] * 2


GRID_BS = (1, 7, 255, 256, 257, 1000, None)      # None: one block, block_size = n


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
def test_restated_staged_limits_match_the_library():
    """irec_decode_tensors_supported on EVERY n from 1 to 20000 (the edges: 60 unit slots -- n = 60, 420, 15300, 15360, 7710, 15000 for
    the block sizes below -- and the LDS)."""
    from irec import _lib
    from irec.engine import Engine
    lib = _lib.load()
    p = Engine.params(3.0, 36, 20)
    edges = {1: 60, 7: 420, 255: 15300, 256: 15360, 257: 7710, 1000: 15000, None: 15360}
    for bs in GRID_BS:
        got = [n for n in range(1, 20001) if lib.irec_decode_tensors_supported(ctypes.byref(p), n, bs or n)]
        want = [n for n in range(1, 20001) if dc.tensors_supported(n, bs or n)]
        assert got == want, bs
        assert got == list(range(1, edges[bs] + 1)), (bs, got[-1])
    assert lib.irec_decode_tensors_supported(ctypes.byref(p), 0, 1) == 0 and lib.irec_decode_tensors_supported(ctypes.byref(p), 5, 0) == 0
    assert lib.irec_decode_tensors_supported(ctypes.byref(p), 25000, 100000) == 0     # (block_size is cut to n first: 98 slots)


@functools.lru_cache(maxsize=1024)
def _uniform_int(seed, count):
    from oracle import oracle as O
    a = O.uniform_int(seed, count)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize("n,bs", dc.LADDER_LAYOUTS)
def test_reference_stays_within_the_float64_bound(oracle, n, bs):
    """The oracle's decode_block of every ladder row against f64_referee.decode64, within test_f64_referee's C_DECODE * U * dmag.
    Measured, as the largest error over bound of any dim: 0.92 at K = 1 (four roundings, which the bound counts one by one), 0.6 at
    K = 2, 0.3 at K = 5, at most 0.01 from K = 31 on; family wide 0.2 to 0.9 at every K."""
    from test_f64_referee import C_DECODE, U
    perm = dc.perm_of(n)
    for family in dc.ladder_families(n, bs):
        case = dc.ladder_case(n, bs, family)
        mp, sp, want = dc.expected(case)
        lay, worst = case.lay, 0.0
        for i in range(lay.n_tensors):
            for j, (lo, hi) in enumerate(oracle.split_blocks(n, lay.bs)):
                b = i * lay.bpt + j
                g = perm[lo:hi]
                s64, dmag = R.decode64(mp[i, g], sp[i, g], case.idx[b, :case.K[b]], dc.SEED, case.S, uniform_int=_uniform_int)
                err = np.abs(want[i, g].astype(np.float64) - s64)
                assert (err <= C_DECODE * U * dmag).all(), (case, b, int(case.K[b]), float((err / dmag).max() / U))
                worst = max(worst, float((err / np.maximum(dmag, 1e-300)).max() / U))
        print(f"{case.name}: worst error {worst:.3f} of the bound")
