"""CPU suite of the canary arena (tests/guarded.py), no GPU.

  * negative controls: five planted violations of the memory contract, each of which Arena.check() / expect_rows must catch and name.
    Each test first shows that the plant is invisible to a comparison of values alone (the outputs the caller looks at are unchanged),
    then that the helper raises.  With the corresponding check of guarded.py disabled (Arena._guard_damage, Arena._input_damage or
    _tail_damage replaced by a function returning None) each of the five fails: pytest.raises finds nothing raised.
  * the host twins of the device kernels -- irec_test_rows_status_host (csrc/irec_rows_core.h), irec_fit_partitions_host /
    irec_fit_aux_ratios_host, irec_rec_test_core_encode_files / _decode_files (csrc/irec_rec_core.h) -- run over arena memory in
    NATURAL placement, outputs pre-filled, workspaces of exactly the sized bytes: the results are those today's tests expect, no canary
    changes and no input is modified.  The device kernels share these lane functions, so this half of the contract is checked on a
    machine without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import guarded as G
import rec_device_cases as RC
import rows_status_cases as C


# ---- negative controls ---------------------------------------------------------------------------------------------------------
def _arena_with_out():
    arena = G.Arena(64 << 10)
    before = arena.region(torch.float32, (8,), "in", name="x")
    before.copy_(torch.arange(8, dtype=torch.float32))
    out = arena.region(torch.int32, (5, 3), "out", name="out_idx")
    arena.arm()
    arena.check()
    return arena, before, out


def _raw(arena, region_view, byte_offset):
    """The arena byte at `byte_offset` relative to the start of the region (negative: before it)."""
    at = region_view.data_ptr() - arena.base + byte_offset
    return arena.buf[at:at + 1]


def test_placement_and_prefill():
    arena = G.Arena(G.slack(5) + 4096)
    f = arena.region(torch.float32, (7,), "out")
    i = arena.region(torch.int32, (2, 3), "out")
    q = arena.region(torch.int64, (3,), "in")
    b = arena.region(torch.uint8, (5,), "out")
    w = arena.workspace(1023, 0xFFFFFFFF)
    assert [t.data_ptr() % 256 for t in (f, i, q, b, w)] == [4, 4, 8, 0, 0] and f.data_ptr() % 16 == 4
    assert all(t.is_contiguous() for t in (f, i, q, b, w)) and w.numel() == 1023
    assert (f.view(torch.int32) == 0x7FC5A5A5).all() and torch.isnan(f).all()
    assert (i == 0x5A5A5A5A).all() and (b == 0xAB).all() and (w == 0xFF).all()
    offs = sorted((r.offset, r.nbytes) for r in arena.regions)
    assert offs[0][0] >= G.GUARD_BYTES and arena.buf.numel() - (offs[-1][0] + offs[-1][1]) >= G.GUARD_BYTES
    for (a, n), (c, _) in zip(offs, offs[1:]):
        assert c - (a + n) >= G.GUARD_BYTES
    one = arena.region(torch.int32, (4,), "scratch", fill=0x00000001)
    assert (one == 1).all()
    q.zero_()
    arena.arm()
    arena.check()


def test_a_byte_one_past_an_output_is_caught():
    arena, _, out = _arena_with_out()
    image = out.clone()
    _raw(arena, out, out.numel() * 4)[0] = 0x11
    assert torch.equal(out, image)                       # nothing the caller compares has changed
    with pytest.raises(AssertionError, match=r"'out_idx'.*1 byte\(s\) past the end of 'out_idx' \(byte offset 60 of the region\)"):
        arena.check()


def test_a_byte_one_before_an_output_is_caught():
    arena, _, out = _arena_with_out()
    image = out.clone()
    _raw(arena, out, -1)[0] = 0
    assert torch.equal(out, image)
    with pytest.raises(AssertionError, match=r"1 byte\(s\) before 'out_idx' \(byte offset -1 of the region\)"):
        arena.check()


def test_an_input_changed_to_an_equal_float_of_other_bytes_is_caught():
    arena, x, _ = _arena_with_out()
    image = x.clone()
    assert x[0] == 0.0
    x[0] = -0.0
    assert torch.equal(x, image)                         # equal as floats
    with pytest.raises(AssertionError, match=r"input 'x' was modified: first at byte offset 3"):
        arena.check()


def test_a_store_into_slot_K_of_a_coded_row_is_caught():
    arena, _, out = _arena_with_out()
    K = np.array([2, 0, 3, 5, -1], dtype=np.int32)       # rows 3 (K > max_K) and 4 (K < 0) are not coded: exempt
    want = [[7, 8], [], [1, 2, 3], None, None]
    out[0, :2] = torch.tensor([7, 8], dtype=torch.int32)
    out[2] = torch.tensor([1, 2, 3], dtype=torch.int32)
    out[3] = 99                                          # a not-coded row may hold anything inside itself
    G.expect_rows(out, K, want)
    arena.check()
    out[0, 2] = 0                                        # idx[row 0, K]
    assert out[0, :2].tolist() == want[0]                # the comparison of [:K] alone still passes
    with pytest.raises(AssertionError, match=r"row 0: slot 2 past the row's 2 entries was written"):
        G.expect_rows(out, K, want)
    out[0, 2] = G.PREFILL_I32
    out[1, 0] = 5                                        # K = 0: the whole row is "rest"
    with pytest.raises(AssertionError, match=r"row 1: slot 0 past the row's 0 entries"):
        G.expect_rows(out, K, want)
    G.expect_rows(out, K, [[7, 8], [5], [1, 2, 3], None, None], live=lambda k: max(k, 1))     # (the importance coder's max(K, 1))
    arena.check()                                        # inside the region: no canary's business


def test_a_workspace_one_byte_short_is_caught():
    need = 1000

    def callee(ptr):                                     # writes every byte it was promised, and nothing else
        ctypes.memset(ptr, 0, need)

    arena = G.Arena(G.slack(1) + need)
    ws = arena.workspace(need, 0xFFFFFFFF)
    callee(ws.data_ptr())
    arena.check()
    arena = G.Arena(G.slack(1) + need)
    ws = arena.workspace(need - 1, 0xFFFFFFFF)
    callee(ws.data_ptr())
    assert not ws.any()
    with pytest.raises(AssertionError, match=r"guard after 'workspace'.*1 byte\(s\) past the end of 'workspace' \(byte offset 999 of the region\)"):
        arena.check()


# ---- host twins under the arena --------------------------------------------------------------------------------------------------
def _referee_rows_status():
    import test_rows_status_host as T
    return T.referee


@pytest.mark.parametrize("which", range(0, len(C.cases()), 8))
def test_rows_status_host_twin_under_the_arena(which):
    import irec
    lib = irec._lib.load()
    referee = _referee_rows_status()
    for case in C.cases()[which:which + 8]:
        base, k_at, ks, i_at, ist = C.buffers(case)
        arena = G.Arena(G.slack(3) + base.nbytes + 8 * case["n_groups"] + 4 * case["K"].size)
        rows = arena.put(base, "in", name="K/idx")
        br = arena.put(case["block_row"], "in", name="block_row") if case["block_row"] is not None else None
        status = arena.region(torch.int32, (case["n_groups"],), "scratch", name="status", fill=0)
        status.copy_(torch.from_numpy(case["status0"].copy()))
        arena.arm()
        st = lib.irec_test_rows_status_host(case["n_groups"], case["bpg"], br.data_ptr() if br is not None else None, rows.data_ptr() + 4 * k_at, ks,
                                            rows.data_ptr() + 4 * i_at, ist, case["max_K"], case["min_K"], case["k_limit"], C.S, status.data_ptr())
        assert st == 0, lib.irec_last_error()
        assert np.array_equal(status.numpy(), referee(case)), case["name"]
        arena.check()


def _smallest_fit_case():
    import test_ratio_fit_host as T
    size = {}
    for name, (make, omega) in T.CASES.items():
        size[name] = make()[0].size
    name = min(sorted(size), key=lambda n: size[n])
    make, omega = T.CASES[name]
    return T, name, make(), omega


def test_fit_host_twins_under_the_arena():
    import irec
    from irec import _lib
    from irec.engine import build_normal_table
    lib = _lib.load()
    T, name, stats, omega = _smallest_fit_case()
    n, D = stats[0].shape
    ref = T.referee_fit(stats, omega)
    M = ref["ratios"].size
    assert M >= 2, name                                  # (a case that fits at least one ratio: the table is read)
    table = build_normal_table(T.SEED, n, D, M - 1)
    need = lib.irec_fit_workspace_bytes(n, D)
    assert need
    arena = G.Arena(G.slack(12) + 4 * (4 * n * D + table.size + 2 * n + 3 * M) + need)
    ins = [arena.put(a, "in", name=nm) for a, nm in zip(stats, ("q_loc", "q_scale", "p_loc", "p_scale"))]
    tab = arena.put(table, "in", name="normal_table")
    out_kl = arena.region(torch.float32, (n,), "out", name="out_kl")
    out_num = arena.region(torch.int32, (n,), "out", name="out_num")
    ratios = arena.region(torch.float32, (M,), "scratch", name="ratios", fill=0)
    counts = arena.region(torch.float32, (M,), "scratch", name="average_counts", fill=0)
    iters = arena.region(torch.int32, (M - 1,), "out", name="out_iters")
    ws = arena.workspace(need, 0xFFFFFFFF)
    ratios[0], counts[0] = 1., 1.
    arena.arm()
    _lib.check(lib.irec_fit_partitions_host(float(np.float32(omega)), n, D, *(t.data_ptr() for t in ins), out_kl.data_ptr(), out_num.data_ptr(), 1),
               "irec_fit_partitions_host")
    arena.check()
    import ratio_fit_referee as R
    kl, num = R.partition_counts(*stats, omega)
    assert np.array_equal(out_num.numpy(), num) and np.allclose(out_kl.numpy(), kl, rtol=1e-6) and int(num.max()) == M
    length = ctypes.c_int32(1)
    params = _lib.IrecFitParams(float(np.float32(omega)), 1e-4, 0.001, 10000)
    _lib.check(lib.irec_fit_aux_ratios_host(ctypes.byref(params), n, D, *(t.data_ptr() for t in ins), tab.data_ptr(), M - 1, ratios.data_ptr(),
                                            counts.data_ptr(), M, ctypes.byref(length), iters.data_ptr(), ws.data_ptr(), need, 1),
               "irec_fit_aux_ratios_host")
    arena.check()
    assert length.value == M
    assert np.array_equal(counts.numpy(), ref["counts"]) and iters.numpy().tolist() == ref["iters"]
    delta = float(np.max(np.abs(ratios.numpy().astype(np.float64) - ref["ratios"].astype(np.float64))))
    assert delta <= T.RATIO_TOL, (name, delta)


def test_rec_core_host_twins_under_the_arena():
    from irec import _lib
    lib = _lib.load()
    c = RC.cases()[RC.case_names().index("9x5x9x12_S36")]
    K, idx = c["K"], c["idx"]
    n, R, bpt = K.shape
    mk = idx.shape[3]
    total = int(c["offsets"][-1])
    arena = G.Arena(G.slack(12) + 8 * (K.size + idx.size) + 2 * total + 16 * (n + 1) + 8 * n + 36 * n)
    Kr, Ir = arena.put(K, "in", name="K"), arena.put(idx, "in", name="idx")
    out = arena.region(torch.uint8, (total,), "out", name="out")              # exactly enough: cap = the files' bytes
    offsets = arena.region(torch.int64, (n + 1,), "out", name="offsets")
    status = arena.region(torch.int32, (n,), "out", name="status")
    arena.arm()
    st = lib.irec_rec_test_core_encode_files(c["seed"], c["block_size"], c["max_index"], *c["shape"], n, R, bpt, mk, Kr.data_ptr(), 1, Ir.data_ptr(), mk,
                                             out.data_ptr(), total, offsets.data_ptr(), status.data_ptr())
    assert st == 0, lib.irec_last_error()
    arena.check()
    assert not status.any() and np.array_equal(offsets.numpy(), c["offsets"]) and np.array_equal(out.numpy(), c["blob"])
    # and back, from the bytes just written
    hdr = arena.region(torch.int32, (n, 9), "out", name="headers")
    K2 = arena.region(torch.int32, (n, R, bpt), "out", name="K2")
    idx2 = arena.region(torch.int32, (n, R, bpt, mk), "out", name="idx2")
    st2 = arena.region(torch.int32, (n,), "out", name="status2")
    blob, off = arena.put(c["blob"], "in", name="bytes"), arena.put(c["offsets"], "in", name="offsets_in")
    arena.arm()
    st = lib.irec_rec_test_core_decode_files(blob.data_ptr(), off.data_ptr(), n, R, bpt, mk, hdr.data_ptr(), K2.data_ptr(), idx2.data_ptr(), st2.data_ptr())
    assert st == 0, lib.irec_last_error()
    arena.check()
    assert not st2.any() and np.array_equal(K2.numpy(), K) and np.array_equal(idx2.numpy(), c["idx_zeroed"])
    h, w, ch = c["shape"]
    assert (hdr.numpy().view(np.uint32) == np.array([c["seed"], c["block_size"], c["max_index"], h, w, ch, 0, 0, R], dtype=np.uint32)).all()
