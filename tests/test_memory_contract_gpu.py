"""The memory contract of include/irec.h held against every device entry point: a call writes only what its header says, reads
nothing of the workspace that it has not written itself, and modifies no input.  Every call below goes through the C ABI directly
(engine.lib), inside ONE canary arena (tests/guarded.py): float32 / int32 arrays 4 bytes past a 256-byte boundary, int64 arrays 8
bytes past one, outputs pre-filled, workspaces of exactly the bytes the sizing function returned and filled with a hostile pattern,
values compared bit for bit with the referee the entry point's own test uses, arena.check() after torch.cuda.synchronize().

What the encoders read from the workspace, and which kernel of the SAME call writes it first (read off the sources; csrc/ = relative-
entropy-coding_amd/csrc/).  Every wait of a cooperative form gives up after COOP_GIVE_UP_TICKS (irec_kernels.h:187).
  preparation kernel   prep_kernel workgroup 0 zeroes every word of the head's counter block but the table books (irec_prep.hip:165-169),
                       rewrites the keep word, the pending key and -- without a match under IREC_FLAG_REUSE_TABLES -- the stamp of all four
                       slots (:170-182); it READS the stamps (:174, :204), the only words a call takes from its caller.  Workgroups
                       [1, 1 + n_granule) zero both parities of the exchange granules of the call's shared blocks (:186-195; n_granule =
                       split_blocks, irec_host.cpp:1265, set at :925 / :944 / :962), the table workgroups write every row of the tables the
                       block kernel reads (:207-214), the cost workgroups one key per row (:223-227, read at irec_team.hip:136).
  stamps               commit_table_stamps copies the pending key (prep: irec_prep.hip:177) over the stamp in every block kernel's
                       first workgroup (irec_team.hip:116, irec_chunk.h:102, irec_kernels.hip:130 / :414).
  team                 counters: head words zeroed by prep; slab: statistics written at irec_team.hip:269 by the first sample stripe
                       before any wave reads them at :313-315 (team barrier between), parked constants :331-332 before :338-339, back
                       pointers :799 before :962, beams: `if (t)` at :862 -- step 1 reads no beam row, step t reads the parents that step
                       t - 1 wrote at :825.
  team, shared rows    the same, plus the granules of exchange slot row - tsplit_first: published at irec_team.hip:747, swept at :761-764
                       for the tag t + 1 >= 1; zeroed by prep for every shared row (n_blocks - share_first <= COOP_MAX_BLOCKS,
                       irec_host.cpp:803); error flag: head word 3, zeroed by prep.
  ten                  statistics irec_ten.hip:297 before :335-337; beams `if (t)` at :584; back pointers :555 before :686.
  lone                 statistics irec_lone.hip:350 before :93-95 (the same wave); nothing else of the slab.
  one-table / fused    counter and deferred count: head words 0-2, zeroed by prep, read at irec_kernels.hip:417 / :457 / :462;
  fast                 statistics :505 before the step constants read them; beams `if (t)` at :998 / :1089.
  split fast           the same on one slab per workgroup, plus granules: published :869, swept :883-886 for tag t + 1; zeroed by prep
                       for every block of the call (n_blocks <= COOP_SPLIT_MAX_BLOCKS = 64).
  chunk                statistics irec_chunk.h:283 and the cumulative variance of parity 0 at :284 before :368-371; sample scale :384
                       before :635; beams `if (t)` at :654.
  chunk gang           the same, plus the arrival counter = first word of the block's granules (irec_chunk.h:183), zeroed by prep
                       (n_blocks <= GANG_MAX_BLOCKS, irec_chunk_gang.hip:27); the exchange behind the slabs is written by its owners
                       (:288, :546, :554, :596) before the gang barrier (:190-228) behind which it is read (:307, :592, :599).
  generic              counter / deferred count as above (irec_kernels.hip:131, :146, :151); the slab's ten statistic rows are written
                       for every dim of the block's groups at :180-181 before the first step.
So a workspace of any contents serves a call without IREC_FLAG_REUSE_TABLES, and section B's pattern 0x00000001 -- counters that look
advanced, granules that carry the first tag a call waits for -- changes nothing.  No region was found that is read before it is written.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import decode_cases
import guarded as G
import kernel_names as kn
import rec_device_cases as RC
import residual_cases as RES
import rows_status_cases as C
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8
SEED = 42


@pytest.fixture(autouse=True)
def _stop_the_session_on_a_gpu_error():
    """A call that left the device in an error state ends the run: nothing more is started on it."""
    yield
    if torch.cuda.is_available():
        try:
            torch.cuda.synchronize()
        except Exception as e:          # noqa: BLE001
            pytest.exit(f"GPU error after a memory-contract test: {e}", returncode=3)


def _plans(n_cu=256):
    from test_kernel_coverage import _plans as plans      # (one enumeration for both modules)
    return plans(n_cu)


def _names():
    try:
        return sorted(_plans())
    except Exception:        # (the library is missing: tests/test_kernel_coverage.py says so)
        return []


def _stream(engine):
    return engine._stream()


def _refill(view):
    G.Arena._fill(view, G.PREFILL[view.dtype])


def _same(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


class _Layout:
    """The descriptor arrays of an engine layout as `in` regions of an arena."""

    def __init__(self, arena, lay):
        self.base = arena.put(lay.block_base.cpu().numpy(), name="block_base")
        self.pos = arena.put(lay.block_pos.cpu().numpy(), name="block_pos")
        self.dim = arena.put(lay.block_dim.cpu().numpy(), name="block_dim")
        self.perm = arena.put(lay.perm_host.astype(np.int32), name="perm") if lay.perm_host is not None else None
        self.nbytes = 8 * lay.n_blocks * 2 + (4 * lay.n if lay.perm_host is not None else 0)

    def args(self):
        return (self.base.data_ptr(), self.pos.data_ptr(), self.dim.data_ptr())

    def perm_ptr(self):
        return self.perm.data_ptr() if self.perm is not None else None


# ==== the encoders =====================================================================================================================
class _EncodeCall:
    """One irec_beam_encode[_ex] call laid out in an arena: inputs, pre-filled outputs, a workspace of exactly the sized bytes."""

    def __init__(self, engine, lay, host, S, B, flags, max_K, ws_fill, zero_head=False):
        from irec import _lib
        self.engine, self.lay, self.max_K = engine, lay, max_K
        self.margins = bool(flags & _lib.IREC_FLAG_MARGINS)
        self.params = engine.with_table_dims(engine.params(3.0, S, B, flags), lay)
        if lay.max_dim > 1024:
            need = engine.lib.irec_encode_workspace_bytes_for(engine.ctx, ctypes.byref(self.params), lay.n_blocks, lay.max_dim, max_K)
        else:
            need = engine.lib.irec_encode_workspace_bytes(engine.ctx, ctypes.byref(self.params), lay.max_dim, max_K)
        assert need > 0, engine.lib.irec_last_error()
        self.need = need
        n_el = lay.n_tensors * lay.n
        width = max(max_K, 1)
        self.arena = arena = G.Arena(G.slack(16) + need + 20 * n_el + 4 * lay.n + 16 * lay.n_blocks + 4 * lay.n_blocks * (width + 5), "cuda")
        self.d = _Layout(arena, lay)
        self.stats = [arena.put(np.ascontiguousarray(a, dtype=np.float32).reshape(-1), name=nm)
                      for a, nm in zip(host, ("q_loc", "q_scale", "p_loc", "p_scale"))]
        self.out_K = arena.region(I32, (lay.n_blocks,), "out", name="out_K")
        self.out_idx = arena.region(I32, (lay.n_blocks, width), "out", name="out_indices")
        self.sample = arena.region(F32, (n_el,), "out", name="out_sample")
        self.margin = arena.region(F32, (lay.n_blocks, 4), "out", name="out_margin") if self.margins else None
        self.ws = arena.workspace(need, ws_fill)
        if zero_head:                      # the engine's own precondition of IREC_FLAG_REUSE_TABLES
            self.ws[:512].zero_()
        arena.arm()

    def issue(self, extra_flags=0):
        e, lay, p = self.engine, self.lay, self.params
        if extra_flags:
            p = e.params(p.kl_per_partition, p.n_samples, p.n_beams, p.flags | extra_flags, list(p.table_dims), p.table_steps)
        common = (e.ctx, ctypes.byref(p), lay.n_blocks, *self.d.args(), lay.max_dim, self.d.perm_ptr(), *(t.data_ptr() for t in self.stats),
                  SEED, self.max_K, self.out_K.data_ptr(), self.out_idx.data_ptr(), self.sample.data_ptr())
        from irec import _lib
        if self.margins:
            _lib.check(e.lib.irec_beam_encode_ex(*common, self.margin.data_ptr(), self.ws.data_ptr(), self.need, _stream(e)), "irec_beam_encode_ex")
        else:
            _lib.check(e.lib.irec_beam_encode(*common, self.ws.data_ptr(), self.need, _stream(e)), "irec_beam_encode")
        torch.cuda.synchronize()
        self.arena.check()
        return self.out_K.cpu().numpy(), self.out_idx.cpu().numpy(), self.sample.cpu().numpy()

    def refill_outputs(self):
        for t in (self.out_K, self.out_idx, self.sample) + ((self.margin,) if self.margins else ()):
            _refill(t)


@functools.lru_cache(maxsize=None)
def _planner_reference(name, n_cu):
    """The oracle's answer to the planner's cheapest call of a kernel name, computed once for sections A and B."""
    from oracle import oracle as O
    ex = _plans(n_cu)[name]
    host = kn.case_inputs(O, ex)
    ridx, rs, _, rm = O.encode_tensors_omp(*host, SEED, 3.0, ex["S"], ex["B"], ex["dim"], max_K=ex["max_K"], margins=True)
    for a in host + [rs, rm]:
        a.setflags(write=False)
    return host, [r[0] for r in ridx], rs, rm[:, 0]


def _planned_encoder(engine, name, ws_fill):
    from irec import _lib
    n_cu = engine.plan(engine.params(3.0, 36, 20), engine.layout(1, 192, 192, SEED), 8)["n_cu"]
    ex = _plans(n_cu)[name]
    B, S, n_blocks, dim, max_K, flags = ex["B"], ex["S"], ex["n_blocks"], ex["dim"], ex["max_K"], ex["flags"]
    margins = bool(flags & _lib.IREC_FLAG_MARGINS)
    host, ridx, rs, rm = _planner_reference(name, n_cu)
    lay = engine.layout(n_blocks, dim, dim, SEED)                      # one block per tensor, shuffled (coder.py:62-83)
    assert lay.n_blocks == n_blocks and lay.max_dim == dim
    plan = engine.plan(engine.params(3.0, S, B, flags & ~_lib.IREC_FLAG_MARGINS), lay, max_K, margins=margins)
    assert kn.canonical(plan["kernel"], plan["split"]) == name, (plan, ex)
    call = _EncodeCall(engine, lay, host, S, B, flags, max_K, ws_fill)
    Kh, ih, sh = call.issue()
    want_K = np.empty(n_blocks, np.int32)
    rows = [None] * n_blocks
    for i in range(n_blocks):
        want_K[lay.natural[i]], rows[lay.natural[i]] = len(ridx[i]), ridx[i]
    assert np.array_equal(Kh, want_K), (name, Kh.tolist(), want_K.tolist())
    assert Kh.min() >= 0 and Kh.max() <= max_K
    G.expect_rows(ih, Kh, rows)
    assert np.array_equal(sh.reshape(n_blocks, dim), rs), name
    if margins:
        mh = call.margin.cpu().numpy()                                 # exactly [n_blocks][4]: the canary starts behind the last one
        assert np.array_equal(mh[lay.natural], rm), name
    else:
        assert call.margin is None


# ---- A ----
@pytest.mark.parametrize("name", _names())
def test_every_planned_encoder_in_hostile_placement(engine, oracle, name):
    _planned_encoder(engine, name, 0xFFFFFFFF)


def test_one_item_per_compiled_encoder():
    compiled = {k for k in kn.compiled_kernels() if k.startswith("encode_")}
    assert set(_names()) == compiled and len(compiled) >= 60


# ---- B ----
def _family_names():
    try:
        plans = _plans()
    except Exception:
        return []
    return [pytest.param(name, id=kn.family_id(family)) for family, name in kn.family_names(plans)]


@pytest.mark.parametrize("name", _family_names())
def test_stale_tags_and_advanced_counters(engine, oracle, name):
    assert name is not None, "the planner names no kernel of this family"
    _planned_encoder(engine, name, 0x00000001)


# ---- C ----
@functools.lru_cache(maxsize=None)
def _small_call():
    """Nine 192-dim blocks as kernel_names.case_inputs makes them -- which all need K = 2 partitions, so the posteriors of the first
    six are sharpened (q_scale halved: about 0.32 nats more a dim, K = 20 and more): at max_K = 2 six rows are not coded, three are."""
    from oracle import oracle as O
    host = [a.copy() for a in kn.case_inputs(O, {"dim": 192, "n_blocks": 9})]
    host[1][:6] *= np.float32(0.5)
    perm = O.tf_shuffle_perm(SEED, 192)
    K = [O.num_aux(O.block_kl(*(a[i][perm] for a in host)), 3.0) for i in range(9)]
    return host, perm, K


@pytest.mark.parametrize("B,flag", [(20, "default"), (1, "lone"), (20, "generic")])
def test_not_coded_rows_stay_inside_their_row(engine, oracle, B, flag):
    from irec import _lib
    host, perm, K = _small_call()
    max_K = next((m for m in range(2, 64) if sum(k <= m for k in K) >= 1 and sum(k > m for k in K) >= 5), None)
    assert max_K is not None, K
    S = 36
    lay = engine.layout(9, 192, 192, SEED)
    # (a one-beam call of nine blocks takes the split encoder; IREC_FLAG_TEAM, as the planner's own grid has it, sends it to encode_lone_kernel)
    flags = {"generic": _lib.IREC_FLAG_FORCE_GENERIC, "lone": _lib.IREC_FLAG_TEAM}.get(flag, 0)
    kernel = engine.plan(engine.params(3.0, S, B, flags), lay, max_K)["kernel"]
    assert {"lone": kernel.startswith("encode_lone_kernel"), "generic": kernel.startswith("encode_generic_kernel")}.get(flag, True), kernel
    call = _EncodeCall(engine, lay, host, S, B, flags, max_K, 0xFFFFFFFF)
    Kh, ih, sh = call.issue()
    sh = sh.reshape(9, 192)
    rows = [None] * 9
    for i in range(9):
        r = lay.natural[i]
        assert Kh[r] == K[i], (i, Kh[r], K[i])
        if K[i] <= max_K:
            ridx, rs = oracle.encode_block(*(a[i][perm] for a in host), SEED, 3.0, S, B)
            rows[r] = ridx
            want = np.empty(192, np.float32)
            want[perm] = rs
            assert np.array_equal(sh[i], want), i
    assert sum(r is not None for r in rows) >= 1 and sum(r is None for r in rows) >= 5
    G.expect_rows(ih, Kh, rows)            # (nothing outside the rows' max_K slots: the region's canaries, in issue())


# ---- D ----
def test_reuse_tables_on_a_dirty_table_area(engine, oracle):
    from irec import _lib
    stats = oracle.synthetic_latent(0, 8192)
    lay = engine.layout(1, 8192, 1000, SEED)
    ridx, rs = oracle.encode_tensor(*stats, SEED, 3.0, 36, 20, block_size=1000)
    call = _EncodeCall(engine, lay, stats, 36, 20, _lib.IREC_FLAG_REUSE_TABLES, 32, 0xFFFFFFFF, zero_head=True)
    plan = engine.plan(engine.params(3.0, 36, 20, _lib.IREC_FLAG_REUSE_TABLES), lay, 32)
    assert plan["n_tables"] >= 1 and plan["table_steps"] >= 1, plan       # (a call that has tables to keep)
    for extra in (0, _lib.IREC_FLAG_TABLES_PRESENT):
        Kh, ih, sh = call.issue(extra)
        rows = [None] * lay.n_blocks
        for j in range(lay.n_blocks):
            rows[lay.natural[j]] = ridx[j]
        assert Kh.tolist() == [len(r) for r in rows], extra
        G.expect_rows(ih, Kh, rows)
        assert np.array_equal(sh, rs.reshape(-1)), extra
        call.refill_outputs()


# ---- E ----
@pytest.mark.parametrize("with_kl", [True, False])
def test_block_kl(engine, oracle, with_kl):
    from irec import _lib
    n_t, n, bs = 3, 8192, 1000
    stats = [oracle.synthetic_latent(40 + i, n) for i in range(n_t)]
    lay = engine.layout(n_t, n, bs, SEED)
    assert lay.n_blocks == 27 and lay.distinct_dims == [1000, 192]
    arena = G.Arena(G.slack(12) + 16 * n_t * n + 4 * n + 16 * 27 + 8 * 27, "cuda")
    d = _Layout(arena, lay)
    dev = [arena.put(np.stack([s[k] for s in stats]).reshape(-1), name=nm) for k, nm in enumerate(("q_loc", "q_scale", "p_loc", "p_scale"))]
    out_kl = arena.region(F32, (27,), "out", name="out_kl")
    out_K = arena.region(I32, (27,), "out", name="out_K")
    arena.arm()
    params = engine.params(3.0, 36, 20)
    _lib.check(engine.lib.irec_block_kl(engine.ctx, ctypes.byref(params), 27, *d.args(), d.perm_ptr(), *(t.data_ptr() for t in dev),
                                        out_kl.data_ptr() if with_kl else None, out_K.data_ptr(), _stream(engine)), "irec_block_kl")
    torch.cuda.synchronize()
    arena.check()
    kl, K = out_kl.cpu().numpy(), out_K.cpu().numpy()
    perm = oracle.tf_shuffle_perm(SEED, n)
    for t in range(n_t):
        for b, (lo, hi) in enumerate(oracle.split_blocks(n, bs)):
            ref = np.float32(oracle.block_kl(*(s[perm[lo:hi]] for s in stats[t])))
            row = lay.natural[t * lay.blocks_per_tensor + b]
            assert K[row] == oracle.num_aux(ref, 3.0), (t, b)
            if with_kl:
                assert kl[row] == ref, (t, b, kl[row], ref)
    if not with_kl:
        assert (out_kl.view(I32) == G.PREFILL_F32_BITS).all()


# ==== F: the decoders ===================================================================================================================
DEC_S, DEC_B = 36, 20
# tensor dims at block_size 1000 -> the decode_tensor_kernel<TABLE, DEC_RMAX> a whole-tensor call takes (irec_decode.hip:578-612: unit
# slots per tensor upt = blocks x ceil(1000 / 256) = 4 x blocks, waves nw = min(upt, 12), DEC_RMAX_BIG when ceil(upt / nw) > 3, i.e. from
# ten blocks on: 9001 dims; 9004 is the first such size with n % 4 == 0).  8192 and 9004: n % 4 == 0, which NATURAL placement sends down
# the scalar staging passes (vec == false, irec_decode.hip:299-315); 8190: n % 4 != 0.
DEC_LAYOUTS = {8192: 3, 8190: 3, 9004: 5}


@functools.lru_cache(maxsize=None)
def _decode_case(n):
    """Three tensors of n dims in 1000-dim blocks: the oracle's rows (natural order) with three planted rows, and what they decode to."""
    from oracle import oracle as O
    n_t, bs = 3, 1000
    stats = [O.synthetic_latent(700 + i, n) for i in range(n_t)]
    host = [np.stack([s[k] for s in stats]) for k in range(4)]
    ridx, _, _ = O.encode_tensors_omp(*host, SEED, 3.0, DEC_S, DEC_B, bs, max_K=64)
    bpt = len(ridx[0])
    max_K = max(len(r) for t in ridx for r in t) + 2
    K = np.array([len(r) for t in ridx for r in t], dtype=np.int32)
    idx = np.full((n_t * bpt, max_K), 7, dtype=np.int32)             # (live slots overwritten below; the rest is never to be read)
    for b, r in enumerate(r for t in ridx for r in t):
        idx[b, :len(r)] = r
    want = np.stack([O.decode_tensor(host[2][i], host[3][i], ridx[i], SEED, DEC_S, block_size=bs) for i in range(n_t)])
    perm = O.tf_shuffle_perm(SEED, n)
    blocks = O.split_blocks(n, bs)
    planted = [0 * bpt + 1, 1 * bpt + 0, next(b for b in range(2 * bpt, 3 * bpt) if K[b] >= 2)]
    K[planted[0]] = -1
    K[planted[1]] = max_K + 1
    idx[planted[2], K[planted[2]] - 1] = DEC_S
    for b in planted:
        i, (lo, hi) = b // bpt, blocks[b % bpt]
        want[i, perm[lo:hi]] = host[2][i, perm[lo:hi]]               # not decodable: p_loc (include/irec.h)
    for a in (K, idx, want, host[2], host[3]):
        a.setflags(write=False)
    return host[2], host[3], K, idx, want, max_K, bpt


@pytest.mark.parametrize("n", sorted(DEC_LAYOUTS))
def test_decoders(engine, oracle, n):
    from irec import _lib
    lib = engine.lib
    pl_h, ps_h, K_nat, idx_nat, want, max_K, bpt = _decode_case(n)
    n_t, bs = 3, 1000
    lay = engine.layout(n_t, n, bs, SEED)
    n_rows = n_t * bpt
    assert lay.n_blocks == n_rows
    plain = engine.params(3.0, DEC_S, DEC_B)
    hinted = engine.with_table_dims(plain, lay)
    need = lib.irec_decode_workspace_bytes(engine.ctx, ctypes.byref(hinted), max_K)
    assert need > 0 and lib.irec_decode_workspace_bytes(engine.ctx, ctypes.byref(plain), max_K) == 0
    assert lib.irec_decode_tensors_supported(ctypes.byref(plain), n, bs) == 1
    big = n_rows + 7
    arena = G.Arena(G.slack(20) + need + 12 * n_t * n + 4 * n + 16 * n_rows + 12 * big * (max_K + 2) + 4 * n_rows, "cuda")
    d = _Layout(arena, lay)
    pl, ps = arena.put(pl_h.reshape(-1), name="p_loc"), arena.put(ps_h.reshape(-1), name="p_scale")
    K_n, idx_n = arena.put(K_nat, name="K (natural)"), arena.put(idx_nat, name="indices (natural)")
    K_lay, idx_lay = np.empty_like(K_nat), np.empty_like(idx_nat)
    K_lay[lay.natural], idx_lay[lay.natural] = K_nat, idx_nat
    K_l, idx_l = arena.put(K_lay, name="K (layout)"), arena.put(idx_lay, name="indices (layout)")
    rng = np.random.default_rng(n)
    block_row = rng.permutation(big)[:n_rows].astype(np.int32)
    K_big = np.full(big, -3, dtype=np.int32)
    idx_big = np.full((big, max_K), -9, dtype=np.int32)
    K_big[block_row], idx_big[block_row] = K_nat, idx_nat
    K_b, idx_b, br = arena.put(K_big, name="K (larger)"), arena.put(idx_big, name="indices (larger)"), arena.put(block_row, name="block_row")
    out = arena.region(F32, (n_t * n,), "out", name="out_sample")
    ws = arena.workspace(need, 0xFFFFFFFF)
    arena.arm()
    P = lambda t: t.data_ptr() if t is not None else None

    def verify(what):
        torch.cuda.synchronize()
        arena.check()                                                   # canaries; K, indices, p_loc, p_scale, descriptors unchanged
        assert np.array_equal(out.cpu().numpy().reshape(n_t, n), want), (n, what)
        _refill(out)
        G.Arena._fill(ws, 0xFFFFFFFF)

    for params, what in ((plain, "irec_beam_decode"), (hinted, "irec_beam_decode (hints)")):
        _lib.check(lib.irec_beam_decode(engine.ctx, ctypes.byref(params), n_rows, *d.args(), d.perm_ptr(), P(pl), P(ps), SEED, max_K, P(K_l), P(idx_l),
                                        P(out), _stream(engine)), what)
        verify(what)
    for params, w, wb, what in ((hinted, ws, need, "irec_beam_decode_ws (tables)"), (plain, None, 0, "irec_beam_decode_ws (no hints)")):
        _lib.check(lib.irec_beam_decode_ws(engine.ctx, ctypes.byref(params), n_rows, *d.args(), lay.max_dim, d.perm_ptr(), P(pl), P(ps), SEED, max_K,
                                           P(K_l), P(idx_l), P(out), P(w), wb, _stream(engine)), what)
        verify(what)
    for rows, Kt, It, how in ((None, K_n, idx_n, "block_row NULL"), (br, K_b, idx_b, "block_row permuted")):
        for w, wb, tab in ((ws, need, "tables"), (None, 0, "fused")):     # decode_tensor_kernel<true, R> / <false, R>
            what = f"irec_beam_decode_tensors ({how}, {tab})"
            _lib.check(lib.irec_beam_decode_tensors(engine.ctx, ctypes.byref(plain), n_t, n, bs, P(rows), d.perm_ptr(), P(pl), P(ps), SEED, max_K, P(Kt),
                                                    P(It), P(out), P(w), wb, _stream(engine)), what)
            verify(what)


def test_decode_layouts_select_both_staged_builds():
    """The dispatch of irec_decode.hip:578-612 restated: which DEC_RMAX a layout of DEC_LAYOUTS takes."""
    for n, rmax in DEC_LAYOUTS.items():
        upt = -(-n // 1000) * 4
        nw = min(upt, 12)
        assert (3 if -(-upt // nw) <= 3 else 5) == rmax and -(-upt // 12) <= 5, n
        assert decode_cases.staged_rmax(n, 1000) == rmax and decode_cases.tensors_supported(n, 1000)   # (the full restatement of the dispatch)
    assert -(-(-(-9000 // 1000) * 4) // 12) <= 3 < -(-(-(-9001 // 1000) * 4) // 12)      # 9001 dims: the first tensor of the big build


# ==== G: the importance coder ===========================================================================================================
GC_S = 21


@functools.lru_cache(maxsize=64)
def _normal(seed, count):
    from oracle import oracle as O
    return O.tf_random_normal(seed, count)


class _CachedOracle:
    def __init__(self, oracle):
        self._o, self.tf_random_normal = oracle, _normal

    def __getattr__(self, name):
        return getattr(self._o, name)


def _golden_block(name, D=None):
    g = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return [np.ascontiguousarray(g[k][:D], dtype=np.float32) for k in ("q_loc", "q_scale", "p_loc", "p_scale")], float(g["kl_per_partition"]), int(g["seed"])


def _gc_call(engine, oracle, host, omega, seed, block_size, entry, max_K, alpha=None):
    """One call of `entry` over one tensor, then irec_gc_importance_decode over its rows and over a damaged copy of them."""
    import gc_referee as R
    import gc_referee_alpha as RA
    from irec import _lib
    from irec.engine import build_gumbel_table, build_normal_table
    lib = engine.lib
    n = host[0].size
    lay = engine.layout(1, n, block_size, seed)
    dims = lay.distinct_dims
    tabs_h = [build_normal_table(seed, GC_S, dd, max_K) for dd in dims]
    need = lib.irec_gc_encode_workspace_bytes(engine.ctx, lay.n_blocks, max(dims))
    assert (need > 0) == (max(dims) > 1024)
    gum_h = build_gumbel_table(seed, GC_S, max_K) if alpha is not None else None
    arena = G.Arena(G.slack(24) + need + 24 * n + sum(t.nbytes for t in tabs_h) + 4096 + 16 * lay.n_blocks * (max_K + 4), "cuda")
    d = _Layout(arena, lay)
    stats = [arena.put(a, name=nm) for a, nm in zip(host, ("q_loc", "q_scale", "p_loc", "p_scale"))]
    tabs = [arena.put(t.reshape(-1), name=f"normal_table[{dd}]") for t, dd in zip(tabs_h, dims)]
    gum = arena.put(gum_h.reshape(-1), name="gumbel_table") if gum_h is not None else None
    out_K = arena.region(I32, (lay.n_blocks,), "out", name="out_K")
    out_idx = arena.region(I32, (lay.n_blocks, max_K), "out", name="out_indices")
    sample = arena.region(F32, (n,), "out", name="out_sample")
    ws = arena.workspace(need, 0xFFFFFFFF) if need else None
    arena.arm()
    c = _lib.IrecNormalTables()
    for i, (dd, t) in enumerate(zip(dims, tabs)):
        c.table[i], c.dim[i] = t.data_ptr(), dd
    c.n_samples, c.steps = GC_S, max_K
    args = [engine.ctx, lay.n_blocks, *d.args(), d.perm_ptr(), *(t.data_ptr() for t in stats), ctypes.byref(c), float(np.float32(omega)), max_K,
            out_K.data_ptr(), out_idx.data_ptr(), sample.data_ptr()]
    if entry != "irec_gc_importance_encode":
        args += [ws.data_ptr() if ws is not None else None, need]
    if entry == "irec_gc_importance_encode_gumbel":
        g = _lib.IrecGumbelTable()
        g.table, g.n_samples, g.steps, g.alpha = gum.data_ptr(), GC_S, max_K, float(alpha)
        args.append(ctypes.byref(g))
    _lib.check(getattr(lib, entry)(*args, _stream(engine)), entry)
    torch.cuda.synchronize()
    arena.check()
    cached = _CachedOracle(oracle)
    if block_size is not None:
        assert alpha is None
        ridx, rz = R.encode_tensor(*host, seed, GC_S, omega, block_size, cached)
    else:
        K0 = oracle.num_aux(oracle.block_kl(*host), omega)
        i0, rz = R.encode_block(*host, seed, GC_S, K0, _normal) if alpha is None else RA.encode_block(*host, seed, GC_S, K0, _normal, alpha)
        ridx = [i0]
    Kh, ih = out_K.cpu().numpy(), out_idx.cpu().numpy()
    rows = [None] * lay.n_blocks
    for j in range(lay.n_blocks):
        rows[lay.natural[j]] = ridx[j]
    assert [max(int(k), 1) for k in Kh] == [len(r) for r in rows], (Kh.tolist(), rows)
    assert Kh.min() >= 0 and Kh.max() <= max_K
    G.expect_rows(ih, Kh, rows, live=lambda k: max(k, 1))
    assert _same(sample.cpu().numpy(), rz)
    # ---- and back: the rows as they are, then with one row damaged
    z = sample.cpu().numpy().copy()
    K_in, idx_in = arena.put(Kh, name="K"), arena.put(np.where(np.arange(max_K)[None, :] < np.maximum(Kh, 1)[:, None], ih, 0), name="indices")
    bad = idx_in.cpu().numpy().copy()
    bad[0, 0] = GC_S                                                    # an index equal to n_samples: row 0 is not decodable
    idx_bad = arena.put(bad, name="indices (damaged)")
    dec = arena.region(F32, (n,), "out", name="decoded")
    arena.arm()
    at = lay.element_index(np.arange(lay.n_blocks), max(dims))
    for rows_dev, damaged in ((idx_in, False), (idx_bad, True)):
        _lib.check(lib.irec_gc_importance_decode(engine.ctx, lay.n_blocks, *d.args(), d.perm_ptr(), stats[2].data_ptr(), stats[3].data_ptr(),
                                                 ctypes.byref(c), max_K, K_in.data_ptr(), rows_dev.data_ptr(), dec.data_ptr(), _stream(engine)),
                   "irec_gc_importance_decode")
        torch.cuda.synchronize()
        arena.check()
        want = z.copy()
        if damaged:
            e = at[0][at[0] >= 0]
            want[e] = host[2].reshape(-1)[e]
        assert _same(dec.cpu().numpy(), want), damaged
        _refill(dec)


@pytest.mark.parametrize("block", ["block_D1_cfg0", "block_D255_ragged", "block_D1000_cfg0"])
def test_gc_importance_encode_and_decode(engine, oracle, block):
    host, omega, seed = _golden_block(block)
    assert host[0].size in (1, 255, 1000) and GC_S % 16 != 0
    _gc_call(engine, oracle, host, omega, seed, None, "irec_gc_importance_encode", 16)


def test_gc_importance_encode_ws_mixing_a_wide_and_a_narrow_block(engine, oracle):
    host, omega, seed = _golden_block("block_D2500_large", 1028)
    lay = engine.layout(1, 1028, 1025, seed)
    assert lay.distinct_dims == [1025, 3]
    _gc_call(engine, oracle, host, omega, seed, 1025, "irec_gc_importance_encode_ws", 16)


def test_gc_importance_encode_gumbel(engine, oracle):
    host, omega, seed = _golden_block("block_D255_ragged")
    _gc_call(engine, oracle, host, omega, seed, None, "irec_gc_importance_encode_gumbel", 16, alpha=1.0)


# ==== H: the ratio fit ===================================================================================================================
def _fit_cases():
    import test_ratio_fit_host as H
    size = {name: make()[0].size for name, (make, _) in H.CASES.items()}
    small = min(sorted(size), key=lambda k: size[k])
    return {"smallest": lambda: (H.CASES[small][0](), H.CASES[small][1]), "257 rows": lambda: (H.survey_rows(257, 1000, first=300), 3.)}


@pytest.mark.parametrize("which", ["smallest", "257 rows"])
def test_fit_entry_points(engine, which):
    import test_ratio_fit_host as H
    from irec import _lib
    from irec.engine import build_normal_table, fit_aux_ratios_host
    lib = engine.lib
    stats, omega = _fit_cases()[which]()
    n, D = stats[0].shape
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    kl_h, num_h = np.empty(n, np.float32), np.empty(n, np.int32)
    _lib.check(lib.irec_fit_partitions_host(float(np.float32(omega)), n, D, *(vp(np.ascontiguousarray(a)) for a in stats), vp(kl_h), vp(num_h), 0),
               "irec_fit_partitions_host")
    M = int(num_h.max())
    assert M >= 2
    r_h, c_h, it_h = fit_aux_ratios_host(*stats, H.SEED, omega, [1.], [1.])
    table = build_normal_table(H.SEED, n, D, M - 1)
    need = lib.irec_fit_workspace_bytes(n, D)
    assert need > 0
    arena = G.Arena(G.slack(8) + need + 16 * n * D + table.nbytes, "cuda")
    dev = [arena.put(a, name=nm) for a, nm in zip(stats, ("q_loc", "q_scale", "p_loc", "p_scale"))]
    tab = arena.put(table.reshape(-1), name="normal_table")
    ws = arena.workspace(need, 0xFFFFFFFF)
    arena.arm()
    kl, num = np.full(n, np.nan, np.float32), np.full(n, -1, np.int32)
    _lib.check(lib.irec_fit_partitions(engine.ctx, float(np.float32(omega)), n, D, *(t.data_ptr() for t in dev), vp(kl), vp(num), ws.data_ptr(), need,
                                       _stream(engine)), "irec_fit_partitions")
    torch.cuda.synchronize()
    arena.check()
    assert kl.tobytes() == kl_h.tobytes() and np.array_equal(num, num_h)
    G.Arena._fill(ws, 0xFFFFFFFF)
    r, c = np.zeros(M, np.float32), np.zeros(M, np.float32)
    r[0] = c[0] = 1.
    length, iters = ctypes.c_int32(1), np.zeros(M - 1, np.int32)
    params = _lib.IrecFitParams(float(np.float32(omega)), 1e-4, 0.001, 10000)
    _lib.check(lib.irec_fit_aux_ratios(engine.ctx, ctypes.byref(params), n, D, *(t.data_ptr() for t in dev), tab.data_ptr(), M - 1, vp(r), vp(c), M,
                                       ctypes.byref(length), vp(iters), ws.data_ptr(), need, _stream(engine)), "irec_fit_aux_ratios")
    torch.cuda.synchronize()
    arena.check()                                                      # the four statistics and the normal table are unchanged
    assert length.value == M == r_h.size
    assert r.tobytes() == r_h.tobytes() and c.tobytes() == c_h.tobytes() and iters.tolist() == it_h.tolist()


# ==== I: the row check and the histograms ================================================================================================
def test_rows_status_in_the_arena(engine):
    lib = engine.lib
    nonzero = 0
    for case in C.cases():
        base, k_at, ks, i_at, ist = C.buffers(case)
        arena = G.Arena(G.slack(3) + base.nbytes + 8 * case["n_groups"] + 4 * case["K"].size, "cuda")
        rows = arena.put(base, name="K / idx")
        br = arena.put(case["block_row"], name="block_row") if case["block_row"] is not None else None
        status = arena.region(I32, (case["n_groups"],), "scratch", name="status", fill=0)
        status.copy_(torch.from_numpy(case["status0"].copy()))
        arena.arm()
        st = lib.irec_decode_rows_status(case["n_groups"], case["bpg"], br.data_ptr() if br is not None else None, rows.data_ptr() + 4 * k_at, ks,
                                         rows.data_ptr() + 4 * i_at, ist, case["max_K"], case["min_K"], case["k_limit"], C.S, status.data_ptr(),
                                         _stream(engine))
        assert st == 0, lib.irec_last_error()
        torch.cuda.synchronize()
        arena.check()
        want = C.host_status(lib, case)
        assert np.array_equal(status.cpu().numpy(), want), (case["name"], case["plants"])
        nonzero += int((want != 0).sum())
    assert nonzero > 1000


def test_device_histograms_in_the_arena(engine):
    from irec import _lib
    from irec.io import hist_rows
    lib = engine.lib
    rng = np.random.default_rng(9)
    for n, bpr, mk, niv, ncv, hi in ((300, (4, 1, 7), 9, 20, 8, 25), (70, (2,) * 64, 5, 10000, 70, 10050), (1, (1,), 3, 5, 4, 5)):
        T, R = sum(bpr), len(bpr)
        K = rng.integers(-1, mk + 3, (n, T)).astype(np.int32)
        idx = rng.integers(-2, hi, (n, T, mk)).astype(np.int32)
        host = hist_rows(K, idx, bpr, niv, ncv)
        host = hist_rows(K, idx, bpr, niv, ncv, into=host)
        arena = G.Arena(G.slack(8) + 2 * (K.nbytes + idx.nbytes) + 8 * (niv + R * ncv + R + 2), "cuda")
        Kd, Id = arena.put(K, name="K"), arena.put(idx, name="idx")
        both = arena.put(RC.joined(K.reshape(n, 1, T), idx.reshape(n, 1, T, mk)), name="K|idx joined")
        outs = [arena.region(I64, shape, "scratch", name=nm, fill=0)
                for nm, shape in (("index_hist", (niv,)), ("count_hist", (R, ncv)), ("streams", (1 + R,)), ("rejected", (1,)))]
        arena.arm()
        b = np.asarray(bpr, dtype=np.int32)
        for kp, ks, ip, ist in ((Kd.data_ptr(), 1, Id.data_ptr(), mk), (both.data_ptr(), 1 + mk, both.data_ptr() + 4, 1 + mk)):
            _lib.check(lib.irec_rec_hist_rows_device(n, R, b.ctypes.data, mk, kp, ks, ip, ist, niv, ncv, *(o.data_ptr() for o in outs), _stream(engine)),
                       "irec_rec_hist_rows_device")
        torch.cuda.synchronize()
        arena.check()
        assert host.rejected[0] > 0 or n == 1
        for got, want in zip(outs, (host.index, host.counts, host.streams, host.rejected)):
            assert np.array_equal(got.cpu().numpy().view(np.uint64), want)


# ==== J: the workspaces of the .rec / .res device coders =================================================================================
def test_rec_device_workspaces(engine):
    from irec import _lib
    lib = engine.lib
    c = RC.cases()[RC.case_names().index("9x5x9x12_S36")]
    K, idx = c["K"], c["idx"]
    n, R, bpt = K.shape
    mk = idx.shape[3]
    total = int(c["offsets"][-1])
    need = lib.irec_rec_device_workspace_bytes(n, R)
    assert need > 0
    arena = G.Arena(G.slack(16) + 2 * need + 8 * (K.size + idx.size) + 2 * total + 128 * (n + 1), "cuda")
    Kd, Id = arena.put(K, name="K"), arena.put(idx, name="idx")
    out = arena.region(U8, (total,), "out", name="out")
    offsets = arena.region(I64, (n + 1,), "out", name="offsets")
    status = arena.region(I32, (n,), "out", name="status")
    ws = arena.workspace(need, 0xFFFFFFFF)
    arena.arm()
    _lib.check(lib.irec_rec_encode_files_device(c["seed"], c["block_size"], c["max_index"], *c["shape"], n, R, bpt, mk, Kd.data_ptr(), 1, Id.data_ptr(), mk,
                                                out.data_ptr(), total, offsets.data_ptr(), status.data_ptr(), ws.data_ptr(), need, _stream(engine)),
               "irec_rec_encode_files_device")
    torch.cuda.synchronize()
    arena.check()
    assert not status.any() and np.array_equal(offsets.cpu().numpy(), c["offsets"]) and np.array_equal(out.cpu().numpy(), c["blob"])
    blob, off = arena.put(c["blob"], name="bytes"), arena.put(c["offsets"], name="offsets (in)")
    hdr = arena.region(I32, (n, 9), "out", name="headers")
    K2 = arena.region(I32, (n, R, bpt), "out", name="K (decoded)")
    idx2 = arena.region(I32, (n, R, bpt, mk), "out", name="idx (decoded)")
    st2 = arena.region(I32, (n,), "out", name="status (decoded)")
    ws2 = arena.workspace(need, 0xFFFFFFFF, name="workspace (decode)")
    arena.arm()
    _lib.check(lib.irec_rec_decode_files_device(blob.data_ptr(), off.data_ptr(), n, R, bpt, mk, hdr.data_ptr(), K2.data_ptr(), idx2.data_ptr(), st2.data_ptr(),
                                                ws2.data_ptr(), need, _stream(engine)), "irec_rec_decode_files_device")
    torch.cuda.synchronize()
    arena.check()
    assert not st2.any() and np.array_equal(K2.cpu().numpy(), K) and np.array_equal(idx2.cpu().numpy(), c["idx_zeroed"])
    h, w, ch = c["shape"]
    assert (hdr.cpu().numpy().view(np.uint32) == np.array([c["seed"], c["block_size"], c["max_index"], h, w, ch, 0, 0, R], dtype=np.uint32)).all()


def test_res_device_workspaces(engine):
    from irec import _lib
    from irec.io import residual as res
    lib = engine.lib
    cases = RES.make_cases()
    name = min(sorted(cases), key=lambda k: cases[k][0].size)
    pixels, loc, scale, stream_len = cases[name]
    n, ch, h, w = pixels.shape
    ns = -(-(ch * h * w) // stream_len)
    blob_h, off_h = res.encode_residuals(pixels, loc, scale, stream_len)
    total = int(off_h[-1])
    need = lib.irec_res_device_workspace_bytes(n, ns)
    assert need > 0
    arena = G.Arena(G.slack(16) + 2 * need + 16 * pixels.size + 2 * total + 64 * (n + 1), "cuda")
    px, lc = arena.put(pixels, name="pixels"), arena.put(loc, name="loc")
    out = arena.region(U8, (total,), "out", name="out")
    offsets = arena.region(I64, (n + 1,), "out", name="offsets")
    status = arena.region(I32, (n,), "out", name="status")
    ws = arena.workspace(need, 0xFFFFFFFF)
    arena.arm()
    s32 = float(np.float32(scale))
    _lib.check(lib.irec_res_encode_files_device(px.data_ptr(), lc.data_ptr(), s32, n, h, w, ch, stream_len, out.data_ptr(), total, offsets.data_ptr(),
                                                status.data_ptr(), ws.data_ptr(), need, _stream(engine)), "irec_res_encode_files_device")
    torch.cuda.synchronize()
    arena.check()
    assert not status.any() and np.array_equal(offsets.cpu().numpy(), off_h) and np.array_equal(out.cpu().numpy(), blob_h[:total])
    blob, off = arena.put(np.ascontiguousarray(blob_h[:total]), name="bytes"), arena.put(np.ascontiguousarray(off_h, dtype=np.int64), name="offsets (in)")
    back = arena.region(U8, tuple(pixels.shape), "out", name="pixels (decoded)")
    st2 = arena.region(I32, (n,), "out", name="status (decoded)")
    ws2 = arena.workspace(need, 0xFFFFFFFF, name="workspace (decode)")
    arena.arm()
    _lib.check(lib.irec_res_decode_files_device(blob.data_ptr(), off.data_ptr(), lc.data_ptr(), s32, n, h, w, ch, stream_len, back.data_ptr(), st2.data_ptr(),
                                                ws2.data_ptr(), need, _stream(engine)), "irec_res_decode_files_device")
    torch.cuda.synchronize()
    arena.check()
    assert not st2.any() and np.array_equal(back.cpu().numpy(), pixels)
    assert np.array_equal(res.decode_residuals(blob_h, off_h, loc, scale, stream_len), pixels)        # (the host coder's answer)
