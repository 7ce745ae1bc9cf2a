"""Lane swaps of the 168-VGPR builds of the team encoder (csrc/irec_kernels.h, "Lane swaps").

The preparation side picks one 32-bit mask per (table, step, dim group): bit j set = the quads j and j + 32 of the group trade lanes.
The first level of every lane tree adds lanes l and l ^ 32, so no emitted bit may depend on the masks: every test runs the same call
with mask 0 (what a call this small gets by default), with every mask all ones (IREC_FLAG_LANE_SWAPS_ONES) and with the searched masks
(IREC_FLAG_LANE_SWAPS) and wants K, indices and samples bit-identical to each other and to the oracle.

A call has at most four proposal tables (irec_params.table_dims), so the eight block dims {1, 4, 130, 192, 256, 257, 1000, 1024} go
into two calls of four dims each.  Every call has three latents whose blocks need 0, 1 and 9 partitions.  The masks and the tables are
read back from the head of the engine's workspace (irec/_lib.py: WS_SWAP_MASKS_OFFSET, WS_HEAD_BYTES)."""
import functools

import numpy as np
import pytest

import tie_tables as T

OMEGA, SEED, MAX_K = 3.0, 42, 16
DIM_SETS = ((1024, 1000, 257, 256), (192, 130, 4, 1))
TARGET_KL = (0.0, 1.5, 25.5)            # of every block of latent 0, 1, 2: K = 0, 1, 9 at Omega = 3


def _flags():
    from irec import _lib
    return _lib


def _layout(engine, dims):
    """One block of every dim of `dims` per latent, three latents, no shuffle: block j of latent i holds the elements
    [i * n + pos_j, + dims[j]) of the call's tensors."""
    import torch
    from irec.engine import BlockLayout
    n, n_lat = int(sum(dims)), len(TARGET_KL)
    pos = np.concatenate([[0], np.cumsum(dims)[:-1]]).astype(np.int64)
    base = np.repeat(np.arange(n_lat, dtype=np.int64) * n, len(dims))
    lay = object.__new__(BlockLayout)
    lay.n_tensors, lay.n, lay.block_size, lay.seed = n_lat, n, None, SEED
    lay.blocks_per_tensor, lay.n_blocks, lay.max_dim = len(dims), n_lat * len(dims), int(max(dims))
    lay.order = lay.natural = np.arange(lay.n_blocks)
    lay.distinct_dims = sorted(set(int(d) for d in dims), reverse=True)
    lay.block_base = torch.from_numpy(base).to(engine.device)
    lay.block_pos = torch.from_numpy(np.tile(pos, n_lat).astype(np.int32)).to(engine.device)
    lay.block_dim = torch.from_numpy(np.tile(np.asarray(dims), n_lat).astype(np.int32)).to(engine.device)
    lay.perm_host = lay.perm = None
    lay.host_blocks = [(int(b + p), int(d)) for b, p, d in zip(base, np.tile(pos, n_lat), np.tile(np.asarray(dims), n_lat))]
    return lay


@functools.lru_cache(maxsize=None)
def _inputs(dims):
    """(mq, sq, mp, sp) float32 [3 * sum(dims)]: q = p shifted by delta_d sp_d with sum delta^2 / 2 = the latent's target KL per block."""
    rng = np.random.default_rng([int(d) for d in dims] + [11])
    n = int(sum(dims))
    mp = (0.5 * rng.standard_normal(3 * n)).astype(np.float32)
    sp = np.exp(0.1 * rng.standard_normal(3 * n)).astype(np.float32)
    mq, sq = mp.copy(), sp.copy()
    for i, kl in enumerate(TARGET_KL):
        at = i * n
        for d in dims:
            u = rng.uniform(0.5, 1.5, d)
            delta = np.sqrt(2.0 * kl * u / u.sum()) * rng.choice([-1.0, 1.0], d)
            mq[at:at + d] = (mp[at:at + d].astype(np.float64) + delta * sp[at:at + d]).astype(np.float32)
            at += d
    return mq, sq, mp, sp


def _reference(oracle, host, lay, S, B):
    out = []
    for start, d in lay.host_blocks:
        out.append(oracle.encode_block(*(a[start:start + d] for a in host), SEED, OMEGA, S, B, max_K=MAX_K))
    return out


def _call(eng, lay, host, S, B, flags, kernel=None):
    """One encode call -> dict(K, idx, sample, masks [4][SWAP_STEPS][4], tabs [per table: uint16 [K_tab][S][Dp]])."""
    import torch
    L = _flags()
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to(eng.device) for a in host]
    params = eng.params(OMEGA, S, B, flags)
    plan = eng.plan(params, lay, MAX_K)
    if kernel is not None:
        assert plan["kernel"] == kernel, plan
    K, idx, sample = eng.encode_blocks(params, lay, *dev, SEED, MAX_K)
    torch.cuda.synchronize()
    ws = eng._ws[int(torch.cuda.current_stream(eng.device).cuda_stream)]
    masks = ws[L.WS_SWAP_MASKS_OFFSET:L.WS_SWAP_MASKS_OFFSET + 4096].view(torch.int32).cpu().numpy().view(np.uint32).reshape(4, L.SWAP_STEPS, 4)
    tabs, off = [], L.WS_HEAD_BYTES
    for d in lay.distinct_dims:
        dp = (d + 3) // 4 * 4
        nbytes = plan["table_steps"] * S * dp * 2
        tabs.append(ws[off:off + nbytes].view(torch.int16).cpu().numpy().view(np.uint16).reshape(plan["table_steps"], S, dp).astype(np.int64))
        off += (nbytes + 255) // 256 * 256
    return dict(K=K.cpu().numpy(), idx=idx.cpu().numpy(), sample=sample.cpu().numpy(), masks=masks.copy(), tabs=tabs,
                keep=ws[:512].view(torch.int32)[8:12].cpu().tolist(), steps=plan["table_steps"])


def _same_outputs(a, b, lay):
    """K of every block; indices and sample (bit for bit, NaNs included) of every block the call codes (0 <= K <= MAX_K: the others
    are left to a later pass or to the caller, and their output words are not written)"""
    if not np.array_equal(a["K"], b["K"]):
        return False
    for r, ((start, d), k) in enumerate(zip(lay.host_blocks, a["K"])):
        if 0 <= k <= MAX_K:
            if not np.array_equal(a["idx"][r, :k], b["idx"][r, :k]):
                return False
            if a["sample"][start:start + d].tobytes() != b["sample"][start:start + d].tobytes():
                return False
    return True


def _equals_reference(got, ref, lay):
    for r, ((start, d), (idx, sample)) in enumerate(zip(lay.host_blocks, ref)):
        assert got["K"][r] == len(idx), (r, d, got["K"][r], len(idx))
        assert got["idx"][r, :len(idx)].tolist() == idx, (r, d)
        assert got["sample"][start:start + d].tobytes() == np.asarray(sample, dtype=np.float32).tobytes(), (r, d)


def _three_ways(eng, oracle, dims, S, B, base_flags, kernel, host=None):
    """mask 0, all ones, searched: the same outputs, the oracle's; the masks that were asked for are the masks in place."""
    L = _flags()
    lay = _layout(eng, dims)
    host = _inputs(tuple(dims)) if host is None else host
    runs = {name: _call(eng, lay, host, S, B, base_flags | f, kernel)
            for name, f in (("zero", 0), ("ones", L.IREC_FLAG_LANE_SWAPS_ONES), ("searched", L.IREC_FLAG_LANE_SWAPS))}
    steps = min(runs["ones"]["steps"], L.SWAP_STEPS)
    for q, d in enumerate(lay.distinct_dims):
        ng = (d + 255) // 256
        assert (runs["ones"]["masks"][q, :steps, :ng] == 0xFFFFFFFF).all() and (runs["ones"]["masks"][q, :steps, ng:] == 0).all(), d
        assert (runs["searched"]["masks"][q, :steps, ng:] == 0).all(), d
    assert _same_outputs(runs["zero"], runs["ones"], lay), "all-ones masks change the outputs"
    assert _same_outputs(runs["zero"], runs["searched"], lay), "searched masks change the outputs"
    return lay, host, runs


def _team_flags(shape=None):
    L = _flags()
    return L.IREC_FLAG_TEAM | (L.IREC_FLAG_SHAPE[shape] if shape else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", DIM_SETS, ids=lambda d: "D" + "_".join(map(str, d)))
def test_masks_do_not_change_the_outputs(engine, oracle, dims):
    """B = 20, S = 36 on the forced three-team build."""
    lay, host, runs = _three_ways(engine, oracle, dims, 36, 20, _team_flags("3"), "encode_team_kernel<20,3,1>")
    ref = _reference(oracle, host, lay, 36, 20)
    Ks = sorted(set(len(i) for i, _ in ref))
    assert Ks[0] == 0 and 1 in Ks and Ks[-1] >= 8, Ks
    _equals_reference(runs["zero"], ref, lay)
    if max(dims) >= 1000:
        assert runs["searched"]["masks"].any(), "the search moved no quad of a 1000-dim table"


@pytest.mark.gpu
@pytest.mark.parametrize("B,kernel,shape", [(11, "encode_team_kernel<20,3,1>", "3"), (50, "encode_team_kernel<60,1,3>", None)],
                         ids=["B11_partly_filled_stripe", "B50_12_wave_stripes"])
def test_masks_on_other_shapes(engine, oracle, B, kernel, shape):
    dims = (1000, 257, 130, 4)
    lay, host, runs = _three_ways(engine, oracle, dims, 36, B, _team_flags(shape), kernel)
    _equals_reference(runs["zero"], _reference(oracle, host, lay, 36, B), lay)


@pytest.mark.gpu
def test_masks_with_non_finite_input(engine, oracle):
    """A block with a NaN, a +inf and a -inf in q_loc, blocks with one of them each: whatever the call answers for them with mask 0 it
    answers with masks."""
    dims = (1000, 257, 130, 4)
    mq, sq, mp, sp = (a.copy() for a in _inputs(dims))
    n = sum(dims)
    two = 2 * n                                    # latent 2: the blocks of nine partitions
    mq[two + 3], mq[two + 500], mq[two + 999] = np.nan, np.inf, -np.inf
    mq[two + 1000 + 7] = np.inf
    mq[two + 1257 + 100] = -np.inf
    mq[n + 5] = np.nan                             # latent 1, the 1000-dim block
    _three_ways(engine, oracle, dims, 36, 20, _team_flags("3"), "encode_team_kernel<20,3,1>", host=(mq, sq, mp, sp))


@pytest.mark.gpu
def test_masks_under_a_poisoned_quantile_table(engine, oracle):
    """Scores that hold +-inf and (inf - inf) NaN (tie_tables.poisoned_lut): the first level of the lane tree must stay commutative for
    them too.  Same outputs with and without masks, and the oracle's."""
    import irec
    dims = (1000, 257, 130, 4)
    lut = T.poisoned_lut(1000, 0.5, 3)
    eng = irec.Engine(engine.device, lut=lut)
    lay, host, runs = _three_ways(eng, oracle, dims, 36, 20, _team_flags("3"), "encode_team_kernel<20,3,1>")
    with T.oracle_table(oracle, lut):
        ref = _reference(oracle, host, lay, 36, 20)
    _equals_reference(runs["zero"], ref, lay)


@pytest.mark.gpu
def test_masks_are_reused_with_their_tables(engine, oracle):
    """IREC_FLAG_REUSE_TABLES: the second call keeps tables and masks; a call planned on another encoder after it is unaffected, and the
    masked call after that builds both again."""
    import torch
    L = _flags()
    dims = (1000, 257, 130, 4)
    lay, host = _layout(engine, dims), _inputs(dims)
    ref = _reference(oracle, host, lay, 36, 20)
    masked = _team_flags("3") | L.IREC_FLAG_LANE_SWAPS | L.IREC_FLAG_REUSE_TABLES
    engine._ws.pop(int(torch.cuda.current_stream(engine.device).cuda_stream), None)   # a fresh (zero-filled) scratch
    first = _call(engine, lay, host, 36, 20, masked, "encode_team_kernel<20,3,1>")
    second = _call(engine, lay, host, 36, 20, masked, "encode_team_kernel<20,3,1>")
    assert first["keep"] == [0, 0, 0, 0] and second["keep"] == [1, 1, 1, 1]
    steps = min(first["steps"], L.SWAP_STEPS)
    assert np.array_equal(first["masks"][:, :steps], second["masks"][:, :steps]) and first["masks"][:, :steps].any()
    assert all(np.array_equal(a, b) for a, b in zip(first["tabs"], second["tabs"]))
    _equals_reference(first, ref, lay)
    _equals_reference(second, ref, lay)
    other = _call(engine, lay, host, 36, 20, _team_flags("2") | L.IREC_FLAG_REUSE_TABLES, "encode_team_kernel<20,2,1>")
    assert other["keep"] == [0, 0, 0, 0]            # copy bits for the identity grouping: another key
    _equals_reference(other, ref, lay)
    plain = _call(engine, lay, host, 36, 20, _team_flags("3") | L.IREC_FLAG_REUSE_TABLES, "encode_team_kernel<20,3,1>")
    assert plain["keep"] == [1, 1, 1, 1]            # (mask 0 on the three-team build: the tables the two-team build left serve it)
    _equals_reference(plain, ref, lay)
    third = _call(engine, lay, host, 36, 20, masked, "encode_team_kernel<20,3,1>")
    assert third["keep"] == [0, 0, 0, 0] and np.array_equal(third["masks"][:, :steps], first["masks"][:, :steps])
    _equals_reference(third, ref, lay)


def _modelled_cost(tab, dim, masks):
    """sum over a step's S * 4 look-up instructions of L(lanes 0-31) + L(lanes 32-63), L = the busiest bank of the 32-lane group under
    the copy bits in `tab` (0 for a group without quads): int64 [steps][dim groups].  tab [steps][S][Dp], masks [steps][4]."""
    steps, S, dp = tab.shape
    bank = (tab % 32).reshape(steps, S, dp // 4, 4)
    ng = (dim + 255) // 256
    cost = np.zeros((steps, ng), dtype=np.int64)
    for t in range(steps):
        for g in range(ng):
            ql = np.arange(64 * g, min(64 * g + 64, dp // 4)) - 64 * g
            hi = (ql >= 32) ^ (((int(masks[t, g]) >> (ql & 31)) & 1) == 1)
            for h in (False, True):
                sel = bank[t][:, 64 * g + ql[hi == h], :]                  # [S][quads of the group][4 slots]
                if sel.shape[1]:
                    cost[t, g] += (sel[..., None] == np.arange(32)).sum(axis=1).max(axis=-1).sum()
    return cost


@pytest.mark.gpu
def test_searched_masks_never_cost_more_than_the_identity(engine, oracle):
    """A condition on the search, not a measurement: for every (step, dim group) the modelled cost of the searched grouping, counted
    in numpy from the tables and masks the device left, is at most that of the identity grouping."""
    L = _flags()
    dims = (1000, 257, 130, 4)
    lay, host = _layout(engine, dims), _inputs(dims)
    zero = _call(engine, lay, host, 36, 20, _team_flags("3"), "encode_team_kernel<20,3,1>")
    srch = _call(engine, lay, host, 36, 20, _team_flags("3") | L.IREC_FLAG_LANE_SWAPS, "encode_team_kernel<20,3,1>")
    steps = min(srch["steps"], L.SWAP_STEPS)
    for q, d in enumerate(lay.distinct_dims):
        assert np.array_equal(zero["tabs"][q] % 10006, srch["tabs"][q] % 10006), d     # the same draws, other copy bits
        c0 = _modelled_cost(zero["tabs"][q][:steps], d, np.zeros((steps, 4), dtype=np.uint32))
        c1 = _modelled_cost(srch["tabs"][q][:steps], d, srch["masks"][q, :steps])
        print(f"dim {d}: modelled cost identity {int(c0.sum())} searched {int(c1.sum())}")
        assert (c1 <= c0).all(), (d, c0, c1)
