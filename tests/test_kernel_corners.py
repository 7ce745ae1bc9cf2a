"""Every planned encoder at the edges of the range of calls it serves.

An encoder instantiation is one template build that serves a range of calls: encode_team_kernel<20,3,1,...> takes 11 to 20 beams, 2 to 38
samples, 1 to 1024 dims and 1 to 2304 blocks.  tests/test_kernel_coverage.py and tests/test_f64_referee.py prove each of the 68 names
reachable and run each ONCE, on the cheapest call of the planner grid: for 33 names a call of one sample, for all of them the fewest beams
of the bucket, 192 or 2048 dims, two partitions.  The beam slots only that build has, the last partial wave of samples, a last chunk of
one dim, a block count past the team slots are never occupied there.  Here every name runs on up to four calls from the corners of its
range (tests/kernel_names.py: enumerate_ranges, corner_cases):

  full    the largest B of the range (the full build: 10, 20, 30, 32, 40, 50, 54 or 60 beams), at the largest dim (1024; 5000 for the
          chunk builds), the fewest blocks and the largest S that fits the budget;
  small   the smallest B that still rejects, the smallest rejecting S, the smallest dim (1; 1025), the fewest blocks;
  wide    the largest S of the range, at a ragged dim (1023; 2049: a last chunk of one dim; 257 or 65 where 1023 does not fit);
  blocks  the smallest block count beyond the call's team slots (257, 513 or 2304) at the smallest dim; the shared-row builds: the far
          end of their window (256, 342, 512); the gang and split builds, which never run out of slots: their largest count that fits.

Every call has S >= 2 and rejects a candidate by its second step.  Omega is per call, the first of kernel_names.OMEGAS at which the blocks
have 4 to 16 partitions (engine.params takes S explicitly), so that several steps run with B_cur = B; blocks of one dim come from
tests/latent_families.py (sharp, mixed).  A call costs sum S * D * (1 + (K - 1) * B) proposal evaluations, at most kernel_names.BUDGET =
4e8 (scripts/soak_parity.py's per-block cap) -- with one exception, OVER_BUDGET_BLOCKS below.

Left out or beyond the budget, as literals that the host tests assert:
  DROPPED_S       largest-S corners no call of which fits the budget: none.  The largest S of every range fits at SOME dim of it (8103
                  samples at 257 or 65 dims for the team builds, at 1023 dims for one to five beams); test_reference_sweep_grid
                  (tests/test_gpu_parity.py) runs S = 8103 at its own shapes as well.
  OVER_BUDGET_BLOCKS  the `blocks` corner of 13 one-team chunk builds of 20 to 60 beam slots.  Their calls of more blocks than team
                  slots start at 257 blocks of 1025 dims: none fits 4e8, the ceiling and the covering rule cannot both hold, and the
                  corner is what these tests are for -- a team's second block after a block with a full beam state; no other test runs
                  one (the soak stops at 8 blocks a call).  They run at the largest B and its smallest rejecting S, 0.8e9 to 6.1e9
                  evaluations (kernel_names.BUDGET_BLOCKS = 8e9): spread over the oracle's 16 threads on the GPU machine, up to 3 s.
                  The host test traces 16 blocks of a call either way.
  KNOWN_UNMET     conditions of part 2 that a name meets on none of the eight input seeds (see there).

1 (both suites)  the calls cover the ranges, and each plans to its name at 256 CUs: test_corner_calls_cover_the_ranges.
2 (both suites)  the calls decide something -- conditions the ORACLE's traces (up to 16 blocks a call) must meet over a name's calls:
                 a non-zero index and a block of four partitions; an emitted path that descends, after the first step, from a beam slot
                 only this build has; an emitted index in the last wave of samples; and the proof of power: the oracle that never
                 selects a child of beam slot B - 1 (oracle.set_masked_slot; numpy over the traced scores says which blocks to code
                 again) emits other indices or another sample in at least one call.  Where seed 7 leaves a condition unmet the inputs
                 of a call come from one of the seeds 8 .. 14 (CORNER_SEEDS).
3 (GPU)          every corner call: the plan names the kernel; K, indices, samples (and margins) equal the oracle's bit for bit; decode
                 returns the sample; the first block's path of one call passes the float64 referee.

Measured.  Host tests (one CPU thread): 144 s in all -- 22 s for the covering test, whose range enumeration the others share, at most
5.2 s a name (encode_lone_kernel).  GPU tests on an MI355X: 47 s for the 68 names, at most 1.9 s a name after the first (8.2 s: it
also pays for the module's first use of the engine).  Every GPU comparison held: no kernel or planner change came out of this.

Findings.  ties_to_higher (oracle.set_wrong_order) changes a traced block of 12 of the 272 corner calls (10 names), all of them calls of
one-dim blocks from the families: synthetic_latent's scores do not tie where it matters (tests/test_tie_breaking.py is the test of
that).  The masked slot is the sharper result: with 50 beams or more and at most 80 samples a coder that never reads its last beam
slot emits the same output on nearly every block -- KNOWN_UNMET lists the two names no seed exposes."""
import functools
import re

import numpy as np
import pytest

import kernel_names as kn
import tie_tables as T

SEED = kn.SEED
N_TRACE = 16
# (name, first role) -> the input seed of that corner call where the first seed, 7, leaves a condition of the name unmet
CORNER_SEEDS = {("encode_chunk_kernel<10,10,1,false>", "wide"): 8, ("encode_chunk_kernel<10,10,2,false>", "wide"): 13,
                ("encode_chunk_kernel<20,10,1,true>", "wide"): 11, ("encode_chunk_kernel<20,10,3,false>", "wide"): 9,
                ("encode_chunk_kernel<20,10,3,true>", "wide"): 9, ("encode_chunk_kernel<30,10,1,false>", "wide"): 12,
                ("encode_chunk_kernel<30,10,1,true>", "wide"): 12, ("encode_chunk_kernel<30,10,3,false>", "wide"): 13,
                ("encode_chunk_kernel<30,10,3,true>", "wide"): 13, ("encode_chunk_kernel<32,16,1,false>", "wide"): 9,
                ("encode_chunk_kernel<32,16,1,true>", "wide"): 9, ("encode_chunk_kernel<32,16,2,false>", "blocks"): 9,
                ("encode_chunk_kernel<32,16,2,false>", "wide"): 11, ("encode_chunk_kernel<40,10,1,false>", "blocks"): 10,
                ("encode_chunk_kernel<50,10,1,false>", "blocks"): 10, ("encode_chunk_kernel<50,10,2,false>", "blocks"): 11,
                ("encode_chunk_kernel<60,10,1,false>", "full"): 8, ("encode_chunk_kernel<60,10,1,true>", "blocks"): 10,
                ("encode_chunk_kernel<60,10,1,true>", "small"): 11, ("encode_chunk_kernel<60,10,2,false>", "small"): 11,
                ("encode_chunk_kernel<60,10,2,false>", "wide"): 14}
# name -> the conditions its calls meet on none of the seeds 7 .. 14: findings, asserted as they stand.  `masked`: the oracle that never
# selects a child of beam slot B - 1 emits the same indices and samples on every traced block of every call of the name -- 50 to 60 beams
# and at most 80 samples: the last slot holds the worst beam kept, and its few children almost never carry the path that wins (measured
# on 64 blocks of 1025 dims: 0 blocks change at B = 60, S = 20, 3 at B = 20, S = 54, 11 at B = 10, S = 80).  A kernel that lost its last
# slot would pass test_corner_calls_match_the_oracle for these names; their emitted paths do pass a slot only the build has (`slot`),
# which is the weaker evidence.
KNOWN_UNMET = {"encode_chunk_kernel<50,10,1,true>": {"masked"}, "encode_chunk_kernel<60,10,1,false>": {"masked"}}
DROPPED_S = []
# name -> (B, S, dim, blocks, evaluations in units of 1e8) of its `blocks` corner where that call exceeds BUDGET (see the docstring)
OVER_BUDGET_BLOCKS = {"encode_chunk_kernel<20,10,1,false>": (20, 54, 1025, 257, 20), "encode_chunk_kernel<20,10,3,false>": (20, 7, 1025, 2304, 24),
                      "encode_chunk_kernel<30,10,1,false>": (30, 80, 1025, 257, 45), "encode_chunk_kernel<30,10,2,false>": (30, 54, 1025, 513, 61),
                      "encode_chunk_kernel<30,10,3,false>": (30, 7, 1025, 2304, 35), "encode_chunk_kernel<32,16,1,false>": (32, 54, 1025, 257, 33),
                      "encode_chunk_kernel<32,16,2,false>": (32, 7, 1025, 513, 8), "encode_chunk_kernel<40,10,1,false>": (40, 54, 1025, 257, 41),
                      "encode_chunk_kernel<40,10,2,false>": (40, 7, 1025, 513, 11), "encode_chunk_kernel<50,10,1,false>": (50, 54, 1025, 257, 51),
                      "encode_chunk_kernel<50,10,2,false>": (50, 20, 1025, 513, 37), "encode_chunk_kernel<60,10,1,false>": (60, 38, 1025, 257, 43),
                      "encode_chunk_kernel<60,10,2,false>": (60, 20, 1025, 513, 45)}
# The referee (f64_referee.rescore) makes about 25 float64 passes over the [S, B_cur, D] candidates of a step where the oracle makes one
# (counted from its array expressions, not timed: it decides only WHICH call the referee reads, never whether a comparison holds)
REFEREE_PASSES = 25


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle import oracle as O
    O.lib()
    return O


@functools.lru_cache(maxsize=None)
def _cases(n_cu=256):
    """kernel_names.corner_cases with the committed seeds: (name -> calls, dropped S corners, names whose blocks corner exceeds BUDGET)."""
    cases, dropped_S, over_budget = kn.corner_cases(n_cu)
    cases = {name: [dict(c, seed=CORNER_SEEDS.get((name, c["roles"][0]), 7)) for c in calls] for name, calls in cases.items()}
    return cases, dropped_S, over_budget


@functools.lru_cache(maxsize=None)
def _names():
    try:
        return sorted(kn.enumerate_plans(256))
    except Exception:        # (the library is missing: tests/test_kernel_coverage.py says so)
        return []


def _words(c):
    return (f"{'+'.join(c['roles']):12s} B={c['B']:3d} S={c['S']:4d} D={c['dim']:4d} blocks={c['n_blocks']:4d} flags={c['flags']:#x} "
            f"Omega={c['omega']} {c['source']} seed={c['seed']} cost={c['cost']:.1e}")


def slot_threshold(name, b_max):
    """The first beam slot only this build has: the slot count of the next smaller build of its family; builds without one (the
    10-slot builds, the generic kernel): B / 2.  None for one-beam builds."""
    if b_max < 2:
        return None
    m = re.match(r"encode_(team|chunk|fast)_kernel<(\d+),", name)
    if m:
        smaller = [int(n.split("<")[1].split(",")[0]) for n in _names() if n.startswith(f"encode_{m.group(1)}_kernel<")]
        smaller = [n for n in smaller if n < int(m.group(2))]
        if smaller:
            return max(smaller)
    return b_max // 2


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
def test_corner_calls_cover_the_ranges():
    ranges = kn.enumerate_ranges(256)
    compiled = {k for k in kn.compiled_kernels() if k.startswith("encode_")}
    assert set(ranges) == compiled and len(compiled) == 68, "the finer grid names other kernels than the library holds"
    cases, dropped_S, over_budget = _cases()
    over_calls = {name: next((c["B"], c["S"], c["dim"], c["n_blocks"], round(c["cost"] / 1e8)) for c in cases[name] if "blocks" in c["roles"])
                  for name in over_budget}
    assert dropped_S == DROPPED_S and over_calls == OVER_BUDGET_BLOCKS, (dropped_S, over_calls)
    assert set(cases) == compiled
    bad = []
    for name in sorted(cases):
        calls, rng = cases[name], kn.range_calls(ranges[name])
        if not 3 <= len(calls) <= 4 or sum(c["cost"] > kn.BUDGET for c in calls) != (name in OVER_BUDGET_BLOCKS):
            bad.append((name, "calls", len(calls)))
        for c in calls:
            key = (c["B"], c["S"], c["dim"], c["n_blocks"])
            assert key in rng and c["S"] >= 2 and kn.rejects_by_step_two(c["B"], c["S"]), (name, c)
            assert c["cost"] <= (kn.BUDGET_BLOCKS if name in OVER_BUDGET_BLOCKS and "blocks" in c["roles"] else kn.BUDGET), (name, c)
            # (the planner does not read Omega today; the call's own is passed all the same)
            assert kn.plan_name(256, c["B"], c["S"], c["dim"], c["max_K"], c["n_blocks"], c["flags"], c["omega"])[0] == name, (name, c)
            Ks = kn.call_stats(_oracle(), c["dim"], c["n_blocks"])[2]
            assert 3 * int(((Ks >= 4) & (Ks <= 16)).sum()) >= len(Ks) and Ks.max() <= c["max_K"], (name, c)
            if c["source"] == "synthetic":        # every block of a synthetic call has 4 to 16 partitions: the strict rule
                assert Ks.min() >= 4 and Ks.max() <= 16, (name, c, int(Ks.min()), int(Ks.max()))
        col = lambda j: {k[j] for k in rng}
        have = lambda j: {(c["B"], c["S"], c["dim"], c["n_blocks"])[j] for c in calls}
        fitting_S = max(S for S in col(1) if (name, S) not in DROPPED_S)
        want = {"largest B": max(col(0)) in have(0), "smallest rejecting B": min(col(0)) in have(0),
                "smallest rejecting S": min(col(1)) in have(1), "largest S that fits": fitting_S in have(1),
                "largest dim": max(col(2)) in have(2), "smallest dim": min(col(2)) in have(2), "fewest blocks": min(col(3)) in have(3),
                "a dim that is no multiple of 64": any(kn.rank_of_dim(d) for d in have(2))}
        if min(col(1)) <= 64 < max(col(1)):
            want["a partial last wave of samples"] = any(S > 64 and S % 64 for S in have(1))
        if name.startswith("encode_chunk_kernel"):
            want["a ragged last chunk"] = any(d % kn.CHUNK for d in have(2))
            want["a last chunk of one dim"] = 2049 in have(2)
        if kn.is_shared(name):
            want["both ends of the block window"] = {min(col(3)), max(col(3))} <= have(3)
        elif any(over for _, over in rng.values()):
            want["more blocks than team slots"] = any(rng[(c["B"], c["S"], c["dim"], c["n_blocks"])][1] for c in calls)
        bad += [(name, what) for what, ok in want.items() if not ok]
    assert not bad, bad


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def _facts(call, idx, smp, tr):
    """What one traced block shows: K; a non-zero index; the highest parent slot on the emitted path after the first step; an emitted
    index in the last wave of samples (S <= 64: sample S - 1); through: the emitted path passes beam slot B - 1; moved: steps whose
    selected set changes when the children of slot B - 1 are masked out of the traced scores; ties: steps with two equal scores among
    the best B_new + 1."""
    S, B = call["S"], call["B"]
    K, sel = tr["K"], tr["sel"]
    path, slot = [], 0                                     # (t, s, parent slot) of the emitted path, last step first
    for t in range(K - 1, -1, -1):
        s, b = (int(v) for v in sel[t][slot])
        assert s == idx[t], "the trace's beam 0 is not the emitted path"
        path.append((t, s, b))
        slot = b
    last = 64 * ((S - 1) // 64) if S > 64 else S - 1
    out = dict(K=K, idx=idx, smp=smp, nonzero=any(idx), parent=max([b for t, s, b in path if t >= 1], default=-1),
               wave=any(s >= last for t, s, b in path), through=any(b == B - 1 and t >= 1 for t, s, b in path), moved=0, ties=0)
    for t, N, Bnew, sc in T.steps_of(tr, S, B):
        Bcur = N // S
        order = T.rank(sc)
        assert order[:Bnew].tolist() == [int(s) * Bcur + int(b) for s, b in sel[t][:Bnew]], "numpy's top-B is not the oracle's"
        top = sc[order[:Bnew + 1]]
        out["ties"] += bool((top[:-1] == top[1:]).any())
        if t >= 1 and Bcur == B and N - S >= Bnew:
            keep = order[order % Bcur != B - 1][:Bnew]          # the selection without the children of slot B - 1
            out["moved"] += set(keep.tolist()) != set(order[:Bnew].tolist())
    return out


def _blocks(c):
    """The first N_TRACE blocks of a corner call as the coder sees them: permuted (coder.py:62-83)."""
    O = _oracle()
    host = kn.corner_inputs(O, c)
    perm = O.tf_shuffle_perm(SEED, c["dim"])
    return [tuple(a[i][perm] for a in host) for i in range(min(c["n_blocks"], N_TRACE))]


@functools.lru_cache(maxsize=None)
def _traced(name, k):
    """(facts of the first N_TRACE blocks, blocks whose output ties_to_higher changes) of corner call k of a name."""
    O = _oracle()
    c = _cases()[0][name][k]
    facts, wrong = [], 0
    for bl in _blocks(c):
        idx, smp, tr = O.encode_block(*bl, SEED, c["omega"], c["S"], c["B"], max_K=c["max_K"], trace=True)
        facts.append(_facts(c, idx, smp, tr))
        if facts[-1]["ties"]:             # (without two equal scores among the best B_new + 1 of some step the tie rule decides nothing)
            O.set_wrong_order(ties_to_higher=True)
            try:
                idx1, smp1 = O.encode_block(*bl, SEED, c["omega"], c["S"], c["B"], max_K=c["max_K"])
            finally:
                O.set_wrong_order()
            wrong += idx1 != idx or not np.array_equal(smp1, smp)
    return facts, wrong


def _masked_slot_changes(name, k):
    """The proof of power of corner call k: the oracle that never selects a child of beam slot B - 1 (oracle.set_masked_slot) emits
    other indices or another sample for one of the traced blocks.  Only blocks whose traced scores say that the mask changes some
    step's selected set are coded again; the first one that comes out differently settles it."""
    O = _oracle()
    c = _cases()[0][name][k]
    facts = _traced(name, k)[0]
    if not any(f["moved"] for f in facts):
        return False
    for bl, f in zip(_blocks(c), facts):
        if not f["moved"]:
            continue
        O.set_masked_slot(c["B"] - 1)
        try:
            idx1, smp1 = O.encode_block(*bl, SEED, c["omega"], c["S"], c["B"], max_K=c["max_K"])
        finally:
            O.set_masked_slot(None)
        if idx1 != f["idx"] or not np.array_equal(smp1, f["smp"]):
            return True
    return False


@pytest.mark.both_suites
@pytest.mark.usefixtures("suite")
@pytest.mark.parametrize("name", _names())
def test_corner_calls_decide_something(name):
    """The oracle alone: over the calls of a name, its traces show a non-zero index, four partitions, an emitted path through a beam slot
    only this build has, an emitted index in the last wave of samples -- and, the proof of power, the oracle with slot B - 1 masked out
    of the selection emits something else: a kernel that drops, overwrites or never fills its last beam slot fails
    test_corner_calls_match_the_oracle of this name.  (Names of one beam have no slot to lose.)"""
    calls = _cases()[0][name]
    b_max = max(c["B"] for c in calls)
    thr = slot_threshold(name, b_max)
    met = dict(nonzero=False, K4=False, slot=thr is None, wave=False, masked=b_max < 2)
    n_wrong = 0
    for k, c in enumerate(calls):
        facts, wrong = _traced(name, k)
        n_wrong += bool(wrong)
        mine = dict(nonzero=any(f["nonzero"] for f in facts), K4=any(f["K"] >= 4 for f in facts),
                    slot=thr is not None and c["B"] > thr and any(f["parent"] >= thr for f in facts),
                    wave=any(f["wave"] for f in facts))
        for what, ok in mine.items():
            met[what] = met[what] or ok
        print(f"{name:52s} {_words(c)}  K {min(f['K'] for f in facts)}..{max(f['K'] for f in facts)}  meets: "
              f"{' '.join(w for w, ok in mine.items() if ok) or '-'}  (blocks through slot >= {thr}: {sum(thr is not None and f['parent'] >= thr for f in facts)}, "
              f"in the last wave: {sum(f['wave'] for f in facts)}, through slot B - 1: {sum(f['through'] for f in facts)}, "
              f"steps the mask changes: {sum(f['moved'] for f in facts)}, steps with a tie: {sum(f['ties'] for f in facts)})")
    print(f"{name:52s} calls whose traced blocks ties_to_higher changes: {n_wrong} of {len(calls)}")
    for k in sorted(range(len(calls)), key=lambda k: calls[k]["cost"]):          # (the cheapest call that proves it)
        if not met["masked"] and _masked_slot_changes(name, k):
            met["masked"] = True
            print(f"{name:52s} slot B - 1 masked changes the output of: {_words(calls[k])}")
    assert {w for w, ok in met.items() if not ok} == KNOWN_UNMET.get(name, set()), (name, met)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def _referee_cost(call, K):
    return REFEREE_PASSES * float(call["S"]) * call["dim"] * (1 + max(K - 1, 0) * call["B"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", _names())
def test_corner_calls_match_the_oracle(engine, oracle, name):
    """Every corner call of the name: the plan names the kernel; K, indices and samples (the four margins for margin names) equal
    oracle.encode_tensors_omp bit for bit; decode_blocks returns the sample; and one block's GPU path passes the float64 referee: a block
    of four partitions or more of the call of the most beams among those where 25 float64 passes over the block fit the budget."""
    import torch
    from irec import _lib
    import f64_referee as R
    from test_f64_referee import path_passes
    n_cu = engine.plan(engine.params(3.0, 36, 20), engine.layout(1, 192, 192, 42), 8)["n_cu"]
    calls = _cases(n_cu)[0][name]
    assert calls and all(c["S"] >= 2 for c in calls)
    firsts = []
    for c in calls:
        B, S, n_blocks, dim, max_K, flags, omega = c["B"], c["S"], c["n_blocks"], c["dim"], c["max_K"], c["flags"], c["omega"]
        margins = bool(flags & _lib.IREC_FLAG_MARGINS)
        host = kn.corner_inputs(oracle, c)
        ql, qs, pl, ps = (torch.from_numpy(a).cuda().contiguous() for a in host)
        lay = engine.layout(n_blocks, dim, dim, SEED)
        assert lay.n_blocks == n_blocks and lay.max_dim == dim
        params = engine.params(omega, S, B, flags & ~_lib.IREC_FLAG_MARGINS)
        plan = engine.plan(params, lay, max_K, margins=margins)
        assert kn.canonical(plan["kernel"], plan["split"]) == name, (plan, c)
        mg = None
        if margins:
            K, idx, sample, mg = engine.encode_blocks_margins(params, lay, ql, qs, pl, ps, SEED, max_K)
        else:
            K, idx, sample = engine.encode_blocks(params, lay, ql, qs, pl, ps, SEED, max_K)
        dec = engine.decode_blocks(params, lay, pl, ps, SEED, K, idx)
        torch.cuda.synchronize()
        Kh, ih, sh = K.cpu().numpy(), idx.cpu().numpy(), sample.cpu().numpy().reshape(n_blocks, dim)
        assert Kh.min() >= 0 and Kh.max() <= max_K, (name, _words(c), int(Kh.min()), int(Kh.max()))
        ridx, rs, _, rmg = oracle.encode_tensors_omp(*host, SEED, omega, S, B, dim, max_K=max_K, margins=True)
        for i in range(n_blocks):
            row = lay.natural[i]
            assert Kh[row] == len(ridx[i][0]) and ih[row, :Kh[row]].tolist() == ridx[i][0], (name, _words(c), i)
        assert np.array_equal(sh, rs), (name, _words(c))
        assert np.array_equal(dec.cpu().numpy().reshape(n_blocks, dim), sh), (name, _words(c))
        if margins:
            mh = mg.cpu().numpy()
            for i in range(n_blocks):
                assert np.array_equal(mh[lay.natural[i]], rmg[i, 0]), (name, _words(c), i, mh[lay.natural[i]], rmg[i, 0])
        Kn = Kh[lay.natural[:n_blocks]]
        i = int(np.argmax(Kn >= 4)) if (Kn >= 4).any() else int(np.argmax(Kn))      # the first block of four partitions or more
        firsts.append((c, host, i, ih[lay.natural[i], :Kh[lay.natural[i]]]))
    # the referee, on one block's GPU path: of the calls whose block fits the budget the one of the most beams (the cheaper of two);
    # where none fits, the cheapest
    cost = [_referee_cost(c, len(path)) for c, _, _, path in firsts]
    order = sorted(range(len(calls)), key=lambda k: (-calls[k]["B"], cost[k]))
    k = next((k for k in order if cost[k] <= kn.BUDGET), int(np.argmin(cost)))
    c, host, i, path = firsts[k]
    assert len(path) >= 1, (name, _words(c), "the referee's block codes nothing")
    bl = tuple(a[i][oracle.tf_shuffle_perm(SEED, c["dim"])] for a in host)
    _, _, tr = oracle.encode_block(*bl, SEED, c["omega"], c["S"], c["B"], max_K=c["max_K"], trace=True)
    bad = path_passes(R.rescore(*bl, SEED, c["omega"], c["S"], c["B"], tr["sel"], n_spread=32), path)
    assert not bad, (name, _words(c), i, bad[:3])
