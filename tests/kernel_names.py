"""Kernel names: what irec_encode_plan says a call launches <-> the instantiations compiled into libirec_hip.so.  Shared by
tests/test_kernel_coverage.py and scripts/kernel_coverage.py (the kernel trace of the GPU suite)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "relative-entropy-coding_amd", "csrc", "libirec_hip.so")


def compiled_kernels(lib=LIB):
    """Every __global__ function of the library, demangled and normalised: no namespace, no argument list, no spaces."""
    out = subprocess.run(["nm", "-C", lib], capture_output=True, text=True, check=True).stdout
    names = set()
    for line in out.splitlines():
        if "__device_stub__" not in line:
            continue
        n = line.split("__device_stub__", 1)[1]
        names.add(normalise(n))
    return names


def normalise(name):
    """'void irec::encode_team_kernel<20, 3, 1, false, ...>(irec::EncArgs)' / 'encode_team_kernel<20,3,1,...>' -> one spelling."""
    n = name.strip()
    n = re.sub(r"^void\s+", "", n)
    n = n.replace("irec::", "")
    depth, cut = 0, len(n)
    for i, ch in enumerate(n):        # the argument list: the first '(' outside the template brackets
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            cut = i
            break
    return n[:cut].replace(" ", "")


def canonical(plan_kernel, split=0):
    """The instantiation behind a name irec_encode_plan returns (first-pass block kernel), as compiled_kernels() spells it."""
    k = plan_kernel.strip()
    if k.startswith("encode_generic_kernel"):
        return "encode_generic_kernel"
    if k == "encode_lone_kernel":
        return k
    m = re.match(r"encode_ten_kernel<(\d+)>$", k)
    if m:
        return f"encode_ten_kernel<{m.group(1)}>"
    m = re.match(r"encode_team_kernel<(\d+),(\d+),(\d+)((?:,\w+)*)>$", k)
    if m:
        tags = set(t for t in m.group(4).split(",") if t)
        b = lambda v: "true" if v else "false"
        share = split >= 2
        return (f"encode_team_kernel<{m.group(1)},{m.group(2)},{m.group(3)},{b('passes' in tags)},{b('one' in tags)},"
                f"{b(share)},{b('margins' in tags)}>")
    m = re.match(r"encode_chunk_kernel<(\d+),(\d+),(\d+)(,gang)?>$", k)
    if m:
        return f"encode_chunk_kernel<{m.group(1)},{m.group(2)},{m.group(3)},{'true' if m.group(4) else 'false'}>"
    m = re.match(r"encode_fast_kernel<(\d+),(\d+),(true|false)(?:,(\d))?>$", k)
    if m:
        return f"encode_fast_kernel<{m.group(1)},{m.group(2)},{m.group(3)},{m.group(4) or 0}>"
    raise ValueError(f"unknown kernel name {plan_kernel!r}")


# the grid the planner is enumerated over (tests/test_kernel_coverage.py): beams, samples, (largest block, max_K), blocks per call, flags
BEAMS = (1, 2, 5, 7, 10, 11, 16, 20, 21, 25, 30, 31, 32, 33, 40, 48, 50, 54, 57, 60, 61, 100)
SAMPLES = (1, 7, 20, 25, 26, 36, 38, 39, 54, 55, 80, 102, 103, 148, 244, 403, 735, 1339, 1808, 8103)
DIMS = ((192, 32), (1000, 32), (2048, 64))
BLOCKS = (1, 9, 13, 40, 63, 64, 72, 126, 200, 256, 257, 302, 342, 400, 512, 513, 700, 2304)


def flag_sets(_lib):
    sh = _lib.IREC_FLAG_SHAPE
    return (0, _lib.IREC_FLAG_NO_SPLIT, _lib.IREC_FLAG_TEAM, _lib.IREC_FLAG_ONE_TABLE, _lib.IREC_FLAG_FUSED_PHILOX, _lib.IREC_FLAG_FORCE_GENERIC,
            _lib.IREC_FLAG_MARGINS, _lib.IREC_FLAG_NO_TEN, _lib.IREC_FLAG_NO_TEN | _lib.IREC_FLAG_NO_SPLIT, sh["2"], sh["3"], sh["1x2"],
            sh["team"] | _lib.IREC_FLAG_TEAM, sh["3"] | _lib.IREC_FLAG_NO_TEN)


def case_inputs(oracle, case, seed=7):
    """The host arrays (mq, sq, mp, sp), each [n_blocks, dim], that the tests of a planner case code: one synthetic latent a block."""
    import numpy as np
    rng = np.random.default_rng(seed)
    stats = [oracle.synthetic_latent(3000 + int(rng.integers(1 << 20)), case["dim"]) for _ in range(case["n_blocks"])]
    return [np.stack([s[j] for s in stats]) for j in range(4)]


def rejects_by_step_two(B, S):
    """A call of B beams and S samples rejects a candidate in its first or second step (S > B, or S * min(B, S) > B): its top-B
    selection has something to decide on every block of two or more partitions."""
    return S > B or S * min(B, S) > B


def _planner():
    """(lib, _lib, Engine) of the product's host library: what enumerate_plans and enumerate_ranges ask."""
    import sys
    for p in (ROOT, os.path.join(ROOT, "relative-entropy-coding_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from irec import _lib
    from irec.engine import Engine
    return _lib.load(), _lib, Engine


def plan_name(n_cu, B, S, dim, max_K, n_blocks, flags, omega=3.0):
    """(canonical kernel name, team slots = workgroups * teams per workgroup) of one call on a device of n_cu compute units."""
    lib, _lib, Engine = _planner()
    info, det = _lib.IrecPlanInfo(), _lib.IrecPlanDetail()
    p = Engine.params(omega, S, B, flags, [dim])
    st = lib.irec_test_plan(n_cu, 2400, ctypes.byref(p), n_blocks, dim, max_K, ctypes.byref(info), ctypes.byref(det))
    assert st == 0, (B, S, dim, flags, n_blocks, lib.irec_last_error())
    return canonical(info.kernel.decode(), info.split), int(det.grid) * int(det.teams_per_wg)


# the finer dim grid of enumerate_ranges: (block dims, max_K).  1, 63 .. 65, 257, 1023 and 1024 for the builds of at most 1024 dims;
# 1025, 2049 (a last chunk of one dim) and 5000 for the chunk builds
RANGE_DIMS = ((1, 32), (63, 32), (64, 32), (65, 32), (192, 32), (257, 32), (1000, 32), (1023, 32), (1024, 32),
              (1025, 64), (2048, 64), (2049, 64), (5000, 64))
_ranges = {}


def enumerate_ranges(n_cu=256):
    """canonical kernel name -> every call of the grid BEAMS x SAMPLES x RANGE_DIMS x BLOCKS x flag_sets that launches it: an int64
    array [n, 6] of rows (B, S, dim, n_blocks, flags, over), over = 1 where the call has more blocks than team slots (workgroups *
    teams per workgroup: some team codes a second block).  About 15 s on one CPU thread; cached per n_cu."""
    import numpy as np
    if n_cu in _ranges:
        return _ranges[n_cu]
    lib, _lib, Engine = _planner()
    info, det = _lib.IrecPlanInfo(), _lib.IrecPlanDetail()
    rows = {}
    for B in BEAMS:
        for S in SAMPLES:
            if S * B >= 1 << 24:
                continue
            for dim, max_K in RANGE_DIMS:
                for flags in flag_sets(_lib):
                    p = Engine.params(3.0, S, B, flags, [dim])
                    for nb in BLOCKS:
                        st = lib.irec_test_plan(n_cu, 2400, ctypes.byref(p), nb, dim, max_K, ctypes.byref(info), ctypes.byref(det))
                        assert st == 0, (B, S, dim, flags, nb, lib.irec_last_error())
                        rows.setdefault((info.kernel, info.split), []).append((B, S, dim, nb, flags, nb > det.grid * det.teams_per_wg))
    out = {}
    for (kernel, split), r in rows.items():
        out.setdefault(canonical(kernel.decode(), split), []).extend(r)
    _ranges[n_cu] = {name: np.array(sorted(set(r)), dtype=np.int64) for name, r in out.items()}
    return _ranges[n_cu]


def max_K_of(dim):
    """The max_K the grids pair with a block dim (DIMS, RANGE_DIMS): 32 up to 1024 dims, 64 beyond."""
    return 32 if dim <= 1024 else 64


def enumerate_plans(n_cu=256, dims=DIMS, blocks=BLOCKS, accept=None):
    """canonical kernel name -> the cheapest call of the grid that launches it: dict(B, S, n_blocks, dim, max_K, flags, plan).
    accept(B, S): only calls of these beams and samples count (tests/test_tie_breaking.py: calls whose selection rejects a candidate)."""
    import sys
    for p in (ROOT, os.path.join(ROOT, "relative-entropy-coding_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from irec import _lib
    from irec.engine import Engine
    lib = _lib.load()
    info, det = _lib.IrecPlanInfo(), _lib.IrecPlanDetail()
    best = {}
    for B in BEAMS:
        for S in SAMPLES:
            if S * B >= 1 << 24 or (accept is not None and not accept(B, S)):
                continue
            for dim, max_K in dims:
                for flags in flag_sets(_lib):
                    p = Engine.params(3.0, S, B, flags, [dim])
                    for nb in blocks:
                        st = lib.irec_test_plan(n_cu, 2400, ctypes.byref(p), nb, dim, max_K, ctypes.byref(info), ctypes.byref(det))
                        assert st == 0, (B, S, dim, flags, nb, lib.irec_last_error())
                        name = canonical(info.kernel.decode(), info.split)
                        cost = nb * dim * S * B
                        if name not in best or cost < best[name]["cost"]:
                            best[name] = dict(B=B, S=S, n_blocks=nb, dim=dim, max_K=max_K, flags=flags, cost=cost,
                                              kernel=info.kernel.decode(), split=int(info.split))
    return best


# ---- the encoder families (tests/test_memory_contract_gpu.py section B, tests/test_seed_domain_gpu.py) ----------------------------
def template_args(name):
    return name[name.index("<") + 1:-1].split(",") if "<" in name else []


# family -> (canonical name, its template arguments) -> whether the build belongs to it: one entry per way an encoder keeps its state
FAMILIES = {
    "split fast": lambda n, a: n.startswith("encode_fast_kernel<") and a[3] != "0",
    "team, shared rows": lambda n, a: n.startswith("encode_team_kernel<") and a[5] == "true",
    "chunk gang": lambda n, a: n.startswith("encode_chunk_kernel<") and a[3] == "true",
    "team": lambda n, a: n.startswith("encode_team_kernel<") and a[5] == "false" and a[6] == "false",
    "ten": lambda n, a: n.startswith("encode_ten_kernel<"),
    "lone": lambda n, a: n == "encode_lone_kernel",
    "one-table fast": lambda n, a: n.startswith("encode_fast_kernel<") and a[2] == "true" and a[3] == "0",
    "chunk": lambda n, a: n.startswith("encode_chunk_kernel<") and a[3] == "false",
    "generic": lambda n, a: n == "encode_generic_kernel",
}


def family_id(family):
    return family.replace(" ", "_").replace(",", "")


def family_members(plans, family):
    """The names of `plans` (enumerate_plans) that belong to a family, cheapest planned call first."""
    return sorted((n for n in plans if FAMILIES[family](n, template_args(n))), key=lambda n: (plans[n]["cost"], n))


def family_names(plans):
    """[(family, the name of its cheapest planned call, or None where the planner names no kernel of the family)]."""
    return [(family, (family_members(plans, family) or [None])[0]) for family in FAMILIES]


# ---- the corner calls of a name (tests/test_kernel_corners.py) -------------------------------------------------------------------
SEED = 42                                  # the coding seed of every corner call
BUDGET = 4e8                               # proposal evaluations per call, at most: scripts/soak_parity.py's per-block cap
# ... except the `blocks` corner of the names none of whose calls of more blocks than team slots fits BUDGET (one-team chunk builds: 257
# blocks of 1025 dims or more): such a call spreads over the oracle's 16 threads at 1.5e8 evaluations a second each, 8e9 take 3.3 s
BUDGET_BLOCKS = 8e9
OMEGAS = (3.0, 1.0, 0.5, 0.25, 0.1, 10.0)  # the ladder a call's Omega is taken from; the last rung is for blocks of 5000 dims
CHUNK = 1024                               # dims per chunk of encode_chunk_kernel (csrc/irec_chunk.h)
_stats, _corners = {}, {}


def rank_of_dim(dim):
    """How ragged a block dim is: 2 a last wave / chunk of one dim short or one dim long (1023, 2049), 1 any other dim beyond 64 that
    is no multiple of 64, 0 the rest."""
    return 2 if dim in (1023, 2049) else int(dim > 64 and dim % 64 != 0)


def corner_inputs(oracle, call, seed=None):
    """The host arrays (mq, sq, mp, sp), each [n_blocks, dim], of a corner call.  source 'synthetic': case_inputs; 'families' (dims too
    small for synthetic_latent to reach four partitions on the ladder): tests/latent_families.py, sharp on the even blocks, the
    members of mixed in turn on the odd ones."""
    import latent_families as L
    seed = call["seed"] if seed is None else seed
    if call["source"] == "synthetic":
        return case_inputs(oracle, call, seed=seed)
    dim, max_K, pools, bl = call["dim"], call["max_K"], {}, []
    for j in range(call["n_blocks"]):
        if j % 2 == 0:
            bl.append(L.block("sharp", dim, 1000 * seed + j, 1.0, max_K))
        else:
            k = seed + j // 20
            if k not in pools:
                pools[k] = L.mixed(dim, k, 1.0, max_K)
            bl.append(pools[k][(j // 2) % len(pools[k])])
    return list(L.stack(bl))


def call_stats(oracle, dim, n_blocks):
    """(Omega, source, K of every block) of the calls of n_blocks blocks of dim dims, on the inputs of seed 7: the first Omega of the
    ladder, on synthetic_latent and failing that on the families, at which no block exceeds max_K, the median K is at most 16 and at
    least a third of the blocks have 4 <= K <= 16 (synthetic_latent's blocks of one dim lie within two partitions of each other: all
    of them do).  Several steps of such a block run with B_cur = B."""
    import numpy as np
    key = (dim, n_blocks)
    if key not in _stats:
        perm = oracle.tf_shuffle_perm(SEED, dim)
        found = None
        for source in ("synthetic", "families"):
            call = dict(dim=dim, n_blocks=n_blocks, max_K=max_K_of(dim), source=source, seed=7)
            host = corner_inputs(oracle, call)
            kl = [oracle.block_kl(*(a[i][perm] for a in host)) for i in range(n_blocks)]
            for omega in OMEGAS:
                Ks = np.array([oracle.num_aux(v, omega) for v in kl])
                if Ks.max() <= call["max_K"] and np.median(Ks) <= 16 and 3 * int(((Ks >= 4) & (Ks <= 16)).sum()) >= n_blocks:
                    found = (omega, source, Ks)
                    break
            if found:
                break
        assert found, f"no Omega of the ladder gives blocks of {dim} dims 4 to 16 partitions"
        _stats[key] = found
    return _stats[key]


def call_cost(oracle, B, S, dim, n_blocks):
    """sum over the blocks of S * D * (1 + (K - 1) * B): the proposal evaluations of the call (step 1 scores S candidates, every later
    step at most S * B)."""
    Ks = call_stats(oracle, dim, n_blocks)[2]
    Ks = Ks[Ks >= 1]
    return float(S) * dim * float((1 + (Ks - 1) * B).sum())


def is_shared(name):
    """The shared-row builds of the team encoder: the sixth template argument."""
    m = re.match(r"encode_team_kernel<\d+,\d+,\d+,\w+,\w+,(\w+),\w+>$", name)
    return bool(m) and m.group(1) == "true"


def range_calls(rng):
    """The rejecting calls of a name's range (enumerate_ranges): {(B, S, dim, n_blocks): (smallest flags, over)}, S >= 2."""
    out = {}
    for B, S, dim, nb, flags, over in rng.tolist():
        if S >= 2 and rejects_by_step_two(B, S) and (B, S, dim, nb) not in out:        # (rows are sorted: the smallest flags first)
            out[(B, S, dim, nb)] = (flags, over)
    return out


def corner_cases(n_cu=256):
    """canonical kernel name -> at most 4 calls from the edges of the range the name serves (enumerate_ranges), each a dict(B, S, dim,
    max_K, n_blocks, flags, omega, source, seed = 7, roles, cost), every one with S >= 2 and rejecting by its second step; and the corners
    left out or beyond the budget: (dropped_S, over_budget), see tests/test_kernel_corners.py.  Every choice is `the first call, in an
    order of preference, that fits BUDGET`:
      full    the largest B, then the largest dim, the fewest blocks, the largest S;
      small   the smallest B, then the smallest S, the smallest dim, the fewest blocks;
      wide    the largest S of the range that fits at all, at the most ragged dim (rank_of_dim), then the largest B and dim;
      blocks  shared-row builds: the other end of their block window.  Names whose range has calls of more blocks than team slots:
              the smallest such count -- where none fits BUDGET, the first that fits BUDGET_BLOCKS (over_budget lists those names).
              The others: their largest block count.  Then the largest B, the smallest S and dim.
    Cached per n_cu."""
    if n_cu in _corners:
        return _corners[n_cu]
    from oracle import oracle as O
    O.lib()
    cases, dropped_S, over_budget = {}, [], []
    for name, rng in sorted(enumerate_ranges(n_cu).items()):
        calls = range_calls(rng)
        # (a third of a call's blocks have four partitions or more: calls far beyond the budget are turned down without their inputs)
        fits = lambda c: c[1] * c[2] * (1 + 3 * c[0]) * (c[3] // 3) <= BUDGET and call_cost(O, *c) <= BUDGET
        first = lambda cs, key: next((c for c in sorted(cs, key=key) if fits(c)), None)
        picked = []

        def take(c, role):
            if c is None:
                return
            for p in picked:
                if p[0] == c:
                    p[1].append(role)
                    return
            picked.append((c, [role]))
        take(first(calls, lambda c: (-c[0], -c[2], c[3], -c[1])), "full")
        take(first(calls, lambda c: (c[0], c[1], c[2], c[3])), "small")
        for S in sorted({c[1] for c in calls}, reverse=True):
            c = first([c for c in calls if c[1] == S], lambda c: (-rank_of_dim(c[2]), -c[0], -c[2], c[3]))
            if c is not None:
                take(c, "wide")
                break
            dropped_S.append((name, S))
        nb_min, nb_max = min(c[3] for c in calls), max(c[3] for c in calls)
        over = [c for c in calls if calls[c][1]]
        if is_shared(name):
            take(first([c for c in calls if c[3] == nb_max], lambda c: (-c[0], c[1], c[2])), "blocks")
        elif over:
            c = first(over, lambda c: (c[3], -c[0], c[1], c[2]))
            if c is None:
                c = next(c for c in sorted(over, key=lambda c: (c[3], -c[0], c[1], c[2])) if call_cost(O, *c) <= BUDGET_BLOCKS)
                over_budget.append(name)
            take(c, "blocks")
        elif nb_max > nb_min:
            take(first([c for c in calls if c[3] > nb_min], lambda c: (-c[3], -c[0], c[1], c[2])), "blocks")
        cases[name] = []
        for (B, S, dim, nb), roles in picked:
            omega, source, _ = call_stats(O, dim, nb)
            cases[name].append(dict(B=B, S=S, dim=dim, max_K=max_K_of(dim), n_blocks=nb, flags=calls[(B, S, dim, nb)][0], omega=omega,
                                    source=source, seed=7, roles=tuple(roles), cost=call_cost(O, B, S, dim, nb)))
    _corners[n_cu] = (cases, dropped_S, over_budget)
    return _corners[n_cu]

