#!/usr/bin/env python3
"""CPU model of the lane swaps of the team encoder (csrc/irec_kernels.h, "Lane swaps") on a call's REAL proposal table.

usage: scripts/lane_swap_model.py [--seed 42] [--samples 36] [--dims 1000 192] [--steps 8] [--out profiles/TAG/lane_swaps.log]
       scripts/lane_swap_model.py --self-check

A look-up instruction of the scoring loop is served in two 32-lane groups; each costs the LDS as many cycles as its busiest bank holds
addresses ("The gather ceiling").  Lane l of dim group g looks up quad 64 g + l of the step's row; its bank is
dlog(r) mod 32 in table copy 0 and 22 banks further in copy 1, and the preparation kernel picks the copy per look-up so that the busiest
bank of the group holds as few as possible (an exact assignment on two 16-rings of banks).  The quads j and j + 32 of a dim group may also
trade lanes (the first level of the lane tree adds lanes l and l ^ 32): one 32-bit mask per (step, dim group) chooses WHICH 32 quads
form a group.  This script draws the table on the host (the library's Philox twin, no GPU), and prints the distribution of the busiest
bank L over all (step, sample, dim slot, 32-lane group) with identity masks and with the masks of the greedy search swap_mask_kernel
runs (flip a bit, keep the flip if the step's sum of L drops; two passes over the 32 bits).

The exact min-max of a ring is computed in closed form: an orientation of a multigraph can keep every in-degree <= L exactly when no
connected subgraph has more than L edges per node (Hakimi), and the connected subgraphs of a ring are its arcs and the ring itself.
--self-check compares that form with the preparation kernel's search (ported line by line) on random counts.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "relative-entropy-coding_amd"))

P = 10007
RING = np.array([[(ring + 22 * p) & 31 for p in range(16)] for ring in range(2)])   # bank of node p of either ring


def dlog_table():
    g = next(c for c in range(2, P) if len({pow(c, e, P) for e in range(P - 1)}) == P - 1)
    dlog = np.zeros(P, dtype=np.int64)
    x = 1
    for e in range(P - 1):
        dlog[x] = e
        x = x * g % P
    return dlog


def busiest(counts):
    """counts [..., 32]: look-ups whose copy-0 bank this is -> [...] busiest bank of the best copy assignment (0 for an empty group)."""
    out = np.zeros(counts.shape[:-1], dtype=np.int64)
    for ring in range(2):
        n = counts[..., RING[ring]]                          # n[p]: edges between node p and node p + 1
        tot = n.sum(-1)
        best = -(-tot // 16)
        c = np.concatenate([np.zeros_like(n[..., :1]), np.cumsum(np.concatenate([n, n], -1), -1)], -1)
        for k in range(1, 16):                               # an arc of k consecutive edge groups spans k + 1 nodes
            arc = (c[..., k:k + 16] - c[..., :16]).max(-1)
            best = np.maximum(best, -(-arc // (k + 1)))
        out = np.maximum(out, best)
    return out


def ring_search(n):
    """the search of ring_min_busiest (csrc/irec_prep.hip), one ring of 16 counts"""
    tot = int(sum(n))
    for L in range((tot + 15) >> 4 if tot > 16 else 1, 32):
        for x0 in range(n[0] + 1):
            xp, ok = x0, True
            for p in range(1, 16):
                ub = L - n[p - 1] + xp
                ok = ok and ub >= 0
                xp = n[p] if n[p] < ub else max(ub, 0)
            if ok and x0 + n[15] - xp <= L:
                return L
    return 32


def self_check(rounds=3000):
    rng = np.random.default_rng(0)
    for _ in range(rounds):
        k = int(rng.integers(1, 33))
        counts = np.bincount(rng.integers(0, 32, k), minlength=32)
        want = max(ring_search([int(v) for v in counts[RING[r]]]) if counts[RING[r]].sum() else 0 for r in range(2))
        got = int(busiest(counts[None])[0])
        assert got == want, (counts, got, want)
    print(f"self-check: closed form == ring search on {rounds} random groups")


def banks_of_step(uniform_int, dlog, seed, t, S, D):
    """[S, 4 slots, quads] copy-0 bank of every look-up of step t (dims past D inside the last quad: entry 0, as the table has them)"""
    r = uniform_int(seed + t, S * D).reshape(S, D).astype(np.int64)
    al = np.zeros((S, (D + 3) // 4 * 4), dtype=np.int64)
    al[:, :D] = dlog[r]
    return (al % 32).reshape(S, -1, 4).transpose(0, 2, 1)


def group_cost(bank, in_hi):
    """bank [S, 4, nq] of one dim group, in_hi [nq] bool: quad sits in lanes 32-63 -> L of both 32-lane groups, [S, 4, 2]"""
    S, _, nq = bank.shape
    out = np.zeros((S, 4, 2), dtype=np.int64)
    for h in range(2):
        sel = bank[:, :, in_hi == bool(h)]
        counts = np.zeros((S, 4, 32), dtype=np.int64)
        for b in range(32):
            counts[..., b] = (sel == b).sum(-1)
        out[..., h] = busiest(counts)
    return out


def search_mask(bank):
    """the greedy search of swap_mask_kernel on one dim group: bank [S, 4, nq <= 64] -> (mask, L identity [S,4,2], L searched)"""
    nq = bank.shape[2]
    hi0 = np.arange(nq) >= 32
    ident = group_cost(bank, hi0)
    best, mask, cur = int(ident.sum()), 0, ident
    for _ in range(2):
        for j in range(min(nq, 32)):
            m = mask ^ (1 << j)
            hi = hi0 ^ np.array([((m >> (q & 31)) & 1) == 1 for q in range(nq)])
            c = group_cost(bank, hi)
            if int(c.sum()) < best:
                best, mask, cur = int(c.sum()), m, c
    return mask, ident, cur


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--samples", type=int, default=36)
    ap.add_argument("--dims", type=int, nargs="+", default=[1000, 192])
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--out")
    ap.add_argument("--self-check", action="store_true")
    a = ap.parse_args()
    if a.self_check:
        return self_check()
    from irec.engine import philox_uniform_int
    dlog = dlog_table()
    lines = [f"# lane-swap model: seed {a.seed}, S = {a.samples}, steps 0..{a.steps - 1}; L = busiest bank of a 32-lane look-up group under the exact copy assignment",
             "# dim | grouping | groups | mean L | share L=1 | L=2 | L=3 | L>=4 | sum L"]
    for D in a.dims:
        Ls = {"identity": [], "searched": []}
        masks = []
        for t in range(a.steps):
            bank = banks_of_step(philox_uniform_int, dlog, a.seed, t, a.samples, D)
            for g in range((bank.shape[2] + 63) // 64):
                m, ident, srch = search_mask(bank[:, :, 64 * g:64 * g + 64])
                masks.append(m)
                Ls["identity"].append(ident.ravel())
                Ls["searched"].append(srch.ravel())
        for k, v in Ls.items():
            v = np.concatenate(v)
            v = v[v > 0]                                      # (a group without quads issues no look-up)
            sh = [float((v == 1).mean()), float((v == 2).mean()), float((v == 3).mean()), float((v >= 4).mean())]
            lines.append(f"{D} | {k} | {v.size} | {v.mean():.4f} | " + " | ".join(f"{x:.4f}" for x in sh) + f" | {int(v.sum())}")
        lines.append(f"# {D}: masks of step 0: " + " ".join(f"{m:08x}" for m in masks[:(((D + 3) // 4) + 63) // 64]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
