#!/usr/bin/env python3
"""Every field of irec_plan_info and irec_plan_detail that irec_test_plan (csrc/irec_internal.h) returns, one line per call, over

  * the grid of tests/kernel_names.py -- BEAMS x SAMPLES x (DIMS + ((8192, 128),)) x flag_sets x BLOCKS, table_dims = [dim] -- and
  * the CALLS of tests/test_planner.py with their own table dims and that test's four flag sets,

each at 32 / 64 / 128 / 256 / 304 CUs.  Host only; no device is touched.  Two builds of the library plan alike exactly when their dumps are
byte-identical: a change that is not meant to retune the planner (a refactor of irec_host.cpp) is checked by

    python scripts/plan_dump.py --lib <the parent's libirec_hip.so> -o before.txt
    python scripts/plan_dump.py -o after.txt && cmp before.txt after.txt

(the SHA-256 of the dump and its line count go to stderr).  --golden FILE writes the CALLS part alone as JSON: tests/golden/plan_snapshot.json,
which tests/test_planner.py compares the live plan with field by field -- an intended retune shows as a diff of that file.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "relative-entropy-coding_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="the library to load instead of the tree's libirec_hip.so (a build of another commit)")
    ap.add_argument("-o", "--out", help="the dump (default: standard output)")
    ap.add_argument("--golden", metavar="FILE", help="write the CALLS part as JSON to FILE instead of the dump")
    args = ap.parse_args()

    from irec import _lib
    from irec.engine import Engine
    import kernel_names
    import test_planner
    lib = _lib.load(args.lib)
    info, det = _lib.IrecPlanInfo(), _lib.IrecPlanDetail()

    def plan(n_cu, B, S, n_blocks, max_dim, dims, max_K, flags):
        p = Engine.params(3.0, S, B, flags, list(dims))
        st = lib.irec_test_plan(n_cu, 2400, ctypes.byref(p), n_blocks, max_dim, max_K, ctypes.byref(info), ctypes.byref(det))
        assert st == 0, (n_cu, B, S, n_blocks, max_dim, dims, max_K, flags, lib.irec_last_error())
        return info.as_dict(), det.as_dict()

    def planner_calls():
        for name, B, S, n_blocks, max_dim, dims, max_K in test_planner.CALLS:
            for n_cu in test_planner.N_CU:
                for flags in (0, _lib.IREC_FLAG_NO_SPLIT, _lib.IREC_FLAG_TEAM, _lib.IREC_FLAG_MARGINS if max_dim <= 1024 else 0):
                    yield name, n_cu, flags, plan(n_cu, B, S, n_blocks, max_dim, dims, max_K, flags)

    if args.golden:
        records = [json.dumps(dict(call=name, n_cu=n_cu, flags=flags, info=i, detail=d), sort_keys=True) for name, n_cu, flags, (i, d) in planner_calls()]
        with open(args.golden, "w") as f:
            f.write("[\n" + ",\n".join(records) + "\n]\n")
        print(f"{len(records)} records -> {args.golden}", file=sys.stderr)
        return

    out = open(args.out, "w") if args.out else sys.stdout
    sha, n_lines = hashlib.sha256(), 0

    def emit(key, planned):
        nonlocal n_lines
        i, d = planned
        line = " ".join(map(str, key)) + " | " + " ".join(f"{k}={v}" for k, v in i.items()) + " | " + " ".join(f"{k}={v}" for k, v in d.items()) + "\n"
        out.write(line)
        sha.update(line.encode())
        n_lines += 1

    for n_cu in test_planner.N_CU:
        for B in kernel_names.BEAMS:
            for S in kernel_names.SAMPLES:
                for dim, max_K in kernel_names.DIMS + ((8192, 128),):
                    for flags in kernel_names.flag_sets(_lib):
                        for nb in kernel_names.BLOCKS:
                            emit((n_cu, B, S, dim, max_K, flags, nb), plan(n_cu, B, S, nb, dim, (dim,), max_K, flags))
    for name, n_cu, flags, planned in planner_calls():
        emit((n_cu, name.replace(" ", "_"), flags), planned)
    if args.out:
        out.close()
    print(f"{n_lines} lines, sha256 {sha.hexdigest()}", file=sys.stderr)


if __name__ == "__main__":
    main()
