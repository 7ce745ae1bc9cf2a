#!/usr/bin/env python3
"""Is the device code of two builds of libirec_hip.so the same, kernel by kernel?  (no GPU needed)

usage: scripts/isa_identity.py A/libirec_hip.so B/libirec_hip.so [out.txt]

Takes every gfx950 code object out of both libraries (llvm-objdump --offloading), and for every function symbol of their .text
compares
  * the disassembled instructions of the LINKED code object: mnemonics, operands, encoding words and the resolved branch targets
    (<symbol+offset>); only the absolute address column is dropped, since a kernel may sit elsewhere in another code object;
  * the kernel's metadata note: VGPRs, AGPRs, SGPRs, scratch, static LDS, kernarg size, launch bound, ... (every scalar key).
Which translation unit a kernel was compiled in is free to differ; a kernel present on one side only is a difference.
Prints one line per kernel and exits 1 on any difference.
"""
import hashlib, os, re, shutil, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
META_SKIP = {".name", ".symbol"}


def code_objects(lib, tmp, tag):
    d = os.path.join(tmp, tag)
    os.makedirs(d)
    shutil.copy(lib, os.path.join(d, "lib.so"))
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=d, check=True, stdout=subprocess.DEVNULL)
    cos = [f for f in os.listdir(d) if "amdgcn" in f]
    return [os.path.join(d, f) for f in sorted(cos, key=lambda f: int(f.split(".")[2]))]


def functions(co):
    """symbol -> (number of instructions, bytes, sha1 of the normalised listing)"""
    txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    out, name, lines, size = {}, None, [], 0

    def close():
        if name is not None:
            out[name] = (len(lines), size, hashlib.sha1("\n".join(lines).encode()).hexdigest()[:16])

    for l in txt.split("\n"):
        m = re.match(r"^[0-9a-f]{16} <(.+)>:$", l)
        if m:
            close()
            name, lines, size = m.group(1), [], 0
            continue
        m = re.match(r"^\t(.*?)\s*// [0-9A-F]{12}: ((?:[0-9A-F]{8} ?)+)\s*(<.*>)?\s*$", l)
        if m and name is not None:
            lines.append(f"{m.group(1)} | {m.group(2).strip()} | {m.group(3) or ''}")
            size += 4 * len(m.group(2).split())
    close()
    return out


def metadata(co):
    """kernel symbol -> {key: value} of the scalar keys of its amdhsa.kernels entry"""
    txt = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for l in txt.split("\n"):
        m = re.match(r"^  (-| ) (\.\w+):\s+(\S.*)$", l)   # a kernel's own keys: "  - .key: v" opens an entry, "    .key: v" goes on
        if l.startswith("amdhsa."):
            cur = {} if l.startswith("amdhsa.kernels") else None
        elif m and cur is not None:
            if m.group(1) == "-":
                cur = {}
            cur[m.group(2)] = m.group(3).strip()
            if m.group(2) == ".symbol":
                out[m.group(3).strip().strip("'").removesuffix(".kd")] = cur
    return {k: {a: b for a, b in v.items() if a not in META_SKIP} for k, v in out.items()}


def survey(lib, tmp, tag):
    fn, md = {}, {}
    for i, co in enumerate(code_objects(lib, tmp, tag)):
        for s, v in functions(co).items():
            fn.setdefault(s, []).append((i, v))
        for s, v in metadata(co).items():
            md.setdefault(s, []).append(v)
    return fn, md


def main():
    a, b = sys.argv[1], sys.argv[2]
    out = open(sys.argv[3], "w") if len(sys.argv) > 3 else sys.stdout
    tmp = tempfile.mkdtemp()
    try:
        fa, ma = survey(a, tmp, "a")
        fb, mb = survey(b, tmp, "b")
    finally:
        shutil.rmtree(tmp)
    syms = sorted(set(fa) | set(fb))
    dem = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    bad = 0
    print("# kernel | code object in A -> in B | instructions | bytes | sha1 of the listing | VGPRs/AGPRs/SGPRs/scratch/static LDS/kernarg/launch bound | verdict", file=out)
    for s, d in zip(syms, dem):
        d = re.sub(r"\(irec::\w+\)$", "", d).replace("void irec::", "").replace("irec::", "")
        va, vb = fa.get(s, []), fb.get(s, [])
        same_code = len(va) == 1 and len(vb) == 1 and va[0][1] == vb[0][1]
        same_meta = ma.get(s) == mb.get(s) and (s not in ma or len(ma[s]) == 1)
        ok = same_code and same_meta
        bad += not ok
        v = (va or vb)[0][1]
        m = (ma.get(s) or mb.get(s) or [{}])[0]
        regs = "/".join(m.get(k, "-") for k in (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size",
                                                ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size"))
        where = f"{','.join(str(i) for i, _ in va) or '-'} -> {','.join(str(i) for i, _ in vb) or '-'}"
        verdict = "same" if ok else "DIFFERENT" + ("" if same_code else " code") + ("" if same_meta else " metadata")
        print(f"{d} | {where} | {v[0]} | {v[1]} | {v[2]} | {regs} | {verdict}", file=out)
    print(f"# {len(syms)} functions, {sum(1 for s in syms if s in ma or s in mb)} kernels with metadata, {bad} different", file=out)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
