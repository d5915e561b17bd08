#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel (CPU only).

    for s in engine waveglow ...; do
        hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S csrc/$s.hip -o DIR/$s.s
    done
    scripts/asm_kernel_diff.py DIR_BEFORE DIR_AFTER

For every .s file of either directory: whether the whole file is byte-identical (apart from hipcc's compile-unit id, which
hashes the source path), and for every kernel (a symbol with a .amdhsa_kernel block) whether its instruction stream and its
.amdhsa_* block are identical, with VGPR / AGPR / SGPR counts, scratch bytes, static LDS bytes (dynamic LDS is a launch
argument) and the compiler's occupancy on both sides.  Kernels present on one side only are listed as such.  Local labels are
compared without their per-file ordinals.  The script only diffs text and reads the resource fields.  Exit status 1 if
anything differs.  --brief prints identical kernels as a count per file.
"""
import pathlib
import re
import sys

FIELDS = ("vgpr", "agpr", "sgpr", "scratch", "lds", "occ")


def demangle_hint(sym):
    # template arguments of gemm_f32_kernel as the mangled name spells them (Li4ELi1E... -> 4,1,...; Lb1E -> true)
    m = re.search(r"gemm_f32_kernelI((?:L[ib]\d+E)+)", sym)
    if not m:
        return sym
    return "gemm_f32_kernel<" + ",".join(re.findall(r"L[ib](\d+)E", m.group(1))) + ">"


def kernels(path):
    """{symbol: (instruction stream, amdhsa block, resources)} of one assembly file."""
    lines = path.read_text().splitlines()
    out = {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if not m:
            i += 1
            continue
        sym = m.group(1)
        j = i
        while not lines[j].strip().startswith(".end_amdhsa_kernel"):
            j += 1
        hsa = [l.strip() for l in lines[i + 1:j]]
        # the body: from the symbol's label to the .amdhsa_kernel block that closes it
        b0 = next(k for k, l in enumerate(lines) if l.startswith(sym + ":"))
        body = []
        for l in lines[b0 + 1:i]:
            l = l.split(";")[0].strip()          # comments carry source positions and compiler statistics
            if l and not l.startswith((".loc", ".file", ".cfi", ".p2align", ".section")):
                # local labels carry the function's ordinal (or a count) in the file, which shifts when a kernel leaves
                body.append(re.sub(r"\.L(BB|tmp|func_begin|func_end|post_getpc)\d+", r".L\1", l))
        f = dict(re.match(r"\.amdhsa_(\S+)\s+(\S+)", l).groups() for l in hsa if l.startswith(".amdhsa_"))
        tail = "\n".join(lines[j:j + 40])

        def stat(name):
            s = re.search(r";\s*" + name + r":\s*(\d+)", tail)
            return int(s.group(1)) if s else -1

        res = {"vgpr": stat("NumVgprs"), "agpr": stat("NumAgprs"), "sgpr": stat("TotalNumSgprs"),
               "scratch": int(f.get("private_segment_fixed_size", -1)), "lds": int(f.get("group_segment_fixed_size", -1)), "occ": stat("Occupancy")}
        out[sym] = (body, hsa, res)
        i = j + 1
    return out


def fmt(res):
    return " ".join(f"{k}={res[k]}" for k in FIELDS)


def main():
    brief = "--brief" in sys.argv
    dirs = [a for a in sys.argv[1:] if a != "--brief"]
    if len(dirs) != 2:
        sys.exit(__doc__)
    da, db = pathlib.Path(dirs[0]), pathlib.Path(dirs[1])
    names = sorted({p.name for p in da.glob("*.s")} | {p.name for p in db.glob("*.s")})
    bad = 0
    for name in names:
        pa, pb = da / name, db / name
        if not pa.exists() or not pb.exists():
            print(f"== {name}: only in {'before' if pa.exists() else 'after'}")
            bad += 1
            continue
        # __hip_cuid_<hash> is hipcc's compile-unit id, a hash of the source file's absolute path: two checkouts differ in it
        cuid = re.compile(rb"__hip_cuid_[0-9a-f]+")
        same_file = cuid.sub(b"__hip_cuid", pa.read_bytes()) == cuid.sub(b"__hip_cuid", pb.read_bytes())
        ka, kb = kernels(pa), kernels(pb)
        print(f"== {name}: {'byte-identical file' if same_file else 'files differ'}, kernels {len(ka)} -> {len(kb)}")
        n_same = 0
        for sym in sorted(set(ka) | set(kb)):
            label = demangle_hint(sym)
            if sym not in kb:
                print(f"  only before  {label}  [{fmt(ka[sym][2])}]")
                bad += 1
            elif sym not in ka:
                print(f"  only after   {label}  [{fmt(kb[sym][2])}]")
                bad += 1
            else:
                same = ka[sym][0] == kb[sym][0] and ka[sym][1] == kb[sym][1]
                bad += not same
                n_same += same
                if same and brief:
                    continue
                tag = "identical" if same else ("DIFFERS (code)" if ka[sym][0] != kb[sym][0] else "DIFFERS (amdhsa)")
                print(f"  {tag:<16} {label}  [{fmt(ka[sym][2])}] -> [{fmt(kb[sym][2])}]")
        if brief:
            print(f"  {n_same} kernels identical in code, .amdhsa block and resources")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
