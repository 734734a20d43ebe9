#!/usr/bin/env python
"""Compare the device code of two source trees, kernel by kernel.

    isa_compare.py CSRC_A CSRC_B [--work DIR] [--jobs N] [file.hip ...]

Every named translation unit (default: all of build.py's SOURCES present in both trees) is compiled from both csrc directories to
device assembly with build.py's FLAGS + FILE_FLAGS[file] (-S --cuda-device-only, as isa_sections.py does).  Each kernel is then
classed as
    identical   the same instruction lines in the same order
    reordered   the same multiset of instruction lines
    different   anything else, with the instruction-count delta (B - A) and the number of lines that have no partner on the other side
and its resources (SGPR, VGPR, AGPR, scratch, occupancy, LDS: the figures kernel_resources.py prints) are compared.
Labels, directives and comments are not instructions; a branch target counts as "a basic block", whatever its number (one block more
or less renumbers every label behind it).
--work keeps the assembly files (a/ and b/); an existing file is reused, so the unchanged side is compiled once."""
import argparse, collections, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
HERE = os.path.dirname(os.path.abspath(__file__)); sys.path.insert(0, os.path.dirname(HERE))
from lightplane_amd.csrc import build as B

RES = ["NumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize"]


def compile_asm(csrc, src, out):
    if not os.path.exists(out):
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + B.FLAGS + B.FILE_FLAGS.get(src, []) + ["-S", "--cuda-device-only", os.path.join(csrc, src), "-o", out + ".tmp"]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        if p.returncode != 0:
            sys.exit(f"--- {' '.join(cmd)} failed ---\n{p.stdout.decode()}")
        os.replace(out + ".tmp", out)
    return out


def kernels(path):
    """{kernel: (instruction lines, {resource: value})} of one assembly file"""
    lines = open(path).read().splitlines()
    names = {m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    out, cur, body = {}, None, False
    for l in lines:
        t = l.split(";")[0].strip() if not l.lstrip().startswith(";") else l.strip()
        m = re.match(r"\.type\s+(\S+),@function", t)
        if m:
            cur, body = (m.group(1) if m.group(1) in names else None), False
            if cur:
                out[cur] = ([], {})
            continue
        if cur is None:
            continue
        if t == cur + ":":
            body = True
        elif t.startswith(".Lfunc_end"):
            body = False
        elif t.startswith(";"):
            m = re.match(r";\s*(\w+): (\d+)", t)
            if m and m.group(1) in RES:
                out[cur][1][m.group(1)] = int(m.group(2))
        elif body and t and not t.startswith(".") and not t.endswith(":"):
            out[cur][0].append(re.sub(r"\.LBB\d+_\d+", ".LBB", re.sub(r"\s+", " ", t)))
    return out


def demangle(names):
    txt = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True).stdout.splitlines()
    return {n: re.sub(r"\(.*", "", d.replace("(anonymous namespace)::", "")).replace("void lp::", "") for n, d in zip(names, txt)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("a"); ap.add_argument("b"); ap.add_argument("files", nargs="*")
    ap.add_argument("--work"); ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_intermixed_args()
    files = args.files or [f for f in B.SOURCES if all(os.path.exists(os.path.join(d, f)) for d in (args.a, args.b))]
    work = args.work or tempfile.mkdtemp(prefix="isa_compare_")
    for side in "ab":
        os.makedirs(os.path.join(work, side), exist_ok=True)
    with ThreadPoolExecutor(args.jobs) as ex:
        jobs = [ex.submit(compile_asm, d, f, os.path.join(work, side, f.replace(".hip", ".s"))) for f in files for side, d in (("a", args.a), ("b", args.b))]
        for j in jobs:
            j.result()
    tally, res_diff = collections.Counter(), 0
    for f in files:
        ka, kb = (kernels(os.path.join(work, side, f.replace(".hip", ".s"))) for side in "ab")
        nice = demangle(sorted(set(ka) | set(kb)))
        print(f"== {f}: {len(ka)} / {len(kb)} kernels")
        for n in sorted(set(ka) | set(kb), key=lambda n: nice[n]):
            if n not in ka or n not in kb:
                cls = "only in " + ("A" if n in ka else "B")
                tally["only in one"] += 1
                print(f"  {cls:24s} {nice[n]}")
                continue
            (ia, ra), (ib, rb) = ka[n], kb[n]
            if ia == ib:
                cls = "identical"
            elif collections.Counter(ia) == collections.Counter(ib):
                cls = "reordered"
            else:
                cls = "different"
            tally[cls] += 1
            ca, cb = collections.Counter(ia), collections.Counter(ib)
            odd = sum((ca - cb).values()) + sum((cb - ca).values())   # lines of either side without a partner on the other
            note = f"{len(ia)} instr" if cls != "different" else f"{len(ia)} -> {len(ib)} instr ({len(ib) - len(ia):+d}; {odd} unpaired)"
            bad = [f"{k} {ra.get(k)} -> {rb.get(k)}" for k in RES if ra.get(k) != rb.get(k)]
            res_diff += bool(bad)
            print(f"  {cls:10s} {note:30s} {'resources equal' if not bad else 'RESOURCES: ' + ', '.join(bad):18s} {nice[n]}")
    print("== total: " + ", ".join(f"{v} {k}" for k, v in sorted(tally.items())) + f"; kernels whose resources differ: {res_diff}")


if __name__ == "__main__":
    main()
