#!/usr/bin/env python
"""How far ahead of their use does the sample loop of the tuned Renderer backward issue its LDS reads?  A static walk of the compiled
loop (the build line of scripts/isa_loop_mix.py: ONE instantiation, -DLP_DEV_ONE -DLP_ASM_MARKS, no GPU needed).

The walk follows the straight-line code of the loop and keeps an issue clock: 4 cycles per VALU / LDS / s_nop instruction, 8 per MFMA
(a lower bound of the time between two instructions of one wave -- what a wave could hide an LDS round trip of ~64 cycles behind if
nothing else held it up).  LDS instructions return in order, so an `s_waitcnt lgkmcnt(N)` waits for all but the youngest N of the
outstanding ones; the DISTANCE of a wait is the issue clock between the youngest READ it waits for and the wait itself.  A wait that
only drains stores (the barriers' lgkmcnt(0) behind tile stores) is listed apart.  Per phase mark: the number of waits on reads and the
histogram of their distances; `immediate` (< 16 cycles) are round trips the wave sits out in full.

    python scripts/isa_lds_waits.py [--c 16|32] [--csrc DIR] [--asm FILE.s] [--keep FILE.s] [--unrolled] [--list]
--unrolled  also prints the table of every quadrant loop of the sample loop (the dW quadrant rounds where they are `#pragma unroll 1`
            loops over the source waves: ONE iteration, which runs 4 -- trunk layer 1 with C = 16: 2 -- times per sample)
--list      every wait on a read with its phase, distance and the read it waits for
--asm       walk an assembly file kept earlier (--keep) instead of compiling"""
import argparse, collections, os, re, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__)); sys.path.insert(0, os.path.dirname(HERE))
from lightplane_amd.csrc import build as B

ap = argparse.ArgumentParser()
ap.add_argument("--c", type=int, default=16)
ap.add_argument("--csrc", default=B.HERE)
ap.add_argument("--asm", default=None)
ap.add_argument("--keep", default=None)
ap.add_argument("--unrolled", action="store_true")
ap.add_argument("--list", action="store_true")
args = ap.parse_args()

tmp = tempfile.mkdtemp()
out = args.asm or args.keep or os.path.join(tmp, "loop.s")
if not args.asm:
    if args.c == 16:
        src = os.path.join(args.csrc, "lp_renderer_mfma_bwd.hip")
    else:
        src = os.path.join(tmp, "one_c32.hip")
        with open(src, "w") as f:
            f.write('#include "lp_renderer_mfma_bwd.h"\nnamespace lp { int one_c32(const LpRendererArgs& a, const MfmaParams& mp, hipStream_t s) '
                    "{ return launch_bwd3w<32, GM_TRIPLANE, true, 3, 4>(a, mp, s); } }\n")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + B.FLAGS + B.FILE_FLAGS["lp_renderer_mfma_bwd.hip"] + \
        ["-DLP_DEV_ONE", "-DLP_ASM_MARKS", "-I", args.csrc, "-S", "--cuda-device-only", src, "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
lines = open(out).read().splitlines()
start = next(i for i, l in enumerate(lines) if l.startswith(f"_ZN2lp16renderer_bwd_bf3ILi{args.c}ELi1ELb1ELi3ELi4ELb0E") and ":" in l)
end = next(i for i in range(start, len(lines)) if "s_endpgm" in lines[i])
body = lines[start:end]
labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
loops = []
for i, l in enumerate(body):
    m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
    if m and m.group(1) in labels and labels[m.group(1)] < i:
        loops.append((labels[m.group(1)], i))
a, b = max(loops, key=lambda x: x[1] - x[0])
inner = sorted((x, y) for x, y in loops if a < x and y < b)
# the quadrant rounds where they are loops: short inner loops whose only MFMAs are v_mfma_f32_16x16x32_bf16
quad = [(x, y) for x, y in inner if any("v_mfma_f32_16x16x32" in l for l in body[x:y + 1]) and not any("v_mfma_f32_32x32" in l for l in body[x:y + 1]) and y - x < 80]

BINS = ((0, 16, "< 16"), (16, 32, "16-31"), (32, 64, "32-63"), (64, 1 << 30, ">= 64"))


def walk(seg, mark0="head"):
    """-> (per-mark {bin: n, 'store-only': n, 'waits': n, 'reads': n}, list of (mark, distance, read opcode))."""
    clock, fifo, cur = 0, [], mark0   # fifo: (issue clock, opcode, is_read) of the outstanding lgkm instructions, oldest first
    per, events = collections.OrderedDict(), []

    def rec(k):
        return per.setdefault(k, collections.Counter())
    for l in seg:
        m = re.search(r"; LPMARK (\w+)", l)
        if m:
            cur = m.group(1)
            continue
        t = l.strip()
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        op = re.split(r"\s", t)[0]
        if op.startswith("ds_") or op.startswith(("s_load", "s_buffer_load")):
            is_read = op.startswith(("ds_read", "ds_load", "s_load", "s_buffer_load"))
            fifo.append((clock, op, is_read))
            if op.startswith("ds_read") or op.startswith("ds_load"):
                rec(cur)["reads"] += 1
            clock += 4
        elif op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", t)
            if m or re.fullmatch(r"s_waitcnt\s+0(x0)?", t):
                n = int(m.group(1)) if m else 0
                done, fifo = fifo[:max(len(fifo) - n, 0)], fifo[max(len(fifo) - n, 0):]
                reads = [x for x in done if x[2]]
                if reads:
                    d = clock - reads[-1][0] - 4   # issue cycles between the end of the read's issue and the wait
                    rec(cur)["waits"] += 1
                    rec(cur)[next(name for lo, hi, name in BINS if lo <= d < hi)] += 1
                    events.append((cur, d, reads[-1][1]))
                elif done:
                    rec(cur)["store-only"] += 1
        elif op.startswith("v_mfma"):
            clock += 8
        elif op.startswith("v_") or op == "s_nop":
            clock += 4
    return per, events


def table(per):
    print(f"  {'phase':12s} {'ds reads':>8s} {'waits':>6s} " + " ".join(f"{n:>6s}" for _, _, n in BINS) + "  store-only")
    tot = collections.Counter()
    for k, c in per.items():
        tot.update(c)
        print(f"  {k:12s} {c['reads']:8d} {c['waits']:6d} " + " ".join(f"{c[n]:6d}" for _, _, n in BINS) + f"  {c['store-only']:6d}")
    print(f"  {'loop':12s} {tot['reads']:8d} {tot['waits']:6d} " + " ".join(f"{tot[n]:6d}" for _, _, n in BINS) + f"  {tot['store-only']:6d}")


loop = body[a:b + 1]
n_wait = sum(1 for l in loop if l.strip().startswith("s_waitcnt"))
n_lgkm0 = sum(1 for l in loop if re.search(r"s_waitcnt.*lgkmcnt\(0\)", l))
print(f"kernel renderer_bwd_bf3<{args.c}, 1, true, 3, 4>, csrc {os.path.relpath(args.csrc, os.path.dirname(HERE))}: sample loop = lines {a}..{b} of the kernel, "
      f"{n_wait} s_waitcnt ({n_lgkm0} lgkmcnt(0)), {len(quad)} quadrant loop(s)")
print("waits on LDS reads by issue-cycle distance to the youngest read waited for (4 cycles per VALU / LDS / s_nop, 8 per MFMA):")
per, events = walk(loop)
table(per)
imm = collections.Counter()
for mk, d, op in events:
    if d < 16:
        imm[(mk, op)] += 1
print("  immediate (< 16) by phase and read: " + ", ".join(f"{mk} {op} x{n}" for (mk, op), n in sorted(imm.items())))
if args.unrolled:
    for x, y in quad:
        mk = "head"
        for l in body[a:x]:
            m = re.search(r"; LPMARK (\w+)", l)
            if m:
                mk = m.group(1)
        n_mfma = sum(1 for l in body[x:y + 1] if l.strip().startswith("v_mfma"))
        print(f"quadrant loop at lines {x}..{y} (the scheduler places it in phase {mk}; {n_mfma} MFMA per iteration), ONE iteration:")
        p, _ = walk(body[x:y + 1], mk)
        table(p)
    if not quad:
        print("no inner loop: the quadrant rounds are unrolled and part of the table above")
if args.list:
    for mk, d, op in events:
        print(f"  {mk:12s} {d:5d}  {op}")
