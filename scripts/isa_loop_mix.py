#!/usr/bin/env python
"""Static instruction mix of the sample loop of the tuned Renderer backward (renderer_bwd_bf3<C, triplane, PLAIN, 3 colours, four
waves>): VALU, v_mov, v_cndmask + v_cmp, address arithmetic, scratch-in-loop, VGPR / SGPR.  Compiles ONE instantiation with the build's
own flags (-DLP_DEV_ONE; C = 32 through a two-line translation unit written next to the output).  No GPU needed.
    python scripts/isa_loop_mix.py [--c 16|32] [--marks] [--csrc DIR] [--keep FILE.s]
--marks adds -DLP_ASM_MARKS and prints the mix per phase of the loop (the marks are comments: the code is the same).
--csrc compiles another checkout's lightplane_amd/csrc (parent against new)."""
import argparse, collections, os, re, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__)); sys.path.insert(0, os.path.dirname(HERE))
from lightplane_amd.csrc import build as B

ap = argparse.ArgumentParser()
ap.add_argument("--c", type=int, default=16)
ap.add_argument("--marks", action="store_true")
ap.add_argument("--csrc", default=B.HERE)
ap.add_argument("--keep", default=None)
ap.add_argument("--top", type=int, default=0, help="also list the N most frequent opcodes of the loop")
args = ap.parse_args()

tmp = tempfile.mkdtemp()
out = args.keep or os.path.join(tmp, "loop.s")
if args.c == 16:
    src = os.path.join(args.csrc, "lp_renderer_mfma_bwd.hip")
else:
    src = os.path.join(tmp, "one_c32.hip")
    with open(src, "w") as f:
        f.write('#include "lp_renderer_mfma_bwd.h"\nnamespace lp { int one_c32(const LpRendererArgs& a, const MfmaParams& mp, hipStream_t s) '
                "{ return launch_bwd3w<32, GM_TRIPLANE, true, 3, 4>(a, mp, s); } }\n")
cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + B.FLAGS + B.FILE_FLAGS["lp_renderer_mfma_bwd.hip"] + ["-DLP_DEV_ONE", "-I", args.csrc]
if args.marks:
    cmd.append("-DLP_ASM_MARKS")
cmd += ["-S", "--cuda-device-only", src, "-o", out]
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


def meta(key):
    return next(l.split()[-1] for l in lines[end:] if key in l)


ADDR = ("v_add_u32", "v_sub_u32", "v_lshl_add_u64", "v_lshl_add_u32", "v_add_lshl_u32", "v_or3_b32", "v_add3_u32", "v_mul_lo_u32", "v_mad_u32_u24",
        "v_mad_u64_u32", "v_mad_i64_i32", "v_lshlrev_b32", "v_lshlrev_b64", "v_add_co_u32", "v_addc_co_u32", "v_lshl_or_b32", "v_and_or_b32", "v_mul_u32_u24", "v_ashrrev_i32")


def mix(seg):
    ops = collections.Counter()
    for l in seg:
        t = l.strip()
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        ops[re.split(r"[\s]", t)[0]] += 1
    n = sum(ops.values())
    valu = sum(v for k, v in ops.items() if k.startswith("v_") and not k.startswith("v_mfma"))
    base = lambda k: re.sub(r"_(e32|e64|sdwa|dpp)$", "", k)
    mov = sum(v for k, v in ops.items() if base(k) == "v_mov_b32")
    cnd = sum(v for k, v in ops.items() if k.startswith("v_cndmask"))
    cmp_ = sum(v for k, v in ops.items() if k.startswith("v_cmp"))
    addr = sum(v for k, v in ops.items() if base(k) in ADDR)
    mfma = sum(v for k, v in ops.items() if k.startswith("v_mfma"))
    scr = sum(v for k, v in ops.items() if k.startswith("scratch_"))
    return dict(all=n, valu=valu, v_mov=mov, v_cndmask=cnd, v_cmp=cmp_, addr=addr, mfma=mfma, scratch=scr), ops


loop = body[a:b + 1]
tot, ops = mix(loop)
zero_mov = sum(1 for l in loop if re.match(r"\s*v_mov_b32(_e32)?\s+v\d+, 0\s*$", l))
print("command:", " ".join(c for c in cmd[:-4] if not c.startswith(tmp)), "...")
print(f"kernel renderer_bwd_bf3<{args.c}, 1, true, 3, 4>: vgpr {meta('.vgpr_count')} agpr {meta('.agpr_count')} sgpr {meta('.sgpr_count')} "
      f"scratch frame {meta('private_segment_fixed_size')} B, vgpr spills {meta('.vgpr_spill_count')}")
print(f"sample loop = lines {a}..{b} of the kernel")
print("loop: " + "  ".join(f"{k} {v}" for k, v in tot.items()) + f"  (v_mov of literal 0: {zero_mov})")
if args.marks:
    cur, segs = "head", collections.OrderedDict()
    for l in loop:
        m = re.search(r"; LPMARK (\w+)", l)
        if m:
            cur = m.group(1)
            continue
        segs.setdefault(cur, []).append(l)
    for k, seg in segs.items():
        t, _ = mix(seg)
        print(f"  {k:12s} " + "  ".join(f"{kk} {v}" for kk, v in t.items()))
if args.top:
    for k, v in ops.most_common(args.top):
        print(f"  {v:5d} {k}")
