"""Instruction classes per loop of one wf_step_ll_kernel instantiation (no GPU needed): the table-path unit of
wf_kernels_ll.hip (-DWF_LL_PART=1) is compiled to assembly under the Makefile's flags plus the flags given here, and
every loop of the named kernel is listed with its instruction count, VALU, LDS, VMEM, SALU, s_waitcnt and moves.
usage: python tools/isa_loop_classes.py [--kernel MANGLED_SUBSTRING] [--licm] [--min N] [--asm FILE.s] [extra hipcc flags]
  e.g.  python tools/isa_loop_classes.py -DWF_LL_TRANS_WAIT=1
        python tools/isa_loop_classes.py --licm -mllvm -sink-insts-to-avoid-spills
  --licm: leave machine LICM on (the Makefile switches it off for this unit); --asm: read a listing instead of compiling.
A loop is a backward branch to a label; loops are listed outermost first with their nesting depth, and a loop's counts
include the loops inside it.  "moves" (v_mov*, v_accvgpr*, s_mov*) are ALSO counted under VALU / SALU: it counts classes,
nothing else.  The transverse pass of the replay is the innermost loop with 36 ds_read_b128 at two slots (marked)."""
import re
import subprocess
import sys
import tempfile
from pathlib import Path

HEADLINE = "wf_step_ll_kernelILi2ELi2ELb1ELb1ELb1ELi4ELb0ELb0E"  # <2, 2, true, true, true, 4, false, false>


def listing(flags, licm):
    src = Path(__file__).resolve().parents[1] / "wfcrl-env_amd" / "csrc" / "wf_kernels_ll.hip"
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "ll.s"
        cmd = ["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-fno-fast-math", "-ffp-contract=off",
               "-fno-slp-vectorize", "-mllvm", "-amdgpu-sched-strategy=iterative-ilp", "-DWF_LL_PART=1", "-S", "--cuda-device-only",
               "-o", str(out), str(src)] + ([] if licm else ["-mllvm", "-disable-machine-licm"]) + flags
        subprocess.run(cmd, check=True)
        return out.read_text()


def classes(seg):
    c = dict(instr=0, valu=0, lds=0, vmem=0, salu=0, waitcnt=0, moves=0, ds128=0)
    for l in seg:
        t = l.split(";")[0].strip()
        if not t or t.endswith(":") or t.startswith("."):
            continue
        op = t.split()[0]
        c["instr"] += 1
        if op == "s_waitcnt":
            c["waitcnt"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
            c["ds128"] += op == "ds_read_b128"
        elif op.startswith(("global_", "buffer_", "scratch_", "flat_")):
            c["vmem"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        if op.startswith(("v_mov", "v_accvgpr", "s_mov")):
            c["moves"] += 1
    return c


def main(argv):
    kernel, licm, least, asm, flags = HEADLINE, False, 20, None, []
    it = iter(argv)
    for a in it:
        if a == "--kernel": kernel = next(it)
        elif a == "--licm": licm = True
        elif a == "--min": least = int(next(it))
        elif a == "--asm": asm = next(it)
        else: flags.append(a)
    lines = (open(asm).read() if asm else listing(flags, licm)).split("\n")
    i = next(n for n, l in enumerate(lines) if kernel in l and l.split(";")[0].strip().endswith(":") and not l.startswith("."))
    end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
    body = lines[i:end]
    lab = {m.group(1): n for n, l in enumerate(body) if (m := re.match(r"(\.LBB\d+_\d+):", l))}
    loops = set()
    for n, l in enumerate(body):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in lab and lab[m.group(1)] < n:
            loops.add((lab[m.group(1)], n))
    # (two back edges to one header: the longer one is the loop)
    loops = sorted({a: max(b2 for a2, b2 in loops if a2 == a) for a, _ in loops}.items())
    res = {}
    for l in lines:
        for key, pat in (("vgprs", r"\.vgpr_count:\s+(\d+)"), ("spilled", r"\.vgpr_spill_count:\s+(\d+)"), ("scratch", r"\.private_segment_fixed_size:\s+(\d+)")):
            if (m := re.search(pat, l)): res.setdefault(key, []).append(int(m.group(1)))
    tot = classes(body)
    print(f"{lines[i].strip()[:90]}  {tot['instr']} instructions, flags: {' '.join(flags) or '-'}{' (machine LICM on)' if licm else ''}")
    print("loop (lines of the kernel)   depth  instr   VALU    LDS   VMEM   SALU  s_waitcnt  moves")
    for a, b in loops:
        c = classes(body[a:b + 1])
        if c["instr"] < least:
            continue
        depth = sum(a2 <= a and b <= b2 for a2, b2 in loops) - 1
        inner = not any((a2, b2) != (a, b) and a <= a2 and b2 <= b for a2, b2 in loops)
        mark = "  <- transverse pass, two sources" if inner and c["ds128"] >= 36 and c["vmem"] == 0 else ""
        print(f"+{a:6d} .. +{b:6d}          {depth:5d} {c['instr']:6d} {c['valu']:6d} {c['lds']:6d} {c['vmem']:6d} {c['salu']:6d} {c['waitcnt']:10d} {c['moves']:6d}{mark}")


if __name__ == "__main__":
    main(sys.argv[1:])
