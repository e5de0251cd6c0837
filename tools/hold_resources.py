"""Resource table of the zero-order-hold instantiations (HOLD) from a gfx950 code object -- no GPU and no
recompilation: every new instantiation (HOLD with DIST 0 and 1, on the 6 lane and the 7 one-CU shapes) beside its sibling without HOLD; and,
given the parent commit's code object too, every kernel the two builds share compared twice -- its figures in the metadata, and its
instruction text per kernel (llvm-objdump, comments and encodings dropped).  rollout_lane_kernel and rollout_mono_kernel gained a trailing
template parameter (HOLD = false) and a trailing kernel argument; an instantiation without HOLD keeps the spelling it had in the parent
(ensemble_minmax_resources.spelling), so the two builds' kernels are matched by their demangled names; a text that differs only in the
immediate offsets of scalar loads is counted as "the same up to kernel-argument offsets".

    llvm-objcopy --dump-section .hip_fatbin=fat.bin neuraloc_amd/csrc/obj/nocf_kernels.o
    clang-offload-bundler --unbundle --type=o --input=fat.bin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=kernels.co
    python tools/hold_resources.py kernels.co [parent.co] > profiles/hold/hold_resources.txt

Columns: VGPRs, AGPRs, SGPRs, scratch [bytes/lane], occupancy [waves/SIMD], SGPR spills, VGPR spills.
Required (exit status 1 otherwise): no existing instantiation changes a register count or gains scratch; no new instantiation has scratch
or a spilled VGPR."""
import os
import re
import shutil
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ensemble_minmax_resources import _tool, fmt, kernels, spelling   # noqa: E402
from noise_corr_resources import LANE, MONO, _LOAD          # noqa: E402


def texts(path):
    """demangled kernel name (no argument list) -> list of instruction lines (no addresses, encodings or comments)"""
    dis = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", path], capture_output=True, text=True,
                         check=True).stdout
    out, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^<(\S+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln.startswith("\t"):
            cur.append(ln.split("//")[0].rstrip())
    syms = list(out)
    plain = subprocess.run([shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "c++filt"], input="\n".join(syms), capture_output=True,
                           text=True, check=True).stdout.split("\n")
    return {spelling(p): out[s] for p, s in zip(plain, syms)}


def main(argv):
    K = kernels(argv[1])
    table = []
    for a, b in LANE:
        for dist in (0, 1):
            table.append(("rollout_lane_kernel<%d, %d, false, false, %d, false, true>" % (a, b, dist),
                          "rollout_lane_kernel<%d, %d, false, false, %d, false>" % (a, b, dist)))
    for a, b in MONO:
        for dist in (0, 1):
            table.append(("rollout_mono_kernel<%d, %d, false, %d, false, true>" % (a, b, dist),
                          "rollout_mono_kernel<%d, %d, false, %d, false>" % (a, b, dist)))
    print("%d kernels in %s" % (len(K), argv[1]))
    bad = 0
    if len(argv) > 2:
        P = kernels(argv[2])
        differ = [k for k in P if k in K and K[k] != P[k]]
        print("%d kernels in %s; figures: %d of them the same in both, %d differ, %d are gone; %d are new" %
              (len(P), argv[2], sum(1 for k in P if K.get(k) == P[k]), len(differ), sum(1 for k in P if k not in K), sum(1 for k in K if k not in P)))
        for k in differ:
            worse = any(K[k][i] != P[k][i] for i in (0, 1, 2)) or K[k][3] > P[k][3]
            bad += worse
            print("  figures differ: %-60s %s | parent %s%s" % (k, fmt(K[k]), fmt(P[k]), "  <-- a register count changed or scratch grew" if worse else ""))
        tn, tp = texts(argv[1]), texts(argv[2])
        same = offs = 0
        other = []
        for sym, body in tp.items():
            if sym not in tn:
                continue
            if tn[sym] == body:
                same += 1
            elif [_LOAD.sub(r"\1#\2", x) for x in tn[sym]] == [_LOAD.sub(r"\1#\2", x) for x in body]:
                offs += 1
            else:
                other.append(sym)
        print("instruction text of the %d shared kernels: %d identical, %d the same up to the immediate offsets of scalar loads (kernel-argument "
              "offsets), %d differ otherwise" % (same + offs + len(other), same, offs, len(other)))
        # what is left are constants the linker and the module-wide passes fix: pc-relative displacements of calls and of constant data
        # (s_add_u32 / s_addc_u32 with a literal), the kernel-argument size in the implicit-argument pointer, and the kernel's number in the
        # LDS lookup table of non-inlined callees (s_mov_b32 s15, N), which shifts when kernels are added in front of it
        for sym in other:
            a, b = tn[sym], tp[sym]
            ops = sorted({x.split()[0] for x, y in zip(a, b) if x != y}) if len(a) == len(b) else ["(length)"]
            print("  text differs: %s (%d instructions, parent %d): in %s" % (sym, len(a), len(b), " ".join(ops)))
    print()
    print("%-72s %-34s | %-34s" % ("kernel", "HOLD: V A S scr occ sS vS", "sibling without HOLD"))
    for new, sib in table:
        r, rs = K.get(new), K.get(sib)
        flag = ""
        if r is None:
            flag, bad = "  <-- MISSING", bad + 1
        elif r[3] or r[6]:
            flag, bad = "  <-- scratch / spilled VGPRs", bad + 1
        elif rs and r[4] < rs[4]:
            flag = "  (occupancy below the sibling's)"
        print("%-72s %s | %s%s" % (new, fmt(r), fmt(rs), flag))
    print()
    print("%d findings against the two requirements" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
