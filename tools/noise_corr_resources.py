"""Resource table of the time-correlated-noise instantiations (DIST == 3) from a gfx950 code object -- no GPU and no
recompilation: every new instantiation beside its white-noise sibling (DIST == 2) and its tensor sibling (DIST == 1); and, given the parent
commit's code object too, every kernel the two builds share compared twice -- its figures in the metadata, and its instruction text per
kernel symbol (llvm-objdump, comments and encodings dropped).  RollArgs grew by two pointers, so the arguments behind it moved: a text that
differs only in the immediate offsets of scalar loads is counted as "the same up to kernel-argument offsets".

    llvm-objcopy --dump-section .hip_fatbin=fat.bin neuraloc_amd/csrc/obj/nocf_kernels.o
    clang-offload-bundler --unbundle --type=o --input=fat.bin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=kernels.co
    python tools/noise_corr_resources.py kernels.co [parent.co] > profiles/noise_corr/noise_corr_resources.txt

Columns: VGPRs, AGPRs, SGPRs, scratch [bytes/lane], occupancy [waves/SIMD], SGPR spills, VGPR spills."""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ensemble_minmax_resources import _tool, fmt, kernels   # noqa: E402

LANE = [(16, 8), (16, 16), (16, 32), (32, 8), (32, 16), (32, 32)]
MONO = [(8, 1), (6, 1), (4, 1), (2, 1), (8, 2), (6, 2), (4, 2)]
_LOAD = re.compile(r"^(\s*s_(?:buffer_)?load_dword\S*\s.*,\s*)0x[0-9a-f]+(\s*)$")


def texts(path):
    """mangled kernel symbol -> list of instruction lines (no addresses, encodings or comments)"""
    dis = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", path], capture_output=True, text=True,
                         check=True).stdout
    out, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^<(\S+)>:$", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and ln.startswith("\t"):
            cur.append(ln.split("//")[0].rstrip())
    return out


def main(argv):
    K = kernels(argv[1])
    tf = lambda b: "true" if b else "false"      # noqa: E731
    table = []
    for rec in (False, True):
        for a, b in LANE:
            table.append(tuple("rollout_lane_kernel<%d, %d, %s, false, %d, false>" % (a, b, tf(rec), q) for q in (3, 2, 1)))
    for rec in (False, True):
        for a, b in MONO:
            table.append(tuple("rollout_mono_kernel<%d, %d, %s, %d, false>" % (a, b, tf(rec), q) for q in (3, 2, 1)))
    tile = sorted(k for k in K if k.startswith("rollout_kernel<") and k.endswith(", 3>"))
    for k in tile:
        table.append((k, k[:-2] + "2>", k[:-2] + "1>"))
    table.append(("noise_fill_corr_kernel", "noise_fill_kernel", None))
    print("%d kernels in %s" % (len(K), argv[1]))
    if len(argv) > 2:
        P = kernels(argv[2])
        print("%d kernels in %s; figures: %d of them the same in both, %d differ, %d are gone; %d are new" %
              (len(P), argv[2], sum(1 for k in P if K.get(k) == P[k]), sum(1 for k in P if k in K and K[k] != P[k]),
               sum(1 for k in P if k not in K), sum(1 for k in K if k not in P)))
        for k in P:
            if k in K and K[k] != P[k]:
                print("  figures differ: %-60s %s | parent %s" % (k, fmt(K[k]), fmt(P[k])))
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
        print("instruction text of the %d shared symbols: %d identical, %d the same up to the immediate offsets of scalar loads (kernel-argument "
              "offsets), %d differ otherwise" % (same + offs + len(other), same, offs, len(other)))
        # what is left are constants the linker and the module-wide passes fix: pc-relative displacements of calls and of constant data
        # (s_add_u32 / s_addc_u32 with a literal), the kernel-argument size in the implicit-argument pointer, and the kernel's number in the
        # LDS lookup table of non-inlined callees (s_mov_b32 s15, N), which shifts when kernels are added in front of it
        for sym in other:
            a, b = tn[sym], tp[sym]
            ops = sorted({x.split()[0] for x, y in zip(a, b) if x != y}) if len(a) == len(b) else ["(length)"]
            print("  text differs: %s (%d instructions, parent %d): in %s" % (sym, len(a), len(b), " ".join(ops)))
    print()
    print("%-66s %-34s | %-34s | %-34s" % ("kernel", "DIST == 3: V A S scr occ sS vS", "DIST == 2 (white noise)", "DIST == 1 (tensor)"))
    bad = 0
    for new, white, tens in table:
        r, rw, rt = K.get(new), K.get(white), K.get(tens) if tens else None
        flag = ""
        if r is None:
            flag, bad = "  <-- MISSING", bad + 1
        elif rw and ((r[3] > rw[3]) or (r[6] > rw[6])):
            flag, bad = "  <-- more scratch / spilled VGPRs than the white sibling", bad + 1
        elif rw and r[4] < rw[4]:
            flag, bad = "  <-- occupancy below the white sibling's", bad + 1
        print("%-66s %s | %s | %s%s" % (new, fmt(r), fmt(rw), fmt(rt), flag))
    print()
    print("%d of %d new instantiations flagged" % (bad, len(table)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
