"""Resource table of the adversarial-ensemble kernel instantiations from a gfx950 code object's metadata -- no GPU
and no recompilation: every new instantiation beside its ENS sibling without W / lamW and its single-network sibling with it.

    llvm-objcopy --dump-section .hip_fatbin=fat.bin neuraloc_amd/csrc/obj/nocf_kernels.o
    clang-offload-bundler --unbundle --type=o --input=fat.bin --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --output=kernels.co
    python tools/ensemble_minmax_resources.py kernels.co [parent.co] > profiles/ensemble_minmax/ensemble_minmax_resources.txt

parent.co: the same code object of the parent commit; every kernel it has is then compared with this build's, field by field.
Columns: VGPRs, AGPRs, SGPRs, scratch [bytes/lane], occupancy [waves/SIMD: 512 unified registers over the kernel's total, which the metadata
gives as .vgpr_count and which is allocated in eights], SGPR spills, VGPR spills."""
import re
import shutil
import subprocess
import sys

FIELDS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".sgpr_spill_count", ".vgpr_spill_count")


def _tool(name):
    return shutil.which(name) or "/opt/rocm/llvm/bin/" + name


# rollout_lane_kernel / rollout_mono_kernel gained a trailing template parameter HOLD; an instantiation without it
# keeps the spelling it had before, so this table and its siblings' (tools/noise_corr_resources.py) still name it
_HOLD_OFF = re.compile(r"^(rollout_lane_kernel<(?:[^,<>]+, ){5}[^,<>]+|rollout_mono_kernel<(?:[^,<>]+, ){4}[^,<>]+), false>$")


def spelling(name):
    """the demangled kernel name without its argument list, HOLD = false dropped"""
    name = re.sub(r"^void |\(.*$", "", name)
    m = _HOLD_OFF.match(name)
    return m.group(1) + ">" if m else name


def kernels(path):
    """demangled kernel name -> (V, A, S, scratch, occupancy, sS, vS)"""
    text = subprocess.run([_tool("llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
    text = text.split("amdhsa.kernels:")[1].split("amdhsa.target:")[0]
    blocks = re.split(r"\n\s+- \.agpr_count:", "\n" + text)[1:]
    names, rows = [], []
    for blk in blocks:
        blk = ".agpr_count:" + blk
        get = lambda key: int(re.search(r"(?m)^\s*" + re.escape(key) + r":\s*(\d+)", blk).group(1))      # noqa: E731
        v, a, s, scr, ss, vs = (get(k) for k in FIELDS)
        total = -(-v // 8) * 8                                       # (.vgpr_count is the unified total: architectural VGPRs + AGPRs)
        names.append(re.search(r"(?m)^\s*\.name:\s*(\S+)", blk).group(1))
        rows.append((v - a, a, s, scr, min(8, 512 // max(total, 8)), ss, vs))
    plain = subprocess.run([shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {spelling(p): r for p, r in zip(plain, rows)}


def fmt(r):
    return "%4d %4d %4d %4d %4d %4d %4d" % r if r else "   (absent)".ljust(34)


def main(argv):
    K = kernels(argv[1])
    lane, mono_f, mono_b = [(16, 8), (16, 16), (16, 32), (32, 8), (32, 16), (32, 32)], [(8, 1), (6, 1), (4, 1), (2, 1), (8, 2), (6, 2), (4, 2)], \
        [(8, 1), (6, 1), (4, 1), (8, 2), (6, 2), (4, 2)]
    tf = lambda b: "true" if b else "false"      # noqa: E731
    table = []
    for rec in (False, True):
        for a, b in lane:
            table.append(("rollout_lane_kernel<%d, %d, %s, false, 1, true>" % (a, b, tf(rec)),
                          "rollout_lane_kernel<%d, %d, %s, false, 0, true>" % (a, b, tf(rec)),
                          "rollout_lane_kernel<%d, %d, %s, false, 1, false>" % (a, b, tf(rec))))
    for rec in (False, True):
        for a, b in mono_f:
            table.append(("rollout_mono_kernel<%d, %d, %s, 1, true>" % (a, b, tf(rec)), "rollout_mono_kernel<%d, %d, %s, 0, true>" % (a, b, tf(rec)),
                          "rollout_mono_kernel<%d, %d, %s, 1, false>" % (a, b, tf(rec))))
    for mode in (2, 1):
        for a, b in lane:
            table.append(("rollout_lane_bwd_kernel<%d, %d, %d, true, false>" % (a, b, mode), "rollout_lane_bwd_kernel<%d, %d, 0, true, false>" % (a, b),
                          "rollout_lane_bwd_kernel<%d, %d, %d, false, false>" % (a, b, mode)))
    for mode in (2, 1):
        for a, b in mono_b:
            table.append(("rollout_mono_bwd_kernel<%d, %d, %d, true, false>" % (a, b, mode), "rollout_mono_bwd_kernel<%d, %d, 0, true, false>" % (a, b),
                          "rollout_mono_bwd_kernel<%d, %d, %d, false, false>" % (a, b, mode)))
    table.append(("disturbance_ascent_ens_kernel", None, "disturbance_ascent_kernel"))
    print("%d kernels in %s" % (len(K), argv[1]))
    if len(argv) > 2:
        P = kernels(argv[2])
        same = [k for k in P if K.get(k) == P[k]]
        print("%d kernels in %s; %d of them carry the same figures in both, %d differ, %d are gone; %d are new" %
              (len(P), argv[2], len(same), sum(1 for k in P if k in K and K[k] != P[k]), sum(1 for k in P if k not in K),
               sum(1 for k in K if k not in P)))
        for k in P:
            if k in K and K[k] != P[k]:
                print("  differs: %-60s %s | parent %s" % (k, fmt(K[k]), fmt(P[k])))
    print()
    print("%-52s %-34s | %-34s | %-34s" % ("kernel", "new: V A S scr occ sS vS", "ENS sibling without W / lamW", "single-network sibling with it"))
    bad = 0
    for new, ens, one in table:
        r, re_, ro = K.get(new), K.get(ens) if ens else None, K.get(one)
        flag = ""
        if r is None:
            flag, bad = "  <-- MISSING", bad + 1
        else:
            sib = [q for q in (re_, ro) if q]
            if (r[3] or r[6]) and all(q[3] == 0 and q[6] == 0 for q in sib):
                flag, bad = "  <-- scratch / spilled VGPRs the siblings do not have", bad + 1
            if re_ and r[4] < re_[4]:
                flag, bad = flag + "  <-- occupancy below the ENS sibling's", bad + 1
        print("%-52s %s | %s | %s%s" % (new, fmt(r), fmt(re_), fmt(ro), flag))
    print()
    print("%d of %d new instantiations flagged" % (bad, len(table)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
