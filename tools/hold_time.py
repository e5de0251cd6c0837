#!/usr/bin/env python3
"""Time the zero-order-hold rollout (nocf_rollout_held_f32: DESIGN.md section 3.19) on the MI355X at n = 1024 and the configs' own nt --
softcorridor and swap12 (lane kernel), singlequad (one-CU kernel) -- for K = 1, 2, 5, 10 against nocf_rollout_means_f32 on the same inputs
in the same process.  tools/disturb_time.py's protocol: the C entry points, with the structs, the workspace and every output buffer made
once outside the HIP event pair; the five legs alternate within a repetition; median of --reps after --warmup, with the smallest and the
largest repetition.  One child process per shape (NOCF_JIT=0: the shipped library).

The yardstick is the evaluation count, no ratio is fixed in advance: the plain call makes 4 nt + 1 network evaluations, the held call
ceil(nt / K) + 1, and both make the same 4 nt physics evaluations.  Per shape the report therefore gives
    t_net   the time per network evaluation the plain call implies: (plain - held(K)) / (4 nt - ceil(nt / K)), for every K
    t_phys  what the held call's remainder says about the physics-only stage: (held(K) - (ceil(nt / K) + 1) t_net) / (4 nt)
and states the one condition: at K = 1 the held call is not slower than the plain call by more than the two legs' spread.

--bench-parent PATH also records bench.py's headline (swarm50, the split-role kernel, whose text this change does not touch) on this
tree's library and on the parent commit's library PATH (NOCF_LIB_PATH), alternating, --bench-runs times each.

    python tools/hold_time.py [--reps 5] [--warmup 2] [--out profiles/hold] [--bench-parent PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disturb_time import load, timed                        # noqa: E402

SHAPES = [("softcorridor", 50, 1024), ("swap12", 20, 1024), ("singlequad", 50, 1024)]
HOLDS = (1, 2, 5, 10)


def child(name, nt, n, reps, warmup):
    import ctypes as C
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib, hold
    from neuraloc_amd.OCflow import _STEPPERS
    dev = torch.device("cuda:0")
    net, prob, x, meta = load(name, n, dev)
    alph = meta["alph"]
    d = x.shape[1]
    out = {"name": name, "nt": nt, "n": n, "d": d, "m": meta["m"]}
    with torch.no_grad(), torch.cuda.device(dev):
        phi_st, keep1, ws = net._c_struct(n)
        prob_st, keep2 = prob._c_struct(dev)
        L = _lib.lib()
        f_held = hold._entry(L)
        persample = torch.empty(n, 7, dtype=torch.float32, device=dev)
        sums = torch.empty(8, dtype=torch.float32, device=dev)
        means = torch.empty(8, dtype=torch.float32, device=dev)
        z_final = torch.empty(n, d + 4, dtype=torch.float32, device=dev)
        alph_c = (C.c_float * 6)(*[float(a) for a in alph[:6]])
        head = (C.byref(phi_st), C.byref(prob_st), _lib.ptr(x))
        tail = (n, 0.0, 1.0, nt, _STEPPERS["rk4"], alph_c, _lib.ptr(z_final), _lib.ptr(persample), _lib.ptr(sums), _lib.ptr(means),
                None, None, _lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_ptr(dev))

        def plain():
            _lib.check(L.nocf_rollout_means_f32(*head, *tail), "nocf_rollout_means_f32")

        def held(K):
            return lambda: _lib.check(f_held(*head, None, K, *tail), "nocf_rollout_held_f32")

        plain()
        out["plain_kernel"] = L.nocf_last_rollout_kernel().decode()
        held(2)()
        out["held_kernel"] = L.nocf_last_rollout_kernel().decode()
        _lib.track_rollout_status(L, dev, "hold_time")
        na.check_errors(sync=True)
        ref = na.held_rollout(x, net, prob, [0.0, 1.0], nt, 2, alph=alph)
        if not (torch.equal(ref[2], persample) and torch.equal(ref[3], z_final)):
            raise SystemExit("the timed call and neuraloc_amd.held_rollout disagree")
        out["held2_LG"] = float(ref[1][0] + alph[0] * ref[1][1])
        res = timed([plain] + [held(K) for K in HOLDS], reps, warmup)
        (out["plain_ms"], out["plain_all"]) = res[0]
        for K, (med, allms) in zip(HOLDS, res[1:]):
            out["held%d_ms" % K], out["held%d_all" % K] = med, allms
        _lib.track_rollout_status(L, dev, "hold_time")
    na.check_errors(sync=True)
    print("RESULT " + json.dumps(out), flush=True)


def bench(lib, steps, warmup):
    env = dict(os.environ, NOCF_JIT="0")
    if lib:
        env["NOCF_LIB_PATH"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                       env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"bench.py failed with exit status {r.returncode}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "hold"))
    p.add_argument("--bench-parent", default=None, metavar="PATH", help="the parent commit's libnocf.so: bench.py's headline on both libraries")
    p.add_argument("--bench-runs", type=int, default=3)
    p.add_argument("--bench-steps", type=int, default=50)
    p.add_argument("--child", nargs=3, default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]), args.reps, args.warmup)
    rows = []
    for name, nt, n in SHAPES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--warmup", str(args.warmup),
                            "--child", name, str(nt), str(n)], env=dict(os.environ, NOCF_JIT="0"), capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"{name} failed with exit status {r.returncode}")
        rows.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))

    def cell(r, k):
        return "%7.3f [%.3f,%.3f]" % (r[k + "_ms"], min(r[k + "_all"]), max(r[k + "_all"]))
    lines = ["median of %d repetitions after %d warm-ups, legs alternating; ms [smallest, largest repetition]" % (args.reps, args.warmup),
             "%-13s %5s %3s  %-30s %-30s %21s " % ("shape", "n", "nt", "plain kernel", "held kernel", "plain (4nt+1 evals)") +
             " ".join("%21s" % ("K=%d" % K) for K in HOLDS)]
    for r in rows:
        lines.append("%-13s %5d %3d  %-30s %-30s %21s " % (r["name"], r["n"], r["nt"], r["plain_kernel"], r["held_kernel"], cell(r, "plain")) +
                     " ".join("%21s" % cell(r, "held%d" % K) for K in HOLDS))
    lines.append("")
    lines.append("evaluation counts: the plain call makes 4 nt + 1 network evaluations, the held call ceil(nt / K) + 1; both make 4 nt physics evaluations")
    for r in rows:
        nt = r["nt"]
        lines.append("%s (nt = %d: plain %d network evaluations):" % (r["name"], nt, 4 * nt + 1))
        for K in HOLDS:
            ne = -(-nt // K) + 1
            t_net = (r["plain_ms"] - r["held%d_ms" % K]) / (4 * nt + 1 - ne)
            t_phys = (r["held%d_ms" % K] - ne * t_net) / (4 * nt)
            lines.append("    K = %2d: %3d network evaluations, held / plain = %.3f; t_net = %.3f us per evaluation implied by the plain call, remainder "
                         "%.3f ms = %.3f us per physics-only stage (launch and terminal block included)" %
                         (K, ne, r["held%d_ms" % K] / r["plain_ms"], 1e3 * t_net, r["held%d_ms" % K] - ne * t_net, 1e3 * t_phys))
        spread = (max(r["plain_all"]) - min(r["plain_all"])) + (max(r["held1_all"]) - min(r["held1_all"]))
        excess = r["held1_ms"] - r["plain_ms"]
        lines.append("    condition at K = 1: held - plain = %+.3f ms, the two legs' spread %.3f ms: %s" %
                     (excess, spread, "met" if excess <= spread else "NOT MET"))
        r["k1_condition_met"] = bool(excess <= spread)
    result = {"shapes": rows}
    if args.bench_parent:
        runs = {"this": [], "parent": []}
        for _ in range(args.bench_runs):
            runs["this"].append(bench(None, args.bench_steps, 5))
            runs["parent"].append(bench(args.bench_parent, args.bench_steps, 5))
        lines.append("")
        lines.append("bench.py --gpus 1 --steps %d --warmup 5, %d runs each, alternating (%s, %s):" %
                     (args.bench_steps, args.bench_runs, runs["this"][0].get("metric", "value"), runs["this"][0].get("unit", "")))
        for tag in ("this", "parent"):
            v = [float(b["value"]) for b in runs[tag]]
            lines.append("    %-6s library: median %.1f [%.1f, %.1f]" % (tag, statistics.median(v), min(v), max(v)))
        vt, vp = (statistics.median([float(b["value"]) for b in runs[t]]) for t in ("this", "parent"))
        lines.append("    this / parent = %.4f" % (vt / vp))
        result["bench"] = {t: [float(b["value"]) for b in runs[t]] for t in runs}
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "hold_time.txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, "hold_time.json"), "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
