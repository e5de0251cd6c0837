#!/usr/bin/env python3
"""Host enqueue cost of the small kernel families, and bench.py's headline, on this tree's library against the parent commit's library
(NOCF_LIB_PATH), alternating in one run on the MI355X.

Enqueue cost: one lane shape (swap2: d = 4, m = 16) and one one-CU shape (singlequad: d = 12, m = 128) at n = 64 and --nt steps -- rollouts
so short that the host's work per call (the binding, the argument checks, the kernel pick, the launches) is what the wall clock sees.
--calls OCflow evaluation calls back to back, then one synchronise; wall time per call.  One child process per library and repetition
(the library is chosen when the process starts), both shapes in it; --reps repetitions each, parent and this tree alternating.
bench.py (swarm50: the split-role kernel) runs the same way, --bench-runs times each.

The parent in the same run is the only yardstick.  Required: this tree's median enqueue cost is not above the parent's largest
repetition; this tree's median bench.py value lies inside the parent's smallest-to-largest range, and Jc is the same.

    python tools/dispatch_time.py --parent PATH/libnocf.so [--reps 5] [--calls 2000] [--bench-runs 5] [--out profiles/dispatch]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from disturb_time import load                               # noqa: E402

SHAPES = ["swap2", "singlequad"]
N = 64


def child(calls, nt):
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib
    dev = torch.device("cuda:0")
    out = {}
    for name in SHAPES:
        net, prob, x, meta = load(name, N, dev)
        alph = meta["alph"]
        with torch.no_grad():
            for _ in range(50):
                na.OCflow(x, net, prob, [0.0, 1.0], nt, "rk4", alph)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                na.OCflow(x, net, prob, [0.0, 1.0], nt, "rk4", alph)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        na.check_errors(sync=True)
        out[name] = {"us_per_call": 1e6 * (t1 - t0) / calls, "kernel": _lib.lib().nocf_last_rollout_kernel().decode(),
                     "d": x.shape[1], "m": meta["m"]}
    print("RESULT " + json.dumps(out), flush=True)


def run(argv, lib, tag):
    env = dict(os.environ, NOCF_JIT="0")
    env.pop("NOCF_LIB_PATH", None)
    if lib:
        env["NOCF_LIB_PATH"] = os.path.abspath(lib)
    r = subprocess.run([sys.executable] + argv, env=env, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{tag} failed with exit status {r.returncode}")
    print("[dispatch_time] %s done" % tag, file=sys.stderr, flush=True)
    return r.stdout


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--parent", default=None, metavar="PATH", help="the parent commit's libnocf.so")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--calls", type=int, default=2000)
    p.add_argument("--nt", type=int, default=4)
    p.add_argument("--bench-runs", type=int, default=5)
    p.add_argument("--bench-steps", type=int, default=200)
    p.add_argument("--bench-warmup", type=int, default=20)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "dispatch"))
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        return child(args.calls, args.nt)
    if not args.parent or not os.path.exists(args.parent):
        raise SystemExit("--parent: the parent commit's libnocf.so is required")
    libs = (("parent", args.parent), ("this", None))
    enq = {tag: [] for tag, _ in libs}
    for _ in range(args.reps):
        for tag, lib in libs:
            o = run([os.path.abspath(__file__), "--child", "--calls", str(args.calls), "--nt", str(args.nt)], lib, "enqueue (%s)" % tag)
            enq[tag].append(json.loads([ln for ln in o.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    lines = ["host enqueue cost: %d OCflow evaluation calls back to back (n = %d, nt = %d, rk4), one synchronise; us per call, median of %d "
             "repetitions [smallest, largest], libraries alternating" % (args.calls, N, args.nt, args.reps),
             "%-11s %3s %4s  %-22s %26s %26s  %s" % ("shape", "d", "m", "kernel", "parent", "this tree", "this median <= parent largest")]
    ok = True
    for name in SHAPES:
        v = {tag: [r[name]["us_per_call"] for r in enq[tag]] for tag in enq}
        met = statistics.median(v["this"]) <= max(v["parent"])
        ok = ok and met and all(r[name]["kernel"] == enq["parent"][0][name]["kernel"] for tag in enq for r in enq[tag])
        r0 = enq["this"][0][name]
        lines.append("%-11s %3d %4d  %-22s %26s %26s  %s" % (
            name, r0["d"], r0["m"], r0["kernel"],
            *("%8.2f [%.2f, %.2f]" % (statistics.median(v[t]), min(v[t]), max(v[t])) for t in ("parent", "this")), "met" if met else "NOT MET"))
    if args.bench_runs > 0:
        runs = {tag: [] for tag, _ in libs}
        for _ in range(args.bench_runs):
            for tag, lib in libs:
                o = run([os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup)],
                        lib, "bench.py (%s)" % tag)
                runs[tag].append(json.loads([ln for ln in o.splitlines() if ln.startswith("{")][-1]))
        b0 = runs["this"][0]
        lines += ["", "bench.py --gpus 1 --steps %d --warmup %d, %d runs each, alternating (%s, %s, kernel %s):" %
                  (args.bench_steps, args.bench_warmup, args.bench_runs, b0.get("metric", "value"), b0.get("unit", ""),
                   b0.get("roofline", {}).get("kernel", "?"))]
        v = {tag: [float(b["value"]) for b in runs[tag]] for tag in runs}
        jc = {tag: sorted({b["config"]["Jc"] for b in runs[tag]}) for tag in runs}
        for tag in ("parent", "this"):
            lines.append("    %-6s library: median %.1f [%.1f, %.1f]   Jc %s" % (tag, statistics.median(v[tag]), min(v[tag]), max(v[tag]),
                                                                            ", ".join("%.9e" % j for j in jc[tag])))
        inside = min(v["parent"]) <= statistics.median(v["this"]) <= max(v["parent"])
        lines.append("    this / parent = %.4f; this median inside the parent's range: %s; Jc identical: %s" %
                     (statistics.median(v["this"]) / statistics.median(v["parent"]), "yes" if inside else "NO",
                      "yes" if jc["this"] == jc["parent"] and len(jc["this"]) == 1 else "NO"))
        ok = ok and inside and jc["this"] == jc["parent"] and len(jc["this"]) == 1
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "dispatch_time.txt"), "w") as f:
        f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
