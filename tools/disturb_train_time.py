#!/usr/bin/env python3
"""Time one Adam iteration of training through disturbed rollouts (neuraloc_amd.disturbed_ocflow_train) on the MI355X, against the
undisturbed training call, for one workload per kernel family:
  * softcorridor n = 1024 nt = 50 (lane kernels), singlequad n = 1024 nt = 50 (one-CU kernels), swarm50 n = 1024 nt = 80 (per-tile kernels);
  * "same": OCflow + backward on the SAME kernels (NOCF_DUO=0 for swarm50: a disturbed call never takes the split-role kernel);
  * "default": the undisturbed path a user gets without a knob (swarm50: the split-role kernel and its tape adjoint; elsewhere it is "same").
An iteration is zero_grad, the training call, Jc.backward() and Adam's step, as trainOC.py runs it, with W drawn once outside the timed
region (the draw, which trainOC.py --noise repeats every iteration, is timed on its own: draw_ms).  A repeat is --warmup iterations and then
--iters iterations inside one HIP event pair; the legs alternate within a repeat and there are --repeats of them.  Each kernel choice
runs in a child process of its own, because the library reads its NOCF_* knobs once.

    python tools/disturb_train_time.py [--iters 20] [--warmup 5] [--repeats 3] [--out profiles/disturb]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.disturb_time import load                                   # noqa: E402  (the fixtures' networks, problems and batches)

# (fixture, nt, n, family)
WORKLOADS = [("softcorridor", 50, 1024, "lane"), ("singlequad", 50, 1024, "one-CU"), ("swarm50", 80, 1024, "per-tile")]


def child(name, nt, n, iters, warmup, repeats, legs):
    import torch
    import neuraloc_amd as na
    from neuraloc_amd import _lib
    dev = torch.device("cuda:0")
    net, prob, x, meta = load(name, n, dev)
    net.train()
    prob.train()
    alph, d = meta["alph"], x.shape[1]
    W = na.brownian_disturbances(nt, n, d, 0.05 * float(meta["r"]), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    optim = torch.optim.Adam(net.parameters(), lr=1e-5)
    kernels = {}

    def iteration(leg):
        optim.zero_grad()
        if leg == "disturbed":
            Jc, _ = na.disturbed_ocflow_train(x, net, prob, [0.0, 1.0], nt, W, "rk4", alph)
        else:
            Jc, _ = na.OCflow(x, net, prob, [0.0, 1.0], nt, "rk4", alph)
        if leg not in kernels:
            kernels[leg] = [_lib.lib().nocf_last_rollout_kernel().decode()]
        Jc.backward()
        if len(kernels[leg]) == 1:
            kernels[leg].append(_lib.lib().nocf_last_rollout_kernel().decode())
        optim.step()

    ms = {leg: [] for leg in legs}
    for _ in range(repeats):
        for leg in legs:
            for _ in range(warmup):
                iteration(leg)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                iteration(leg)
            e1.record()
            e1.synchronize()
            na.check_errors(sync=True)
            ms[leg].append(e0.elapsed_time(e1) / iters)
    g = torch.Generator(device=dev).manual_seed(3)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        na.brownian_disturbances(nt, n, d, 0.05, generator=g, device=dev)
    e1.record()
    e1.synchronize()
    out = {"name": name, "nt": nt, "n": n, "d": d, "m": meta["m"], "NOCF_DUO": os.environ.get("NOCF_DUO", "1"), "iters": iters,
           "warmup": warmup, "ms_per_iteration": ms, "kernels": kernels, "draw_ms": e0.elapsed_time(e1) / iters}
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, name, nt, n, duo, legs):
    env = dict(os.environ, NOCF_JIT="0")
    if duo is not None:
        env["NOCF_DUO"] = duo
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--iters", str(args.iters), "--warmup", str(args.warmup), "--repeats",
                        str(args.repeats), "--child", name, str(nt), str(n), ",".join(legs)], env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{name} (NOCF_DUO={duo}) failed with exit status {r.returncode}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=3)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "disturb"))
    p.add_argument("--child", nargs=4, default=None, help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.child:
        return child(args.child[0], int(args.child[1]), int(args.child[2]), args.iters, args.warmup, args.repeats, args.child[3].split(","))
    rows = []
    for name, nt, n, family in WORKLOADS:
        wide = name == "swarm50"
        a = run_child(args, name, nt, n, "0" if wide else None, ["disturbed", "same"])
        row = {"name": name, "family": family, "nt": nt, "n": n, "m": a["m"], "iters": args.iters, "warmup": args.warmup,
               "disturbed_ms": a["ms_per_iteration"]["disturbed"], "same_ms": a["ms_per_iteration"]["same"],
               "disturbed_kernels": a["kernels"]["disturbed"], "same_kernels": a["kernels"]["same"], "draw_ms": a["draw_ms"]}
        if wide:
            b = run_child(args, name, nt, n, "1", ["same"])
            row["default_ms"], row["default_kernels"] = b["ms_per_iteration"]["same"], b["kernels"]["same"]
        else:
            row["default_ms"], row["default_kernels"] = row["same_ms"], row["same_kernels"]
        # per repeat: disturbed over undisturbed; the spread is the largest minus the smallest of the repeats' ratios
        rs = [dv / sv for dv, sv in zip(row["disturbed_ms"], row["same_ms"])]
        rd = [dv / sv for dv, sv in zip(row["disturbed_ms"], row["default_ms"])]
        row["ratio_same"], row["ratio_same_spread"] = statistics.median(rs), max(rs) - min(rs)
        row["ratio_default"], row["ratio_default_spread"] = statistics.median(rd), max(rd) - min(rd)
        rows.append(row)
        print("%s: disturbed / same kernels %.3f, disturbed / default %.3f" % (name, row["ratio_same"], row["ratio_default"]), flush=True)
    lines = ["%-13s %-8s %5s %3s  %-30s %-30s %-30s %9s %9s %8s" % (
        "workload", "family", "n", "nt", "disturbed ms/iter (repeats)", "same kernels ms/iter", "default path ms/iter", "dist/same", "dist/dflt", "draw ms")]

    def cell(v):
        return " ".join("%.3f" % t for t in v)
    for r in rows:
        lines.append("%-13s %-8s %5d %3d  %-30s %-30s %-30s %5.3f+-%.3f %5.3f+-%.3f %8.3f" % (
            r["name"], r["family"], r["n"], r["nt"], cell(r["disturbed_ms"]), cell(r["same_ms"]), cell(r["default_ms"]),
            r["ratio_same"], r["ratio_same_spread"], r["ratio_default"], r["ratio_default_spread"], r["draw_ms"]))
        lines.append("    forward / adjoint: disturbed %s, same %s, default %s" % (
            " / ".join(r["disturbed_kernels"]), " / ".join(r["same_kernels"]), " / ".join(r["default_kernels"])))
    text = "\n".join(lines)
    print(text)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "disturb_train_time.txt"), "w") as f:
        f.write(text + "\n")
    with open(os.path.join(args.out, "disturb_train_time.json"), "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
