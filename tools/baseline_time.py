#!/usr/bin/env python3
"""Time the direct-transcription baseline solver (neuraloc_amd.solve_baseline: one kernel launch per solve) on the MI355X for the four
point-agent configurations of the reference's timing log (timeDeployment/log_deploy_results, `baseline` blocks: nt = 20, 301 iterations,
the alph of each line), at B = 1 and B = 1024 starts per launch.  HIP events around the launch (the state tensors are allocated
outside); median of --reps launches after --warmup.

Prints a table and writes it with the raw numbers to --out (default profiles/baseline/).

--prec double times the double-precision kernels (float64 tensors) and writes baseline_time_f64.txt / .json beside the fp32 table.

    python tools/baseline_time.py [--reps 5] [--warmup 2] [--prec single|double] [--out profiles/baseline]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import neuraloc_amd as na                                 # noqa: E402

# (problem, alph G / Q / W, seconds per iteration on the reference's Xeon E5-4627 v3 at iteration 300 of its log)
CONFIGS = [("softcorridor", [100.0, 10000.0, 300.0], 0.029039),
           ("swap2", [300.0, 1000000.0, 100000.0], 0.025769),
           ("swap12", [300.0, 0.0, 100000.0], 0.017536),
           ("swarm", [900.0, 10000000.0, 25000.0], 0.040227)]
NT, NITERS = 20, 301


def time_solve(prob, z0, alphG, reps, warmup):
    B, d = z0.shape
    U0 = na.baseline.initial_guess(z0, prob, NT, torch.Generator(device=z0.device).manual_seed(0))
    st = [U0.clone(), torch.zeros_like(U0), torch.zeros_like(U0), torch.full((B,), float("inf"), device=z0.device, dtype=z0.dtype),
          torch.zeros_like(U0)]
    ms = []
    for r in range(warmup + reps):
        st[0].copy_(U0); st[1].zero_(); st[2].zero_(); st[3].fill_(float("inf"))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        na.baseline_adam_steps(z0, *st, prob, alphG, NITERS)
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms, float(st[3].min()), float(st[3].max())


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--prec", choices=["single", "double"], default="single")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "baseline"))
    args = p.parse_args(argv)
    dev = torch.device("cuda:0")
    dtype = torch.float64 if args.prec == "double" else torch.float32
    stem = "baseline_time_f64" if args.prec == "double" else "baseline_time"
    torch.manual_seed(0)
    rows = []
    for name, alph, cpu_s in CONFIGS:
        prob, _, _, xInit = na.initProb(name, 10, 10, var0=1.0, cvt=lambda t: t.to(dtype).to(dev),
                                        alph=[alph[0], alph[1], alph[2], 0.0, 0.0, 0.0])
        prob.train()
        d = xInit.numel()
        for B in (1, 1024):
            z0 = xInit.reshape(1, d) if B == 1 else xInit.reshape(1, d) + torch.randn(B, d, device=dev).to(dtype)
            med, ms, bmin, bmax = time_solve(prob, z0, alph[0], args.reps, args.warmup)
            rows.append(dict(problem=name, d=d, alph=alph, nt=NT, niters=NITERS, B=B, ms_per_solve=med, ms_all=ms,
                             us_per_iter=1e3 * med / NITERS, ms_per_start=med / B, cpu_ms_per_iter=1e3 * cpu_s,
                             best_loss_min=bmin, best_loss_max=bmax))
            print(f"{name:13s} B={B:5d}  {med:9.3f} ms/solve  {1e3 * med / NITERS:8.2f} us/iter  "
                  f"({1e3 * cpu_s:.1f} ms/iter on the reference's CPU, one start)", flush=True)
    for name, _, _ in CONFIGS:
        r1, rB = [r for r in rows if r["problem"] == name]
        print(f"{name:13s} B=1024 / B=1: {rB['ms_per_solve'] / r1['ms_per_solve']:.2f}x the time for 1024x the starts")
    os.makedirs(args.out, exist_ok=True)
    info = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip, reps=args.reps,
                warmup=args.warmup, prec=args.prec, rows=rows)
    with open(os.path.join(args.out, stem + ".json"), "w") as f:
        json.dump(info, f, indent=1)
    with open(os.path.join(args.out, stem + ".txt"), "w") as f:
        f.write("problem        d    B   ms/solve   us/iter  reference CPU ms/iter (one start)\n")
        for r in rows:
            f.write(f"{r['problem']:13s} {r['d']:3d} {r['B']:5d} {r['ms_per_solve']:9.3f} {r['us_per_iter']:9.2f}  {r['cpu_ms_per_iter']:.1f}\n")
    print("wrote", os.path.join(args.out, stem + ".json"))


if __name__ == "__main__":
    main()
