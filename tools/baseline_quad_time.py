#!/usr/bin/env python3
"""Time the quadcopter baseline (neuraloc_amd.quad_baseline_loss / solve_baseline_quad) on the MI355X.

  eval   one objective + gradient launch at nt = 20 (the reference's timing log, timeDeployment/log_deploy_results, `baseline` block of
         singlequad: 0.0312 s per L-BFGS iteration on its CPU), B = 1 and B = 1024
  solve  one whole solve at the reference's settings (nt = 50, alphG = 5000, max_iter 16000, max_eval 10000, strong Wolfe,
         tolerance_grad 1e-5, tolerance_change 1e-6, history 100) from xInit (B = 1) and from 1024 starts around it; the time per
         evaluation inside the solve is the launch time over the largest func_evals of the batch

HIP events around the launch; median of --reps launches after --warmup.  Prints a table and writes it with the raw numbers to --out
(default profiles/baseline/).

--prec double times the double-precision kernels (float64 tensors) and writes baseline_quad_time_f64.txt / .json beside the fp32 table.

    python tools/baseline_quad_time.py [--reps 5] [--warmup 2] [--prec single|double] [--out profiles/baseline]
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

CPU_S_PER_ITER = 0.0312
SETTINGS = dict(lr=1., max_iter=16000, max_eval=10000, tolerance_grad=1e-5, tolerance_change=1e-6, history_size=100)


def timed(fn, reps, warmup):
    ms, out = [], None
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms, out


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--prec", choices=["single", "double"], default="single")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "baseline"))
    args = p.parse_args(argv)
    dev = torch.device("cuda:0")
    dtype = torch.float64 if args.prec == "double" else torch.float32
    stem = "baseline_quad_time_f64" if args.prec == "double" else "baseline_quad_time"
    torch.manual_seed(0)
    prob, _, _, xInit = na.initProb("singlequad", 10, 10, var0=1.0, cvt=lambda t: t.to(dtype).to(dev), alph=[5000., 0., 0., 0., 0., 0.])
    rows = []
    for B in (1, 1024):
        z0 = xInit.reshape(1, 12).repeat(B, 1)
        if B > 1:
            z0[:, :3] += torch.randn(B, 3, device=dev).to(dtype)
        U20 = na.quad_initial_guess(20, B, dtype=dtype).to(dev)
        med, ms, _ = timed(lambda: na.quad_baseline_loss(z0, U20, prob, 5000., grad=True), args.reps, args.warmup)
        rows.append(dict(what="eval", nt=20, B=B, ms=med, ms_all=ms, cpu_ms_per_iter=1e3 * CPU_S_PER_ITER))
        print(f"eval   nt=20  B={B:5d}  {1e3 * med:9.2f} us/launch (objective + gradient of every start)", flush=True)
        U50 = na.quad_initial_guess(50, B, dtype=dtype).to(dev)
        med, ms, out = timed(lambda: na.solve_baseline_quad(z0, prob, nt=50, alphG=5000., U0=U50, **SETTINGS), args.reps, args.warmup)
        _, loss, info = out
        it, ev = info["n_iter"].cpu(), info["n_evals"].cpu()
        rows.append(dict(what="solve", nt=50, B=B, ms=med, ms_all=ms, n_iter_max=int(it.max()), n_iter_min=int(it.min()),
                         n_evals_max=int(ev.max()), us_per_iter=1e3 * med / int(it.max()), us_per_eval=1e3 * med / int(ev.max()),
                         loss_min=float(loss.min()), loss_max=float(loss.max()), cpu_ms_per_iter=1e3 * CPU_S_PER_ITER))
        print(f"solve  nt=50  B={B:5d}  {med:9.3f} ms/solve  {int(it.min())}-{int(it.max())} iterations  "
              f"{1e3 * med / int(it.max()):7.2f} us/iter  ({1e3 * CPU_S_PER_ITER:.1f} ms/iter on the reference's CPU, one start)",
              flush=True)
    os.makedirs(args.out, exist_ok=True)
    info = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip, reps=args.reps,
                warmup=args.warmup, prec=args.prec, rows=rows)
    with open(os.path.join(args.out, stem + ".json"), "w") as f:
        json.dump(info, f, indent=1)
    with open(os.path.join(args.out, stem + ".txt"), "w") as f:
        f.write("singlequad     what   nt     B   time             iterations  us/iter  us/eval  reference CPU ms/iter (one start)\n")
        for r in rows:
            if r["what"] == "eval":
                f.write(f"singlequad     eval  {r['nt']:3d} {r['B']:5d} {1e3 * r['ms']:9.2f} us/launch  {'':10s}  {'':7s}  "
                        f"{1e3 * r['ms']:7.2f}  {r['cpu_ms_per_iter']:.1f}\n")
            else:
                f.write(f"singlequad     solve {r['nt']:3d} {r['B']:5d} {r['ms']:9.3f} ms/solve   {r['n_iter_min']:4d}-{r['n_iter_max']:<5d} "
                        f"{r['us_per_iter']:7.2f}  {r['us_per_eval']:7.2f}  {r['cpu_ms_per_iter']:.1f}\n")
    print("wrote", os.path.join(args.out, stem + ".json"))


if __name__ == "__main__":
    main()
