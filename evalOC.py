#!/usr/bin/env python3
"""evalOC-style driver on the MI355X path.

Same flags as the reference's evalOC.py:14-24 (--nt --alph --resume --save --prec --approach --make_vid --do_shock): loads a
NeuralOC checkpoint (the reference's .pth files or ones written here), evaluates the costs on xInit and prints them in the
reference's log layout (evalOC.py:76-85), runs the intermediates rollout the reference's plots start from and saves it
(`<save>/figs/eval_<name>.npz`: zFull, ctrlFull -- figures and videos themselves are out of scope),
times the deployment like timeDeployment/timeOC.py:76-81 (nex = 1, nt steps; same 'time: ... avg time / RK4 timestep: ...'
line, appended to `<save>/deploy_times`) plus a batch, and with --do_shock runs the reference's two softcorridor shocks
(evalOC.py:113-122) through neuraloc_amd.shock for any problem.

--prec double runs the double-precision rollout (nocf_rollout_f64), like the reference's evalOC.py:28-31.
Differences, on purpose: --make_vid only states that videos are out of scope; --gpu/--batch are additions, and so is
--noise SIGMA [--noise_paths R --noise_seed S]: the distribution of the costs over R rollouts of xInit under per-step Brownian
disturbances (neuraloc_amd.disturb; single precision), one line per quantity and `<save>/figs/eval_<name>_noise.npz`;
--noise_rho RHO (with --noise): those disturbances correlated in time, an Ornstein-Uhlenbeck path of lag-one correlation 0 < RHO < 1
(neuraloc_amd.noise_study(..., rho=RHO); the default 0 is the white noise);
--worst EPS [--worst_steps K]: the disturbance path of energy ||W||_2 <= EPS that hurts the control objective L + alph0 G of xInit most
(neuraloc_amd.worst_case_disturbances, K projected ascent steps; single precision), one line per quantity, nominal against worst case,
and `<save>/figs/eval_<name>_worst.npz`;
--hold K1,K2,... : what xInit costs when the control is refreshed only every K-th step and held in between (neuraloc_amd.hold_study,
DESIGN.md section 3.19; single precision, the lane and one-CU kernels), one line per K with the plain closed loop as hold 0, and
`<save>/figs/eval_<name>_hold.npz`; with --noise SIGMA [--noise_paths R --noise_seed S --noise_rho RHO] every K meets the same R disturbance
paths (drawn inside the library from the seed) and the lines give the mean and the 5 / 50 / 95 % quantiles."""
import argparse
import os
import time

import numpy as np
import torch

import neuraloc_amd as na
from neuraloc_amd.checkpoint import load_checkpoint
from neuraloc_amd.shock import shock_rollout

p = argparse.ArgumentParser("Optimal Control")
p.add_argument("--nt", type=int, default=50, help="number of time steps")
p.add_argument("--alph", type=str, default="1.0, 1.0, 1.0, 1.0, 1.0, 1.0", help="(ignored like in the reference: the checkpoint's alph is used, evalOC.py:53-54)")
p.add_argument("--resume", type=str, default="experiments/oc/pretrained/softcorridor_nn_checkpt.pth")
p.add_argument("--save", type=str, default="experiments/oc/eval")
p.add_argument("--prec", type=str, default="single", choices=["single", "double"], help="single or double precision")
p.add_argument("--approach", type=str, default="ocflow", choices=["ocflow"])
p.add_argument("--make_vid", default=False, action="store_true", help="including this flag will produce video")
p.add_argument("--do_shock", default=False, action="store_true", help="including this flag will incorporate shocks")
p.add_argument("--batch", type=int, default=1024, help="(addition) batch size of the throughput line")
p.add_argument("--gpu", type=int, default=0, help="(addition) device index")
p.add_argument("--noise", type=float, default=None, metavar="SIGMA",
               help="(addition) roll xInit out under Brownian state disturbances sigma dB at every step (neuraloc_amd.noise_study)")
p.add_argument("--noise_paths", type=int, default=256, metavar="R", help="(addition) noise realisations per start for --noise")
p.add_argument("--noise_seed", type=int, default=0, metavar="S", help="(addition) seed of the disturbances for --noise")
p.add_argument("--noise_rng", type=str, default="torch", choices=["torch", "counter"],
               help="(addition) torch: the disturbances are drawn with torch.randn; counter: inside the kernels from (seed, row, step, "
                    "component) (neuraloc_amd.noisy_rollout): no tensor, and the figures do not depend on the chunking")
p.add_argument("--noise_rho", type=float, default=0.0, metavar="RHO",
               help="(addition, with --noise) 0 <= RHO < 1: time-correlated (Ornstein-Uhlenbeck) disturbances of lag-one correlation RHO, on either "
                    "--noise_rng (neuraloc_amd.noise_study with rho=RHO); 0: the white noise of --noise")
p.add_argument("--worst", type=float, default=None, metavar="EPS",
               help="(addition) search the per-step state disturbances of path norm <= EPS that hurt xInit's L + G most (neuraloc_amd.worst_case_disturbances)")
p.add_argument("--worst_steps", type=int, default=20, metavar="K", help="(addition) projected ascent steps for --worst")
p.add_argument("--hold", type=str, default=None, metavar="K1,K2,...",
               help="(addition) roll xInit out with the control refreshed every K-th step and held in between, for every K of the list "
                    "(neuraloc_amd.hold_study); with --noise under the same disturbances for every K")


def parse_holds(text):
    """--hold: a comma-separated list of integers >= 1"""
    try:
        holds = [int(item) for item in text.split(",")]
    except ValueError:
        raise SystemExit("--hold K1,K2,... must be a comma-separated list of integers >= 1") from None
    if not holds or min(holds) < 1:
        raise SystemExit("--hold K1,K2,... must be a comma-separated list of integers >= 1")
    return holds


def noise_rho_refusals(args):
    """--noise_rho: what the time-correlated noise does not take, refused before anything runs or is written"""
    if args.noise_rho == 0:
        return
    if not 0.0 <= args.noise_rho < 1.0:                    # (a NaN fails both comparisons)
        raise SystemExit("--noise_rho RHO must be a number with 0 <= RHO < 1")
    if args.noise is None:
        raise SystemExit("--noise_rho needs --noise SIGMA: it shapes that noise in time")
    if args.prec == "double":
        raise SystemExit("--noise_rho runs in single precision only (the double-precision rollout takes no disturbance)")


def main(argv=None):
    args = p.parse_args(argv)
    noise_rho_refusals(args)
    args.alph = [float(item) for item in args.alph.split(",")]
    prec = torch.float64 if args.prec == "double" else torch.float32          # evalOC.py:28-31
    if args.noise is not None and prec != torch.float32:                     # refused before anything runs or is written
        raise SystemExit("--noise runs in single precision only (the double-precision rollout takes no disturbance)")
    if args.noise_rng == "counter" and prec != torch.float32:
        raise SystemExit("--noise_rng counter runs in single precision only (the double-precision rollout takes no disturbance)")
    if args.noise_rng == "counter" and not 0 <= args.noise_seed < 2 ** 64:
        raise SystemExit("--noise_rng counter needs 0 <= --noise_seed < 2**64")
    if args.worst is not None and prec != torch.float32:
        raise SystemExit("--worst runs in single precision only (the double-precision rollout takes no disturbance)")
    holds = None if args.hold is None else parse_holds(args.hold)
    if holds is not None and prec != torch.float32:
        raise SystemExit("--hold runs in single precision only (the double-precision rollout takes no held control)")
    if holds is not None and args.noise is not None and not 0 <= args.noise_seed < 2 ** 64:
        raise SystemExit("--hold with --noise needs 0 <= --noise_seed < 2**64")
    os.makedirs(os.path.join(args.save, "figs"), exist_ok=True)
    print(args)
    dev = f"cuda:{args.gpu}"
    print(" ")
    print("loading model: {:}".format(args.resume))
    print(" ")
    net, prob, x0, _, xInit, a = load_checkpoint(args.resume, device=dev, n_train=args.batch, n_val=args.batch, dtype=prec)
    prob.eval()
    net.eval()
    alph = net.alph
    nt = args.nt
    strTitle = "eval_" + os.path.basename(args.resume)[:-12]
    out = {}
    with torch.no_grad():
        print("{:8s} {:12s} {:11s} {:11s} {:11s} {:11s} {:11s} {:11s} {:11s} ".format(
            "just xInit", "L+G", "L", "G w/ a0", "HJt", "HJfin", "HJgrad", "Q", "W"))
        Jc, cs = na.OCflow(xInit, net, prob, tspan=[0.0, 1.0], nt=nt, stepper="rk4", alph=alph)
        zFull, ctrlFull = na.OCflow(xInit, net, prob, tspan=[0.0, 1.0], nt=nt, stepper="rk4", alph=alph, intermediates=True)
        print("         {:12.4e} {:11.3e} {:11.3e} {:11.3e} {:11.3e} {:11.3e} {:11.3e} {:11.3e}".format(
            cs[0] + alph[0] * cs[1], cs[0], alph[0] * cs[1], alph[3] * cs[2], alph[4] * cs[3], alph[5] * cs[4], cs[5], cs[6]))
        sPath = os.path.join(args.save, "figs", strTitle + ".npz")
        np.savez(sPath, zFull=zFull.cpu().numpy(), ctrlFull=ctrlFull.cpu().numpy(), Jc=float(Jc), cs=np.array([float(c) for c in cs]))
        print("trajectory saved to " + sPath + " (plots are out of scope here)")
        out["Jc"], out["cs"] = float(Jc), [float(c) for c in cs]

        # -------TIME THE DEPLOYED MODEL (timeDeployment/timeOC.py:76-81: one call, nex = 1), then a warm call and a batch
        with open(os.path.join(args.save, "deploy_times"), "a") as timeFile:
            print("problem: ", a.data, file=timeFile)
            print("device: ", torch.cuda.get_device_name(dev), file=timeFile)
            torch.cuda.synchronize()
            start = time.time()
            na.OCflow(xInit, net, prob, tspan=[0.0, 1.0], nt=nt, stepper="rk4", alph=alph)
            torch.cuda.synchronize()
            end = time.time()
            line = "time: %5f   avg time / RK4 timestep: %5f" % (end - start, (end - start) / nt)
            print(line, file=timeFile)
            print(line)
            out["deploy_time"] = end - start
        for name, x in (("warm deployment (nex=1)", xInit), (f"batch (nex={x0.shape[0]})", x0)):
            for _ in range(3):
                na.OCflow(x, net, prob, [0.0, 1.0], nt, "rk4", alph)
            torch.cuda.synchronize()
            t0 = time.time()
            reps = 20
            for _ in range(reps):
                na.OCflow(x, net, prob, [0.0, 1.0], nt, "rk4", alph)
            torch.cuda.synchronize()
            na.check_errors()
            dt = (time.time() - t0) / reps
            print("%s time: %5f   avg time / RK4 timestep: %5f   trajectories/s: %.1f" % (name, dt, dt / nt, x.shape[0] / dt))
        if args.make_vid:
            print("video not implemented on this path (plotting is out of scope); the trajectory file above holds the frames' data")
        if args.do_shock:
            d = xInit.shape[1]
            for tag, vals in (("shock", [-0.2, -0.7, -0.0, -0.6]), ("majorshock", [-1.4, -1.0, -5.2, -2.8])):       # evalOC.py:115-120
                shock = torch.zeros(1, d, device=xInit.device, dtype=xInit.dtype)
                shock[0, : min(4, d)] = torch.tensor(vals, dtype=xInit.dtype)[: min(4, d)]
                res = shock_rollout(xInit, net, prob, nt, 0.1, shock)
                np.savez(os.path.join(args.save, "figs", f"{strTitle}_{tag}.npz"), traj=res["traj"].cpu().numpy(), ctrl=res["ctrl"].cpu().numpy())
                print("%s at t=0.1: nShock=%d, final state error %.4e" %
                      (tag, res["nShock"], float((res["traj"][0, :, -1] - prob.xtarget.reshape(-1)).norm())))
        if args.noise is not None:
            rho_kw = {"rho": args.noise_rho} if args.noise_rho != 0 else {}         # (0: the white path and its entry points)
            if args.noise_rng == "counter":
                st = na.noise_study(xInit, net, prob, nt, args.noise, args.noise_paths, alph=alph, rng="counter", seed=args.noise_seed, **rho_kw)
            else:
                gen = torch.Generator(device=xInit.device).manual_seed(args.noise_seed)
                st = na.noise_study(xInit, net, prob, nt, args.noise, args.noise_paths, alph=alph, generator=gen, **rho_kw)
            print("noise sigma=%g, %d paths, seed %d: %-4s %11s %11s %11s %11s %11s" %
                  (args.noise, args.noise_paths, args.noise_seed, "", "mean", "std", "5%", "50%", "95%"))
            keys = ("mean", "std", "q05", "q50", "q95")
            for name in ("L+G", "G", "Q", "W"):
                print("noise %-4s" % name + "".join(" %11.4e" % float(st[name][k][0]) for k in keys))
            sPath = os.path.join(args.save, "figs", strTitle + "_noise.npz")
            np.savez(sPath, sigma=args.noise, paths=args.noise_paths, seed=args.noise_seed, persample=st["persample"].cpu().numpy(),
                     **{f"{name}/{k}": st[name][k].cpu().numpy() for name in ("L+G", "G", "Q", "W") for k in keys})
            print("saved the noise study to " + sPath)
            out["noise"] = {name: {k: float(st[name][k][0]) for k in keys} for name in ("L+G", "G", "Q", "W")}
        if args.worst is not None:
            nom = na.disturbed_rollout(xInit, net, prob, nt, torch.zeros(nt, xInit.shape[0], xInit.shape[1], device=xInit.device), alph=alph)
            res = na.worst_case_disturbances(xInit, net, prob, nt, args.worst, steps=args.worst_steps, alph=alph, objective="control")
            na.check_errors(sync=True)
            t0_, t1_ = nom["persample"][0], res["persample"][0]
            print("worst eps=%g, %d steps: %-4s %11s %11s" % (args.worst, args.worst_steps, "", "nominal", "worst case"))
            rows = {"L+G": (float(t0_[0] + alph[0] * t0_[1]), float(t1_[0] + alph[0] * t1_[1])), "G": (float(t0_[1]), float(t1_[1])),
                    "Q": (float(t0_[5]), float(t1_[5])), "W": (float(t0_[6]), float(t1_[6]))}
            for name in ("L+G", "G", "Q", "W"):
                print("worst %-4s %11.4e %11.4e" % ((name,) + rows[name]))
            sPath = os.path.join(args.save, "figs", strTitle + "_worst.npz")
            np.savez(sPath, eps=args.worst, steps=args.worst_steps, W=res["W"].cpu().numpy(), history=res["history"].cpu().numpy(),
                     persample=res["persample"].cpu().numpy(), nominal=nom["persample"].cpu().numpy())
            print("saved the worst-case disturbance to " + sPath)
            out["worst"] = {name: {"nominal": rows[name][0], "worst": rows[name][1]} for name in rows}
            out["worst"]["norm"] = float(res["W"].pow(2).sum().sqrt())
        if holds is not None:
            kw = {}
            if args.noise is not None:
                kw = dict(sigma=args.noise, seed=args.noise_seed, paths=args.noise_paths, rho=args.noise_rho if args.noise_rho != 0 else None)
            st = na.hold_study(xInit, net, prob, nt, holds=holds, alph=alph, **kw)
            names = ("L+G", "G", "L", "Q", "W")
            save = {"holds": np.array([0] + holds), "sigma": np.nan if args.noise is None else args.noise,
                    "paths": 1 if args.noise is None else args.noise_paths, "seed": args.noise_seed}
            out["hold"] = {}
            if args.noise is None:
                print("hold %4s" % "K" + "".join(" %11s" % name for name in names))
                for k in [0] + holds:
                    print("hold %4d" % k + "".join(" %11.4e" % float(st[k][name][0]) for name in names))
                    out["hold"][k] = {name: float(st[k][name][0]) for name in names}
                    save.update({f"{k}/{name}": st[k][name].cpu().numpy() for name in names})
            else:
                keys = ("mean", "std", "q05", "q50", "q95")
                print("hold sigma=%g, %d paths, seed %d (the same disturbances for every K; mean [5%%, 50%%, 95%%])" %
                      (args.noise, args.noise_paths, args.noise_seed))
                print("hold %4s" % "K" + "".join(" %47s" % name for name in names))
                for k in [0] + holds:
                    print("hold %4d" % k + "".join(" %11.4e [%10.3e,%10.3e,%10.3e]" % tuple(float(st[k][name][q][0]) for q in ("mean", "q05", "q50", "q95"))
                                                   for name in names))
                    out["hold"][k] = {name: {q: float(st[k][name][q][0]) for q in keys} for name in names}
                    save.update({f"{k}/{name}/{q}": st[k][name][q].cpu().numpy() for name in names for q in keys})
            save.update({f"{k}/persample": st[k]["persample"].cpu().numpy() for k in [0] + holds})
            sPath = os.path.join(args.save, "figs", strTitle + "_hold.npz")
            np.savez(sPath, **save)
            print("saved the hold study to " + sPath)
    return out


if __name__ == "__main__":
    main()
