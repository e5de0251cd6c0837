#!/usr/bin/env python3
"""baseline2D-style driver on the MI355X path: the direct-transcription baseline that the NeuralOC results are compared against.

Same flags, defaults, log lines, table and controls file as the reference driver (baseline2D.py:12-26 flags, :101-102 the `i loss`
line every 10 iterations, :146-147 the table, :124 the controls file: torch.save of the [nt, d] tensor ubest, read back by
--resume).  The whole Adam solve is one kernel launch (neuraloc_amd.solve_baseline); the table is the report loop in eval mode.
No plotting.

Additions: --gpu, --seed (the reference is unseeded; the default seed 0 makes a run repeatable: the problem factory and the initial
guess draw from the CPU generator in the reference's order), --nx N (N starts drawn around xInit with spread --var0, solved in one
launch; the log lines and the table show the mean over the starts and the controls file holds [N, nt, d]).

    python baseline2D.py                      # softcorridor from xInit, nt = 50, 600 iterations
    python baseline2D.py --data swarm --nt 20 --alph 900,1e7,25000 --nx 1024
"""
import argparse
import os
import sys

import torch

import neuraloc_amd as na
from neuraloc_amd.initProb import initProb

# the reference's --data choices (baseline2D.py:13-16) and swarm50, the other SwarmTraj problem of this project
DATA = ["softcorridor", "swap2", "swap12", "swarm", "swarm50", "swap12_1pair", "swap12_2pair", "swap12_3pair", "swap12_4pair",
        "swap12_5pair", "midcross2", "midcross4", "midcross20", "midcross30"]


def parse_args(argv=None):
    p = argparse.ArgumentParser("Baseline (MI355X)")
    p.add_argument("--data", choices=DATA, type=str, default="softcorridor")
    p.add_argument("--nt", type=int, default=50, help="number of time steps")
    p.add_argument("--alph", type=str, default="100.0, 10000.0, 300.0", help="alphas: G, Q (obstacle), W (interaction)")
    p.add_argument("--niters", type=int, default=600)
    p.add_argument("--prec", type=str, default="single", choices=["single", "double"], help="single only on this path")
    p.add_argument("--save", type=str, default="experiments/oc/baseline", help="directory of the controls file")
    p.add_argument("--resume", type=str, default=None, help="evaluate a stored controls file instead of solving")
    p.add_argument("--gpu", type=int, default=0, help="(addition) device index")
    p.add_argument("--seed", type=int, default=0, help="(addition) torch seed; the reference is unseeded")
    p.add_argument("--nx", type=int, default=1, help="(addition) number of starts: xInit (1) or N draws around it")
    p.add_argument("--var0", type=float, default=1.0, help="(addition) spread of the --nx starts around xInit")
    args = p.parse_args(argv)
    args.alph = [float(item) for item in args.alph.split(",")]
    if len(args.alph) < 3:
        p.error("--alph needs three values: G, Q, W")
    if args.nx < 1:
        p.error("--nx must be >= 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.prec == "double":
        sys.exit("baseline2D.py: --prec double is not supported: the baseline kernels compute in fp32 (use --prec single)")
    if not torch.cuda.is_available():
        sys.exit("baseline2D.py: needs the MI355X (ROCm 'cuda' device); there is no CPU path")
    dev = torch.device("cuda", args.gpu)
    torch.manual_seed(args.seed)
    alphG = args.alph[0]
    nt = args.nt
    # the problem factory draws its batches on the CPU generator first, as the reference does (baseline2D.py:113-114)
    prob, _, _, xInit = initProb(args.data, 10, 10, var0=1.0, cvt=lambda t: t.float(),
                                 alph=[alphG, args.alph[1], args.alph[2], 0.0, 0.0, 0.0])
    d = xInit.numel()
    strTitle = "baseline_" + args.data + "_{:}_{:}_{:}".format(int(alphG), int(prob.alph_Q), int(prob.alph_W))
    x0 = xInit.reshape(1, d) if args.nx == 1 else xInit.reshape(1, d) + args.var0 * torch.randn(args.nx, d)
    path = None
    if args.resume is not None:
        uopt = torch.load(args.resume, map_location="cpu").float()
        if uopt.shape[-2:] != (nt, d):
            sys.exit(f"baseline2D.py: {args.resume} holds controls of shape {list(uopt.shape)}, expected [{nt}, {d}] (--nt, --data)")
        uopt = uopt.to(dev)
    else:
        # the straight-line guess of baseline2D.py:80-83, start by start, from the CPU generator
        U0 = torch.stack([(prob.xtarget.reshape(-1) - x0[i]) * torch.ones(nt, d) + 0.1 * torch.randn(nt, d)
                          for i in range(x0.shape[0])])
        prob.train()
        Ubest, best, hist = na.solve_baseline(x0.to(dev), prob, nt, niters=args.niters, alphG=alphG, U0=U0.to(dev), history=True)
        hist = hist.mean(0).cpu()
        for i in range(args.niters):
            if i % 10 == 0:
                print(i, hist[i].item())
        uopt = Ubest[0] if args.nx == 1 else Ubest
        os.makedirs(args.save, exist_ok=True)
        path = os.path.join(args.save, strTitle + ".pth")
        torch.save(uopt.detach().cpu().clone(), path)
    prob.eval()
    rows, traj = na.baseline_report(x0.to(dev), uopt, prob, alphG)
    row = rows.mean(0).cpu()
    print("{:10s} {:10s} {:10s} {:10s} {:10s}".format("loss", "L", "G", "Q", "W"))
    print("{:10.4e} {:10.4e} {:10.4e} {:10.4e} {:10.4e}".format(*[v.item() for v in row]))
    if path is not None:
        print("controls saved to " + path)
    return dict(rows=rows.cpu(), traj=traj.cpu(), controls=uopt.detach().cpu(), path=path)


if __name__ == "__main__":
    main()
