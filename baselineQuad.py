#!/usr/bin/env python3
"""baselineQuad-style driver on the MI355X path: the quadcopter baseline that compareQuad.py draws against the NeuralOC singlequad
controller.

Same flags, defaults, printed line and output file as the reference driver (baselineQuad.py:19-29 flags; :129 the `loss: ...
L(x,T): ...  G: ...` line; :135-141 the file baseline_quadcopter_alph{G}_{Q}_{W}.pth with ctrls [nt, 4], traj [12, nt+1], loss [1],
L [1] and G [], which compareQuad.py --baseline loads).  The whole torch.optim.LBFGS step (strong Wolfe, the reference's tolerances) is
one kernel launch (neuraloc_amd.solve_baseline_quad); the printed line is the reference's final loop.  The file goes to --save (the
reference writes to experiments/oc/baseline whatever --save says).  No plotting.

Additions: --seed (the reference is unseeded; the default seed 0 makes a run repeatable: the problem factory's draws, then the
guess 1e-2 randn(nt, 4), from the CPU generator in the reference's order), --nx N (N starts drawn around xInit with spread --var0,
solved in one launch; the line shows the mean over the starts and the file's tensors gain a leading [N] dimension), --max-iter (the
reference hard-codes 16000).

    python baselineQuad.py                    # xInit, nt = 50, alphG = 5000
    python baselineQuad.py --nx 1024 --save /tmp/quad
"""
import argparse
import os
import sys

import torch

import neuraloc_amd as na
from neuraloc_amd.initProb import initProb


def parse_args(argv=None):
    p = argparse.ArgumentParser("Baseline (MI355X)")
    p.add_argument("--data", choices=["singlequad"], type=str, default="singlequad")
    p.add_argument("--nt", type=int, default=50, help="number of time steps")
    p.add_argument("--alph", type=str, default="5000.0, 0.0, 0.0", help="alphas: G, Q (obstacle), W (interaction)")
    p.add_argument("--niters", type=int, default=600,
                   help="parsed and unused, as in the reference (its L-BFGS runs max_iter = 16000; see --max-iter)")
    p.add_argument("--gpu", type=int, default=0, help="send to specific gpu")
    p.add_argument("--prec", type=str, default="single", choices=["single", "double"], help="single only on this path")
    p.add_argument("--save", type=str, default="experiments/oc/baseline", help="define the save directory")
    p.add_argument("--seed", type=int, default=0, help="(addition) torch seed; the reference is unseeded")
    p.add_argument("--nx", type=int, default=1, help="(addition) number of starts: xInit (1) or N draws around it")
    p.add_argument("--var0", type=float, default=1.0, help="(addition) spread of the --nx starts around xInit")
    p.add_argument("--max-iter", type=int, default=16000, help="(addition) L-BFGS max_iter; the reference hard-codes 16000")
    args = p.parse_args(argv)
    args.alph = [float(item) for item in args.alph.split(",")]
    if len(args.alph) < 3:
        p.error("--alph needs three values: G, Q, W")
    if args.nx < 1:
        p.error("--nx must be >= 1")
    if args.max_iter < 0:
        p.error("--max-iter must be >= 0")
    return args


def main(argv=None):
    args = parse_args(argv)
    if args.prec == "double":
        sys.exit("baselineQuad.py: --prec double is not supported: the baseline kernels compute in fp32 (use --prec single)")
    if not torch.cuda.is_available():
        sys.exit("baselineQuad.py: needs the MI355X (ROCm 'cuda' device); there is no CPU path")
    dev = torch.device("cuda", args.gpu)
    torch.manual_seed(args.seed)
    alphG = args.alph[0]
    nt = args.nt
    # the problem factory draws its batches on the CPU generator first, as the reference does (baselineQuad.py:97-98)
    prob, _, _, xInit = initProb(args.data, 10, 10, var0=1.0, cvt=lambda t: t.float(),
                                 alph=[alphG, args.alph[1], args.alph[2], 0.0, 0.0, 0.0])
    d = xInit.numel()
    if args.nx == 1:
        x0 = xInit.reshape(1, d)
    else:
        x0 = xInit.reshape(1, d).repeat(args.nx, 1)
        x0[:, :3] += args.var0 * torch.randn(args.nx, 3)
    # the guess of baselineQuad.py:75, start by start, from the CPU generator
    U0 = na.quad_initial_guess(nt, args.nx)
    U, _, info = na.solve_baseline_quad(x0.to(dev), prob, nt=nt, alphG=alphG, U0=U0.to(dev), max_iter=args.max_iter)
    rows, traj = na.quad_baseline_report(x0.to(dev), U, prob, alphG)
    rows, traj, U = rows.cpu(), traj.cpu(), U.detach().cpu()
    row = rows.mean(0)
    print("loss: ", row[0].item(), " L(x,T): ", row[1].item(), "  G: ", row[2].item())
    strTitle = "baseline_quadcopter_alph{:}_{:}_{:}".format(int(alphG), int(args.alph[1]), int(args.alph[2]))
    if args.nx == 1:
        ckpt = {"ctrls": U[0].clone(), "traj": traj[0].clone(), "loss": rows[0, 0:1].clone(), "L": rows[0, 1:2].clone(),
                "G": rows[0, 2].clone()}
    else:
        ckpt = {"ctrls": U.clone(), "traj": traj.clone(), "loss": rows[:, 0:1].clone(), "L": rows[:, 1:2].clone(),
                "G": rows[:, 2].clone()}
    os.makedirs(args.save, exist_ok=True)
    path = os.path.join(args.save, strTitle + ".pth")
    torch.save(ckpt, path)
    print("controls saved to " + path)
    return dict(rows=rows, traj=traj, controls=U, path=path, info={k: v.cpu() for k, v in info.items()})


if __name__ == "__main__":
    main()
