#!/usr/bin/env python3
"""
Pin the quadcopter baseline (the reference's baselineQuad.py) -> tests/golden/baseline_quad.npz.

The problem object is the REFERENCE's (src/initProb.py 'singlequad': Quadcopter.f, mass, grav, xtarget); the objective is baselineQuad.py's
compute_loss written out (dyn, the Euler loop, the running cost and G), on the CPU.  Runs only in the build container (imports the
reference read-only); the fixture is data.

  ckpt/*      the shipped experiments/oc/pretrained/singlequad_baseline_checkpt.pth: ctrls [50, 4], traj [12, 51], loss, L, G
  obj/nt{nt}  nt in 1, 7, 20, 50: three seeded starts (xInit and two perturbed) and seeded controls (thrust about mass * grav):
              J and dJ/dU (autograd) in fp64 and fp32
  solve/*     four starts (xInit and three perturbed by randn(3)) and guesses 1e-2 randn(50, 4): torch.optim.LBFGS at the reference's
              settings in fp64 and fp32 -> final loss, n_iter, func_evals
  lock/*      starts and guesses for the lockstep comparison: kept only when torch's fp32 and fp64 runs agree on n_iter and func_evals
              at every cap the tests use (max_iter 1, 2, 3, 5, 10; max_eval 7), so that the count a test pins is not one rounding
              away from another

usage:  python tests/golden/make_golden_baseline_quad.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
from src.initProb import initProb as ref_initProb      # noqa: E402  (reference)

ALPHG = 5000.0
NT_LIST = (1, 7, 20, 50)
LBFGS = dict(max_iter=16000, max_eval=10000, line_search_fn="strong_wolfe", tolerance_grad=1e-05, tolerance_change=1e-06)
LOCK_CAPS = [dict(max_iter=m) for m in (1, 2, 3, 5, 10)] + [dict(max_iter=16000, max_eval=7)]


def make_prob(dtype):
    prob, _, _, xInit = ref_initProb("singlequad", 10, 10, var0=1.0, cvt=lambda t: t.to(dtype),
                                     alph=[ALPHG, 0.0, 0.0, 0.0, 0.0, 0.0])
    return prob, xInit.reshape(-1)


def dyn(ctrls, x, prob):
    """baselineQuad.py:44-50"""
    f7, f8, f9 = prob.f(x[3:6].unsqueeze(0))
    tmp = (ctrls[0] / prob.mass)
    return torch.cat([x[6:], tmp * f7, tmp * f8, tmp * f9 - prob.grav, ctrls[1:4]])


def compute_loss(ctrls, x0, prob, alphG=ALPHG):
    """baselineQuad.py:53-70"""
    nt = ctrls.shape[0]
    h = 1.0 / nt
    J = 0.0
    x = x0
    for i in range(nt):
        dx = dyn(ctrls[i, :], x, prob)
        x = x + h * dx
        J = J + h * (2 + torch.norm(ctrls[i, :], p=2) ** 2)
    J += alphG * 0.5 * torch.norm(x - prob.xtarget, p=2) ** 2
    return J


def loss_grad(U, x0, prob):
    u = U.detach().clone().requires_grad_(True)
    J = compute_loss(u, x0, prob)
    (g,) = torch.autograd.grad(J, u)
    return float(J), g.detach()


def lbfgs(x0, U0, prob, **kw):
    """trainBaseline (baselineQuad.py:74-91) without the prints -> (final loss, n_iter, func_evals, final U)"""
    ctrls = torch.nn.Parameter(U0.detach().clone())
    opt = torch.optim.LBFGS([ctrls], **kw)

    def closure():
        opt.zero_grad()
        err = compute_loss(ctrls, x0, prob)
        err.backward()
        return err

    opt.step(closure)
    st = opt.state[ctrls]
    with torch.no_grad():
        f = float(compute_loss(ctrls, x0, prob))
    return f, int(st["n_iter"]), int(st["func_evals"]), ctrls.detach().clone()


def starts(gen, xInit, k):
    """xInit and k - 1 starts perturbed in position by randn(3)"""
    z = [xInit.clone()]
    for _ in range(k - 1):
        p = xInit.clone()
        p[:3] += torch.randn(3, generator=gen, dtype=torch.float64).to(p.dtype)
        z.append(p)
    return torch.stack(z)


def main():
    torch.set_num_threads(4)
    out = {}
    prob64, xInit64 = make_prob(torch.float64)
    prob32, xInit32 = make_prob(torch.float32)
    out["xInit"] = xInit32.numpy()
    out["xtarget"] = prob32.xtarget.numpy()

    ck = torch.load(os.path.join(REF, "experiments/oc/pretrained/singlequad_baseline_checkpt.pth"), map_location="cpu")
    for k in ("ctrls", "traj", "loss", "L", "G"):
        out["ckpt/" + k] = ck[k].detach().float().numpy()

    gen = torch.Generator().manual_seed(20261016)
    for nt in NT_LIST:
        z = starts(gen, xInit64, 3)
        U = torch.randn(3, nt, 4, generator=gen, dtype=torch.float64)
        U[:, :, 0] = 9.81 + 2.0 * U[:, :, 0]                 # thrust about mass * grav; angular accelerations ~ N(0, 1)
        J64, g64, J32, g32 = [], [], [], []
        for b in range(3):
            j, g = loss_grad(U[b], z[b], prob64)
            J64.append(j); g64.append(g.numpy())
            j, g = loss_grad(U[b].float(), z[b].float(), prob32)
            J32.append(j); g32.append(g.numpy())
        out[f"obj/nt{nt}/z0"] = z.float().numpy()
        out[f"obj/nt{nt}/U"] = U.float().numpy()
        out[f"obj/nt{nt}/J64"] = np.array(J64)
        out[f"obj/nt{nt}/g64"] = np.stack(g64)
        out[f"obj/nt{nt}/J32"] = np.array(J32, dtype=np.float32)
        out[f"obj/nt{nt}/g32"] = np.stack(g32)
    # the fixture stores fp32 inputs: the fp64 values above are recomputed from exactly those inputs
    for nt in NT_LIST:
        z = torch.from_numpy(out[f"obj/nt{nt}/z0"]).double()
        U = torch.from_numpy(out[f"obj/nt{nt}/U"]).double()
        res = [loss_grad(U[b], z[b], prob64) for b in range(3)]
        out[f"obj/nt{nt}/J64"] = np.array([r[0] for r in res])
        out[f"obj/nt{nt}/g64"] = np.stack([r[1].numpy() for r in res])

    # full solves at the reference's settings
    gen = torch.Generator().manual_seed(7)
    z = starts(gen, xInit64, 4).float()
    U0 = (1.e-2 * torch.randn(4, 50, 4, generator=gen, dtype=torch.float64)).float()
    rec = {k: [] for k in ("loss64", "n_iter64", "evals64", "loss32", "n_iter32", "evals32")}
    for b in range(4):
        f, it, ev, _ = lbfgs(z[b].double(), U0[b].double(), prob64, **LBFGS)
        rec["loss64"].append(f); rec["n_iter64"].append(it); rec["evals64"].append(ev)
        f, it, ev, _ = lbfgs(z[b], U0[b], prob32, **LBFGS)
        rec["loss32"].append(f); rec["n_iter32"].append(it); rec["evals32"].append(ev)
        print(f"solve {b}: fp64 {rec['loss64'][-1]:.6f} ({rec['n_iter64'][-1]} it, {rec['evals64'][-1]} ev)  "
              f"fp32 {rec['loss32'][-1]:.6f} ({rec['n_iter32'][-1]} it, {rec['evals32'][-1]} ev)", flush=True)
    out["solve/z0"] = z.numpy()
    out["solve/U0"] = U0.numpy()
    for k, v in rec.items():
        out["solve/" + k] = np.array(v, dtype=np.float64 if k.startswith("loss") else np.int32)

    # lockstep starts: screened on fp32 / fp64 agreement of the counts at every cap
    gen = torch.Generator().manual_seed(11)
    keep_z, keep_u, tried = [], [], 0
    while len(keep_z) < 3:
        tried += 1
        zc = starts(gen, xInit64, 2)[1].float()
        uc = (1.e-2 * torch.randn(50, 4, generator=gen, dtype=torch.float64)).float()
        ok = True
        for cap in LOCK_CAPS:
            kw = dict(LBFGS, **cap)
            a = lbfgs(zc.double(), uc.double(), prob64, **kw)
            c = lbfgs(zc, uc, prob32, **kw)
            if a[1:3] != c[1:3]:
                ok = False
                break
        print(f"lock candidate {tried}: {'kept' if ok else 'screened out'}", flush=True)
        if ok:
            keep_z.append(zc.numpy()); keep_u.append(uc.numpy())
    keep_z.insert(0, xInit32.numpy())                         # xInit with the first solve's guess is screened the same way
    keep_u.insert(0, U0[0].numpy())
    for cap in LOCK_CAPS:
        kw = dict(LBFGS, **cap)
        a = lbfgs(torch.from_numpy(keep_z[0]).double(), torch.from_numpy(keep_u[0]).double(), prob64, **kw)
        c = lbfgs(torch.from_numpy(keep_z[0]), torch.from_numpy(keep_u[0]), prob32, **kw)
        if a[1:3] != c[1:3]:
            keep_z.pop(0); keep_u.pop(0)
            print("xInit screened out", flush=True)
            break
    out["lock/z0"] = np.stack(keep_z)
    out["lock/U0"] = np.stack(keep_u)

    path = os.path.join(HERE, "baseline_quad.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes", flush=True)


if __name__ == "__main__":
    main()
