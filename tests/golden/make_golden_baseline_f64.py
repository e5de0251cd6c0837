#!/usr/bin/env python3
"""
Pin the two baselines in DOUBLE precision (the reference's baseline2D.py / baselineQuad.py with --prec double) -> tests/golden/baseline_f64.npz.

The problem objects are the REFERENCE's, built with a float64 cvt; the objectives, the report loop and the optimiser loops are the ones
make_golden_baseline.py / make_golden_baseline_quad.py write out with the reference's semantics, run here on float64 tensors on the CPU.
Runs only in the build container (imports the reference read-only through those two generators); the fixture is data.  Before anything
is written, the repository's own fp64 restatements (tests/util_oracle.restate on the fp64 trajectory, tests/util_quad.objective) are
asserted equal to the reference's values at 1e-12 of each quantity's scale.

Point agents, the eight problems of baseline.npz, train and eval mode (keys {name}/nt{nt}/...):
  nt = 20    the three starts and controls of baseline.npz (swarm50: the first two; fp32 values, widened: their screen against the
             decision edges holds)
  nt = 1, 50 one screened start each (nt = 50 where the double-precision kernels take it: not swarm50, whose limit is 38)
             -> z0, U, and per mode loss [S], grad [S, nt, d], report [S, 5]; traj [S, d, nt+1] once (it does not depend on the mode)
  nt = limit the largest nt of the double-precision kernels (LIMITS below; tests/test_baseline_f64_cpu.py pins them against
             nocf_baseline_max_nt), one screened start (inputs stored as the fp32 values they are) -> per mode loss, report, the two
             marginals of dJ/dU (summed over the steps [d], over the coordinates [nt]) and the final state
  adam10     10 reference Adam steps in double from baseline.npz's first U at xInit, train mode, nt = 20 -> losses [10], final U
Quadcopter (keys quad/...), inputs from baseline_quad.npz:
  ckpt       the shipped controls evaluated in double: loss, L, G, grad, traj
  cap{k}     start LOCK_START of lock/*: torch.optim.LBFGS in double capped at max_iter 1, 2, 3, 5, 10 and at max_eval 7
             -> U, loss, n_iter, func_evals (the start is the first on which util_quad's restatement, driven through torch.optim.LBFGS,
             gives the same counts and iterate at all six caps: meta["lock_start"])
  solve      the reference-settings solve from xInit (solve/z0[0], solve/U0[0] of baseline_quad.npz) at nt = 50: final loss, n_iter,
             func_evals, and the cap on max_iter in meta["solve_max_iter"] (16000: the reference's own, the CPU solve takes seconds)

usage:  python tests/golden/make_golden_baseline_f64.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_baseline as gb             # noqa: E402  (imports the reference; before the repository root is on the path, whose src/
import make_golden_baseline_quad as gq        # noqa: E402   shims would answer `import src` otherwise)
assert gb.ref_initProb.__module__ == "src.initProb" and gb.REF in sys.modules["src.initProb"].__file__
sys.path.append(os.path.dirname(HERE))
sys.path.append(os.path.dirname(os.path.dirname(HERE)))
import util_oracle as uo                      # noqa: E402
import util_quad as uq                        # noqa: E402
from oracle import ocflow_oracle as orc       # noqa: E402

# the largest nt of nocf_baseline_eval_f64 / nocf_baseline_adam_f64 (one limit for both): 3 nt d + d + 3 nt + 8 doubles plus three partial
# sums per thread (256 threads, 1024 when nt * agents >= 512) within 160 KiB
LIMITS = {"softcorridor": 256, "swap2": 256, "swap12": 231, "swap12_3pair": 256, "midcross4": 256, "midcross20": 141, "swarm": 59,
          "swarm50": 38}
CAPS = [dict(max_iter=m) for m in (1, 2, 3, 5, 10)] + [dict(max_iter=16000, max_eval=7)]
DT = torch.float64


def make_prob64(name, alph):
    prob, _, _, xInit = gb.ref_initProb(name, 10, 10, var0=1.0, cvt=lambda t: t.double(), alph=[alph[0], alph[1], alph[2], 0., 0., 0.])
    return prob, xInit.reshape(-1)


def report64(U, z0, prob, nt, alphG):
    """make_golden_baseline.report without its fp32 casts"""
    d = z0.numel()
    h = 1. / nt
    traj = torch.zeros(d, nt + 1, dtype=DT)
    traj[:, 0] = z0
    accL = accQ = accW = 0
    for j in range(nt):
        L, _, Q, W = prob.calcLHQW(traj[:, j].view(1, -1), U[j, :].view(1, -1))
        accL = accL + h * L
        accQ = accQ + h * Q
        accW = accW + h * W
        traj[:, j + 1] = traj[:, j] + h * U[j, :]
    cG = 0.5 * torch.sum(gb.ref_ocG(traj[:, -1].view(1, -1), prob.xtarget) ** 2, 1, keepdims=True)
    G = alphG * cG
    row = [float(torch.as_tensor(v).double().reshape(-1)[0]) for v in (G + accL, accL, G, accQ, accW)]
    return np.array(row), traj.numpy()


def evaluate(prob, z0s, Us, nt, alphG):
    """the reference in double, start by start, in the problem's current mode -> loss [S], grad [S, nt, d], report [S, 5], traj [S, d, nt+1]"""
    J, G, R, T = [], [], [], []
    for z0, U in zip(z0s, Us):
        u = U.clone().requires_grad_(True)
        j = gb.objective(u, z0, prob, nt, alphG)
        j.backward()
        J.append(j.item())
        G.append(u.grad.numpy().copy())
        with torch.no_grad():
            row, traj = report64(U, z0, prob, nt, alphG)
        R.append(row)
        T.append(traj)
    return np.array(J), np.stack(G), np.stack(R), np.stack(T)


def check_restatement(prob, z0s, Us, alphG, J, G, R, T, what):
    S = orc.ProbSpec.from_object(prob)
    z, U = torch.stack(z0s), torch.stack(Us)
    traj = torch.from_numpy(T).permute(0, 2, 1).contiguous()
    r = uo.restate(S, z, U, alphG, DT, traj=traj)
    for name, got, want in (("J", r["J"], J), ("grad", r["grad"], G), ("report", r["report"], R)):
        want = torch.from_numpy(np.asarray(want))
        err = float((got - want).abs().max())
        scale = max(float(want.abs().max()), 1e-300)
        assert err <= 1e-12 * scale, f"{what}: the fp64 restatement's {name} is {err / scale:.3g} (relative) away from the reference"


# the screen of the new starts: both sides compute in double here and differ by rounding only, so the decision edges need a margin of
# 1e-6 (pair distances, hard-corridor norms) and 1e-8 (block bounds), not make_golden_baseline's fp32 margins -- which twenty agents over
# fifty steps cannot keep
MARGIN64, BOX_MARGIN64 = 1e-6, 1e-8


def screened_input(prob32, xInit32, nt, base):
    """make_golden_baseline's inputs (fp32 values) and its screen on the double-precision states: the first seed from `base` on that passes"""
    gb.MARGIN, gb.BOX_MARGIN = MARGIN64, BOX_MARGIN64
    for seed in range(base, base + 5000):
        z0, U = gb.case_input(prob32, xInit32, nt, 1, seed)
        if gb.near_threshold(prob32, gb.states(U.double(), z0.double(), nt)) > 1.0:
            return z0.double(), U.double(), seed
    raise AssertionError(f"nt = {nt}: no seed passes the screen")


def quad_lbfgs_restated(z0, U0, **kw):
    """util_quad's objective driven through torch.optim.LBFGS, in double"""
    ctrls = torch.nn.Parameter(U0.detach().clone())
    opt = torch.optim.LBFGS([ctrls], **kw)
    zb = z0.reshape(1, -1)

    def closure():
        opt.zero_grad()
        L, traj = uq.rollout(zb, ctrls.unsqueeze(0), dtype=DT)
        err = (L + uq.ALPHG * 0.5 * torch.norm(traj[:, :, -1] - torch.tensor(uq.XTARGET, dtype=DT), p=2, dim=1) ** 2)[0]
        err.backward()
        return err

    opt.step(closure)
    st = opt.state[ctrls]
    return int(st["n_iter"]), int(st["func_evals"]), ctrls.detach().clone()


def main():
    torch.set_num_threads(8)
    out, meta = {}, {"torch": torch.__version__, "limits": LIMITS, "seeds": {}}
    base = np.load(os.path.join(HERE, "baseline.npz"))
    for name in gb.NAMES:
        alph = gb.ALPH[name]
        prob, xInit = make_prob64(name, alph)
        prob32, xInit32 = gb.make_prob(name, alph)
        keep = 2 if name == "swarm50" else 3                  # (swarm50's rows are the fixture's largest: two starts keep it well under 1 MiB)
        cases = {20: ([torch.from_numpy(z).double() for z in base[f"{name}/nt20/z0"][:keep]],
                      [torch.from_numpy(u).double() for u in base[f"{name}/nt20/U"][:keep]], None)}
        for nt in (1, 50, LIMITS[name]):
            if nt == 50 and LIMITS[name] < 50:
                continue
            z0, U, seed = screened_input(prob32, xInit32, nt, 70000 + 100 * nt)
            cases[nt] = ([z0], [U], seed)
        for nt, (z0s, Us, seed) in cases.items():
            lim = nt == LIMITS[name] and nt not in (1, 20, 50)
            pre = f"{name}/lim" if lim else f"{name}/nt{nt}"
            if seed is not None:
                meta["seeds"][pre] = seed
            # (the inputs are fp32 values: at the limit they are stored as such, half the bytes)
            out[f"{pre}/z0"] = torch.stack(z0s).numpy().astype(np.float32 if lim else np.float64)
            out[f"{pre}/U"] = torch.stack(Us).numpy().astype(np.float32 if lim else np.float64)
            for mode in ("train", "eval"):
                prob.train() if mode == "train" else prob.eval()
                J, G, R, T = evaluate(prob, z0s, Us, nt, alph[0])
                check_restatement(prob, z0s, Us, alph[0], J, G, R, T, f"{name} nt={nt} {mode}")
                out[f"{pre}/{mode}/loss"] = J
                out[f"{pre}/{mode}/report"] = R
                if lim:
                    out[f"{pre}/{mode}/grad_sum_t"] = G.sum(1)
                    out[f"{pre}/{mode}/grad_sum_k"] = G.sum(2)
                    out[f"{pre}/final"] = T[:, :, -1]
                else:
                    out[f"{pre}/{mode}/grad"] = G
                    out[f"{pre}/traj"] = T
            print(name, "nt", nt, "J(train)", out[f"{pre}/train/loss"], flush=True)
        # 10 Adam iterations in double (train mode, xInit, nt = 20) from the fixture's first U
        prob.train()
        u = torch.nn.Parameter(cases[20][1][0].clone())
        opt = torch.optim.Adam([{"params": u}], lr=0.1, weight_decay=0.0)
        losses = []
        for _ in range(10):
            opt.zero_grad()
            err = gb.objective(u, xInit, prob, 20, alph[0])
            losses.append(err.item())
            err.backward()
            opt.step()
        out[f"{name}/adam10/loss"] = np.array(losses)
        out[f"{name}/adam10/U"] = u.detach().numpy().copy()
        out[f"{name}/xInit"] = xInit.numpy()

    # ---- quadcopter
    qg = np.load(os.path.join(HERE, "baseline_quad.npz"))
    prob, xInit = gq.make_prob(DT)
    U = torch.from_numpy(qg["ckpt/ctrls"]).double()
    J, g = gq.loss_grad(U, xInit, prob)
    rows, traj = uq.report(xInit.reshape(1, -1), U.unsqueeze(0))
    Jr, gr = uq.objective(xInit.reshape(1, -1), U.unsqueeze(0), grad=True)
    assert abs(float(Jr[0]) - J) <= 1e-12 * abs(J) and float((gr[0] - g).abs().max()) <= 1e-12 * float(g.abs().max())
    out["quad/ckpt/loss"] = np.array(J)
    out["quad/ckpt/grad"] = g.numpy()
    out["quad/ckpt/rows"] = rows[0].numpy()
    out["quad/ckpt/traj"] = traj[0].numpy()
    lock = None
    for s in range(qg["lock/z0"].shape[0]):
        z0 = torch.from_numpy(qg["lock/z0"][s]).double()
        U0 = torch.from_numpy(qg["lock/U0"][s]).double()
        runs, agree = [], True
        for cap in CAPS:
            kw = dict(gq.LBFGS, **cap)
            f, it, ev, Uf = gq.lbfgs(z0, U0, prob, **kw)
            it2, ev2, Uf2 = quad_lbfgs_restated(z0, U0, **kw)
            agree &= (it, ev) == (it2, ev2) and float((Uf - Uf2).abs().max()) <= 1e-8 * float(Uf.abs().max())
            runs.append((f, it, ev, Uf))
        print(f"lock start {s}: restatement {'agrees' if agree else 'DISAGREES'} at all six caps", [(r[1], r[2]) for r in runs], flush=True)
        if agree:
            lock = s
            break
    assert lock is not None, "no lock start on which the restatement agrees with the reference at all six caps"
    meta["lock_start"] = lock
    for k, (f, it, ev, Uf) in enumerate(runs):
        out[f"quad/cap{k}/U"] = Uf.numpy()
        out[f"quad/cap{k}/loss"] = np.array(f)
        out[f"quad/cap{k}/counts"] = np.array([it, ev], dtype=np.int32)
    meta["caps"] = CAPS
    z0 = torch.from_numpy(qg["solve/z0"][0]).double()
    U0 = torch.from_numpy(qg["solve/U0"][0]).double()
    f, it, ev, _ = gq.lbfgs(z0, U0, prob, **gq.LBFGS)
    print(f"full solve: loss {f!r}, {it} iterations, {ev} evaluations", flush=True)
    out["quad/solve/loss"] = np.array(f)
    out["quad/solve/counts"] = np.array([it, ev], dtype=np.int32)
    meta["solve_max_iter"] = gq.LBFGS["max_iter"]

    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(HERE, "baseline_f64.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
