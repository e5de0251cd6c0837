"""oracle-side helpers of disturbed training's tests (CPU only: nothing here touches a GPU)

The reference has no rollout under per-step disturbances, so the yardstick of neuraloc_amd.disturbed_ocflow_train is the pinned oracle under
torch autograd: grads_disturbed() is util_lane.autograd_grads with util_disturb.restate (the disturbed rollout written with the oracle's
steppers and terminal block) in place of oracle.rollout.  Cases, starts, disturbances and the edge screen are util_disturb's, unchanged.
tests/test_disturb_train_gpu.py runs them on the GPU; tests/test_disturb_train_cpu.py pins this helper to the oracle at W = 0 and checks
that the comparator rejects wrong restatements' gradients."""
import torch

import util_disturb as ud
import util_mono as um
import util_oracle as uo
from oracle import ocflow_oracle as orc


def grads_disturbed(sd, S, x, W, tspan, nt, stepper, alph, dtype, scale=1.0, mutation=None):
    """Jc of the disturbed restatement in `dtype` and, by torch autograd, scale * dJc/dtheta and scale * dJc/dx
    -> (Jc, {parameter name: gradient}, x gradient, cs [7]).  S: ProbSpec (CPU); W [nt, n, d] (converted to dtype, no gradient).
    Jc = mean L + a0 mean G + a3 mean HJt + a4 mean HJfin + a5 mean HJgrad over the table's columns, the means formed as oracle.rollout
    forms them (a strided column for the four cost integrals, a contiguous one for G, HJfin and HJgrad), so that W = 0 reproduces
    util_lane.autograd_grads bit for bit.  mutation: one of util_disturb.MUTATIONS."""
    P = orc.PhiParams.from_state_dict({k: v.clone() for k, v in sd.items()}, dtype=dtype)
    for t in [*P.K, *P.b, P.w, P.A, P.cw, P.cb]:
        t.requires_grad_(True)
    xx = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    tab = ud.restate(P, S.to(dtype), xx, W.detach().cpu(), list(tspan), nt, stepper, alph, mutation)["table"]
    cs = [torch.mean(tab[:, c].contiguous() if c in (1, 3, 4) else tab[:, c]) for c in range(7)]
    J = cs[0] + alph[0] * cs[1] + alph[3] * cs[2] + alph[4] * cs[3] + alph[5] * cs[4]
    (J * scale).backward()
    out = {"A": P.A.grad, "c.weight": P.cw.grad, "c.bias": P.cb.grad, "w.weight": P.w.grad}
    for i in range(P.nTh):
        out[f"N.layers.{i}.weight"], out[f"N.layers.{i}.bias"] = P.K[i].grad, P.b[i].grad
    return float(J.detach()), out, xx.grad, torch.stack([c.detach() for c in cs])


_CACHE = {}


def case_grads(case, dtype, n_total=None, rows=None, mutation=None, w_scale=1.0):
    """grads_disturbed on a util_disturb case's screened starts and disturbances (rows: a slice of them; n_total: the batch the means run
    over, default the rows given) -> dict Jc, grads, gx, cs; cached"""
    key = (case, dtype, n_total, None if rows is None else (rows.start, rows.stop), mutation, w_scale)
    if key not in _CACHE:
        data = ud.case_data(case)
        x, W = data["x"], data["W"] * w_scale
        if rows is not None:
            x, W = x[rows], W[:, rows]
        J, g, gx, cs = grads_disturbed(um.case_sd(case), um.spec(case), x, W, case.tspan, case.nt, case.stepper, case.alph, dtype,
                                       x.shape[0] / (n_total or x.shape[0]), mutation)
        _CACHE[key] = dict(Jc=J, grads=g, gx=gx, cs=cs)
    return _CACHE[key]


def compare_grads(got, g64, g32):
    """{name: gradient} (and "x": dJc/dx) against fp64 under util_oracle's rule (4 x the fp32 restatement's own error, floor 1e-6 of the
    scale) -> {name: (ok, err, tol, err32)}"""
    return {k: uo.compare(got[k], g64[k], g32[k]) for k in g64}


def with_x(r):
    """case_grads' dict -> one {name: gradient} dict with the start's gradient under "x" """
    out = dict(r["grads"])
    out["x"] = r["gx"]
    return out


def failures(res):
    return {k: v for k, v in res.items() if not v[0]}
