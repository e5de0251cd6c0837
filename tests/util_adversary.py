"""oracle-side helpers of the disturbance gradient's and the worst-case search's tests (CPU only: nothing here touches a GPU)

The yardstick of neuraloc_amd.disturbance_gradient is torch autograd of util_disturb.restate with W as a leaf (restate keeps the graph:
W.to(x.dtype) does), in fp64, with the fp32 run of the same restatement as the rule's own error (util_oracle.compare: four times that error,
floor 1e-6 of the scale).  Cases, screened starts and disturbances are util_disturb's, unchanged.  search() restates
neuraloc_amd.worst_case_disturbances in torch.  tests/test_adversary_gpu.py runs them on the GPU; tests/test_adversary_cpu.py pins
dw_grads to the oracle at W = 0 and checks that the comparator rejects two wrong answers on every case."""
import torch

import util_disturb as ud
import util_lane as ul
import util_mono as um
import util_oracle as uo
from oracle import ocflow_oracle as orc

OBJECTIVES = ("Jc", "control")
BWD_KERNEL = {"lane": "rollout_lane_bwd_kernel<states>", "mono": "rollout_mono_bwd_kernel<states>", "tile": "rollout_bwd_kernel<states>",
              "tile-fixed": "rollout_bwd_kernel<states>"}


def objective_alph(alph, objective):
    """the multipliers the objective is formed with: "control" is L + alph0 G alone"""
    a = [float(v) for v in alph[:6]]
    if objective == "control":
        a[3] = a[4] = a[5] = 0.0
    return a


def grads_wrt_W(sd, S, x, W, tspan, nt, stepper, alph, dtype, objective="Jc", scale=1.0, mutation=None):
    """-> dict Jc (float, the full objective's mean), cs [7], table [n, 7], dW [nt, n, d] = scale * d(mean objective)/dW, dx [n, d] likewise.
    The means are formed as util_disturb_train.grads_disturbed forms them, so that W = 0 and objective "Jc" give util_lane.autograd_grads'
    Jc bit for bit."""
    P = orc.PhiParams.from_state_dict({k: v.clone() for k, v in sd.items()}, dtype=dtype)
    xx = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    Wl = W.detach().cpu().to(dtype).clone().requires_grad_(True)
    tab = ud.restate(P, S.to(dtype), xx, Wl, list(tspan), nt, stepper, alph, mutation)["table"]
    cs = [torch.mean(tab[:, c].contiguous() if c in (1, 3, 4) else tab[:, c]) for c in range(7)]
    J = cs[0] + alph[0] * cs[1] + alph[3] * cs[2] + alph[4] * cs[3] + alph[5] * cs[4]
    a = objective_alph(alph, objective)
    Jo = J if objective == "Jc" else cs[0] + a[0] * cs[1]
    (Jo * scale).backward()
    return dict(Jc=float(J.detach()), cs=torch.stack([c.detach() for c in cs]), table=tab.detach(), dW=Wl.grad, dx=xx.grad)


_CACHE = {}


def case_grads(case, dtype, objective="Jc", n_total=None, rows=None, mutation=None):
    """grads_wrt_W on a util_disturb case's screened starts and disturbances (rows: a slice of them; n_total: the batch the mean runs over,
    default the rows given); cached and never modified"""
    key = (case, dtype, objective, n_total, None if rows is None else (rows.start, rows.stop), mutation)
    if key not in _CACHE:
        data = ud.case_data(case)
        x, W = data["x"], data["W"]
        if rows is not None:
            x, W = x[rows], W[:, rows]
        _CACHE[key] = grads_wrt_W(um.case_sd(case), um.spec(case), x, W, case.tspan, case.nt, case.stepper, case.alph, dtype, objective,
                                  x.shape[0] / (n_total or x.shape[0]), mutation)
    return _CACHE[key]


def median_path_norm(W):
    """the median over the rows of ||W_i||_2 over the row's whole [nt, d] path"""
    return float(W.double().pow(2).sum((0, 2)).sqrt().median())


def search(case, dtype, x, eps, steps, objective="control", step_size=None, mask=None, W0=None):
    """neuraloc_amd.worst_case_disturbances restated in torch in `dtype`: projected ascent on every row's own objective (autograd of
    util_disturb.restate, rows independent) over ||W_i|| <= eps, the best iterate per row kept, the initial one included
    -> dict W, objective [n], nominal [n], history [steps+1, n], bad (bool [n]: util_mono.near_edge over every iterate's states)"""
    P = orc.PhiParams.from_state_dict({k: v.clone() for k, v in um.case_sd(case).items()}, dtype=dtype)
    S, a, n = um.spec(case).to(dtype), objective_alph(case.alph, objective), x.shape[0]
    step = 2.5 * eps / max(steps, 1) if step_size is None else step_size
    mk = torch.ones(case.d, dtype=dtype) if mask is None else (torch.as_tensor(mask) != 0).to(dtype)
    W = torch.zeros(case.nt, n, case.d, dtype=dtype) if W0 is None else W0.to(dtype).clone()
    bad, hist, best_o, best_W = torch.zeros(n, dtype=torch.bool), [], None, W.clone()
    for it in range(steps + 1):
        Wl = W.clone().requires_grad_(True)
        stages, steps_, disp = [], [], []
        with ul.recording(stages, steps_):
            tab = ud.restate(P, S, x.to(dtype), Wl, list(case.tspan), case.nt, case.stepper, case.alph, None, disp)["table"]
        o = tab[:, 0] + a[0] * tab[:, 1] + a[3] * tab[:, 2] + a[4] * tab[:, 3] + a[5] * tab[:, 4]
        o.sum().backward()
        bad |= um.near_edge(case, torch.stack([s.detach() for s in stages] + [s.detach() for s in disp], 1).double())
        o = o.detach()
        hist.append(o)
        up = torch.ones(n, dtype=torch.bool) if best_o is None else o > best_o
        best_o = o.clone() if best_o is None else torch.where(up, o, best_o)
        best_W[:, up] = W[:, up]
        if it == steps:
            break
        g = Wl.grad * mk
        gn = g.pow(2).sum((0, 2)).sqrt()
        W = W + step * g / gn.clamp_min(1e-30)[None, :, None]
        wn = W.pow(2).sum((0, 2)).sqrt()
        W = W * torch.where(wn > eps, eps / wn, torch.ones_like(wn))[None, :, None]
    return dict(W=best_W, objective=best_o, nominal=hist[0], history=torch.stack(hist), bad=bad)


def ascent_reference(W, g, mask, step, eps):
    """nocf_disturbance_ascent_f32's formulas in fp64 -> the updated W [nt, n, d] (double)"""
    W, g = W.double().clone(), g.double()
    mk = torch.ones(W.shape[2], dtype=torch.float64) if mask is None else (mask != 0).double()
    gm = g * mk
    gn = gm.pow(2).sum((0, 2)).sqrt()
    ok = (gn > 0) & torch.isfinite(gn)
    W[:, ok] = W[:, ok] + step * gm[:, ok] / gn[ok][None, :, None]
    wn = W.pow(2).sum((0, 2)).sqrt()
    proj = ok & (wn > eps)
    W[:, proj] = W[:, proj] * (eps / wn[proj])[None, :, None]
    return W


def compare(got, want64, ref32):
    return uo.compare(got, want64, ref32)


def failures(res):
    return {k: v for k, v in res.items() if not v[0]}
