"""oracle-side helpers of risk-sensitive training's tests (CPU only: nothing here touches a GPU)

neuraloc_amd.weighted_ocflow_train differentiates J = sum_i w_i J_i over the rows of a disturbed rollout, neuraloc_amd.risk_ocflow_train a risk
measure of the J_i.  The yardstick is the pinned oracle under torch autograd, built the way util_disturb_train.grads_disturbed builds the mean:
util_disturb.restate's table, J_i = tab[i,0] + a0 tab[i,1] + a3 tab[i,2] + a4 tab[i,3] + a5 tab[i,4], and either the weighted sum of given
weights (weighted_grads) or the risk's value written out here from its definition (value_formula: a sort and a sum, a logsumexp), differentiated
as a whole (value_grads) -- not neuraloc_amd.risk_weights' closed form, which tests/test_risk_cpu.py holds to this file.  Cases, starts,
disturbances and the edge screen are util_disturb's; the comparator is util_oracle.compare (four times the fp32 restatement's own error, floor
1e-6 of the scale)."""
import math

import numpy as np
import torch

import util_disturb as ud
import util_disturb_train as ut
import util_mono as um
import util_noise as un
import util_oracle as uo
from oracle import ocflow_oracle as orc

WEIGHTED_KERNEL = {"lane": "rollout_lane_bwd_kernel<weighted>", "mono": "rollout_mono_bwd_kernel<weighted>",
                   "tile": "rollout_bwd_kernel<weighted>", "tile-fixed": "rollout_bwd_kernel<weighted>"}
FAMILY_CASES = [ud.CASES[1], ud.CASES[3], ud.CASES[5]]             # one per family: lane, one-CU, per-tile
GAP_FACTOR = 100.0                                                  # CVaR: fp64 gap at the tail's boundary >= this x the fp32 error on J


def row_costs(tab, alph):
    return tab[:, 0] + alph[0] * tab[:, 1] + alph[3] * tab[:, 2] + alph[4] * tab[:, 3] + alph[5] * tab[:, 4]


def tail_counts(level, R):
    """k = (1 - level) R -> (k, floor(k), k - floor(k)) with the floor taken at 1e-9 (0.2 * 5 is 1, not 0.9999999999999998)"""
    k = (1.0 - level) * R
    kf = int(math.floor(k + 1e-9))
    return k, kf, max(k - kf, 0.0)


def value_formula(J, risk, level, paths=None, mix=1.0):
    """the risk's value from its definition, differentiable in J [n]: groups of `paths` consecutive rows,
    value = (1/G) sum_g [(1 - mix) mean_g J + mix rho_g]"""
    n = J.shape[0]
    R = n if paths is None else paths
    assert n % R == 0
    Jg = J.reshape(n // R, R)
    if risk == "mean":
        rho = Jg.mean(1)
    elif risk == "entropic":
        rho = (torch.logsumexp(level * Jg, 1) - math.log(R)) / level
    else:
        k, kf, frac = tail_counts(level, R)
        srt = torch.sort(Jg, dim=1, descending=True).values
        rho = srt[:, :kf].sum(1) / k
        if kf < R and frac > 0.0:
            rho = rho + frac * srt[:, kf] / k
    return ((1.0 - mix) * Jg.mean(1) + mix * rho).mean()


def autograd_weights(J, risk, level, paths=None, mix=1.0):
    """(d value / dJ, value) by torch autograd of value_formula, in J's dtype"""
    Jv = J.detach().clone().requires_grad_(True)
    v = value_formula(Jv, risk, level, paths, mix)
    (g,) = torch.autograd.grad(v, Jv)
    return g, v.detach()


def case_weights(case, n=None):
    """[n] float32 weights drawn once per case: both signs, one exact zero, magnitudes over a range of about 100, of the order of 1 / n"""
    n = case.n if n is None else n
    g = torch.Generator().manual_seed(104729 * case.seed + 17 * n + 5)
    mag = 10.0 ** (2.0 * torch.rand(n, generator=g, dtype=torch.float64) - 2.0)          # 0.01 ... 1
    sgn = torch.where(torch.rand(n, generator=g, dtype=torch.float64) < 0.3, -1.0, 1.0)
    w = mag * sgn
    if n > 1:
        w[0], w[n - 1] = 1.0, -0.01                                                      # (the range's ends and both signs, whatever the draw)
    w[n // 2] = 0.0
    return (w / n).to(torch.float32)


def _params(sd, dtype):
    P = orc.PhiParams.from_state_dict({k: v.clone() for k, v in sd.items()}, dtype=dtype)
    for t in [*P.K, *P.b, P.w, P.A, P.cw, P.cb]:
        t.requires_grad_(True)
    return P


def _collect(P, xx):
    out = {"A": P.A.grad, "c.weight": P.cw.grad, "c.bias": P.cb.grad, "w.weight": P.w.grad}
    for i in range(P.nTh):
        out[f"N.layers.{i}.weight"], out[f"N.layers.{i}.bias"] = P.K[i].grad, P.b[i].grad
    out["x"] = xx.grad
    return out


def objective_grads(case, x, W, dtype, objective):
    """objective(J [n]) of the disturbed restatement in `dtype`, differentiated by torch autograd -> (value, {parameter name: gradient,
    "x": d/dx}, J [n] detached).  A parameter the objective does not reach has gradient None."""
    P = _params(um.case_sd(case), dtype)
    xx = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    tab = ud.restate(P, um.spec(case).to(dtype), xx, W.detach().cpu(), list(case.tspan), case.nt, case.stepper, case.alph)["table"]
    J = row_costs(tab, case.alph)
    v = objective(J)
    v.backward()
    return float(v.detach()), _collect(P, xx), J.detach()


_CACHE = {}


def weighted_grads(case, dtype, weights=None, rows=None):
    """the reference of weighted_ocflow_train on a util_disturb case's screened starts and disturbances: J = sum_i w_i J_i
    (weights: default case_weights(case); rows: an index tensor / slice of the rows that take part, with their weights) -> dict Jw, grads"""
    key = (case, dtype, None if weights is None else tuple(weights.tolist()), None if rows is None else tuple(torch.arange(case.n)[rows].tolist()))
    if key not in _CACHE:
        data = ud.case_data(case)
        w = case_weights(case) if weights is None else weights
        x, W = data["x"], data["W"]
        if rows is not None:
            x, W, w = x[rows], W[:, rows], w[rows]
        v, g, _ = objective_grads(case, x, W, dtype, lambda J: (w.to(dtype) * J).sum())
        _CACHE[key] = dict(Jw=v, grads=g)
    return _CACHE[key]


def compare_grads(got, g64, g32):
    """util_disturb_train.compare_grads with a zero for a gradient autograd does not have"""
    w64, w32 = dict(g64), dict(g32)
    for k in w64:
        if w64[k] is None:
            w64[k] = torch.zeros_like(got[k], dtype=torch.float64)
        if w32[k] is None:
            w32[k] = torch.zeros_like(got[k], dtype=torch.float32)
    return ut.compare_grads(got, w64, w32)


failures = ut.failures

# ---------------------------------------------------------------------------------------------------------------------------------
# risk cases: S starts of a util_disturb case, each under R paths of the counter-based noise
# ---------------------------------------------------------------------------------------------------------------------------------
RISK_STARTS, RISK_PATHS, RISK_SEED = 5, 4, 20261
# (risk, level): CVaR at a fractional k = 2.4 and at an integer k = 2; the entropic theta is set per case from the fp64 costs' spread
RISK_LEVELS = [("cvar", 0.4), ("cvar", 0.5), ("entropic", None)]


AMP_MAX = 100.0          # a row's dJ/dx may move by at most this many times the relative size of a perturbation of its start
AMP_EXTRA = 3            # candidates: the case's first S + AMP_EXTRA screened starts


def _cpu_noise(case, rows, seed):
    ref, _, _ = un.disturbances(seed, case.nt, rows, case.d, ud.SIGMA_REL * case.rad, case.tspan)
    return torch.from_numpy(np.ascontiguousarray(ref)).to(torch.float32)


def amplification(case, x, W):
    """[rows]: how far a row's fp64 dJ/dx moves, relative to its largest entry, when the row's start is perturbed by 2^-24 relative (fixed
    signs) -- in units of 2^-24: the row's condition number, from the fp64 reference alone.  The comparator takes the LARGEST error over a
    tensor against the fp32 restatement's largest error; a row that amplifies rounding a thousandfold makes both the error of a handful of
    entries, which differs severalfold between two correct fp32 computations (two CPUs' matrix products), and the rule a coin toss."""
    g0 = objective_grads(case, x, W, torch.float64, lambda J: J.sum())[1]["x"]
    sgn = torch.where(torch.rand(x.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64) < 0.5, -1.0, 1.0)
    g1 = objective_grads(case, x.double() * (1.0 + 2.0 ** -24 * sgn), W, torch.float64, lambda J: J.sum())[1]["x"]
    return (g1 - g0).abs().max(1).values / (2.0 ** -24 * g0.abs().max(1).values)


def risk_inputs(case, seed=RISK_SEED, W=None):
    """x [S R, d] (S of the case's screened starts, each R times: repeat_interleave), sigma, and the noise W [nt, S R, d] float32 on the
    CPU: util_noise's restatement of the generator rounded to float32, or the tensor given (the device's own values).  The starts are the
    first S of the case's first S + AMP_EXTRA whose R paths all have amplification() <= AMP_MAX (chosen under the restated noise, whatever W
    is given: the choice needs no device)."""
    key = ("starts", case, seed)
    if key not in _CACHE:
        cand = ud.case_data(case)["x"][:RISK_STARTS + AMP_EXTRA]
        xc = cand.repeat_interleave(RISK_PATHS, 0).contiguous()
        amp = amplification(case, xc, _cpu_noise(case, xc.shape[0], seed)).reshape(-1, RISK_PATHS).max(1).values
        keep = (amp <= AMP_MAX).nonzero().flatten()[:RISK_STARTS]
        assert keep.numel() == RISK_STARTS, f"{case.id}: only {keep.numel()} of {cand.shape[0]} starts are conditioned well enough ({amp.tolist()})"
        _CACHE[key] = cand[keep].repeat_interleave(RISK_PATHS, 0).contiguous()
    x = _CACHE[key]
    if W is None:
        W = _cpu_noise(case, x.shape[0], seed)
    return x, ud.SIGMA_REL * case.rad, W.detach().cpu()


def cvar_gaps(J64, level, R):
    """the smallest fp64 gap between two neighbours in the descending order of a group whose CVaR weights differ"""
    k, kf, frac = tail_counts(level, R)
    srt = torch.sort(J64.reshape(-1, R), dim=1, descending=True).values
    gaps = []
    if 1 <= kf < R and frac < 1.0:
        gaps.append(srt[:, kf - 1] - srt[:, kf])                  # the last full-weight row against the boundary row
    if frac > 0.0 and kf + 1 < R:
        gaps.append(srt[:, kf] - srt[:, kf + 1])                  # the boundary row against the first row outside
    return float(torch.stack(gaps).min()) if gaps else float("inf")


def risk_case(case, risk, level, seed=RISK_SEED, W=None):
    """One risk case, built and checked on the CPU: the inputs, the fp64 and fp32 references of weights, value, rho and the gradient of the
    VALUE ITSELF (value_formula under autograd through the restated oracle).  Asserts what makes the comparison meaningful: no evaluated
    state near a decision edge, no badly conditioned row (amplification), and for CVaR the fp64 gap at the tail's boundary >= GAP_FACTOR x the fp32 restatement's error on J."""
    key = ("risk", case, risk, level, seed, None if W is None else hash(W.cpu().numpy().tobytes()))
    if key in _CACHE:
        return _CACHE[key]
    x, sigma, Wc = risk_inputs(case, seed, W)
    if ("rows",) + key[1:2] + key[4:] not in _CACHE:                # (the rows' costs serve every risk and level of the case)
        r64 = ud.case_restate(case, x.double(), Wc, torch.float64)
        assert not bool(um.near_edge(case, r64["stages"]).any()), f"{case.id}: a noise path of seed {seed} comes near a decision edge"
        amp = float(amplification(case, x, Wc).max())
        assert amp <= AMP_MAX, f"{case.id}: a row amplifies a perturbation of its start {amp:.0f}-fold (> {AMP_MAX})"
        _CACHE[("rows",) + key[1:2] + key[4:]] = (row_costs(r64["table"], case.alph),
                                                  row_costs(ud.case_restate(case, x, Wc, torch.float32)["table"], case.alph))
    J64, J32 = _CACHE[("rows",) + key[1:2] + key[4:]]
    e32 = float((J32.double() - J64).abs().max())
    if risk == "entropic" and level is None:
        level = 2.0 / float((J64.reshape(-1, RISK_PATHS).max(1).values - J64.reshape(-1, RISK_PATHS).min(1).values).mean())
    if risk == "cvar":
        gap = cvar_gaps(J64, level, RISK_PATHS)
        assert gap >= GAP_FACTOR * e32, f"{case.id} level {level}: gap {gap:.3e} at the tail's boundary < {GAP_FACTOR} x fp32 error {e32:.3e}"
    out = dict(x=x, sigma=sigma, W=Wc, seed=seed, level=level, e32=e32)
    for name, dtype in (("r64", torch.float64), ("r32", torch.float32)):
        v, g, J = objective_grads(case, x, Wc, dtype, lambda Jv: value_formula(Jv, risk, level, RISK_PATHS, 1.0))
        w, _ = autograd_weights(J, risk, level, RISK_PATHS, 1.0)
        out[name] = dict(value=torch.tensor(v, dtype=dtype), grads=g, weights=w, J=J)
    _CACHE[key] = out
    return out
