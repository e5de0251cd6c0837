"""Risk-sensitive training: per-sample weights in the adjoint kernels.

noisy_ocflow_train and disturbed_ocflow_train differentiate the batch MEAN of the per-sample costs.  A risk measure of those costs -- the
conditional value at risk of a start's noise paths, the entropic risk -- is a function rho(J_1 .. J_n) whose gradient is the weighted sum
sum_i w_i grad J_i with w = d rho / dJ, a function of the per-sample table the recording forward already returns.  The weighted adjoint
entries (nocf_rollout_bwd_small_rw_f32 / _mid_rw_f32 / _act_rw_f32: the full adjoint kernels of the three families with one weight per row
where the scalar 1 / n stands) form that sum in the one launch the mean costs today.

    risk_weights            (w [n], value) of "mean" / "cvar" / "entropic" over groups of consecutive rows; plain torch, no synchronisation
    weighted_ocflow_train   Jw = sum_i w_i J_i for GIVEN weights (tail risk, importance weights, a soft-max tilt), differentiable
    risk_ocflow_train       one recording forward, risk_weights on its table, the weighted adjoint: the exact gradient of the risk

Single precision, one GPU, one network.  No CPU or eager-torch fallback; every check raises before a device is touched."""
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .noise import _OCflowTrainNoisy, _check_row_offset, _check_seed, noise_corr_scales, noise_scale
from .train import _STEPPERS, _OCflowTrain, _OCflowTrainDisturbed

RISKS = ("mean", "cvar", "entropic")


def _row_costs(tab, alph):
    """J_i = L_i + a0 G_i + a3 HJt_i + a4 HJfin_i + a5 HJgrad_i from the [n, 7] per-sample table"""
    a = [float(v) for v in alph[:6]]
    return tab[:, 0] + a[0] * tab[:, 1] + a[3] * tab[:, 2] + a[4] * tab[:, 3] + a[5] * tab[:, 4]


def _check_risk(risk, level, paths, mix, n=None):
    if risk not in RISKS:
        raise ValueError(f"risk must be one of {RISKS}, got {risk!r}")
    level, mix = float(level), float(mix)
    if risk == "cvar" and not 0.0 <= level < 1.0:
        raise ValueError(f"risk='cvar' needs 0 <= level < 1, got {level}")
    if risk == "entropic" and not (level > 0.0 and level < float("inf")):
        raise ValueError(f"risk='entropic' needs a finite level (theta) > 0, got {level}")
    if not 0.0 <= mix <= 1.0:
        raise ValueError(f"mix must lie in [0, 1], got {mix}")
    if paths is not None:
        if isinstance(paths, bool) or not isinstance(paths, int) or paths < 1:
            raise ValueError(f"paths must be a Python int >= 1 or None, got {paths!r}")
        if n is not None and n % paths != 0:
            raise ValueError(f"the batch of {n} rows is not a whole number of groups of paths={paths} consecutive rows")
    return level, mix


def _group_risk(Jg, risk, level):
    """Jg [G, R] -> (u [G, R] = d rho_g / dJ, rho [G])"""
    G, R = Jg.shape
    if risk == "mean":
        return torch.full_like(Jg, 1.0 / R), Jg.mean(1)
    if risk == "entropic":
        t = level * Jg
        return torch.softmax(t, 1), (torch.logsumexp(t, 1) - math.log(R)) / level
    # cvar: the average of the (1 - level) R largest costs; the row at the boundary takes the fractional rest
    k = (1.0 - level) * R
    kf = min(int(math.floor(k + 1e-9)), R)
    rank = torch.arange(R, device=Jg.device)
    by_rank = (rank < kf).to(Jg.dtype) * (1.0 / k) + (rank == kf).to(Jg.dtype) * (max(k - kf, 0.0) / k)      # (formed on the device: no copy)
    order = torch.argsort(Jg, dim=1, descending=True, stable=True)
    u = torch.zeros_like(Jg).scatter_(1, order, by_rank.expand(G, R).contiguous())
    return u, (u * Jg).sum(1)


def risk_weights(persample, alph, risk, level, paths=None, mix=1.0, _rho=None):
    """The weights of a risk measure of the per-sample costs, and its value.
        J_i = L_i + a0 G_i + a3 HJt_i + a4 HJfin_i + a5 HJgrad_i        from the [n, 7] table of a rollout
        groups: consecutive blocks of `paths` rows (repeat_interleave's layout: the noise paths of one start); None: the whole batch.
                G groups of R rows
        "cvar", 0 <= level < 1:  k = (1 - level) R;  u = 1/k on the floor(k) largest J of the group, (k - floor(k))/k on the next one, 0
                                 elsewhere;  rho = sum u J  (level 0: the mean)
        "entropic", level = theta > 0:  u = softmax(theta J);  rho = (logsumexp(theta J) - log R) / theta
        "mean":  u = 1/R
        w_i = ((1 - mix)/R + mix u_i)/G ,   value = (1/G) sum_g [(1 - mix) mean_g J + mix rho_g] ,   sum w = 1
    w is d value / dJ: everywhere for the entropic risk and the mean, wherever the group has no tie at the boundary for CVaR.
    Plain torch in persample's dtype on its device; nothing synchronises.  -> (w [n], value)"""
    if not isinstance(persample, torch.Tensor) or persample.dim() != 2 or persample.shape[1] != 7 or persample.shape[0] < 1:
        raise ValueError("persample must be an n-by-7 tensor")
    if len(alph) < 6:
        raise ValueError("alph needs 6 entries")
    n = persample.shape[0]
    level, mix = _check_risk(risk, level, paths, mix, n)
    R = n if paths is None else paths
    G = n // R
    with torch.no_grad():
        Jg = _row_costs(persample, alph).reshape(G, R)
        u, rho = _group_risk(Jg, risk, level)
        w = ((1.0 - mix) / R + mix * u) / G
        value = ((1.0 - mix) * Jg.mean(1) + mix * rho).mean()
    if _rho is not None:
        _rho.append(rho)
    return w.reshape(n), value


class _OCflowTrainWeighted(torch.autograd.Function):
    """_OCflowTrainDisturbed / _OCflowTrainNoisy with a weighted sum over the rows in place of their mean: the same recording forward
    (nocf_rollout_record_disturbed_f32 / nocf_rollout_record_noisy_f32: the lane, one-CU or per-tile kernel, never the split-role kernel), and as
    backward ONE launch of the weighted entry of the forward's family, picked in _OCflowTrain._adjoint's lane -> one-CU -> per-tile order.
    wspec: a [n] tensor (given weights: J = sum w_i J_i) or (risk, level, paths, mix) (the weights are risk_weights of the forward's own table:
    J = the risk's value, whose gradient those weights give)"""

    @staticmethod
    def forward(ctx, x, net, prob, tspan, nt, stepper, alph, dist, wspec, *params):
        if dist[0] == "W":
            _, means = _OCflowTrainDisturbed.forward(ctx, x, net, prob, tspan, nt, stepper, alph, None, None, dist[1])
        else:
            _, means = _OCflowTrainNoisy.forward(ctx, x, net, prob, tspan, nt, stepper, alph, None, None, dist[1])
        ctx.n_plain_args = 8
        tab = ctx.persample
        ctx.persample = None
        if isinstance(wspec, torch.Tensor):
            w = wspec.detach().contiguous()
            J = (w * _row_costs(tab, alph)).sum()
            rho = w.new_empty(0)
            w_out = w.new_empty(0)
        else:
            risk, level, paths, mix = wspec
            keep = []
            w, J = risk_weights(tab, alph, risk, level, paths, mix, _rho=keep)
            w = w.to(torch.float32).contiguous()
            rho, w_out = keep[0], w.clone()
        ctx.wrow = w
        ctx.mark_non_differentiable(means, tab, w_out, rho)
        return J, means, tab, w_out, rho

    @staticmethod
    @once_differentiable
    def backward(ctx, gJ, _gmeans, _gtab, _gw, _grho):
        return _OCflowTrain._adjoint(ctx, gJ, wrow=ctx.wrow)


def _checked_call(what, x, net, prob, tspan, nt, W, sigma, seed, mask, row_offset, stepper, alph, n_total, group, weights=None, rho=None):
    """every refusal of weighted_ocflow_train / risk_ocflow_train, in front of anything that touches a device -> (alph, dist)"""
    from .ensemble import PhiEnsemble
    if isinstance(net, PhiEnsemble):
        raise NotImplementedError(f"{what}: ensembles are not supported; the weighted adjoint takes one network")
    if n_total is not None or group is not None:
        raise NotImplementedError(f"{what}: sharded batches (n_total / group) are not supported; the weights already carry the normalisation "
                                  "and the call runs on one GPU")
    alph = list(net.alph if alph is None else alph)
    tensors = [("x", x), ("W", W), ("weights", weights)] + [(name, p_) for name, p_ in net.named_parameters()]
    if isinstance(sigma, torch.Tensor):
        tensors.append(("sigma", sigma))
    if isinstance(rho, torch.Tensor):
        tensors.append(("rho", rho))
    for name, t in tensors:
        if isinstance(t, torch.Tensor) and t.dtype == torch.float64:
            raise NotImplementedError(f"{what}: {name} is float64; double precision is not supported: the weighted adjoint is single precision only "
                                      "(the double-precision kernels take no disturbance and no weights)")
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if stepper not in _STEPPERS:
        raise ValueError(f"stepper must be 'rk4' or 'rk1', got {stepper!r}")
    if x.dim() != 2:
        raise ValueError("x must be nex-by-d")
    n, d = x.shape
    if d != net.d:
        raise ValueError(f"x has d={d} but Phi was built for d={net.d}")
    pd_ = getattr(prob, "d", None)
    if pd_ is not None and int(pd_) != d:
        raise ValueError(f"the problem object has d={pd_} but x has d={d}")
    if int(nt) < 1:
        raise ValueError("nt must be >= 1")
    if n < 1:
        raise ValueError("x has no rows")
    if len(alph) < 6:
        raise ValueError("alph needs 6 entries")
    if (W is None) == (sigma is None):
        raise ValueError(f"{what}: exactly one of W and sigma (with seed) must be given; sigma=0.0 runs undisturbed")
    if W is not None:
        if seed is not None:
            raise ValueError(f"{what}: seed belongs to sigma; W is a tensor of given disturbances")
        if rho is not None:
            raise ValueError(f"{what}: rho belongs to sigma (the noise drawn inside the kernel); W is a tensor of given disturbances")
        if not isinstance(W, torch.Tensor):
            raise TypeError("W must be a torch.Tensor")
        if tuple(W.shape) != (int(nt), n, d):
            raise ValueError(f"W must be nt-by-nex-by-d = {(int(nt), n, d)}, got {tuple(W.shape)}")
        if W.requires_grad:
            raise NotImplementedError(f"{what}: W requires a gradient, but dJ/dW together with weights is not supported; pass W.detach()")
        if W.device != x.device:
            raise ValueError("x and W must be on the same device")
        dist = ("W", W)
    else:
        if seed is None:
            raise ValueError(f"{what}: sigma needs a seed")
        scale = noise_scale(sigma, nt, d, tspan, mask)
        corr = () if rho is None else tuple(noise_corr_scales(sigma, rho, nt, d, tspan, mask)[1:])
        dist = ("noise", (scale, _check_seed(seed), _check_row_offset(row_offset)) + corr)
    if weights is not None:
        if not isinstance(weights, torch.Tensor):
            raise TypeError("weights must be a torch.Tensor")
        if weights.dtype != torch.float32 or tuple(weights.shape) != (n,) or weights.requires_grad or weights.device != x.device:
            raise NotImplementedError(f"{what}: weights must be a float32 tensor of shape [{n}] on x's device that does not require a gradient "
                                      f"(got {weights.dtype}, {tuple(weights.shape)}, {weights.device}, requires_grad={weights.requires_grad}); "
                                      "anything else is not supported")
    return alph, dist


def _require_device(x, W):
    """the last refusal, behind every argument check: CPU tensors"""
    _lib.require_device_f32(x, "x")
    if W is not None:
        _lib.require_device_f32(W, "W")


def weighted_ocflow_train(x, net, prob, tspan, nt, weights, *, W=None, sigma=None, seed=None, mask=None, row_offset=0, stepper="rk4",
                          alph=None, n_total=None, group=None, rho=None):
    """The weighted sum of the per-sample training costs of a disturbed rollout:  Jw = sum_i weights[i] J_i ,
    J_i = L_i + a0 G_i + a3 HJt_i + a4 HJfin_i + a5 HJgrad_i, differentiable w.r.t. every parameter of `net` and w.r.t. x when x requires a
    gradient (x.grad[i] = weights[i] dJ_i/dx_i).  One recording forward and one launch of the weighted adjoint of the forward's family.
    :param weights: [nex] float32 on x's device, no gradient: any finite values (negative and zero included); 1/nex gives the mean
    :param W:     nt-by-nex-by-d disturbances (disturbed_ocflow_train's), or
    :param sigma, seed, mask, row_offset: the noise of noisy_ocflow_train, drawn inside the kernel.  Exactly one of W and sigma must be given;
                  sigma=0.0 (with any seed) runs undisturbed
    :param rho:   with sigma: a float or [d] in [0, 1), the time-correlated noise of noisy_ocflow_train(..., rho=); refused together with W
    :return: (Jw, cs) -- cs the 7 UNWEIGHTED means, as disturbed_ocflow_train logs them
    Single precision, one GPU, one network: float64 anywhere, CPU tensors, n_total / group and ensembles are refused (NotImplementedError /
    RuntimeError), before anything is launched and with every .grad untouched."""
    if not isinstance(weights, torch.Tensor):
        raise TypeError("weights must be a torch.Tensor")
    alph, dist = _checked_call("weighted_ocflow_train", x, net, prob, tspan, nt, W, sigma, seed, mask, row_offset, stepper, alph,
                               n_total, group, weights, rho=rho)
    _require_device(x, W)
    params = [p for _, p in net.named_parameters()]
    Jw, means, _, _, _ = _OCflowTrainWeighted.apply(x, net, prob, list(tspan), int(nt), stepper, alph, dist, weights, *params)
    return Jw, [means[i] for i in range(7)]


def risk_ocflow_train(x, net, prob, tspan, nt, risk, level, *, paths=None, mix=1.0, W=None, sigma=None, seed=None, mask=None, row_offset=0,
                      stepper="rk4", alph=None, n_total=None, group=None, rho=None):
    """A risk measure of the per-sample training costs as the objective: one recording forward, risk_weights on its table, and the weighted
    adjoint as the backward -- one forward launch and one adjoint launch, the cost of a mean.
    :param risk, level, paths, mix: risk_weights' ("cvar" with 0 <= level < 1, "entropic" with level = theta > 0, or "mean"; groups of `paths`
                  consecutive rows, the layout x.repeat_interleave(paths, 0) gives; mix blends the risk with the group's mean)
    :param W / sigma, seed, mask, row_offset, stepper, alph, rho: as for weighted_ocflow_train
    :return: (Jr, cs, info): Jr = risk_weights' value, differentiable w.r.t. the parameters and x -- the exact gradient of the value
             (everywhere for the entropic risk; wherever no group has a tie at the VaR boundary for CVaR); cs the 7 unweighted means;
             info = dict(weights [nex], persample [nex, 7], rho [groups])
    The refusals are weighted_ocflow_train's, and risk_weights' argument checks; all of them come before anything is launched."""
    alph, dist = _checked_call("risk_ocflow_train", x, net, prob, tspan, nt, W, sigma, seed, mask, row_offset, stepper, alph, n_total, group,
                               rho=rho)
    level, mix = _check_risk(risk, level, paths, mix, x.shape[0])
    _require_device(x, W)
    params = [p for _, p in net.named_parameters()]
    Jr, means, tab, w, rho = _OCflowTrainWeighted.apply(x, net, prob, list(tspan), int(nt), stepper, alph, dist, (risk, level, paths, mix), *params)
    return Jr, [means[i] for i in range(7)], dict(weights=w, persample=tab, rho=rho)
