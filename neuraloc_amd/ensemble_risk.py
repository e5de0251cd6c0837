"""Risk-sensitive ensembles: per-row weights in the ensemble adjoints.

ensemble_noise.py rolls out and trains E networks under in-kernel Brownian noise in one launch each; risk.py trains ONE network on a risk
measure of its noise paths, the adjoint seeding row i with a weight w_i where 1 / n stands.  Here the two meet: the ensemble adjoints'
weighted instantiation (nocf_rollout_bwd_small_ensemble_rw_f32 / nocf_rollout_bwd_mid_ensemble_rw_f32) reads wrow [E, n], so a sweep over the
risk level -- CVaR at 0, 0.5, 0.8, 0.95, or over theta -- is one recording forward and one adjoint launch for all members, and member e's
results are bit for bit those of weighted_ocflow_train / risk_ocflow_train on ens.member(e) alone with (sigma_e, seed_e, mask, row_offset).

    w, value, rho = ensemble_risk_weights(persample, ens.alph, "cvar", [0.0, 0.5, 0.8, 0.95], paths=8)     # risk_weights per member
    Jw, cs = ensemble_weighted_ocflow_train(x, ens, prob, tspan, nt, weights, sigma=sigma, seed=seed)      # GIVEN weights [E, n]
    Jr, cs, info = ensemble_risk_ocflow_train(x, ens, prob, tspan, nt, "cvar", [0.0, 0.5, 0.8, 0.95], paths=8, sigma=sigma, seed=seed)

Single precision, one device, family "lane" or "mid" as in ensemble.py.  No CPU or eager-torch fallback: everything else is refused before a
device is touched, CPU tensors last."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib, ensemble
from .ensemble import FAMILIES, PhiEnsemble, _alph_rows, _refuse
from .ensemble_noise import _Noise, scale_table, seed_list
from .noise import _check_row_offset
from .risk import _check_risk, _row_costs, risk_weights

SYMBOLS = tuple(ensemble._WEIGHTED[family] for family in FAMILIES)


def _per_member(value, members, name):
    """one value for all members or a sequence of E -> a list of E"""
    if isinstance(value, (list, tuple)):
        if len(value) != members:
            raise ValueError(f"{name} must be one value (every member the same) or a sequence of {members} (one per member), "
                             f"got {len(value)} entries")
        return list(value)
    return [value] * members


def _member_specs(risk, level, mix, members, paths, n=None):
    """risk / level / mix, each one value or E of them -> E tuples (risk_e, level_e, mix_e), every one checked as risk_weights checks it"""
    risks, levels, mixes = (_per_member(v, members, name) for v, name in ((risk, "risk"), (level, "level"), (mix, "mix")))
    return [(r_,) + _check_risk(r_, lv, paths, mx, n) for r_, lv, mx in zip(risks, levels, mixes)]


def ensemble_risk_weights(persample, alph_rows, risk, level, paths=None, mix=1.0):
    """risk_weights for every member of an ensemble.
    :param persample: [E, n, 7], the members' per-sample tables (a lane launch's [E * n, 7] viewed member-major)
    :param alph_rows: one list of six multipliers or E rows of six (ens.alph)
    :param risk, level, mix: each one value for all members or a sequence of E -- a level sweep is level=[0.0, 0.5, 0.8, 0.95]; the members
                      may mix "cvar", "entropic" and "mean"
    :param paths:     groups of `paths` consecutive rows inside every member (None: a member's whole batch), common to the members
    :return: (w [E, n], value [E], rho [E, G]); member e's slices are bit for bit risk_weights(persample[e], alph_rows[e], risk_e, level_e,
             paths, mix_e) -- the members are formed one after the other by that function.  Plain torch, nothing synchronises."""
    if not isinstance(persample, torch.Tensor) or persample.dim() != 3 or persample.shape[2] != 7 or persample.shape[0] < 1 \
            or persample.shape[1] < 1:
        raise ValueError("persample must be an E-by-n-by-7 tensor")
    E, n = persample.shape[0], persample.shape[1]
    rows = _alph_rows(alph_rows, E)
    specs = _member_specs(risk, level, mix, E, paths, n)
    ws, values, rhos = [], [], []
    for e, (r_, lv, mx) in enumerate(specs):
        keep = []
        w, v = risk_weights(persample[e], rows[e], r_, lv, paths, mx, _rho=keep)
        ws.append(w)
        values.append(v)
        rhos.append(keep[0])
    return torch.stack(ws), torch.stack(values), torch.stack(rhos)


class _WeightedEnsembleTrain(torch.autograd.Function):
    """ensemble_noise's recording forward (ensemble._EnsembleTrain._forward / _EnsembleTrainMid._forward with its noise) with a weighted sum
    over every member's rows in place of their mean, and as backward ONE launch of the weighted ensemble adjoint of the family.
    wspec: a [E, n] tensor (given weights: J_e = sum_i w_ei J_ei) or (specs, paths) (the weights are ensemble_risk_weights of the forward's own
    table: J_e = the value of member e's risk, whose gradient those weights give)"""

    @staticmethod
    def forward(ctx, x, ens, prob, tspan, nt, stepper, alph, noise, family, wspec, *params):
        base = ensemble._EnsembleTrainMid if family == "mid" else ensemble._EnsembleTrain
        _Jc, cs = base._forward(ctx, x, ens, prob, tspan, nt, stepper, alph, noise)
        ctx.family = family
        E = ens.members
        tab = ctx.persample.view(E, -1, 7)                          # (lane: [E * n, 7], member-contiguous; one-CU: [E, n, 7])
        ctx.persample = None
        rows = ens.alph if alph is None else _alph_rows(alph, E)
        if isinstance(wspec, torch.Tensor):
            w = wspec.detach().contiguous()
            # per member the statements of the single-network call on the member's [n, 7] block: the same bits
            J = torch.stack([(w[e] * _row_costs(tab[e], rows[e])).sum() for e in range(E)])
            rho = w.new_empty(0)
            w_out = w.new_empty(0)
        else:
            specs, paths = wspec
            risks, levels, mixes = zip(*specs)
            w, J, rho = ensemble_risk_weights(tab, rows, list(risks), list(levels), paths, list(mixes))
            w = w.to(torch.float32).contiguous()
            w_out = w.clone()
        ctx.wrow = w
        ctx.mark_non_differentiable(cs, tab, w_out, rho)
        return J, cs, tab, w_out, rho

    @staticmethod
    @once_differentiable
    def backward(ctx, gJ, _gcs, _gtab, _gw, _grho):
        base = ensemble._EnsembleTrainMid if ctx.family == "mid" else ensemble._EnsembleTrain
        g = base._adjoint(ctx, gJ, wrow=ctx.wrow)                   # (x, six plain arguments, the parameters)
        return g[:7] + (None,) * 3 + g[7:]


def _prepare(fn, x, ens, prob, tspan, nt, sigma, seed, mask, row_offset, stepper, family, W, n_total, group, weights=None, risk=None):
    """every refusal of ensemble_weighted_ocflow_train / ensemble_risk_ocflow_train, in front of anything that touches a device
    -> (_Noise, member specs or None).  risk: (risk, level, paths, mix) of ensemble_risk_ocflow_train"""
    if W is not None:
        raise NotImplementedError(f"{fn}: a disturbance tensor W is not supported for ensembles; the members' noise is drawn in the kernel "
                                  "(sigma, seed)")
    if n_total is not None or group is not None:
        raise NotImplementedError(f"{fn}: sharded batches (n_total / group) are not supported; the weights already carry the normalisation "
                                  "and the call runs on one GPU")
    if family not in FAMILIES:
        raise ValueError(f"{fn}: family must be 'lane' (the small-network lane kernels) or 'mid' (the one-CU kernels), got {family!r}")
    for name, t in (("weights", weights), ("sigma", sigma)):
        if isinstance(t, torch.Tensor) and t.dtype == torch.float64:
            raise RuntimeError(f"{fn}: {name} is float64; ensembles are single precision only (the double-precision kernels take one network "
                               "and no weights)")
    row_offset = _check_row_offset(row_offset)
    nz = specs = None
    if isinstance(ens, PhiEnsemble) and isinstance(x, torch.Tensor) and (x.dim() == 2 or (x.dim() == 3 and x.shape[0] == ens.members)):
        E, n, d = ens.members, int(x.shape[-2]), int(x.shape[-1])
        if weights is not None and (weights.dtype != torch.float32 or tuple(weights.shape) != (E, n) or weights.requires_grad
                                    or weights.device != x.device):
            raise NotImplementedError(f"{fn}: weights must be a float32 tensor of shape [{E}, {n}] (members by rows) on x's device that does "
                                      f"not require a gradient (got {weights.dtype}, {tuple(weights.shape)}, {weights.device}, "
                                      f"requires_grad={weights.requires_grad}); anything else is not supported")
        if risk is not None:
            specs = _member_specs(risk[0], risk[1], risk[3], E, risk[2], n)
        if int(nt) >= 1 and d >= 1:
            nz = _Noise(scale_table(sigma, E, nt, d, tspan, mask), seed_list(seed, E), row_offset)
    ensemble.weighted_entry(_lib.lib(), family)                      # (a library without the symbols: RuntimeError)
    _refuse(fn, x, ens, prob, nt, stepper, True, family=family)      # shapes and float64 of x and the parameters; CPU tensors last
    return nz, specs


def ensemble_weighted_ocflow_train(x, ens, prob, tspan, nt, weights, *, sigma=0.0, seed=0, mask=None, row_offset=0, stepper="rk4", alph=None,
                                   family="lane", W=None, n_total=None, group=None):
    """The weighted sums of every member's per-sample training costs:  Jw[e] = sum_i weights[e, i] J_{e,i} , J_{e,i} = L + a0 G + a3 HJt +
    a4 HJfin + a5 HJgrad of row i of member e under member e's multipliers; differentiable in every stacked parameter of `ens` (and in x when
    every member has its own starts: x.grad[e, i] = weights[e, i] dJ_{e,i}/dx).  One recording forward (ensemble_noisy_ocflow_train's) and
    ONE launch of the weighted ensemble adjoint of the family.
    :param weights: [E, nex] float32 on x's device, no gradient: any finite values (negative and zero included); 1 / nex gives
                  ensemble_noisy_ocflow_train's bits
    :param sigma, seed, mask, row_offset: the noise of ensemble_noisy_ocflow_train, per member exactly as there; a row of zeros (the default)
                  runs that member undisturbed
    :param x, ens, prob, tspan, nt, stepper, alph, family: as for ensemble_ocflow_train
    :return: (Jw [E], cs [E, 7]) -- cs the UNWEIGHTED means.  An upstream gradient gJ [E] scales each member's gradients.
    Member e's Jw, gradients and x.grad[e] are bit for bit those of weighted_ocflow_train + backward() on ens.member(e) with weights[e],
    sigma_e, seed_e, mask and row_offset.  float64 anywhere, a tensor W, n_total / group, a shape outside the family and CPU tensors are
    refused before anything is launched and with every .grad untouched."""
    if not isinstance(weights, torch.Tensor):
        raise TypeError("weights must be a torch.Tensor")
    nz, _ = _prepare("ensemble_weighted_ocflow_train", x, ens, prob, tspan, nt, sigma, seed, mask, row_offset, stepper, family, W, n_total,
                     group, weights=weights)
    params = [p for _, p in ens._params()]
    Jw, cs, _, _, _ = _WeightedEnsembleTrain.apply(x, ens, prob, [float(tspan[0]), float(tspan[1])], int(nt), stepper, alph, nz, family,
                                                   weights, *params)
    return Jw, cs


def ensemble_risk_ocflow_train(x, ens, prob, tspan, nt, risk, level, *, paths=None, mix=1.0, sigma, seed, mask=None, row_offset=0,
                               stepper="rk4", alph=None, family="lane", W=None, n_total=None, group=None):
    """A risk measure of every member's per-sample training costs as that member's objective -- each member its own measure and level: one
    recording forward, ensemble_risk_weights on its table, and the weighted ensemble adjoint as the backward.
    :param risk, level, mix: each one value for all members or a sequence of E (ensemble_risk_weights'); level=[0.0, 0.5, 0.8, 0.95] is a sweep
                  of the CVaR level over four members
    :param paths: groups of `paths` consecutive rows of every member: the layout x.repeat_interleave(paths, -2) gives
    :param sigma, seed, mask, row_offset, stepper, alph, family: as for ensemble_weighted_ocflow_train (sigma and seed are required)
    :return: (Jr [E], cs [E, 7], info): Jr[e] = the value of member e's risk, differentiable; cs the unweighted means;
             info = dict(weights [E, nex], persample [E, nex, 7], rho [E, groups]).  Member e's values, gradients and x.grad[e] are bit for bit
             those of risk_ocflow_train + backward() on ens.member(e) with (risk_e, level_e, paths, mix_e, sigma_e, seed_e).
    The refusals are ensemble_weighted_ocflow_train's, and risk_weights' argument checks for every member; all come before a launch."""
    nz, specs = _prepare("ensemble_risk_ocflow_train", x, ens, prob, tspan, nt, sigma, seed, mask, row_offset, stepper, family, W, n_total,
                         group, risk=(risk, level, paths, mix))
    params = [p for _, p in ens._params()]
    Jr, cs, tab, w, rho = _WeightedEnsembleTrain.apply(x, ens, prob, [float(tspan[0]), float(tspan[1])], int(nt), stepper, alph, nz, family,
                                                       (specs, paths), *params)
    return Jr, cs, dict(weights=w, persample=tab, rho=rho)
