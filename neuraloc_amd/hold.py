"""Zero-order-hold rollouts: the control is refreshed every K-th step and applied, unchanged, in between.

Every other rollout of the package re-evaluates the feedback law at every Runge-Kutta stage.  A deployed controller samples the state,
evaluates the network once and applies that control until the next sample; here that is ONE launch (nocf_rollout_held_f32, the contract in
include/nocf.h):

    z = [x, 0, 0, 0, 0]
    for k in 0 .. nt-1:
        if k % K == 0:  c = calcCtrls(x_k, grad_x Phi(x_k, t_k))      # the state the controller really meets: W[k-1] is already on it
        z = step(z) with the right-hand side [ f(x, c) | L(x, c) | 0 | Q(x) | W(x) ]
        if W: z[:, :d] += W[k]
    terminal block at z(T), unchanged

The network runs ceil(nt / K) + 1 times where OCflow runs it 4 nt + 1 times; a held step is the problem physics and the cost quadrature
alone, the control coming from registers or LDS.  The lane (m <= 32, point agents) and one-CU (m <= 128) kernels only; single precision; an
evaluation (no autograd); one network; quadcopter problems with one craft.  There is no CPU or eager-torch fallback, and every check raises
before anything is enqueued."""
import numbers

import torch

from . import _lib
from .OCflow import _evaluate, _launch
from .disturb import disturbed_rollout, path_statistics

_FAMILIES = ("the held rollout runs on the lane kernel (nTh = 2, m <= 32, d + 1 <= 32, point agents, at most 16 of them) and on the one-CU "
             "kernel (nTh = 2, m <= 128, d + 1 <= 32) only")


def _entry(L):
    """nocf_rollout_held_f32 of library L; a library without it is an error, never a fallback"""
    return _lib.require(L, ("nocf_rollout_held_f32",), "held_rollout")[0]


def check_hold(hold, what="held_rollout"):
    """hold as a Python int >= 1 (ValueError otherwise: bools, floats, 0 and negative values)"""
    if isinstance(hold, bool) or not isinstance(hold, numbers.Integral) or int(hold) < 1:
        raise ValueError(f"{what}: hold must be an integer >= 1 (the control is refreshed every hold-th step), got {hold!r}")
    if int(hold) >= 2 ** 31:
        raise ValueError(f"{what}: hold must fit 32 bits, got {hold!r}")
    return int(hold)


def hold_family(net, prob):
    """"lane" / "one-CU": the kernel family a held rollout of this network and problem takes by its shape, or None (host attributes only)"""
    quad = prob.KIND == _lib.PROB_QUADCOPTER
    if net.nTh != 2 or net.d + 1 > 32:
        return None
    if net.m <= 32 and not quad and prob.nAgents <= 16:
        return "lane"
    return "one-CU" if net.m <= 128 else None


def _refuse(what, x, net, prob, hold, W=None, n_total=None, group=None):
    """every refusal of a held call, in an order that needs no device: -> hold as an int"""
    from .ensemble import PhiEnsemble
    if isinstance(net, PhiEnsemble):
        raise NotImplementedError(f"{what}: a PhiEnsemble is not supported; the held rollout takes one network (no ensemble instantiation "
                                  "of the held kernels is built)")
    hold = check_hold(hold, what)
    if n_total is not None or group is not None:
        raise NotImplementedError(f"{what}: n_total / group belong to training; the held rollout is an evaluation of the rows it is given")
    if hold_family(net, prob) is None:
        raise NotImplementedError(f"{what}: nTh = {net.nTh}, m = {net.m}, d = {net.d}: {_FAMILIES}; the per-tile and split-role kernels "
                                  "take no held control")
    if prob.KIND == _lib.PROB_QUADCOPTER and prob.nAgents != 1:
        raise NotImplementedError(f"{what}: a quadcopter problem of {prob.nAgents} craft is not supported; the held rollout takes one craft")
    for name, t in (("x", x), ("W", W)):
        if isinstance(t, torch.Tensor) and t.dtype == torch.float64:
            raise RuntimeError(f"{what}: {name} is float64; the held rollout is single precision only (the double-precision kernel "
                               "takes no held control)")
    for name, p_ in net.named_parameters():
        if p_.dtype == torch.float64:
            raise RuntimeError(f"{what}: {name} is float64; the held rollout is single precision only")
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    net._guard_no_autograd(x, what)
    if W is not None and isinstance(W, torch.Tensor) and torch.is_grad_enabled() and W.requires_grad:
        raise NotImplementedError(f"{what}: W requires a gradient; the held rollout is an evaluation (no adjoint of it is built)")
    return hold


def _held(x, net, prob, tspan, nt, hold, W, stepper, alph, intermediates, what="held_rollout"):
    """the launch behind held_rollout -> (means [8], persample, z_final, zFull, ctrlFull), the last two time-major or None"""
    hold = _refuse(what, x, net, prob, hold, W)
    alph = list(net.alph if alph is None else alph)
    refused = NotImplementedError(f"{what}: nTh = {net.nTh}, m = {net.m}, d = {net.d}, r = {net.A.shape[0]}: no lane and no one-CU "
                                  f"instantiation takes this shape; {_FAMILIES}")
    # (the shipped library: a per-shape build specialises the per-tile kernels, which take no held control)
    means, persample, _sums, z_final, zFull, ctrlFull = _evaluate(what, "nocf_rollout_held_f32", x, net, prob, tspan, nt, stepper, alph,
                                                                  intermediates, extra=(hold,), W=W, shipped=True, shape_error=refused)
    return means, persample, z_final, zFull, ctrlFull


def held_rollout(x, net, prob, tspan, nt, hold, W=None, stepper="rk4", alph=None, intermediates=False, n_total=None, group=None):
    """
    :param x:    nex-by-d initial states on the MI355X, float32
    :param hold: K >= 1, a Python int: the control is sampled at steps 0, K, 2K, ... and held in between.  K = 1 still holds the control
                 over the four stages of a step; K >= nt is the open-loop rollout of the initial control
    :param W:    None, or nt-by-nex-by-d float32 on x's device: disturbed_rollout's tensor, W[k] added to the state behind step k.  The
                 controller samples the displaced state.  Not modified
    :param alph: 6 multipliers (default: net.alph)
    :return: Jc, cs, persample [nex, 7] ([L, G, HJt, HJfin, HJgrad, Q, W]; the HJt column is identically 0: a held control has no HJB
             residual, and Jc / cs are the existing means arithmetic on that table), z_final [nex, d+4]; with intermediates also
             traj [nex, d+4, nt+1] and ctrl [nex, a, nt+1] in the reference's layout, ctrl[:, :, k+1] the control APPLIED over step k
    n_total / group are training's and are refused, like everything that requires a gradient (NotImplementedError)."""
    _refuse("held_rollout", x, net, prob, hold, W, n_total, group)
    means, persample, z_final, zFull, ctrlFull = _held(x, net, prob, tspan, nt, hold, W, stepper, alph, intermediates)
    out = (means[7], [means[i] for i in range(7)], persample, z_final)
    if intermediates:
        out += (zFull.permute(1, 2, 0), ctrlFull.permute(1, 2, 0))
    return out


def _columns(tab, a0):
    """tab [starts, paths, 7] -> {name: [starts, paths]} for L + alph[0] G, G, L, Q, W"""
    return {"L+G": tab[:, :, 0] + a0 * tab[:, :, 1], "G": tab[:, :, 1], "L": tab[:, :, 0], "Q": tab[:, :, 5], "W": tab[:, :, 6]}


def hold_study(x, net, prob, nt, holds=(1, 2, 4, 8), sigma=None, seed=0, rho=None, paths=1, tspan=(0., 1.), alph=None, stepper="rk4",
               mask=None, max_rows=1 << 16):
    """What the trained law costs when its control is refreshed every K-th step, for every K of `holds`, on the same starts -- and, with
    sigma, under the same disturbances: W is drawn ONCE per chunk by noise.counter_disturbances(nt, rows, d, sigma, seed, tspan, mask,
    row_offset, rho=rho) and the same W goes to every K, so the rows of the result are a paired comparison.  Each start is repeated `paths`
    times as rows of one batch (start-major: row i * paths + p, noise_study's layout) in chunks of whole starts of at most max_rows rows,
    one launch per (K, chunk); start i, path p meets the noise of global row i * paths + p whatever max_rows is.
    :param sigma: None (no disturbance; paths must be 1), or a float or [d]
    :return: {K: entry} for every K of holds, and entry 0: the plain closed loop for reference (OCflow's noMean table without sigma,
             disturbed_rollout on the same W with it).  An entry holds "L+G" (L + alph[0] G), "G", "L", "Q", "W" -- without sigma each a
             [nex] tensor, with sigma each a dict mean / std / q05 / q50 / q95 of [nex] tensors over the paths -- and "persample"
             [nex, paths, 7], the table every figure is formed from"""
    from .noise import _check_seed, check_rho, counter_disturbances
    holds = [check_hold(k, "hold_study") for k in holds]
    if not holds:
        raise ValueError("hold_study: holds is empty")
    _refuse("hold_study", x, net, prob, holds[0])
    alph = list(net.alph if alph is None else alph)
    paths = int(paths)
    if paths < 1:
        raise ValueError("paths must be >= 1")
    if sigma is None and (paths != 1 or rho is not None):
        raise ValueError("hold_study: paths > 1 and rho belong to a disturbed study; pass sigma")
    if int(max_rows) < paths:
        raise ValueError(f"max_rows = {int(max_rows)} holds no whole start of {paths} paths")
    if sigma is not None:
        _check_seed(seed)
        if rho is not None and isinstance(x, torch.Tensor) and x.dim() == 2:
            check_rho(rho, x.shape[1], "hold_study")
    x = _lib.require_device_f32(x, "x")
    if x.dim() != 2:
        raise ValueError("x must be nex-by-d")
    n, d = x.shape
    per = int(max_rows) // paths                           # starts per chunk
    tabs = {k: [] for k in [0] + holds}
    with torch.no_grad():
        for s0 in range(0, n, per):
            xs = x[s0:s0 + per].repeat_interleave(paths, dim=0).contiguous()
            Wc = None
            if sigma is not None:
                Wc = counter_disturbances(nt, xs.shape[0], d, sigma, seed, tspan=tspan, mask=mask, row_offset=s0 * paths, device=x.device,
                                          rho=rho)
                tabs[0].append(disturbed_rollout(xs, net, prob, nt, Wc, tspan=tspan, alph=alph, stepper=stepper)["persample"])
            else:
                tabs[0].append(_launch(xs, net, prob, list(tspan), nt, stepper, alph, False)[0])
            for k in holds:
                tabs[k].append(_held(xs, net, prob, tspan, nt, k, Wc, stepper, alph, False, "hold_study")[1])
    _lib.check_errors(sync=True)
    out = {}
    for k, parts in tabs.items():
        tab = torch.cat(parts).view(n, paths, 7)
        cols = _columns(tab, alph[0])
        entry = {name: (path_statistics(v) if sigma is not None else v[:, 0]) for name, v in cols.items()}
        entry["persample"] = tab
        out[k] = entry
    return out
