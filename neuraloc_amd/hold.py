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
import ctypes as C
import numbers

import torch

from . import _lib
from .OCflow import _STEPPERS, _launch
from .disturb import disturbed_rollout, path_statistics

_ARGTYPES = [C.POINTER(_lib.NocfPhi), C.POINTER(_lib.NocfProb), C.c_void_p, C.c_void_p, C.c_int32, C.c_int64,
             C.c_double, C.c_double, C.c_int32, C.c_int32, _lib.fp,
             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
             C.c_void_p, C.c_size_t, C.c_void_p]
_FAMILIES = ("the held rollout runs on the lane kernel (nTh = 2, m <= 32, d + 1 <= 32, point agents, at most 16 of them) and on the one-CU "
             "kernel (nTh = 2, m <= 128, d + 1 <= 32) only")


def _entry(L):
    """nocf_rollout_held_f32 of library L with its prototype set; a library without it is an error, never a fallback"""
    if not hasattr(L, "nocf_rollout_held_f32"):
        raise RuntimeError("held_rollout: the HIP library does not export nocf_rollout_held_f32; rebuild it")
    f = L.nocf_rollout_held_f32
    if f.argtypes is None:
        f.restype = C.c_int
        f.argtypes = _ARGTYPES
    return f


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
    x = _lib.require_device_f32(x, "x")
    if W is not None:
        W = _lib.require_device_f32(W, "W")
    if x.dim() != 2:
        raise ValueError("x must be nex-by-d")
    n, d = x.shape
    if d != net.d:
        raise ValueError(f"x has d={d} but Phi was built for d={net.d}")
    if int(nt) < 1:
        raise ValueError("nt must be >= 1")
    if n < 1:
        raise ValueError("x has no rows")
    if W is not None and tuple(W.shape) != (int(nt), n, d):
        raise ValueError(f"W must be nt-by-nex-by-d = {(int(nt), n, d)}, got {tuple(W.shape)}")
    if W is not None and W.device != x.device:
        raise ValueError("x and W must be on the same device")
    if stepper not in _STEPPERS:
        raise ValueError(f"stepper must be 'rk4' or 'rk1', got {stepper!r}")
    if len(alph) < 6:
        raise ValueError("alph needs 6 entries")
    with torch.no_grad():
        _lib.check_errors()
        phi_st, keep1, ws = net._c_struct(n)
        prob_st, keep2 = prob._c_struct(x.device)
        dev = x.device
        persample = torch.empty(n, 7, dtype=torch.float32, device=dev)
        sums = torch.empty(8, dtype=torch.float32, device=dev)
        means = torch.empty(8, dtype=torch.float32, device=dev)
        z_final = torch.empty(n, d + 4, dtype=torch.float32, device=dev)
        zFull = ctrlFull = None
        if intermediates:
            cdim = _lib.lib().nocf_ctrl_dim(C.byref(prob_st), d)
            zFull = torch.empty(nt + 1, n, d + 4, dtype=torch.float32, device=dev)
            ctrlFull = torch.empty(nt + 1, n, cdim, dtype=torch.float32, device=dev)
        alph_c = (C.c_float * 6)(*[float(a) for a in alph[:6]])
        with torch.cuda.device(dev):
            # (the shipped library: a per-shape build specialises the per-tile kernels, which take no held control)
            L = _lib.lib()
            f = _entry(L)
            rc = f(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), _lib.ptr(W), hold, n,
                   float(tspan[0]), float(tspan[1]), int(nt), _STEPPERS[stepper], alph_c,
                   _lib.ptr(z_final), _lib.ptr(persample), _lib.ptr(sums), _lib.ptr(means), _lib.ptr(zFull), _lib.ptr(ctrlFull),
                   _lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_ptr(dev))
        if rc == -2:                                       # NOCF_E_SHAPE: refused before anything was enqueued
            raise NotImplementedError(f"{what}: nTh = {net.nTh}, m = {net.m}, d = {net.d}, r = {phi_st.r}: no lane and no one-CU "
                                      f"instantiation takes this shape; {_FAMILIES}")
        _lib.check(rc, "nocf_rollout_held_f32")
        _lib.track_rollout_status(L, dev, what)
        if intermediates:
            _lib.check_errors(sync=True)                   # consumed on the host (plots, files): a failed launch raises here
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
