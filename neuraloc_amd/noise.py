"""Brownian disturbances from a counter-based generator, drawn inside the rollout kernels.

disturb.brownian_disturbances draws a tensor W [nt, n, d] with torch.randn; here the disturbance of (row, step k, component i) is a pure
function of (seed, GLOBAL row, k, i) -- Philox4x32-10 and a Box-Muller transform, csrc/nocf_noise.inc -- evaluated by the lane, one-CU and
per-tile kernels where they otherwise load W[k][row][i].  No tensor exists; a row meets the same noise alone, in any batch, on any rank and
in any chunk (row_offset = the global index of the call's first row), and a prefix in nt stays a prefix as long as sigma sqrt(h) is the same.

    counter_disturbances   the same values as a tensor (nocf_noise_fill_f32): what disturbance_gradient and the worst-case search start from
    noisy_rollout          disturbed_rollout on that tensor, bit for bit, without it (nocf_rollout_noisy_f32)
    noisy_ocflow_train     disturbed_ocflow_train likewise (nocf_rollout_record_noisy_f32); the adjoint is the same code

rho= on all three: the disturbance of a (row, component) becomes an AR(1) / Ornstein-Uhlenbeck path in k,
    w_0 = v_0(s0),  w_k = fl32(fl32(rho_i w_{k-1}) + v_k(s1)),   s0 = sigma_i sqrt(h),  s1 = s0 sqrt(1 - rho_i^2),
with v_k(s) the white entry of scale s -- every w_k keeps the white variance and corr(w_k, w_{k+j}) = rho_i^j.  The carried value stays in
the kernels (nocf_noise_fill_corr_f32, nocf_rollout_noisy_corr_f32, nocf_rollout_record_noisy_corr_f32); rho=None is the white path and
its entry points, untouched, and rho=0.0 gives the white values through the new ones.

Single precision only; no CPU or eager-torch fallback; every check raises before a device is touched."""
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .OCflow import _check_args, _evaluate
from .train import _OCflowTrain, _record_forward, _structs


def _entry(L, name):
    """entry `name` of library L, or None when L does not export it"""
    f = _lib.entries(L, (name,))
    return f and f[0]


def _entry_for(L, name, what):
    """(library, entry): L's, or the shipped library's when L is a per-shape library cached by an older build"""
    L, (f,) = _lib.entry_for(L, (name,), what)
    return L, f


def _check_seed(seed):
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be a Python int with 0 <= seed < 2**64, got {seed!r}")
    return seed


def _check_row_offset(row_offset):
    if isinstance(row_offset, bool) or not isinstance(row_offset, int) or not 0 <= row_offset < 2 ** 62:
        raise ValueError(f"row_offset must be a Python int >= 0, got {row_offset!r}")
    return row_offset


def noise_scale(sigma, nt, d, tspan=(0., 1.), mask=None):
    """scale [d] on the host, float32: fp32(sigma_i sqrt(h)) formed in double with h = (tspan[1] - tspan[0]) / nt; 0 where mask == 0"""
    if int(nt) < 1 or int(d) < 1:
        raise ValueError("nt and d must be >= 1")
    h = (float(tspan[1]) - float(tspan[0])) / int(nt)
    if not h > 0:
        raise ValueError("tspan must have positive length")
    sg = (sigma.detach().to("cpu", torch.float64) if isinstance(sigma, torch.Tensor) else torch.as_tensor(sigma, dtype=torch.float64))
    if sg.dim() > 1 or (sg.dim() == 1 and sg.numel() != int(d)):
        raise ValueError("sigma must be a float or a [d] tensor")
    scale = (sg.expand(int(d)) * math.sqrt(h)).to(torch.float32)
    if mask is not None:
        mk = torch.as_tensor(mask).detach().to("cpu")
        if mk.numel() != int(d):
            raise ValueError("mask must have d entries")
        scale = scale * (mk.reshape(-1) != 0).to(torch.float32)
    return scale.contiguous()


def check_rho(rho, d, what="rho"):
    """rho, a float or [d], as a float64 [d] tensor on the host; every refusal of a rho (outside [0, 1), non-finite, wrong shape, float64)"""
    if isinstance(rho, bool):
        raise ValueError(f"{what}: rho must be a float or a [d] tensor with 0 <= rho < 1, got {rho!r}")
    if isinstance(rho, torch.Tensor):
        if rho.dtype == torch.float64:
            raise RuntimeError(f"{what}: rho is float64; the correlated noise is single precision only: pass a float or a float32 [d] tensor")
        r = rho.detach().to("cpu", torch.float64)
    else:
        try:
            r = torch.as_tensor(rho, dtype=torch.float64)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"{what}: rho must be a float or a [d] tensor with 0 <= rho < 1, got {rho!r}") from None
    if r.dim() > 1 or (r.dim() == 1 and r.numel() != int(d)):
        raise ValueError(f"{what}: rho must be a float or a [d] tensor with d = {int(d)}, got shape {tuple(r.shape)}")
    r = r.expand(int(d)).contiguous()
    # (the kernels multiply by fp32(rho): a rho that rounds to 1 there is no longer inside the interval)
    if not bool(torch.isfinite(r).all()) or bool((r < 0).any()) or bool((r.to(torch.float32) >= 1).any()):
        raise ValueError(f"{what}: rho must be finite with 0 <= rho < 1 (in float32), got {rho!r}")
    return r


def noise_corr_scales(sigma, rho, nt, d, tspan=(0., 1.), mask=None):
    """(s0, s1, rho) [d] on the host, float32, of the correlated noise: s0 = noise_scale(sigma, ...) = fp32(sigma_i sqrt(h)),
    s1 = fp32(sigma_i sqrt(h) sqrt(1 - rho_i^2)) -- both formed in double, both 0 where mask == 0 -- and fp32(rho_i).  rho = 0: s1 == s0"""
    s0 = noise_scale(sigma, nt, d, tspan, mask)
    r = check_rho(rho, d, "noise_corr_scales")
    h = (float(tspan[1]) - float(tspan[0])) / int(nt)
    sg = (sigma.detach().to("cpu", torch.float64) if isinstance(sigma, torch.Tensor) else torch.as_tensor(sigma, dtype=torch.float64))
    s1 = (sg.expand(int(d)) * math.sqrt(h) * torch.sqrt(1.0 - r * r)).to(torch.float32)
    if mask is not None:
        s1 = s1 * (torch.as_tensor(mask).detach().to("cpu").reshape(-1) != 0).to(torch.float32)
    return s0, s1.contiguous(), r.to(torch.float32).contiguous()


def _refuse_ensemble(net, what):
    from .ensemble import PhiEnsemble
    if isinstance(net, PhiEnsemble):
        raise NotImplementedError(f"{what}: rho with a PhiEnsemble is not supported; the correlated noise takes one network "
                                  "(per-member rho is not built)")


def _require_device(device, what):
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError(f"{what}: device is {device}: the generator runs only on an MI355X (ROCm 'cuda' device); there is no CPU fallback")
    return torch.device(device)


def counter_disturbances(nt, n, d, sigma, seed, tspan=(0., 1.), mask=None, row_offset=0, device=None, rho=None):
    """The counterpart of brownian_disturbances: W [nt, n, d], float32, W[k, row, i] = the disturbance of (seed, row_offset + row, k, i) with
    scale sigma_i sqrt(h) -- the values noisy_rollout adds, as a tensor (nocf_noise_fill_f32).
    sigma: a float or [d]; mask [d]: coordinates with mask == 0 are not disturbed; seed: a Python int, 0 <= seed < 2**64;
    row_offset: global index of row 0; device: an MI355X.
    rho: a float or [d] in [0, 1): W[:, row, i] is the correlated path of the module's docstring (nocf_noise_fill_corr_f32)."""
    if int(nt) < 1 or int(n) < 1 or int(d) < 1:
        raise ValueError("nt, n and d must be >= 1")
    scale = noise_scale(sigma, nt, d, tspan, mask)
    tabs = None if rho is None else noise_corr_scales(sigma, rho, nt, d, tspan, mask)
    seed, row_offset = _check_seed(seed), _check_row_offset(row_offset)
    dev = _require_device(device, "counter_disturbances")
    W = torch.empty(int(nt), int(n), int(d), dtype=torch.float32, device=dev)
    if tabs is not None:
        s0, s1, rh = (t.to(dev) for t in tabs)
        with torch.cuda.device(dev):
            _, f = _entry_for(_lib.lib(), "nocf_noise_fill_corr_f32", "counter_disturbances")
            rc = f(_lib.ptr(W), int(n), int(nt), int(d), _lib.ptr(s0), _lib.ptr(s1), _lib.ptr(rh), seed, row_offset, _lib.stream_ptr(dev))
        _lib.check(rc, "nocf_noise_fill_corr_f32")
        return W
    scale = scale.to(dev)
    with torch.cuda.device(dev):
        _, f = _entry_for(_lib.lib(), "nocf_noise_fill_f32", "counter_disturbances")
        rc = f(_lib.ptr(W), int(n), int(nt), int(d), _lib.ptr(scale), seed, row_offset, _lib.stream_ptr(dev))
    _lib.check(rc, "nocf_noise_fill_f32")
    return W


def _check_call(what, x, net, nt, stepper, alph):
    if isinstance(x, torch.Tensor) and x.dtype == torch.float64:
        raise RuntimeError(f"{what}: x is float64; the noisy rollout is single precision only (the double-precision kernel takes no disturbance)")
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    return _check_args(x, net, nt, stepper, alph, rows=True)


def noisy_rollout(x, Phi, prob, nt, sigma, seed, tspan=(0., 1.), alph=None, stepper="rk4", intermediates=False, mask=None, row_offset=0,
                  rho=None):
    """disturbed_rollout(x, Phi, prob, nt, counter_disturbances(nt, nex, d, sigma, seed, tspan, mask, row_offset), ...) without the tensor: the
    kernels draw each disturbance where they would load it, and every output equals that call's bit for bit.
    :param sigma: a float or [d];  seed: a Python int, 0 <= seed < 2**64;  mask [d]: coordinates with mask == 0 are not disturbed
    :param row_offset: global index of x's first row: row j of this call meets the noise of global row row_offset + j
    :param rho: a float or [d] in [0, 1): the correlated path (module docstring), counter_disturbances(..., rho=rho) without the tensor
                (nocf_rollout_noisy_corr_f32); None: white noise
    :return: the dict of disturbed_rollout"""
    if rho is not None:
        _refuse_ensemble(Phi, "noisy_rollout")
    alph = list(Phi.alph if alph is None else alph)
    n, d = _check_call("noisy_rollout", x, Phi, nt, stepper, alph)
    scale = noise_scale(sigma, nt, d, tspan, mask)
    corr = None if rho is None else noise_corr_scales(sigma, rho, nt, d, tspan, mask)[1:]
    seed, row_offset = _check_seed(seed), _check_row_offset(row_offset)
    name = "nocf_rollout_noisy_f32" if corr is None else "nocf_rollout_noisy_corr_f32"
    means, persample, _sums, z_final, zFull, ctrlFull = _evaluate("noisy_rollout", name, x, Phi, prob, tspan, nt, stepper, alph, intermediates,
                                                                  extra=(scale,) + tuple(corr or ()) + (seed, row_offset))
    out = {"Jc": means[7], "cs": [means[i] for i in range(7)], "persample": persample, "z_final": z_final}
    if intermediates:
        out["traj"], out["ctrl"] = zFull.permute(1, 2, 0), ctrlFull.permute(1, 2, 0)
    return out


class _OCflowTrainNoisy(torch.autograd.Function):
    """_OCflowTrainDisturbed with the disturbances drawn inside the recording forward (nocf_rollout_record_noisy_f32): it saves the same
    stage inputs and displaced z(T), so the backward is _OCflowTrain's, unchanged."""

    @staticmethod
    def forward(ctx, x, net, prob, tspan, nt, stepper, alph, n_total, group, noise, *params):
        ctx.n_plain_args = 9
        ctx.x_needs_grad = bool(x.requires_grad)
        x = _lib.require_device_f32(x.detach(), "x")
        scale, seed, row_offset = noise[:3]                # (with rho: two more entries, the tables s1 and rho; scale is then s0)
        tables = [t.to(x.device) for t in (scale,) + tuple(noise[3:])]
        name = "nocf_rollout_record_noisy_corr_f32" if noise[3:] else "nocf_rollout_record_noisy_f32"
        # (the activation record is the one-CU kernel's here, as in _OCflowTrainDisturbed: m = 512 records on the per-tile kernel)
        return _record_forward(ctx, _structs(x, net, prob), name, "noisy_ocflow_train", x, tuple(_lib.ptr(t) for t in tables) + (seed, row_offset),
                               net, prob, tspan, nt, stepper, alph, n_total, group, one_cu_only=True)

    @staticmethod
    @once_differentiable
    def backward(ctx, gJ, _gmeans):
        return _OCflowTrain._adjoint(ctx, gJ)


def noisy_ocflow_train(x, net, prob, tspan, nt, sigma, seed, stepper="rk4", alph=None, mask=None, row_offset=0, n_total=None, group=None,
                       rho=None):
    """disturbed_ocflow_train under counter_disturbances(nt, nex, d, sigma, seed, tspan, mask, row_offset), without the tensor: (Jc, cs) with Jc
    differentiable w.r.t. every parameter of `net` and w.r.t. x when x requires a gradient.
    :param row_offset: global index of x's first row -- a rank passes the first row of its shard, and the noise a sample meets then does not
                       depend on how the batch is cut;  n_total, group: as for ocflow_train
    :param rho: a float or [d] in [0, 1): training under the correlated path (module docstring; nocf_rollout_record_noisy_corr_f32).  The
                path does not depend on the parameters, so the adjoint is the white one's, on the recorded displaced states
    Single precision only.  Every check below raises before a device is touched."""
    if rho is not None:
        _refuse_ensemble(net, "noisy_ocflow_train")
    alph = list(net.alph if alph is None else alph)
    for name, t in [("x", x)] + [(name, p_) for name, p_ in net.named_parameters()]:
        if isinstance(t, torch.Tensor) and t.dtype == torch.float64:
            raise RuntimeError(f"noisy_ocflow_train: {name} is float64; the noisy rollout is single precision only "
                               "(the double-precision kernels take no disturbance)")
    n, d = _check_call("noisy_ocflow_train", x, net, nt, stepper, alph)
    pd_ = getattr(prob, "d", None)
    if pd_ is not None and int(pd_) != d:
        raise ValueError(f"the problem object has d={pd_} but x has d={d}")
    scale = noise_scale(sigma, nt, d, tspan, mask)
    corr = () if rho is None else noise_corr_scales(sigma, rho, nt, d, tspan, mask)[1:]
    seed, row_offset = _check_seed(seed), _check_row_offset(row_offset)
    _lib.require_device_f32(x, "x")
    params = [p for _, p in net.named_parameters()]
    Jc, means = _OCflowTrainNoisy.apply(x, net, prob, list(tspan), int(nt), stepper, alph, n_total, group,
                                        (scale, seed, row_offset) + tuple(corr), *params)
    return Jc, [means[i] for i in range(7)]
