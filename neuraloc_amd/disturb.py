"""Rollouts of the feedback controller under per-step disturbances.

u = -grad_p H(x, grad Phi(x, t)) reacts to wherever the state is.  shock.py displaces the state once; here it is displaced behind EVERY
step, by a caller-supplied W [nt, n, d] (time-major like the kernels' zFull):

    z = [x, 0, 0, 0, 0];  for k in 0 .. nt-1:  z = step(z, tk, tk + h);  z[:, :d] += W[k];  tk += h;   terminal terms at the displaced z(T)

-- additive noise in the Euler-Maruyama position.  The whole disturbed rollout is ONE launch (nocf_rollout_disturbed_f32): the lane, one-CU
and per-tile kernels take W as one more input.  The split-role kernel does not: m = 512 point-agent networks run on the per-tile kernel here.
Single precision, no segments.  These calls are evaluations (no autograd); training through disturbed rollouts is
train.disturbed_ocflow_train (nocf_rollout_record_disturbed_f32).  There is no CPU or eager-torch fallback."""
import math

import torch

from . import _lib
from .OCflow import _evaluate


def _entry(L):
    """nocf_rollout_disturbed_f32 of library L, or None when L does not export it"""
    f = _lib.entries(L, ("nocf_rollout_disturbed_f32",))
    return f and f[0]


def disturbed_rollout(x, Phi, prob, nt, W, tspan=(0., 1.), alph=None, stepper="rk4", intermediates=False):
    """
    :param x:   nex-by-d initial states on the MI355X, float32
    :param W:   nt-by-nex-by-d float32 device tensor: W[k] is added to the state (not to the four cost columns) behind step k;
                W[nt-1] lands on the terminal state.  Not modified.
    :param alph: 6 multipliers (default: Phi.alph)
    :return: dict with
        Jc, cs      the means, as OCflow returns them
        persample   nex-by-7 table [L, G, HJt, HJfin, HJgrad, Q, W]
        z_final     nex-by-(d+4)
        traj, ctrl  with intermediates: nex-by-(d+4)-by-(nt+1) and nex-by-a-by-(nt+1), the reference's layout (ctrl[:, :, k+1] from
                    grad Phi at the displaced state and the step's start time, like src/OCflow.py:53)
    """
    alph = list(Phi.alph if alph is None else alph)
    for name, t in (("x", x), ("W", W)):
        if isinstance(t, torch.Tensor) and t.dtype == torch.float64:
            raise RuntimeError(f"disturbed_rollout: {name} is float64; the disturbed rollout is single precision only "
                               "(the double-precision kernel takes no disturbance)")
    if not isinstance(W, torch.Tensor):                    # (to _evaluate, None is the held call's "no disturbance")
        raise TypeError("W must be a torch.Tensor")
    means, persample, _sums, z_final, zFull, ctrlFull = _evaluate("disturbed_rollout", "nocf_rollout_disturbed_f32", x, Phi, prob, tspan, nt,
                                                                  stepper, alph, intermediates, W=W)
    out = {"Jc": means[7], "cs": [means[i] for i in range(7)], "persample": persample, "z_final": z_final}
    if intermediates:
        out["traj"], out["ctrl"] = zFull.permute(1, 2, 0), ctrlFull.permute(1, 2, 0)
    return out


def brownian_disturbances(nt, n, d, sigma, tspan=(0., 1.), generator=None, device=None, mask=None, rho=None):
    """sigma * sqrt(h) * randn, time-major [nt, n, d], float32: the increments of sigma dB over steps of h = (tspan[1] - tspan[0]) / nt.
    sigma: a float or a [d] tensor; mask [d]: coordinates with mask == 0 are not disturbed (the quadcopter's velocities only, say);
    generator: a torch.Generator of `device` (default: that device's global one).
    rho: a float or [d] in [0, 1): the white draws v_k become an AR(1) / Ornstein-Uhlenbeck path in k, w_0 = v_0 and
    w_k = rho_i w_{k-1} + sqrt(1 - rho_i^2) v_k -- the recursion of noise.counter_disturbances(..., rho=) in plain torch on randn draws (the
    same variance at every step, corr(w_k, w_{k+j}) = rho_i^j; no bit contract).  rho=0.0 gives the white tensor."""
    if int(nt) < 1 or int(n) < 1 or int(d) < 1:
        raise ValueError("nt, n and d must be >= 1")
    if rho is not None:
        from .noise import check_rho
        rho = check_rho(rho, d, "brownian_disturbances")
    h = (float(tspan[1]) - float(tspan[0])) / int(nt)
    if not h > 0:
        raise ValueError("tspan must have positive length")
    if device is None:
        device = generator.device if generator is not None else "cpu"
    W = torch.randn(int(nt), int(n), int(d), generator=generator, device=device, dtype=torch.float32)
    scale = torch.as_tensor(sigma, dtype=torch.float32, device=W.device)
    if scale.dim() > 1 or (scale.dim() == 1 and scale.numel() != int(d)):
        raise ValueError("sigma must be a float or a [d] tensor")
    W = W * (scale * math.sqrt(h))
    if mask is not None:
        mk = torch.as_tensor(mask, device=W.device)
        if mk.numel() != int(d):
            raise ValueError("mask must have d entries")
        W = W * (mk.reshape(-1) != 0).to(torch.float32)
    if rho is not None:
        r = rho.to(W.device, torch.float32)
        q = torch.sqrt(1.0 - rho * rho).to(W.device, torch.float32)
        for k in range(1, int(nt)):
            W[k] = r * W[k - 1] + q * W[k]
    return W.contiguous()


QUANTILES = (0.05, 0.5, 0.95)


def path_statistics(v):
    """v [starts, paths] -> dict mean, std (unbiased; 0 for one path), q05, q50, q95, each [starts]"""
    q = torch.quantile(v, torch.tensor(QUANTILES, dtype=v.dtype, device=v.device), dim=1)
    std = v.std(dim=1) if v.shape[1] > 1 else torch.zeros_like(v[:, 0])
    return {"mean": v.mean(dim=1), "std": std, "q05": q[0], "q50": q[1], "q95": q[2]}


def noise_study(x, Phi, prob, nt, sigma, paths, tspan=(0., 1.), alph=None, stepper="rk4", generator=None, mask=None, max_rows=1 << 16,
                rng="torch", seed=None, rho=None):
    """The distribution of the costs over `paths` Brownian disturbances of every start: each start is repeated `paths` times as rows of one
    batch (start-major: row i * paths + p), in chunks of whole starts of at most max_rows rows (max_rows < paths is a ValueError), one launch
    per chunk.  The disturbances are drawn chunk by chunk from `generator` (brownian_disturbances(nt, rows, d, sigma, tspan=tspan,
    generator=generator, device=x.device, mask=mask)).
    rng="counter" (needs `seed`, a Python int in [0, 2**64); takes no generator): nothing is drawn -- every chunk is one noise.noisy_rollout
    with row_offset = the chunk's first row, so start i, path p meets the noise of global row i * paths + p whatever max_rows is.
    rho (a float or [d] in [0, 1)): the disturbances are correlated in time -- rng="counter": noisy_rollout(..., rho=rho), the path of a
    global row whatever max_rows is; rng="torch": brownian_disturbances(..., rho=rho).  A PhiEnsemble with rho is refused.
    :return: dict with, per quantity "L+G" (L + alph[0] G), "G", "Q", "W": a dict mean / std / q05 / q50 / q95 of [nex] tensors; and
             "persample" [nex, paths, 7], the table every figure is formed from"""
    alph = list(Phi.alph if alph is None else alph)
    if rng not in ("torch", "counter"):
        raise ValueError(f"rng must be 'torch' or 'counter', got {rng!r}")
    if rng == "counter":
        from .noise import _check_seed, noisy_rollout
        if generator is not None:
            raise ValueError("noise_study: rng='counter' draws nothing and takes no generator; pass seed")
        if seed is None:
            raise ValueError("noise_study: rng='counter' needs seed")
        _check_seed(seed)
    elif seed is not None:
        raise ValueError("noise_study: seed belongs to rng='counter'; rng='torch' is seeded through generator")
    if rho is not None:
        from .noise import _refuse_ensemble, check_rho
        _refuse_ensemble(Phi, "noise_study")
        if isinstance(x, torch.Tensor) and x.dim() == 2:
            check_rho(rho, x.shape[1], "noise_study")
    paths = int(paths)
    if paths < 1:
        raise ValueError("paths must be >= 1")
    if int(max_rows) < paths:
        raise ValueError(f"max_rows = {int(max_rows)} holds no whole start of {paths} paths")
    x = _lib.require_device_f32(x, "x")
    if x.dim() != 2:
        raise ValueError("x must be nex-by-d")
    n, d = x.shape
    per = int(max_rows) // paths                           # starts per chunk
    tabs = []
    for s0 in range(0, n, per):
        xs = x[s0:s0 + per].repeat_interleave(paths, dim=0).contiguous()
        if rng == "counter":
            kw = {} if rho is None else {"rho": rho}
            tabs.append(noisy_rollout(xs, Phi, prob, nt, sigma, seed, tspan=tspan, alph=alph, stepper=stepper, mask=mask,
                                      row_offset=s0 * paths, **kw)["persample"])
            continue
        kw = {} if rho is None else {"rho": rho}
        Wc = brownian_disturbances(nt, xs.shape[0], d, sigma, tspan=tspan, generator=generator, device=x.device, mask=mask, **kw)
        tabs.append(disturbed_rollout(xs, Phi, prob, nt, Wc, tspan=tspan, alph=alph, stepper=stepper)["persample"])
    tab = torch.cat(tabs).view(n, paths, 7)
    _lib.check_errors(sync=True)
    out = {"L+G": path_statistics(tab[:, :, 0] + alph[0] * tab[:, :, 1]), "G": path_statistics(tab[:, :, 1]),
           "Q": path_statistics(tab[:, :, 5]), "W": path_statistics(tab[:, :, 6]), "persample": tab}
    return out
