"""Ensembles under in-kernel Brownian noise: E networks of one shape, every member at its own noise level, in one launch.

ensemble.py rolls out and trains E networks in one launch, undisturbed; noise.py draws the per-step Brownian disturbance of ONE network inside
the rollout kernels, a pure function of (seed, global row, step, component).  Here the two meet: the ensemble launches with the disturbance
drawn in the kernel, member e under its own level sigma_e and its own seed.  The key of a row is its index INSIDE its member (plus row_offset),
so members given one seed meet identical noise realisations -- common random numbers, a paired comparison across the levels, which is what a
sweep over sigma wants -- and member e's results are bit for bit those of noisy_rollout / noisy_ocflow_train on ens.member(e) alone with
(sigma_e, seed_e, mask, row_offset), on the same kernel family.

    Jc, cs = ensemble_noisy_rollout(x, ens, prob, tspan, nt, sigma=[[0.0], [0.1], [0.2]], seed=7)
    Jc, cs = ensemble_noisy_ocflow_train(x, ens, prob, tspan, nt, sigma, seed)       # one recording forward, the ensemble adjoint unchanged
    stats  = ensemble_noise_study(x, ens, prob, nt, sigma, paths, seed)              # noise_study(..., rng="counter") per member

The adjoint is ensemble.py's: the disturbance does not depend on the parameters, so it runs on the recorded displaced states as it is.
Single precision, one device, family "lane" or "mid" as in ensemble.py.  No CPU or eager-torch fallback: everything else is refused before a
device is touched."""
import ctypes as C
import math

import torch
from torch.autograd.function import once_differentiable

from . import _lib, ensemble
from .disturb import path_statistics
from .ensemble import _refuse
from .noise import _check_row_offset, _check_seed

_NAMES = {"lane": ("nocf_rollout_noisy_ensemble_f32", "nocf_rollout_record_noisy_ensemble_f32"),
          "mid": ("nocf_rollout_noisy_mid_ensemble_f32", "nocf_rollout_record_noisy_mid_ensemble_f32")}
SYMBOLS = _NAMES["lane"] + _NAMES["mid"]


def _entries(L, family):
    """(evaluation entry, recording entry, their names) of library L for one family; RuntimeError when L lacks one"""
    return _lib.require(L, _NAMES[family], "ensemble_noise") + (_NAMES[family],)


def scale_table(sigma, members, nt, d, tspan=(0., 1.), mask=None):
    """sigma -> the scale table [E, d] on the host, float32: row e is noise.noise_scale(sigma_e, nt, d, tspan, mask) -- its arithmetic
    (the product with sqrt(h) in double, one rounding to float32, the mask) on all rows at once: the table is formed in every call.
    sigma: a float or [d] (every member that level); a 2-D tensor or nested list [E, 1] or [E, d] (member e its row).  A 1-D sequence of a
    length other than d is a ValueError: [E] against [d] would be ambiguous -- write [E, 1]"""
    E, d = int(members), int(d)
    if int(nt) < 1 or d < 1:
        raise ValueError("nt and d must be >= 1")
    h = (float(tspan[1]) - float(tspan[0])) / int(nt)
    if not h > 0:
        raise ValueError("tspan must have positive length")
    sg = sigma.detach().to("cpu", torch.float64) if isinstance(sigma, torch.Tensor) else torch.as_tensor(sigma, dtype=torch.float64)
    if sg.dim() == 0 or (sg.dim() == 1 and sg.numel() == d):
        sg = sg.expand(d)
    elif sg.dim() == 1:
        raise ValueError(f"sigma: a 1-D sequence must have d = {d} entries (one level per coordinate, shared by the members), got {sg.numel()}; "
                         f"a level per member is [E, 1] = [{E}, 1] or [E, d]")
    elif not (sg.dim() == 2 and sg.shape[0] == E and sg.shape[1] in (1, d)):
        raise ValueError(f"sigma must be a float, [d], [E, 1] or [E, d] with E = {E}, d = {d}; got shape {tuple(sg.shape)}")
    scale = (sg.expand(E, d) * math.sqrt(h)).to(torch.float32)
    if mask is not None:
        mk = torch.as_tensor(mask).detach().to("cpu")
        if mk.numel() != d:
            raise ValueError("mask must have d entries")
        scale = scale * (mk.reshape(-1) != 0).to(torch.float32)
    return scale.contiguous()


def seed_list(seed, members):
    """seed -> E Python ints: one int (every member the same noise) or a sequence of E ints, each checked as noise.py checks a seed"""
    E = int(members)
    if isinstance(seed, (list, tuple)):
        if len(seed) != E:
            raise ValueError(f"seed must be a Python int or a sequence of {E} ints (one per member), got {len(seed)} entries")
        return [_check_seed(s) for s in seed]
    return [_check_seed(seed)] * E


class _Noise:
    """what a noisy ensemble launch takes beside its undisturbed sibling's arguments (ensemble._launch / _launch_mid, noise=): the scale
    table, the seeds and the key of every member's row 0"""

    def __init__(self, scale, seeds, row_offset):
        self.scale, self.seeds, self.row_offset = scale, list(seeds), row_offset
        self._dev = {}

    def entries(self, L, family):
        return _entries(L, family)

    def args(self, dev):
        t = self._dev.get(dev)
        if t is None:
            # both tables in ONE buffer, one host-to-device copy per call like noisy_rollout's: the scale rows, then (8-byte aligned) the seeds
            # as the int64 of the same bits -- torch has no unsigned 64-bit arithmetic, the kernel reads the words as they are
            words = torch.tensor([s - (1 << 64) if s >= (1 << 63) else s for s in self.seeds], dtype=torch.int64)
            nb = self.scale.numel() * 4
            off = (nb + 7) // 8 * 8
            buf = torch.zeros(off + 8 * len(self.seeds), dtype=torch.uint8)
            buf[:nb] = self.scale.view(torch.uint8).reshape(-1)
            buf[off:] = words.view(torch.uint8)
            t = self._dev[dev] = (buf.to(dev), off)
        return (C.c_void_p(t[0].data_ptr()), C.c_void_p(t[0].data_ptr() + t[1]), self.row_offset)


def _prepare(fn, x, ens, prob, tspan, nt, sigma, seed, stepper, train, mask, row_offset, family, rho=None):
    """every refusal of a noisy ensemble call -> (E, n, d, _Noise); nothing here touches a device"""
    if rho is not None:
        raise NotImplementedError(f"{fn}: rho is not supported for ensembles; the time-correlated noise takes one network "
                                  "(noisy_rollout / noisy_ocflow_train with rho=; per-member rho is not built)")
    if isinstance(ens, ensemble.PhiEnsemble) and isinstance(x, torch.Tensor) and x.dim() in (2, 3):
        table = scale_table(sigma, ens.members, nt, x.shape[-1], tspan, mask) if int(nt) >= 1 else None
        seeds = seed_list(seed, ens.members)
    else:
        table = seeds = None
    row_offset = _check_row_offset(row_offset)
    E, n, d, _own = _refuse(fn, x, ens, prob, nt, stepper, train, family=family)
    if family in _NAMES:
        _entries(_lib.lib(), family)                                 # (a library without the symbols: RuntimeError, before any launch)
    return E, n, d, _Noise(table, seeds, row_offset)


def ensemble_noisy_rollout(x, ens, prob, tspan, nt, sigma, seed, stepper="rk4", alph=None, intermediates=False, *, mask=None, row_offset=0,
                           family="lane", rho=None):
    """ensemble_rollout with every member under per-step Brownian noise drawn inside the kernel, in one launch.
    :param sigma: a float or [d] (every member that level), or [E, 1] / [E, d] (a 2-D tensor or nested list: member e its row).  A member at 0
                  is rolled out undisturbed, bit for bit
    :param seed:  a Python int, 0 <= seed < 2**64: all members meet the same noise (row j of every member the disturbances of key
                  row_offset + j); or a sequence of E ints, one per member
    :param mask:  [d]: coordinates with mask == 0 are not disturbed;  row_offset: the key of row 0 of every member, as in noisy_rollout
    :param x, ens, prob, tspan, nt, stepper, alph, intermediates, family: as for ensemble_rollout
    :param rho:   refused (NotImplementedError) unless None: the time-correlated noise of noisy_rollout takes one network
    :return: what ensemble_rollout returns: (Jc [E], cs [E, 7]); with intermediates also the trajectories [E, nex, d+4, nt+1] and the controls
             [E, nex, a, nt+1].  Member e's values are bit for bit noisy_rollout's on ens.member(e) with sigma_e, seed_e, mask and row_offset."""
    E, n, d, nz = _prepare("ensemble_noisy_rollout", x, ens, prob, tspan, nt, sigma, seed, stepper, False, mask, row_offset, family, rho)
    nt = int(nt)
    if family == "mid":
        b = ensemble._launch_mid(x, ens, prob, tspan, nt, stepper, alph, intermediates, noise=nz)
        Jc, cs = b["means"][:, 7], b["means"][:, :7]
        if not intermediates:
            return Jc, cs
        return Jc, cs, b["zFull"].permute(0, 2, 3, 1), b["ctrlFull"].permute(0, 2, 3, 1)
    b = ensemble._launch(x, ens, prob, tspan, nt, stepper, alph, intermediates, noise=nz)
    Jc, cs = b["means"][:, 7], b["means"][:, :7]
    if not intermediates:
        return Jc, cs
    zF, cF = b["zFull"], b["ctrlFull"]
    return Jc, cs, zF.view(nt + 1, E, n, d + 4).permute(1, 2, 3, 0), cF.view(nt + 1, E, n, cF.shape[-1]).permute(1, 2, 3, 0)


class _NoisyEnsembleTrain(torch.autograd.Function):
    """ensemble._EnsembleTrain with the disturbances drawn inside the recording forward (nocf_rollout_record_noisy_ensemble_f32): it saves the
    same stage inputs and displaced z(T), so the backward is the undisturbed ensemble's, unchanged"""

    @staticmethod
    def forward(ctx, x, ens, prob, tspan, nt, stepper, alph, noise, *params):
        return ensemble._EnsembleTrain._forward(ctx, x, ens, prob, tspan, nt, stepper, alph, noise)

    @staticmethod
    @once_differentiable
    def backward(ctx, gJ, _gmeans):
        g = ensemble._EnsembleTrain._adjoint(ctx, gJ)                # (x, six plain arguments, the parameters)
        return g[:7] + (None,) + g[7:]


class _NoisyEnsembleTrainMid(torch.autograd.Function):
    """the same on the one-CU family (nocf_rollout_record_noisy_mid_ensemble_f32, ensemble._EnsembleTrainMid's adjoint)"""

    @staticmethod
    def forward(ctx, x, ens, prob, tspan, nt, stepper, alph, noise, *params):
        return ensemble._EnsembleTrainMid._forward(ctx, x, ens, prob, tspan, nt, stepper, alph, noise)

    @staticmethod
    @once_differentiable
    def backward(ctx, gJ, _gmeans):
        g = ensemble._EnsembleTrainMid._adjoint(ctx, gJ)
        return g[:7] + (None,) + g[7:]


def ensemble_noisy_ocflow_train(x, ens, prob, tspan, nt, sigma, seed, stepper="rk4", alph=None, *, mask=None, row_offset=0, family="lane",
                                rho=None):
    """(Jc [E], cs [E, 7]) under per-member Brownian noise, Jc differentiable in every stacked parameter of `ens` (and in x when every member
    has its own starts): one recording forward that draws the disturbances, then the ensemble adjoint launch of ensemble_ocflow_train
    unchanged.  Member e's Jc, gradients and x.grad[e] are bit for bit those of noisy_ocflow_train + backward() on ens.member(e) with sigma_e,
    seed_e, mask and row_offset.  Arguments as for ensemble_noisy_rollout; shapes and problems as for ensemble_ocflow_train (rho: refused unless None)."""
    _E, _n, _d, nz = _prepare("ensemble_noisy_ocflow_train", x, ens, prob, tspan, nt, sigma, seed, stepper, True, mask, row_offset, family, rho)
    params = [p for _, p in ens._params()]
    fn = _NoisyEnsembleTrainMid if family == "mid" else _NoisyEnsembleTrain
    Jc, means = fn.apply(x, ens, prob, [float(tspan[0]), float(tspan[1])], int(nt), stepper, alph, nz, *params)
    return Jc, means


def ensemble_noise_study(x, ens, prob, nt, sigma, paths, seed, tspan=(0., 1.), alph=None, stepper="rk4", mask=None, max_rows=1 << 16,
                         family="lane", rho=None):
    """noise_study(..., rng="counter") for every member of an ensemble, one launch per chunk: each start is repeated `paths` times as rows
    of a member's batch (start-major: row i * paths + p), in chunks of whole starts.  max_rows bounds the rows of ONE MEMBER per launch, as it
    bounds the rows of noise_study's launch: a launch holds at most E * max_rows rows in all (max_rows < paths is a ValueError).  Every chunk
    is one ensemble_noisy_rollout with row_offset = the chunk's first row, so start i, path p of member e meets the noise of
    (seed_e, i * paths + p) whatever max_rows is.
    :param x: nex-by-d (shared) or E-by-nex-by-d;  sigma, seed, mask, family: as for ensemble_noisy_rollout
    :return: dict with, per quantity "L+G" (L + member e's alph[0] G), "G", "Q", "W": a dict mean / std / q05 / q50 / q95 of [E, nex] tensors;
             and "persample" [E, nex, paths, 7].  Member e's slices equal noise_study(x_e, ens.member(e), ..., sigma_e, rng="counter",
             seed=seed_e) on the same kernel family."""
    if rho is not None:
        _prepare("ensemble_noise_study", x, ens, prob, tspan, nt, sigma, seed, stepper, False, mask, 0, family, rho)
    paths = int(paths)
    if paths < 1:
        raise ValueError("paths must be >= 1")
    if int(max_rows) < paths:
        raise ValueError(f"max_rows = {int(max_rows)} holds no whole start of {paths} paths")
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3):
        raise ValueError("x must be nex-by-d (shared by the members) or E-by-nex-by-d")
    nex = x.shape[-2]
    per = int(max_rows) // paths                                     # starts per chunk
    # every refusal before the first launch, on the whole batch
    E, _n, _d, _nz = _prepare("ensemble_noise_study", x, ens, prob, tspan, nt, sigma, seed, stepper, False, mask, 0, family)
    rows_a = ens.alph if alph is None else ensemble._alph_rows(alph, E)
    tabs = []
    for s0 in range(0, nex, per):
        xs = x[..., s0:s0 + per, :].repeat_interleave(paths, dim=-2).contiguous()
        n = xs.shape[-2]
        nz = _Noise(_nz.scale, _nz.seeds, s0 * paths)
        with torch.no_grad():
            if family == "mid":
                tabs.append(ensemble._launch_mid(xs, ens, prob, tspan, int(nt), stepper, alph, noise=nz)["persample"])
            else:
                tabs.append(ensemble._launch(xs, ens, prob, tspan, int(nt), stepper, alph, noise=nz)["persample"].view(E, n, 7))
    tab = torch.cat(tabs, dim=1).view(E, nex, paths, 7)
    _lib.check_errors(sync=True)
    out = {"persample": tab}
    for key, pick in (("L+G", None), ("G", 1), ("Q", 5), ("W", 6)):
        per_member = [path_statistics(tab[e, :, :, 0] + rows_a[e][0] * tab[e, :, :, 1] if pick is None else tab[e, :, :, pick])
                      for e in range(E)]
        out[key] = {k: torch.stack([st[k] for st in per_member]) for k in per_member[0]}
    return out
