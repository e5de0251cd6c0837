"""Adversarial ensembles: E networks of one shape, every member against its own per-step state disturbance, in one launch.

ensemble.py rolls out and trains E networks in one launch; disturb.py / adversary.py / minmax.py roll ONE network out under a tensor
disturbance W [nt, n, d], differentiate the rollout with respect to W and search for the worst W of a given energy.  Here the two meet: the
ensemble launches run under W [E, nt, n, d] -- member e's slice is exactly the tensor its single-network call takes --, the ensemble adjoints
write every member's dJ/dW [E, nt, n, d] beside (joint) or instead of (state-only) the parameter gradients, and one ascent launch steps all
members, each with its own radius eps_e and step length.  An adversary budget is then a sweep parameter like a noise level: min-max training
or a worst-case search at E budgets costs the launches of one.  Member e's results are bit for bit those of disturbed_rollout /
minmax_ocflow_train / disturbance_gradient / ascend_disturbances / worst_case_disturbances on ens.member(e) alone with W[e], on the same kernel
family.

    out    = ensemble_disturbed_rollout(x, ens, prob, tspan, nt, W)                   # what ensemble_rollout returns
    Jc, cs = ensemble_minmax_ocflow_train(x, ens, prob, tspan, nt, W)                 # Jc.sum().backward(): parameter gradients AND W.grad
    g      = ensemble_disturbance_gradient(x, ens, prob, nt, W, objective="control")  # dW [E, nt, n, d] from the state-only adjoint
    W      = ensemble_ascend_disturbances(W, g["dW"], eps=[0.0, 0.1, 0.2], step_size=[0.0, 0.05, 0.1])
    res    = ensemble_worst_case_disturbances(x, ens, prob, nt, eps=[0.0, 0.1, 0.2])  # three launches per iteration for all members
    Jc, cs = ensemble_adversarial_step(x, ens, prob, tspan, nt, W, eps, step_size)    # one "free" adversarial iteration

Single precision, one device, family "lane" or "mid" as in ensemble.py.  A weighted (risk-sensitive) adversarial ensemble is not built.  No
CPU or eager-torch fallback: everything else is refused before a device is touched."""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _lib, ensemble
from .adversary import OBJECTIVES
from .ensemble import _refuse
from .train import _STEPPERS, _step_sizes

_FORWARD = {"lane": ("nocf_rollout_disturbed_ensemble_f32", "nocf_rollout_record_disturbed_ensemble_f32"),
            "mid": ("nocf_rollout_disturbed_mid_ensemble_f32", "nocf_rollout_record_disturbed_mid_ensemble_f32")}
# the joint (gpart, lam0, lamW) and the state-only (lam0, lamW) ensemble adjoints of a family
_ADJOINT = {"lane": ("nocf_rollout_bwd_small_ensemble_w_f32", "nocf_rollout_bwd_small_ensemble_states_f32"),
            "mid": ("nocf_rollout_bwd_mid_ensemble_w_f32", "nocf_rollout_bwd_mid_ensemble_states_f32")}
# (in the header's order: the four forwards, the two joint adjoints, the two state-only ones, the ascent step)
SYMBOLS = _FORWARD["lane"] + _FORWARD["mid"] + tuple(_ADJOINT[fam][which] for which in (0, 1) for fam in ("lane", "mid")) + \
          ("nocf_disturbance_ascent_ensemble_f32",)


def _entries(L):
    """name -> entry of library L for all nine symbols; RuntimeError naming the missing ones (a library is rebuilt as a whole)"""
    return dict(zip(SYMBOLS, _lib.require(L, SYMBOLS, "ensemble_minmax")))


class _Disturbance:
    """what a disturbed ensemble launch takes beside its undisturbed sibling's arguments (ensemble._launch / _launch_mid, dist=): the tensor W
    [E, nt, n, d], or one [nt, n, d] for all members (stride 0).  It speaks ensemble_noise._Noise's protocol"""

    def __init__(self, W, shared):
        self.W, self.shared = W, shared

    def entries(self, L, family):
        f = _entries(L)
        names = tuple(_FORWARD[family])
        return f[names[0]], f[names[1]], names

    def args(self, dev):
        W = self.W
        return (_lib.ptr(W), 0 if self.shared else W.shape[-3] * W.shape[-2] * W.shape[-1])


def _check_W(fn, W, x, ens, nt, name="W", shared_ok=True):
    """the checks of a disturbance tensor, none of which touches a device: type, precision, shape against (E, nt, n, d), contiguity, x's
    device.  -> shared (a [nt, n, d] for all members)"""
    if not isinstance(W, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if W.dtype == torch.float64:
        raise RuntimeError(f"{fn}: {name} is float64; the disturbed ensemble is single precision only (the double-precision kernels take no "
                           "disturbance and one network)")
    if not (isinstance(ens, ensemble.PhiEnsemble) and isinstance(x, torch.Tensor) and x.dim() in (2, 3)):
        return False                                                 # (_refuse names what is wrong with x / ens)
    E, n, d = ens.members, x.shape[-2], x.shape[-1]
    full, one = (E, int(nt), n, d), (int(nt), n, d)
    if tuple(W.shape) == full or (shared_ok and tuple(W.shape) == one):
        if W.dtype != torch.float32:
            raise RuntimeError(f"{fn}: {name} has dtype {W.dtype}: the HIP path computes in fp32 only")
        if not W.is_contiguous():
            raise ValueError(f"{fn}: {name} must be contiguous ([E, nt, nex, d] member-major: the kernels index it in place)")
        if W.device != x.device:
            raise ValueError(f"{fn}: x and {name} must be on the same device")
        return tuple(W.shape) != full
    raise ValueError(f"{name} must be E-by-nt-by-nex-by-d = {full} (member-major: every member its own disturbance)" +
                     (f" or nt-by-nex-by-d = {one} (one disturbance shared by the members)" if shared_ok else "") + f", got {tuple(W.shape)}")


def _prepare(fn, x, ens, prob, nt, W, stepper, train, family):
    """every refusal of a disturbed ensemble call -> (E, n, d, own, _Disturbance); nothing here touches a device"""
    shared = _check_W(fn, W, x, ens, nt) if int(nt) >= 1 else False
    E, n, d, own = _refuse(fn, x, ens, prob, nt, stepper, train, family=family)
    _entries(_lib.lib())                                             # (a library without the symbols: RuntimeError, before any launch)
    return E, n, d, own, _Disturbance(W.detach(), shared)


def ensemble_disturbed_rollout(x, ens, prob, tspan, nt, W, stepper="rk4", alph=None, intermediates=False, *, family="lane"):
    """ensemble_rollout with every member under its own per-step state disturbance, z_{k+1} = step(z_k) + W[e][k], in one launch.
    :param W: E-by-nt-by-nex-by-d float32, contiguous, on x's device (member e's slice is the W of disturbed_rollout on that member), or
              nt-by-nex-by-d: one disturbance that every member meets.  Not modified
    :param x, ens, prob, tspan, nt, stepper, alph, intermediates, family: as for ensemble_rollout
    :return: what ensemble_rollout returns: (Jc [E], cs [E, 7]); with intermediates also the trajectories [E, nex, d+4, nt+1] and the controls
             [E, nex, a, nt+1].  Member e's values are bit for bit disturbed_rollout's on ens.member(e) with W[e].  An evaluation: nothing
             here is differentiable."""
    E, n, d, _own, ds = _prepare("ensemble_disturbed_rollout", x, ens, prob, nt, W, stepper, False, family)
    nt = int(nt)
    with torch.no_grad():
        if family == "mid":
            b = ensemble._launch_mid(x, ens, prob, tspan, nt, stepper, alph, intermediates, dist=ds)
            Jc, cs = b["means"][:, 7], b["means"][:, :7]
            if not intermediates:
                return Jc, cs
            return Jc, cs, b["zFull"].permute(0, 2, 3, 1), b["ctrlFull"].permute(0, 2, 3, 1)
        b = ensemble._launch(x, ens, prob, tspan, nt, stepper, alph, intermediates, dist=ds)
        Jc, cs = b["means"][:, 7], b["means"][:, :7]
        if not intermediates:
            return Jc, cs
        zF, cF = b["zFull"], b["ctrlFull"]
        return Jc, cs, zF.view(nt + 1, E, n, d + 4).permute(1, 2, 3, 0), cF.view(nt + 1, E, n, cF.shape[-1]).permute(1, 2, 3, 0)


def _base(family):
    return ensemble._EnsembleTrainMid if family == "mid" else ensemble._EnsembleTrain


class _DisturbedEnsembleTrain(torch.autograd.Function):
    """ensemble._EnsembleTrain / _EnsembleTrainMid with the recording forward under a tensor disturbance
    (nocf_rollout_record_disturbed_ensemble_f32 / _mid_): it saves the same stage inputs and displaced z(T), so the backward is the undisturbed
    ensemble's, unchanged.  W is a plain argument here: it takes no gradient"""

    @staticmethod
    def forward(ctx, x, ens, prob, tspan, nt, stepper, alph, family, ds, *params):
        ctx.family = family
        return _base(family)._forward(ctx, x, ens, prob, tspan, nt, stepper, alph, dist=ds)

    @staticmethod
    @once_differentiable
    def backward(ctx, gJ, _gmeans):
        g = _base(ctx.family)._adjoint(ctx, gJ)                      # (x, six plain arguments, the parameters)
        return g[:7] + (None, None) + g[7:]


class _MinmaxEnsembleTrain(torch.autograd.Function):
    """the same forward with W differentiated too: as backward ONE launch of the joint ensemble adjoint of the family
    (nocf_rollout_bwd_small_ensemble_w_f32 / nocf_rollout_bwd_mid_ensemble_w_f32), which writes dJ/dW [E, nt, n, d] beside the partials"""

    @staticmethod
    def forward(ctx, x, ens, prob, tspan, nt, stepper, alph, family, ds, W, *params):
        ctx.family = family
        ctx.w_shape = tuple(W.shape)
        return _base(family)._forward(ctx, x, ens, prob, tspan, nt, stepper, alph, dist=ds)

    @staticmethod
    @once_differentiable
    def backward(ctx, gJ, _gmeans):
        name = list(_ADJOINT[ctx.family])[0]
        f = _entries(_lib.lib())[name]
        E = ctx.w_shape[0]
        lamW = torch.empty(ctx.w_shape, device=gJ.device, dtype=torch.float32)
        g = _base(ctx.family)._adjoint(ctx, gJ, joint=(f, name, lamW))
        return g[:7] + (None, None, gJ.reshape(E, 1, 1, 1) * lamW) + g[7:]


def ensemble_disturbed_ocflow_train(x, ens, prob, tspan, nt, W, stepper="rk4", alph=None, *, family="lane"):
    """(Jc [E], cs [E, 7]) of the disturbed ensemble rollout, Jc differentiable in every stacked parameter of `ens` (and in x when every member
    has its own starts): one recording forward under W, then the ensemble adjoint launch of ensemble_ocflow_train unchanged (the disturbance
    does not depend on the parameters).  Member e's Jc, gradients and x.grad[e] are bit for bit those of disturbed_ocflow_train + backward()
    on ens.member(e) with W[e].  W takes no gradient here (ensemble_minmax_ocflow_train).  Arguments as for ensemble_disturbed_rollout;
    shapes and problems as for ensemble_ocflow_train."""
    _E, _n, _d, _own, ds = _prepare("ensemble_disturbed_ocflow_train", x, ens, prob, nt, W, stepper, True, family)
    params = [p for _, p in ens._params()]
    Jc, means = _DisturbedEnsembleTrain.apply(x, ens, prob, [float(tspan[0]), float(tspan[1])], int(nt), stepper, alph, family, ds, *params)
    return Jc, means


def ensemble_minmax_ocflow_train(x, ens, prob, tspan, nt, W, stepper="rk4", alph=None, *, family="lane"):
    """ensemble_disturbed_ocflow_train with Jc differentiable in W as well: after Jc.sum().backward() (or any upstream gJ [E]) the stacked
    parameter gradients, x.grad (own starts) and W.grad [E, nt, nex, d] = gJ[e] dJc_e/dW[e], all from ONE joint ensemble adjoint launch.
    Member e's values are bit for bit those of minmax_ocflow_train + backward() on ens.member(e) with W[e].
    :param W: E-by-nt-by-nex-by-d.  When it does not require a gradient the call is ensemble_disturbed_ocflow_train.  A shared nt-by-nex-by-d
              W that requires a gradient is refused: the members' dJ/dW are not summed (the rule for a shared x)"""
    fn = "ensemble_minmax_ocflow_train"
    if isinstance(W, torch.Tensor) and not W.requires_grad:
        return ensemble_disturbed_ocflow_train(x, ens, prob, tspan, nt, W, stepper, alph, family=family)
    if isinstance(W, torch.Tensor) and W.dtype != torch.float64 and int(nt) >= 1 and _check_W(fn, W, x, ens, nt):
        raise NotImplementedError(f"{fn}: W.requires_grad needs every member's own disturbance (W of shape [E, nt, nex, d]): the members' "
                                  "dJ/dW of a shared W are not summed")
    _E, _n, _d, _own, ds = _prepare(fn, x, ens, prob, nt, W, stepper, True, family)
    params = [p for _, p in ens._params()]
    Jc, means = _MinmaxEnsembleTrain.apply(x, ens, prob, [float(tspan[0]), float(tspan[1])], int(nt), stepper, alph, family, ds, W, *params)
    return Jc, means


def _per_member(fn, what, v, E):
    """eps / step_size: a float (every member that value) or E of them -> E Python floats, each finite and >= 0"""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().tolist()
    vals = [v] * E if not isinstance(v, (list, tuple)) else list(v)
    if len(vals) != E:
        raise ValueError(f"{fn}: {what} must be a number or {E} of them (one per member), got {len(vals)}")
    try:
        vals = [float(q) for q in vals]
    except (TypeError, ValueError):
        raise ValueError(f"{fn}: {what} must be a number or {E} of them (one per member)") from None
    if not all(q >= 0.0 and q != float("inf") for q in vals):
        raise ValueError(f"{fn}: every {what} must be a finite number >= 0")
    return vals


def _mask_of(mask, d):
    if mask is None:
        return None
    mask = torch.as_tensor(mask)
    if mask.numel() != d:
        raise ValueError("mask must have d entries")
    return mask


def _ascent_launch(f, W, g, mk, tables, E, nt, n, d):
    dev = W.device
    with torch.cuda.device(dev):
        rc = f(_lib.ptr(W), _lib.ptr(g), _lib.ptr(mk), int(n), int(E), int(nt), int(d), _lib.ptr(tables[0]), _lib.ptr(tables[1]),
               _lib.stream_ptr(dev))
    _lib.check(rc, "nocf_disturbance_ascent_ensemble_f32")


_TABLES = {}


def _tables(step_size, eps, dev):
    """the device tables steps [E] and epss [E], float32 (the rounding the single-network entry gives its two doubles), in one copy; cached per
    device and value like PhiEnsemble.alph_table: a training loop passes the same budgets every iteration, and a host-to-device copy in front
    of every ascent step would make the host wait for the adjoint it has just enqueued"""
    key = (dev, tuple(step_size), tuple(eps))
    t = _TABLES.get(key)
    if t is None:
        if len(_TABLES) > 8:
            _TABLES.clear()
        t = _TABLES[key] = torch.tensor([step_size, eps], dtype=torch.float32).to(dev)
    return t[0], t[1]


def ensemble_ascend_disturbances(W, g, eps, step_size, mask=None):
    """ascend_disturbances for every member in one launch, in place (nocf_disturbance_ascent_ensemble_f32): for every row i of member e over
    its [nt, d] path,  W_ei += step_size_e (mask o g_ei) / ||mask o g_ei||  (untouched when that norm is 0 or not finite), then
    W_ei *= eps_e / ||W_ei|| when ||W_ei|| > eps_e.  Member e's slice is bit for bit ascend_disturbances(W[e], g[e], eps_e, step_size_e, mask).
    :param W:    E-by-nt-by-nex-by-d float32, contiguous, on the MI355X: updated;  g: the ascent direction, W's shape (W.grad); not modified
    :param eps, step_size: a float (every member) or E of them, finite and >= 0;  mask: [d] of 0 / 1 or None
    :return: W.  The call does not synchronise.  A W that requires a gradient is refused while autograd records: wrap the call in
    torch.no_grad() (ensemble_adversarial_step does).  Every check raises before a device is touched."""
    fn = "ensemble_ascend_disturbances"
    for name, t in (("W", W), ("g", g)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dtype == torch.float64:
            raise RuntimeError(f"{fn}: {name} is float64; the disturbed ensemble is single precision only (the double-precision kernels take "
                               "no disturbance and one network)")
    if W.dim() != 4 or min(W.shape) < 1:
        raise ValueError("W must be E-by-nt-by-nex-by-d")
    if tuple(g.shape) != tuple(W.shape):
        raise ValueError(f"g must have W's shape {tuple(W.shape)}, got {tuple(g.shape)}")
    E, nt, n, d = W.shape
    eps, step_size = _per_member(fn, "eps", eps, E), _per_member(fn, "step_size", step_size, E)
    mask = _mask_of(mask, d)
    if W.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"{fn} updates W in place: call it under torch.no_grad()")
    if g.device != W.device:
        raise ValueError("W and g must be on the same device")
    _lib.require_device_f32(W, "W")
    _lib.require_device_f32(g, "g")
    if not W.is_contiguous():
        raise ValueError("W must be contiguous (it is updated in place)")
    f = _entries(_lib.lib())["nocf_disturbance_ascent_ensemble_f32"]
    dev = W.device
    gc = g.detach().contiguous()
    mk = None if mask is None else (mask.reshape(-1) != 0).to(device=dev, dtype=torch.float32).contiguous()
    _ascent_launch(f, W.detach(), gc, mk, _tables(step_size, eps, dev), E, nt, n, d)
    return W


class _Search:
    """the buffers and the entries of one (x, ens, prob, nt) problem, adversary._Search for an ensemble: gradient() is one recording forward
    under W and one state-only ensemble adjoint; ascent() one projected step of all members.  Everything is allocated once; no call
    synchronises."""

    def __init__(self, x, ens, prob, nt, tspan, alph, stepper, objective, inv_n, want_dx, family):
        self.x, self.ens, self.prob, self.family = x.detach(), ens, prob, family
        self.E, self.n, self.d = E, n, d = ens.members, x.shape[-2], x.shape[-1]
        self.nt, self.tspan, self.stepper = int(nt), (float(tspan[0]), float(tspan[1])), stepper
        self.dev = dev = x.device
        rows = [list(r_) for r_ in (ens.alph if alph is None else ensemble._alph_rows(alph, E))]
        self.alph = rows
        # the adjoint's multipliers: "control" zeroes entries 3..5 of every member's row (adversary._Search does for one network)
        self.table_bwd = ens.alph_table([r_[:3] + [0.0, 0.0, 0.0] for r_ in rows] if objective == "control" else rows)
        self.inv_n = float(inv_n)
        self.L = L = _lib.lib()
        f = _entries(L)
        self.f_states = f[list(_ADJOINT[family])[1]]
        self.states_name = list(_ADJOINT[family])[1]
        self.f_ascent = f["nocf_disturbance_ascent_ensemble_f32"]
        self.hs = _step_sizes(self.tspan, self.nt).to(dev)
        self.dW = torch.empty(E, self.nt, n, d, device=dev)
        self.dx = torch.empty(E, n, d, device=dev) if want_dx else None
        self.bufs = {}
        self.forward_kernel = self.adjoint_kernel = None

    def gradient(self, W, shared=False):
        """persample [E, n, 7], dW [E, nt, n, d] (and dx) at W: two launches.  The returned tensors are this object's buffers."""
        ens, prob, dev, E, n, nt = self.ens, self.prob, self.dev, self.E, self.n, self.nt
        launch = ensemble._launch_mid if self.family == "mid" else ensemble._launch
        b = launch(self.x, ens, prob, self.tspan, nt, self.stepper, self.alph, record=True, bufs=self.bufs, dist=_Disturbance(W, shared))
        self.bufs = {k: v for k, v in b.items() if k in ("persample", "z_out", "sums", "s_all") or (k == "act" and v is not None)}
        if self.forward_kernel is None:
            self.forward_kernel = self.L.nocf_last_rollout_kernel().decode()
        phi_st, keep1 = ens._c_struct()
        prob_st, keep2 = prob._c_struct(dev)
        head = (C.byref(phi_st), C.byref(prob_st), n, E, nt, _STEPPERS[self.stepper], self.tspan[1], _lib.ptr(self.table_bwd), self.inv_n,
                _lib.ptr(b["s_all"]), _lib.ptr(b["z_out"]), _lib.ptr(self.hs))
        with torch.cuda.device(dev):
            if self.family == "mid":
                ws = ens.mid_workspace(self.L, dev)
                rc = self.f_states(*head, _lib.ptr(b.get("act")), _lib.ptr(self.dx), _lib.ptr(self.dW), _lib.ptr(ws), ws.numel(),
                                   _lib.stream_ptr(dev))
            else:
                rc = self.f_states(*head, _lib.ptr(self.dx), _lib.ptr(self.dW), _lib.stream_ptr(dev))
        _lib.check(rc, self.states_name)
        if self.adjoint_kernel is None:
            self.adjoint_kernel = self.L.nocf_last_rollout_kernel().decode()
        self.sums, self.table = b["sums"], b["table"]
        return b["persample"].view(E, n, 7), self.dW

    def ascent(self, W, mk, tables):
        _ascent_launch(self.f_ascent, W, self.dW, mk, tables, self.E, self.nt, self.n, self.d)

    def objective(self, tab):
        """[E, n] per-row objective of the adjoint's multipliers from a persample table [E, n, 7]"""
        a = self.table_bwd
        return tab[:, :, 0] + a[:, 0:1] * tab[:, :, 1] + a[:, 3:4] * tab[:, :, 2] + a[:, 4:5] * tab[:, :, 3] + a[:, 5:6] * tab[:, :, 4]


def _check_objective(objective):
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be 'Jc' or 'control', got {objective!r}")


def ensemble_disturbance_gradient(x, ens, prob, nt, W, tspan=(0., 1.), alph=None, stepper="rk4", objective="Jc", want_dx=False, *,
                                  family="lane"):
    """disturbance_gradient for every member in two launches: the recording forward under W and the state-only ensemble adjoint
    (nocf_rollout_bwd_small_ensemble_states_f32 / nocf_rollout_bwd_mid_ensemble_states_f32), under no_grad.
    :param W: E-by-nt-by-nex-by-d (or nt-by-nex-by-d, shared: dW[e] is then member e's gradient at that W); not modified
    :param objective: "Jc", or "control": L + alph0 G alone (the adjoint runs with entries 3..5 of every member's multipliers at 0)
    :return: dict Jc [E], cs [E, 7], persample [E, nex, 7], dW [E, nt, nex, d] = d(member e's mean objective)/dW[e], forward_kernel /
             adjoint_kernel (names), and with want_dx: dx [E, nex, d].  Member e's slices are bit for bit disturbance_gradient's on
             ens.member(e) with W[e] on the same kernel family.  Every check raises before a device is touched."""
    fn = "ensemble_disturbance_gradient"
    _check_objective(objective)
    E, n, d, _own, ds = _prepare(fn, x, ens, prob, nt, W, stepper, True, family)
    with torch.no_grad():
        s = _Search(x, ens, prob, nt, tspan, alph, stepper, objective, 1.0 / float(n), want_dx, family)
        tab, dW = s.gradient(ds.W, ds.shared)
        sums, a = s.sums, s.table
        means = sums[:, :7] / sums[:, 7:8]
        Jc = means[:, 0] + a[:, 0] * means[:, 1] + a[:, 3] * means[:, 2] + a[:, 4] * means[:, 3] + a[:, 5] * means[:, 4]
        out = {"Jc": Jc, "cs": means, "persample": tab, "dW": dW, "forward_kernel": s.forward_kernel, "adjoint_kernel": s.adjoint_kernel}
        if want_dx:
            out["dx"] = s.dx
    return out


def ensemble_worst_case_disturbances(x, ens, prob, nt, eps, steps=20, step_size=None, tspan=(0., 1.), alph=None, stepper="rk4",
                                     objective="control", mask=None, W0=None, *, family="lane"):
    """worst_case_disturbances for every member at once, member e over its own ball ||W_ei||_2 <= eps_e: projected gradient ascent on every
    start's own objective (inv_n = 1), every iteration three launches for all members (recording forward, state-only ensemble adjoint, ascent
    step) and no host round trip.
    :param eps:  a float or E of them: the members' radii;  steps: ascent steps;  step_size: a float or E of them (default, per member:
                 2.5 eps_e / steps)
    :param objective, mask: as for worst_case_disturbances;  W0: E-by-nt-by-nex-by-d start (default zeros); not modified
    :return: dict W [E, nt, nex, d] -- per start the iterate with the highest objective seen, the initial one included --, persample
             [E, nex, 7] and objective [E, nex] at that W, nominal [E, nex], history [steps + 1, E, nex].  Member e's slices are bit for bit
             worst_case_disturbances' on ens.member(e) with eps_e (a member at eps 0 keeps its nominal objective).
    The loop does not synchronise.  Every check raises before a device is touched."""
    fn = "ensemble_worst_case_disturbances"
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps must be >= 0")
    _check_objective(objective)
    E_ = ens.members if isinstance(ens, ensemble.PhiEnsemble) else 1
    eps = _per_member(fn, "eps", eps, E_)
    step_size = [2.5 * e_ / max(steps, 1) for e_ in eps] if step_size is None else _per_member(fn, "step_size", step_size, E_)
    if isinstance(x, torch.Tensor) and x.dim() in (2, 3):
        mask = _mask_of(mask, x.shape[-1])
    if W0 is not None:
        _check_W(fn, W0, x, ens, nt, "W0", shared_ok=False)
    E, n, d, _own = _refuse(fn, x, ens, prob, nt, stepper, True, family=family)
    _entries(_lib.lib())
    with torch.no_grad():
        _lib.check_errors()
        s = _Search(x, ens, prob, nt, tspan, alph, stepper, objective, 1.0, False, family)
        W = torch.zeros(E, int(nt), n, d, device=x.device) if W0 is None else W0.detach().clone()
        mk = None if mask is None else (mask.reshape(-1) != 0).to(device=s.dev, dtype=torch.float32).contiguous()
        tables = _tables(step_size, eps, s.dev)
        history = torch.empty(steps + 1, E, n, device=s.dev)
        best_W = best_tab = best_obj = None
        for it in range(steps + 1):
            tab, _ = s.gradient(W)
            obj = s.objective(tab)
            history[it] = obj
            if it == 0:
                best_W, best_tab, best_obj = W.clone(), tab.clone(), obj.clone()
            else:
                up = obj > best_obj
                best_obj = torch.where(up, obj, best_obj)
                best_tab = torch.where(up[:, :, None], tab, best_tab)
                best_W = torch.where(up[:, None, :, None], W, best_W)
            if it < steps:
                s.ascent(W, mk, tables)
    return {"W": best_W, "persample": best_tab, "objective": best_obj, "nominal": history[0].clone(), "history": history,
            "forward_kernel": s.forward_kernel, "adjoint_kernel": s.adjoint_kernel}


def ensemble_adversarial_step(x, ens, prob, tspan, nt, W, eps, step_size, mask=None, stepper="rk4", alph=None, *, family="lane"):
    """adversarial_step for an ensemble, one "free" adversarial iteration of all members in this order: (Jc [E], cs [E, 7]) =
    ensemble_minmax_ocflow_train at the current W; Jc.sum().backward() (the stacked parameters' .grad accumulate as usual, x.grad too when x
    requires one); W takes one projected ascent step along W.grad in place, member e with (eps_e, step_size_e)
    (ensemble_ascend_disturbances, under no_grad); W.grad is cleared.  Three launches.  The optimizer step stays the caller's, and the call
    does not synchronise.  W must be a leaf [E, nt, nex, d] that requires a gradient: it persists across the iterations on a batch.  Jc is
    returned detached (its graph is spent)."""
    fn = "ensemble_adversarial_step"
    if not isinstance(W, torch.Tensor):
        raise TypeError("W must be a torch.Tensor")
    E_ = ens.members if isinstance(ens, ensemble.PhiEnsemble) else 1
    eps, step_size = _per_member(fn, "eps", eps, E_), _per_member(fn, "step_size", step_size, E_)
    if W.dim() == 4:
        _mask_of(mask, W.shape[3])
    if W.dtype != torch.float64 and not (W.requires_grad and W.is_leaf):     # (float64: ensemble_minmax_ocflow_train's own refusal)
        raise ValueError(f"{fn}: W must be a leaf tensor that requires a gradient")
    Jc, cs = ensemble_minmax_ocflow_train(x, ens, prob, tspan, nt, W, stepper, alph, family=family)
    Jc.sum().backward()
    with torch.no_grad():
        ensemble_ascend_disturbances(W, W.grad, eps, step_size, mask)
    W.grad = None
    return Jc.detach(), cs
