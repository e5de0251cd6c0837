"""Sensitivity to, and the worst case over, per-step state disturbances.

disturb.py rolls the feedback law out under a given W [nt, n, d]; train.disturbed_ocflow_train differentiates such a rollout with respect
to the parameters.  Here it is differentiated with respect to W itself: since z_{k+1} = step(z_k) + W[k], dJ/dW[k] is the state cotangent
behind step k, which every adjoint kernel holds.  nocf_rollout_bwd_states_f32 is the adjoint with the parameter-gradient work compiled out
and those cotangents written out; nocf_disturbance_ascent_f32 is one projected ascent step.  An iteration of the search is three launches
(recording forward, state-only adjoint, ascent step) and no host round trip.  Single precision.  There is no CPU or eager-torch fallback."""
import ctypes as C

import torch

from . import _lib
from .train import _STEPPERS, _activation_record, _step_sizes

OBJECTIVES = ("Jc", "control")

_ENTRIES = ("nocf_rollout_record_disturbed_f32", "nocf_rollout_bwd_states_f32", "nocf_disturbance_ascent_f32")


def _entries(L):
    """the three entries _ENTRIES of library L, or None when L lacks one of them"""
    return _lib.entries(L, _ENTRIES)


def _check(fn, x, net, prob, nt, W, alph, stepper, objective, extra=()):
    """the argument checks of disturbed_ocflow_train, with its messages; every one raises before a device is touched.  W None: a search
    that starts from zeros"""
    tensors = [("x", x)] + ([] if W is None else [("W", W)]) + list(extra) + [(name, p_) for name, p_ in net.named_parameters()]
    for name, t in tensors:
        if isinstance(t, torch.Tensor) and t.dtype == torch.float64:
            raise RuntimeError(f"{fn}: {name} is float64; the disturbed rollout is single precision only "
                               "(the double-precision kernels take no disturbance)")
    for name, t in tensors[:2 - (W is None)]:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    if stepper not in _STEPPERS:
        raise ValueError(f"stepper must be 'rk4' or 'rk1', got {stepper!r}")
    if objective not in OBJECTIVES:
        raise ValueError(f"objective must be 'Jc' or 'control', got {objective!r}")
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
    if W is not None and tuple(W.shape) != (int(nt), n, d):
        raise ValueError(f"W must be nt-by-nex-by-d = {(int(nt), n, d)}, got {tuple(W.shape)}")
    if len(alph) < 6:
        raise ValueError("alph needs 6 entries")
    if W is not None and W.device != x.device:
        raise ValueError("x and W must be on the same device")
    _lib.require_device_f32(x, "x")
    if W is not None:
        _lib.require_device_f32(W, "W")
    return n, d


class _Search:
    """the buffers and the three entry points of one (x, net, prob, nt) problem: gradient() is one recording forward and one state-only
    adjoint at a given W; ascent() one projected step.  Everything is allocated once; no call synchronises."""

    def __init__(self, x, net, prob, nt, tspan, alph, stepper, objective, inv_n, want_dx, fn):
        self.x = _lib.require_device_f32(x.detach(), "x")
        self.n, self.d = n, d = self.x.shape
        self.nt, self.tspan, self.stepper, self.fn = int(nt), (float(tspan[0]), float(tspan[1])), stepper, fn
        self.dev = dev = self.x.device
        self.net = net
        self.phi_st, self._keep1, self.ws = net._c_struct(n)
        self.prob_st, self._keep2 = prob._c_struct(dev)
        nstage = 4 if stepper == "rk4" else 1
        self.persample = torch.empty(n, 7, device=dev)
        self.sums = torch.empty(8, device=dev)
        self.z_out = torch.empty(n, d + 4, device=dev)
        self.s_all = torch.empty(self.nt * nstage, n, d + 1, device=dev)
        self.dW = torch.empty(self.nt, n, d, device=dev)
        self.dx = torch.empty(n, d, device=dev) if want_dx else None
        self.hs = _step_sizes(self.tspan, self.nt).to(dev)
        a = [float(v) for v in alph[:6]]
        self.alph = a
        self.alph_fwd = (C.c_float * 6)(*a)
        self.alph_bwd = (C.c_float * 6)(*(a[:3] + [0.0, 0.0, 0.0] if objective == "control" else a))
        self.inv_n = float(inv_n)
        with torch.cuda.device(dev):
            L = _lib.lib_for(net.d, net.m, net.nTh, self.phi_st.r, self.prob_st.n_agents, fwd=self.prob_st.kind != _lib.PROB_QUADCOPTER)
            self.L, (self.f_rec, self.f_states, self.f_ascent) = _lib.entry_for(L, _ENTRIES, fn)
            # the activation record is the one-CU kernel's (m <= 128), as in train._OCflowTrainDisturbed
            self.act = _activation_record(self.L, net, n, self.nt, stepper, dev, one_cu_only=True)
        self.forward_kernel = self.adjoint_kernel = None

    def gradient(self, W):
        """persample [n, 7], dW [nt, n, d] (and dx) at W: two launches.  The returned tensors are this object's buffers."""
        dev, n = self.dev, self.n
        recorded = C.c_int32(0)
        with torch.cuda.device(dev):
            rc = self.f_rec(C.byref(self.phi_st), C.byref(self.prob_st), _lib.ptr(self.x), _lib.ptr(W), n,
                            self.tspan[0], self.tspan[1], self.nt, _STEPPERS[self.stepper], self.alph_fwd,
                            _lib.ptr(self.z_out), _lib.ptr(self.persample), _lib.ptr(self.sums), _lib.ptr(self.s_all), _lib.ptr(self.act),
                            C.byref(recorded), _lib.ptr(self.ws), self.ws.numel(), _lib.stream_ptr(dev))
            _lib.check(rc, "nocf_rollout_record_disturbed_f32")
            if self.forward_kernel is None:
                self.forward_kernel = self.L.nocf_last_rollout_kernel().decode()
            rc = self.f_states(C.byref(self.phi_st), C.byref(self.prob_st), n, self.nt, _STEPPERS[self.stepper], self.tspan[1],
                               self.alph_bwd, self.inv_n, _lib.ptr(self.s_all), _lib.ptr(self.z_out), _lib.ptr(self.hs),
                               _lib.ptr(self.act if recorded.value else None), _lib.ptr(self.dx), _lib.ptr(self.dW),
                               _lib.ptr(self.ws), self.ws.numel(), _lib.stream_ptr(dev))
            _lib.check(rc, "nocf_rollout_bwd_states_f32")
            if self.adjoint_kernel is None:
                self.adjoint_kernel = self.L.nocf_last_rollout_kernel().decode()
        return self.persample, self.dW

    def ascent(self, W, mask, step, eps):
        with torch.cuda.device(self.dev):
            rc = self.f_ascent(_lib.ptr(W), _lib.ptr(self.dW), _lib.ptr(mask), self.n, self.nt, self.d, float(step), float(eps),
                               _lib.stream_ptr(self.dev))
        _lib.check(rc, "nocf_disturbance_ascent_f32")

    def objective(self, tab):
        """[n] per-row objective of the adjoint's multipliers from a persample table"""
        a = self.alph_bwd
        return tab[:, 0] + a[0] * tab[:, 1] + a[3] * tab[:, 2] + a[4] * tab[:, 3] + a[5] * tab[:, 4]


def disturbance_gradient(x, net, prob, nt, W, tspan=(0., 1.), alph=None, stepper="rk4", n_total=None, objective="Jc", want_dx=False):
    """The disturbed rollout of disturb.disturbed_rollout at W and the gradient of its mean objective with respect to W: one recording
    forward (nocf_rollout_record_disturbed_f32) and one state-only adjoint (nocf_rollout_bwd_states_f32), under no_grad.
    :param W:   nt-by-nex-by-d float32 tensor on x's device; not modified
    :param alph: 6 multipliers (default: net.alph);  n_total: the global batch size when x is one shard of it (the mean runs over n_total rows)
    :param objective: "Jc" -- L + alph0 G + alph3 HJt + alph4 HJfin + alph5 HJgrad, what training minimises -- or "control": L + alph0 G alone
                      (the adjoint runs with alph[3:6] = 0; Jc and cs are the full forward's either way)
    :return: dict Jc, cs (7 means), persample [nex, 7], dW [nt, nex, d] = d(mean objective)/dW, forward_kernel / adjoint_kernel (names), and
             with want_dx: dx [nex, d] = d(mean objective)/dx
    Single precision only.  Every check raises before a device is touched."""
    alph = list(net.alph if alph is None else alph)
    if n_total is not None and int(n_total) < 1:
        raise ValueError("n_total must be >= 1")
    n, d = _check("disturbance_gradient", x, net, prob, nt, W, alph, stepper, objective)
    with torch.no_grad():
        _lib.check_errors()
        s = _Search(x, net, prob, nt, tspan, alph, stepper, objective, 1.0 / float(n_total or n), want_dx, "disturbance_gradient")
        tab, dW = s.gradient(_lib.require_device_f32(W.detach(), "W"))
        _lib.track_rollout_status(s.L, s.dev, "disturbance_gradient")
        means = s.sums[:7] / s.sums[7]
        Jc = means[0] + alph[0] * means[1] + alph[3] * means[2] + alph[4] * means[3] + alph[5] * means[4]
        out = {"Jc": Jc, "cs": [means[i] for i in range(7)], "persample": tab, "dW": dW,
               "forward_kernel": s.forward_kernel, "adjoint_kernel": s.adjoint_kernel}
        if want_dx:
            out["dx"] = s.dx
    return out


def worst_case_disturbances(x, net, prob, nt, eps, steps=20, step_size=None, tspan=(0., 1.), alph=None, stepper="rk4", objective="control",
                            mask=None, W0=None):
    """Projected gradient ascent on every start's OWN objective over the ball ||W_i||_2 <= eps (the norm over the row's whole [nt, d] path):
    the disturbance of a given energy that hurts the feedback law most.  Rows are independent (inv_n = 1).
    :param eps:  radius of the ball;  steps: ascent steps;  step_size: length of a step (default 2.5 eps / steps)
    :param objective: "control" -- L + alph0 G -- or "Jc": plus the three HJ terms
    :param mask: [d] of 0 / 1 (brownian_disturbances' meaning): components with 0 are not searched over
    :param W0:   nt-by-nex-by-d start (default zeros); not modified.  A W0 outside the ball is evaluated as it is and projected by the first step
    :return: dict W [nt, nex, d] -- per start the iterate with the highest objective seen, the initial one included --, persample [nex, 7] and
             objective [nex] at that W, nominal [nex] (the objective at the initial iterate), history [steps + 1, nex]
    The loop does not synchronise.  Single precision only.  Every check raises before a device is touched."""
    alph = list(net.alph if alph is None else alph)
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps must be >= 0")
    if not float(eps) >= 0.0 or float(eps) == float("inf"):
        raise ValueError("eps must be a finite number >= 0")
    step_size = (2.5 * float(eps) / max(steps, 1)) if step_size is None else float(step_size)
    if not step_size >= 0.0 or step_size == float("inf"):
        raise ValueError("step_size must be a finite number >= 0")
    if mask is not None:
        mask = torch.as_tensor(mask)
        if isinstance(x, torch.Tensor) and x.dim() == 2 and mask.numel() != x.shape[1]:
            raise ValueError("mask must have d entries")
    n, d = _check("worst_case_disturbances", x, net, prob, nt, W0, alph, stepper, objective)
    with torch.no_grad():
        _lib.check_errors()
        s = _Search(x, net, prob, nt, tspan, alph, stepper, objective, 1.0, False, "worst_case_disturbances")
        W = torch.zeros(int(nt), n, d, device=x.device) if W0 is None else _lib.require_device_f32(W0.detach(), "W").clone()
        mk = None if mask is None else (mask.reshape(-1) != 0).to(device=s.dev, dtype=torch.float32).contiguous()
        history = torch.empty(steps + 1, n, device=s.dev)
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
                best_tab = torch.where(up[:, None], tab, best_tab)
                best_W = torch.where(up[None, :, None], W, best_W)
            if it < steps:
                s.ascent(W, mk, step_size, eps)
        _lib.track_rollout_status(s.L, s.dev, "worst_case_disturbances")
    return {"W": best_W, "persample": best_tab, "objective": best_obj, "nominal": history[0].clone(), "history": history,
            "forward_kernel": s.forward_kernel, "adjoint_kernel": s.adjoint_kernel}
