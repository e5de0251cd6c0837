"""Min-max training against per-step state disturbances.

train.disturbed_ocflow_train differentiates a disturbed rollout with respect to the parameters; adversary.disturbance_gradient with respect
to the disturbance W, with a recording forward and a state-only adjoint of its own.  dJ/dW[k] is the state cotangent every FULL adjoint
kernel already holds when the last stage of step k begins, so the joint instantiations (nocf_rollout_bwd_small_w_f32 / _mid_w_f32 /
_act_w_f32) write it out beside the parameter gradients: one forward and one backward give both.  That is "free" adversarial training:
W persists across the iterations on a batch and takes one projected ascent step (nocf_disturbance_ascent_f32) per parameter step.
pgd_ocflow_train is the K-step adversary as the exact composition of the existing calls.  Single precision.  No CPU or eager-torch fallback."""
import torch

from . import _lib
from . import adversary
from .train import _OCflowTrain, _OCflowTrainDisturbed, disturbed_ocflow_train


class _OCflowTrainMinmax(torch.autograd.Function):
    """_OCflowTrainDisturbed with W differentiated too: the same recording forward (nocf_rollout_record_disturbed_f32), and as backward ONE
    launch of the joint entry of the forward's family, picked in _OCflowTrain._adjoint's lane -> one-CU -> per-tile order"""

    @staticmethod
    def forward(ctx, x, net, prob, tspan, nt, stepper, alph, n_total, group, W, *params):
        return _OCflowTrainDisturbed.forward(ctx, x, net, prob, tspan, nt, stepper, alph, n_total, group, W, *params)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gJ, _gmeans):
        return _OCflowTrain._adjoint(ctx, gJ, want_w=True)


def minmax_ocflow_train(x, net, prob, tspan, nt, W, stepper="rk4", alph=None, n_total=None, group=None):
    """disturbed_ocflow_train with Jc differentiable in W as well: (Jc, cs) of the disturbed rollout, and after Jc.backward() the parameter
    gradients, x.grad (when x requires one) and W.grad = dJc/dW [nt, nex, d] from one joint adjoint launch.
    :param W:   nt-by-nex-by-d float32 tensor on x's device.  When it does not require a gradient the call is disturbed_ocflow_train
    :param alph, n_total, group: as for disturbed_ocflow_train.  With n_total the mean runs over n_total rows (W.grad carries 1 / n_total);
                with group the parameter gradients are all-reduced; W.grad is the shard's own (rows are independent) and is not reduced
    Single precision only.  Every check raises before a device is touched."""
    alph = list(net.alph if alph is None else alph)
    adversary._check("minmax_ocflow_train", x, net, prob, nt, W, alph, stepper, "Jc")
    if not W.requires_grad:
        return disturbed_ocflow_train(x, net, prob, tspan, nt, W, stepper, alph, n_total, group)
    params = [p for _, p in net.named_parameters()]
    Jc, means = _OCflowTrainMinmax.apply(x, net, prob, list(tspan), int(nt), stepper, alph, n_total, group, W, *params)
    return Jc, [means[i] for i in range(7)]


def _ascent_scalars(eps, step_size, mask, d):
    """the checks of eps, step_size and mask (worst_case_disturbances' messages) -> (eps, step_size, mask as a tensor or None)"""
    eps, step_size = float(eps), float(step_size)
    if not eps >= 0.0 or eps == float("inf"):
        raise ValueError("eps must be a finite number >= 0")
    if not step_size >= 0.0 or step_size == float("inf"):
        raise ValueError("step_size must be a finite number >= 0")
    if mask is not None:
        mask = torch.as_tensor(mask)
        if d is not None and mask.numel() != d:
            raise ValueError("mask must have d entries")
    return eps, step_size, mask


def ascend_disturbances(W, g, eps, step_size, mask=None):
    """One projected ascent step on every row's disturbance path, in place (nocf_disturbance_ascent_f32): for every row i over its [nt, d]
    path,  W_i += step_size (mask o g_i) / ||mask o g_i||  (untouched when that norm is 0 or not finite), then W_i *= eps / ||W_i|| when
    ||W_i|| > eps.  Masked components keep their bits in the step.
    :param W:    nt-by-nex-by-d float32, contiguous, on the MI355X: updated;  g: the ascent direction, W's shape (W.grad); not modified
    :param mask: [d] of 0 / 1 (brownian_disturbances' meaning) or None
    :return: W.  The call does not synchronise.  A W that requires a gradient is refused while autograd records: wrap the call in
    torch.no_grad() (adversarial_step does).  Every check raises before a device is touched."""
    for name, t in (("W", W), ("g", g)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if t.dtype == torch.float64:
            raise RuntimeError(f"ascend_disturbances: {name} is float64; the disturbed rollout is single precision only "
                               "(the double-precision kernels take no disturbance)")
    if W.dim() != 3 or min(W.shape) < 1:
        raise ValueError("W must be nt-by-nex-by-d")
    if tuple(g.shape) != tuple(W.shape):
        raise ValueError(f"g must have W's shape {tuple(W.shape)}, got {tuple(g.shape)}")
    eps, step_size, mask = _ascent_scalars(eps, step_size, mask, W.shape[2])
    if W.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("ascend_disturbances updates W in place: call it under torch.no_grad()")
    if g.device != W.device:
        raise ValueError("W and g must be on the same device")
    _lib.require_device_f32(W, "W")
    _lib.require_device_f32(g, "g")
    if not W.is_contiguous():
        raise ValueError("W must be contiguous (it is updated in place)")
    nt, n, d = W.shape
    dev = W.device
    (ascent,) = _lib.require(_lib.lib(), ("nocf_disturbance_ascent_f32",), "ascend_disturbances")
    gc = g.detach().contiguous()
    mk = None if mask is None else (mask.reshape(-1) != 0).to(device=dev, dtype=torch.float32).contiguous()
    with torch.cuda.device(dev):
        rc = ascent(_lib.ptr(W.detach()), _lib.ptr(gc), _lib.ptr(mk), int(n), int(nt), int(d), step_size, eps, _lib.stream_ptr(dev))
    _lib.check(rc, "nocf_disturbance_ascent_f32")
    return W


def adversarial_step(x, net, prob, tspan, nt, W, eps, step_size, mask=None, stepper="rk4", alph=None, n_total=None, group=None):
    """One "free" adversarial iteration, in this order: (Jc, cs) = minmax_ocflow_train at the current W; Jc.backward() (the parameters'
    .grad accumulate as usual, x.grad too when x requires one); W takes one projected ascent step along W.grad in place
    (ascend_disturbances, under no_grad); W.grad is cleared.  The optimizer step stays the caller's, and the call does not synchronise.
    W must be a leaf that requires a gradient: it persists across the iterations on a batch.  Jc is returned detached (its graph is spent)."""
    if not isinstance(W, torch.Tensor):
        raise TypeError("W must be a torch.Tensor")
    _ascent_scalars(eps, step_size, mask, W.shape[2] if W.dim() == 3 else None)
    if W.dtype != torch.float64 and not (W.requires_grad and W.is_leaf):     # (float64: minmax_ocflow_train's own refusal)
        raise ValueError("adversarial_step: W must be a leaf tensor that requires a gradient")
    Jc, cs = minmax_ocflow_train(x, net, prob, tspan, nt, W, stepper, alph, n_total, group)
    Jc.backward()
    with torch.no_grad():
        ascend_disturbances(W, W.grad, eps, step_size, mask)
    W.grad = None
    return Jc.detach(), cs


def pgd_ocflow_train(x, net, prob, tspan, nt, eps, steps, objective="Jc", mask=None, W0=None, stepper="rk4", alph=None,
                     n_total=None, group=None):
    """The K-step adversary, as the exact composition of the existing calls:
        W = worst_case_disturbances(x, ..., eps, steps=steps, objective=objective, mask=mask, W0=W0)["W"]
        Jc, cs = disturbed_ocflow_train(x, ..., W)
    The search runs on the same x with tspan, alph and stepper passed through; objective "control" (L + alph0 G) is what the free mode cannot
    offer, because its adversary climbs the training loss itself.  -> (Jc, cs, W)"""
    W = adversary.worst_case_disturbances(x, net, prob, nt, eps, steps=steps, tspan=tuple(tspan), alph=alph,
                                          stepper=stepper, objective=objective, mask=mask, W0=W0)["W"]
    Jc, cs = disturbed_ocflow_train(x, net, prob, tspan, nt, W, stepper, alph, n_total, group)
    return Jc, cs, W
