"""The reference's direct-transcription baseline (baseline2D.py) on the MI355X: the nt x d control sequence of one initial state is
the unknown, forward Euler with h = 1/nt, Adam on the discretised cost.  B initial states are solved at once, one workgroup each, and
a whole solve is one kernel launch (include/nocf.h: nocf_baseline_eval_f32, nocf_baseline_adam_f32; neuraloc_amd/csrc/nocf_baseline.inc).

Point-agent problems only (Cross2D, SwarmTraj), on the GPU only.  The precision follows the tensors, as in Phi.forward / OCflow:
float32 z0 / U take the fp32 kernels, float64 ones (the reference's --prec double; every tensor of the call float64) the double-precision
kernels (nocf_baseline_eval_f64, nocf_baseline_adam_f64; nocf_baseline_f64.inc) and give float64 results.  The problem's current
train() / eval() mode is used, as OCflow does: the reference optimises in train mode (baseline2D.py:115) and reports in eval mode (:129).

Shapes: z0 is [d] or [B, d]; controls are [nt, d] or [B, nt, d] (a single set of controls or a single start is broadcast against a
batch).  When neither argument has a batch dimension, the results have none either."""
import ctypes as C

import torch

from . import _lib

ADAM_BETAS = (0.9, 0.999)      # torch.optim.Adam defaults (baseline2D.py:86)
ADAM_EPS = 1e-8


def _check_prob(prob):
    kind = getattr(prob, "KIND", None)
    if kind == _lib.PROB_QUADCOPTER:
        raise ValueError("the direct-transcription baseline covers the point-agent problems (Cross2D, SwarmTraj); the quadcopter "
                         "baseline (baselineQuad.py: other dynamics, L-BFGS) is not this method: use solve_baseline_quad")
    if kind not in (_lib.PROB_CROSS2D, _lib.PROB_SWARMTRAJ) or not hasattr(prob, "_c_struct"):
        raise TypeError(f"prob must be a neuraloc_amd Cross2D or SwarmTraj object, got {type(prob).__name__}")


def _prob_struct(prob, device, double=False):
    _check_prob(prob)
    return prob._c_struct64(device) if double else prob._c_struct(device)


def max_nt(prob, adam=False, double=False):
    """the largest nt the eval (adam=False) / Adam (adam=True) kernels take for this problem in fp32 or double: the one point's arrays
    must fit the LDS (include/nocf.h: nocf_baseline_max_nt)"""
    _check_prob(prob)
    st = _lib.NocfProb()
    st.kind, st.n_agents = prob.KIND, prob.nAgents
    return _lib.lib().nocf_baseline_max_nt(C.byref(st), prob.d, int(bool(adam)), 8 if double else 4)


def _check_rc(rc, what, prob, nt, adam, double):
    if rc == -2 and double:
        lim = max_nt(prob, adam, True)
        if nt > lim:
            raise RuntimeError(f"{what}: nt = {nt} is past the double-precision limit of {lim} steps for this problem (d = {prob.d}: at most 256, and "
                               "U, z and dJ/dU of one start within the 160 KiB of LDS as doubles)")
    _lib.check(rc, what)


def _check_shapes(z0, U, prob, nt=None):
    """-> (B, nt, single); raises ValueError on a shape mismatch or an unsupported problem (before anything touches the device)"""
    _check_prob(prob)
    for name, t in (("z0", z0), ("U", U)):
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    d = prob.d
    if z0.dim() not in (1, 2) or z0.shape[-1] != d:
        raise ValueError(f"z0 must be [d] or [B, d] with d = {d}, got {list(z0.shape)}")
    B = z0.shape[0] if z0.dim() == 2 else 1
    single = z0.dim() == 1
    if U is not None:
        if U.dim() not in (2, 3) or U.shape[-1] != d:
            raise ValueError(f"controls must be [nt, d] or [B, nt, d] with d = {d}, got {list(U.shape)}")
        if U.dim() == 3:
            if z0.dim() == 2 and U.shape[0] != B:
                raise ValueError(f"z0 has {B} points but the controls have {U.shape[0]}")
            B, single = U.shape[0], False
        nt = U.shape[-2]
    if nt is None or int(nt) < 1:
        raise ValueError("nt must be >= 1")
    return B, int(nt), single


def _batch(z0, U, B, nt, d, double=False):
    z = _lib.require_device(z0, "z0", double).reshape(-1, d).expand(B, d).contiguous()
    u = None if U is None else _lib.require_device(U, "U", double).reshape(-1, nt, d).expand(B, nt, d).contiguous()
    return z, u


def _eval(z0, U, prob, alphG, grad, report):
    B, nt, single = _check_shapes(z0, U, prob)
    d = prob.d
    double = _lib.is_double(z0, U)
    z, u = _batch(z0, U, B, nt, d, double)
    dev = z.device
    st, keep = _prob_struct(prob, dev, double)
    dt = torch.float64 if double else torch.float32
    loss = torch.empty(B, dtype=dt, device=dev)
    g = torch.empty(B, nt, d, dtype=dt, device=dev) if grad else None
    rep = torch.empty(B, 5, dtype=dt, device=dev) if report else None
    traj = torch.empty(B, d, nt + 1, dtype=dt, device=dev) if report else None
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = (L.nocf_baseline_eval_f64 if double else L.nocf_baseline_eval_f32)(
            C.byref(st), d, B, nt, float(alphG), _lib.ptr(z), _lib.ptr(u), _lib.ptr(loss), _lib.ptr(g), _lib.ptr(rep), _lib.ptr(traj),
            _lib.stream_ptr(dev))
    _check_rc(rc, "nocf_baseline_eval_f64" if double else "nocf_baseline_eval_f32", prob, nt, False, double)
    if single:
        loss = loss[0]
        g = None if g is None else g[0]
        rep = None if rep is None else rep[0]
        traj = None if traj is None else traj[0]
    return loss, g, rep, traj


def baseline_loss(z0, U, prob, alphG, grad=False):
    """The objective of baseline2D.py:42-63 (loss_fun): z_{i+1} = z_i + h U_i, then h L(z_{i+1}, U_i), plus alphG |z_nt - xtarget|^2 / 2.
    -> J [B] (and dJ/dU [B, nt, d] when grad=True, from the hand-written adjoint)."""
    loss, g, _, _ = _eval(z0, U, prob, alphG, grad, False)
    return (loss, g) if grad else loss


def baseline_report(z0, U, prob, alphG):
    """The report of baseline2D.py:136-150 / compareCorridor.py:100-113: L(z_j, U_j) at the state BEFORE the step.
    -> (rows [B, 5] = L+G, L, G, Q, W;  trajectory [B, d, nt+1]).  Q as calcLHQW returns it (scaled by alph_Q for Cross2D only).
    The reference reports in eval mode: call prob.eval() first."""
    _, _, rep, traj = _eval(z0, U, prob, alphG, False, True)
    return rep, traj


def baseline_adam_steps(z0, U, m, v, best, Ubest, prob, alphG, niters, step0=0, lr=0.1, betas=ADAM_BETAS, eps=ADAM_EPS, hist=None):
    """Advance a batched solve IN PLACE by niters iterations of trainBaseline (baseline2D.py:88-105) in one launch: evaluate J(U);
    if J < best keep U in Ubest; take torch's single-tensor Adam step (weight decay 0, constant lr).  U, m, v, Ubest: [B, nt, d];
    best: [B] (+inf for a fresh solve); hist: [B, niters] or None; step0: Adam steps already taken.  A solve split into launches is
    bitwise the same as one launch."""
    if U.dim() != 3:
        raise ValueError("U must be [B, nt, d]")
    B, nt, single = _check_shapes(z0, U, prob)
    d = prob.d
    double = _lib.is_double(z0, U)
    z = _lib.require_device(z0, "z0", double).reshape(-1, d).expand(B, d).contiguous()
    for name, t, shape in (("U", U, (B, nt, d)), ("m", m, (B, nt, d)), ("v", v, (B, nt, d)), ("Ubest", Ubest, (B, nt, d)),
                           ("best", best, (B,)), ("hist", hist, (B, int(niters)))):
        if t is None and name == "hist":
            continue
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must be {list(shape)}, got {list(t.shape)}")
        _lib.require_device(t, name, double)
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous (it is updated in place)")
    dev = z.device
    st, keep = _prob_struct(prob, dev, double)
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = (L.nocf_baseline_adam_f64 if double else L.nocf_baseline_adam_f32)(
            C.byref(st), d, B, nt, float(alphG), float(lr), float(betas[0]), float(betas[1]), float(eps), int(step0), int(niters),
            _lib.ptr(z), _lib.ptr(U), _lib.ptr(m), _lib.ptr(v), _lib.ptr(best), _lib.ptr(Ubest), _lib.ptr(hist), _lib.stream_ptr(dev))
    _check_rc(rc, "nocf_baseline_adam_f64" if double else "nocf_baseline_adam_f32", prob, nt, True, double)


def initial_guess(z0, prob, nt, generator=None):
    """baseline2D.py:80-83: (xtarget - z0) on every row plus 0.1 randn(nt, d), drawn on z0's device from `generator`, in z0's dtype"""
    z = z0.reshape(-1, prob.d)
    y = prob.xtarget.to(device=z.device, dtype=z.dtype).reshape(1, 1, -1) - z.unsqueeze(1)
    U0 = y * torch.ones(z.shape[0], int(nt), prob.d, device=z.device, dtype=z.dtype) + \
        0.1 * torch.randn(z.shape[0], int(nt), prob.d, device=z.device, dtype=z.dtype, generator=generator)
    return U0[0] if z0.dim() == 1 else U0


def solve_baseline(z0, prob, nt, niters=600, alphG=100., lr=0.1, U0=None, generator=None, history=False):
    """trainBaseline (baseline2D.py:65-107) for every start in z0 ([d] or [B, d]) in one launch.
    U0: the initial controls ([nt, d] or [B, nt, d]); None: the reference's straight-line guess drawn on the device from `generator`.
    -> (Ubest, best_loss[, loss_hist]): the controls of the best objective seen (the reference returns ubest, not the last iterate),
    that objective, and with history=True the objective of every iteration [B, niters]."""
    if U0 is None:
        _check_shapes(z0, None, prob, nt)
        _lib.require_device(z0, "z0", _lib.is_double(z0))
        U0 = initial_guess(z0, prob, nt, generator)
    B, nt, single = _check_shapes(z0, U0, prob)
    d = prob.d
    z, U = _batch(z0, U0, B, nt, d, _lib.is_double(z0, U0))
    U = U.clone()
    m = torch.zeros_like(U)
    v = torch.zeros_like(U)
    Ubest = torch.zeros_like(U)
    best = torch.full((B,), float("inf"), dtype=U.dtype, device=U.device)
    hist = torch.empty(B, int(niters), dtype=U.dtype, device=U.device) if history else None
    baseline_adam_steps(z, U, m, v, best, Ubest, prob, alphG, int(niters), 0, lr, hist=hist)
    if single:
        Ubest, best, hist = Ubest[0], best[0], (None if hist is None else hist[0])
    return (Ubest, best, hist) if history else (Ubest, best)
