"""The reference's quadcopter baseline (baselineQuad.py) on the MI355X: the nt x 4 controls of one start of a single quadcopter are
the unknowns, forward Euler with h = 1/nt, torch.optim.LBFGS with the strong-Wolfe line search on the discretised cost.  B starts
are solved at once, one 64-lane workgroup each, and a whole LBFGS.step is one kernel launch (include/nocf.h:
nocf_baseline_quad_eval_f32, nocf_baseline_quad_lbfgs_f32; neuraloc_amd/csrc/nocf_baseline_quad.inc).

Single-agent Quadcopter only (d = 12), on the GPU only.  mass, grav and xtarget come from the problem; alph_Q and alph_W are
ignored, as the reference ignores them.  The precision follows the tensors, as in Phi.forward / OCflow: float32 z0 / U take the fp32
kernels, float64 ones (the reference's --prec double; every tensor of the call float64) the double-precision kernels
(nocf_baseline_quad_eval_f64, nocf_baseline_quad_lbfgs_f64; the same source, instantiated for double) and give float64 results.  With the
reference's tolerances (tolerance_change = 1e-6 on a loss of about 2182) only the double solve runs to the optimum: the fp32 one
stops where the loss stalls at fp32 resolution.

Shapes: z0 is [12] or [B, 12]; controls are [nt, 4] or [B, nt, 4] (a single set of controls or a single start is broadcast against
a batch).  When neither argument has a batch dimension, the results have none either."""
import ctypes as C

import torch

from . import _lib

NU = 4                              # controls per step: thrust and three angular accelerations
D = 12                              # the state of one quadcopter

# the exit that ended a solve (include/nocf.h NOCF_LB_*), in torch.optim.LBFGS's order of tests
REASONS = {0: "not run", 1: "tolerance_grad at start", 2: "gtd > -tolerance_change", 3: "max_iter", 4: "max_eval",
           5: "tolerance_grad", 6: "step <= tolerance_change", 7: "loss change < tolerance_change"}
TOLERANCE_EXITS = (1, 2, 5, 6, 7)
MAX_NT = 256                        # NOCF_BLQ_MAX_NT
MAX_HISTORY = 1024                  # NOCF_BLQ_MAX_HISTORY


def _check_prob(prob):
    if getattr(prob, "KIND", None) != _lib.PROB_QUADCOPTER or not hasattr(prob, "_c_struct"):
        raise TypeError(f"prob must be a neuraloc_amd Quadcopter object, got {type(prob).__name__}")
    if prob.d != D:
        raise ValueError(f"the quadcopter baseline solves for a single quadcopter (d = 12); this Quadcopter has d = {prob.d}")


def _check_shapes(z0, U, prob, nt=None):
    """-> (B, nt, single); raises before anything touches the device"""
    _check_prob(prob)
    for name, t in (("z0", z0), ("U", U)):
        if t is not None and not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    if z0.dim() not in (1, 2) or z0.shape[-1] != D:
        raise ValueError(f"z0 must be [12] or [B, 12], got {list(z0.shape)}")
    B = z0.shape[0] if z0.dim() == 2 else 1
    single = z0.dim() == 1
    if U is not None:
        if U.dim() not in (2, 3) or U.shape[-1] != NU:
            raise ValueError(f"controls must be [nt, 4] or [B, nt, 4], got {list(U.shape)}")
        if U.dim() == 3:
            if z0.dim() == 2 and U.shape[0] != B:
                raise ValueError(f"z0 has {B} points but the controls have {U.shape[0]}")
            B, single = U.shape[0], False
        nt = U.shape[-2]
    if nt is None or int(nt) < 1:
        raise ValueError("nt must be >= 1")
    if int(nt) > MAX_NT:
        raise ValueError(f"nt = {nt} is past the quadcopter baseline's limit of {MAX_NT} steps")
    if B < 1:
        raise ValueError("no starts")
    return B, int(nt), single


def _batch(z0, U, B, nt, double=False):
    z = _lib.require_device(z0, "z0", double).reshape(-1, D).expand(B, D).contiguous()
    u = None if U is None else _lib.require_device(U, "U", double).reshape(-1, nt, NU).expand(B, nt, NU).contiguous()
    return z, u


def _eval(z0, U, prob, alphG, grad, report):
    B, nt, single = _check_shapes(z0, U, prob)
    double = _lib.is_double(z0, U)
    z, u = _batch(z0, U, B, nt, double)
    dev = z.device
    st, keep = prob._c_struct64(dev) if double else prob._c_struct(dev)
    dt = torch.float64 if double else torch.float32
    loss = torch.empty(B, dtype=dt, device=dev)
    g = torch.empty(B, nt, NU, dtype=dt, device=dev) if grad else None
    rep = torch.empty(B, 3, dtype=dt, device=dev) if report else None
    traj = torch.empty(B, D, nt + 1, dtype=dt, device=dev) if report else None
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = (L.nocf_baseline_quad_eval_f64 if double else L.nocf_baseline_quad_eval_f32)(
            C.byref(st), D, B, nt, float(alphG), _lib.ptr(z), _lib.ptr(u), _lib.ptr(loss), _lib.ptr(g), _lib.ptr(rep), _lib.ptr(traj),
            _lib.stream_ptr(dev))
    _lib.check(rc, "nocf_baseline_quad_eval_f64" if double else "nocf_baseline_quad_eval_f32")
    if single:
        loss = loss[0]
        g = None if g is None else g[0]
        rep = None if rep is None else rep[0]
        traj = None if traj is None else traj[0]
    return loss, g, rep, traj


def quad_baseline_loss(z0, U, prob, alphG, grad=False):
    """compute_loss of baselineQuad.py:56-73: x_{i+1} = x_i + h dyn(U_i, x_i), J = sum_i h (2 + |U_i|^2) + alphG |x_nt - xtarget|^2 / 2.
    -> J [B] (and dJ/dU [B, nt, 4] when grad=True, from the hand-written adjoint of the Euler scheme)."""
    loss, g, _, _ = _eval(z0, U, prob, alphG, grad, False)
    return (loss, g) if grad else loss


def quad_baseline_report(z0, U, prob, alphG):
    """The final loop of baselineQuad.py:115-134 -> (rows [B, 3] = L+G, L, G;  trajectory [B, 12, nt+1])"""
    _, _, rep, traj = _eval(z0, U, prob, alphG, False, True)
    return rep, traj


def quad_initial_guess(nt, B=None, generator=None, dtype=torch.float32):
    """baselineQuad.py:75: 1e-2 randn(nt, 4) on the CPU generator, start by start ([nt, 4] when B is None, else [B, nt, 4]); the
    reference draws in the default dtype and converts (cvt), so a double guess is the fp32 draw widened"""
    if B is None:
        return (1.e-2 * torch.randn(int(nt), NU, generator=generator)).to(dtype)
    return torch.stack([1.e-2 * torch.randn(int(nt), NU, generator=generator) for _ in range(int(B))]).to(dtype)


def solve_baseline_quad(z0, prob, nt=50, alphG=5000., U0=None, generator=None, lr=1., max_iter=16000, max_eval=10000,
                        tolerance_grad=1e-5, tolerance_change=1e-6, history_size=100, line_search_fn="strong_wolfe"):
    """trainBaseline (baselineQuad.py:74-91): one torch.optim.LBFGS(...).step(closure) per start in z0 ([12] or [B, 12]), all in
    one launch.  U0: the initial controls ([nt, 4] or [B, nt, 4]); None: quad_initial_guess from `generator` (CPU).  max_eval=None
    is torch's default, max_iter * 5 // 4.
    -> (U, loss, info): the final iterate (torch leaves the last accepted point, not the best), its objective, and info =
    {"n_iter", "n_evals", "reason"} (int32 per start; reason: REASONS).  max_iter = 0 leaves U0 and reports n_evals = 0."""
    if line_search_fn != "strong_wolfe":
        raise ValueError("only line_search_fn='strong_wolfe' is built (the reference's setting)")
    if max_eval is None:
        max_eval = int(max_iter) * 5 // 4
    if int(max_iter) < 0 or int(max_eval) < 1:
        raise ValueError("max_iter must be >= 0 and max_eval >= 1")
    if not 1 <= int(history_size) <= MAX_HISTORY:
        raise ValueError(f"history_size must be in [1, {MAX_HISTORY}]")
    if U0 is None:
        B, nt, single = _check_shapes(z0, None, prob, nt)
        double = _lib.is_double(z0)
        _lib.require_device(z0, "z0", double)
        U0 = quad_initial_guess(nt, None if single else B, generator, torch.float64 if double else torch.float32).to(z0.device)
    B, nt, single = _check_shapes(z0, U0, prob)
    double = _lib.is_double(z0, U0)
    z, U = _batch(z0, U0, B, nt, double)
    U = U.clone()
    dev = U.device
    loss = torch.empty(B, dtype=U.dtype, device=dev)
    info = {k: torch.zeros(B, dtype=torch.int32, device=dev) for k in ("n_iter", "n_evals", "reason")}
    L = _lib.lib()
    nbytes = (L.nocf_baseline_quad_workspace_bytes_f64 if double else L.nocf_baseline_quad_workspace_bytes)(B, nt, int(history_size))
    if nbytes == 0:
        raise ValueError(f"no workspace for B = {B}, nt = {nt}, history_size = {history_size}")
    ws = torch.empty(nbytes // U.element_size(), dtype=U.dtype, device=dev)
    st, keep = prob._c_struct64(dev) if double else prob._c_struct(dev)
    with torch.cuda.device(dev):
        rc = (L.nocf_baseline_quad_lbfgs_f64 if double else L.nocf_baseline_quad_lbfgs_f32)(
            C.byref(st), D, B, nt, float(alphG), float(lr), int(max_iter), int(max_eval), float(tolerance_grad), float(tolerance_change),
            int(history_size), _lib.ptr(z), _lib.ptr(U), _lib.ptr(loss), _lib.ptr(info["n_iter"]), _lib.ptr(info["n_evals"]),
            _lib.ptr(info["reason"]), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
    _lib.check(rc, "nocf_baseline_quad_lbfgs_f64" if double else "nocf_baseline_quad_lbfgs_f32")
    if int(max_iter) == 0:
        loss = quad_baseline_loss(z, U, prob, alphG)
    if single:
        U, loss = U[0], loss[0]
        info = {k: v[0] for k, v in info.items()}
    return U, loss, info
