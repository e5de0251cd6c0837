"""CPU helpers of the quadcopter L-BFGS sweep: baseline_quad_lbfgs_kernel<T, E> (nocf_baseline_quad.inc) is built for E = 1, 2, 4, 8, 16
vector elements per lane and for float and double; the case list below reaches each of the ten builds on both sides of every boundary of
the dispatch rule, and the references, their self-agreement screens and the comparator live here so that the CPU file can test them
without a GPU.

References.  fp64: torch.optim.LBFGS on util_quad.rollout in double on the CPU (objective64: the closure of test_baseline_f64_gpu's
_restated_lbfgs).  fp32: torch.optim.LBFGS on the CPU around an objective the caller hands in (the GPU's own in the GPU file, util_quad's
fp32 restatement in the CPU file), so that only the optimiser's arithmetic differs from the kernel's.

Screens.  A case counts only if its reference agrees with itself.  fp32: the same solve with the flattened unknowns permuted (the
objective sees them un-permuted, bit for bit; only the order of torch's reductions changes, which is how the kernel differs from torch) must
give the same counts, PERMS times.  fp64: the counts must not move when J and the gradient carry NOISE relative noise, NOISE_RUNS times.

Tolerances.  fp64: REL_LBFGS of max|U| (the project's figure for capped L-BFGS iterates in double).  fp32: max(REL32 of max|U|,
TOL_FACTOR x the largest deviation among the permuted runs)."""
import collections
import concurrent.futures
import os
import threading

import numpy as np
import torch

import util_oracle as uo
import util_quad as uq

WAVE = 64                            # NOCF_BLQ_WAVE
PF_E = 8                             # NOCF_BLQ_PF_E: up to here the two-loop recursion loads the next pair ahead
BUILDS = (1, 2, 4, 8, 16)
REF_SETTINGS = dict(lr=1., max_iter=16000, max_eval=10000, tolerance_grad=1e-5, tolerance_change=1e-6, history_size=100)
REL_LBFGS = 1e-8                     # test_baseline_f64_gpu.REL_LBFGS
REL32 = 1e-4                         # test_baseline_quad_gpu.test_lbfgs_lockstep_with_torch
TOL_FACTOR = uo.TOL_FACTOR
PERMS = 3
NOISE = 1e-14
NOISE_RUNS = 3
MAX_LEFT_OUT = 1                     # per precision, over the whole sweep

# both sides of every boundary of E(nt); 4 nt below 64 (1, 4), a multiple of 64 (16, 32, 64, 128, 256) and every ragged tail (the rest)
HORIZONS = (1, 4, 16, 17, 32, 33, 64, 65, 128, 129, 256)
CAPS = (dict(max_iter=1), dict(max_iter=2), dict(max_iter=3), dict(max_iter=5),
        dict(max_iter=12, history_size=3),          # the ring wraps, head != 0
        dict(max_iter=12, history_size=1),
        dict(max_iter=16000, max_eval=7))           # cuts the line search at max_ls
WRAP_CAP = CAPS[4]
BIG_HISTORY = dict(max_iter=5, history_size=1024)   # the largest LDS layout
BIG_HISTORY_HORIZONS = (256, 64)
# One setting per exit reason (neuraloc_amd.baseline_quad.REASONS), found on the CPU with the fp64 restatement; each holds at both
# REASON_HORIZONS with the margin given (the nearest quantity that would have ended the solve elsewhere or otherwise, as a ratio).
#   1: |g|_inf of the start is 1.8e3 / 7.0e2, far below 1e9: (n_iter, n_evals) = (0, 1).
#   2: g.d = -|g|^2 of the first direction is -9.9e7 / -3.9e7 > -1e12: ends in the first iteration with one evaluation.
#   3, 4: the caps, past the point where a ring of 3 pairs has wrapped (7 iterations; 9 evaluations are reached in iteration 5).
#   5: |g|_inf after iterations 1, 2, 3, 4 is 1489, 871, 219, 150 at nt = 50 and 239, 394, 75, 61 at nt = 129: 180 ends the solve after
#      iteration 4 / 3, 17 % away from the nearest of them.
#   6: max|t d| of iterations 1 .. 4 is 2.6, 13, 2.2, 0.78 at nt = 50 and 10, 5.8, 2.6, 0.61 at nt = 129 while the loss moves by more
#      than 1e3 and g.d < -1e3: tolerance_change = 1 ends both after iteration 4, 22 % away.
#   7: met only near the optimum, 150 iterations from the reference's guess.  From the near-optimal controls of the fixture
#      (tests/golden/quad_sweep.npz, make_golden_quad_sweep.py) the first iteration moves U by 5.7e-6 and the loss by 9.3e-8 (nt = 50): the
#      reference's own tolerance_change = 1e-6 lies a factor 5 from either.
REASON_HORIZONS = (50, 129)                         # E = 4 (prefetch) and E = 16 (no prefetch)
REASON_SETTINGS = {1: dict(tolerance_grad=1e9),
                   2: dict(tolerance_change=1e12),
                   3: dict(max_iter=7, history_size=3),
                   4: dict(max_eval=9, history_size=3),
                   5: dict(tolerance_grad=180.),
                   6: dict(tolerance_change=1.0),
                   7: dict()}
WARM_REASONS = (7,)                                 # started from the fixture's controls
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quad_sweep.npz")

Case = collections.namedtuple("Case", "nt settings tag want_reason warm")


def lbfgs_E(nt):
    """the build the host picks: the smallest E in BUILDS that holds per_lane = ceil(4 nt / 64) elements"""
    per_lane = (4 * int(nt) + WAVE - 1) // WAVE
    for E in BUILDS:
        if per_lane <= E:
            return E
    raise ValueError(f"nt = {nt} is past the largest build")


def case_id(c):
    return f"nt{c.nt}-{c.tag}"


def _tag(d):
    return "-".join(f"{k}{v:g}" for k, v in d.items())


def cases():
    out = [Case(nt, dict(REF_SETTINGS, **cap), _tag(cap), None, False) for nt in HORIZONS for cap in CAPS]
    out += [Case(nt, dict(REF_SETTINGS, **BIG_HISTORY), _tag(BIG_HISTORY), None, False) for nt in BIG_HISTORY_HORIZONS]
    out += [Case(nt, dict(REF_SETTINGS, **s), f"reason{r}", r, r in WARM_REASONS) for nt in REASON_HORIZONS
            for r, s in sorted(REASON_SETTINGS.items())]
    return out


def case_start(c, dtype=torch.float32):
    """-> (z0 [12], U0 [nt, 4]) of a case"""
    z0, U0 = start(c.nt, dtype)
    if c.warm:
        U0 = torch.from_numpy(np.load(GOLDEN)[f"warm/nt{c.nt}"]).to(dtype)
    return z0, U0


def start(nt, dtype=torch.float32):
    """-> (z0 [12], U0 [nt, 4]): xInit and the reference's guess from a generator seeded by nt (a double guess is the fp32 draw widened)"""
    from neuraloc_amd import quad_initial_guess
    return torch.tensor(uq.XINIT, dtype=dtype), quad_initial_guess(nt, None, torch.Generator().manual_seed(int(nt)), dtype)


def batch_starts(nt, B, dtype=torch.float32):
    """B different starts around xInit with their own guesses"""
    from neuraloc_amd import quad_initial_guess
    g = torch.Generator().manual_seed(1000 + int(nt))
    z0 = torch.tensor(uq.XINIT).repeat(B, 1)
    z0[:, :3] += 0.5 * torch.randn(B, 3, generator=g)
    return z0.to(dtype), quad_initial_guess(nt, B, g, dtype)


def objective64(z0):
    """U [nt, 4] -> (J, dJ/dU) in double: the closure of test_baseline_f64_gpu._restated_lbfgs, op for op"""
    z = z0.double().reshape(1, -1)
    xt = torch.tensor(uq.XTARGET, dtype=torch.float64)

    def fun(U):
        ctrls = U.detach().clone().requires_grad_(True)
        L, traj = uq.rollout(z, ctrls.unsqueeze(0))
        err = (L + uq.ALPHG * 0.5 * torch.norm(traj[:, :, -1] - xt, p=2, dim=1) ** 2)[0]
        (g,) = torch.autograd.grad(err, ctrls)
        return err.detach(), g
    return fun


def objective32(z0):
    """util_quad's fp32 restatement: the stand-in for the GPU's objective where no GPU runs"""
    def fun(U):
        J, g = uq.objective(z0.reshape(1, -1), U.unsqueeze(0), dtype=torch.float32, grad=True)
        return J[0], g[0]
    return fun


def noisy(fun, seed, eps=NOISE):
    gen = torch.Generator().manual_seed(seed)

    def f(U):
        J, g = fun(U)
        return J * (1 + eps * float(torch.randn((), generator=gen))), g * (1 + eps * torch.randn(g.shape, generator=gen, dtype=g.dtype))
    return f


def dead_tail(fun, nt):
    """the objective with its gradient zeroed from element 64 (4 nt // 64) on: a tail slot that no lane fills"""
    def f(U):
        J, g = fun(U)
        g = g.clone()
        g.reshape(-1)[WAVE * (4 * nt // WAVE):] = 0
        return J, g
    return f


def expected_reason(opt, closure):
    """torch does not say which test ended LBFGS.step: re-apply its exit tests, in its order, to the state the optimiser saved (d, t,
    prev_flat_grad, prev_loss and the counters) and to the loss and gradient at the iterate it left, which `closure` evaluates again
    (torch's line search evaluated them at x + t d formed the same way, so they are the same bits) -> a key of REASONS"""
    group, st = opt.param_groups[0], opt.state[opt._params[0]]
    if st["n_iter"] == 0:
        return 1
    if st["prev_flat_grad"].dot(st["d"]) > -group["tolerance_change"]:       # (the exit copies the gradient into prev_flat_grad first)
        return 2
    if st["n_iter"] == group["max_iter"]:
        return 3
    if st["func_evals"] >= group["max_eval"]:
        return 4
    loss = float(closure())
    if opt._gather_flat_grad().abs().max() <= group["tolerance_grad"]:
        return 5
    if st["d"].mul(st["t"]).abs().max() <= group["tolerance_change"]:
        return 6
    if abs(loss - st["prev_loss"]) < group["tolerance_change"]:
        return 7
    raise AssertionError("no exit test of torch.optim.LBFGS holds at the state it left")


Solve = collections.namedtuple("Solve", "U n_iter n_evals reason pairs")


def torch_lbfgs(fun, U0, perm=None, **kw):
    """torch.optim.LBFGS(strong_wolfe).step on fun(U [nt, 4]) -> (J, dJ/dU) from U0; perm: the optimiser sees the flattened unknowns in
    this order (fun sees them in their own).  pairs: the (s, y) pairs held at the end."""
    n = U0.numel()
    perm = torch.arange(n) if perm is None else perm
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n)
    p = torch.nn.Parameter(U0.reshape(-1)[perm].clone())
    opt = torch.optim.LBFGS([p], line_search_fn="strong_wolfe", **kw)

    def closure():
        J, g = fun(p.detach()[inv].reshape(U0.shape))
        p.grad = g.reshape(-1)[perm].to(p.dtype).clone()
        return J

    opt.step(closure)
    st = opt.state[p]
    reason = expected_reason(opt, closure)
    return Solve(p.detach()[inv].reshape(U0.shape).clone(), int(st["n_iter"]), int(st["func_evals"]), reason, len(st.get("old_dirs") or ()))


def wrapped(sol, settings):
    """the history ring has wrapped: more iterations stored a pair than the ring holds (every iteration after the first stores one
    unless y.s <= 1e-10, which these solves do not meet before they end)"""
    return sol.pairs == settings["history_size"] and sol.n_iter - 1 > settings["history_size"]


Screened = collections.namedtuple("Screened", "ref ok spread counts")


def _perm(n, k):
    return torch.randperm(n, generator=torch.Generator().manual_seed(7919 * (k + 1) + n))


def _screened(ref, runs):
    counts = [(r.n_iter, r.n_evals) for r in [ref] + runs]
    same = len(set(counts)) == 1
    spread = max(float((r.U - ref.U).abs().max()) for r in runs) if same else float("nan")
    return Screened(ref, same, spread, counts)


class _SideBySide:
    """Several solves of one case ask for the objective one evaluation at a time each, and on the CPU an evaluation costs the same for a
    batch of controls as for one.  The solves run in a thread each; an evaluation waits until every solve still running has asked for
    its own, and the rows are then evaluated in one call of batched_fun(U [rows, nt, 4]) -> (J [rows], dJ/dU).  A solve keeps its row,
    and the batch keeps its size (a finished solve's row is filled with U0), so a row's arithmetic does not depend on the others."""

    def __init__(self, batched_fun, rows, fill):
        self.fun, self.rows, self.fill, self.active = batched_fun, rows, fill, rows
        self.cv, self.pending, self.results, self.error = threading.Condition(), {}, {}, None

    def _flush(self):
        if self.error is None and self.active and len(self.pending) == self.active:
            try:
                with torch.enable_grad():
                    J, g = self.fun(torch.stack([self.pending.get(i, self.fill) for i in range(self.rows)]))
                for i in self.pending:
                    self.results[i] = (J[i].clone(), g[i].clone())
            except BaseException as ex:                      # noqa: BLE001 -- the solves that wait must not wait for ever
                self.error = ex
            self.pending.clear()
            self.cv.notify_all()

    def row(self, i):
        def fun(U):
            with self.cv:
                self.pending[i] = U.detach().clone()
                self._flush()
                while i not in self.results and self.error is None:
                    self.cv.wait()
                if self.error is not None:
                    raise RuntimeError("the batched objective failed") from self.error
                return self.results.pop(i)
        return fun

    def done(self, i):
        with self.cv:
            self.active -= 1
            self._flush()


def side_by_side(batched_fun, U0, jobs, settings):
    """jobs: (wrap, perm) per solve: the solve sees wrap(its row's objective) with its unknowns in the order perm -> [Solve]"""
    sbs = _SideBySide(batched_fun, len(jobs), U0)

    def run(i):
        try:
            wrap, perm = jobs[i]
            return torch_lbfgs(wrap(sbs.row(i)), U0, perm=perm, **settings)
        finally:
            sbs.done(i)

    with concurrent.futures.ThreadPoolExecutor(len(jobs)) as ex:
        return list(ex.map(run, range(len(jobs))))


def objective64_batched(z0):
    """objective64 for U [rows, nt, 4]: the same restatement, its rows independent (the noisy solves of the fp64 screen)"""
    z = z0.double().reshape(1, -1)
    xt = torch.tensor(uq.XTARGET, dtype=torch.float64)

    def fun(Ub):
        ctrls = Ub.detach().clone().requires_grad_(True)
        L, traj = uq.rollout(z.expand(Ub.shape[0], -1), ctrls)
        err = L + uq.ALPHG * 0.5 * torch.norm(traj[:, :, -1] - xt, p=2, dim=1) ** 2
        (g,) = torch.autograd.grad(err.sum(), ctrls)
        return err.detach(), g
    return fun


def objective32_batched(z0):
    """objective32 for U [rows, nt, 4]"""
    def fun(Ub):
        return uq.objective(z0.reshape(1, -1).expand(Ub.shape[0], -1), Ub, dtype=torch.float32, grad=True)
    return fun


def screen32(fun, U0, settings):
    """the reference solve and PERMS permuted ones, one after the other (the GPU's objective) -> Screened: ok when all four give the same
    counts; spread: the largest deviation of a permuted run's U from the reference's"""
    ref = torch_lbfgs(fun, U0, **settings)
    return _screened(ref, [torch_lbfgs(fun, U0, perm=_perm(U0.numel(), k), **settings) for k in range(PERMS)])


def screen32_cpu(z0, U0, settings):
    """screen32 with util_quad's fp32 restatement standing in for the GPU's objective, the four solves side by side"""
    keep = lambda f: f                                       # noqa: E731
    jobs = [(keep, None)] + [(keep, _perm(U0.numel(), k)) for k in range(PERMS)]
    runs = side_by_side(objective32_batched(z0), U0, jobs, settings)
    return _screened(runs[0], runs[1:])


def screen64(z0, U0, settings):
    """the fp64 reference solve (on objective64, alone: the bits of _restated_lbfgs) and NOISE_RUNS solves with NOISE relative noise on J
    and on the gradient (side by side)"""
    ref = torch_lbfgs(objective64(z0), U0, **settings)
    jobs = [(lambda f, k=k: noisy(f, 31 * U0.numel() + k), None) for k in range(NOISE_RUNS)]
    return _screened(ref, side_by_side(objective64_batched(z0), U0, jobs, settings))


def tolerance(double, ref_U, spread):
    scale = float(ref_U.abs().max())
    return REL_LBFGS * scale if double else max(REL32 * scale, TOL_FACTOR * spread)


def compare_solve(got_U, got_counts, ref, tol):
    """-> (ok, err, why): the counts equal and max|U - ref.U| <= tol"""
    err = float((torch.as_tensor(got_U).detach().cpu().to(ref.U.dtype) - ref.U).abs().max())
    if tuple(int(c) for c in got_counts) != (ref.n_iter, ref.n_evals):
        return False, err, f"counts {tuple(got_counts)} against the reference's {(ref.n_iter, ref.n_evals)}"
    if not err <= tol:
        return False, err, f"U err {err:.3e} > tol {tol:.3e}"
    return True, err, ""
