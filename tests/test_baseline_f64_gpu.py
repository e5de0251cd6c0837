"""GPU: the double-precision baseline kernels (nocf_baseline_f64.inc, nocf_baseline_quad.inc instantiated for double) against the reference's own
double-precision values (tests/golden/baseline_f64.npz).

Tolerances.  REL = 1e-9 of each quantity's scale is the project's double-precision tolerance.  The capped L-BFGS
iterates are compared at 1e-8 of max|U| (a few iterations amplify the last-ulp differences of the dot products' summation order).
The full solve's margin over the reference's fp64 loss is 4x the gap observed on the MI355X with a floor of 1e-9 (SOLVE_GAP_OBSERVED
below; DESIGN section 3.7 records the run)."""
import json
import os

import numpy as np
import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import baseline as bl
import util_oracle as uo
import util_quad as uq

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
REL = 1e-9
REL_LBFGS = 1e-8
# relative gap (GPU double loss - fixture loss) / fixture loss of the full solve from xInit, measured on the MI355X: 2182.6809517867223
# after 152 iterations and 162 evaluations (the reference's own counts) against the fixture's 2182.6809517873417.  The GPU solve ended
# below the reference's loss, so the floor is the margin.
SOLVE_GAP_OBSERVED = -2.838e-13
SOLVE_MARGIN = max(4.0 * SOLVE_GAP_OBSERVED, 1e-9)
REF_SETTINGS = dict(lr=1., max_iter=16000, max_eval=10000, tolerance_grad=1e-5, tolerance_change=1e-6, history_size=100)
NAMES = ("softcorridor", "swap2", "swap12", "swap12_3pair", "midcross4", "midcross20", "swarm", "swarm50")
D64 = dict(dtype=torch.float64, device=DEV)


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_f64.npz"))
    g = {k: z[k] for k in z.files}
    g["meta"] = json.loads(str(g["meta"]))
    return g


def make_prob(name, mode):
    a = uo.BASE_ALPH[name]
    prob, _, _, xInit = na.initProb(name, 2, 2, var0=1.0, cvt=lambda t: t.double().to(DEV), alph=[a[0], a[1], a[2], 0.0, 0.0, 0.0])
    prob.train() if mode == "train" else prob.eval()
    return prob, xInit.reshape(-1), a[0]


def close(got, want, what, rel=REL):
    want = torch.as_tensor(want).double()
    got = got.detach().cpu().double().reshape(want.shape)
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"{what}: err {err:.3e}, scale {scale:.3e}, rel {err / scale if scale else 0.0:.3e}")
    assert err <= rel * scale, f"{what}: err {err:.3e} > {rel:g} x {scale:.3e}"


def check_case(gold, name, mode, key, B):
    """J, dJ/dU, the report rows and the trajectory of the fixture's starts at `key`, tiled to B starts"""
    prob, _, aG = make_prob(name, mode)
    z0, U = torch.from_numpy(gold[f"{name}/{key}/z0"]).double(), torch.from_numpy(gold[f"{name}/{key}/U"]).double()
    S = z0.shape[0]
    idx = np.arange(B) % S
    zb, Ub = z0[torch.from_numpy(idx)].to(DEV), U[torch.from_numpy(idx)].to(DEV)
    if B == 1:
        zb, Ub = zb[0], Ub[0]                                  # the unbatched form of the call
    J, g = na.baseline_loss(zb, Ub, prob, aG, grad=True)
    rows, traj = na.baseline_report(zb, Ub, prob, aG)
    assert all(t.dtype == torch.float64 for t in (J, g, rows, traj))
    J, g, rows, traj = (t.reshape((B,) + t.shape[(0 if B == 1 else 1):]) for t in (J, g, rows, traj))
    pre = f"{name}/{key}/{mode}"
    close(J, gold[f"{pre}/loss"][idx], f"{pre} B={B} J")
    for c, col in enumerate(("L+G", "L", "G", "Q", "W")):
        close(rows[:, c], gold[f"{pre}/report"][idx][:, c], f"{pre} B={B} report.{col}")
    if key == "lim":
        close(g.sum(1), gold[f"{pre}/grad_sum_t"][idx], f"{pre} B={B} sum_t dJ/dU")
        close(g.sum(2), gold[f"{pre}/grad_sum_k"][idx], f"{pre} B={B} sum_k dJ/dU")
        close(traj[:, :, -1], gold[f"{name}/{key}/final"][idx], f"{pre} B={B} z_nt")
    else:
        close(g, gold[f"{pre}/grad"][idx], f"{pre} B={B} dJ/dU")
        close(traj, gold[f"{name}/{key}/traj"][idx], f"{pre} B={B} traj")


@pytest.mark.parametrize("mode", ("train", "eval"))
@pytest.mark.parametrize("name", NAMES)
def test_objective_gradient_report(gold, name, mode):
    """nt = 1, 20, 50 (where the fixture has it: not swarm50, past its double limit) and the double limit; B = 1, 3 and, once per problem
    at nt = 20, 1027"""
    for key, B in (("nt1", 1), ("nt20", 3), ("nt20", 1), ("nt50", 1), ("lim", 1), ("lim", 3)) + ((("nt20", 1027),) if mode == "train" else ()):
        if f"{name}/{key}/z0" in gold:
            check_case(gold, name, mode, key, B)
        else:
            assert (name, key) == ("swarm50", "nt50")


@pytest.mark.parametrize("name", NAMES)
def test_one_past_the_limit_raises(gold, name):
    lim = gold["meta"]["limits"][name]
    prob, xInit, aG = make_prob(name, "train")
    assert bl.max_nt(prob, double=True) == bl.max_nt(prob, adam=True, double=True) == lim
    U = torch.zeros(lim + 1, prob.d, **D64)
    with pytest.raises(RuntimeError, match="double-precision limit"):
        na.baseline_loss(xInit, U, prob, aG)
    with pytest.raises(RuntimeError, match="double-precision limit"):
        na.solve_baseline(xInit, prob, lim + 1, niters=1, U0=U)
    Ub, best = na.solve_baseline(xInit, prob, lim, niters=2, U0=U[:lim])          # the limit itself runs
    assert torch.isfinite(Ub).all() and torch.isfinite(best)


def _adam(prob, z, U0, aG, niters, splits=None):
    U = U0.clone()
    m, v, Ub = torch.zeros_like(U), torch.zeros_like(U), torch.zeros_like(U)
    best = torch.full((U.shape[0],), float("inf"), **D64)
    hist = torch.empty(U.shape[0], niters, **D64)
    if splits is None:
        na.baseline_adam_steps(z, U, m, v, best, Ub, prob, aG, niters, 0, hist=hist)
    else:
        s0 = 0
        for k in splits:
            h = torch.empty(U.shape[0], k, **D64)
            na.baseline_adam_steps(z, U, m, v, best, Ub, prob, aG, k, s0, hist=h)
            hist[:, s0:s0 + k] = h
            s0 += k
        assert s0 == niters
    return U, m, v, best, Ub, hist


@pytest.mark.parametrize("name", NAMES)
def test_adam_ten_steps(gold, name):
    """10 reference Adam steps in double at 1e-9 of max|U| (and of the losses' scale); a split launch, a start inside a batch of 1027 and a
    second run give the same bits"""
    prob, xInit, aG = make_prob(name, "train")
    xi = torch.from_numpy(gold[f"{name}/xInit"]).to(DEV)
    assert float((xi - xInit).abs().max()) <= 1e-15 * float(xi.abs().max())      # (the fixture's start is the one used)
    U0 = torch.from_numpy(gold[f"{name}/nt20/U"][:1]).to(DEV)
    z = xi.reshape(1, -1)
    U, m, v, best, Ub, hist = _adam(prob, z, U0, aG, 10)
    close(U, gold[f"{name}/adam10/U"], f"{name} adam10 U")
    close(hist, gold[f"{name}/adam10/loss"], f"{name} adam10 losses")
    assert float(best) == float(hist.min())
    again = _adam(prob, z, U0, aG, 10)
    split = _adam(prob, z, U0, aG, 10, splits=(3, 1, 6))
    for a, b, c in zip((U, m, v, best, Ub, hist), again, split):
        assert torch.equal(a, b) and torch.equal(a, c)
    if name in ("softcorridor", "swarm"):                      # (one small and one 1024-thread problem: the batch costs GPU time)
        B = 1027
        g = torch.Generator().manual_seed(11)
        zb = (xi.cpu() + 0.3 * torch.randn(B, prob.d, generator=g, dtype=torch.float64)).to(DEV)
        Ub0 = (U0.cpu() + 0.5 * torch.randn(B, 20, prob.d, generator=g, dtype=torch.float64)).to(DEV)
        zb[700], Ub0[700] = xi, U0[0]
        big = _adam(prob, zb, Ub0, aG, 10)
        for a, b in zip((U, m, v, best, Ub, hist), big):
            assert torch.equal(a[0], b[700])


def test_adam_at_the_limit(gold):
    """midcross20 at its double limit (nt = 141: 1024 threads, the moments in the global M / V arrays) against the same solve by
    torch's Adam on the kernel's own gradient, and a split launch bitwise"""
    name = "midcross20"
    prob, xInit, aG = make_prob(name, "train")
    nt = gold["meta"]["limits"][name]
    U0 = torch.from_numpy(gold[f"{name}/lim/U"]).double().to(DEV)
    z = torch.from_numpy(gold[f"{name}/lim/z0"]).double().to(DEV)
    U, m, v, best, Ub, hist = _adam(prob, z, U0, aG, 6)
    split = _adam(prob, z, U0, aG, 6, splits=(2, 4))
    for a, b in zip((U, m, v, best, Ub, hist), split):
        assert torch.equal(a, b)
    p = torch.nn.Parameter(U0.clone())
    opt = torch.optim.Adam([p], lr=0.1)
    for _ in range(6):
        _, g = na.baseline_loss(z, p.detach(), prob, aG, grad=True)
        p.grad = g
        opt.step()
    close(U, p.detach().cpu(), "midcross20 nt=141 adam U")


def quad64():
    return na.Quadcopter(torch.tensor(uq.XTARGET, **D64), alph_Q=0.0, alph_W=0.0)


def test_quad_checkpoint_in_double(gold):
    """the shipped singlequad_baseline_checkpt.pth controls (baseline_quad.npz), evaluated in double"""
    q32 = uq.load_golden()
    z0 = torch.tensor(uq.XINIT, **D64)
    U = torch.from_numpy(q32["ckpt/ctrls"]).double().to(DEV)
    prob = quad64()
    J, g = na.quad_baseline_loss(z0, U, prob, uq.ALPHG, grad=True)
    rows, traj = na.quad_baseline_report(z0, U, prob, uq.ALPHG)
    assert all(t.dtype == torch.float64 for t in (J, g, rows, traj))
    close(J, gold["quad/ckpt/loss"], "quad ckpt J")
    close(g, gold["quad/ckpt/grad"], "quad ckpt dJ/dU")
    for c, col in enumerate(("L+G", "L", "G")):
        close(rows[c], gold["quad/ckpt/rows"][c], f"quad ckpt {col}")
    close(traj, gold["quad/ckpt/traj"], "quad ckpt traj")
    # batched, B = 1027: every row the same bits as the single call
    Jb, gb = na.quad_baseline_loss(z0.repeat(1027, 1), U, prob, uq.ALPHG, grad=True)
    assert torch.equal(Jb, J.expand(1027)) and torch.equal(gb, g.expand(1027, -1, -1))


def _restated_lbfgs(z0, U0, **kw):
    """util_quad's fp64 restatement driven through torch.optim.LBFGS on the CPU -> (n_iter, func_evals, U)"""
    ctrls = torch.nn.Parameter(U0.clone())
    opt = torch.optim.LBFGS([ctrls], line_search_fn="strong_wolfe", **kw)

    def closure():
        opt.zero_grad()
        L, traj = uq.rollout(z0.reshape(1, -1), ctrls.unsqueeze(0))
        err = (L + uq.ALPHG * 0.5 * torch.norm(traj[:, :, -1] - torch.tensor(uq.XTARGET, dtype=torch.float64), p=2, dim=1) ** 2)[0]
        err.backward()
        return err

    opt.step(closure)
    st = opt.state[ctrls]
    return int(st["n_iter"]), int(st["func_evals"]), ctrls.detach()


def test_quad_lbfgs_capped(gold):
    """the six capped runs: n_iter and func_evals of the reference's torch.optim.LBFGS in double, the iterate within 1e-8 of max|U|.  A
    case on which the CPU fp64 restatement itself disagrees with the fixture may be left out (at most one, printed)"""
    q32 = uq.load_golden()
    s = gold["meta"]["lock_start"]
    z0 = torch.from_numpy(q32["lock/z0"][s]).double()
    U0 = torch.from_numpy(q32["lock/U0"][s]).double()
    prob = quad64()
    left_out = []
    for k, cap in enumerate(gold["meta"]["caps"]):
        kw = dict(REF_SETTINGS, **cap)
        want_counts = tuple(int(c) for c in gold[f"quad/cap{k}/counts"])
        want_U = torch.from_numpy(gold[f"quad/cap{k}/U"])
        U, loss, info = na.solve_baseline_quad(z0.to(DEV), prob, nt=50, alphG=uq.ALPHG, U0=U0.to(DEV), **kw)
        got_counts = (int(info["n_iter"]), int(info["n_evals"]))
        err = float((U.cpu() - want_U).abs().max()) / float(want_U.abs().max())
        print(f"cap {cap}: counts {got_counts} (fixture {want_counts}), U rel err {err:.3e}, loss {float(loss)!r} (fixture {float(gold[f'quad/cap{k}/loss'])!r})")
        if got_counts != want_counts or err > REL_LBFGS:
            it, ev, Ur = _restated_lbfgs(z0, U0, **kw)
            if (it, ev) != want_counts or float((Ur - want_U).abs().max()) > REL_LBFGS * float(want_U.abs().max()):
                left_out.append(cap)
                print(f"cap {cap}: LEFT OUT -- the CPU fp64 restatement gives {(it, ev)} against the fixture's {want_counts}")
                continue
        assert got_counts == want_counts, (cap, got_counts, want_counts)
        assert err <= REL_LBFGS, (cap, err)
        assert U.dtype == loss.dtype == torch.float64
        assert float(loss) == float(na.quad_baseline_loss(z0.to(DEV), U, prob, uq.ALPHG))
    assert len(left_out) <= 1, left_out


def test_quad_full_solve_reaches_the_fp64_optimum(gold):
    """the reference-settings solve from xInit at nt = 50: a tolerance exit, a loss not above the reference's fp64 loss by more than the
    measured margin, and strictly below what the fp32 kernel reaches from the same start (the point of the feature); run to run and
    inside a batch the same bits"""
    q32 = uq.load_golden()
    z0 = torch.from_numpy(q32["solve/z0"][0])
    U0 = torch.from_numpy(q32["solve/U0"][0])
    assert gold["meta"]["solve_max_iter"] == REF_SETTINGS["max_iter"]
    U, loss, info = na.solve_baseline_quad(z0.double().to(DEV), quad64(), nt=50, alphG=uq.ALPHG, U0=U0.double().to(DEV), **REF_SETTINGS)
    want = float(gold["quad/solve/loss"])
    gap = (float(loss) - want) / want
    print(f"full solve in double: loss {float(loss)!r} ({int(info['n_iter'])} iterations, {int(info['n_evals'])} evaluations, reason "
          f"{int(info['reason'])}); fixture {want!r} ({[int(c) for c in gold['quad/solve/counts']]}); relative gap {gap:.3e}")
    assert int(info["reason"]) in na.baseline_quad.TOLERANCE_EXITS
    assert gap <= SOLVE_MARGIN, gap
    prob32 = na.Quadcopter(torch.tensor(uq.XTARGET, device=DEV), alph_Q=0.0, alph_W=0.0)
    U32, loss32, info32 = na.solve_baseline_quad(z0.to(DEV), prob32, nt=50, alphG=uq.ALPHG, U0=U0.to(DEV), **REF_SETTINGS)
    print(f"full solve in fp32: loss {float(loss32)!r} ({int(info32['n_iter'])} iterations)")
    assert loss32.dtype == torch.float32 and float(loss) < float(loss32)
    # determinism: a second run, and the same start among others (B = 3), bit for bit
    zb = z0.double().repeat(3, 1).to(DEV)
    zb[0, :3] += 0.25
    zb[2, :3] -= 0.25
    Ub, lb, ib = na.solve_baseline_quad(zb, quad64(), nt=50, alphG=uq.ALPHG, U0=U0.double().to(DEV), **REF_SETTINGS)
    assert torch.equal(Ub[1], U) and torch.equal(lb[1], loss) and int(ib["n_iter"][1]) == int(info["n_iter"])
    assert all(int(r) in na.baseline_quad.TOLERANCE_EXITS for r in ib["reason"].cpu())


def test_quad_default_guess_and_long_horizon():
    """U0 = None draws the reference's guess in z0's dtype; nt = 256 (E = 16, no prefetch) and a 3-pair history ring run in double"""
    prob = quad64()
    z0 = torch.tensor(uq.XINIT, **D64)
    U, loss, info = na.solve_baseline_quad(z0, prob, nt=20, generator=torch.Generator().manual_seed(2), max_iter=30)
    assert U.dtype == torch.float64 and U.shape == (20, 4) and int(info["n_iter"]) >= 10
    U, loss, info = na.solve_baseline_quad(z0, prob, nt=256, U0=na.quad_initial_guess(256, dtype=torch.float64).to(DEV), max_iter=40,
                                           history_size=5)
    assert torch.isfinite(U).all() and int(info["n_iter"]) >= 10
    assert float(loss) < float(na.quad_baseline_loss(z0, torch.zeros(256, 4, **D64), prob, uq.ALPHG))
    J, g = na.quad_baseline_loss(z0, U, prob, uq.ALPHG, grad=True)
    Jr, gr = uq.objective(z0.cpu().reshape(1, -1), U.cpu().unsqueeze(0), grad=True)
    close(J, Jr[0], "quad nt=256 J")
    close(g, gr[0], "quad nt=256 dJ/dU")
