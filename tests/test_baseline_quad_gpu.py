"""GPU: the quadcopter baseline kernels (nocf_baseline_quad.inc) against the reference's shipped result, the fixture and the fp64
restatement (util_quad), torch.optim.LBFGS in lockstep, convergence at the reference's settings, batch independence and the driver."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import neuraloc_amd as na
import util_quad as uq

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
REF_SETTINGS = dict(lr=1., max_iter=16000, max_eval=10000, tolerance_grad=1e-5, tolerance_change=1e-6, history_size=100)


@pytest.fixture(scope="module")
def gold():
    return uq.load_golden()


def quad(mass=1.0, grav=9.81):
    return na.Quadcopter(torch.tensor(uq.XTARGET, device=DEV), alph_Q=0.0, alph_W=0.0, mass=mass, grav=grav)


def test_reference_checkpoint(gold):
    """the shipped controls from xInit: loss, L, G and the trajectory of the reference's final loop"""
    rows, traj = na.quad_baseline_report(torch.tensor(uq.XINIT, device=DEV), torch.from_numpy(gold["ckpt/ctrls"]).to(DEV), quad(),
                                         uq.ALPHG)
    rows, traj = rows.cpu().double(), traj.cpu().double()
    for got, want in zip(rows.tolist(), (2182.70898, 2111.23608, 71.47299)):
        assert abs(got - want) <= 1e-5 * want, (got, want)
    ref = torch.from_numpy(gold["ckpt/traj"]).double()
    assert float((traj - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


def _check_objective(z0, U, prob_kw, ref64=None):
    prob = quad(**prob_kw)
    zc, uc = torch.as_tensor(z0).float(), torch.as_tensor(U).float()
    J, g = na.quad_baseline_loss(zc.to(DEV), uc.to(DEV), prob, uq.ALPHG, grad=True)
    B = max(zc.shape[0] if zc.dim() == 2 else 1, uc.shape[0] if uc.dim() == 3 else 1)
    zb, ub = zc.reshape(-1, 12).expand(B, 12), uc.reshape(-1, uc.shape[-2], 4).expand(B, -1, 4)
    J64, g64 = ref64 if ref64 is not None else uq.objective(zb, ub, grad=True, **prob_kw)
    J32, g32 = uq.objective(zb, ub, dtype=torch.float32, grad=True, **prob_kw)
    for name, got, w64, r32 in (("J", J, J64, J32), ("dJ/dU", g, g64, g32)):
        ok, err, tol = uq.compare(got.reshape(w64.shape), w64, r32)
        assert ok, f"{name}: err {err:.3e} > tol {tol:.3e}"
    rows, traj = na.quad_baseline_report(zc.to(DEV), uc.to(DEV), prob, uq.ALPHG)
    r64, t64 = uq.report(zb, ub, **prob_kw)
    r32, t32 = uq.report(zb, ub, dtype=torch.float32, **prob_kw)
    assert uq.compare(rows.reshape(r64.shape), r64, r32)[0]
    assert uq.compare(traj.reshape(t64.shape), t64, t32)[0]
    assert torch.equal(rows.reshape(-1, 3)[:, 0], J.reshape(-1))


@pytest.mark.parametrize("nt", uq.NT_LIST)
def test_objective_fixture(gold, nt):
    z0, U = gold[f"obj/nt{nt}/z0"], gold[f"obj/nt{nt}/U"]
    ref64 = (torch.from_numpy(gold[f"obj/nt{nt}/J64"]), torch.from_numpy(gold[f"obj/nt{nt}/g64"]))
    _check_objective(z0, U, {}, ref64)


@pytest.mark.parametrize("nt,B", [(1, 1027), (7, 3), (20, 1), (50, 1027), (256, 3)])
def test_objective_shapes(nt, B):
    g = torch.Generator().manual_seed(nt * 1000 + B)
    z0 = torch.tensor(uq.XINIT).repeat(B, 1)
    z0[:, :3] += torch.randn(B, 3, generator=g)
    z0[:, 3:] += 0.3 * torch.randn(B, 9, generator=g)
    U = torch.randn(B, nt, 4, generator=g)
    U[:, :, 0] = 9.81 + 2.0 * U[:, :, 0]
    _check_objective(z0, U, {})


def test_objective_broadcast_and_other_physics():
    g = torch.Generator().manual_seed(5)
    z0 = torch.tensor(uq.XINIT) + 0.2 * torch.randn(12, generator=g)
    Z = z0 + 0.5 * torch.randn(3, 12, generator=g)
    U = 5.0 + torch.randn(20, 4, generator=g)
    UB = 5.0 + torch.randn(3, 20, 4, generator=g)
    _check_objective(z0, UB, {})                              # one start, a batch of controls
    _check_objective(Z, U, {})                                # a batch of starts, one set of controls
    _check_objective(z0, U, {})                               # neither batched
    _check_objective(Z, UB, dict(mass=2.0, grav=5.0))         # a Quadcopter built directly with other physics
    J = na.quad_baseline_loss(z0.to(DEV), U.to(DEV), quad(), uq.ALPHG)
    assert J.dim() == 0


def _torch_lbfgs(z0, U0, prob, **kw):
    """torch.optim.LBFGS on the CPU whose closure returns the GPU's own objective and gradient"""
    ctrls = torch.nn.Parameter(U0.clone())
    opt = torch.optim.LBFGS([ctrls], line_search_fn="strong_wolfe", **kw)
    zd = z0.to(DEV)

    def closure():
        J, g = na.quad_baseline_loss(zd, ctrls.detach().to(DEV), prob, uq.ALPHG, grad=True)
        ctrls.grad = g.cpu()
        return J.cpu()

    opt.step(closure)
    st = opt.state[ctrls]
    return ctrls.detach(), int(st["n_iter"]), int(st["func_evals"])


@pytest.mark.parametrize("cap", [dict(max_iter=1), dict(max_iter=2), dict(max_iter=3), dict(max_iter=5), dict(max_iter=10),
                                 dict(max_iter=16000, max_eval=7)], ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_lbfgs_lockstep_with_torch(gold, cap):
    prob = quad()
    kw = dict(REF_SETTINGS, **cap)
    torch_kw = {k: v for k, v in kw.items()}
    for z0, U0 in zip(gold["lock/z0"], gold["lock/U0"]):
        z0, U0 = torch.from_numpy(z0), torch.from_numpy(U0)
        Ut, it, ev = _torch_lbfgs(z0, U0, prob, **torch_kw)
        Ug, loss, info = na.solve_baseline_quad(z0.to(DEV), prob, nt=50, alphG=uq.ALPHG, U0=U0.to(DEV), **kw)
        assert (int(info["n_iter"]), int(info["n_evals"])) == (it, ev)
        err = float((Ug.cpu() - Ut).abs().max())
        assert err <= 1e-4 * float(Ut.abs().max()), err
        J = na.quad_baseline_loss(z0.to(DEV), Ug, prob, uq.ALPHG)
        assert float(loss) == float(J)                       # the loss returned is the final iterate's


def test_lbfgs_converges_at_reference_settings(gold):
    prob = quad()
    z0 = torch.from_numpy(gold["solve/z0"]).to(DEV)
    U0 = torch.from_numpy(gold["solve/U0"]).to(DEV)
    U, loss, info = na.solve_baseline_quad(z0, prob, nt=50, alphG=uq.ALPHG, U0=U0, **REF_SETTINGS)
    want = torch.from_numpy(gold["solve/loss64"])
    assert (loss.cpu().double() <= want * (1 + 3e-4)).all(), (loss.cpu(), want)
    assert all(int(r) in na.baseline_quad.TOLERANCE_EXITS for r in info["reason"].cpu()), info["reason"]
    assert (info["n_evals"].cpu() >= info["n_iter"].cpu()).all() and (info["n_iter"].cpu() > 10).all()
    # tolerance_grad met at the start: returns at once with U unchanged
    U1, l1, i1 = na.solve_baseline_quad(z0[0], prob, nt=50, alphG=uq.ALPHG, U0=U0[0], **dict(REF_SETTINGS, tolerance_grad=1e9))
    assert torch.equal(U1, U0[0]) and (int(i1["n_iter"]), int(i1["n_evals"]), int(i1["reason"])) == (0, 1, 1)
    assert float(l1) == float(na.quad_baseline_loss(z0[0], U0[0], prob, uq.ALPHG))


def test_lbfgs_batch_independence():
    g = torch.Generator().manual_seed(1234)
    B = 1024
    z0 = torch.tensor(uq.XINIT).repeat(B, 1)
    z0[:, :3] += torch.randn(B, 3, generator=g)
    U0 = na.quad_initial_guess(50, B, g)
    z0, U0 = z0.to(DEV), U0.to(DEV)
    prob = quad()
    Ub, lb, ib = na.solve_baseline_quad(z0, prob, nt=50, U0=U0, **REF_SETTINGS)
    assert len(set(ib["n_iter"].cpu().tolist())) > 5            # the starts stop at different iteration counts
    for k in (0, 517, 1023):
        Ua, la, ia = na.solve_baseline_quad(z0[k], prob, nt=50, U0=U0[k], **REF_SETTINGS)
        assert torch.equal(Ua, Ub[k]) and torch.equal(la, lb[k])
        assert all(int(ia[n]) == int(ib[n][k]) for n in ("n_iter", "n_evals", "reason"))


def test_lbfgs_long_horizon_and_small_history():
    """nt at the limit (256) runs, and a history of 3 pairs wraps its ring many times"""
    prob = quad()
    z0 = torch.tensor(uq.XINIT, device=DEV)
    U, loss, info = na.solve_baseline_quad(z0, prob, nt=256, U0=na.quad_initial_guess(256).to(DEV), max_iter=40, history_size=5)
    assert torch.isfinite(U).all() and int(info["n_iter"]) >= 10
    assert float(loss) < float(na.quad_baseline_loss(z0, torch.zeros(256, 4, device=DEV), prob, uq.ALPHG))
    U, loss, info = na.solve_baseline_quad(z0, prob, nt=50, U0=na.quad_initial_guess(50).to(DEV), history_size=3, max_iter=200)
    assert int(info["n_iter"]) > 6 and torch.isfinite(U).all()


def test_driver(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(REPO, "baselineQuad.py"), "--nx", "1", "--max-iter", "20", "--save",
                        str(tmp_path)], capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"loss:\s+(\S+)\s+L\(x,T\):\s+(\S+)\s+G:\s+(\S+)", r.stdout)
    assert m, r.stdout
    loss, L, G = (float(v) for v in m.groups())
    assert abs(loss - (L + G)) <= 1e-5 * loss
    ck = torch.load(tmp_path / "baseline_quadcopter_alph5000_0_0.pth")
    assert set(ck) == {"ctrls", "traj", "loss", "L", "G"}
    assert ck["ctrls"].shape == (50, 4) and ck["traj"].shape == (12, 51)
    assert ck["loss"].shape == (1,) and ck["L"].shape == (1,) and ck["G"].shape == ()
    assert abs(float(ck["loss"][0]) - loss) <= 1e-5 * loss
