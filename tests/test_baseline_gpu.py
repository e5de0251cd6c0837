"""GPU: the direct-transcription baseline kernels (neuraloc_amd.baseline; include/nocf.h nocf_baseline_*) against the reference fixture
tests/golden/baseline.npz (make_golden_baseline.py), their determinism over batch size and launch splits, and the baseline2D.py driver."""
import json
import os
import re

import numpy as np
import pytest
import torch

import neuraloc_amd as na

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(REPO, "tests", "golden", "baseline.npz"))
META = json.loads(str(FIX["meta"]))
CASES = [(name, nt, mode) for name, info in META["problems"].items() for nt in info["nts"] for mode in ("train", "eval")]
DEV = torch.device("cuda:0")


def make_prob(name, alph):
    prob, _, _, xInit = na.initProb(name, 10, 10, var0=1.0, cvt=lambda t: t.float().to(DEV),
                                    alph=[alph[0], alph[1], alph[2], 0.0, 0.0, 0.0])
    return prob, xInit.reshape(-1)


def fx(key):
    return torch.from_numpy(np.array(FIX[key])).to(DEV)


def w_atol(prob):
    """Rounding of the reference's W itself: for more than two agents calcW sums exp() over all N^2 entries, the masked ones and the
    diagonal included (each is 1), and then subtracts their count (Cross2D.py:150-160, SwarmTraj.py:149-160).  In fp32 that difference
    carries an absolute error of up to ~N^2 2^-24 per state; the kernels sum the pairs inside the threshold only.  Over the report's
    sum of h W (sum h = 1) the bound stays N^2 2^-24; the L columns see it times alph_W."""
    N = prob.nAgents
    return (N * N * 2.0 ** -24) if (N > 2 and prob.alph_W != 0.0) else 0.0


def assert_rows(got, want, what, wtol=0.0, alphW=0.0):
    got, want = got.double().cpu(), want.double().cpu()
    tol = 1e-5 * torch.clamp(want.abs(), min=1e-3)
    tol[[0, 1]] += abs(alphW) * wtol
    tol[4] += wtol
    assert bool(((got - want).abs() <= tol).all()), f"{what}: got {got.tolist()} want {want.tolist()}"


@pytest.mark.parametrize("name,nt,mode", CASES)
def test_objective_gradient_report_match_reference(name, nt, mode):
    info = META["problems"][name]
    prob, _ = make_prob(name, info["alph"])
    prob.train() if mode == "train" else prob.eval()
    pre = f"{name}/nt{nt}"
    z0, U = fx(f"{pre}/z0"), fx(f"{pre}/U")
    J, g = na.baseline_loss(z0, U, prob, info["alph"][0], grad=True)
    want = fx(f"{pre}/{mode}/loss")
    assert torch.allclose(J, want, rtol=1e-5, atol=0), (J.tolist(), want.tolist())
    gw = fx(f"{pre}/{mode}/grad")
    for k in range(z0.shape[0]):
        err = float((g[k] - gw[k]).abs().max())
        assert err <= 1e-5 * float(gw[k].abs().max()), (k, err, float(gw[k].abs().max()))
    rows, traj = na.baseline_report(z0, U, prob, info["alph"][0])
    for k in range(z0.shape[0]):
        assert_rows(rows[k], fx(f"{pre}/{mode}/report")[k], f"{pre} {mode} start {k}", w_atol(prob), prob.alph_W)
    tw = fx(f"{pre}/{mode}/traj")
    assert float((traj - tw).abs().max()) <= 1e-5 * float(tw.abs().max())


def test_shipped_controls_reproduce_compare_corridor():
    calph = META["checkpt_alph"]
    prob, xInit = make_prob("softcorridor", calph)
    prob.eval()
    assert torch.equal(xInit.cpu(), torch.from_numpy(FIX["checkpt/z0"]))
    rows, traj = na.baseline_report(xInit, fx("checkpt/U"), prob, calph[0])
    assert rows.shape == (5,) and traj.shape == (4, 51)
    assert_rows(rows, fx("checkpt/report"), "softcorridor_baseline_checkpt.pth")
    assert float((traj - fx("checkpt/traj")).abs().max()) <= 1e-5 * float(fx("checkpt/traj").abs().max())


@pytest.mark.parametrize("name", list(META["problems"]))
def test_adam_path_matches_reference(name):
    info = META["problems"][name]
    prob, _ = make_prob(name, info["alph"])
    prob.train()
    z0 = fx(f"{name}/nt20/z0")[0:1]
    U = fx(f"{name}/nt20/U")[0:1].clone()
    m, v, Ub = torch.zeros_like(U), torch.zeros_like(U), torch.zeros_like(U)
    best = torch.full((1,), float("inf"), device=DEV)
    hist = torch.empty(1, 10, device=DEV)
    na.baseline_adam_steps(z0, U, m, v, best, Ub, prob, info["alph"][0], 10, hist=hist)
    want = fx(f"{name}/adam10/loss")
    assert torch.allclose(hist[0], want, rtol=1e-4, atol=0), (hist[0].tolist(), want.tolist())
    err = float((U[0] - fx(f"{name}/adam10/U")).abs().max())
    assert err <= 1e-4, err
    assert float(best[0]) == float(hist[0].min())


def test_full_default_solve_reaches_reference_loss():
    alph = META["solve600"]["alph"]
    prob, _ = make_prob("softcorridor", alph)
    prob.train()
    Ubest, best = na.solve_baseline(fx("solve600/z0"), prob, 50, niters=600, alphG=alph[0], U0=fx("solve600/U0"))
    ref = float(FIX["solve600/best"])
    assert Ubest.shape == (50, 4)
    assert float(best) <= 1.01 * ref, (float(best), ref)
    prob.eval()
    rows, _ = na.baseline_report(fx("solve600/z0"), Ubest, prob, alph[0])
    assert float(rows[0]) <= 1.01 * float(FIX["solve600/report"][0])


@pytest.mark.parametrize("name,alph", [("softcorridor", [100.0, 1e4, 300.0]), ("swarm", [900.0, 1e7, 25000.0])])
def test_batch_of_64_equals_single_launches(name, alph):
    prob, xInit = make_prob(name, alph)
    prob.train()
    g = torch.Generator(device=DEV).manual_seed(7)
    z0 = xInit + 0.5 * torch.randn(64, xInit.numel(), device=DEV, generator=g)
    Ub, best, hist = na.solve_baseline(z0, prob, 20, niters=20, alphG=alph[0], generator=g, history=True)
    assert Ub.shape == (64, 20, xInit.numel()) and hist.shape == (64, 20) and bool(torch.isfinite(hist).all())
    U0 = Ub.clone()                                        # any fixed controls: re-solve from them, batched and one by one
    Ub, best, hist = na.solve_baseline(z0, prob, 20, niters=20, alphG=alph[0], U0=U0, history=True)
    J = na.baseline_loss(z0, U0, prob, alph[0])
    for i in range(64):
        u1, b1, h1 = na.solve_baseline(z0[i], prob, 20, niters=20, alphG=alph[0], U0=U0[i], history=True)
        assert torch.equal(u1, Ub[i]) and torch.equal(b1, best[i]) and torch.equal(h1, hist[i]), i
        assert torch.equal(na.baseline_loss(z0[i], U0[i], prob, alph[0]), J[i]), i


def test_split_solve_equals_one_launch():
    prob, xInit = make_prob("swap12", [300.0, 0.0, 1e5])
    prob.train()
    z0 = xInit.reshape(1, -1).repeat(3, 1)
    z0[1:] += 0.3
    U0 = na.baseline.initial_guess(z0, prob, 20, torch.Generator(device=DEV).manual_seed(3))

    def state():
        return [U0.clone(), torch.zeros_like(U0), torch.zeros_like(U0), torch.full((3,), float("inf"), device=DEV),
                torch.zeros_like(U0)]
    one = state()
    h1 = torch.empty(3, 40, device=DEV)
    na.baseline_adam_steps(z0, *one[:5], prob, 300.0, 40, hist=h1)
    two = state()
    ha, hb = torch.empty(3, 15, device=DEV), torch.empty(3, 25, device=DEV)
    na.baseline_adam_steps(z0, *two[:5], prob, 300.0, 15, step0=0, hist=ha)
    na.baseline_adam_steps(z0, *two[:5], prob, 300.0, 25, step0=15, hist=hb)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    assert torch.equal(h1, torch.cat([ha, hb], 1))


def test_driver_logs_table_and_resume(tmp_path, capsys):
    import baseline2D
    out = baseline2D.main(["--niters", "50", "--nt", "20", "--save", str(tmp_path), "--gpu", "0"])
    text = capsys.readouterr().out
    lines = text.splitlines()
    logs = [l for l in lines if re.match(r"^\d+ \S+$", l)]
    assert [int(l.split()[0]) for l in logs] == [0, 10, 20, 30, 40]
    hdr = [i for i, l in enumerate(lines) if l.split() == ["loss", "L", "G", "Q", "W"]]
    assert len(hdr) == 1 and len(lines[hdr[0] + 1].split()) == 5
    assert out["path"] and os.path.exists(out["path"])
    u = torch.load(out["path"])
    assert u.shape == (20, 4) and u.dtype == torch.float32
    back = baseline2D.main(["--nt", "20", "--resume", out["path"], "--gpu", "0"])
    assert torch.equal(back["rows"], out["rows"])
    assert back["path"] is None
