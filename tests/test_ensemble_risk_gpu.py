"""Risk-sensitive ensembles on the MI355X: member e of one weighted ensemble call against weighted_ocflow_train / risk_ocflow_train on that
member alone with its weights, sigma row, seed, mask and row offset -- bit for bit, at every adjoint instantiation of both families (cases:
tests/util_ensemble_risk.py).  The single-network weighted calls are unchanged by the ensemble work and tests/test_risk_gpu.py holds them to
the fp64 oracle, so every comparison against a member is torch.equal.  One line carries a tolerance, stated where it stands: the VALUE Jw at
w = 1/n against the mean ensemble_noisy_ocflow_train forms from the kernel's column sums (two summation orders; the gradients there are bits)."""
import glob
import os
import subprocess
import sys

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, ensemble, ensemble_noise

import util_ensemble_noise as uen
import util_ensemble_risk as uer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = uer.E
GJ = [1.0, 0.5, -2.0]
ENS_W = {"lane": "rollout_lane_bwd_kernel<ens,weighted>", "mid": "rollout_mono_bwd_kernel<ens,weighted>"}
ONE_W = {"lane": "rollout_lane_bwd_kernel<weighted>", "mid": "rollout_mono_bwd_kernel<weighted>"}
ENS_BWD = {"lane": "rollout_lane_bwd_kernel<ens>", "mid": "rollout_mono_bwd_kernel<ens>"}


def _kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def _setup(nc, members=E, x=None):
    u, case = nc.util, nc.case
    nets = u.member_nets(case, DEV, members)
    rows = u.member_rows(members)
    ens = na.PhiEnsemble.from_members(nets, alph=rows)
    x = (u.starts(case, members) if x is None else x).to(DEV)
    prob = u.member_problem(case, 0, DEV)                       # (its alph_Q / alph_W are not read by an ensemble call)
    return ens, rows, x, prob


def _noise_kw(nc):
    return dict(mask=nc.mask, row_offset=nc.row_offset, stepper=nc.base.stepper)


def _member_grads_equal(ens, net, e):
    for name, p in ens.named_parameters():
        q = dict(net.named_parameters())[name]
        assert p.grad is not None and q.grad is not None and torch.equal(p.grad[e], q.grad), (e, name)


def _given(nc, ens, x, prob, w, gJ=None, sigma=None, seed=None):
    """ensemble_weighted_ocflow_train + backward on fresh gradients -> (Jw, cs, x.grad, {name: grad})"""
    b = nc.base
    for p in ens.parameters():
        p.grad = None
    xe = x.clone().requires_grad_(True)
    Jw, cs = na.ensemble_weighted_ocflow_train(xe, ens, prob, b.tspan, b.nt, w, sigma=nc.sigma if sigma is None else sigma,
                                               seed=nc.seed if seed is None else seed, family=nc.family, **_noise_kw(nc))
    (Jw.sum() if gJ is None else (gJ * Jw).sum()).backward()
    assert _kernel() == ENS_W[nc.family]
    return Jw.detach(), cs, xe.grad, {name: p.grad.clone() for name, p in ens.named_parameters()}


# ---- 1. given weights, every adjoint instantiation of both families
@pytest.mark.parametrize("nc", uer.GIVEN, ids=lambda c: c.id)
def test_given_weights_members_equal_weighted_ocflow_train_on_the_member(nc):
    b = nc.base
    assert nc.own_x
    ens, rows, x, prob = _setup(nc)
    w = uer.weights(nc).to(DEV)
    Jw, cs, gx, _ = _given(nc, ens, x, prob, w)
    assert tuple(Jw.shape) == (E,) and tuple(cs.shape) == (E, 7) and not cs.requires_grad
    for e in range(E):
        net, pe = ens.member(e), nc.util.member_problem(nc.case, e, DEV)
        x1 = x[e].clone().requires_grad_(True)
        J1, c1 = na.weighted_ocflow_train(x1, net, pe, list(b.tspan), b.nt, w[e], sigma=uen.member_sigma(nc.sigma, e), seed=nc.member_seed(e),
                                          alph=rows[e], **_noise_kw(nc))
        J1.backward()
        assert _kernel() == ONE_W[nc.family]                    # the yardstick ran the single-network weighted kernel of the same family
        assert torch.equal(Jw[e], J1.detach()) and torch.equal(cs[e], torch.stack(c1)), e
        assert torch.equal(gx[e], x1.grad), e
        _member_grads_equal(ens, net, e)
    assert all(bool((p.grad[e] != 0).any()) for e in range(E) for _, p in ens.named_parameters())
    assert bool((gx[:, b.n // 2] == 0).all()) and bool((gx[:, 0] != 0).any())          # the row of weight 0 takes no gradient


# ---- 2. uniform weights: the unweighted ensemble's bits
@pytest.mark.parametrize("nc", [uen.first(uer.GIVEN, "lane", isigma=1), uen.first(uer.GIVEN, "mid", isigma=1)], ids=lambda c: c.id)
def test_uniform_weights_give_the_bits_of_the_noisy_ensemble(nc):
    b = nc.base
    ens, rows, x, prob = _setup(nc)
    gJ = torch.tensor(GJ, device=DEV)
    w = torch.full((E, b.n), 1.0 / b.n, dtype=torch.float32, device=DEV)               # (float)(1 / n): what the unweighted entry takes
    Jw, cs, gx, grads = _given(nc, ens, x, prob, w, gJ=gJ)
    for p in ens.parameters():
        p.grad = None
    xe = x.clone().requires_grad_(True)
    Jc, cs0 = na.ensemble_noisy_ocflow_train(xe, ens, prob, b.tspan, b.nt, nc.sigma, nc.seed, b.stepper, mask=nc.mask,
                                             row_offset=nc.row_offset, family=nc.family)
    (gJ * Jc).sum().backward()
    assert _kernel() == ENS_BWD[nc.family]
    assert torch.equal(cs, cs0) and torch.equal(gx, xe.grad)
    for name, p in ens.named_parameters():
        assert torch.equal(grads[name], p.grad), name
    # Jw = sum_i fl(1/n) J_i over the rows, Jc is formed from the kernel's column sums: two orders of at most 5 n <= 85 fp32 additions and
    # products of non-negative terms, so they agree to 85 * 2^-24 < 1e-5 relative (the gradients above are the bits)
    assert torch.allclose(Jw, Jc.detach(), rtol=1e-5, atol=0.0)


# ---- 3. the risks
@pytest.mark.parametrize("nc", uer.RISK, ids=lambda c: c.id)
def test_risk_members_equal_risk_ocflow_train_on_the_member(nc):
    b = nc.base
    n, paths = uer.RISK_N[nc.family], uer.PATHS
    ens, rows, x, prob = _setup(nc, x=uer.risk_starts(nc))
    assert tuple(x.shape) == (E, n, b.d)
    sigma, kw = uer.RISK_SIGMA, _noise_kw(nc)
    with torch.no_grad():                                       # the entropic member's theta, from its own costs: ensemble_noisy_rollout's launch
        nz = ensemble_noise._Noise(ensemble_noise.scale_table(sigma, E, b.nt, b.d, b.tspan, nc.mask), ensemble_noise.seed_list(nc.seed, E),
                                   nc.row_offset)
        launch = ensemble._launch if nc.family == "lane" else ensemble._launch_mid
        probe = launch(x, ens, prob, b.tspan, b.nt, b.stepper, None, noise=nz)["persample"].view(E, n, 7)
    specs = [(r_, uer.theta_of(probe[e], rows[e]) if lv is None else lv, mx) for e, (r_, lv, mx) in enumerate(uer.RISK_SPECS)]
    risks, levels, mixes = (list(t) for t in zip(*specs))
    assert 0 < levels[1] < float("inf")
    xe = x.clone().requires_grad_(True)
    Jr, cs, info = na.ensemble_risk_ocflow_train(xe, ens, prob, b.tspan, b.nt, risks, levels, paths=paths, mix=mixes, sigma=sigma,
                                                 seed=nc.seed, family=nc.family, **kw)
    assert tuple(Jr.shape) == (E,) and tuple(info["weights"].shape) == (E, n) and tuple(info["persample"].shape) == (E, n, 7)
    assert tuple(info["rho"].shape) == (E, n // paths)
    Jr.sum().backward()
    assert _kernel() == ENS_W[nc.family]
    for e in range(E):
        net, pe = ens.member(e), nc.util.member_problem(nc.case, e, DEV)
        x1 = x[e].clone().requires_grad_(True)
        J1, c1, i1 = na.risk_ocflow_train(x1, net, pe, list(b.tspan), b.nt, risks[e], levels[e], paths=paths, mix=mixes[e],
                                          sigma=uen.member_sigma(sigma, e), seed=nc.member_seed(e), alph=rows[e], **kw)
        J1.backward()
        assert _kernel() == ONE_W[nc.family]
        assert torch.equal(Jr[e].detach(), J1.detach()) and torch.equal(cs[e], torch.stack(c1)), e
        assert torch.equal(info["weights"][e], i1["weights"]) and torch.equal(info["rho"][e], i1["rho"]), e
        assert torch.equal(info["persample"][e], i1["persample"]), e
        assert torch.equal(xe.grad[e], x1.grad), e
        _member_grads_equal(ens, net, e)
    # member 0 is undisturbed: its paths tie, and the stable sort gives the tail to the first rows of every group
    w0 = info["weights"][0].reshape(-1, paths)
    assert torch.equal(info["persample"][0].reshape(-1, paths, 7)[:, 0], info["persample"][0].reshape(-1, paths, 7)[:, 2])
    assert bool((w0[:, 0] > w0[:, 1]).all()) and bool((w0[:, 1] > 0).all()) and bool((w0[:, 2] == 0).all())
    assert not torch.equal(info["persample"][1].reshape(-1, paths, 7)[:, 0], info["persample"][1].reshape(-1, paths, 7)[:, 2])


# ---- 4. the members do not interact
@pytest.mark.parametrize("nc", [uen.first(uer.GIVEN, "lane", isigma=0), uen.first(uer.GIVEN, "mid", isigma=0)], ids=lambda c: c.id)
def test_a_members_weights_reach_that_member_only(nc):
    ens, rows, x, prob = _setup(nc)
    w = uer.weights(nc).to(DEV)
    J0, cs0, gx0, g0 = _given(nc, ens, x, prob, w)
    w2 = w.clone()
    w2[1] *= 2.0
    J2, cs2, gx2, g2 = _given(nc, ens, x, prob, w2)
    assert torch.equal(cs2, cs0)
    for e in range(E):
        f = 2.0 if e == 1 else 1.0                             # (doubling is exact in every product and sum of the adjoint)
        assert torch.equal(J2[e], f * J0[e]) and torch.equal(gx2[e], f * gx0[e]), e
        for name in g0:
            assert torch.equal(g2[name][e], f * g0[name][e]), (e, name)
    gJ = torch.tensor(GJ, device=DEV)
    J3, cs3, gx3, g3 = _given(nc, ens, x, prob, w, gJ=gJ)
    assert torch.equal(J3, J0)
    for e in range(E):
        assert torch.equal(gx3[e], gJ[e] * gx0[e]), e
        for name in g0:
            assert torch.equal(g3[name][e], gJ[e] * g0[name][e]), (e, name)


# ---- 5. the capped one-CU grid
def test_capped_grid_walks_a_members_tiles_under_its_weights():
    nc = uer.CAPPED
    b = nc.base
    members = uer.CAPPED_E
    ens, rows, x, prob = _setup(nc, members=members)
    xs = x[0].contiguous()
    assert (b.n + 15) // 16 > 1024                              # more tiles per member than workgroups: tiles j, j + 1024
    w = uer.weights(nc, members).to(DEV)
    sigma, seed = [[0.05], [0.1]], uen.SEED_SHARED
    Jw, cs = na.ensemble_weighted_ocflow_train(xs, ens, prob, b.tspan, b.nt, w, sigma=sigma, seed=seed, stepper=b.stepper, family="mid")
    Jw.sum().backward()
    assert _kernel() == ENS_W["mid"]
    for e in range(members):
        net, pe = ens.member(e), nc.util.member_problem(nc.case, e, DEV)
        J1, c1 = na.weighted_ocflow_train(xs, net, pe, list(b.tspan), b.nt, w[e], sigma=sigma[e][0], seed=seed, stepper=b.stepper, alph=rows[e])
        J1.backward()
        assert _kernel() == ONE_W["mid"]
        assert torch.equal(Jw[e].detach(), J1.detach()) and torch.equal(cs[e], torch.stack(c1)), e
        _member_grads_equal(ens, net, e)


# ---- 6. the driver
def test_driver_members_risk(tmp_path):
    save = tmp_path / "out"
    argv = [sys.executable, os.path.join(REPO, "trainOC.py"), "--data", "softcorridor", "--m", "16", "--nt", "4", "--niters", "2", "--n_train", "32",
            "--val_freq", "2", "--seed", "5", "--members", "2", "--members_sigma", "0.05,0.1", "--members_risk", "cvar",
            "--members_risk_level", "0.5,0.8", "--members_risk_paths", "2", "--save", str(save)]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines()]
    its = [cols for cols in lines if len(cols) > 4 and cols[0] in ("m0", "m1") and cols[1].isdigit()]
    assert [(c[0], c[1]) for c in its] == [("m0", "00001"), ("m1", "00001"), ("m0", "00002"), ("m1", "00002")]
    assert all(float(c[4]) == float(c[4]) and abs(float(c[4])) < float("inf") for c in its)       # the loss column: each member's risk value
    assert len(glob.glob(str(save / "*_m0_checkpt.pth"))) == 1 and len(glob.glob(str(save / "*_m1_checkpt.pth"))) == 1
