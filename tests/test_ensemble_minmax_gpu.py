"""Adversarial ensembles on the MI355X: member e of one disturbed ensemble launch against the single-network call on that member alone with its
slice of W -- disturbed_rollout, minmax_ocflow_train + backward, disturbance_gradient, ascend_disturbances, worst_case_disturbances -- bit for
bit, at every instantiation of both families (cases: tests/util_ensemble_minmax.py).  Nothing here carries a tolerance: the kernels run the
single-network DIST == 1 / STATES statements on the member's blocks.  Every comparison is torch.equal."""
import glob
import os
import types

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, ensemble, ensemble_minmax as em

import util_ensemble_minmax as uea

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024
E = uea.E
ENS_FWD = {"lane": "rollout_lane_kernel<ens,disturbed>", "mid": "rollout_mono_kernel<ens,disturbed>"}
ONE_FWD = {"lane": "rollout_lane_kernel<dist>", "mid": "rollout_mono_kernel<dist>"}
ENS_JOINT = {"lane": "rollout_lane_bwd_kernel<ens,joint>", "mid": "rollout_mono_bwd_kernel<ens,joint>"}
ONE_JOINT = {"lane": "rollout_lane_bwd_kernel<joint>", "mid": "rollout_mono_bwd_kernel<joint>"}
ENS_STATES = {"lane": "rollout_lane_bwd_kernel<ens,states>", "mid": "rollout_mono_bwd_kernel<ens,states>"}
ONE_STATES = {"lane": "rollout_lane_bwd_kernel<states>", "mid": "rollout_mono_bwd_kernel<states>"}
ENS_BWD = {"lane": "rollout_lane_bwd_kernel<ens>", "mid": "rollout_mono_bwd_kernel<ens>"}


def _kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def _guarded(*shape):
    """a NaN-filled buffer with GUARD floats on either side of a tensor of `shape` -> (buffer, the view in the middle)"""
    count = 1
    for v in shape:
        count *= v
    buf = torch.full((count + 2 * GUARD,), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + count].view(*shape)


def _guards_intact(guards, bufs):
    for key, g in guards.items():
        mid = bufs[key].numel()
        assert bool(g[:GUARD].isnan().all()) and bool(g[GUARD + mid:].isnan().all()), key


def _setup(ac, members=E):
    u, case = ac.util, ac.case
    nets = u.member_nets(case, DEV, members)
    rows = u.member_rows(members)
    ens = na.PhiEnsemble.from_members(nets, alph=rows)
    x = u.starts(case, members).to(DEV)
    prob = u.member_problem(case, 0, DEV)                       # (its alph_Q / alph_W are not read by an ensemble call)
    return ens, rows, x, prob


def _member_x(ac, x, e):
    return (x[e] if ac.own_x else x[0]).contiguous()


def _cdim(b):
    return 4 * b.n_agents if getattr(b, "kind", "") == "quad" else b.d


def _launch(ac, xe, ens, prob, **kw):
    b = ac.base
    fn = ensemble._launch if ac.family == "lane" else ensemble._launch_mid
    return fn(xe, ens, prob, b.tspan, b.nt, b.stepper, None, **kw)


def _shapes(ac, record):
    b = ac.base
    n, d, nt = b.n, b.d, b.nt
    nstage = 4 if b.stepper == "rk4" else 1
    if ac.family == "lane":
        s = {"persample": (E * n, 7), "z_out": (E * n, d + 4), "sums": (E, 8)}
        s.update({"s_all": (nt * nstage, E * n, d + 1)} if record else
                 {"means": (E, 8), "zFull": (nt + 1, E * n, d + 4), "ctrlFull": (nt + 1, E * n, _cdim(b))})
    else:
        s = {"persample": (E, n, 7), "z_out": (E, n, d + 4), "sums": (E, 8)}
        s.update({"s_all": (E, nt * nstage, n, d + 1)} if record else
                 {"means": (E, 8), "zFull": (E, nt + 1, n, d + 4), "ctrlFull": (E, nt + 1, n, _cdim(b))})
    return s


# ---- 1. evaluation
@pytest.mark.parametrize("ac", uea.FORWARD, ids=lambda c: c.id)
def test_evaluation_members_equal_disturbed_rollout_on_the_member(ac):
    b = ac.base
    n, d, nt = b.n, b.d, b.nt
    ens, rows, x, prob = _setup(ac)
    xe = x if ac.own_x else x[0]
    W = uea.disturbance(ac).to(DEV)
    bufs, guards = {}, {}
    for key, shape in _shapes(ac, False).items():
        guards[key], bufs[key] = _guarded(*shape)
    with torch.no_grad():
        out = _launch(ac, xe, ens, prob, intermediates=True, bufs=bufs, dist=em._Disturbance(W, False))
        assert _kernel() == ENS_FWD[ac.family]
        Jc, cs = na.ensemble_disturbed_rollout(xe, ens, prob, b.tspan, nt, W, b.stepper, family=ac.family)
        assert _kernel() == ENS_FWD[ac.family]
        Jc2, cs2, traj, ctrl = na.ensemble_disturbed_rollout(xe, ens, prob, b.tspan, nt, W, b.stepper, intermediates=True, family=ac.family)
    torch.cuda.synchronize()
    _guards_intact(guards, bufs)                                # nothing outside the stated rows is written, every stated row is
    for key in guards:
        assert bool(torch.isfinite(out[key]).all()), key
    assert tuple(Jc.shape) == (E,) and tuple(cs.shape) == (E, 7)
    assert tuple(traj.shape) == (E, n, d + 4, nt + 1) and tuple(ctrl.shape) == (E, n, _cdim(b), nt + 1)
    assert torch.equal(Jc, out["means"][:, 7]) and torch.equal(cs, out["means"][:, :7]) and torch.equal(Jc2, Jc) and torch.equal(cs2, cs)
    tab = out["persample"].view(E, n, 7)
    for e in range(E):
        net, pe, x1 = ens.member(e), ac.util.member_problem(ac.case, e, DEV), _member_x(ac, x, e)
        with torch.no_grad():
            ref = na.disturbed_rollout(x1, net, pe, nt, W[e], tspan=b.tspan, alph=rows[e], stepper=b.stepper, intermediates=True)
            assert _kernel() == ONE_FWD[ac.family]              # the yardstick ran the single-network kernel of the same family
            plain = na.OCflow(x1, net, pe, list(b.tspan), nt, b.stepper, rows[e])
        assert torch.equal(Jc[e], ref["Jc"]) and torch.equal(cs[e], torch.stack(ref["cs"])), e
        assert torch.equal(tab[e], ref["persample"]), e
        assert torch.equal(traj[e], ref["traj"]) and torch.equal(ctrl[e], ref["ctrl"]), e
        assert not torch.equal(Jc[e], plain[0]), e              # (not vacuous: the disturbance moves the member)


# ---- 2. recording forward plus joint adjoint
@pytest.mark.parametrize("ac", uea.TRAIN, ids=lambda c: c.id)
def test_recording_forward_and_joint_adjoint_equal_minmax_ocflow_train_on_the_member(ac):
    b = ac.base
    n, d, nt = b.n, b.d, b.nt
    assert ac.own_x
    ens, rows, x, prob = _setup(ac)
    W = uea.disturbance(ac).to(DEV)
    gJ = torch.tensor(uea.GJ, device=DEV)
    # the recording launch into guarded buffers, then the joint adjoint with guards around lamW
    bufs, guards = {}, {}
    for key, shape in _shapes(ac, True).items():
        guards[key], bufs[key] = _guarded(*shape)
    out = _launch(ac, x, ens, prob, record=True, bufs=bufs, dist=em._Disturbance(W, False))
    assert _kernel() == ENS_FWD[ac.family]
    guards["lamW"], lamW = _guarded(E, nt, n, d)
    ctx = types.SimpleNamespace(saved_tensors=(out["s_all"], out["z_out"]), ens=ens, prob=prob, nt=nt, tspan=list(b.tspan), stepper=b.stepper,
                                table=out["table"], param_versions=[p._version for _, p in ens._params()], x_needs_grad=True,
                                act=out.get("act"))
    name = list(em._ADJOINT[ac.family])[0]
    em._base(ac.family)._adjoint(ctx, gJ, joint=(em._entries(_lib.lib())[name], name, lamW))
    assert _kernel() == ENS_JOINT[ac.family]
    torch.cuda.synchronize()
    _guards_intact(guards, dict(bufs, lamW=lamW))
    assert bool(torch.isfinite(lamW).all())
    # ... and the public call with its backward
    xe, We = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    Jc, cs = na.ensemble_minmax_ocflow_train(xe, ens, prob, b.tspan, nt, We, b.stepper, family=ac.family)
    assert _kernel() == ENS_FWD[ac.family]
    assert tuple(Jc.shape) == (E,) and tuple(cs.shape) == (E, 7) and Jc.requires_grad and not cs.requires_grad
    (gJ * Jc).sum().backward()
    assert _kernel() == ENS_JOINT[ac.family]
    assert tuple(We.grad.shape) == (E, nt, n, d) and torch.equal(We.grad, gJ.reshape(E, 1, 1, 1) * lamW)
    joint = {name: p.grad.clone() for name, p in ens.named_parameters()}
    for e in range(E):
        net, pe = ens.member(e), ac.util.member_problem(ac.case, e, DEV)
        x1, W1 = x[e].clone().requires_grad_(True), W[e].clone().requires_grad_(True)
        J1, c1 = na.minmax_ocflow_train(x1, net, pe, list(b.tspan), nt, W1, b.stepper, rows[e])
        assert _kernel() == ONE_FWD[ac.family]
        (gJ[e] * J1).backward()
        assert _kernel() == ONE_JOINT[ac.family]
        assert torch.equal(Jc[e].detach(), J1.detach()) and torch.equal(cs[e], torch.stack(c1)), e
        assert torch.equal(xe.grad[e], x1.grad), e
        assert torch.equal(We.grad[e], W1.grad) and bool((W1.grad != 0).any()), e
        for name, p in ens.named_parameters():
            assert torch.equal(joint[name][e], dict(net.named_parameters())[name].grad), (e, name)
    assert all(bool((g[e] != 0).any()) for e in range(E) for g in joint.values())
    # a W that takes no gradient: the call is ensemble_disturbed_ocflow_train (the existing ensemble adjoint)
    got = []
    for fn in (na.ensemble_minmax_ocflow_train, na.ensemble_disturbed_ocflow_train):
        ens.zero_grad()
        xg = x.clone().requires_grad_(True)
        J2, c2 = fn(xg, ens, prob, b.tspan, nt, W, b.stepper, family=ac.family)
        (gJ * J2).sum().backward()
        assert _kernel() == ENS_BWD[ac.family]
        got.append((J2.detach(), c2, xg.grad, {name: p.grad.clone() for name, p in ens.named_parameters()}))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and torch.equal(got[0][2], got[1][2])
    assert all(torch.equal(got[0][3][name], got[1][3][name]) for name in joint)
    assert torch.equal(got[0][0], Jc.detach())


# ---- 3. state-only adjoint
@pytest.mark.parametrize("ac", uea.TRAIN, ids=lambda c: c.id)
def test_disturbance_gradient_members_equal_disturbance_gradient_on_the_member(ac):
    b = ac.base
    n, d, nt = b.n, b.d, b.nt
    ens, rows, x, prob = _setup(ac)
    W = uea.disturbance(ac).to(DEV)
    for objective in ("Jc", "control"):
        got = na.ensemble_disturbance_gradient(x, ens, prob, nt, W, tspan=b.tspan, stepper=b.stepper, objective=objective, want_dx=True,
                                               family=ac.family)
        assert got["forward_kernel"] == ENS_FWD[ac.family] and got["adjoint_kernel"] == ENS_STATES[ac.family] == _kernel()
        assert tuple(got["dW"].shape) == (E, nt, n, d) and tuple(got["dx"].shape) == (E, n, d) and tuple(got["persample"].shape) == (E, n, 7)
        assert tuple(got["Jc"].shape) == (E,) and tuple(got["cs"].shape) == (E, 7)
        for e in range(E):
            net, pe = ens.member(e), ac.util.member_problem(ac.case, e, DEV)
            want = na.disturbance_gradient(x[e].contiguous(), net, pe, nt, W[e], tspan=b.tspan, alph=rows[e], stepper=b.stepper,
                                           objective=objective, want_dx=True)
            assert want["forward_kernel"] == ONE_FWD[ac.family] and want["adjoint_kernel"] == ONE_STATES[ac.family]
            assert torch.equal(got["dW"][e], want["dW"]) and bool((want["dW"] != 0).any()), (objective, e)
            assert torch.equal(got["dx"][e], want["dx"]), (objective, e)
            assert torch.equal(got["persample"][e], want["persample"]), (objective, e)
            assert torch.equal(got["Jc"][e], want["Jc"]) and torch.equal(got["cs"][e], torch.stack(want["cs"])), (objective, e)


def test_the_state_only_entry_keeps_its_guards():
    """lam0 and lamW of the state-only ensemble adjoints in NaN guard bands: only the stated rows are written, all of them"""
    for ac in (uea.first(uea.TRAIN, "lane"), uea.first(uea.TRAIN, "mid")):
        b = ac.base
        n, d, nt = b.n, b.d, b.nt
        ens, rows, x, prob = _setup(ac)
        W = uea.disturbance(ac).to(DEV)
        with torch.no_grad():
            s = em._Search(x, ens, prob, nt, b.tspan, None, b.stepper, "Jc", 1.0 / n, True, ac.family)
            g_dW, s.dW = _guarded(E, nt, n, d)
            g_dx, s.dx = _guarded(E, n, d)
            s.gradient(W)
        torch.cuda.synchronize()
        _guards_intact({"dW": g_dW, "dx": g_dx}, {"dW": s.dW, "dx": s.dx})
        assert bool(torch.isfinite(s.dW).all()) and bool(torch.isfinite(s.dx).all())


# ---- 4. ascent
@pytest.mark.parametrize("nt, n, d, masked", [(2, 5, 4, False), (3, 5, 7, True), (10, 6, 9, True)])
def test_ascent_members_equal_ascend_disturbances_on_a_copy(nt, n, d, masked):
    members = 4
    gen = torch.Generator().manual_seed(17 * nt + d)
    W0 = (0.05 * torch.randn(members, nt, n, d, generator=gen)).to(DEV)
    g = torch.randn(members, nt, n, d, generator=gen).to(DEV)
    g[3] = 0.0                                                  # member 3: no direction, its rows are untouched
    eps = [0.0, 0.05, 10.0, 0.3]                                # member 0: radius 0; member 1: the step leaves the ball; member 2: it stays inside
    step = [0.1, 0.2, 0.1, 0.1]
    mask = uea.mask_of(d) if masked else None
    guard, W = _guarded(members, nt, n, d)
    W.copy_(W0)
    ret = na.ensemble_ascend_disturbances(W, g, eps, step, mask)
    assert ret is W
    torch.cuda.synchronize()
    _guards_intact({"W": guard}, {"W": W})
    for e in range(members):
        one = W0[e].clone()
        na.ascend_disturbances(one, g[e].contiguous(), eps[e], step[e], mask)
        assert torch.equal(W[e], one), e
    norms = W.permute(0, 2, 1, 3).reshape(members, n, nt * d).norm(dim=2)
    assert bool((W[0] == 0).all())
    assert bool((norms[1] <= 0.05 * (1 + 1e-6)).all()) and bool((norms[1] >= 0.05 * (1 - 1e-6)).all())      # on the sphere: it was projected
    assert bool((norms[2] < 10.0).all()) and not torch.equal(W[2], W0[2])
    assert torch.equal(W[3], W0[3])
    if masked:                                                  # inside the ball nothing is scaled: masked components keep their bits
        off = [i for i, v in enumerate(mask) if v == 0.0]
        assert torch.equal(W[2][:, :, off], W0[2][:, :, off]) and not torch.equal(W[2], W0[2])
    # a float stands for every member
    W2 = W0.clone()
    na.ensemble_ascend_disturbances(W2, g, 0.3, 0.1, mask)
    for e in range(members):
        one = W0[e].clone()
        na.ascend_disturbances(one, g[e].contiguous(), 0.3, 0.1, mask)
        assert torch.equal(W2[e], one), e
    with pytest.raises(RuntimeError, match="no_grad"):
        na.ensemble_ascend_disturbances(W0.clone().requires_grad_(True), g, eps, step, mask)


# ---- 5. search
@pytest.mark.parametrize("ac", [uea.first(uea.TRAIN, "lane", masked=True), uea.first(uea.TRAIN, "mid", masked=False)], ids=lambda c: c.id)
def test_search_members_equal_worst_case_disturbances_on_the_member(ac):
    b = ac.base
    n, d, nt = b.n, b.d, b.nt
    ens, rows, x, prob = _setup(ac)
    kw = dict(steps=3, tspan=b.tspan, stepper=b.stepper, mask=ac.mask)
    got = na.ensemble_worst_case_disturbances(x, ens, prob, nt, uea.EPS, family=ac.family, **kw)
    assert got["forward_kernel"] == ENS_FWD[ac.family] and got["adjoint_kernel"] == ENS_STATES[ac.family]
    assert tuple(got["W"].shape) == (E, nt, n, d) and tuple(got["history"].shape) == (4, E, n)
    assert tuple(got["objective"].shape) == (E, n) == tuple(got["nominal"].shape) and tuple(got["persample"].shape) == (E, n, 7)
    for e in range(E):
        net, pe = ens.member(e), ac.util.member_problem(ac.case, e, DEV)
        want = na.worst_case_disturbances(x[e].contiguous(), net, pe, nt, uea.EPS[e], alph=rows[e], **kw)
        assert want["forward_kernel"] == ONE_FWD[ac.family] and want["adjoint_kernel"] == ONE_STATES[ac.family]
        assert torch.equal(got["W"][e], want["W"]), e
        assert torch.equal(got["objective"][e], want["objective"]) and torch.equal(got["nominal"][e], want["nominal"]), e
        assert torch.equal(got["history"][:, e], want["history"]) and torch.equal(got["persample"][e], want["persample"]), e
    assert uea.EPS[0] == 0.0 and torch.equal(got["objective"][0], got["nominal"][0]) and bool((got["W"][0] == 0).all())
    assert bool((got["objective"][2] > got["nominal"][2]).any())                            # (not vacuous: the largest ball hurts)


# ---- 6. shared W, and the members' slices
@pytest.mark.parametrize("ac", [uea.first(uea.FORWARD, "lane", own_x=True), uea.first(uea.FORWARD, "mid", own_x=False)], ids=lambda c: c.id)
def test_a_shared_disturbance_and_swapped_slices(ac):
    b = ac.base
    n, nt = b.n, b.nt
    ens, rows, x, prob = _setup(ac)
    xe = x if ac.own_x else x[0]
    W = uea.disturbance(ac).to(DEV)
    swapped = W.clone()
    swapped[0], swapped[2] = W[2], W[0]
    with torch.no_grad():
        shared = na.ensemble_disturbed_rollout(xe, ens, prob, b.tspan, nt, W[1].contiguous(), b.stepper, intermediates=True, family=ac.family)
        assert _kernel() == ENS_FWD[ac.family]
        own = na.ensemble_disturbed_rollout(xe, ens, prob, b.tspan, nt, W, b.stepper, intermediates=True, family=ac.family)
        swp = na.ensemble_disturbed_rollout(xe, ens, prob, b.tspan, nt, swapped, b.stepper, intermediates=True, family=ac.family)
        for e in range(E):
            net, pe, x1 = ens.member(e), ac.util.member_problem(ac.case, e, DEV), _member_x(ac, x, e)
            for got, We in ((shared, W[1]), (swp, swapped[e])):
                ref = na.disturbed_rollout(x1, net, pe, nt, We.contiguous(), tspan=b.tspan, alph=rows[e], stepper=b.stepper, intermediates=True)
                assert torch.equal(got[0][e], ref["Jc"]) and torch.equal(got[1][e], torch.stack(ref["cs"])), e
                assert torch.equal(got[2][e], ref["traj"]) and torch.equal(got[3][e], ref["ctrl"]), e
    for k in range(4):                                          # member 1 kept its slice: nothing of it moved; members 0 and 2 did
        assert torch.equal(own[k][1], swp[k][1]) and torch.equal(own[k][1], shared[k][1])
    assert not torch.equal(own[0][0], swp[0][0]) and not torch.equal(own[0][2], swp[0][2])


# ---- 7. the driver
def _run_driver(argv, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("trainOC_under_test", os.path.join(REPO, "trainOC.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    capsys.readouterr()
    mod.main(argv)
    lines = [ln.split() for ln in capsys.readouterr().out.splitlines()]
    # the members' iteration lines without their wall-clock column
    return [cols[:3] + cols[4:] for cols in lines if len(cols) > 4 and cols[0] in ("m0", "m1", "m2") and cols[1].isdigit()]


@pytest.mark.parametrize("family, common", [
    ("lane", ["--data", "softcorridor", "--m", "16"]),
    ("mid", ["--data", "singlequad", "--m", "64", "--members_family", "mid"]),
])
def test_driver_members_adv(family, common, tmp_path, capsys):
    common = common + ["--nt", "4", "--niters", "3", "--n_train", "32", "--val_freq", "3", "--seed", "5", "--members", "3"]
    adv = _run_driver(common + ["--members_adv", "0,0.1,0.2", "--save", str(tmp_path / "adv")], capsys)
    assert _kernel() == ENS_FWD[family].replace(",disturbed", "")                           # (the last launch: the undisturbed validation)
    plain = _run_driver(common + ["--save", str(tmp_path / "plain")], capsys)
    assert len(adv) == 9 and len(plain) == 9                    # three members, three iterations: one line each
    assert [ln[0] for ln in adv[:3]] == ["m0", "m1", "m2"]
    assert len(glob.glob(str(tmp_path / "adv" / "*_m[012]_checkpt.pth"))) == 3
    # iteration 1 runs at W = 0 for every member; from iteration 2 on the members with a budget meet their adversary, member 0 never does
    assert adv[:3] == plain[:3]
    assert [ln for ln in adv if ln[0] == "m0"] == [ln for ln in plain if ln[0] == "m0"]
    assert [ln for ln in adv[3:] if ln[0] != "m0"] != [ln for ln in plain[3:] if ln[0] != "m0"]
