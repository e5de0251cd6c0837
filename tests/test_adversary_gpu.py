"""GPU: dJ/dW from the state-only adjoint (neuraloc_amd.disturbance_gradient, nocf_rollout_bwd_states_f32) against fp64 autograd of the
restated oracle with W as a leaf (tests/util_adversary.py) on every case of util_disturb.CASES under util_oracle's rule, for both
objectives; the entry point's bounds, nullable outputs and workspace at the C ABI; agreement with the full adjoint; shards with n_total;
nocf_disturbance_ascent_f32 against its formulas; the worst-case search against its fp64 restatement; evalOC.py --worst."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, adversary, train
import util_adversary as ua
import util_disturb as ud
import util_disturb_train as ut
import util_hip
import util_lane as ul
import util_mono as um
import util_oracle as uo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(res, what):
    for k, v in res.items():
        print(f"{what} {k}: err {v[1]:.3e} tol {v[2]:.3e} fp32 restatement {v[3]:.3e}")
    assert not ua.failures(res), (what, ua.failures(res))


def _gradient(case, x, W, objective, n_total=None):
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    out = na.disturbance_gradient(x.to(DEV), net, prob, case.nt, W.to(DEV), tspan=case.tspan, alph=case.alph, stepper=case.stepper,
                                  n_total=n_total, objective=objective, want_dx=True)
    torch.cuda.synchronize()
    na.check_errors(sync=True)
    return out


@pytest.mark.parametrize("objective", ua.OBJECTIVES)
@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
def test_dW_against_fp64_autograd(fc, objective):
    family, case = fc
    data = ud.case_data(case)
    out = _gradient(case, data["x"], data["W"], objective)
    assert out["forward_kernel"] == ud.KERNEL[family] and out["adjoint_kernel"] == ua.BWD_KERNEL[family], (out["forward_kernel"], out["adjoint_kernel"])
    r64, r32 = ua.case_grads(case, torch.float64, objective), ua.case_grads(case, torch.float32, objective)
    assert out["dW"].shape == data["W"].shape and out["dx"].shape == data["x"].shape
    _check({"dW": uo.compare(out["dW"], r64["dW"], r32["dW"]), "dx": uo.compare(out["dx"], r64["dx"], r32["dx"])}, f"{case.id} {objective}")
    f64, f32 = ul._summary(case, dict(table=data["r64"]["table"])), ul._summary(case, dict(table=data["r32"]["table"]))
    got = dict(Jc=out["Jc"].cpu(), cs=torch.stack(list(out["cs"])).cpu(), table=out["persample"].cpu())
    _check(ul.compare_forward(got, f64, f32), f"{case.id} forward")


ABI_CASES = [ud.CASES[0], ud.CASES[1], ud.CASES[3], ud.CASES[4], ud.CASES[5], ud.CASES[7]]          # n = 5, 7, 17, 33, 17, 16
POISONED = {ud.CASES[1][1].id, ud.CASES[3][1].id, ud.CASES[5][1].id, ud.CASES[7][1].id}
GUARD = 1024


def _guarded(count):
    """a NaN-filled buffer with GUARD floats on either side of `count` floats -> (buffer, the view in the middle)"""
    buf = torch.full((count + 2 * GUARD,), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + count]


@pytest.mark.parametrize("fc", ABI_CASES, ids=ud.case_id)
def test_states_entry_at_the_abi(fc):
    """lamW and lam0 sit inside larger NaN-filled buffers: every [k < nt, row < n, i < d] is finite afterwards and every guard float still
    NaN; either output alone gives the same bits; a NaN-filled workspace (the entry packs what it reads) changes nothing"""
    family, case = fc
    data = ud.case_data(case)
    n, d, nt, m = case.n, case.d, case.nt, case.m
    if case.id in POISONED:
        util_hip.poison_allocator(torch.device(DEV), big=1)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x, W = data["x"].to(DEV), data["W"].to(DEV)
    E = nt * (4 if case.stepper == "rk4" else 1)
    L = _lib.lib()
    rec_f, st_f, _ = adversary._entries(L)
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(x.device)
    nan = float("nan")
    s_all, z = torch.full((E, n, d + 1), nan, device=DEV), torch.full((n, d + 4), nan, device=DEV)
    tab, sums = torch.full((n, 7), nan, device=DEV), torch.full((8,), nan, device=DEV)
    nact = int(L.nocf_activation_record_floats(d, m, case.nTh, n, nt, train._STEPPERS[case.stepper])) if family == "mono" else 0
    act = torch.full((nact,), nan, device=DEV) if nact else None
    rec = C.c_int32(-1)
    alph_c = (C.c_float * 6)(*case.alph)
    hs = train._step_sizes(case.tspan, nt).to(DEV)
    with torch.cuda.device(x.device):
        rc = rec_f(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), _lib.ptr(W), n, float(case.tspan[0]), float(case.tspan[1]), nt,
                   train._STEPPERS[case.stepper], alph_c, _lib.ptr(z), _lib.ptr(tab), _lib.ptr(sums), _lib.ptr(s_all), _lib.ptr(act),
                   C.byref(rec), _lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == 0 and L.nocf_last_rollout_kernel().decode() == ud.KERNEL[family]

    def states(lam0, lamW, use_act=True):
        if case.id in POISONED:
            ws.fill_(255)                                            # every float of the workspace a NaN: the entry packs what it reads
        with torch.cuda.device(x.device):
            rc = st_f(C.byref(phi_st), C.byref(prob_st), n, nt, train._STEPPERS[case.stepper], float(case.tspan[1]), alph_c, 1.0 / n,
                      _lib.ptr(s_all), _lib.ptr(z), _lib.ptr(hs), _lib.ptr(act if (use_act and rec.value) else None),
                      _lib.ptr(lam0), _lib.ptr(lamW), _lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_ptr(x.device))
        torch.cuda.synchronize()
        assert rc == 0 and L.nocf_last_rollout_kernel().decode() == ua.BWD_KERNEL[family]

    bufW, lamW = _guarded(nt * n * d)
    buf0, lam0 = _guarded(n * d)
    states(lam0, lamW)
    for buf, mid in ((bufW, lamW), (buf0, lam0)):
        assert bool(torch.isfinite(mid).all())
        assert bool(buf[:GUARD].isnan().all()) and bool(buf[GUARD + mid.numel():].isnan().all())
    r64, r32 = ua.case_grads(case, torch.float64), ua.case_grads(case, torch.float32)
    _check({"lamW": uo.compare(lamW.view(nt, n, d), r64["dW"], r32["dW"]), "lam0": uo.compare(lam0.view(n, d), r64["dx"], r32["dx"])}, case.id)
    bufW2, lamW2 = _guarded(nt * n * d)
    states(None, lamW2)
    assert torch.equal(lamW2, lamW) and bool(bufW2[:GUARD].isnan().all()) and bool(bufW2[GUARD + lamW2.numel():].isnan().all())
    buf02, lam02 = _guarded(n * d)
    states(lam02, None)
    assert torch.equal(lam02, lam0) and bool(buf02[:GUARD].isnan().all()) and bool(buf02[GUARD + lam02.numel():].isnan().all())
    if rec.value:                                                    # without the activation record the one-CU kernel recomputes: the rule again
        bufW3, lamW3 = _guarded(nt * n * d)
        states(None, lamW3, use_act=False)
        _check({"lamW (no record)": uo.compare(lamW3.view(nt, n, d), r64["dW"], r32["dW"])}, case.id)


AGREE_CASES = [ud.CASES[1], ud.CASES[3], ud.CASES[5], ud.CASES[7]]


@pytest.mark.parametrize("fc", AGREE_CASES, ids=ud.case_id)
def test_full_and_state_only_adjoints_agree(fc):
    """dx of the state-only call and x.grad of disturbed_ocflow_train on the same inputs both pass the rule against fp64"""
    family, case = fc
    data = ud.case_data(case)
    out = _gradient(case, data["x"], data["W"], "Jc")
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    xx = data["x"].to(DEV).clone().requires_grad_(True)
    Jc, _ = na.disturbed_ocflow_train(xx, net, prob, list(case.tspan), case.nt, data["W"].to(DEV), case.stepper, case.alph)
    Jc.backward()
    torch.cuda.synchronize()
    r64, r32 = ut.case_grads(case, torch.float64), ut.case_grads(case, torch.float32)
    _check({"states dx": uo.compare(out["dx"], r64["gx"], r32["gx"]), "full x.grad": uo.compare(xx.grad, r64["gx"], r32["gx"])}, case.id)
    a64 = ua.case_grads(case, torch.float64)
    assert torch.equal(a64["dx"], r64["gx"])                         # (the two fp64 references are one)


def test_shards_with_n_total():
    family, case = ud.CASES[3]
    data = ud.case_data(case)
    n = case.n
    parts = [_gradient(case, data["x"][sl], data["W"][:, sl].contiguous(), "Jc", n_total=n) for sl in (slice(0, 8), slice(8, n))]
    for p in parts:
        assert p["adjoint_kernel"] == ua.BWD_KERNEL[family]
    dW = torch.cat([p["dW"] for p in parts], 1)
    dx = torch.cat([p["dx"] for p in parts], 0)
    r64, r32 = ua.case_grads(case, torch.float64), ua.case_grads(case, torch.float32)
    _check({"dW": uo.compare(dW, r64["dW"], r32["dW"]), "dx": uo.compare(dx, r64["dx"], r32["dx"])}, case.id + " (two shards)")


@pytest.mark.parametrize("d", [2, 12, 150])
@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("n", [1, 5, 67])
def test_ascent_step_against_its_formulas(n, nt, d):
    """nocf_disturbance_ascent_f32 against torch fp64, with and without a mask.  Row 0 (n >= 5): all-zero gradient, unchanged bit for bit;
    row 1: already outside the ball; row 2: inside and stays inside (a short step), so not projected.  Per-element tolerance
    (nt d + 16) 2^-23 max(eps, |W|_inf): an fp32 sum of nt d squares and a handful of roundings.  Two runs are bitwise equal."""
    gen = torch.Generator().manual_seed(1000 * n + 10 * nt + d)
    eps, step = 1.5, 0.25
    W = torch.randn(nt, n, d, generator=gen)
    W = W * (0.9 * eps / W.pow(2).sum((0, 2)).sqrt())[None, :, None]                # every row at 0.9 eps: a step of 0.25 may leave the ball
    g = torch.randn(nt, n, d, generator=gen) * 37.0
    if n >= 5:
        g[:, 0] = 0.0
        W[:, 1] *= 3.0                                                              # outside
        W[:, 2] *= 0.2                                                              # 0.18 eps + 0.25 < eps: stays inside
    asc = adversary._entries(_lib.lib())[2]
    for mask in (None, (torch.arange(d) % 2 == 0).float()):
        want = ua.ascent_reference(W, g, mask, step, eps)
        runs = []
        for _ in range(2):
            Wd, gd = W.to(DEV).clone(), g.to(DEV)
            md = None if mask is None else mask.to(DEV)
            with torch.cuda.device(Wd.device):
                rc = asc(_lib.ptr(Wd), _lib.ptr(gd), _lib.ptr(md), n, nt, d, step, eps, _lib.stream_ptr(Wd.device))
            torch.cuda.synchronize()
            assert rc == 0 and torch.equal(gd.cpu(), g)
            runs.append(Wd.cpu())
        got = runs[0]
        assert torch.equal(runs[0], runs[1])
        tol = (nt * d + 16) * 2.0 ** -23 * max(eps, float(W.abs().max()))
        err = float((got.double() - want).abs().max())
        print(f"n {n} nt {nt} d {d} mask {mask is not None}: err {err:.3e} tol {tol:.3e}")
        assert err <= tol
        norms = got.double().pow(2).sum((0, 2)).sqrt()
        if n >= 5:
            assert torch.equal(got[:, 0], W[:, 0])
            assert abs(float(norms[1]) - eps) <= tol * (nt * d) ** 0.5 and float(norms[2]) < eps * 0.5
            assert float((got[:, 2].double() - (W[:, 2].double() + step * (g[:, 2].double() * (1 if mask is None else mask.double()))
                                                / (g[:, 2].double() * (1 if mask is None else mask.double())).norm())).abs().max()) <= tol
        if mask is not None and n >= 5:                                 # masked components of a row that is not projected keep their bits
            assert torch.equal(got[:, 2][:, mask == 0], W[:, 2][:, mask == 0])


SEARCH_CASES = [ud.CASES[0], ud.CASES[3], ud.CASES[5], ud.CASES[7]]
SEARCH_STEPS = 3
_SEARCH = {}


def _search_refs(case):
    """the search restated on the CPU in fp64 and fp32 (the rule's own error), once per case"""
    if case not in _SEARCH:
        data = ud.case_data(case)
        eps = ua.median_path_norm(data["W"])
        _SEARCH[case] = (eps, ua.search(case, torch.float64, data["x"], eps, SEARCH_STEPS), ua.search(case, torch.float32, data["x"], eps, SEARCH_STEPS))
    return _SEARCH[case]


@pytest.mark.parametrize("fc", SEARCH_CASES, ids=ud.case_id)
def test_worst_case_search(fc):
    family, case = fc
    data = ud.case_data(case)
    eps, s64, s32 = _search_refs(case)
    n = case.n
    bad = s64["bad"]
    print(f"{case.id}: eps {eps:.4f}, the screen drops {int(bad.sum())} of {n} rows")
    assert 8 * int(bad.sum()) <= n
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x = data["x"].to(DEV)
    kw = dict(steps=SEARCH_STEPS, tspan=case.tspan, alph=case.alph, stepper=case.stepper, objective="control")
    res = na.worst_case_disturbances(x, net, prob, case.nt, eps, **kw)
    torch.cuda.synchronize()
    na.check_errors(sync=True)
    assert res["forward_kernel"] == ud.KERNEL[family] and res["adjoint_kernel"] == ua.BWD_KERNEL[family]
    assert res["W"].shape == data["W"].shape and res["history"].shape == (SEARCH_STEPS + 1, n)
    assert bool((res["objective"] >= res["nominal"]).all())
    assert torch.equal(res["nominal"], res["history"][0]) and torch.equal(res["objective"], res["history"].max(0).values)
    norms = res["W"].double().pow(2).sum((0, 2)).sqrt()
    assert bool((norms <= eps * (1 + 1e-5)).all()), float(norms.max())
    a = ua.objective_alph(case.alph, "control")
    tab = res["persample"]
    assert torch.equal(res["objective"], tab[:, 0] + a[0] * tab[:, 1] + a[3] * tab[:, 2] + a[4] * tab[:, 3] + a[5] * tab[:, 4])
    # persample is the disturbed rollout at the returned W: both against the restatement at that W
    with torch.no_grad():
        fresh = na.disturbed_rollout(x, net, prob, case.nt, res["W"], tspan=case.tspan, alph=case.alph, stepper=case.stepper)
    Wc = res["W"].cpu()
    r64, r32 = ud.case_restate(case, data["x"], Wc, torch.float64), ud.case_restate(case, data["x"], Wc, torch.float32)
    keep = ~(bad | um.near_edge(case, r64["stages"]))
    assert 8 * int((~keep).sum()) <= n
    r64k, r32k = {k: v[keep] for k, v in r64.items()}, {k: v[keep] for k, v in r32.items()}
    _check(ud.compare(dict(table=tab.cpu()[keep]), r64k, r32k), case.id + " persample")
    _check(ud.compare(dict(table=fresh["persample"].cpu()[keep]), r64k, r32k), case.id + " fresh rollout")
    # the objective reached against the same search in fp64
    _check({"objective": uo.compare(res["objective"].cpu()[~bad], s64["objective"][~bad], s32["objective"][~bad]),
            "nominal": uo.compare(res["nominal"].cpu()[~bad], s64["nominal"][~bad], s32["nominal"][~bad])}, case.id)
    assert bool((s64["objective"] > s64["nominal"]).all())           # the fp64 search gains on every start
    res2 = na.worst_case_disturbances(x, net, prob, case.nt, eps, **kw)
    torch.cuda.synchronize()
    assert torch.equal(res2["W"], res["W"]) and torch.equal(res2["objective"], res["objective"])


def test_search_from_a_start_and_with_a_mask():
    """W0 is not modified and is the nominal iterate; masked components of the returned W keep W0's values (here 0)"""
    family, case = ud.CASES[0]
    data = ud.case_data(case)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x = data["x"].to(DEV)
    eps = ua.median_path_norm(data["W"])
    mask = torch.tensor([1.0, 0.0, 1.0, 0.0])
    res = na.worst_case_disturbances(x, net, prob, case.nt, eps, steps=2, tspan=case.tspan, alph=case.alph, stepper=case.stepper, mask=mask)
    assert bool((res["W"][:, :, 1] == 0).all()) and bool((res["W"][:, :, 3] == 0).all()) and bool((res["W"][:, :, 0] != 0).any())
    W0 = (0.5 * data["W"]).to(DEV)
    keep = W0.clone()
    res = na.worst_case_disturbances(x, net, prob, case.nt, 10.0 * eps, steps=1, tspan=case.tspan, alph=case.alph, stepper=case.stepper, W0=W0)
    torch.cuda.synchronize()
    assert torch.equal(W0, keep)
    with torch.no_grad():
        nom = na.disturbed_rollout(x, net, prob, case.nt, W0, tspan=case.tspan, alph=case.alph, stepper=case.stepper)["persample"]
    a = case.alph
    want = nom[:, 0] + a[0] * nom[:, 1]
    assert float((res["nominal"] - want).abs().max()) <= 1e-5 * float(want.abs().max())
    res0 = na.worst_case_disturbances(x, net, prob, case.nt, eps, steps=0, tspan=case.tspan, alph=case.alph, stepper=case.stepper)
    assert bool((res0["W"] == 0).all()) and torch.equal(res0["objective"], res0["nominal"])


def test_evalOC_worst_flag(tmp_path, capsys):
    """evalOC.py --worst on the checkpoint tests/test_disturb_gpu.py builds for --noise"""
    import evalOC
    from neuraloc_amd.checkpoint import save_checkpoint
    from conftest import load_golden
    g = load_golden("softcorridor")
    m = g.meta
    net = na.Phi(nTh=m["nTh"], m=m["m"], d=m["d"], alph=m["alph"])
    net.load_state_dict(g.state_dict())
    ck = os.path.join(str(tmp_path), "softcorridor_nn_checkpt.pth")
    save_checkpoint(ck, net, argparse.Namespace(data="softcorridor", m=m["m"], nTh=m["nTh"], alph=m["alph"], n_train=64, var0=1.0))
    save = os.path.join(str(tmp_path), "eval")
    nt = int(g["xinit_eval/nt"])
    out = evalOC.main(["--resume", ck, "--nt", str(nt), "--save", save, "--batch", "16", "--worst", "0.5", "--worst_steps", "2"])
    text = capsys.readouterr().out
    lines = [ln for ln in text.splitlines() if ln.startswith("worst ")]
    assert [ln.split()[1] for ln in lines[1:]] == ["L+G", "G", "Q", "W"], lines
    z = np.load(os.path.join(save, "figs", "eval_softcorridor_nn_worst.npz"))
    assert z["W"].shape == (nt, 1, m["d"]) and np.isfinite(z["W"]).all() and z["history"].shape == (3, 1)
    assert float(np.sqrt((z["W"].astype(np.float64) ** 2).sum())) <= 0.5 * (1 + 1e-5)
    assert out["worst"]["L+G"]["worst"] >= out["worst"]["L+G"]["nominal"]
    assert abs(out["worst"]["L+G"]["nominal"] - (out["cs"][0] + m["alph"][0] * out["cs"][1])) <= 1e-4 * abs(out["worst"]["L+G"]["nominal"])
    want_J = float(g["xinit_eval/Jc"])
    assert abs(out["Jc"] - want_J) <= 1e-4 * abs(want_J)
    save2 = os.path.join(str(tmp_path), "eval2")
    with pytest.raises(SystemExit, match="single precision"):
        evalOC.main(["--resume", ck, "--nt", str(nt), "--save", save2, "--batch", "16", "--prec", "double", "--worst", "0.5"])
    assert not os.path.exists(save2) and "loading model" not in capsys.readouterr().out
