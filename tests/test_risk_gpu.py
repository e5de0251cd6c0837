"""GPU: risk-sensitive training (neuraloc_amd.weighted_ocflow_train / risk_ocflow_train, nocf_rollout_bwd_small_rw_f32 / _mid_rw_f32 /
_act_rw_f32).  Gradients under given weights against fp64 autograd of the restated oracle (tests/util_risk.py) on every case of
util_disturb.CASES under util_oracle's rule; the weighted entries at w = 1/n against the existing call bit for bit at every lane and one-CU
adjoint instantiation and on the per-tile cases; row independence; the risks' weights, value and gradient from the device against the fp64
autograd of the value itself; the noisy path against the tensor path bit for bit; trainOC.py --risk."""
import os

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib
import util_disturb as ud
import util_lane as ul
import util_mono as um
import util_oracle as uo
import util_risk as ur

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FULL_KERNEL = {"lane": "rollout_lane_bwd_kernel", "mono": "rollout_mono_bwd_kernel", "tile": "rollout_bwd_kernel", "tile-fixed": "rollout_bwd_kernel"}


def last_kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def _check(res, what):
    for k, v in res.items():
        print(f"{what} {k}: err {v[1]:.3e} tol {v[2]:.3e} fp32 restatement {v[3]:.3e}")
    assert not ur.failures(res), (what, ur.failures(res))


def _mods(case):
    u = ul if isinstance(case, ul.LaneCase) else um
    return u.make_net(case, DEV), u.make_problem(case, DEV)


def _backward(case, x, call):
    """call(xx, net, prob) -> (J, ...); its backward -> (J, rest, {name: gradient, "x": dJ/dx} on the CPU, forward kernel, adjoint kernel)"""
    net, prob = _mods(case)
    xx = x.to(DEV).clone().requires_grad_(True)
    out = call(xx, net, prob)
    kf = last_kernel()
    out[0].backward()
    torch.cuda.synchronize()
    kb = last_kernel()
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    got["x"] = xx.grad.cpu()
    return out[0].detach().cpu(), out[1:], got, kf, kb


def _weighted(case, w, W=None, **noise):
    ts = list(case.tspan)
    Wd = None if W is None else W.to(DEV)
    return lambda xx, net, prob: na.weighted_ocflow_train(xx, net, prob, ts, case.nt, w.to(DEV), W=Wd, stepper=case.stepper, alph=case.alph, **noise)


# ---------------------------------------------------------------- 1. gradients with given weights
@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
def test_gradients_with_given_weights_against_fp64_autograd(fc):
    family, case = fc
    data = ud.case_data(case)
    w = ur.case_weights(case)
    Jw, _, got, kf, kb = _backward(case, data["x"], _weighted(case, w, data["W"]))
    assert kf == ud.KERNEL[family] and kb == ur.WEIGHTED_KERNEL[family], (kf, kb)
    r64, r32 = ur.weighted_grads(case, torch.float64), ur.weighted_grads(case, torch.float32)
    res = ur.compare_grads(got, r64["grads"], r32["grads"])
    res["Jw"] = uo.compare(Jw, torch.tensor(r64["Jw"], dtype=torch.float64), torch.tensor(r32["Jw"]))
    _check(res, case.id)


# ---------------------------------------------------------------- 2. the bitwise anchor at every instantiation
ANCHOR = [("lane", c) for c in ul.ADJOINT] + [("mono", c) for c in um.ADJOINT] + [fc for fc in ud.CASES if fc[0].startswith("tile")]


def _any_W(case, n):
    g = torch.Generator().manual_seed(911 * case.seed + case.nt)
    return 0.02 * torch.randn(case.nt, n, case.d, generator=g)


@pytest.mark.parametrize("fc", ANCHOR, ids=ud.case_id)
def test_uniform_weights_are_the_existing_adjoint_bitwise(fc, monkeypatch):
    """wrow filled with float32(1 / n_total) in the weighted entry against the existing entry on the same recorded inputs (the same disturbed
    forward, which is deterministic): every parameter gradient and lam0 (x.grad) under torch.equal"""
    family, case = fc
    if not getattr(case, "act_rec", True):
        monkeypatch.setenv("NOCF_ACT_REC", "0")
    # (a bitwise comparison needs no screened starts: the candidates themselves)
    if isinstance(case, ul.LaneCase):
        x = (ul.layout(case)[0] + ul.VAR0 * ul.closed_form_normal(case.n, case.d, case.seed)).contiguous()
    else:
        x = um.candidates(case, case.n)
    n = x.shape[0]
    n_total = getattr(case, "n_total", None) or n
    W = _any_W(case, n)
    ts = list(case.tspan)
    old = lambda xx, net, prob: na.disturbed_ocflow_train(xx, net, prob, ts, case.nt, W.to(DEV), case.stepper, case.alph, n_total=n_total)  # noqa: E731
    w = torch.full((n,), 1.0 / n_total, dtype=torch.float32)
    J0, _, g0, kf0, kb0 = _backward(case, x, old)
    J1, _, g1, kf1, kb1 = _backward(case, x, _weighted(case, w, W))
    assert kf0 == kf1 and kb0 == FULL_KERNEL[family] and kb1 == ur.WEIGHTED_KERNEL[family], (kf0, kf1, kb0, kb1)
    for k in g0:
        assert bool(torch.isfinite(g0[k]).all()) and torch.equal(g0[k], g1[k]), (case.id, k, float((g0[k] - g1[k]).abs().max()))
    assert bool(g0["x"].abs().max() > 0)


# ---------------------------------------------------------------- 3. row independence
SUBSET = [1, 2, 3, 5, 8, 9, 10]          # (ends inside the first 16-row tile of the one-CU kernel, and inside a 4-row tile of the other two)


@pytest.mark.parametrize("fc", [ud.CASES[2], ud.CASES[3], ud.CASES[5]], ids=ud.case_id)
def test_rows_with_weight_zero_do_not_take_part(fc):
    family, case = fc
    data = ud.case_data(case)
    idx = torch.tensor([i for i in SUBSET if i < case.n])
    w = ur.case_weights(case)
    w_sub = w[idx].clone()
    w_sub[w_sub == 0] = 0.5 / case.n                                 # (every row of the subset takes part)
    w_full = torch.zeros_like(w)
    w_full[idx] = w_sub
    _, _, full, _, kb = _backward(case, data["x"], _weighted(case, w_full, data["W"]))
    _, _, sub, _, kb2 = _backward(case, data["x"][idx], _weighted(case, w_sub, data["W"][:, idx].contiguous()))
    assert kb == kb2 == ur.WEIGHTED_KERNEL[family]
    outside = torch.ones(case.n, dtype=torch.bool)
    outside[idx] = False
    assert bool((full["x"][outside] == 0).all())                     # lam0 of a zeroed row: exactly zero
    full_x = dict(full, x=full["x"][idx])
    r64 = ur.weighted_grads(case, torch.float64, weights=w_full, rows=idx)["grads"]
    r32 = ur.weighted_grads(case, torch.float32, weights=w_full, rows=idx)["grads"]
    _check(ur.compare_grads(full_x, r64, r32), case.id + " (zero weights outside the subset)")
    _check(ur.compare_grads(sub, r64, r32), case.id + " (the subset alone)")
    for k in sub:                                                    # ... and the two calls against each other, under the same rule
        ref64 = torch.zeros_like(sub[k], dtype=torch.float64) if r64[k] is None else r64[k]
        ref32 = torch.zeros_like(sub[k]) if r32[k] is None else r32[k]
        tol, _ = uo.tolerance(ref64, ref32)
        assert float((full_x[k].double() - sub[k].double()).abs().max()) <= tol, (case.id, k)


# ---------------------------------------------------------------- 4. weights from the device
@pytest.mark.parametrize("fc", ur.FAMILY_CASES, ids=ud.case_id)
@pytest.mark.parametrize("risk, level", ur.RISK_LEVELS)
def test_risk_weights_value_and_gradient_from_the_device(fc, risk, level):
    family, case = fc
    x, sigma, _ = ur.risk_inputs(case)
    n, R = x.shape[0], ur.RISK_PATHS
    Wdev = na.counter_disturbances(case.nt, n, case.d, sigma, ur.RISK_SEED, tspan=case.tspan, device=DEV)
    rc = ur.risk_case(case, risk, level, W=Wdev.cpu())              # (the device's own disturbances; asserts the ranking condition on them)
    ts = list(case.tspan)
    call = lambda xx, net, prob: na.risk_ocflow_train(xx, net, prob, ts, case.nt, risk, rc["level"], paths=R, sigma=sigma,       # noqa: E731
                                                      seed=ur.RISK_SEED, stepper=case.stepper, alph=case.alph)
    Jr, (cs, info), got, kf, kb = _backward(case, x, call)
    assert kb == ur.WEIGHTED_KERNEL[family] and not kf.startswith("rollout_duo"), (kf, kb)
    r64, r32 = rc["r64"], rc["r32"]
    res = {"weights": uo.compare(info["weights"].cpu(), r64["weights"], r32["weights"]),
           "Jr": uo.compare(Jr, r64["value"], r32["value"]),
           "J rows": uo.compare(ur.row_costs(info["persample"].cpu(), case.alph), r64["J"], r32["J"])}
    w64, v64 = na.risk_weights(ud.case_restate(case, x.double(), rc["W"], torch.float64)["table"], case.alph, risk, rc["level"], paths=R)
    res["weights (risk_weights on the fp64 table)"] = uo.compare(info["weights"].cpu(), w64, r32["weights"])
    res["Jr (risk_weights on the fp64 table)"] = uo.compare(Jr, v64, r32["value"])
    assert info["rho"].shape == (n // R,) and abs(float(info["weights"].sum()) - 1.0) <= 1e-5
    assert abs(float(info["rho"].double().mean()) - float(Jr)) <= 1e-5 * abs(float(Jr))
    res.update(ur.compare_grads(got, r64["grads"], r32["grads"]))   # the fp64 autograd of the VALUE, not of frozen weights
    _check(res, f"{case.id} {risk} {rc['level']:.4g}")


# ---------------------------------------------------------------- 5. the noisy path is the tensor path
@pytest.mark.parametrize("fc", ur.FAMILY_CASES, ids=ud.case_id)
def test_noisy_path_equals_the_tensor_path_bitwise(fc):
    family, case = fc
    x = ud.case_data(case)["x"]
    w = ur.case_weights(case)
    sigma, seed, row0 = ud.SIGMA_REL * case.rad, 77, 5
    W = na.counter_disturbances(case.nt, case.n, case.d, sigma, seed, tspan=case.tspan, row_offset=row0, device=DEV)
    J0, _, g0, kf0, kb0 = _backward(case, x, _weighted(case, w, W))
    J1, _, g1, kf1, kb1 = _backward(case, x, _weighted(case, w, sigma=sigma, seed=seed, row_offset=row0))
    assert kf0 == ud.KERNEL[family] and kf1 == kf0.replace("dist>", "noise>") and kb0 == kb1 == ur.WEIGHTED_KERNEL[family], (kf0, kf1, kb0, kb1)
    assert torch.equal(J0, J1)
    for k in g0:
        assert torch.equal(g0[k], g1[k]), (case.id, k)
    # sigma = 0.0 is the undisturbed call: W = 0
    J2, _, g2, _, _ = _backward(case, x, _weighted(case, w, torch.zeros_like(W)))
    J3, _, g3, _, _ = _backward(case, x, _weighted(case, w, sigma=0.0, seed=1))
    assert torch.equal(J2, J3) and all(torch.equal(g2[k], g3[k]) for k in g2) and not torch.equal(J0, J2)


def test_parameters_changed_before_backward_are_refused():
    family, case = ud.CASES[0]
    data = ud.case_data(case)
    net, prob = _mods(case)
    Jw, _ = _weighted(case, ur.case_weights(case), data["W"])(data["x"].to(DEV), net, prob)
    with torch.no_grad():
        next(net.parameters()).add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        Jw.backward()
    assert all(p.grad is None for p in net.parameters())


# ---------------------------------------------------------------- 6. the driver
def test_trainOC_risk(tmp_path, capsys):
    import trainOC
    from neuraloc_amd.initProb import initProb
    save = os.path.join(str(tmp_path), "r")
    flags = ["--data", "softcorridor", "--niters", "2", "--val_freq", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save,
             "--seed", "1", "--lr", "0.02", "--noise", "0.1", "--noise_seed", "3", "--noise_rng", "counter",
             "--risk", "cvar", "--risk_level", "0.8", "--risk_paths", "4"]
    trainOC.main(flags)
    lines = [ln.split() for ln in capsys.readouterr().out.splitlines() if ln[:5].isdigit()]
    assert [len(ln) for ln in lines] == [11, 19]
    assert all(float(v) == float(v) and abs(float(v)) < float("inf") for ln in lines for v in ln[3:])
    assert last_kernel().startswith("rollout_lane") and any(f.endswith("_checkpt.pth") for f in os.listdir(save))
    # the first iteration's logged value is risk_ocflow_train on the run's first batch and initial network, under the run's seed
    a = trainOC.parse_args(flags)
    torch.manual_seed(1)
    cvt = lambda t: t.to(torch.float32).to(DEV)                      # noqa: E731
    prob, x0, _, _ = initProb("softcorridor", 16, 16, var0=a.var0, alph=a.alph, cvt=cvt)
    net = na.Phi(nTh=2, m=16, d=x0.size(1), alph=a.alph).to(DEV)
    net.train()
    prob.train()
    Jr, cs, info = na.risk_ocflow_train(x0.repeat_interleave(4, 0), net, prob, [0.0, 1.0], 4, "cvar", 0.8, paths=4, sigma=0.1,
                                        seed=(3 << 32) | 1, alph=net.alph)
    assert last_kernel() == "rollout_lane_kernel<noise>"
    assert "{:9.3e}".format(Jr.item()) == lines[0][3]
    assert ["{:8.2e}".format(c.item()) for c in cs] == lines[0][4:11]
    # the risk is the objective: it lies above the mean of the same rows, and the tail takes all the weight
    J = ur.row_costs(info["persample"].double().cpu(), a.alph)
    assert Jr.item() > float(J.mean()) and int((info["weights"] > 0).sum()) == 16
