"""GPU: training through disturbed rollouts (neuraloc_amd.disturbed_ocflow_train, nocf_rollout_record_disturbed_f32).  Jc, cs, every
parameter gradient and dJc/dx against fp64 autograd of the restated oracle (tests/util_disturb_train.py) on every case of
util_disturb.CASES under util_oracle's rule; the record at the C entry point; W = 0 against the existing training call bitwise; shards
with n_total; the refusals; trainOC.py --noise."""
import ctypes as C
import os

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, train
import util_disturb as ud
import util_disturb_train as ut
import util_lane as ul
import util_mono as um
import util_oracle as uo

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BWD_KERNEL = {"lane": "rollout_lane_bwd_kernel", "mono": "rollout_mono_bwd_kernel", "tile": "rollout_bwd_kernel",
              "tile-fixed": "rollout_bwd_kernel"}


def last_kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def _check(res, what):
    for k, v in res.items():
        print(f"{what} {k}: err {v[1]:.3e} tol {v[2]:.3e} fp32 restatement {v[3]:.3e}")
    assert not ut.failures(res), (what, ut.failures(res))


def _run(case, x, W, n_total=None, family=None):
    """one disturbed training call and its backward -> (Jc, cs [7], {name: gradient, "x": dJc/dx}), all on the CPU"""
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    xx = x.to(DEV).clone().requires_grad_(True)
    Jc, cs = na.disturbed_ocflow_train(xx, net, prob, list(case.tspan), case.nt, W.to(DEV), case.stepper, case.alph, n_total=n_total)
    kf = last_kernel()
    Jc.backward()
    torch.cuda.synchronize()
    kb = last_kernel()
    if family is not None:
        assert kf == ud.KERNEL[family] and not kf.startswith("rollout_duo"), kf
        assert kb == BWD_KERNEL[family], kb
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    got["x"] = xx.grad.cpu()
    return Jc.detach().cpu(), torch.stack(list(cs)).detach().cpu(), got


def _grad_res(got, r64, r32):
    w64, w32 = ut.with_x(r64), ut.with_x(r32)
    for k in w64:                                                   # (a parameter Jc does not reach has no autograd gradient: zero)
        if w64[k] is None:
            w64[k] = torch.zeros_like(got[k], dtype=torch.float64)
        if w32[k] is None:
            w32[k] = torch.zeros_like(got[k])
    return ut.compare_grads(got, w64, w32)


def _forward_refs(case, data, rows=None):
    """the table's summary (Jc, cs, jc_rows) in fp64 and fp32, for util_lane.compare_forward's rule on the means"""
    sl = slice(None) if rows is None else rows
    return (ul._summary(case, dict(table=data["r64"]["table"][sl])), ul._summary(case, dict(table=data["r32"]["table"][sl])))


@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
def test_gradients_against_fp64_autograd(fc):
    family, case = fc
    data = ud.case_data(case)
    Jc, cs, got = _run(case, data["x"], data["W"], family=family)
    f64, f32 = _forward_refs(case, data)
    _check(ul.compare_forward(dict(Jc=Jc, cs=cs), f64, f32), case.id)
    r64, r32 = ut.case_grads(case, torch.float64), ut.case_grads(case, torch.float32)
    assert abs(r64["Jc"] - float(f64["Jc"])) <= 1e-12 * abs(r64["Jc"])             # (the two fp64 references are one)
    _check(_grad_res(got, r64, r32), case.id)


RECORD_CASES = [ud.CASES[1], ud.CASES[3], ud.CASES[5], ud.CASES[7]]


@pytest.mark.parametrize("fc", RECORD_CASES, ids=ud.case_id)
def test_record_at_the_abi(fc):
    """s_all of nocf_rollout_record_disturbed_f32 holds the displaced states where a step begins (a record taken in front of the
    displacement fails here, whatever the adjoint does with it), and z_out the displaced z(T)"""
    family, case = fc
    data = ud.case_data(case)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x, W = data["x"].to(DEV), data["W"].to(DEV)
    n, d, nt, m = case.n, case.d, case.nt, case.m
    E = nt * (4 if case.stepper == "rk4" else 1)
    L = _lib.lib()
    f = train._disturbed_entry(L)
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(x.device)
    nan = float("nan")
    s_all = torch.full((E, n, d + 1), nan, device=DEV)
    z = torch.full((n, d + 4), nan, device=DEV)
    tab, sums = torch.full((n, 7), nan, device=DEV), torch.full((8,), nan, device=DEV)
    nact = int(L.nocf_activation_record_floats(d, m, case.nTh, n, nt, train._STEPPERS[case.stepper])) if family == "mono" else 0
    act = torch.full((nact,), nan, device=DEV) if nact else None
    rec = C.c_int32(-1)
    alph_c = (C.c_float * 6)(*case.alph)
    with torch.cuda.device(x.device):
        rc = f(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), _lib.ptr(W), n, float(case.tspan[0]), float(case.tspan[1]), nt,
               train._STEPPERS[case.stepper], alph_c, _lib.ptr(z), _lib.ptr(tab), _lib.ptr(sums), _lib.ptr(s_all), _lib.ptr(act),
               C.byref(rec), _lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == 0 and last_kernel() == ud.KERNEL[family]
    assert rec.value == (1 if nact else 0)
    if act is not None:
        assert family == "mono" and not bool(act.isnan().any())
    s = s_all.cpu()
    assert not bool(s.isnan().any()) and not bool(z.isnan().any()) and not bool(tab.isnan().any())
    res = {"s_all": uo.compare(s[:, :, :d].permute(1, 0, 2), data["r64"]["stages"][:, :E], data["r32"]["stages"][:, :E]),
           "z": uo.compare(z.cpu(), data["r64"]["z"], data["r32"]["z"]),
           "table": uo.compare(tab.cpu(), data["r64"]["table"], data["r32"]["table"])}
    tt = torch.tensor(um.stage_times(case), dtype=torch.float64).reshape(E, 1).expand(E, n)
    assert float((s[:, :, d].double() - tt).abs().max()) <= (nt + 2) * 2.0 ** -23
    _check(res, case.id)
    # the first stage input of step 1 is the displaced state behind step 0, not the undisplaced one: they differ by W[0], far above the rule
    nst = E // nt
    und = s[nst, :, :d] - data["W"][0]
    assert not uo.compare(und, data["r64"]["stages"][:, nst], data["r32"]["stages"][:, nst])[0]


ZERO_CASES = [ud.CASES[1], ud.CASES[3], ud.CASES[4], ud.CASES[5], ud.CASES[7]]


@pytest.mark.parametrize("fc", ZERO_CASES, ids=ud.case_id)
def test_zero_disturbance_is_the_existing_training_call_bitwise(fc, monkeypatch):
    family, case = fc
    if case.m == 512:
        monkeypatch.setenv("NOCF_DUO", "0")                          # (the undisturbed m = 512 call then records on the per-tile kernel too)
    data = ud.case_data(case)
    Jc, cs, got = _run(case, data["x"], torch.zeros_like(data["W"]), family=family)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    xx = data["x"].to(DEV).clone().requires_grad_(True)
    J0, cs0 = na.OCflow(xx, net, prob, list(case.tspan), case.nt, case.stepper, case.alph)
    k1 = last_kernel()
    J0.backward()
    torch.cuda.synchronize()
    assert ud.KERNEL[family].replace("<dist>", "").replace(", dist>", ">") == k1 and last_kernel() == BWD_KERNEL[family], (k1, last_kernel())
    assert torch.equal(Jc, J0.detach().cpu())
    assert torch.equal(cs, torch.stack(list(cs0)).detach().cpu())
    for k, p in net.named_parameters():
        assert torch.equal(got[k], p.grad.cpu()), k
    assert torch.equal(got["x"], xx.grad.cpu())


def test_two_halves_with_n_total_sum_to_the_whole_batch():
    family, case = ud.CASES[1]
    data = ud.case_data(case)
    n = case.n
    h = n // 2
    parts = [_run(case, data["x"][sl], data["W"][:, sl].contiguous(), n_total=n, family=family) for sl in (slice(0, h), slice(h, n))]
    got = {k: parts[0][2][k] + parts[1][2][k] for k in parts[0][2] if k != "x"}
    got["x"] = torch.cat([parts[0][2]["x"], parts[1][2]["x"]])
    _check(_grad_res(got, ut.case_grads(case, torch.float64), ut.case_grads(case, torch.float32)), case.id + " (two halves)")
    # each half logs its own means; weighted by the halves' rows they recombine to the whole batch's
    cs = (h * parts[0][1].double() + (n - h) * parts[1][1].double()) / n
    a = case.alph
    Jc = cs[0] + a[0] * cs[1] + a[3] * cs[2] + a[4] * cs[3] + a[5] * cs[4]
    f64, f32 = _forward_refs(case, data)
    _check(ul.compare_forward(dict(Jc=Jc, cs=cs), f64, f32), case.id + " (recombined means)")
    # ... and a half alone, normalised by its own rows, is the fp64 reference of those rows (n_total changes the gradients only)
    sl = slice(0, h)
    r64, r32 = ut.case_grads(case, torch.float64, n_total=n, rows=sl), ut.case_grads(case, torch.float32, n_total=n, rows=sl)
    _check(_grad_res(parts[0][2], r64, r32), case.id + " (first half of n_total)")
    f64, f32 = _forward_refs(case, data, sl)
    _check(ul.compare_forward(dict(Jc=parts[0][0], cs=parts[0][1]), f64, f32), case.id + " (first half's means)")


def test_refusals_leave_the_gradients_untouched():
    family, case = ud.CASES[0]
    data = ud.case_data(case)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x, W = data["x"].to(DEV), data["W"].to(DEV)
    ts, nt = list(case.tspan), case.nt
    Jc, _ = na.disturbed_ocflow_train(x, net, prob, ts, nt, W, case.stepper, case.alph)
    Jc.backward()
    torch.cuda.synchronize()
    before = {k: p.grad.clone() for k, p in net.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in before.values())

    def refused(exc, match, *a, **kw):
        with pytest.raises(exc, match=match):
            na.disturbed_ocflow_train(*a, **kw)
        for k, p in net.named_parameters():
            assert torch.equal(p.grad, before[k]), k

    refused(RuntimeError, "single precision only", x.double(), net, prob, ts, nt, W)
    refused(RuntimeError, "single precision only", x, net, prob, ts, nt, W.double())
    refused(NotImplementedError, "dJ/dW", x, net, prob, ts, nt, W.clone().requires_grad_(True))
    refused(ValueError, "nt-by-nex-by-d", x, net, prob, ts, nt, W[:-1])
    refused(ValueError, "nt-by-nex-by-d", x, net, prob, ts, nt, W[:, :-1])
    refused(ValueError, "nt-by-nex-by-d", x, net, prob, ts, nt, W[:, :, :-1])
    refused(ValueError, "nex-by-d", x[0], net, prob, ts, nt, W)
    refused(ValueError, "nt must be", x, net, prob, ts, 0, W)
    refused(ValueError, "stepper", x, net, prob, ts, nt, W, stepper="rk2")
    refused(ValueError, "same device", x, net, prob, ts, nt, W.cpu())
    # disturbed_rollout keeps its refusal under autograd; the training call is the differentiable one
    with pytest.raises(NotImplementedError):
        na.disturbed_rollout(x, net, prob, nt, W)
    net.zero_grad()
    xx = x.clone().requires_grad_(True)
    Jc, cs = na.disturbed_ocflow_train(xx, net, prob, ts, nt, W, case.stepper, case.alph)
    Jc.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Jc)) and all(bool(torch.isfinite(c)) for c in cs) and bool(torch.isfinite(xx.grad).all())
    for k, p in net.named_parameters():
        assert torch.equal(p.grad, before[k]), k                     # (the same call again: the same gradients, bit for bit)


def _train_lines(capsys, tmp_path, name, *flags):
    import trainOC
    save = os.path.join(str(tmp_path), name)
    trainOC.main(["--data", "softcorridor", "--niters", "2", "--val_freq", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save,
                  "--seed", "1", "--lr", "0.02", *flags])
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln[:5].isdigit()]
    assert len(lines) == 2
    return lines


def test_trainOC_noise_flag(tmp_path, capsys):
    """trainOC.py --noise on the problem tests/test_drivers_gpu.py trains (softcorridor, m = 16): 2 iterations of 16 samples"""
    import trainOC
    a = _train_lines(capsys, tmp_path, "a", "--noise", "0.1", "--noise_seed", "3")
    b = _train_lines(capsys, tmp_path, "b", "--noise", "0.1", "--noise_seed", "3")
    c = _train_lines(capsys, tmp_path, "c", "--noise", "0.1", "--noise_seed", "4")
    p = _train_lines(capsys, tmp_path, "p")
    loss = lambda lines: [ln.split()[3] for ln in lines]             # noqa: E731
    untimed = lambda lines: [ln.split()[:2] + ln.split()[3:] for ln in lines]          # noqa: E731  (column 2 is the wall time)
    assert loss(a) == loss(b) and untimed(a) == untimed(b)           # same seeds: the same log
    assert loss(a)[0] != loss(p)[0] and loss(a)[0] != loss(c)[0]     # the disturbances reach the first iteration's loss, and follow their seed
    assert all(float(v) == float(v) and abs(float(v)) < float("inf") for v in loss(a) + loss(p))
    # the validation line keeps its format: 11 training columns on every line, 8 validation columns behind them where validation ran
    for lines in (a, p):
        assert [len(ln.split()) for ln in lines] == [11, 19]
    assert os.listdir(os.path.join(str(tmp_path), "a")) and os.listdir(os.path.join(str(tmp_path), "p"))
    # validation is undisturbed: with a learning rate of 0 the parameters stay put, and the validation costs are the undisturbed run's
    a0 = _train_lines(capsys, tmp_path, "a0", "--noise", "0.1", "--noise_seed", "3", "--lr", "0")
    p0 = _train_lines(capsys, tmp_path, "p0", "--lr", "0")
    assert a0[1].split()[11:] == p0[1].split()[11:] and a0[1].split()[3] != p0[1].split()[3]
    # --prec double with --noise is refused before anything runs or is written
    save = os.path.join(str(tmp_path), "d")
    with pytest.raises(SystemExit, match="single precision"):
        trainOC.main(["--data", "softcorridor", "--niters", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save,
                      "--prec", "double", "--noise", "0.1"])
    assert not os.path.exists(save) and capsys.readouterr().out == ""
