"""CPU: min-max training's yardstick helper (tests/util_minmax.py) has teeth on a W.grad one step late and on the "w_before_step"
restatement on every case; the three joint entries' export, prototypes and refusals; every refusal of neuraloc_amd.minmax_ocflow_train /
ascend_disturbances / adversarial_step / pgd_ocflow_train and of trainOC.py's --adv flags -- none of which touches a device."""
import ctypes as C
import os

import pytest
import torch

import __graft_entry__ as entry
import neuraloc_amd as na
from neuraloc_amd import _lib, train
import util_disturb as ud
import util_minmax as umm
import util_mono as um


@pytest.fixture(scope="module")
def L():
    entry.build()
    return _lib.lib()


def _as_got(r):
    """a reference dict as an answer (a parameter Jc does not reach has no autograd gradient: zero)"""
    return {k: (torch.zeros(1) if v is None else v) for k, v in r.items()}


@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
def test_wrong_W_gradients_fail_the_helper(fc):
    """the fp32 restatement passes the rule on every entry; with W.grad shifted by one step the helper reports W and W alone (it does not
    fail wholesale); the gradients of the "w_before_step" restatement (W added in front of the step: the cotangent one step too early)
    fail on W too"""
    family, case = fc
    r64, r32 = umm.references(case, torch.float64), umm.references(case, torch.float32)
    assert set(r64) == {k for k, _ in um.make_net(case, "cpu").named_parameters()} | {"x", "W"}
    res = umm.compare(_as_got(r32), r64, r32)
    assert not umm.failures(res), (case.id, umm.failures(res))
    late = _as_got(r64)
    late["W"] = umm.shifted(r64["W"])
    fails = umm.failures(umm.compare(late, r64, r32))
    assert set(fails) == {"W"}, (case.id, "shifted by one step", fails)
    wrong = umm.references(case, torch.float64, mutation="w_before_step")
    fails = umm.failures(umm.compare(_as_got(wrong), r64, r32))
    assert "W" in fails, (case.id, "w_before_step", fails)


def _norm(s):
    return " ".join(s.split())


def test_symbols_are_exported_and_declared(L):
    f = train._joint_entries(L)
    assert f is not None
    small, mid, act = f
    assert small.restype is C.c_int and len(small.argtypes) == len(L.nocf_rollout_bwd_small_f32.argtypes) + 1
    assert mid.restype is C.c_int and len(mid.argtypes) == len(L.nocf_rollout_bwd_mid_f32.argtypes) + 1
    assert act.restype is C.c_int and len(act.argtypes) == len(L.nocf_rollout_bwd_act_f32.argtypes) + 1
    with open(entry.REPO + "/include/nocf.h") as fh:
        text = _norm(fh.read())
    head = ("(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1, "
            "const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs, ")
    assert "int nocf_rollout_bwd_small_w_f32" + head + "float* gpart, float* lam0, float* lamW, void* stream);" in text
    assert ("int nocf_rollout_bwd_mid_w_f32" + head + "const float* act_rec, float* gpart, int64_t gpart_rows, float* lam0, float* lamW, "
            "void* workspace, size_t workspace_bytes, void* stream);") in text
    assert ("int nocf_rollout_bwd_act_w_f32" + head + "float* Y, float* Ob, float* V, float* Ab, float* Qb, float* U0, float* Wb, float* Gb, "
            "float* Sx, float* PHIb, float* lam0, float* lamW, const float* act_rec, void* workspace, size_t workspace_bytes, void* stream);") in text
    # the existing prototypes stay, and so does the version: callers probe for the symbols
    assert "int nocf_rollout_bwd_small_f32" + head + "float* gpart, float* lam0, void* stream);" in text
    assert L.nocf_version() == 113


def _phi(d, m, nTh=2, r=5):
    phi = _lib.NocfPhi()
    phi.d, phi.m, phi.nTh, phi.r = d, m, nTh, r
    for k in ("K0", "b0", "K", "b", "w", "A", "cw", "cb_dev"):
        setattr(phi, k, 0x1000)
    return phi


def _calls(L, fam, phi, prob, n=4, nt=2, stepper=4, alph=1, s_all=1, z=1, hs=1, out=1, lamW=1, ws=1, wsb=1 << 30):
    """(existing entry's answer, joint entry's answer) of family fam (0 lane, 1 one-CU, 2 per-tile) on the same arguments; out: the gradient
    buffers.  Only that family's two entries are called, and every caller passes arguments that family refuses: the pointers are fakes"""
    p = C.c_void_p(0x1000)
    nz = lambda f: p if f else None                                  # noqa: E731
    a = (C.c_float * 6)(1, 1, 1, 1, 1, 1) if alph else None
    small, mid, act = train._joint_entries(L)
    head = (C.byref(phi) if phi is not None else None, C.byref(prob) if prob is not None else None, n, nt, stepper, 1.0, a, 1.0,
            nz(s_all), nz(z), nz(hs))
    w = (nz(lamW),)
    if fam == 0:
        return L.nocf_rollout_bwd_small_f32(*head, nz(out), p, None), small(*head, nz(out), p, *w, None)
    if fam == 1:
        return (L.nocf_rollout_bwd_mid_f32(*head, None, nz(out), 1 << 20, p, nz(ws), wsb, None),
                mid(*head, None, nz(out), 1 << 20, p, *w, nz(ws), wsb, None))
    return (L.nocf_rollout_bwd_act_f32(*head, *([nz(out)] * 10), p, None, nz(ws), wsb, None),
            act(*head, *([nz(out)] * 10), p, *w, None, nz(ws), wsb, None))


def test_abi_refusals_are_the_existing_entries(L):
    """every refusal of a joint entry is the answer the existing entry gives to the same arguments, with and without lamW, and returns before
    a launch: the pointers are never dereferenced.  One shape per family: lane (m = 16), one-CU (m = 64), per-tile (m = 129)"""
    prob, keep = na.Cross2D(torch.zeros(4))._c_struct("cpu")
    prob6, keep6 = na.Cross2D(torch.zeros(6))._c_struct("cpu")
    for fam, m in enumerate((16, 64, 129)):
        phi = _phi(4, m)
        for lamW in (1, 0):
            for kw, want in ((dict(alph=0), -1), (dict(s_all=0), -1), (dict(z=0), -1), (dict(hs=0), -1), (dict(out=0), -1),
                             (dict(n=0), -2), (dict(nt=0), -2), (dict(stepper=3), -5)):
                old, new = _calls(L, fam, phi, prob, lamW=lamW, **kw)
                assert old == new == want, (m, lamW, kw, old, new)
            old, new = _calls(L, fam, None, prob, lamW=lamW)
            assert old == new == -1
            old, new = _calls(L, fam, _phi(4, m), prob6, lamW=lamW)
            assert old == new == -3                                   # NOCF_E_PROB: the problem's agents do not match d
            if fam:                                                   # (the lane kernel needs no workspace)
                old, new = _calls(L, fam, phi, prob, lamW=lamW, ws=0)
                assert old == new == -1
                old, new = _calls(L, fam, phi, prob, lamW=lamW, wsb=16)
                assert old == new == -4                               # NOCF_E_WORKSPACE
    # a shape that is not the family's own: NOCF_E_SHAPE from the lane and the one-CU entry, as from the existing ones (the per-tile
    # entry would take this shape and launch: it is not called)
    for lamW in (1, 0):
        for fam in (0, 1):
            assert _calls(L, fam, _phi(4, 129), prob, lamW=lamW) == (-2, -2)


def test_python_refusals_need_no_device():
    case = ud.CASES[0][1]
    net = um.make_net(case, "cpu")
    prob = um.make_problem(case)
    n, nt, d = 3, case.nt, case.d
    ts = list(case.tspan)
    x = um.candidates(case, n)
    W = torch.zeros(nt, n, d, requires_grad=True)
    net64 = um.make_net(case, "cpu").double()
    mm = na.minmax_ocflow_train
    for Wv in (W, W.detach()):                                       # with and without a gradient: the same checks, the same messages
        with pytest.raises(RuntimeError, match="single precision only"):
            mm(x.double(), net, prob, ts, nt, Wv)
        with pytest.raises(RuntimeError, match="single precision only"):
            mm(x, net, prob, ts, nt, Wv.double())
        with pytest.raises(RuntimeError, match="single precision only"):
            mm(x, net64, prob, ts, nt, Wv)
        for bad in (Wv[:-1], Wv[:, :-1], Wv[:, :, :-1], Wv[0]):
            with pytest.raises(ValueError, match="nt-by-nex-by-d"):
                mm(x, net, prob, ts, nt, bad)
        with pytest.raises(ValueError, match="nex-by-d"):
            mm(x[0], net, prob, ts, nt, Wv)
        with pytest.raises(ValueError, match="nt must be"):
            mm(x, net, prob, ts, 0, Wv)
        with pytest.raises(ValueError, match="stepper"):
            mm(x, net, prob, ts, nt, Wv, stepper="rk2")
        with pytest.raises(ValueError, match="alph"):
            mm(x, net, prob, ts, nt, Wv, alph=[1.0] * 5)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            mm(x, net, prob, ts, nt, Wv)
    with pytest.raises(TypeError):
        mm(x, net, prob, ts, nt, W.detach().numpy())
    # disturbed_ocflow_train keeps its own refusal
    with pytest.raises(NotImplementedError, match="dJ/dW"):
        na.disturbed_ocflow_train(x, net, prob, ts, nt, W)

    adv = na.adversarial_step
    with pytest.raises(RuntimeError, match="single precision only"):
        adv(x, net, prob, ts, nt, W.detach().double().requires_grad_(True), 0.1, 0.05)
    with pytest.raises(RuntimeError, match="single precision only"):
        adv(x.double(), net, prob, ts, nt, W, 0.1, 0.05)
    with pytest.raises(ValueError, match="requires a gradient"):
        adv(x, net, prob, ts, nt, W.detach(), 0.1, 0.05)
    with pytest.raises(ValueError, match="eps"):
        adv(x, net, prob, ts, nt, W, -0.1, 0.05)
    with pytest.raises(ValueError, match="step_size"):
        adv(x, net, prob, ts, nt, W, 0.1, float("nan"))
    with pytest.raises(ValueError, match="mask"):
        adv(x, net, prob, ts, nt, W, 0.1, 0.05, mask=torch.ones(d + 1))
    with pytest.raises(ValueError, match="nt-by-nex-by-d"):
        adv(x, net, prob, ts, nt, W[:-1].detach().requires_grad_(True), 0.1, 0.05)
    with pytest.raises(TypeError):
        adv(x, net, prob, ts, nt, None, 0.1, 0.05)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        adv(x, net, prob, ts, nt, W, 0.1, 0.05)
    assert W.grad is None and all(p.grad is None for p in net.parameters())

    pgd = na.pgd_ocflow_train
    with pytest.raises(RuntimeError, match="single precision only"):
        pgd(x.double(), net, prob, ts, nt, 0.1, 2)
    with pytest.raises(RuntimeError, match="single precision only"):
        pgd(x, net, prob, ts, nt, 0.1, 2, W0=W.detach().double())
    with pytest.raises(ValueError, match="eps"):
        pgd(x, net, prob, ts, nt, -1.0, 2)
    with pytest.raises(ValueError, match="steps"):
        pgd(x, net, prob, ts, nt, 0.1, -1)
    with pytest.raises(ValueError, match="objective"):
        pgd(x, net, prob, ts, nt, 0.1, 2, objective="L")
    with pytest.raises(ValueError, match="mask"):
        pgd(x, net, prob, ts, nt, 0.1, 2, mask=torch.ones(d + 1))
    with pytest.raises(ValueError, match="stepper"):
        pgd(x, net, prob, ts, nt, 0.1, 2, stepper="rk2")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pgd(x, net, prob, ts, nt, 0.1, 2)


def test_ascend_disturbances_argument_checks():
    W, g = torch.zeros(2, 3, 4), torch.ones(2, 3, 4)
    asc = na.ascend_disturbances
    with pytest.raises(TypeError):
        asc(W.numpy(), g, 1.0, 0.1)
    with pytest.raises(TypeError):
        asc(W, None, 1.0, 0.1)
    with pytest.raises(RuntimeError, match="single precision only"):
        asc(W.double(), g, 1.0, 0.1)
    with pytest.raises(RuntimeError, match="single precision only"):
        asc(W, g.double(), 1.0, 0.1)
    with pytest.raises(ValueError, match="nt-by-nex-by-d"):
        asc(W[0], g[0], 1.0, 0.1)
    with pytest.raises(ValueError, match="nt-by-nex-by-d"):
        asc(W[:, :0], g[:, :0], 1.0, 0.1)
    with pytest.raises(ValueError, match="W's shape"):
        asc(W, g[:1], 1.0, 0.1)
    for eps in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            asc(W, g, eps, 0.1)
    for step in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="step_size"):
            asc(W, g, 1.0, step)
    with pytest.raises(ValueError, match="mask"):
        asc(W, g, 1.0, 0.1, mask=torch.ones(5))
    with pytest.raises(RuntimeError, match="no_grad"):
        asc(W.clone().requires_grad_(True), g, 1.0, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asc(W, g, 1.0, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        with torch.no_grad():
            asc(W.clone().requires_grad_(True), g, 1.0, 0.1)
    assert bool((W == 0).all())


@pytest.mark.parametrize("flags, match", [
    (["--adv", "0.5", "--prec", "double"], "single precision"),
    (["--adv", "0.5", "--noise", "0.1"], "exclude"),
    (["--adv", "-0.5"], "--adv EPS must be"),
    (["--adv", "0.5", "--adv_objective", "control"], "--adv_mode pgd"),
    (["--adv", "0.5", "--adv_mode", "pgd", "--adv_steps", "0"], "--adv_steps"),
])
def test_trainOC_adv_refusals_come_before_anything_runs(tmp_path, capsys, flags, match):
    import trainOC
    save = os.path.join(str(tmp_path), "run")
    with pytest.raises(SystemExit, match=match):
        trainOC.main(["--data", "softcorridor", "--niters", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save, *flags])
    assert not os.path.exists(save) and capsys.readouterr().out == ""


def test_trainOC_adv_flag_defaults():
    import trainOC
    a = trainOC.parse_args([])
    assert a.adv == 0.0 and a.adv_mode == "free" and a.adv_objective == "Jc" and a.adv_steps >= 1
    with pytest.raises(SystemExit):
        trainOC.parse_args(["--adv_mode", "fast"])
