"""CPU: the yardstick of the disturbance gradient (tests/util_adversary.py) pinned to the oracle at W = 0, the comparator's teeth on two
wrong answers on every case, the two new symbols' export, prototypes and refusals, and the Python argument errors of
neuraloc_amd.disturbance_gradient / worst_case_disturbances -- none of which needs a device."""
import ctypes as C

import pytest
import torch

import __graft_entry__ as entry
import neuraloc_amd as na
from neuraloc_amd import _lib, adversary
import util_adversary as ua
import util_disturb as ud
import util_lane as ul
import util_mono as um
import util_oracle as uo


@pytest.fixture(scope="module")
def L():
    entry.build()
    return _lib.lib()


@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_zero_disturbance_is_autograd_of_the_oracle_bitwise(fc, dtype):
    """grads_wrt_W with W = 0 gives util_lane.autograd_grads' Jc and dJc/dx: the helper adds nothing of its own to the pinned oracle"""
    family, case = fc
    data = ud.case_data(case)
    args = (um.case_sd(case), um.spec(case), data["x"])
    tail = (case.tspan, case.nt, case.stepper, case.alph, dtype)
    r = ua.grads_wrt_W(*args, torch.zeros_like(data["W"]), *tail)
    J0, g0, gx0 = ul.autograd_grads(*args, *tail)
    assert r["Jc"] == J0
    assert torch.equal(r["dx"], gx0)
    assert r["dW"].shape == data["W"].shape and bool(torch.isfinite(r["dW"]).all())


@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
@pytest.mark.parametrize("objective", ua.OBJECTIVES)
def test_wrong_answers_fail_the_comparator(fc, objective):
    """the fp32 restatement passes its own rule and is never exact; dJ/dW shifted by one step and the gradient of the "w_before_step"
    restatement (W added in front of the step: the cotangent one step too early) both fail it"""
    family, case = fc
    r64, r32 = ua.case_grads(case, torch.float64, objective), ua.case_grads(case, torch.float32, objective)
    ok, err, tol, e32 = uo.compare(r32["dW"], r64["dW"], r32["dW"])
    print(f"{case.id} {objective}: max |dW| {float(r64['dW'].abs().max()):.3e}, fp32 restatement {e32:.3e}, tol {tol:.3e}")
    assert ok and e32 > 0.0
    assert uo.compare(r32["dx"], r64["dx"], r32["dx"])[0]
    assert not uo.compare(torch.roll(r64["dW"], 1, 0), r64["dW"], r32["dW"])[0], (case.id, "shifted by one step")
    wrong = ua.case_grads(case, torch.float64, objective, mutation="w_before_step")
    assert not uo.compare(wrong["dW"], r64["dW"], r32["dW"])[0], (case.id, "w_before_step")


def test_search_restatement_is_monotone_and_stays_in_the_ball():
    """util_adversary.search in fp64 on the smallest case: the history never decreases (the best iterate is kept), every iterate is feasible"""
    family, case = ud.CASES[0]
    data = ud.case_data(case)
    eps = ua.median_path_norm(data["W"])
    r = ua.search(case, torch.float64, data["x"], eps, 3)
    assert bool((r["objective"] >= r["nominal"]).all()) and bool((r["objective"] > r["nominal"]).any())
    assert bool((r["W"].pow(2).sum((0, 2)).sqrt() <= eps * (1 + 1e-12)).all())
    assert torch.equal(r["objective"], r["history"].max(0).values)


def test_ascent_reference_formulas():
    g = torch.tensor([[[3.0, 4.0], [0.0, 0.0], [1.0, 0.0]]])                    # nt = 1, n = 3, d = 2
    W = torch.tensor([[[0.0, 0.0], [0.5, 0.5], [10.0, 0.0]]])
    out = ua.ascent_reference(W, g, None, 0.5, 2.0)
    assert torch.allclose(out[0, 0], torch.tensor([0.3, 0.4], dtype=torch.float64))         # a step of length 0.5 along g
    assert torch.equal(out[0, 1], W[0, 1].double())                                           # zero gradient: untouched
    assert torch.allclose(out[0, 2], torch.tensor([2.0, 0.0], dtype=torch.float64))         # outside the ball: projected
    out = ua.ascent_reference(W, g, torch.tensor([0.0, 1.0]), 0.5, 2.0)
    assert torch.allclose(out[0, 0], torch.tensor([0.0, 0.5], dtype=torch.float64))
    assert torch.equal(out[0, 2], W[0, 2].double())                                           # the masked gradient is zero: untouched


def _norm(s):
    return " ".join(s.split())


def test_symbols_are_exported_and_declared(L):
    f = adversary._entries(L)
    assert f is not None
    rec, st, asc = f
    assert st.restype is C.c_int and len(st.argtypes) == 17
    assert asc.restype is C.c_int and len(asc.argtypes) == 9
    with open(entry.REPO + "/include/nocf.h") as fh:
        text = _norm(fh.read())
    proto = ("int nocf_rollout_bwd_states_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1, "
             "const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs, "
             "const float* act_rec, float* lam0, float* lamW, void* workspace, size_t workspace_bytes, void* stream);")
    assert proto in text
    proto = ("int nocf_disturbance_ascent_f32(float* W, const float* g, const float* mask, int64_t n, int32_t nt, int32_t d, "
             "double step, double eps, void* stream);")
    assert proto in text
    assert L.nocf_version() == 113


def _call(L, phi, prob, n=4, nt=2, stepper=4, alph=1, s_all=1, z=1, hs=1, act=0, lam0=1, lamW=1, ws=1, wsb=1 << 30):
    p = C.c_void_p(0x1000)
    nz = lambda f: p if f else None                                  # noqa: E731
    a = (C.c_float * 6)(1, 1, 1, 1, 1, 1) if alph else None
    st = adversary._entries(L)[1]
    return st(C.byref(phi) if phi is not None else None, C.byref(prob) if prob is not None else None, n, nt, stepper, 1.0, a, 1.0,
              nz(s_all), nz(z), nz(hs), nz(act), nz(lam0), nz(lamW), nz(ws), wsb, None)


def _phi(d, m, nTh=2, r=5):
    phi = _lib.NocfPhi()
    phi.d, phi.m, phi.nTh, phi.r = d, m, nTh, r
    for k in ("K0", "b0", "K", "b", "w", "A", "cw", "cb_dev"):
        setattr(phi, k, 0x1000)
    return phi


def test_abi_refusals_need_no_device(L):
    """every refusal returns before a launch: the pointers are never dereferenced.  One shape per family: lane (m = 16), one-CU (m = 64),
    per-tile (m = 129)"""
    prob, keep = na.Cross2D(torch.zeros(4))._c_struct("cpu")
    for m in (16, 64, 129):
        phi = _phi(4, m)
        assert _call(L, phi, prob, lam0=0, lamW=0) == -1, m          # NOCF_E_NULL: nothing to write
        assert _call(L, phi, prob, alph=0) == -1
        assert _call(L, phi, prob, s_all=0) == -1
        assert _call(L, phi, prob, z=0) == -1
        assert _call(L, phi, prob, hs=0) == -1
        assert _call(L, phi, prob, ws=0) == -1
        assert _call(L, phi, None) == -1
        assert _call(L, None, prob) == -1
        assert _call(L, phi, prob, n=0) == -2                         # NOCF_E_SHAPE
        assert _call(L, phi, prob, nt=0) == -2
        assert _call(L, phi, prob, stepper=3) == -5                   # NOCF_E_STEPPER
    for m in (64, 129):                                               # (the lane kernel needs no workspace)
        assert _call(L, _phi(4, m), prob, wsb=16) == -4               # NOCF_E_WORKSPACE
    assert _call(L, _phi(4, 16, nTh=1), prob) != 0                    # a depth no kernel takes
    prob6, keep6 = na.Cross2D(torch.zeros(6))._c_struct("cpu")
    assert _call(L, _phi(4, 16), prob6) == -3                         # NOCF_E_PROB: the problem's agents do not match d
    asc = adversary._entries(L)[2]
    p = C.c_void_p(0x1000)
    assert asc(None, p, None, 4, 2, 3, 0.1, 1.0, None) == -1
    assert asc(p, None, None, 4, 2, 3, 0.1, 1.0, None) == -1
    assert asc(p, p, None, 0, 2, 3, 0.1, 1.0, None) == -2
    assert asc(p, p, None, 4, 0, 3, 0.1, 1.0, None) == -2
    assert asc(p, p, None, 4, 2, 0, 0.1, 1.0, None) == -2
    assert asc(p, p, None, 4, 2, 3, -0.1, 1.0, None) == -2
    assert asc(p, p, None, 4, 2, 3, 0.1, float("nan"), None) == -2
    assert asc(p, p, None, 4, 2, 3, float("inf"), 1.0, None) == -2


def test_python_argument_errors_need_no_device():
    case = ud.CASES[0][1]
    net = um.make_net(case, "cpu")
    prob = um.make_problem(case)
    n, nt, d = 3, case.nt, case.d
    x = um.candidates(case, n)
    W = torch.zeros(nt, n, d)
    g, w = na.disturbance_gradient, na.worst_case_disturbances
    with pytest.raises(RuntimeError, match="single precision only"):
        g(x.double(), net, prob, nt, W)
    with pytest.raises(RuntimeError, match="single precision only"):
        g(x, net, prob, nt, W.double())
    net64 = um.make_net(case, "cpu").double()
    with pytest.raises(RuntimeError, match="single precision only"):
        g(x, net64, prob, nt, W)
    for bad in (W[:-1], W[:, :-1], W[:, :, :-1], W[0]):
        with pytest.raises(ValueError, match="nt-by-nex-by-d"):
            g(x, net, prob, nt, bad)
    with pytest.raises(ValueError, match="nex-by-d"):
        g(x[0], net, prob, nt, W)
    with pytest.raises(ValueError):
        g(x[:, :-1], net, prob, nt, W[:, :, :-1])
    with pytest.raises(ValueError, match="nt must be"):
        g(x, net, prob, 0, W)
    with pytest.raises(ValueError, match="stepper"):
        g(x, net, prob, nt, W, stepper="rk2")
    with pytest.raises(ValueError, match="alph"):
        g(x, net, prob, nt, W, alph=[1.0] * 5)
    with pytest.raises(ValueError, match="objective"):
        g(x, net, prob, nt, W, objective="L")
    with pytest.raises(ValueError, match="n_total"):
        g(x, net, prob, nt, W, n_total=0)
    with pytest.raises(TypeError):
        g(x, net, prob, nt, W.numpy())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g(x, net, prob, nt, W)

    with pytest.raises(RuntimeError, match="single precision only"):
        w(x.double(), net, prob, nt, 0.1)
    with pytest.raises(RuntimeError, match="single precision only"):
        w(x, net, prob, nt, 0.1, W0=W.double())
    with pytest.raises(RuntimeError, match="single precision only"):
        w(x, net64, prob, nt, 0.1, W0=W)
    with pytest.raises(ValueError, match="nt-by-nex-by-d"):
        w(x, net, prob, nt, 0.1, W0=W[:-1])
    with pytest.raises(ValueError, match="eps"):
        w(x, net, prob, nt, -1.0, W0=W)
    with pytest.raises(ValueError, match="eps"):
        w(x, net, prob, nt, float("nan"), W0=W)
    with pytest.raises(ValueError, match="steps"):
        w(x, net, prob, nt, 0.1, steps=-1, W0=W)
    with pytest.raises(ValueError, match="step_size"):
        w(x, net, prob, nt, 0.1, step_size=-0.5, W0=W)
    with pytest.raises(ValueError, match="objective"):
        w(x, net, prob, nt, 0.1, objective="L", W0=W)
    with pytest.raises(ValueError, match="stepper"):
        w(x, net, prob, nt, 0.1, stepper="rk2", W0=W)
    with pytest.raises(ValueError, match="mask"):
        w(x, net, prob, nt, 0.1, mask=torch.ones(d + 1), W0=W)
    with pytest.raises(ValueError, match="nt must be"):
        w(x, net, prob, 0, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w(x, net, prob, nt, 0.1, W0=W)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        w(x, net, prob, nt, 0.1)


def test_disturbed_training_still_refuses_a_differentiable_W():
    case = ud.CASES[0][1]
    net, prob = um.make_net(case, "cpu"), um.make_problem(case)
    x = um.candidates(case, 3)
    W = torch.zeros(case.nt, 3, case.d, requires_grad=True)
    with pytest.raises(NotImplementedError, match="dJ/dW"):
        na.disturbed_ocflow_train(x, net, prob, list(case.tspan), case.nt, W)
