"""CPU: the yardstick of disturbed training (tests/util_disturb_train.py) pinned to the oracle at W = 0, the comparator's teeth on wrong
restatements' gradients, and nocf_rollout_record_disturbed_f32's export, prototype and refusals plus the Python argument errors of
neuraloc_amd.disturbed_ocflow_train -- none of which needs a device."""
import ctypes as C

import pytest
import torch

import __graft_entry__ as entry
import neuraloc_amd as na
from neuraloc_amd import _lib, train
import util_disturb as ud
import util_disturb_train as ut
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
    """grads_disturbed with W = 0 is util_lane.autograd_grads: the helper adds nothing of its own to the pinned oracle"""
    family, case = fc
    data = ud.case_data(case)
    args = (um.case_sd(case), um.spec(case), data["x"])
    tail = (case.tspan, case.nt, case.stepper, case.alph, dtype)
    J, g, gx, cs = ut.grads_disturbed(*args, torch.zeros_like(data["W"]), *tail)
    J0, g0, gx0 = ul.autograd_grads(*args, *tail)
    assert J == J0 and set(g) == set(g0)
    for k in g0:
        assert torch.equal(g[k], g0[k]), k
    assert torch.equal(gx, gx0)


# one case per kernel family, the smallest of each, plus the rk1 and the train-mode variants
TEETH = [ud.CASES[1], ud.CASES[4], ud.CASES[5], ud.CASES[8], ud.CASES[10]]
W_SCALE = 1.0            # sigma = 0.05 r is enough on every one of them: no scaling of W


@pytest.mark.parametrize("fc", TEETH, ids=ud.case_id)
def test_wrong_gradients_fail_the_comparator(fc):
    """The fp64 gradients of a wrong rollout fail util_oracle's rule against the correct ones (W at its own scale, factor 1):
      - the undisturbed rollout (W ignored) and "w_before_step" on at least one parameter (in fact on every weight) and on dJc/dx;
      - "w_on_costs" adds W to the four cost integrals, a constant offset: its gradients are the correct ones, and it is the logged
        means of Q and W that the rule rejects (the GPU test compares every entry of cs under the same rule; the offsets of L and HJt
        average out below their fp32 error on the larger batches);
      - "ctrl_undisplaced" moves only the logged controls, which neither Jc nor the logged costs read: nothing a training call returns can
        tell it apart, so its gradients, Jc and cs are asserted EQUAL (its teeth are the forward test's, tests/test_disturb_cpu.py)."""
    family, case = fc
    data = ud.case_data(case)
    r64, r32 = ut.case_grads(case, torch.float64, w_scale=W_SCALE), ut.case_grads(case, torch.float32, w_scale=W_SCALE)
    want64, want32 = ut.with_x(r64), ut.with_x(r32)
    assert not ut.failures(ut.compare_grads(want32, want64, want32))
    J0, g0, gx0 = ul.autograd_grads(um.case_sd(case), um.spec(case), data["x"], case.tspan, case.nt, case.stepper, case.alph, torch.float64)
    plain = dict(g0, x=gx0)
    bad = ut.failures(ut.compare_grads(plain, want64, want32))
    assert [k for k in bad if k != "x"] and "x" in bad, (case.id, "undisturbed", sorted(bad))
    wrong = ut.case_grads(case, torch.float64, mutation="w_before_step", w_scale=W_SCALE)
    bad = ut.failures(ut.compare_grads(ut.with_x(wrong), want64, want32))
    assert [k for k in bad if k != "x"] and "x" in bad, (case.id, "w_before_step", sorted(bad))
    wrong = ut.case_grads(case, torch.float64, mutation="w_on_costs", w_scale=W_SCALE)
    assert not ut.failures(ut.compare_grads(ut.with_x(wrong), want64, want32))
    for c in (5, 6):
        assert not uo.compare(wrong["cs"][c], r64["cs"][c], r32["cs"][c])[0], (case.id, "w_on_costs", c)
    wrong = ut.case_grads(case, torch.float64, mutation="ctrl_undisplaced", w_scale=W_SCALE)
    assert wrong["Jc"] == r64["Jc"] and torch.equal(wrong["cs"], r64["cs"]) and torch.equal(wrong["gx"], r64["gx"])
    assert all(torch.equal(wrong["grads"][k], r64["grads"][k]) for k in r64["grads"])
    assert set(ud.MUTATIONS) == {"w_before_step", "w_on_costs", "ctrl_undisplaced"}           # (a new mutation needs its own lines above)


def test_symbol_is_exported_and_declared(L):
    assert hasattr(L, "nocf_rollout_record_disturbed_f32")
    f = train._disturbed_entry(L)
    assert f is not None and f.restype is C.c_int and len(f.argtypes) == 19
    with open(entry.REPO + "/include/nocf.h") as fh:
        text = " ".join(fh.read().split())
    proto = ("int nocf_rollout_record_disturbed_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, const float* W, int64_t n, "
             "double t0, double t1, int32_t nt, int32_t stepper, const float* alph, float* z_out, float* persample, float* cost_sums, "
             "float* s_all, float* act_rec, int32_t* recorded, void* workspace, size_t workspace_bytes, void* stream);")
    assert proto in text
    # ... which is nocf_rollout_record_act_f32's with W behind x
    act = proto.replace("nocf_rollout_record_disturbed_f32", "nocf_rollout_record_act_f32").replace(" const float* W,", "")
    assert act in text
    assert L.nocf_version() == 113


def _call(L, phi, prob, n=4, nt=2, W=1, x=1, stepper=4, ws=1, s_all=1, z_out=1, alph=1, act=0, wsb=1 << 30, rec=None):
    p = C.c_void_p(0x1000)
    nz = lambda f: p if f else None                                  # noqa: E731
    a = (C.c_float * 6)(1, 1, 1, 1, 1, 1) if alph else None
    return train._disturbed_entry(L)(C.byref(phi), C.byref(prob), nz(x), nz(W), n, 0.0, 1.0, nt, stepper, a,
                                     nz(z_out), p, p, nz(s_all), nz(act), rec, nz(ws), wsb, None)


def test_abi_refusals_need_no_device(L):
    """every refusal returns before a launch: the pointers are never dereferenced"""
    phi = _lib.NocfPhi()
    phi.d, phi.m, phi.nTh, phi.r = 4, 16, 2, 5
    for k in ("K0", "b0", "K", "b", "w", "A", "cw", "cb_dev"):
        setattr(phi, k, 0x1000)
    prob, keep = na.Cross2D(torch.zeros(4))._c_struct("cpu")
    assert _call(L, phi, prob, W=0) == -1                     # NOCF_E_NULL
    assert _call(L, phi, prob, s_all=0) == -1
    assert _call(L, phi, prob, z_out=0) == -1
    assert _call(L, phi, prob, x=0) == -1
    assert _call(L, phi, prob, alph=0) == -1
    assert _call(L, phi, prob, ws=0) == -1
    assert _call(L, phi, prob, n=0) == -2                     # NOCF_E_SHAPE
    assert _call(L, phi, prob, nt=0) == -2
    assert _call(L, phi, prob, stepper=3) == -5               # NOCF_E_STEPPER
    assert _call(L, phi, prob, wsb=16) == -4                  # NOCF_E_WORKSPACE
    rec = C.c_int32(7)                                        # a refused call reports that nothing was recorded
    assert _call(L, phi, prob, W=0, act=1, rec=C.byref(rec)) == -1 and rec.value == 0
    rec.value = 7
    assert _call(L, phi, prob, n=0, act=1, rec=C.byref(rec)) == -2 and rec.value == 0


def test_python_argument_errors_need_no_device():
    case = ud.CASES[0][1]
    net = um.make_net(case, "cpu")
    prob = um.make_problem(case)
    n, nt, d = 3, case.nt, case.d
    x = um.candidates(case, n)
    W = torch.zeros(nt, n, d)
    ts = list(case.tspan)
    with pytest.raises(RuntimeError, match="single precision only"):
        na.disturbed_ocflow_train(x.double(), net, prob, ts, nt, W)
    with pytest.raises(RuntimeError, match="single precision only"):
        na.disturbed_ocflow_train(x, net, prob, ts, nt, W.double())
    net64 = um.make_net(case, "cpu").double()
    with pytest.raises(RuntimeError, match="single precision only"):
        na.disturbed_ocflow_train(x, net64, prob, ts, nt, W)
    for bad in (W[:-1], W[:, :-1], W[:, :, :-1], W[0]):
        with pytest.raises(ValueError, match="nt-by-nex-by-d"):
            na.disturbed_ocflow_train(x, net, prob, ts, nt, bad)
    with pytest.raises(ValueError):
        na.disturbed_ocflow_train(x[0], net, prob, ts, nt, W)
    with pytest.raises(ValueError):
        na.disturbed_ocflow_train(x[:, :-1], net, prob, ts, nt, W[:, :, :-1])
    with pytest.raises(ValueError):
        na.disturbed_ocflow_train(x, net, prob, ts, 0, W)
    with pytest.raises(ValueError):
        na.disturbed_ocflow_train(x, net, prob, ts, nt, W, stepper="rk2")
    with pytest.raises(ValueError):
        na.disturbed_ocflow_train(x, net, prob, ts, nt, W, alph=[1.0] * 5)
    with pytest.raises(NotImplementedError, match="dJ/dW"):
        na.disturbed_ocflow_train(x, net, prob, ts, nt, W.clone().requires_grad_(True))
    # good arguments on the CPU: the hot path runs on the device only
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.disturbed_ocflow_train(x, net, prob, ts, nt, W)
    assert all(p.grad is None for p in net.parameters())
