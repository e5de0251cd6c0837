"""CPU: the disturbed rollout's restatement (tests/util_disturb.py) against the pinned oracle, the screen of its cases, the comparator's
teeth on three wrong restatements, brownian_disturbances, and the C entry point's export and refusals (no device needed)."""
import ctypes as C
import math

import pytest
import torch

import __graft_entry__ as entry
import neuraloc_amd as na
from neuraloc_amd import _lib, disturb
import util_disturb as ud
import util_lane as ul
import util_mono as um
from oracle import ocflow_oracle as orc


@pytest.fixture(scope="module")
def L():
    entry.build()
    return _lib.lib()


def _params(case, dtype):
    return orc.PhiParams.from_state_dict({k: v.clone() for k, v in um.case_sd(case).items()}, dtype=dtype), um.spec(case).to(dtype)


# one case per problem class, both steppers, t0 = 0.25
ZERO_CASES = [ud._C("cross2d", 4, 16, 5, "softcorridor", "eval", 3, "rk4", 3, ud.T2),
              ud._C("swarm", 15, 33, 10, "blocks", "train", 3, "rk1", 3, ud.T2),
              ud._C("quad", 12, 32, 10, None, "eval", 3, "rk4", 2, ud.T2),
              ud._C("quad", 24, 48, 10, None, "eval", 2, "rk1", 3, ud.T2),
              ud._C("cross2d", 6, 16, 5, "hardcorridor", "train", 3, "rk1", 2, ud.T2),
              ud._C("swarm", 15, 16, 10, "blocks", "eval", 2, "rk4", 2, ud.T2)]


@pytest.mark.parametrize("case", ZERO_CASES, ids=lambda c: c.id)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_zero_disturbance_is_the_oracle_bitwise(case, dtype):
    P, S = _params(case, dtype)
    x = um.candidates(case, case.n).to(dtype)
    W = torch.zeros(case.nt, case.n, case.d)
    with torch.no_grad():
        got = ud.restate(P, S, x, W, list(case.tspan), case.nt, case.stepper, case.alph)
        tab = orc.persample_table(x, P, S, list(case.tspan), case.nt, case.stepper, case.alph)
        zF, cF = orc.rollout(x, P, S, list(case.tspan), case.nt, case.stepper, case.alph, intermediates=True)
    assert torch.equal(got["table"], tab)
    assert torch.equal(got["zFull"], zF) and torch.equal(got["ctrlFull"], cF)
    assert torch.equal(got["z"], zF[:, :, -1])


@pytest.mark.parametrize("case", [ZERO_CASES[0], ZERO_CASES[2], ud._C("swarm", 15, 33, 10, "blocks", "eval", 3, "rk4", 4)], ids=lambda c: c.id)
@pytest.mark.parametrize("k", [0, 1, -1])
def test_one_nonzero_step_is_two_chained_rollouts(case, k):
    k = k % case.nt
    P, S = _params(case, torch.float32)
    x = um.candidates(case, case.n)
    W = torch.zeros(case.nt, case.n, case.d)
    W[k] = ud.disturbances(case, case.n)[k] * 4.0
    with torch.no_grad():
        got = ud.restate(P, S, x, W, list(case.tspan), case.nt, case.stepper, case.alph)
        want = ud.chained(P, S, x, W, k, list(case.tspan), case.nt, case.stepper, case.alph)
    assert ud.state_close(got["zFull"], want)
    assert float((got["zFull"][:, :case.d, k + 1] - want[:, :case.d, k + 1] ).abs().max()) <= 1e-6
    assert float(W[k].abs().max()) > 10 * ud.STATE_ATOL            # (the displacement itself is far above the tolerance)


@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
def test_cases_pass_the_screen_and_exercise_their_physics(fc):
    family, case = fc
    data = ud.case_data(case)
    assert 8 * data["screened"] <= data["total"]
    assert data["x"].shape == (case.n, case.d) and data["W"].shape == (case.nt, case.n, case.d)
    assert not um.near_edge(case, data["r64"]["stages"]).any()
    r = case.rad
    assert 0.0 < float(data["W"].abs().max()) < r                  # sigma = 0.05 r: displacements well inside an agent's radius
    assert not ul.failures(ud.compare(data["r32"], data["r64"], data["r32"]))
    assert not um.physics_gaps(case, data["r64"])
    # the dispatcher's choice of family, mirrored: lane, then one-CU, then per-tile
    lane = ul.lane_forward_eligible(case.nTh, case.m, case.d, case.spec_kind, case.n_agents)
    mono = um.mono_plan_ok(case.nTh, case.m, case.d, case.r, case.n_agents)
    assert family.split("-")[0] == ("lane" if lane else ("mono" if mono else "tile"))


def test_the_new_instantiations_are_all_reached():
    lanes = {ul.lane_shape(c.m, c.d) for f, c in ud.CASES if f == "lane"}
    assert lanes == {(16, 8), (32, 8), (32, 32)}
    monos = {um.mono_shape(c.m, c.d) for f, c in ud.CASES if f == "mono"}
    assert monos == {(8, 1), (4, 1)}
    assert {c.kind for f, c in ud.CASES if f == "mono"} == {"quad", "cross2d"}          # singlequad's wave-local path and the generic one
    assert {f for f, _ in ud.CASES} == set(ud.KERNEL)
    assert {c.stepper for _, c in ud.CASES} == {"rk4", "rk1"} and {c.tspan for _, c in ud.CASES} == {ud.T1, ud.T2}
    assert {c.mode for _, c in ud.CASES} == {"eval", "train"}


@pytest.mark.parametrize("mutation", ud.MUTATIONS)
def test_wrong_restatements_fail_the_comparator(mutation):
    for family, case in (ud.CASES[1], ud.CASES[3]):
        data = ud.case_data(case)
        wrong = ud.case_restate(case, data["x"].double(), data["W"], torch.float64, mutation)
        assert ul.failures(ud.compare(wrong, data["r64"], data["r32"])), (mutation, case.id)


def test_brownian_disturbances():
    nt, n, d, sigma = 8, 512, 3, 0.3
    g = torch.Generator().manual_seed(5)
    W = na.brownian_disturbances(nt, n, d, sigma, (0.25, 1.0), generator=g)
    assert W.shape == (nt, n, d) and W.dtype == torch.float32 and W.is_contiguous()
    g = torch.Generator().manual_seed(5)
    assert torch.equal(W, na.brownian_disturbances(nt, n, d, sigma, (0.25, 1.0), generator=g))
    g = torch.Generator().manual_seed(6)
    assert not torch.equal(W, na.brownian_disturbances(nt, n, d, sigma, (0.25, 1.0), generator=g))
    # sample variance of 4096 draws against sigma^2 h: the standard error of a Gaussian's sample variance is var sqrt(2 / (N - 1))
    h = 0.75 / nt
    v = W.flatten()[:4096].double()
    var, want = float(v.var()), sigma * sigma * h
    assert abs(var - want) <= 5.0 * want * math.sqrt(2.0 / 4095)
    assert abs(float(v.mean())) <= 5.0 * math.sqrt(want / 4096)
    # a [d] sigma scales per coordinate; the mask zeroes coordinates
    g = torch.Generator().manual_seed(5)
    Wv = na.brownian_disturbances(nt, n, d, torch.tensor([0.3, 0.6, 0.0]), (0.25, 1.0), generator=g)
    assert torch.equal(Wv[..., 0], W[..., 0]) and torch.allclose(Wv[..., 1], 2 * W[..., 1]) and not Wv[..., 2].any()
    g = torch.Generator().manual_seed(5)
    Wm = na.brownian_disturbances(nt, n, d, sigma, (0.25, 1.0), generator=g, mask=torch.tensor([0, 1, 1]))
    assert not Wm[..., 0].any() and torch.equal(Wm[..., 1:], W[..., 1:])
    with pytest.raises(ValueError):
        na.brownian_disturbances(0, n, d, sigma)
    with pytest.raises(ValueError):
        na.brownian_disturbances(nt, n, d, torch.ones(d + 1))
    with pytest.raises(ValueError):
        na.brownian_disturbances(nt, n, d, sigma, mask=torch.ones(d + 1))


def test_path_statistics():
    v = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0], [2.0, 2.0, 2.0, 2.0, 2.0]])
    st = disturb.path_statistics(v)
    assert torch.allclose(st["mean"], torch.tensor([3.0, 2.0])) and torch.allclose(st["q50"], torch.tensor([3.0, 2.0]))
    assert torch.allclose(st["std"], torch.tensor([math.sqrt(2.5), 0.0])) and torch.allclose(st["q05"], torch.tensor([1.2, 2.0]))
    assert torch.allclose(st["q95"], torch.tensor([4.8, 2.0]))


def test_symbol_is_exported_and_declared(L):
    assert hasattr(L, "nocf_rollout_disturbed_f32")
    assert disturb._entry(L) is not None
    with open(entry.REPO + "/include/nocf.h") as f:
        assert "int nocf_rollout_disturbed_f32(" in f.read()
    assert L.nocf_version() == 113


def _call(L, phi, prob, n=4, nt=2, W=1, x=1, stepper=4, ws=1):
    p = C.c_void_p(0x1000)
    nz = lambda f: p if f else None
    alph = (C.c_float * 6)(1, 1, 1, 1, 1, 1)
    return disturb._entry(L)(C.byref(phi), C.byref(prob), nz(x), nz(W), n, 0.0, 1.0, nt, stepper, alph,
                             None, p, p, p, None, None, nz(ws), 1 << 30, None)


def test_abi_refusals_need_no_device(L):
    """every refusal returns before a launch: the pointers are never dereferenced"""
    phi = _lib.NocfPhi()
    phi.d, phi.m, phi.nTh, phi.r = 4, 16, 2, 5
    for k in ("K0", "b0", "K", "b", "w", "A", "cw", "cb_dev"):
        setattr(phi, k, 0x1000)
    prob, keep = na.Cross2D(torch.zeros(4))._c_struct("cpu")
    assert _call(L, phi, prob, W=0) == -1                     # NOCF_E_NULL
    assert _call(L, phi, prob, x=0) == -1
    assert _call(L, phi, prob, ws=0) == -1
    assert _call(L, phi, prob, n=0) == -2                     # NOCF_E_SHAPE
    assert _call(L, phi, prob, nt=0) == -2
    assert _call(L, phi, prob, stepper=3) == -5               # NOCF_E_STEPPER
    p = C.c_void_p(0x1000)
    alph = (C.c_float * 6)(1, 1, 1, 1, 1, 1)
    # cost_means without cost_sums, zFull without ctrlFull
    f = disturb._entry(L)
    assert f(C.byref(phi), C.byref(prob), p, p, 4, 0.0, 1.0, 2, 4, alph, None, p, None, p, None, None, p, 1 << 30, None) == -1
    assert f(C.byref(phi), C.byref(prob), p, p, 4, 0.0, 1.0, 2, 4, alph, None, p, p, p, p, None, p, 1 << 30, None) == -1
    assert f(C.byref(phi), C.byref(prob), p, p, 4, 0.0, 1.0, 2, 4, alph, None, p, p, p, None, None, p, 16, None) == -4      # NOCF_E_WORKSPACE


def test_python_argument_errors():
    case = ud.CASES[0][1]
    net = um.make_net(case, "cpu")
    prob = um.make_problem(case)
    x = um.candidates(case, 3)
    W = torch.zeros(case.nt, 3, case.d)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.disturbed_rollout(x, net, prob, case.nt, W)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.noise_study(x, net, prob, case.nt, 0.1, 4)
    with pytest.raises(RuntimeError, match="single precision only"):
        na.disturbed_rollout(x.double(), net, prob, case.nt, W)
    with pytest.raises(RuntimeError, match="single precision only"):
        na.disturbed_rollout(x, net, prob, case.nt, W.double())
