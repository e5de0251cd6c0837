"""CPU: the zero-order-hold rollout's restatement (tests/util_hold.py) checked against the oracle where the two must agree, the screen's
cap on every case, the comparator's teeth on the wrong restatements, every Python refusal of neuraloc_amd.hold, and the evalOC parser."""
import pytest
import torch

import neuraloc_amd as na
import util_hold as uh
import util_lane as ul
import util_mono as um
from oracle import ocflow_oracle as orc


def _params(case, dtype=torch.float64):
    P = orc.PhiParams.from_state_dict({k: v.clone() for k, v in um.case_sd(case).items()}, dtype=dtype)
    return P, um.spec(case).to(dtype)


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


RK1 = [fc for fc in uh.CASES if fc[1].stepper == "rk1"]


@pytest.mark.parametrize("fc", RK1, ids=uh.case_id)
def test_hold_1_under_rk1_is_the_closed_loop(fc):
    """one stage per step and a sample at every step: the held rollout IS oracle.rollout, except for the HJB column"""
    case = fc[1]
    assert {c.kind for _, c in RK1} >= {"cross2d", "quad"}
    P, S = _params(case)
    x = um.candidates(case, case.n).double()
    with torch.no_grad():
        got = uh.restate(P, S, x, None, 1, list(case.tspan), case.nt, "rk1", case.alph)
        zF, cF = orc.rollout(x, P, S, list(case.tspan), case.nt, "rk1", case.alph, intermediates=True)
    d = case.d
    assert _rel(got["zFull"][:, :d], zF[:, :d]) <= 1e-12
    for col in (d, d + 2, d + 3):                                      # L, Q, W
        assert _rel(got["zFull"][:, col], zF[:, col]) <= 1e-12, col
    assert bool((got["zFull"][:, d + 1] == 0).all()) and bool((zF[:, d + 1, -1] > 0).all())
    # the control applied over step k is the one the oracle evaluates at x_k: its slot k + 1 holds the control at x_{k+1}
    with torch.no_grad():
        c0 = orc.prob_ctrls(S, x, orc.phi_grad(P, torch.nn.functional.pad(x, [0, 1, 0, 0], value=case.tspan[0]))[:, :d])
    assert _rel(got["ctrlFull"][:, :, 1], c0) <= 1e-12


def test_open_loop_without_obstacle_is_a_straight_line():
    fam, case = uh.GROUP_II[2]
    assert case.obstacle is None and case.kind == "cross2d"
    P, S = _params(case)
    x = um.candidates(case, case.n).double()
    t0, t1 = case.tspan
    for K in (case.nt, case.nt + 3):
        with torch.no_grad():
            got = uh.restate(P, S, x, None, K, [t0, t1], case.nt, case.stepper, case.alph)
        c0 = got["ctrlFull"][:, :, 1]
        assert _rel(got["z"][:, :case.d], x + (t1 - t0) * c0) <= 1e-12
        assert all(torch.equal(got["ctrlFull"][:, :, k], c0) for k in range(1, case.nt + 1))


def test_quadcopter_L_is_the_reference_formula_at_the_sampling_instant():
    case = uh.GROUP_I[3][1]
    assert case.kind == "quad"
    P, S = _params(case)
    x = um.candidates(case, case.n).double()
    z = torch.cat((x, torch.zeros(case.n, 4, dtype=torch.float64)), 1)
    with torch.no_grad():
        smp = uh._sample(P, S, x, 0.3)
        out = uh.held_rhs(P, S, z, 0.3, smp)
        L, _, Q, W = orc.prob_LHQW(S, x, smp["p"])
        f = -orc.prob_gradpH(S, x, smp["p"])
    assert _rel(out[:, case.d], L.squeeze(1)) <= 1e-12
    assert _rel(out[:, :case.d], f) <= 1e-12                               # ... and so is f, where the angles are the sample's
    assert bool((out[:, case.d + 1:] == 0).all())


@pytest.mark.parametrize("fc", uh.CASES, ids=uh.case_id)
def test_the_screen_keeps_its_cap(fc):
    case = fc[1]
    assert case.n % (4 if fc[0] == "lane" else 16) != 0 or fc in uh.GROUP_I
    for ki, dist in uh.COMBOS:
        data = uh.case_data(case, uh.holds(case)[ki], dist)           # (asserts the cap and that every fp64 figure is finite)
        assert 8 * data["screened"] <= data["total"] == case.n + max(2, case.n // 8)
        assert data["x"].shape == (case.n, case.d)
        assert bool((data["r64"]["table"][:, 2] == 0).all()) and bool((data["r32"]["table"][:, 2] == 0).all())


def test_the_cases_reach_every_instantiation():
    lane = {ul.lane_shape(c.m, c.d) for f, c in uh.GROUP_II if f == "lane"}
    mono = {um.mono_shape(c.m, c.d) for f, c in uh.GROUP_II if f == "mono"}
    assert lane == set(ul.INSTANTIATIONS) and mono == set(um.FORWARD_SHAPES)
    for fam, c in uh.CASES:
        S = um.spec(c)
        if fam == "lane":
            assert ul.lane_forward_eligible(c.nTh, c.m, c.d, S.kind, c.n_agents)
        else:
            assert um.mono_forward_eligible(c.nTh, c.m, c.d, c.r, S.kind, c.n_agents)
            assert c.kind != "quad" or c.n_agents == 1
    assert {c.stepper for _, c in uh.CASES} == {"rk1", "rk4"} and {c.mode for _, c in uh.CASES} == {"eval", "train"}
    assert any(c.tspan == uh.T2 for _, c in uh.CASES)
    assert all(c.nt == 3 for _, c in uh.GROUP_II)                      # K = 2: a ragged last interval


# where each wrong restatement must show: the control's source needs W, re-sampling needs K > 1, the frozen f7..f9 a quadcopter
WHERE = {"ctrl_undisplaced": lambda c, K, dist: dist and K == 1,
         "resample_every_step": lambda c, K, dist: K == 2,
         "L_from_current_costate": lambda c, K, dist: True,
         "hjt_not_zeroed": lambda c, K, dist: True,
         "f_frozen_at_sample": lambda c, K, dist: c.kind == "quad"}


@pytest.mark.parametrize("mutation", uh.MUTATIONS)
def test_the_comparator_catches_every_wrong_restatement(mutation):
    caught = []
    for fam, case in uh.GROUP_I + uh.GROUP_III:
        for ki, dist in uh.COMBOS:
            K = uh.holds(case)[ki]
            if not WHERE[mutation](case, K, dist):
                continue
            data = uh.case_data(case, K, dist)
            wrong = uh.case_restate(case, data["x"], data["W"], K, torch.float32, mutation)
            bad = ul.failures(uh.compare(wrong, data["r64"], data["r32"]))
            if bad:
                caught.append((case.id, K, dist, sorted(bad)))
            # the right restatement in fp32 passes its own comparator
            assert not ul.failures(uh.compare(data["r32"], data["r64"], data["r32"]))
        if len(caught) >= 2:
            break
    print(mutation, caught)
    assert caught, f"{mutation} passes the comparator on every case"


def _cpu_net(case):
    return um.make_net(case, "cpu"), um.make_problem(case, "cpu")


def test_every_python_refusal_raises_before_a_device_is_touched():
    case = uh.GROUP_I[0][1]
    net, prob = _cpu_net(case)
    for p_ in net.parameters():
        p_.requires_grad_(False)
    x = um.candidates(case, 3)
    ts = list(case.tspan)
    # CPU tensors, float64
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.held_rollout(x, net, prob, ts, case.nt, 2)
    with pytest.raises(RuntimeError, match="single precision only"):
        na.held_rollout(x.double(), net, prob, ts, case.nt, 2)
    with pytest.raises(RuntimeError, match="single precision only"):
        na.held_rollout(x, net, prob, ts, case.nt, 2, W=torch.zeros(case.nt, 3, case.d, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="single precision only"):
        na.hold_study(x.double(), net, prob, case.nt)
    # hold < 1 or not an integer
    for bad in (0, -1, 1.0, 2.5, "2", True, None):
        with pytest.raises(ValueError, match="hold must be an integer >= 1"):
            na.held_rollout(x, net, prob, ts, case.nt, bad)
    with pytest.raises(ValueError, match="hold must be an integer >= 1"):
        na.hold_study(x, net, prob, case.nt, holds=(1, 0))
    # an ensemble
    ens = na.PhiEnsemble.from_members([net, net])
    with pytest.raises(NotImplementedError, match="PhiEnsemble"):
        na.held_rollout(x, ens, prob, ts, case.nt, 2)
    with pytest.raises(NotImplementedError, match="PhiEnsemble"):
        na.hold_study(x, ens, prob, case.nt)
    # n_total / group are training's
    with pytest.raises(NotImplementedError, match="n_total / group"):
        na.held_rollout(x, net, prob, ts, case.nt, 2, n_total=8)
    with pytest.raises(NotImplementedError, match="n_total / group"):
        na.held_rollout(x, net, prob, ts, case.nt, 2, group=object())
    # grad mode with anything that requires a gradient: an evaluation, as disturbed_rollout is
    with pytest.raises(NotImplementedError, match="autograd"):
        na.held_rollout(x.clone().requires_grad_(True), net, prob, ts, case.nt, 2)
    net.A.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="autograd"):
        na.held_rollout(x, net, prob, ts, case.nt, 2)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):      # (under no_grad the call gets as far as the device check)
        na.held_rollout(x, net, prob, ts, case.nt, 2)
    net.A.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="W requires a gradient"):
        na.held_rollout(x, net, prob, ts, case.nt, 2, W=torch.zeros(case.nt, 3, case.d, requires_grad=True))


@pytest.mark.parametrize("shape", [dict(m=129), dict(m=512), dict(nTh=3, m=48), dict(kind="cross2d", d=32, m=64)], ids=str)
def test_shapes_outside_the_two_families_are_refused(shape):
    kw = dict(kind="cross2d", d=4, m=16, nTh=2)
    kw.update(shape)
    case = um.MonoCase(kw["kind"], kw["d"], kw["m"], 4, None, "eval", 3, "rk4", 2, nTh=kw["nTh"])
    net, prob = _cpu_net(case)
    x = um.candidates(case, 3)
    with pytest.raises(NotImplementedError, match="lane.*one-CU"):
        na.held_rollout(x, net, prob, [0.0, 1.0], 2, 1)
    with pytest.raises(NotImplementedError, match="lane.*one-CU"):
        na.hold_study(x, net, prob, 2)


def test_a_quadcopter_problem_of_two_craft_is_refused():
    case = um.MonoCase("quad", 24, 64, 10, None, "eval", 3, "rk4", 2)
    net, prob = _cpu_net(case)
    with pytest.raises(NotImplementedError, match="2 craft"):
        na.held_rollout(um.candidates(case, 3), net, prob, [0.0, 1.0], 2, 1)


def test_evalOC_parses_as_before_without_the_flag():
    import evalOC
    args = evalOC.p.parse_args([])
    assert args.hold is None and args.noise is None and args.worst is None and args.nt == 50 and args.prec == "single"
    args = evalOC.p.parse_args(["--nt", "20", "--noise", "0.1", "--noise_paths", "8", "--do_shock"])
    assert args.hold is None and (args.nt, args.noise, args.noise_paths, args.do_shock) == (20, 0.1, 8, True)
    assert evalOC.p.parse_args(["--hold", "1,2,5"]).hold == "1,2,5" and evalOC.parse_holds("1,2,5") == [1, 2, 5]
    for bad in ("0", "1,x", "", "2,-1"):
        with pytest.raises(SystemExit, match="--hold"):
            evalOC.parse_holds(bad)
    with pytest.raises(SystemExit, match="single precision"):          # refused before anything runs or is written
        evalOC.main(["--hold", "2", "--prec", "double", "--save", "/nonexistent/never_made"])
