"""The one-CU sweep's case lists (tests/util_mono.py) without a GPU: the dispatcher's mirror at its boundaries, the lists reach every
instantiation of the one-CU kernels with the widths, inputs, ranks, batches, steppers, spans and problems they claim, every case exercises
its physics in fp64 and keeps clear of the screen's margins, and the comparator rejects eight wrong restatements."""
import pytest
import torch

import util_mono as um
from oracle import ocflow_oracle as orc

SMALL = [c for c in um.FORWARD if c.n < um.BIG]
KINDS = {"cross2d": orc.KIND_CROSS2D, "swarm": orc.KIND_SWARM, "quad": orc.KIND_QUAD}


def test_dispatch_mirror_boundaries():
    assert [um.mono_shape(m, 12)[0] for m in (1, 32, 33, 64, 65, 96, 97, 128)] == [2, 2, 4, 4, 6, 6, 8, 8]
    assert [um.mono_shape(64, d)[1] for d in (12, 14, 15, 16, 24, 30, 31, 32)] == [1, 1, 1, 2, 2, 2, 2, 3]
    ok = um.mono_forward_eligible
    assert ok(2, 128, 12, 10, orc.KIND_QUAD, 1) and not ok(2, 129, 12, 10, orc.KIND_QUAD, 1)
    assert ok(2, 64, 30, 10, orc.KIND_CROSS2D, 15) and not ok(2, 64, 32, 10, orc.KIND_CROSS2D, 16)              # d + 1 = 33
    assert not ok(3, 64, 12, 10, orc.KIND_QUAD, 1) and not ok(2, 64, 16, 17, orc.KIND_CROSS2D, 8)               # nTh = 3, r = 17
    # the lane kernel wins where it is eligible: point agents of m <= 32; quadcopters never take it
    assert not ok(2, 32, 14, 10, orc.KIND_CROSS2D, 7) and ok(2, 32, 14, 10, orc.KIND_CROSS2D, 7, lane=False) and ok(2, 33, 14, 10, orc.KIND_CROSS2D, 7)
    assert ok(2, 32, 12, 10, orc.KIND_QUAD, 1) and ok(2, 1, 12, 1, orc.KIND_QUAD, 1) and not ok(2, 64, 12, 10, orc.KIND_QUAD, 1, mono=False)
    # adjoint: KBM in {4, 6, 8}; record: whole 16-blocks of more than 32 units
    assert um.mono_adjoint_eligible(2, 33, 12, 10, 1) and not um.mono_adjoint_eligible(2, 32, 12, 10, 1)
    assert um.mono_adjoint_eligible(2, 128, 24, 16, 2) and not um.mono_adjoint_eligible(2, 129, 24, 16, 2)
    assert um.mono_record_eligible(2, 48, 24, 10, 12) and not um.mono_record_eligible(2, 49, 24, 10, 12) and not um.mono_record_eligible(2, 32, 12, 10, 1)
    assert um.mid_grad_rows(16384) == 1024 and um.mid_grad_rows(16385) == 1024 and um.mid_grad_rows(17) == 2
    assert sorted(um.FORWARD_INSTANTIATIONS) == sorted((a, b, r) for a, b in um.FORWARD_SHAPES for r in (False, True))
    assert len(um.FORWARD_INSTANTIATIONS) == 14 and len(um.ADJOINT_SHAPES) == 6


def test_agent_caps_and_lds_limits_never_bind():
    """with d + 1 <= 16 / 32 a problem class gives at most 7 / 15 agents (MONO_NAG is 8 / 16), the state rows fit MONO_ZLD and every
    instantiation fits its LDS limit: over every admissible d the plan depends on (m, d, r, nTh) alone"""
    for d in range(1, 32):
        kbd = um.cdiv(d + 1, 16)
        for ad in (2, 3, 12):
            if d % ad == 0:
                assert d // ad <= (7 if kbd == 1 else 15) < um.mono_nag(kbd), (d, ad)
                for m in (1, 33, 65, 128)[kbd - 1:]:                 # (no (2, 2) instantiation: m <= 32 needs d + 1 <= 16)
                    assert um.mono_plan_ok(2, m, d, 1, d // ad) and um.mono_plan_ok(2, m, d, min(16, d + 1), d // ad, bwd=True), (d, ad, m)
        assert -(-(d + 4) // 4) * 4 <= um.mono_zld(kbd)
    assert all(31 % ad for ad in (2, 3, 12))                               # d + 1 = 32 has no problem class
    assert not um.mono_plan_ok(2, 32, 24, 10, 2)                           # two quadcopters with m <= 32: the per-tile kernel
    for kbm, kbd in um.FORWARD_SHAPES:
        assert 4 * um.mono_fwd_lds_floats(kbm, kbd) <= 96 * 1024 and 4 * um.mono_bwd_lds_floats(kbm, kbd) <= 160 * 1024
    assert 4 * um.mono_fwd_lds_floats(8, 2) > 64 * 1024                    # (the dynamic-LDS attribute is needed: more than the static limit)


def test_forward_list_covers_every_instantiation():
    for c in um.FORWARD:
        assert um.mono_forward_eligible(c.nTh, c.m, c.d, c.r, KINDS[c.kind], c.n_agents), c.id
    assert {c.shape for c in um.FORWARD} == set(um.FORWARD_SHAPES)
    for shape in um.FORWARD_SHAPES:
        fw = [c for c in um.FORWARD if c.shape == shape]
        small = [c for c in fw if c.n < um.BIG]
        assert {c.n for c in small} >= {1, 15, 16, 17} and any(c.n > 17 and c.n % 16 not in (0, 1, 15) for c in small), shape
        big = um.big_case(shape)
        assert big.n > 16384 and big.n % 16 != 0, shape                     # more than 1024 tiles, ragged
        assert {c.stepper for c in fw} == {"rk4", "rk1"} and {c.tspan for c in fw} == {um.T1, um.T2}, shape
        assert {c.nt for c in fw} == {1, 7, 9} and {c.mode for c in fw} == {"eval", "train"}, shape
    assert {c.m for c in um.FORWARD if c.kind != "quad"} >= {33, 48, 49, 64, 65, 80, 81, 96, 97, 100, 127, 128}
    assert {c.m for c in um.FORWARD} >= {33, 48, 49, 64, 65, 80, 81, 96, 97, 100, 127, 128}
    assert {c.m for c in um.FORWARD if c.kind == "quad" and c.m <= 32} == {1, 16, 17, 32}
    assert {c.d + 1 for c in um.FORWARD if c.shape[1] == 1} == {13, 15, 16}
    assert {c.d + 1 for c in um.FORWARD if c.shape[1] == 2} == {17, 25, 31}
    for kbd in (1, 2):
        cs = [c for c in um.FORWARD if c.shape[1] == kbd]
        assert any(c.r == 1 for c in cs) and any(c.r == 10 for c in cs) and any(c.r == min(16, c.d + 1) for c in cs), kbd
    assert {c.r for c in um.FORWARD} >= {1, 10, 13, 15, 16}


def test_forward_list_covers_every_problem_class():
    kinds = {(c.kind, c.obstacle) for c in um.FORWARD}
    assert kinds == {("cross2d", None), ("cross2d", "softcorridor"), ("cross2d", "hardcorridor"), ("swarm", "blocks"), ("quad", None)}
    assert {c.n_agents for c in um.FORWARD if c.kind == "swarm"} == {5, 10}
    assert {c.n_agents for c in um.FORWARD if c.kind == "quad"} == {1, 2}
    assert any((c.mass, c.grav) != (1.0, 9.81) for c in um.FORWARD if c.kind == "quad")
    assert any(c.alph_Q == 0.0 and c.obstacle is not None for c in um.FORWARD)
    assert any(c.alph_W == 0.0 and c.n_agents >= 2 for c in um.FORWARD)
    for kbd in (1, 2):                                                      # the angle cases: at one and at two craft; beyond 1000 once
        assert any(c.angles == "quadrants" and c.n >= 16 and c.shape[1] == kbd for c in um.FORWARD)
    assert any(c.angles == "quadrants" and c.m <= 32 for c in um.FORWARD)
    assert any(c.angles == "big" and c.n >= 16 and c.tspan == um.T1 for c in um.FORWARD)
    assert len({c.id for c in um.FORWARD}) == len(um.FORWARD)


def test_adjoint_list_covers_every_instantiation():
    for c in um.ADJOINT:
        assert um.mono_forward_eligible(c.nTh, c.m, c.d, c.r, KINDS[c.kind], c.n_agents), c.id
        assert um.mono_adjoint_eligible(c.nTh, c.m, c.d, c.r, c.n_agents) and c.mode == "train", c.id
    assert {c.shape for c in um.ADJOINT} == set(um.ADJOINT_SHAPES)
    for kbm in (4, 6, 8):
        cs = [c for c in um.ADJOINT if c.shape[0] == kbm]
        assert any(um.mono_record_eligible(c.nTh, c.m, c.d, c.r, c.n_agents) for c in cs), kbm
        assert any(c.m % 16 != 0 for c in cs), kbm
    assert {c.stepper for c in um.ADJOINT} == {"rk4", "rk1"} and {c.tspan for c in um.ADJOINT} == {um.T1, um.T2}
    assert any(c.n_total not in (None, c.n) for c in um.ADJOINT)
    assert any(c.n > 16384 and c.n % 16 != 0 and c.nt == 2 for c in um.ADJOINT)
    assert any(c.kind == "quad" and c.n_agents == 2 for c in um.ADJOINT)
    assert any(not c.act_rec and c.m % 16 == 0 for c in um.ADJOINT)
    assert len({c.id for c in um.ADJOINT}) == len(um.ADJOINT)


def test_segment_list():
    shapes = {c.shape for c in um.SEGMENTS}
    assert (8, 1) in shapes and any(s[1] == 2 for s in shapes)
    assert um.SEGMENTS[0].kind == "quad" and any(c.kind == "swarm" for c in um.SEGMENTS)
    assert any(c.kind == "cross2d" and c.shape[1] == 2 for c in um.SEGMENTS)
    for c in um.SEGMENTS:
        assert um.mono_forward_eligible(c.nTh, c.m, c.d, c.r, KINDS[c.kind], c.n_agents, lane=False), c.id
    assert [s[0] for s in um.SEGMENT_LAYOUTS] == [1, 3, 16]
    for nseg, rows, last in um.SEGMENT_LAYOUTS:
        n = (nseg - 1) * rows + last
        assert rows % 16 == 0 and 0 < last < rows and n % 16 != 0 and n % rows != 0
        t0s, nts, slot0s = um.segment_plan(nseg)
        assert min(nts) >= 1 and min(slot0s) >= 0 and all(t < 1.0 for t in t0s)
        assert nseg == 1 or (len(set(t0s)) == nseg and len(set(nts)) > 1 and len(set(slot0s)) > 1)


@pytest.mark.parametrize("case", um.FORWARD + um.ADJOINT, ids=lambda c: c.id)
def test_cases_exercise_their_physics(case):
    """Q / W nonzero where they are on and exactly zero where off, both craft interact (W > 0 in some sample, = 0 in another), the angle
    cases visit all eight quadrant / sign pairs and both sides of 1000 (read from the recorded fp64 stages); the case finds its n starts among
    n + max(16, n / 2) candidates, none of their evaluated states within the screen's margins; the fp32 restatement passes its own comparator"""
    D = um.case_data(case)
    assert D["x"].shape == (case.n, case.d)
    assert um.physics_gaps(case, D["r64"]) == []
    assert not bool(um.near_edge(case, D["r64"]["stages"]).any())
    assert um.failures(um.compare_forward(D["r32"], D["r64"], D["r32"])) == {}


def test_two_craft_interact():
    for c in SMALL + um.ADJOINT:
        if c.kind == "quad" and c.n_agents == 2 and c.n >= 16:
            w = um.case_data(c)["r64"]["table"][:, 6]
            assert bool((w > 0).any()), c.id
    both = [c for c in um.FORWARD if c.kind == "quad" and c.n_agents == 2 and c.n >= um.BIG]
    assert both
    for c in both:                                                           # in the large batch the 2r edge lies inside the batch
        dist = um.quad_pair_distance(um.case_data(c)["r64"]["stages"])
        assert bool((dist < 2 * um.QUAD_R).any()) and bool((dist > 2 * um.QUAD_R).any()), c.id


def _teeth(mutation, cases):
    """-> the cases on which the mutated fp64 oracle fails the comparator"""
    caught = []
    for c in cases:
        D = um.case_data(c)
        bad = um.oracle_forward(c, D["x"].double(), torch.float64, mutation)
        if um.failures(um.compare_forward(bad, D["r64"], D["r32"])):
            caught.append(c)
    return caught


@pytest.mark.parametrize("mutation", ["rank_minus_one", "last_hidden_dropped", "k_block_dropped"])
def test_comparator_rejects_a_wrong_bound_at_every_width(mutation):
    """A'A from r - 1 rows of A, the last hidden unit dropped, the last hidden k-block dropped: caught at every KBM and both KBD"""
    caught = _teeth(mutation, SMALL)
    assert {c.shape for c in caught} == set(um.FORWARD_SHAPES), (mutation, [c.id for c in caught])


def test_comparator_rejects_wrong_time_and_threshold():
    assert _teeth("time_from_zero", [c for c in SMALL if c.tspan[0] != 0.0])
    assert _teeth("train_threshold_in_eval", [c for c in SMALL if c.mode == "eval" and c.alph_W != 0.0 and c.n_agents >= 2 and c.kind != "quad"])


def test_comparator_rejects_wrong_quadcopter_physics():
    """the sine's sign flipped in one quadrant: caught on every angle case, the one whose angles pass 1000 (where the fp32 restatement itself
    has lost 1e-4 of the angle and the tolerance has grown with it) included; the second craft dropped from W and the pair distance taken
    over all 12 coordinates: caught at two craft"""
    ang = [c for c in SMALL if c.angles != "small"]
    assert {c.angles for c in ang} == {"quadrants", "big"}
    assert _teeth("sin_sign_in_one_quadrant", ang) == ang
    two = [c for c in SMALL if c.kind == "quad" and c.n_agents == 2 and c.n >= 16]
    for mutation in ("second_craft_dropped_from_W", "quad_pair_distance_over_all_12"):
        assert _teeth(mutation, two), mutation
    assert set(um.MUTATIONS) == {"rank_minus_one", "last_hidden_dropped", "time_from_zero", "train_threshold_in_eval", "sin_sign_in_one_quadrant",
                                 "second_craft_dropped_from_W", "k_block_dropped", "quad_pair_distance_over_all_12"}


def test_oracle_activations_are_the_oracles_grad_phi():
    """the record's reference: its grad section is phi_grad bit for bit, and the other four rebuild it"""
    case = um.ADJOINT[0]
    D = um.case_data(case)
    s = torch.nn.functional.pad(D["x"], (0, 1), value=0.3).unsqueeze(0)
    a64, a32 = um.oracle_activations(case, s)
    P = orc.PhiParams.from_state_dict(um.case_sd(case), dtype=torch.float64)
    assert torch.equal(a64["grad"][0], orc.phi_grad(P, s[0].double()))
    assert a64["u0"].shape == (1, case.n, case.m) and a32["grad"].shape == (1, case.n, case.d + 1) and a32["a"].dtype == torch.float32
    g = (a64["tanh_o"][0] * a64["a"][0]) @ P.K[0] + s[0].double() @ (P.A.t() @ P.A) + P.cw
    assert float((g - a64["grad"][0]).abs().max()) <= 1e-12 * float(g.abs().max())
    q = a64["u0"][0] @ P.K[1].t() + P.b[1]
    assert float((torch.tanh(q) - a64["tanh_q"][0]).abs().max()) <= 1e-14
