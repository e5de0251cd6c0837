"""The lane sweep's case list (tests/util_lane.py) without a GPU: it reaches every instantiation of the lane kernels with the batches,
steppers, spans and problems it claims, every case exercises its physics in fp64, and the comparator rejects four wrong restatements."""
import pytest
import torch

import util_lane as ul
from oracle import ocflow_oracle as orc

SMALL = [c for c in ul.FORWARD if c.n < ul.BIG]


def test_dispatch_mirror_boundaries():
    assert [ul.lane_shape(m, 4)[0] for m in (1, 7, 9, 16, 17, 31, 32)] == [16] * 4 + [32] * 3
    assert [ul.lane_shape(16, d)[1] for d in (2, 7, 8, 14, 15, 16, 30, 31)] == [8, 8, 16, 16, 16, 32, 32, 32]
    assert ul.lane_forward_eligible(2, 32, 31, orc.KIND_CROSS2D, 15) and not ul.lane_forward_eligible(2, 33, 8, orc.KIND_CROSS2D, 4)
    assert not ul.lane_forward_eligible(2, 16, 32, orc.KIND_CROSS2D, 16) and not ul.lane_forward_eligible(3, 16, 8, orc.KIND_CROSS2D, 4)
    assert ul.lane_forward_eligible(2, 16, 15, orc.KIND_SWARM, 5) and not ul.lane_adjoint_eligible(2, 16, 15, orc.KIND_SWARM, 5)
    assert len(ul.agent_pairs(15)) == 105 and ul.agent_pairs(12)[64:] == [(9, 11), (10, 11)]


def test_case_list_covers_every_instantiation():
    for c in ul.FORWARD:
        assert ul.lane_forward_eligible(c.nTh, c.m, c.d, c.spec_kind, c.n_agents), c.id
        assert c.r <= min(ul.MAX_RANK, c.d + 1), c.id
    for c in ul.ADJOINT:
        assert ul.lane_adjoint_eligible(c.nTh, c.m, c.d, c.spec_kind, c.n_agents) and c.mode == "train", c.id
    assert {c.shape for c in ul.FORWARD} == set(ul.INSTANTIATIONS)
    assert {c.shape for c in ul.ADJOINT} == set(ul.INSTANTIATIONS)
    for shape in ul.INSTANTIATIONS:
        fw = [c for c in ul.FORWARD if c.shape == shape]
        assert {c.n % 4 for c in fw if c.n < ul.BIG} >= {1, 2, 3}, shape
        assert any(c.n >= ul.BIG for c in fw), shape                     # grid > 1024 workgroups
        assert ul.big_case(shape).n > 4 * 1024
    # widths and inputs on both sides of every padding bound, SwarmTraj filling DP exactly
    assert {c.m for c in ul.FORWARD} >= {1, 7, 9, 16, 17, 31, 32}
    assert {c.d + 1 for c in ul.FORWARD if c.kind == "cross2d"} >= {3, 5, 7, 9, 15, 17, 25, 31}
    assert {c.d + 1 for c in ul.FORWARD if c.kind == "swarm"} >= {16, 31}
    assert {c.d + 1 for c in ul.ADJOINT} >= {3, 5, 7, 9, 15, 17, 25, 31}
    # rank: 1, the cap min(16, d + 1), something in between
    for cases in (ul.FORWARD, ul.ADJOINT):
        assert any(c.r == 1 for c in cases) and any(c.r == min(16, c.d + 1) and c.d + 1 >= 16 for c in cases)
        assert any(1 < c.r < min(16, c.d + 1) for c in cases)


def test_case_list_covers_steppers_spans_problems_and_modes():
    for cases in (ul.FORWARD, ul.ADJOINT):
        assert {(c.stepper, c.nt) for c in cases} >= {("rk4", 1), ("rk4", 7), ("rk1", 9)}
        assert {c.tspan for c in cases} >= {(0.0, 1.0), ul.T2}
        assert any(c.alph_Q == 0.0 and c.obstacle is not None for c in cases)
        assert any(c.alph_W == 0.0 and c.n_agents >= 2 for c in cases)
        assert any(c.n_agents >= 12 for c in cases)                       # pairs of the second 64-lane trip
    assert any(c.n_total not in (None, c.n) for c in ul.ADJOINT)
    assert {c.obstacle for c in ul.FORWARD} == {None, "softcorridor", "hardcorridor", "blocks"}
    assert {c.obstacle for c in ul.ADJOINT} == {None, "softcorridor", "hardcorridor"}
    # the W threshold: 2.0 r (eval), 2.2 r (train), 3.2 r (SwarmTraj train, N > 2)
    thr = {2.0 if c.mode == "eval" else (3.2 if c.kind == "swarm" and c.n_agents > 2 else 2.2) for c in ul.FORWARD if c.alph_W != 0}
    assert thr == {2.0, 2.2, 3.2}
    assert len({c.id for c in ul.FORWARD}) == len(ul.FORWARD) and len({c.id for c in ul.ADJOINT}) == len(ul.ADJOINT)


@pytest.mark.parametrize("case", ul.FORWARD + ul.ADJOINT, ids=lambda c: c.id)
def test_cases_exercise_their_physics(case):
    """Q / W nonzero where they are on (exactly zero where off), a second-trip pair inside the W threshold for N >= 12; the screened
    starts are the case's own (no state within a margin of a decision edge)"""
    D = ul.case_data(case)
    assert D["x"].shape == (case.n, case.d)
    assert ul.physics_gaps(case, D["r64"]) == []
    assert not bool(ul.near_edge(case, D["r64"]["stages"]).any())
    assert ul.failures(ul.compare_forward(D["r32"], D["r64"], D["r32"])) == {}


def _teeth(mutation, cases):
    """-> the cases on which the mutated fp64 oracle fails the comparator"""
    caught = []
    for c in cases:
        D = ul.case_data(c)
        bad = ul.oracle_forward(c, D["x"].double(), torch.float64, mutation)
        if ul.failures(ul.compare_forward(bad, D["r64"], D["r32"])):
            caught.append(c)
    return caught


def test_comparator_has_teeth():
    """four wrong restatements of the lane kernels' arithmetic, each caught on some case: A'A from r - 1 rows of A (a rank bound off by
    one), the last hidden unit dropped (a padding bound off by one: its row and column of K0 / b0 / K1 / w zeroed), time started at 0
    instead of t0, the train-mode W threshold in eval mode.  The first two are caught at both widths (MP = 16 and 32)."""
    for mutation in ("rank_minus_one", "last_hidden_dropped"):
        caught = _teeth(mutation, SMALL)
        assert {c.shape[0] for c in caught} == {16, 32}, (mutation, [c.id for c in caught])
    caught = _teeth("time_from_zero", [c for c in SMALL if c.tspan[0] != 0.0])
    assert caught, "time_from_zero"
    caught = _teeth("train_threshold_in_eval", [c for c in SMALL if c.mode == "eval" and c.alph_W != 0.0 and c.n_agents >= 2])
    assert caught, "train_threshold_in_eval"


def test_rollout_workspace_fits_every_rank():
    """Phi sizes its workspace with nocf_rollout_workspace_bytes, which knows (d, m, nTh) but not the rank of A: it must cover the image of
    A at the largest rank a plan accepts (r (d+1) floats, r <= 16) -- sized for r = 10, ranks 11 ... 16 were refused with NOCF_E_WORKSPACE"""
    from neuraloc_amd import _lib
    L = _lib.lib()
    for d, m in ((16, 16), (24, 16), (24, 17), (30, 32)):
        rup4 = lambda v: -(-v // 4) * 4                                                   # (the plan pads A's image to 4 floats)
        extra = 4 * (rup4(min(ul.MAX_RANK, d + 1) * (d + 1)) - rup4(10 * (d + 1)))
        assert L.nocf_rollout_workspace_bytes(d, m, 2, 1) >= L.nocf_workspace_bytes(d, m, 2) + extra, (d, m)
