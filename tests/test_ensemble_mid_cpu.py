"""Ensembles on the one-CU kernels (neuraloc_amd/ensemble.py with family="mid", trainOC.py --members_family mid) without a GPU: every refusal
-- each raised before the HIP library is reached and, in the driver, before anything is written --, the C prototypes, the eligibility mirror
and the case lists' coverage.  The default family keeps its messages."""
import os
import re

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, ensemble

import util_ensemble as ue
import util_ensemble_mid as uem
import util_mono as um

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = [na.ensemble_rollout, na.ensemble_ocflow_train]
TS, NT = [0.0, 1.0], 2


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to load or use the HIP library fails the test"""
    def reached(*a, **k):
        raise AssertionError("the HIP library was reached")
    monkeypatch.setattr(_lib, "lib", reached)
    monkeypatch.setattr(_lib, "lib_for", reached)


def _valid():
    case = uem.TRAIN[1]
    ens = na.PhiEnsemble.from_members(uem.member_nets(case, "cpu"), alph=uem.member_rows())
    return case, ens, uem.member_problem(case, 0, "cpu"), uem.starts(case)


def _cross(d):
    return na.Cross2D(torch.zeros(d), obstacle=None, alph_Q=1.0, alph_W=1.0, r=0.5)


@pytest.mark.parametrize("fn", FNS)
def test_mid_refusals_before_the_library(no_library, fn):
    case, ens, prob, x = _valid()
    kw = dict(family="mid")
    # CPU tensors, float64 anywhere, noMean, disturbances: as for the lane family
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(x, ens, prob, TS, NT, **kw)
    with pytest.raises(RuntimeError, match="single precision only"):
        fn(x.double(), ens, prob, TS, NT, **kw)
    e64 = na.PhiEnsemble.from_members(uem.member_nets(case, "cpu"), alph=uem.member_rows()).double()
    with pytest.raises(RuntimeError, match="single precision only"):
        fn(x, e64, prob, TS, NT, **kw)
    with pytest.raises(NotImplementedError, match="noMean"):
        fn(x, ens, prob, TS, NT, noMean=True, **kw)
    with pytest.raises(NotImplementedError, match="disturbed"):
        fn(x, ens, prob, TS, NT, W=torch.zeros(NT, x.shape[1], x.shape[2]), **kw)
    # outside the one-CU family: depth, width, input width, rank, agents -- the message names the limits
    for shape in (dict(nTh=3, m=64, d=4), dict(nTh=2, m=129, d=4), dict(nTh=2, m=64, d=32), dict(nTh=2, m=64, d=20, r=17)):
        big = na.PhiEnsemble(2, shape["nTh"], shape["m"], shape["d"], r=shape.get("r", 10))
        with pytest.raises(ValueError) as ex:
            fn(torch.zeros(2, 3, shape["d"]), big, _cross(shape["d"]), TS, NT, **kw)
        for limit in ("nTh = 2", "m <= 128", "d + 1 <= 32", "rank of A <= 16", "32 < m", "MONO_NAG"):
            assert limit in str(ex.value), (shape, limit)
    nine = _cross(14)
    nine.nAgents = 9                                            # d + 1 <= 16: MONO_NAG is 8
    with pytest.raises(ValueError, match="at most 8 agents"):
        fn(torch.zeros(2, 3, 14), na.PhiEnsemble(2, 2, 64, 14), nine, TS, NT, **kw)
    # shapes of x, nt, stepper
    with pytest.raises(ValueError, match="nex-by-d"):
        fn(torch.zeros(2, 5, case.base.d), ens, prob, TS, NT, **kw)
    with pytest.raises(ValueError, match="nt must be"):
        fn(x, ens, prob, TS, 0, **kw)
    with pytest.raises(ValueError, match="stepper"):
        fn(x, ens, prob, TS, NT, "rk2", **kw)


def test_mid_training_refusals_before_the_library(no_library):
    case, ens, prob, x = _valid()
    with pytest.raises(NotImplementedError, match="requires_grad"):
        na.ensemble_ocflow_train(x[0].clone().requires_grad_(), ens, prob, TS, NT, family="mid")
    # 32 < m for training: a quadcopter network of 32 units evaluates on the one-CU kernels but has no one-CU adjoint
    quad = na.Quadcopter(torch.zeros(12), obstacle=None, alph_Q=1.0, alph_W=1.0, r=0.5)
    small = na.PhiEnsemble(2, 2, 32, 12)
    with pytest.raises(ValueError, match="32 < m"):
        na.ensemble_ocflow_train(torch.zeros(2, 3, 12), small, quad, TS, NT, family="mid")
    with pytest.raises(RuntimeError, match="no CPU fallback"):                      # (evaluation: the shape passes, the CPU tensor does not)
        na.ensemble_rollout(torch.zeros(2, 3, 12), small, quad, TS, NT, family="mid")


@pytest.mark.parametrize("fn", FNS)
def test_an_unknown_family_is_a_value_error(no_library, fn):
    case, ens, prob, x = _valid()
    for family in ("duo", "", None, "MID"):
        with pytest.raises(ValueError, match="family must be"):
            fn(x, ens, prob, TS, NT, family=family)


@pytest.mark.parametrize("fn", FNS)
def test_the_default_family_keeps_its_messages(no_library, fn):
    """the calls of tests/test_ensemble_cpu.py, with and without family="lane": the lane family's refusals and texts"""
    for kw in ({}, dict(family="lane")):
        big = na.PhiEnsemble(2, 2, 33, 4)
        with pytest.raises(ValueError, match="m <= 32"):
            fn(torch.zeros(2, 3, 4), big, _cross(4), TS, NT, **kw)
        quad = na.Quadcopter(torch.zeros(12), obstacle=None, alph_Q=1.0, alph_W=1.0, r=0.5)
        with pytest.raises(ValueError, match="point-agent"):
            fn(torch.zeros(2, 3, 12), na.PhiEnsemble(2, 2, 9, 12), quad, TS, NT, **kw)
    sw = ue.FORWARD[1]
    e2 = na.PhiEnsemble.from_members(ue.member_nets(sw, "cpu"), alph=ue.member_rows())
    with pytest.raises(ValueError, match="Cross2D"):
        na.ensemble_ocflow_train(ue.starts(sw), e2, ue.member_problem(sw, 0, "cpu"), TS, NT)


def _driver():
    import importlib.util
    spec = importlib.util.spec_from_file_location("trainOC_under_test", os.path.join(REPO, "trainOC.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("extra, text", [
    (["--prec", "double"], "single precision"),
    (["--noise", "0.1"], "--noise"),
    (["--adv", "0.1"], "--adv"),
    (["--resume", "SOME.pth"], "--resume"),
    (["--m", "32"], "outside the one-CU kernels"),
    (["--m", "129"], "outside the one-CU kernels"),
    (["--nTh", "3"], "outside the one-CU kernels"),
    (["--data", "swarm50"], "outside the one-CU kernels"),
    (["--members", "0"], "must be >= 1"),
    (["--members", "NONE"], "must be >= 1"),
])
def test_driver_mid_refusals_write_nothing(no_library, tmp_path, monkeypatch, extra, text):
    drv = _driver()
    save = tmp_path / "out"
    argv = ["--members", "2", "--members_family", "mid", "--data", "singlequad", "--m", "64", "--niters", "1", "--save", str(save)]
    if extra[0] == "--members":
        argv = argv[2:]
        extra = [] if extra[1] == "NONE" else extra             # (--members_family mid without --members)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as ex:
        drv.main(argv + extra)
    assert text in str(ex.value)
    assert not save.exists()


def test_driver_mid_refuses_more_than_one_rank_and_lane_keeps_its_refusals(no_library, tmp_path, monkeypatch):
    drv = _driver()
    save = tmp_path / "out"
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as ex:
        drv.main(["--members", "2", "--members_family", "mid", "--data", "singlequad", "--m", "64", "--save", str(save)])
    assert "one rank" in str(ex.value)
    monkeypatch.delenv("WORLD_SIZE")
    for extra, text in ((["--m", "64"], "outside the small-network kernels"), (["--data", "singlequad"], "point-agent")):
        for fam in ([], ["--members_family", "lane"]):
            with pytest.raises(SystemExit) as ex:
                drv.main(["--members", "2", "--data", "softcorridor", "--niters", "1", "--save", str(save)] + extra + fam)
            assert text in str(ex.value)
    assert not save.exists()
    # ... and what family mid accepts passes the refusals (nothing runs: members_refusals only)
    for data, m in (("singlequad", 128), ("softcorridor", 64), ("swap12", 128)):
        args = drv.parse_args(["--members", "2", "--members_family", "mid", "--data", data, "--m", str(m)])
        assert len(drv.members_refusals(args, 1)) == 2


def test_prototypes_are_in_the_header():
    flat = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "nocf.h")).read())
    assert re.search(r"size_t nocf_mid_ensemble_workspace_bytes\(int32_t d, int32_t m, int32_t nTh, int32_t r, int32_t members\);", flat)
    want = {"nocf_rollout_mid_ensemble_f32": "float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull, "
                                             "void* workspace, size_t workspace_bytes, void* stream",
            "nocf_rollout_record_mid_ensemble_f32": "float* z_out, float* persample, float* cost_sums, float* s_all, float* act_rec, "
                                                    "int32_t* recorded, void* workspace, size_t workspace_bytes, void* stream",
            "nocf_rollout_bwd_mid_ensemble_f32": "const float* act_rec, float* gpart, int64_t gpart_rows, float* lam0, void* workspace, "
                                                 "size_t workspace_bytes, void* stream"}
    assert set(ensemble._MID) == set(want)
    for name, tail in want.items():
        mt = re.search(r"int " + name + r"\(([^;]*)\);", flat)
        assert mt, name
        args = mt.group(1)
        assert "int32_t members" in args and "const float* alph" in args and args.endswith(tail), name
        assert ("int64_t x_member_stride" in args) == (name != "nocf_rollout_bwd_mid_ensemble_f32")
        assert len(_lib.PROTOTYPES[name][1]) == len(args.split(",")), name          # the ctypes prototypes have the header's argument counts
    # the lane family's three entries are what they were
    assert set(ensemble._LANE) == {"nocf_rollout_ensemble_f32", "nocf_rollout_record_ensemble_f32", "nocf_rollout_bwd_small_ensemble_f32"}


def test_the_eligibility_mirror_agrees_with_the_one_cu_sweep():
    for c in um.FORWARD + um.ADJOINT:
        for train in (False, True):
            want = um.mono_adjoint_eligible(2, c.m, c.d, c.r, c.n_agents) if train else um.mono_plan_ok(2, c.m, c.d, c.r, c.n_agents)
            assert uem.mid_eligible(2, c.m, c.d, c.r, c.n_agents, train) == want, (c.id, train)
            assert ensemble._mid_eligible(2, c.m, c.d, c.r, c.n_agents, train) == want, (c.id, train)
    # ... and outside the lists: every bound from both sides
    for nTh, m, d, r, na_ in ((3, 64, 12, 10, 1), (2, 128, 12, 10, 1), (2, 129, 12, 10, 1), (2, 64, 31, 10, 1), (2, 64, 32, 10, 1),
                              (2, 64, 20, 16, 10), (2, 64, 20, 17, 10), (2, 64, 14, 10, 8), (2, 64, 14, 10, 9), (2, 64, 30, 10, 16),
                              (2, 64, 30, 10, 17), (2, 32, 12, 10, 1), (2, 33, 12, 10, 1)):
        for train in (False, True):
            want = um.mono_adjoint_eligible(nTh, m, d, r, na_) if train else um.mono_plan_ok(nTh, m, d, r, na_)
            assert uem.mid_eligible(nTh, m, d, r, na_, train) == ensemble._mid_eligible(nTh, m, d, r, na_, train) == want, (nTh, m, d, r, na_, train)


def test_cases_reach_every_instantiation():
    assert [c.base.shape for c in uem.FORWARD] == um.FORWARD_SHAPES
    assert [c.base.shape for c in uem.TRAIN] == um.ADJOINT_SHAPES and uem.CAPPED.base.shape in um.ADJOINT_SHAPES
    for c in uem.FORWARD + uem.TRAIN:
        b = c.base
        assert b.n == 17 and b.nt == 2 and um.mono_plan_ok(2, b.m, b.d, b.r, b.n_agents)
        # the single-network leg runs the one-CU kernel too (not the lane kernel)
        assert um.mono_forward_eligible(2, b.m, b.d, b.r, b.spec_kind, b.n_agents)
    assert all(um.mono_adjoint_eligible(2, c.base.m, c.base.d, c.base.r, c.base.n_agents) and c.own_x for c in uem.TRAIN + [uem.CAPPED][:0])
    assert um.mono_adjoint_eligible(2, uem.CAPPED.base.m, uem.CAPPED.base.d, uem.CAPPED.base.r, uem.CAPPED.base.n_agents)
    assert uem.CAPPED.base.n == um.BIG and uem.CAPPED.base.nt == 1 and uem.CAPPED.base.stepper == "rk1"
    assert {c.own_x for c in uem.FORWARD} == {True, False} and {c.base.mode for c in uem.FORWARD} == {"train", "eval"}
    assert [c.base.stepper for c in uem.FORWARD].count("rk1") == 1 and {c.base.kind for c in uem.FORWARD} == {"cross2d", "swarm", "quad"}
    f = uem.FORWARD
    assert (f[0].base.kind, f[0].base.d, f[0].base.m) == ("quad", 12, 128) and (f[4].base.kind, f[4].base.n_agents) == ("quad", 2)
    # record read and recompute, in training and in the recording forward
    for cases in (uem.FORWARD, uem.TRAIN):
        assert {um.mono_record_eligible(2, c.base.m, c.base.d, c.base.r, c.base.n_agents) for c in cases} == {True, False}
