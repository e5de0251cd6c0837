"""Ensembles (neuraloc_amd/ensemble.py, trainOC.py --members) without a GPU: the parameter container, the C prototypes, and every refusal --
each raised before the HIP library is reached and, in the driver, before anything is written."""
import os
import re

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, ensemble

import util_ensemble as ue
import util_lane as ul

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["A", "c.weight", "c.bias", "w.weight", "N.layers.0.weight", "N.layers.0.bias", "N.layers.1.weight", "N.layers.1.bias"]


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to load or use the HIP library fails the test"""
    def reached(*a, **k):
        raise AssertionError("the HIP library was reached")
    monkeypatch.setattr(_lib, "lib", reached)
    monkeypatch.setattr(_lib, "lib_for", reached)


def test_round_trip_names_and_shapes():
    case = ue.FORWARD[0]
    nets = ue.member_nets(case, "cpu")
    rows = ue.member_rows()
    ens = na.PhiEnsemble.from_members(nets, alph=rows)
    E, m, d, r = 3, case.base.m, case.base.d, case.base.r
    assert [k for k, _ in ens.named_parameters()] == NAMES == [k for k, _ in nets[0].named_parameters()]
    assert list(ens.state_dict().keys()) == NAMES
    shapes = {"A": (r, d + 1), "c.weight": (1, d + 1), "c.bias": (1,), "w.weight": (1, m), "N.layers.0.weight": (m, d + 1),
              "N.layers.0.bias": (m,), "N.layers.1.weight": (m, m), "N.layers.1.bias": (m,)}
    for name, p in ens.named_parameters():
        assert tuple(p.shape) == (E,) + shapes[name] and p.is_contiguous() and p.requires_grad
    assert ens.alph == rows and (ens.members, ens.nTh, ens.m, ens.d, ens.r) == (E, 2, m, d, r)
    for e in range(E):
        sd, want = ens.member_state_dict(e), nets[e].state_dict()
        assert list(sd.keys()) == list(want.keys())
        for k in want:
            assert sd[k].shape == want[k].shape and torch.equal(sd[k], want[k])
        q = ens.member(e)
        assert isinstance(q, na.Phi) and q.alph == rows[e]
        for k, v in q.state_dict().items():
            assert torch.equal(v, want[k])
        fresh = na.Phi(2, m, d, r=r)
        fresh.load_state_dict(sd)                          # (the reference's checkpoint layout: a member loads like any network)
    back = na.PhiEnsemble.from_members([ens.member(e) for e in range(E)])
    for (k, p), (_, q) in zip(ens.named_parameters(), back.named_parameters()):
        assert torch.equal(p, q)
    # copies in both directions: neither side aliases the other
    ens.A.data[0].zero_()
    assert not torch.equal(nets[0].A, ens.A[0]) and not torch.equal(back.A[0], ens.A[0])
    assert ens.alph_table().dtype == torch.float32 and ens.alph_table().tolist() == rows


def test_member_checkpoint_loads_like_any_network(tmp_path):
    from neuraloc_amd.checkpoint import load_file
    ens = na.PhiEnsemble(2, 2, 16, 4, alph=ue.member_rows(2), seeds=[3, 4])
    path = tmp_path / "m1_checkpt.pth"
    torch.save({"args": __import__("argparse").Namespace(data="softcorridor", m=16, nTh=2, alph=ens.alph[1]),
                "state_dict": ens.member_state_dict(1)}, path)
    ck = load_file(str(path))
    net = na.Phi(nTh=ck["args"].nTh, m=ck["args"].m, d=4, alph=ck["args"].alph)
    net.load_state_dict(ck["state_dict"])
    for k, v in net.state_dict().items():
        assert torch.equal(v, ens.member_state_dict(1)[k])


def test_seeded_construction_is_phi_under_that_seed():
    seeds = [11, 5, 11 + 2 ** 20]
    torch.manual_seed(99)
    before = torch.get_rng_state()
    ens = na.PhiEnsemble(3, 2, 9, 6, r=4, alph=[1.0] * 6, seeds=seeds)
    assert torch.equal(torch.get_rng_state(), before)          # the global generator is left as it was
    for e, s in enumerate(seeds):
        torch.manual_seed(s)
        want = na.Phi(2, 9, 6, r=4)
        got = ens.member_state_dict(e)
        for k, v in want.state_dict().items():
            assert torch.equal(got[k], v), (e, k)
    assert not torch.equal(ens.A[0], ens.A[1])
    with pytest.raises(ValueError):
        na.PhiEnsemble(2, 2, 9, 6, seeds=[1])
    with pytest.raises(ValueError):
        na.PhiEnsemble(2, 2, 9, 6, alph=[[1.0] * 6] * 3)
    with pytest.raises(ValueError):
        na.PhiEnsemble(0, 2, 9, 6)
    with pytest.raises(ValueError):
        na.PhiEnsemble.from_members([na.Phi(2, 9, 6), na.Phi(2, 8, 6)])


def test_prototypes_are_in_the_header():
    text = open(os.path.join(REPO, "include", "nocf.h")).read()
    flat = re.sub(r"\s+", " ", text)
    for name, extra in (("nocf_rollout_ensemble_f32", "float* cost_means, float* zFull, float* ctrlFull"),
                        ("nocf_rollout_record_ensemble_f32", "float* s_all"),
                        ("nocf_rollout_bwd_small_ensemble_f32", "float* gpart, float* lam0")):
        mt = re.search(r"int " + name + r"\(([^;]*)\);", flat)
        assert mt, name
        args = mt.group(1)
        assert "int32_t members" in args and "const float* alph" in args and extra in args, name
        assert ("int64_t x_member_stride" in args) == (name != "nocf_rollout_bwd_small_ensemble_f32")
    assert set(ensemble._LANE) == {"nocf_rollout_ensemble_f32", "nocf_rollout_record_ensemble_f32", "nocf_rollout_bwd_small_ensemble_f32"}
    # the ctypes prototypes have the header's argument counts
    for name, argtypes in ((name, _lib.PROTOTYPES[name][1]) for name in ensemble._LANE):
        args = re.search(r"int " + name + r"\(([^;]*)\);", flat).group(1)
        assert len(argtypes) == len(args.split(",")), name


def _valid():
    case = ue.TRAIN[0]
    ens = na.PhiEnsemble.from_members(ue.member_nets(case, "cpu"), alph=ue.member_rows())
    prob = ue.member_problem(case, 0, "cpu")
    x = ue.starts(case)
    return case, ens, prob, x


@pytest.mark.parametrize("fn", [na.ensemble_rollout, na.ensemble_ocflow_train])
def test_refusals_before_the_library(no_library, fn):
    case, ens, prob, x = _valid()
    ts, nt = [0.0, 1.0], 2
    # CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(x, ens, prob, ts, nt)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(x[0], ens, prob, ts, nt)
    # float64 anywhere
    with pytest.raises(RuntimeError, match="single precision only"):
        fn(x.double(), ens, prob, ts, nt)
    e64 = na.PhiEnsemble.from_members(ue.member_nets(case, "cpu"), alph=ue.member_rows()).double()
    with pytest.raises(RuntimeError, match="single precision only"):
        fn(x, e64, prob, ts, nt)
    p64 = ue.member_problem(case, 0, "cpu")
    p64.xtarget = p64.xtarget.double()
    with pytest.raises(RuntimeError, match="single precision only"):
        fn(x, ens, p64, ts, nt)
    # noMean, disturbances
    with pytest.raises(NotImplementedError, match="noMean"):
        fn(x, ens, prob, ts, nt, noMean=True)
    with pytest.raises(NotImplementedError, match="disturbed"):
        fn(x, ens, prob, ts, nt, W=torch.zeros(nt, x.shape[1], x.shape[2]))
    # outside the lane family: depth, width, input width, a quadcopter, too many agents -- the message names the limits
    for kw in (dict(nTh=3, m=9, d=4), dict(nTh=2, m=33, d=4), dict(nTh=2, m=9, d=32)):
        big = na.PhiEnsemble(2, kw["nTh"], kw["m"], kw["d"])
        pb = na.Cross2D(torch.zeros(kw["d"]), obstacle=None, alph_Q=1.0, alph_W=1.0, r=0.5)
        with pytest.raises(ValueError, match="m <= 32"):
            fn(torch.zeros(2, 3, kw["d"]), big, pb, ts, nt)
    quad = na.Quadcopter(torch.zeros(12), obstacle=None, alph_Q=1.0, alph_W=1.0, r=0.5)
    with pytest.raises(ValueError, match="point-agent"):
        fn(torch.zeros(2, 3, 12), na.PhiEnsemble(2, 2, 9, 12), quad, ts, nt)
    many = na.PhiEnsemble(2, 2, 9, 30)
    swarm17 = na.Cross2D(torch.zeros(30), obstacle=None, alph_Q=1.0, alph_W=1.0, r=0.5)
    swarm17.nAgents = 17
    with pytest.raises(ValueError, match="at most 16 agents"):
        fn(torch.zeros(2, 3, 30), many, swarm17, ts, nt)
    # shapes
    with pytest.raises(ValueError, match="nex-by-d"):
        fn(torch.zeros(2, 5, case.base.d), ens, prob, ts, nt)          # a leading axis that is not the member axis
    with pytest.raises(ValueError):
        fn(x[..., :-1], ens, prob, ts, nt)
    with pytest.raises(ValueError, match="nt must be"):
        fn(x, ens, prob, ts, 0)
    with pytest.raises(ValueError, match="stepper"):
        fn(x, ens, prob, ts, nt, "rk2")


def test_training_refusals_before_the_library(no_library):
    case, ens, prob, x = _valid()
    # a shared x that requires a gradient
    with pytest.raises(NotImplementedError, match="requires_grad"):
        na.ensemble_ocflow_train(x[0].clone().requires_grad_(), ens, prob, [0.0, 1.0], 2)
    # the lane adjoint takes Cross2D agents: a SwarmTraj ensemble evaluates but does not train
    sw = ue.FORWARD[1]
    e2 = na.PhiEnsemble.from_members(ue.member_nets(sw, "cpu"), alph=ue.member_rows())
    with pytest.raises(ValueError, match="Cross2D"):
        na.ensemble_ocflow_train(ue.starts(sw), e2, ue.member_problem(sw, 0, "cpu"), [0.0, 1.0], 2)


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
    (["--m", "64"], "outside the small-network kernels"),
    (["--nTh", "3"], "outside the small-network kernels"),
    (["--data", "swarm50"], "outside the small-network kernels"),
    (["--data", "singlequad"], "point-agent"),
    (["--members", "0"], "must be >= 1"),
    (["--members_alph", "MISSING_ROWS"], "lines of six"),
])
def test_driver_refusals_write_nothing(no_library, tmp_path, monkeypatch, extra, text):
    drv = _driver()
    save = tmp_path / "out"
    argv = ["--members", "2", "--data", "softcorridor", "--niters", "1", "--save", str(save)]
    if extra[0] == "--members":
        argv = argv[2:]
    if extra[0] == "--members_alph":
        f = tmp_path / "alph.txt"
        f.write_text("1,1,1,1,1,1\n")                      # one line for two members
        extra = ["--members_alph", str(f)]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as ex:
        drv.main(argv + extra)
    assert text in str(ex.value)
    assert not save.exists()


def test_driver_refuses_more_than_one_rank(no_library, tmp_path, monkeypatch):
    drv = _driver()
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit) as ex:
        drv.main(["--members", "2", "--save", str(tmp_path / "out")])
    assert "one rank" in str(ex.value) and not (tmp_path / "out").exists()


def test_cases_reach_every_instantiation():
    for cases in (ue.FORWARD, ue.TRAIN):
        assert [c.base.shape for c in cases] == ul.INSTANTIATIONS
        assert all(c.base.n == 5 and c.base.nt == 2 for c in cases)
    assert {c.own_x for c in ue.FORWARD} == {True, False}
    assert {c.base.mode for c in ue.FORWARD} == {"train", "eval"}
    assert [c.base.stepper for c in ue.FORWARD].count("rk1") == 1
    assert all(ul.lane_adjoint_eligible(2, c.base.m, c.base.d, c.base.spec_kind, c.base.n_agents) for c in ue.TRAIN)
    rows = ue.ALPH_ROWS
    assert rows[1][2] == 0.0 and rows[0][2] > 0.0 and len({tuple(r_) for r_ in rows}) == 3
    assert all(float(torch.tensor(v, dtype=torch.float32)) == v for r_ in rows for v in r_)
