"""CPU: the direct-transcription baseline's fixture, argument validation, C-ABI error codes and the driver's flags (no GPU needed)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib
from oracle import ocflow_oracle as orc
import util_oracle as uo
from util_oracle import oracle_objective

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(REPO, "tests", "golden", "baseline.npz"))
META = json.loads(str(FIX["meta"]))
CASES = [(name, nt, mode) for name, info in META["problems"].items() for nt in info["nts"] for mode in ("train", "eval")]


def make_prob(name, alph, device="cpu"):
    prob, _, _, xInit = na.initProb(name, 10, 10, var0=1.0, cvt=lambda t: t.float().to(device),
                                    alph=[alph[0], alph[1], alph[2], 0.0, 0.0, 0.0])
    return prob, xInit.reshape(-1)


@pytest.mark.parametrize("name,nt,mode", CASES)
def test_fixture_reproduced_by_oracle_restatement(name, nt, mode):
    info = META["problems"][name]
    prob, _ = make_prob(name, info["alph"])
    prob.train() if mode == "train" else prob.eval()
    S = orc.ProbSpec.from_object(prob)
    pre = f"{name}/nt{nt}"
    z0s, Us = torch.from_numpy(FIX[f"{pre}/z0"]), torch.from_numpy(FIX[f"{pre}/U"])
    for k in range(z0s.shape[0]):
        u = Us[k].clone().requires_grad_(True)
        J = oracle_objective(S, u, z0s[k], nt, info["alph"][0])
        J.backward()
        want = float(FIX[f"{pre}/{mode}/loss"][k])
        assert abs(J.item() - want) <= 1e-5 * abs(want), (k, J.item(), want)
        gw = torch.from_numpy(FIX[f"{pre}/{mode}/grad"][k])
        assert float((u.grad - gw).abs().max()) <= 1e-5 * float(gw.abs().max()) + 1e-7, k


def test_fixture_is_small_and_complete():
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "baseline.npz")) < 2 * 1024 * 1024
    assert set(META["problems"]) == {"softcorridor", "swap2", "swap12", "swap12_3pair", "midcross4", "midcross20", "swarm", "swarm50"}
    assert FIX["solve600/ubest"].shape == (50, 4) and FIX["checkpt/U"].shape == (50, 4)


def test_quadcopter_is_refused():
    prob, _, _, xInit = na.initProb("singlequad", 2, 2, var0=1.0, cvt=lambda t: t.float(), alph=[1.0] * 6)
    U = torch.zeros(20, 12)
    with pytest.raises(ValueError, match="quadcopter"):
        na.baseline_loss(xInit.reshape(-1), U, prob, 100.0)
    with pytest.raises(ValueError, match="quadcopter"):
        na.solve_baseline(xInit.reshape(-1), prob, 20, niters=5, U0=U)


def test_wrong_shapes_raise():
    prob, xInit = make_prob("softcorridor", [100.0, 1e4, 300.0])
    with pytest.raises(ValueError):
        na.baseline_loss(torch.zeros(3), torch.zeros(20, 4), prob, 100.0)           # z0 of the wrong d
    with pytest.raises(ValueError):
        na.baseline_loss(xInit, torch.zeros(20, 5), prob, 100.0)                    # controls of the wrong d
    with pytest.raises(ValueError):
        na.baseline_loss(torch.zeros(3, 4), torch.zeros(2, 20, 4), prob, 100.0)      # batch sizes disagree
    with pytest.raises(ValueError):
        na.baseline_report(xInit, torch.zeros(4), prob, 100.0)
    with pytest.raises(ValueError):
        na.solve_baseline(xInit, prob, 0, niters=5)


def test_cpu_tensors_raise():
    prob, xInit = make_prob("softcorridor", [100.0, 1e4, 300.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.baseline_loss(xInit, torch.zeros(20, 4), prob, 100.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.solve_baseline(xInit, prob, 20, niters=5)


def _struct(kind, obstacle, n_agents, training=1):
    st = _lib.NocfProb()
    st.kind, st.obstacle, st.n_agents, st.training = kind, obstacle, n_agents, training
    st.r, st.alph_Q, st.alph_W, st.mass, st.grav = 0.5, 1.0, 1.0, 1.0, 9.81
    st.xtarget = 16                                    # never dereferenced: every call below returns before a launch
    return st


def test_abi_argument_errors():
    import __graft_entry__ as entry
    entry.build()
    L = _lib.lib()
    fake = C.c_void_p(16)
    ev = L.nocf_baseline_eval_f32
    ad = L.nocf_baseline_adam_f32
    quad = _struct(_lib.PROB_QUADCOPTER, 0, 1)
    cross = _struct(_lib.PROB_CROSS2D, 1, 2)
    swarm50 = _struct(_lib.PROB_SWARMTRAJ, 3, 50)
    assert ev(C.byref(quad), 12, 1, 20, 100.0, fake, fake, fake, None, None, None, None) == -3          # NOCF_E_PROB
    assert ev(C.byref(cross), 4, 1, 20, 100.0, None, fake, fake, None, None, None, None) == -1          # NOCF_E_NULL
    assert ev(C.byref(cross), 4, 1, 0, 100.0, fake, fake, fake, None, None, None, None) == -2           # NOCF_E_SHAPE: nt
    assert ev(C.byref(cross), 4, 0, 20, 100.0, fake, fake, fake, None, None, None, None) == -2          # B
    assert ev(C.byref(cross), 6, 1, 20, 100.0, fake, fake, fake, None, None, None, None) == -3          # d != 2 n_agents
    args = (0.1, 0.9, 0.999, 1e-8, 0, 10, fake, fake, fake, fake, fake, fake, None, None)
    assert ad(C.byref(quad), 12, 1, 20, 100.0, *args) == -3
    # the LDS limit: swarm50 fits up to nt = 50 (U, m, v, z, dJ/dU of one point in 160 KiB), not beyond
    assert ad(C.byref(swarm50), 150, 1, 51, 100.0, *args) == -2
    assert ad(C.byref(swarm50), 150, 1, 50, 100.0, *(args[:5] + (0,) + args[6:])) == 0    # niters = 0: nothing to launch


def test_driver_flags_parse():
    import baseline2D
    a = baseline2D.parse_args([])
    assert (a.data, a.nt, a.alph, a.niters, a.prec, a.save, a.resume) == \
        ("softcorridor", 50, [100.0, 10000.0, 300.0], 600, "single", "experiments/oc/baseline", None)
    a = baseline2D.parse_args(["--data", "swarm", "--nt", "20", "--alph", "900,1e7,25000", "--niters", "301", "--nx", "64",
                               "--seed", "3", "--gpu", "0", "--resume", "u.pth", "--save", "out"])
    assert (a.data, a.nt, a.alph, a.niters, a.nx, a.seed, a.resume, a.save) == \
        ("swarm", 20, [900.0, 1e7, 25000.0], 301, 64, 3, "u.pth", "out")
    with pytest.raises(SystemExit):
        baseline2D.parse_args(["--data", "singlequad"])
    with pytest.raises(SystemExit, match="double"):
        baseline2D.main(["--prec", "double"])


@pytest.mark.parametrize("name", sorted(uo.BASE_ALPH))
def test_abi_nt_limits(name):
    """the largest nt each entry point accepts (bl_layout in 160 KiB of LDS, NOCF_BL_MAX_NT), refused one past it on the host before
    any launch; the GPU sweep launches at these limits"""
    import __graft_entry__ as entry
    entry.build()
    L = _lib.lib()
    fake = C.c_void_p(16)
    N = uo.N_AGENTS[name]
    swarm = name.startswith("swarm")
    st = _struct(_lib.PROB_SWARMTRAJ if swarm else _lib.PROB_CROSS2D, 0, N)
    d = (3 if swarm else 2) * N
    ev, ad = uo.nt_limits(name)
    assert L.nocf_baseline_eval_f32(C.byref(st), d, 1, ev + 1, 100.0, fake, fake, fake, None, None, None, None) == -2
    args = (0.1, 0.9, 0.999, 1e-8, 0, 0, fake, fake, fake, fake, fake, fake, None, None)     # niters = 0: nothing to launch
    assert L.nocf_baseline_adam_f32(C.byref(st), d, 1, ad, 100.0, *args) == 0
    assert L.nocf_baseline_adam_f32(C.byref(st), d, 1, ad + 1, 100.0, *args) == -2
    if ad < ev:                                         # the eval layout has room for more
        assert L.nocf_baseline_adam_f32(C.byref(st), d, 1, ev, 100.0, *args) == -2


def test_sweep_cases_cover_every_launch_shape():
    """the shared case list: every point-agent problem, both modes, every (threads, lanes) pair of baseline_setup in both modes"""
    names = {c.name for c in uo.SWEEP}
    assert names == set(na.initProb.__globals__["PROBLEM_NAMES"]) - {"singlequad"}
    for name in names:
        assert {c.mode for c in uo.SWEEP if c.name == name} == {"train", "eval"}
        assert {c.nt for c in uo.SWEEP if c.name == name} >= {1, 7, 9, *uo.nt_limits(name)}
    seen = {}
    for c in uo.SWEEP:
        seen.setdefault(uo.launch_shape(uo.N_AGENTS[c.name], c.nt), set()).add(c.mode)
    assert set(seen) == {(256, g) for g in (1, 2, 4, 8, 16, 32, 64)} | {(1024, g) for g in (4, 8, 16, 32, 64)}
    assert all(m == {"train", "eval"} for m in seen.values()), seen
    assert len({c.id for c in uo.SWEEP}) == len(uo.SWEEP)


def test_comparator_has_teeth():
    """the comparator of the GPU sweep rejects each deliberately wrong fp32 restatement on at least one case: L at the state before the
    step, h = 1/(nt+1), the train threshold in eval mode, the last step's state detached.  (That it accepts the right fp32 restatement
    holds by construction, its error being what calibrates the tolerance; what the loop checks besides is that every case passes the
    physics guard.)"""
    caught = {m: [] for m in uo.MUTATIONS}
    for case in uo.SWEEP:
        S, z0, U, traj = uo.case_data(case)
        aG = case.alph[0]
        r64 = uo.restate(S, z0, U, aG, torch.float64, traj)
        r32 = uo.restate(S, z0, U, aG, torch.float32, traj)
        res = uo.compare_all(r32, r64, r32)
        assert all(v[0] for v in res.values()), (case.id, res)
        assert not uo.physics_gaps(case, S, r64), case.id
        for m in uo.MUTATIONS:
            if m == "train_threshold_in_eval" and S.training:
                continue
            bad = uo.restate(S, z0, U, aG, torch.float32, traj, mutation=m)
            if not all(v[0] for v in uo.compare_all(bad, r64, r32).values()):
                caught[m].append(case.id)
    print("[teeth] " + ", ".join(f"{m}: {len(ids)} of {len(uo.SWEEP)} cases" for m, ids in caught.items()))
    missed = [m for m, ids in caught.items() if not ids]
    assert not missed, f"mutations no sweep case rejects: {missed}"
