"""The small-network lane kernels (csrc/nocf_lane.inc, csrc/nocf_lane_bwd.inc) at every instantiation against the oracle in fp64.

Each case of tests/util_lane.py runs on the MI355X and is compared with fp64 under util_oracle's rule (4x the fp32 restatement's own error,
with a floor): forward Jc, the means, the per-sample table, the final state and the intermediates; the recording forward and the adjoint
against fp64 autograd; the three shipped lane configurations at a training-size ragged batch; the eligibility boundaries by kernel name;
the one-launch variant bitwise against the two-launch path, also as a process's very first call on a side stream."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import neuraloc_amd as na
import util_lane as ul
import util_oracle as uo
from conftest import load_golden
from neuraloc_amd import _lib
from neuraloc_amd.train import ocflow_train
from oracle import ocflow_oracle as orc
from util_hip import closed_form_normal, make_net as golden_net, make_prob as golden_prob

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STEPPERS = {"rk4": _lib.NOCF_RK4, "rk1": _lib.NOCF_RK1}

# every instantiation is reached, forward and adjoint (the mirror of the dispatcher says which one a case takes)
assert {c.shape for c in ul.FORWARD} == set(ul.INSTANTIATIONS) and {c.shape for c in ul.ADJOINT} == set(ul.INSTANTIATIONS)


def kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def _setup(case, train=False):
    D = ul.case_data(case)
    net = ul.make_net(case, DEV)
    net.train() if train else net.eval()
    return D, net, ul.make_problem(case, DEV), D["x"].to(DEV)


def _raw(case, x, net, prob):
    """nocf_rollout_f32 with the final state: -> (persample [n, 7], z [n, d+4])"""
    n = x.shape[0]
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(DEV)
    tab = torch.full((n, 7), float("nan"), device=DEV)
    z = torch.full((n, case.d + 4), float("nan"), device=DEV)
    sums = torch.empty(8, device=DEV)
    alph_c = (C.c_float * 6)(*[float(a) for a in case.alph])
    rc = _lib.lib().nocf_rollout_f32(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), n, float(case.tspan[0]), float(case.tspan[1]),
                                     case.nt, STEPPERS[case.stepper], alph_c, _lib.ptr(z), _lib.ptr(tab), _lib.ptr(sums), None, None,
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    _lib.check(rc, "nocf_rollout_f32")
    torch.cuda.synchronize()
    return tab, z


def _forward(case, x, net, prob):
    """every forward output of the case -> (dict for ul.compare_forward, kernel name of each call)"""
    ts = list(case.tspan)
    with torch.no_grad():
        Jc, cs = na.OCflow(x, net, prob, ts, case.nt, case.stepper, case.alph)
        k = [kernel()]
        _, csn = na.OCflow(x, net, prob, ts, case.nt, case.stepper, case.alph, noMean=True)
        k.append(kernel())
        zF, cF = na.OCflow(x[:8], net, prob, ts, case.nt, case.stepper, case.alph, intermediates=True)
        k.append(kernel())
        tab, z = _raw(case, x, net, prob)
        k.append(kernel())
    got = dict(Jc=Jc.cpu(), cs=torch.stack([c.reshape(()) for c in cs]).cpu(), table=torch.cat(csn, 1).cpu(), z=z.cpu(),
               zFull=zF.cpu(), ctrlFull=cF.cpu())
    assert torch.equal(got["table"], tab.cpu())
    return got, k


def _check(res, what):
    bad = ul.failures(res)
    assert not bad, f"{what}: " + "; ".join(f"{k}: err {e:.3g} > tol {t:.3g} (fp32 oracle {e32:.3g})" for k, (_, e, t, e32) in bad.items())


@pytest.mark.parametrize("case", ul.FORWARD, ids=lambda c: c.id)
def test_forward_against_fp64(case):
    D, net, prob, x = _setup(case)
    got, kernels = _forward(case, x, net, prob)
    assert kernels == ["rollout_lane_kernel"] * 4, kernels
    _check(ul.compare_forward(got, D["r64"], D["r32"]), case.id)


def _grad_check(got, want64, ref32, what):
    res = {}
    for k in want64:
        w = want64[k] if want64[k] is not None else torch.zeros_like(got[k], dtype=torch.float64)
        r = ref32[k] if ref32[k] is not None else torch.zeros_like(got[k])
        res[k] = uo.compare(got[k], w, r)
    _check(res, what)


@pytest.mark.parametrize("case", ul.ADJOINT, ids=lambda c: c.id)
def test_adjoint_against_fp64_autograd(case):
    D, net, prob, x = _setup(case, train=True)
    xx = x.clone().requires_grad_(True)
    Jc, cs = ocflow_train(xx, net, prob, list(case.tspan), case.nt, case.stepper, case.alph, n_total=case.n_total)
    assert kernel() == "rollout_lane_kernel"
    Jc.backward()
    assert kernel() == "rollout_lane_bwd_kernel"
    _check(ul.compare_forward(dict(Jc=Jc.detach().cpu(), cs=torch.stack(cs).detach().cpu()), D["r64"], D["r32"]), case.id)
    J64, g64, x64 = ul.oracle_grads(case, D["x"], torch.float64)
    J32, g32, x32 = ul.oracle_grads(case, D["x"], torch.float32)
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    got["x"] = xx.grad.cpu()
    g64["x"], g32["x"] = x64, x32
    _grad_check(got, g64, g32, case.id)


@pytest.mark.parametrize("name", ["swap2", "softcorridor", "swap12"])
def test_training_size_adjoint_against_fp64_autograd(name):
    """the shipped lane configurations with their weights and nt, train mode, a ragged batch of 1027: the per-sample gradient rows of the
    lane adjoint summed by train._unpack_partials against fp64 autograd"""
    g = load_golden(name)
    m = g.meta
    n, nt, alph = 1027, m["nt"], m["alph"]
    sd = g.state_dict()
    S = orc.ProbSpec(kind=orc.KIND_CROSS2D, xtarget=g.t("xtarget"), obstacle=m["obstacle"], alph_Q=m["alph_Q"], alph_W=m["alph_W"],
                     r=m["r"], training=True)
    cand = (g.t("xInit").reshape(1, -1) + m["var0"] * closed_form_normal(n + 512, m["d"], 5)).contiguous()
    x = ul.screen_starts(sd, S, cand, (0.0, 1.0), nt, "rk4", alph, n)
    net = golden_net(g, DEV).train()
    prob = golden_prob(g, DEV, training=True)
    Jc, _ = na.OCflow(x.to(DEV), net, prob, [0.0, 1.0], nt, "rk4", alph)
    assert kernel() == "rollout_lane_kernel"
    Jc.backward()
    assert kernel() == "rollout_lane_bwd_kernel"
    J64, g64, _ = ul.autograd_grads(sd, S, x, (0.0, 1.0), nt, "rk4", alph, torch.float64)
    J32, g32, _ = ul.autograd_grads(sd, S, x, (0.0, 1.0), nt, "rk4", alph, torch.float32)
    ok, err, tol, _ = uo.compare(Jc.detach().cpu().reshape(1), torch.tensor([J64]), torch.tensor([J32]))
    assert ok, (float(Jc), J64, J32)
    _grad_check({k: p.grad.detach().cpu() for k, p in net.named_parameters()}, g64, g32, name)


# ---- eligibility boundaries: the kernel that runs, and the result against fp64
def _boundary(case):
    D, net, prob, x = _setup(case)
    got, kernels = _forward(case, x, net, prob)
    _check(ul.compare_forward(got, D["r64"], D["r32"]), case.id)
    return kernels


def test_swarm_training_runs_the_lane_forward_and_the_tile_adjoint():
    case = next(c for c in ul.FORWARD if c.kind == "swarm" and c.mode == "train" and c.n < ul.BIG)
    D, net, prob, x = _setup(case, train=True)
    Jc, cs = na.OCflow(x, net, prob, list(case.tspan), case.nt, case.stepper, case.alph)
    assert kernel() == "rollout_lane_kernel"
    Jc.backward()
    assert kernel() == "rollout_bwd_kernel"                      # the lane adjoint is Cross2D-only
    _check(ul.compare_forward(dict(Jc=Jc.detach().cpu(), cs=torch.stack(cs).detach().cpu()), D["r64"], D["r32"]), case.id)
    J64, g64, _ = ul.oracle_grads(case, D["x"], torch.float64)
    J32, g32, _ = ul.oracle_grads(case, D["x"], torch.float32)
    _grad_check({k: p.grad.detach().cpu() for k, p in net.named_parameters()}, g64, g32, case.id)


@pytest.mark.parametrize("case,expect", [
    (ul.LaneCase("cross2d", 8, 33, 4, "softcorridor", "eval", 5, "rk4", 7, seed=3), "rollout_mono_kernel"),        # m = 33
    (ul.LaneCase("cross2d", 32, 16, 8, None, "train", 6, "rk4", 7, seed=4), "rollout_kernel<"),                    # d + 1 = 33
    (ul.LaneCase("cross2d", 8, 16, 4, "hardcorridor", "train", 7, "rk1", 9, seed=5, nTh=3), "rollout_kernel<"),    # nTh = 3
], ids=["m33", "d32", "nTh3"])
def test_eligibility_boundaries(case, expect):
    kernels = _boundary(case)
    assert all(k.startswith(expect) for k in kernels), kernels


def test_lane_switched_off():
    case = ul.FORWARD[2]
    os.environ["NOCF_LANE"] = "0"
    try:
        kernels = _boundary(case)
    finally:
        os.environ.pop("NOCF_LANE", None)
    assert "rollout_lane_kernel" not in kernels, kernels


def test_rank_above_16_is_refused_before_any_launch():
    d, m = 16, 16
    net = na.Phi(nTh=2, m=m, d=d, r=17).to(DEV)
    assert net.A.shape == (17, 17)
    prob = na.Cross2D(torch.zeros(d, device=DEV), obstacle=None, alph_Q=1.0, alph_W=1.0, r=0.5)
    case = ul.LaneCase("cross2d", d, m, 17, None, "eval", 5, "rk4", 3)
    x = torch.zeros(5, d, device=DEV)
    with pytest.raises(RuntimeError, match="nocf_rollout_f32"):
        _raw(case, x, net, prob)
    phi_st, keep1, ws = net._c_struct(5)
    prob_st, keep2 = prob._c_struct(DEV)
    P = int(_lib.lib().nocf_small_grad_floats(d, m))
    gpart = torch.full((5, P), float("nan"), device=DEV)
    z = torch.zeros(5, d + 4, device=DEV)
    s_all = torch.zeros(12, 5, d + 1, device=DEV)
    hs = torch.full((3,), 1.0 / 3, device=DEV)
    alph_c = (C.c_float * 6)(*[1.0] * 6)
    rc = _lib.lib().nocf_rollout_bwd_small_f32(C.byref(phi_st), C.byref(prob_st), 5, 3, _lib.NOCF_RK4, 1.0, alph_c, 0.2,
                                                _lib.ptr(s_all), _lib.ptr(z), _lib.ptr(hs), _lib.ptr(gpart), None, _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == -2                                              # NOCF_E_SHAPE
    assert bool(gpart.isnan().all())


# ---- the one-launch variant (NOCF_LANE_ONE=1) on the >= 4097-row case of every instantiation
@pytest.mark.parametrize("shape", ul.INSTANTIATIONS, ids=lambda s: f"MP{s[0]}-DP{s[1]}")
def test_one_launch_against_fp64_and_two_launches(shape):
    case = ul.big_case(shape)
    D, net, prob, x = _setup(case)
    out = {}
    for one in ("1", "0"):
        os.environ["NOCF_LANE_ONE"] = one
        try:
            with torch.no_grad():
                Jc, cs = na.OCflow(x, net, prob, list(case.tspan), case.nt, case.stepper, case.alph)
            torch.cuda.synchronize()
        finally:
            os.environ.pop("NOCF_LANE_ONE", None)
        assert kernel() == "rollout_lane_kernel"
        out[one] = (Jc.cpu(), torch.stack([c.reshape(()) for c in cs]).cpu())
    assert torch.equal(out["1"][0], out["0"][0]) and torch.equal(out["1"][1], out["0"][1])
    _check(ul.compare_forward(dict(Jc=out["1"][0], cs=out["1"][1]), D["r64"], D["r32"]), case.id)


CHILD = r"""
import os, sys
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import torch
import neuraloc_amd as na
from neuraloc_amd import _lib
from conftest import load_golden
from util_hip import closed_form_normal, make_net, make_prob
dev = torch.device("cuda:0")
g = load_golden("swap12")
m = g.meta
net, prob = make_net(g, dev), make_prob(g, dev, False)
x = (g.t("xInit") + m["var0"] * closed_form_normal(3001, m["d"], 9)).contiguous().to(dev)
st = torch.cuda.Stream(dev)
os.environ["NOCF_LANE_ONE"] = "1"
with torch.no_grad(), torch.cuda.stream(st):
    J1, c1 = na.OCflow(x, net, prob, [0.0, 1.0], m["nt"], "rk4", m["alph"])      # the process's first lane call: on a side stream
assert _lib.lib().nocf_last_rollout_kernel().decode() == "rollout_lane_kernel"
torch.cuda.synchronize()
os.environ["NOCF_LANE_ONE"] = "0"
with torch.no_grad():
    J2, c2 = na.OCflow(x, net, prob, [0.0, 1.0], m["nt"], "rk4", m["alph"])
torch.cuda.synchronize()
print("EQUAL", int(torch.equal(J1, J2) and all(torch.equal(a, b) for a, b in zip(c1, c2))), float(J1), float(J2))
"""


def test_first_one_launch_call_on_a_side_stream():
    """a fresh process whose very first one-launch call runs on a non-default stream (the ticket words are zeroed on that stream)"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("NOCF_LANE_ONE", None)
    r = subprocess.run([sys.executable, "-c", CHILD, repo], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("EQUAL")][-1]
    assert line.split()[1] == "1", line
