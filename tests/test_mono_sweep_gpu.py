"""The one-CU weight-stationary kernels (csrc/nocf_mono.inc, csrc/nocf_mono_bwd.inc) at every instantiation against the oracle in fp64.

Each case of tests/util_mono.py runs on the MI355X and is compared with fp64 under util_oracle's rule (4x the fp32 restatement's own error,
with a floor): forward Jc, the means, the per-sample table, the final state and the intermediates, with the kernel named by
nocf_last_rollout_kernel and its (KBM, KBD) by the NOCF_DEBUG line; the recording forward's stage inputs and the five sections of its
activation record; the adjoint against fp64 autograd, a batch of more than 1024 tiles included; nocf_rollout_segments_f32 bitwise against
per-segment calls; the eligibility boundaries by kernel name."""
import ctypes as C
import dataclasses
import os
import re

import pytest
import torch

import neuraloc_amd as na
import util_mono as um
import util_oracle as uo
from neuraloc_amd import _lib
from neuraloc_amd.train import ocflow_train
from oracle import ocflow_oracle as orc
from util_hip import poison_allocator

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STEPPERS = {"rk4": _lib.NOCF_RK4, "rk1": _lib.NOCF_RK1}
KINDS = {"cross2d": orc.KIND_CROSS2D, "swarm": orc.KIND_SWARM, "quad": orc.KIND_QUAD}
E_SHAPE = -2
SMALL = [c for c in um.FORWARD if c.n < um.BIG]
RECORD = [c for c in SMALL if c.mode == "train"]

# every instantiation is reached by construction: 7 shapes x (evaluation, recording) forward, 6 adjoint shapes
assert {c.shape for c in um.FORWARD} == set(um.FORWARD_SHAPES) == {c.shape for c in RECORD}
assert {c.shape for c in um.ADJOINT} == set(um.ADJOINT_SHAPES)
assert {(c.shape, um.mono_record_eligible(2, c.m, c.d, c.r, c.n_agents)) for c in RECORD} >= {(s, True) for s in um.ADJOINT_SHAPES}


def kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


@pytest.fixture
def knobs():
    """set NOCF_* knobs for one test: knobs(NOCF_MONO="0"); restored afterwards"""
    saved = {}

    def put(**kw):
        for k, v in kw.items():
            saved.setdefault(k, os.environ.get(k))
            os.environ[k] = v
    yield put
    for k, v in saved.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _debug_shapes(err):
    return [(int(a), int(b)) for a, b in re.findall(r"mono kernel: (\d+) hidden / (\d+) input k-blocks", err)]


def _setup(case, train=False):
    D = um.case_data(case)
    net = um.make_net(case, DEV)
    net.train() if train else net.eval()
    return D, net, um.make_problem(case, DEV), D["x"].to(DEV)


def _alph(case):
    return (C.c_float * 6)(*[float(a) for a in case.alph])


def _raw(case, x, net, prob, tspan=None, nt=None, full=False):
    """nocf_rollout_f32 -> (persample [n, 7], z [n, d+4], sums [8], zFull, ctrlFull (time-major, with full=True))"""
    n = x.shape[0]
    t0, t1 = tspan or case.tspan
    nt = nt or case.nt
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(DEV)
    tab = torch.full((n, 7), float("nan"), device=DEV)
    z = torch.full((n, case.d + 4), float("nan"), device=DEV)
    sums = torch.full((8,), float("nan"), device=DEV)
    zF = cF = None
    if full:
        cdim = _lib.lib().nocf_ctrl_dim(C.byref(prob_st), case.d)
        zF = torch.full((nt + 1, n, case.d + 4), float("nan"), device=DEV)
        cF = torch.full((nt + 1, n, cdim), float("nan"), device=DEV)
    rc = _lib.lib().nocf_rollout_f32(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), n, float(t0), float(t1), nt, STEPPERS[case.stepper],
                                     _alph(case), _lib.ptr(z), _lib.ptr(tab), _lib.ptr(sums), _lib.ptr(zF), _lib.ptr(cF),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    _lib.check(rc, "nocf_rollout_f32")
    torch.cuda.synchronize()
    return tab, z, sums, zF, cF


def _forward(case, x, net, prob):
    """every forward output of the case -> (dict for um.compare_forward, kernel name of each call)"""
    ts = list(case.tspan)
    with torch.no_grad():
        Jc, cs = na.OCflow(x, net, prob, ts, case.nt, case.stepper, case.alph)
        k = [kernel()]
        _, csn = na.OCflow(x, net, prob, ts, case.nt, case.stepper, case.alph, noMean=True)
        k.append(kernel())
        zF, cF = na.OCflow(x[:8], net, prob, ts, case.nt, case.stepper, case.alph, intermediates=True)
        k.append(kernel())
        tab, z, _, _, _ = _raw(case, x, net, prob)
        k.append(kernel())
        tab2, z2, _, _, _ = _raw(case, x, net, prob)
        k.append(kernel())
    got = dict(Jc=Jc.cpu(), cs=torch.stack([c.reshape(()) for c in cs]).cpu(), table=torch.cat(csn, 1).cpu(), z=z.cpu(),
               zFull=zF.cpu(), ctrlFull=cF.cpu())
    assert torch.equal(got["table"], tab.cpu()), "noMean's table differs from nocf_rollout_f32's"
    assert torch.equal(tab, tab2) and torch.equal(z, z2), "not run-to-run deterministic"
    assert float(cF[:, :, 0].abs().max()) == 0.0                      # slot 0 of the controls is exactly zero
    return got, k


def _check(res, what):
    bad = um.failures(res)
    assert not bad, f"{what}: " + "; ".join(f"{k}: err {e:.3g} > tol {t:.3g} (fp32 oracle {e32:.3g})" for k, (_, e, t, e32) in bad.items())


# ---- forward
@pytest.mark.parametrize("case", um.FORWARD, ids=lambda c: c.id)
def test_forward_against_fp64(case, knobs, capfd):
    D, net, prob, x = _setup(case)
    knobs(NOCF_DEBUG="1")
    capfd.readouterr()
    got, kernels = _forward(case, x, net, prob)
    shapes = _debug_shapes(capfd.readouterr().err)
    assert kernels == ["rollout_mono_kernel"] * 5, kernels
    assert shapes == [case.shape] * 5, (shapes, case.shape)
    _check(um.compare_forward(got, D["r64"], D["r32"]), case.id)


# ---- recording forward: the stage inputs and the activation record
def _record(case, x, net, prob, with_act=True):
    """nocf_rollout_record_act_f32 -> (s_all [E, n, d+1], act (NaN-filled before the call, sized for the record) or None, recorded, z)"""
    n, d, m = x.shape[0], case.d, case.m
    E = case.nt * (4 if case.stepper == "rk4" else 1)
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(DEV)
    tab = torch.empty(n, 7, device=DEV)
    z = torch.full((n, d + 4), float("nan"), device=DEV)
    sums = torch.empty(8, device=DEV)
    s_all = torch.full((E, n, d + 1), float("nan"), device=DEV)
    act = torch.full((E * n * (4 * m + d + 1),), float("nan"), device=DEV) if with_act else None
    recorded = C.c_int32(-1)
    rc = _lib.lib().nocf_rollout_record_act_f32(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), n, float(case.tspan[0]), float(case.tspan[1]),
                                                case.nt, STEPPERS[case.stepper], _alph(case), _lib.ptr(z), _lib.ptr(tab), _lib.ptr(sums),
                                                _lib.ptr(s_all), _lib.ptr(act), C.byref(recorded), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    _lib.check(rc, "nocf_rollout_record_act_f32")
    torch.cuda.synchronize()
    return s_all, act, recorded.value, z


@pytest.mark.parametrize("case", RECORD, ids=lambda c: c.id)
def test_recording_forward_against_fp64(case, knobs, capfd):
    D, net, prob, x = _setup(case, train=True)
    n, d, m = case.n, case.d, case.m
    E = case.nt * (4 if case.stepper == "rk4" else 1)
    knobs(NOCF_DEBUG="1")
    capfd.readouterr()
    s_all, act, recorded, z = _record(case, x, net, prob)
    assert kernel() == "rollout_mono_kernel" and _debug_shapes(capfd.readouterr().err) == [case.shape]
    expect = um.mono_record_eligible(case.nTh, m, d, case.r, case.n_agents)
    nact = int(_lib.lib().nocf_activation_record_floats(d, m, case.nTh, n, case.nt, STEPPERS[case.stepper]))
    assert nact == (act.numel() if expect else 0)
    assert recorded == int(expect)
    # the stage inputs: the states under the rule, the time column within the roundings of nt + 2 fp32 additions
    s = s_all.cpu()
    res = {"s_all": uo.compare(s[:, :, :d].permute(1, 0, 2), D["r64"]["stages"][:, :E], D["r32"]["stages"][:, :E]),
           "z": uo.compare(z.cpu(), D["r64"]["z"], D["r32"]["z"])}
    tt = torch.tensor(um.stage_times(case), dtype=torch.float64).reshape(E, 1).expand(E, n)
    assert float((s[:, :, d].double() - tt).abs().max()) <= (case.nt + 2) * 2.0 ** -23
    if not expect:
        assert bool(act.isnan().all()), "no record announced, but the buffer was written"
    else:
        a = act.cpu()
        assert not bool(a.isnan().any()), "the record has rows nobody wrote"
        sec = [a[k * E * n * m:(k + 1) * E * n * m].reshape(E, n, m) for k in range(4)] + [a[4 * E * n * m:].reshape(E, n, d + 1)]
        a64, a32 = um.oracle_activations(case, s)                      # at the kernel's own recorded stage inputs
        for name, got in zip(um.SECTIONS, sec):
            res["record." + name] = uo.compare(got, a64[name], a32[name])
    _check(res, case.id)


# ---- adjoint
def _grad_check(got, want64, ref32, what):
    res = {}
    for k in want64:
        w = want64[k] if want64[k] is not None else torch.zeros_like(got[k], dtype=torch.float64)
        r = ref32[k] if ref32[k] is not None else torch.zeros_like(got[k])
        res[k] = uo.compare(got[k], w, r)
    _check(res, what)


def _adjoint(case, fwd_kernel, bwd_kernel):
    D, net, prob, x = _setup(case, train=True)
    xx = x.clone().requires_grad_(True)
    Jc, cs = ocflow_train(xx, net, prob, list(case.tspan), case.nt, case.stepper, case.alph, n_total=case.n_total)
    assert kernel() == fwd_kernel, kernel()
    Jc.backward()
    torch.cuda.synchronize()
    assert kernel() == bwd_kernel, kernel()
    _check(um.compare_forward(dict(Jc=Jc.detach().cpu(), cs=torch.stack(list(cs)).detach().cpu()), D["r64"], D["r32"]), case.id)
    J64, g64, x64 = um.oracle_grads(case, D["x"], torch.float64)
    J32, g32, x32 = um.oracle_grads(case, D["x"], torch.float32)
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    got["x"] = xx.grad.cpu()
    g64["x"], g32["x"] = x64, x32
    _grad_check(got, g64, g32, case.id)


@pytest.mark.parametrize("case", um.ADJOINT, ids=lambda c: c.id)
def test_adjoint_against_fp64_autograd(case, knobs):
    if not case.act_rec:
        knobs(NOCF_ACT_REC="0")
    if case.n >= um.BIG:
        poison_allocator(DEV, big=2)               # (more than 1024 tiles: a row read before it is written must not find an earlier run's values)
    _adjoint(case, "rollout_mono_kernel", "rollout_mono_bwd_kernel")


def test_narrow_quadcopter_training_runs_the_mono_forward_and_the_tile_adjoint():
    case = next(c for c in SMALL if c.kind == "quad" and c.m <= 32 and c.mode == "train" and c.n >= 16)
    assert not um.mono_adjoint_eligible(case.nTh, case.m, case.d, case.r, case.n_agents)
    _adjoint(case, "rollout_mono_kernel", "rollout_bwd_kernel")


# ---- nocf_rollout_segments_f32
SENTINEL = -1234.5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _untouched(t):
    return bool((_bits(t) == _bits(torch.tensor([SENTINEL], device=t.device))).all())


def _segments(case, net, prob, x, n, nseg, rows, t0s, t1, nts, slot0s, slots, full=True):
    """nocf_rollout_segments_f32 into sentinel-filled buffers -> (rc, persample, z_out, sums, zFull, ctrlFull)"""
    phi_st, keep1, ws = net._c_struct(max(n, 1))
    prob_st, keep2 = prob._c_struct(DEV)
    cdim = _lib.lib().nocf_ctrl_dim(C.byref(prob_st), case.d)
    rows_alloc = max(n, 1)
    tab = torch.full((rows_alloc, 7), SENTINEL, device=DEV)
    z = torch.full((rows_alloc, case.d + 4), SENTINEL, device=DEV)
    sums = torch.full((max(nseg, 1), 8), SENTINEL, device=DEV)
    zF = torch.full((slots, rows_alloc, case.d + 4), SENTINEL, device=DEV) if full else None
    cF = torch.full((slots, rows_alloc, cdim), SENTINEL, device=DEV) if full else None
    k = len(t0s)
    rc = _lib.lib().nocf_rollout_segments_f32(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), n, nseg, rows, (C.c_double * k)(*t0s), float(t1),
                                              (C.c_int32 * k)(*nts), (C.c_int32 * k)(*slot0s) if slot0s is not None else None,
                                              STEPPERS[case.stepper], _alph(case), _lib.ptr(z), _lib.ptr(tab), _lib.ptr(sums), _lib.ptr(zF),
                                              _lib.ptr(cF), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return rc, tab, z, sums, zF, cF


def _supported(net, prob):
    phi_st, keep1, ws = net._c_struct(16)
    prob_st, keep2 = prob._c_struct(DEV)
    return int(_lib.lib().nocf_segments_supported(C.byref(phi_st), C.byref(prob_st)))


@pytest.mark.parametrize("layout", um.SEGMENT_LAYOUTS, ids=lambda s: f"nseg{s[0]}x{s[1]}-last{s[2]}")
@pytest.mark.parametrize("case", um.SEGMENTS, ids=lambda c: c.id)
def test_segments_bitwise_against_per_segment_calls(case, layout):
    nseg, rows, last = layout
    t0s, nts, slot0s = um.segment_plan(nseg)
    net, prob = um.make_net(case, DEV).eval(), um.make_problem(case, DEV)
    assert _supported(net, prob) == int(um.mono_forward_eligible(case.nTh, case.m, case.d, case.r, KINDS[case.kind], case.n_agents, lane=False)) == 1
    segs = [dataclasses.replace(case, n=(rows if k < nseg - 1 else last), nt=nts[k], tspan=(t0s[k], 1.0), draw=11 * k)
            for k in range(nseg)]
    data = [um.case_data(s) for s in segs]
    x = torch.cat([D["x"] for D in data]).contiguous().to(DEV)
    n = x.shape[0]
    assert n == (nseg - 1) * rows + last
    slots = max(s0 + v for s0, v in zip(slot0s, nts)) + 3
    rc, tab, z, sums, zF, cF = _segments(case, net, prob, x, n, nseg, rows, t0s, 1.0, nts, slot0s, slots)
    assert rc == 0 and kernel() == "rollout_mono_kernel"
    res = {}
    for k, (s, D) in enumerate(zip(segs, data)):
        r0 = k * rows
        tk, zk, sk, zFk, cFk = _raw(s, x[r0:r0 + s.n].contiguous(), net, prob, full=True)
        assert kernel() == "rollout_mono_kernel"
        assert torch.equal(_bits(tab[r0:r0 + s.n]), _bits(tk)) and torch.equal(_bits(z[r0:r0 + s.n]), _bits(zk)), f"segment {k}"
        assert torch.equal(_bits(sums[k]), _bits(sk)), f"segment {k}: sums"
        lo, hi = slot0s[k], slot0s[k] + nts[k] + 1
        assert torch.equal(_bits(zF[lo:hi, r0:r0 + s.n]), _bits(zFk)) and torch.equal(_bits(cF[lo:hi, r0:r0 + s.n]), _bits(cFk)), f"segment {k}"
        for buf in (zF, cF):                                          # every slot outside the segment's window keeps the sentinel
            assert _untouched(buf[:lo, r0:r0 + s.n]) and _untouched(buf[hi:, r0:r0 + s.n]), f"segment {k}: a slot outside its window was written"
        sc = sums[k].cpu()
        assert float(sc[7]) == s.n
        got = dict(cs=sc[:7] / sc[7], table=tab[r0:r0 + s.n].cpu(), z=z[r0:r0 + s.n].cpu())
        res.update({f"seg{k}.{q}": v for q, v in um.compare_forward(got, D["r64"], D["r32"]).items()})
    _check(res, case.id)


def test_segments_refuse_bad_arguments_before_any_launch():
    case = um.SEGMENTS[0]
    net, prob = um.make_net(case, DEV).eval(), um.make_problem(case, DEV)
    x = um.candidates(dataclasses.replace(case, n=64), 17 * 16).to(DEV)
    ok3 = ([0.1, 0.2, 0.3], [2, 3, 1], [0, 1, 2])
    bad = [("nseg = 17", 17 * 16, 17, 16, [0.1] * 17, [1] * 17, [0] * 17),
           ("rows_per_seg = 24", 60, 3, 24, *ok3), ("rows_per_seg = 0", 40, 3, 0, *ok3),
           ("n = (nseg - 1) rows", 32, 3, 16, *ok3), ("n = nseg rows + 1", 49, 3, 16, *ok3),
           ("nts entry 0", 40, 3, 16, ok3[0], [2, 0, 1], ok3[2]), ("negative slot", 40, 3, 16, ok3[0], ok3[1], [0, -1, 2])]
    for what, n, nseg, rows, t0s, nts, slot0s in bad:
        rc, *bufs = _segments(case, net, prob, x[:n].contiguous(), n, nseg, rows, t0s, 1.0, nts, slot0s, slots=8)
        assert rc == E_SHAPE, (what, rc)
        assert all(_untouched(b) for b in bufs), what
    rc, *bufs = _segments(case, net, prob, x[:40].contiguous(), 40, 3, 16, ok3[0], 1.0, ok3[1], ok3[2], slots=8)
    assert rc == 0 and not any(_untouched(b) for b in bufs)          # (the same call with good arguments runs)


def test_segments_without_a_one_cu_kernel_are_refused():
    wide = um.MonoCase("cross2d", 14, 129, 10, "softcorridor", "eval", 40, "rk4", 2, seed=3)
    net, prob = um.make_net(wide, DEV).eval(), um.make_problem(wide, DEV)
    assert _supported(net, prob) == 0 and not um.mono_plan_ok(2, 129, 14, 10, 7)
    x = um.candidates(wide, 40).to(DEV)
    rc, *bufs = _segments(wide, net, prob, x, 40, 3, 16, [0.1, 0.2, 0.3], 1.0, [2, 3, 1], [0, 1, 2], slots=8)
    assert rc == E_SHAPE and all(_untouched(b) for b in bufs)


# ---- eligibility boundaries: the kernel that runs, and the result against fp64
def _boundary(case):
    D, net, prob, x = _setup(case)
    ts = list(case.tspan)
    with torch.no_grad():
        Jc, cs = na.OCflow(x, net, prob, ts, case.nt, case.stepper, case.alph)
        k = [kernel()]
        _, csn = na.OCflow(x, net, prob, ts, case.nt, case.stepper, case.alph, noMean=True)
        k.append(kernel())
        zF, cF = na.OCflow(x[:8], net, prob, ts, case.nt, case.stepper, case.alph, intermediates=True)
        k.append(kernel())
    got = dict(Jc=Jc.cpu(), cs=torch.stack([c.reshape(()) for c in cs]).cpu(), table=torch.cat(csn, 1).cpu(), zFull=zF.cpu(), ctrlFull=cF.cpu())
    _check(um.compare_forward(got, D["r64"], D["r32"]), case.id)
    return k


@pytest.mark.parametrize("case", [
    um.MonoCase("cross2d", 14, 129, 10, "softcorridor", "eval", 21, "rk4", 7, seed=3),                  # m = 129
    um.MonoCase("cross2d", 32, 64, 10, None, "train", 18, "rk4", 7, seed=4),                            # d + 1 = 33
    um.MonoCase("cross2d", 14, 64, 10, "hardcorridor", "train", 19, "rk1", 9, seed=5, nTh=3),           # nTh = 3
], ids=["m129", "d32", "nTh3"])
def test_eligibility_boundaries(case):
    assert not um.mono_forward_eligible(case.nTh, case.m, case.d, case.r, KINDS[case.kind], case.n_agents)
    kernels = _boundary(case)
    assert "rollout_mono_kernel" not in kernels, kernels


def test_mono_switched_off(knobs):
    case = next(c for c in SMALL if c.shape == (8, 1) and c.n == 57)
    knobs(NOCF_MONO="0")
    kernels = _boundary(case)
    assert "rollout_mono_kernel" not in kernels, kernels


def test_mono_recording_switched_off(knobs):
    """NOCF_MONO_REC=0: evaluation stays on the one-CU kernel, the recording forward and the adjoint are the per-tile kernels'"""
    case = um.ADJOINT[0]
    knobs(NOCF_MONO_REC="0")
    assert _boundary(dataclasses.replace(case, mode="eval")) == ["rollout_mono_kernel"] * 3
    D, net, prob, x = _setup(case, train=True)
    s_all, act, recorded, z = _record(case, x, net, prob, with_act=False)
    assert kernel().startswith("rollout_kernel<") and recorded == 0
    assert int(_lib.lib().nocf_activation_record_floats(case.d, case.m, 2, case.n, case.nt, STEPPERS[case.stepper])) == 0
    E = s_all.shape[0]
    _check({"s_all": uo.compare(s_all.cpu()[:, :, :case.d].permute(1, 0, 2), D["r64"]["stages"][:, :E], D["r32"]["stages"][:, :E])}, case.id)


def test_mono_adjoint_switched_off(knobs):
    knobs(NOCF_MONO_BWD="0")
    _adjoint(um.ADJOINT[0], "rollout_mono_kernel", "rollout_bwd_kernel")


def test_rank_above_16_is_refused_before_any_launch():
    d, m, n = 16, 64, 5
    net = na.Phi(nTh=2, m=m, d=d, r=17).to(DEV)
    assert net.A.shape == (17, 17) and not um.mono_plan_ok(2, m, d, 17, 8)
    prob = na.Cross2D(torch.zeros(d, device=DEV), obstacle=None, alph_Q=1.0, alph_W=1.0, r=0.5)
    case = um.MonoCase("cross2d", d, m, 17, None, "eval", n, "rk4", 3)
    x = torch.zeros(n, d, device=DEV)
    with pytest.raises(RuntimeError, match="nocf_rollout_f32"):
        _raw(case, x, net, prob)
    assert _supported(net, prob) == 0
    L = _lib.lib()
    assert int(L.nocf_mid_grad_rows(d, m, 2, 17, 8, n)) == 0
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(DEV)
    gpart = torch.full((1, int(L.nocf_small_grad_floats(d, m))), float("nan"), device=DEV)
    z = torch.zeros(n, d + 4, device=DEV)
    s_all = torch.zeros(12, n, d + 1, device=DEV)
    hs = torch.full((3,), 1.0 / 3, device=DEV)
    rc = L.nocf_rollout_bwd_mid_f32(C.byref(phi_st), C.byref(prob_st), n, 3, _lib.NOCF_RK4, 1.0, (C.c_float * 6)(*[1.0] * 6), 0.2,
                                    _lib.ptr(s_all), _lib.ptr(z), _lib.ptr(hs), None, _lib.ptr(gpart), 1, None,
                                    _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == E_SHAPE and bool(gpart.isnan().all())
