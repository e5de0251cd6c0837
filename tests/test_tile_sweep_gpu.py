"""The per-tile kernels (csrc/nocf_kernels.hip rollout_kernel<S, Plan>, csrc/nocf_bwd.inc rollout_bwd_kernel<S, Plan>) at every plan
geometry against the oracle in fp64.

Each case of tests/util_tile.py runs on the MI355X under its knobs and is compared with fp64 under util_oracle's rule (4x the fp32
restatement's own error, with a floor): forward Jc, the means, the per-sample table, the final state and the intermediates; the recording
forward's stage inputs; the adjoint and the two stand-alone modes of its kernel against fp64 autograd, a batch of more than 4096 tiles
included.  Every test proves the geometry that ran from the NOCF_DEBUG line and nocf_last_rollout_kernel against the Python mirror of
plan_layout (tests/test_tile_sweep_cpu.py holds the mirror against the library).  The per-tile forward writes no activation record at any
depth (rollout_impl hands it none): the recording tests require the record buffer untouched; the adjoint reads the one-CU forward's record
in the two cases whose forward is that kernel's.  One yardstick is doubled: the residual layers' weight gradients
of the depth-12 adjoint case take the larger of two fp32 restatements' errors, the plain one and the one that forms sigma and tanh as the
kernels do (util_tile.kernel_activations); factor and floor are util_oracle's.  The tests named *forced* run the geometries only a knob reaches (NOCF_NWAVES,
NOCF_SUBTILES); they come last in the file so that a run can take them in a process of their own (-k forced / -k "not forced")."""
import ctypes as C
import os
import re

import pytest
import torch

import neuraloc_amd as na
import util_disturb as ud
import util_mono as um
import util_oracle as uo
import util_tile as ut
from neuraloc_amd import _lib
from neuraloc_amd.train import ocflow_train
from util_hip import poison_allocator

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
STEPPERS = {"rk4": _lib.NOCF_RK4, "rk1": _lib.NOCF_RK1}
SENTINEL = -1234.5
GENERIC, SPECIALISED = "rollout_kernel<generic>", "rollout_kernel<shape-specialised>"


def kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


@pytest.fixture
def knobs():
    """set NOCF_* knobs for one test: knobs(NOCF_MONO="0"); restored afterwards"""
    saved = {}

    def put(**kw):
        for k, v in kw.items():
            saved.setdefault(k, os.environ.get(k))
            os.environ[k] = str(v)
    yield put
    for k, v in saved.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


_FIGURES = []


@pytest.fixture(autouse=True)
def figures():
    """every measured error of the test, printed when it ends (what a test prints before it reads the captured [nocf] lines is consumed
    with them)"""
    del _FIGURES[:]
    yield
    print("\n".join(_FIGURES))


_GEO = r"T (\d+), (\d+) waves, SK1/SK6/SKm (\d+)/(\d+)/(\d+), cap (\d+), LDS (\d+) B/workgroup"


def _forward_lines(err):
    """the [nocf] lines of the per-tile forward launches, in order: a geometry tuple (generic) or "specialised" """
    out = []
    for line in err.splitlines():
        g = re.search(r"\[nocf\] generic rollout kernel: " + _GEO, line)
        if g:
            out.append(tuple(int(v) for v in g.groups()))
        elif "[nocf] shape-specialised rollout kernel" in line:
            out.append("specialised")
    return out


def _adjoint_lines(err):
    """-> [(specialised / generic, the geometry ..., "from the record" / "recomputed")] of the per-tile adjoint launches"""
    return [(g.group(1),) + tuple(int(v) for v in g.groups()[1:-1]) + (g.group(9),)
            for g in re.finditer(r"\[nocf\] (specialised|generic) rollout adjoint kernel: " + _GEO + r", activations (from the record|recomputed)", err)]


def _geometry(p):
    return (p["T"], p["nwaves"], p["SK1"], p["SK6"], p["SKm"], p["cap"], 4 * p["ldsFloats"])


def _setup(tc, knobs, train=False):
    case = tc.case
    D = um.case_data(case)
    knobs(NOCF_DEBUG="1", **tc.env)
    net = um.make_net(case, DEV)
    net.train() if train else net.eval()
    return D, net, um.make_problem(case, DEV), D["x"].to(DEV)


def _alph(case):
    return (C.c_float * 6)(*[float(a) for a in case.alph])


def _raw(case, x, net, prob):
    """nocf_rollout_f32 into NaN-filled buffers -> (persample [n, 7], z [n, d+4])"""
    n = x.shape[0]
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(DEV)
    tab = torch.full((n, 7), float("nan"), device=DEV)
    z = torch.full((n, case.d + 4), float("nan"), device=DEV)
    sums = torch.full((8,), float("nan"), device=DEV)
    rc = _lib.lib().nocf_rollout_f32(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), n, float(case.tspan[0]), float(case.tspan[1]), case.nt,
                                     STEPPERS[case.stepper], _alph(case), _lib.ptr(z), _lib.ptr(tab), _lib.ptr(sums), None, None,
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    _lib.check(rc, "nocf_rollout_f32")
    torch.cuda.synchronize()
    return tab, z


def _forward(case, x, net, prob):
    """the five forward calls of a case -> (dict for um.compare_forward, kernel name of each call)"""
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
        tab2, z2 = _raw(case, x, net, prob)
        k.append(kernel())
    got = dict(Jc=Jc.cpu(), cs=torch.stack([c.reshape(()) for c in cs]).cpu(), table=torch.cat(csn, 1).cpu(), z=z.cpu(),
               zFull=zF.cpu(), ctrlFull=cF.cpu())
    assert torch.equal(got["table"], tab.cpu()), "noMean's table differs from nocf_rollout_f32's"
    assert torch.equal(tab, tab2) and torch.equal(z, z2), "not run-to-run deterministic"
    assert float(cF[:, :, 0].abs().max()) == 0.0                      # slot 0 of the controls is exactly zero
    return got, k


def _check(res, what):
    for k, (ok, e, t, e32) in res.items():
        _FIGURES.append(f"{what} {k}: err {e:.3e} tol {t:.3e} fp32 oracle {e32:.3e}")
    bad = um.failures(res)
    assert not bad, f"{what}: " + "; ".join(f"{k}: err {e:.3g} > tol {t:.3g} (fp32 oracle {e32:.3g})" for k, (_, e, t, e32) in bad.items())


def _run_forward(tc, knobs, capfd):
    D, net, prob, x = _setup(tc, knobs)
    if tc.case.n >= ut.BIG:
        poison_allocator(DEV, big=2)               # (more than 4096 tiles: a row read before it is written must not find an earlier run's values)
    capfd.readouterr()
    got, kernels = _forward(tc.case, x, net, prob)
    lines = _forward_lines(capfd.readouterr().err)
    if tc.specialised():
        assert kernels == [SPECIALISED] * 5 and lines == ["specialised"] * 5, (kernels, lines)
    else:
        assert kernels == [GENERIC] * 5, kernels
        assert lines == [_geometry(tc.plan())] * 5, (lines, _geometry(tc.plan()))
    _check(um.compare_forward(got, D["r64"], D["r32"]), tc.id)


# ---- recording forward: the stage inputs
def _record(case, x, net, prob):
    """nocf_rollout_record_act_f32 -> (s_all [E, n, d+1], act (NaN-filled before the call, sized for a record), recorded, z)"""
    n, d, m = x.shape[0], case.d, case.m
    E = case.nt * (4 if case.stepper == "rk4" else 1)
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(DEV)
    tab = torch.empty(n, 7, device=DEV)
    z = torch.full((n, d + 4), float("nan"), device=DEV)
    sums = torch.empty(8, device=DEV)
    s_all = torch.full((E, n, d + 1), float("nan"), device=DEV)
    act = torch.full((E * n * (4 * m + d + 1),), float("nan"), device=DEV)
    recorded = C.c_int32(-1)
    rc = _lib.lib().nocf_rollout_record_act_f32(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), n, float(case.tspan[0]), float(case.tspan[1]),
                                                case.nt, STEPPERS[case.stepper], _alph(case), _lib.ptr(z), _lib.ptr(tab), _lib.ptr(sums),
                                                _lib.ptr(s_all), _lib.ptr(act), C.byref(recorded), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    _lib.check(rc, "nocf_rollout_record_act_f32")
    torch.cuda.synchronize()
    return s_all, act, recorded.value, z


def _run_record(tc, knobs, capfd):
    case = tc.case
    D, net, prob, x = _setup(tc, knobs, train=True)
    n, d = case.n, case.d
    E = case.nt * (4 if case.stepper == "rk4" else 1)
    capfd.readouterr()
    s_all, act, recorded, z = _record(case, x, net, prob)
    lines = _forward_lines(capfd.readouterr().err)
    if tc.specialised(recording=True):
        assert kernel() == SPECIALISED and lines == ["specialised"], (kernel(), lines)
    else:
        assert kernel() == GENERIC and lines == [_geometry(tc.plan())], (kernel(), lines)
    # the per-tile forward writes no activation record, at any depth: none announced, the buffer as it was
    assert recorded == 0 and bool(act.isnan().all()), "no record announced, but the buffer was written"
    if case.nTh > 2:
        assert int(_lib.lib().nocf_activation_record_floats(d, case.m, case.nTh, n, case.nt, STEPPERS[case.stepper])) == 0
    s = s_all.cpu()
    assert not bool(s.isnan().any()), "stage inputs nobody wrote"
    res = {"s_all": uo.compare(s[:, :, :d].permute(1, 0, 2), D["r64"]["stages"][:, :E], D["r32"]["stages"][:, :E]),
           "z": uo.compare(z.cpu(), D["r64"]["z"], D["r32"]["z"])}
    tt = torch.tensor(um.stage_times(case), dtype=torch.float64).reshape(E, 1).expand(E, n)
    assert float((s[:, :, d].double() - tt).abs().max()) <= (case.nt + 2) * 2.0 ** -23
    _check(res, tc.id)


# ---- adjoint
def _grad_check(got, want64, ref32, what, second=None, pattern=None):
    """second / pattern: a second fp32 restatement's gradients and the names whose yardstick is the larger of the two restatements' errors"""
    res = {}
    for k in want64:
        w = want64[k] if want64[k] is not None else torch.zeros_like(got[k], dtype=torch.float64)
        r = ref32[k] if ref32[k] is not None else torch.zeros_like(got[k])
        res[k] = uo.compare(got[k], w.reshape(got[k].shape), r.reshape(got[k].shape))
        if pattern and re.fullmatch(pattern, k):
            alt = uo.compare(got[k], w.reshape(got[k].shape), second[k].reshape(got[k].shape))
            _FIGURES.append(f"{what} {k}: fp32 oracle {res[k][3]:.3e}, under the kernels' activation arithmetic {alt[3]:.3e}")
            res[k] = max(res[k], alt, key=lambda v: v[2])
    _check(res, what)


def _run_adjoint(tc, knobs, capfd):
    case = tc.case
    D, net, prob, x = _setup(tc, knobs, train=True)
    if case.n >= ut.BIG:
        poison_allocator(DEV, big=2)
    # the adjoint loads the activations only where the forward was the one-CU kernel's and its record was not switched off
    rec = tc.fwd == "mono" and case.act_rec
    want = ("specialised" if tc.specialised(bwd=1) else "generic",) + _geometry(tc.plan(1)) + ("from the record" if rec else "recomputed",)
    xx = x.clone().requires_grad_(True)
    capfd.readouterr()
    Jc, cs = ocflow_train(xx, net, prob, list(case.tspan), case.nt, case.stepper, case.alph, n_total=case.n_total)
    fwd = "rollout_mono_kernel" if tc.fwd == "mono" else SPECIALISED if tc.specialised(recording=True) else GENERIC
    assert kernel() == fwd, kernel()
    assert (getattr(Jc.grad_fn, "act", None) is not None) == rec, "the forward's activation record: announced and kept exactly where expected"
    Jc.backward()
    torch.cuda.synchronize()
    assert kernel() == "rollout_bwd_kernel", kernel()
    assert _adjoint_lines(capfd.readouterr().err) == [want]
    got_cs = torch.stack(list(cs)).detach().cpu()
    _check(um.compare_forward(dict(Jc=Jc.detach().cpu(), cs=got_cs), D["r64"], D["r32"]), tc.id)
    if tc.id in ut.SECOND_YARDSTICK:
        # what entitles the case to its second yardstick: where the activation arithmetic dominates, the kernel's forward error is that
        # arithmetic's.  A mean that the restatement under util_tile.kernel_activations puts more than twice as far from fp64 as the plain
        # fp32 run does is as far off in the kernel, within a factor 2 either way; there must be such a mean
        with ut.kernel_activations():
            rk = um.oracle_forward(case, D["x"], torch.float32, rows=0)
        told = 0
        for c in range(5):
            e_gpu, e_k, e_32 = (abs(float(v[c]) - float(D["r64"]["cs"][c])) for v in (got_cs, rk["cs"], D["r32"]["cs"]))
            _FIGURES.append(f"{tc.id} cs[{c}]: err {e_gpu:.3e}, fp32 oracle {e_32:.3e}, under the kernels' activation arithmetic {e_k:.3e}")
            if e_k > 2.0 * e_32:
                told += 1
                assert 0.5 * e_k <= e_gpu <= 2.0 * e_k, (c, e_gpu, e_k, e_32)
        assert told >= 1, "the two restatements no longer tell apart: the second yardstick has lost its reason"
    J64, g64, x64 = um.oracle_grads(case, D["x"], torch.float64)
    J32, g32, x32 = um.oracle_grads(case, D["x"], torch.float32)
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    got["x"] = xx.grad.cpu()
    g64["x"], g32["x"] = x64, x32
    pattern = ut.SECOND_YARDSTICK.get(tc.id)
    _grad_check(got, g64, g32, tc.id, ut.oracle_grads_kernel_activations(case, D["x"])[1] if pattern else None, pattern)
    # the stand-alone modes of the same kernel: sum Phi(s) and <g, grad Phi(s)> under autograd, on the same plan
    s, g = ut.standalone_inputs(case, 19)
    ref64, ref32 = ut.standalone_grads(case, s, g, torch.float64), ut.standalone_grads(case, s, g, torch.float32)
    p1 = ut.tile_plan(case.d, case.m, case.nTh, case.r, 1, 1, tc.nw, tc.S)            # (no physics on these paths: the plan of one agent)
    want = ("specialised" if p1["fixed"] and tc.env.get("NOCF_FIXED") != "0" else "generic",) + _geometry(p1) + ("recomputed",)
    for mode, (w64, w32) in enumerate(zip(ref64, ref32)):
        net.zero_grad()
        ss = s.to(DEV).requires_grad_(True)
        capfd.readouterr()
        if mode == 0:
            net(ss).sum().backward()
        else:
            net.getGrad(ss).backward(g.float().to(DEV))
        torch.cuda.synchronize()
        assert kernel() == "rollout_bwd_kernel" and _adjoint_lines(capfd.readouterr().err) == [want], mode
        got = {k: p.grad.detach().cpu() if p.grad is not None else torch.zeros(p.shape) for k, p in net.named_parameters()}
        got["x"] = ss.grad.cpu()
        _grad_check(got, w64, w32, f"{tc.id} {'net(x).sum()' if mode == 0 else 'getGrad(x) . g'}")


# ---- the default geometry
@pytest.mark.parametrize("tc", ut.FORWARD_DEFAULT, ids=lambda tc: tc.id)
def test_forward_against_fp64(tc, knobs, capfd):
    _run_forward(tc, knobs, capfd)


@pytest.mark.parametrize("tc", ut.FIXED_EVAL, ids=lambda tc: tc.id)
def test_specialised_forward_against_fp64(tc, knobs, capfd):
    _run_forward(tc, knobs, capfd)


@pytest.mark.parametrize("tc", [t for t in ut.FORWARD_DEFAULT if t.case.mode == "train"] + ut.FIXED_TRAIN, ids=lambda tc: tc.id)
def test_recording_forward_against_fp64(tc, knobs, capfd):
    _run_record(tc, knobs, capfd)


@pytest.mark.parametrize("tc", [t for t in ut.ADJOINT if not t.nw], ids=lambda tc: tc.id)
def test_adjoint_against_fp64_autograd(tc, knobs, capfd):
    _run_adjoint(tc, knobs, capfd)


# ---- refusals: clean codes, outputs untouched
def _bits(t):
    return t.contiguous().view(torch.int32)


def _untouched(t):
    return bool((_bits(t) == _bits(torch.tensor([SENTINEL], device=t.device))).all())


def _hand_phi(case):
    """a NocfPhi of the case's shape over zero weights, with a workspace of its own (the module refuses to size one for a shape without a plan)"""
    d, m, nTh, r = case.d, case.m, case.nTh, case.r
    t = dict(K0=torch.zeros(m, d + 1, device=DEV), b0=torch.zeros(m, device=DEV), K=torch.zeros(nTh - 1, m, m, device=DEV),
             b=torch.zeros(nTh - 1, m, device=DEV), w=torch.zeros(m, device=DEV), A=torch.zeros(r, d + 1, device=DEV),
             cw=torch.zeros(d + 1, device=DEV), cb_dev=torch.zeros(1, device=DEV))
    st = _lib.NocfPhi()
    st.d, st.m, st.nTh, st.r, st.cb = d, m, nTh, r, 0.0
    for k, v in t.items():
        setattr(st, k, v.data_ptr())
    return st, t, torch.zeros(64 << 20, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("ref", ut.REFUSALS, ids=lambda r: r[0].replace(" ", "_"))
def test_refusals_return_codes_and_leave_the_outputs_untouched(ref, knobs):
    what, case, kn, bwd, code = ref
    knobs(**kn)
    n, d, m, L = case.n, case.d, case.m, case.nTh - 1
    E = case.nt * 4
    prob = um.make_problem(case, DEV)
    prob_st, keep2 = prob._c_struct(DEV)
    phi_st, keep1, ws = _hand_phi(case)
    x = torch.zeros(n, d, device=DEV)
    S = lambda *shape: torch.full(shape, SENTINEL, device=DEV)                       # noqa: E731
    lib = _lib.lib()
    _lib.watch_env(lib)
    if not bwd:
        bufs = [S(n, d + 4), S(n, 7), S(8)]
        rc = lib.nocf_rollout_f32(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), n, 0.0, 1.0, case.nt, _lib.NOCF_RK4, _alph(case),
                                  _lib.ptr(bufs[0]), _lib.ptr(bufs[1]), _lib.ptr(bufs[2]), None, None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    else:
        rows = (E + 2) * n
        s_all, z, hs = torch.zeros(E, n, d + 1, device=DEV), torch.zeros(n, d + 4, device=DEV), torch.full((case.nt,), 1.0 / case.nt, device=DEV)
        bufs = [S(rows, m), S(rows, m), S(L, rows, m), S(L, rows, m), S(L, rows, m), S(L, rows, m), S(rows, m), S(rows, d + 1), S(rows, d + 1),
                S(n), S(n, d)]
        rc = lib.nocf_rollout_bwd_act_f32(C.byref(phi_st), C.byref(prob_st), n, case.nt, _lib.NOCF_RK4, 1.0, _alph(case), 1.0 / n,
                                          _lib.ptr(s_all), _lib.ptr(z), _lib.ptr(hs), *[_lib.ptr(b) for b in bufs], None,
                                          _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert rc == code, (what, rc)
    assert all(_untouched(b) for b in bufs), what


def test_python_layer_names_the_refusal(knobs):
    """the Python layer raises RuntimeError naming the code: NOCF_E_LDS for the adjoint of m = 1024 and for a forward of m = 2048 at d = 150,
    NOCF_E_SHAPE for the adjoint under NOCF_SUBTILES=2 (whose T = 8 forward runs)"""
    what, case, kn, bwd, code = ut.REFUSALS[1]
    net, prob = um.make_net(case, DEV).train(), um.make_problem(case, DEV)
    x = um.candidates(case, case.n).to(DEV)
    Jc, _ = ocflow_train(x, net, prob, [0.0, 1.0], case.nt, case.stepper, case.alph)
    assert kernel() == GENERIC
    with pytest.raises(RuntimeError, match="NOCF_E_LDS"):
        Jc.backward()
    what, case, kn, bwd, code = ut.REFUSALS[2]
    net, prob = um.make_net(case, DEV).eval(), um.make_problem(case, DEV)
    with pytest.raises(RuntimeError, match="NOCF_E_LDS"), torch.no_grad():
        na.OCflow(um.candidates(case, case.n).to(DEV), net, prob, [0.0, 1.0], case.nt, case.stepper, case.alph)


# ---- the geometries only a knob reaches (NOCF_NWAVES, NOCF_SUBTILES): last in the file
@pytest.mark.parametrize("tc", ut.FORWARD_FORCED, ids=lambda tc: tc.id)
def test_forced_geometry_forward_against_fp64(tc, knobs, capfd):
    _run_forward(tc, knobs, capfd)


@pytest.mark.parametrize("tc", [t for t in ut.FORWARD_FORCED if t.case.mode == "train"], ids=lambda tc: tc.id)
def test_forced_geometry_recording_forward_against_fp64(tc, knobs, capfd):
    _run_record(tc, knobs, capfd)


@pytest.mark.parametrize("tc", ut.DISTURBED, ids=lambda tc: tc.id)
def test_forced_geometry_disturbed_rollout_against_fp64(tc, knobs, capfd):
    """rollout_kernel<2, DynPlan, true> and <4, DynPlan, true> (T = 4 is in tests/test_disturb_gpu.py)"""
    case = tc.case
    data = ud.case_data(case)
    knobs(NOCF_DEBUG="1", **tc.env)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    capfd.readouterr()
    with torch.no_grad():
        out = na.disturbed_rollout(data["x"].to(DEV), net, prob, case.nt, data["W"].to(DEV), tspan=case.tspan, alph=case.alph,
                                   stepper=case.stepper, intermediates=True)
    torch.cuda.synchronize()
    assert kernel() == "rollout_kernel<generic, dist>" and _forward_lines(capfd.readouterr().err) == [_geometry(tc.plan())]
    got = dict(table=out["persample"], z=out["z_final"], zFull=out["traj"], ctrlFull=out["ctrl"])
    _check(ud.compare(got, data["r64"], data["r32"]), tc.id)


@pytest.mark.parametrize("tc", [t for t in ut.ADJOINT if t.nw], ids=lambda tc: tc.id)
def test_forced_geometry_adjoint_against_fp64_autograd(tc, knobs, capfd):
    _run_adjoint(tc, knobs, capfd)


def test_forced_geometry_adjoint_under_subtiles_is_refused_by_the_python_layer(knobs):
    what, case, kn, bwd, code = ut.REFUSALS[0]
    knobs(**kn)
    net, prob = um.make_net(case, DEV).train(), um.make_problem(case, DEV)
    Jc, _ = ocflow_train(um.candidates(case, case.n).to(DEV), net, prob, [0.0, 1.0], case.nt, case.stepper, case.alph)
    assert kernel() == GENERIC
    with pytest.raises(RuntimeError, match="NOCF_E_SHAPE"):
        Jc.backward()
