"""The double-precision kernels (csrc/nocf_f64.inc rollout_f64_kernel<T, WIDE>, phi_f64_kernel<T, WIDE>, prob_f64_kernel<4>;
csrc/nocf_f64_bwd.inc rollout_bwd_f64_kernel<T, true>, rollout_bwd_f64_narrow_kernel<T>) at every instantiation against extended precision.

Each case of tests/util_f64.py runs on the MI355X and is compared with the numpy.longdouble restatement (values) and its complex-step
directional derivatives (gradients) under util_f64's rule: TOL_FACTOR x the torch-fp64 oracle's own error against the same truth, floor
TOL_FLOOR * 2**-29 of the scale (util_oracle's factor and floor, precisions shifted).  The truth covers a subset of rows (first, middle and
last workgroup, the ragged tail); every row is additionally held to the existing 1e-9 comparison against the torch-fp64 oracle.  Every test
proves its instantiation from the NOCF_DEBUG line against the Python mirror of the plan (tests/test_f64_sweep_cpu.py holds the mirror against
the library).  The tests named *forced* run the adjoint instantiations under NOCF_F64_BWD_T; they come last so that a run can take them in a
process of their own (-k forced / -k "not forced").  The last test prints, per family, the largest err / tol / oracle-error triple.

The entries of util_f64.SECOND, keyed by case and quantity, take the larger of two fp64 restatements' errors as their yardstick, factor and
floor unchanged; tests/test_f64_sweep_cpu.py shows for each that the second restatement is that far from the truth.  Every other
quantity is held to the oracle's error alone.  prob_f64_kernel has one instantiation and prints no NOCF_DEBUG line, and the cost-sum test
runs the recording entry whose instantiations the rollout tests prove: those two groups of tests prove none."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import neuraloc_amd as na
import util_f64 as uf
from neuraloc_amd import _lib
from util_f64 import ADJOINT, ALPH, PHI, ROLLOUT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64 = torch.float64
STEPPERS = {"rk4": _lib.NOCF_RK4, "rk1": _lib.NOCF_RK1}
U = 2.0 ** -53


@pytest.fixture
def knobs():
    """set NOCF_* knobs for one test; restored afterwards"""
    saved = {}

    def put(**kw):
        for k, v in kw.items():
            saved.setdefault(k, os.environ.get(k))
            os.environ[k] = str(v)
    yield put
    for k, v in saved.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


_WORST = {}            # family -> (err / tol, name, err, tol, oracle error)
_FIGURES = []


@pytest.fixture(autouse=True)
def figures():
    """every measured error of the test, printed when it ends (what a test prints before it reads the captured [nocf] lines is consumed
    with them)"""
    del _FIGURES[:]
    yield
    print("\n".join(_FIGURES))
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                   # a sticky GPU error: nothing more is started on the card
        pytest.exit(f"GPU error after this test: {e}", 3)


def _check(res, family, what):
    for k, (ok, e, t, e64) in res.items():
        _FIGURES.append(f"{what} {k}: err {e:.3e} tol {t:.3e} fp64 oracle {e64:.3e}")
        ratio = e / t if t > 0 else (0.0 if e == 0 else float("inf"))
        if family not in _WORST or ratio > _WORST[family][0]:
            _WORST[family] = (ratio, f"{what} {k}", e, t, e64)
    bad = uf.failures(res)
    assert not bad, f"{what}: " + "; ".join(f"{k}: err {e:.3g} > tol {t:.3g} (fp64 oracle {e64:.3g})" for k, (_, e, t, e64) in bad.items())


def _lines(err, entry):
    """the [nocf] lines of one double-precision entry ("f64 kernel" / "f64 adjoint kernel" / "f64 phi kernel") -> [(T, wide, LDS bytes)]"""
    pat = r"\[nocf\] " + entry + r": (\d+) sample\(s\) per workgroup, wide (\d), LDS (\d+) B"
    return [tuple(int(v) for v in g.groups()) for g in re.finditer(pat, err)]


def _want_line(case, which, n=None):
    p = case.plan(which, n)
    assert p["rc"] == 0
    return (p["T"], p["wide"], 8 * p["lds"])


def _np(t):
    return t.detach().cpu().numpy()


def _record(case, x, net, prob):
    """nocf_rollout_record_f64 into NaN-filled buffers -> s_all [E, n, d+1], z [n, d+4], table [n, 7], sums [8]"""
    n, d = x.shape
    E = case.nt * (4 if case.stepper == "rk4" else 1)
    phi_st, keep1, ws = net._c_struct64()
    prob_st, keep2 = prob._c_struct64(DEV)
    nan = dict(dtype=F64, device=DEV)
    tab, z, sums = torch.full((n, 7), float("nan"), **nan), torch.full((n, d + 4), float("nan"), **nan), torch.full((8,), float("nan"), **nan)
    s_all = torch.full((E, n, d + 1), float("nan"), **nan)
    rc = _lib.lib().nocf_rollout_record_f64(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), n, float(case.tspan[0]), float(case.tspan[1]), case.nt,
                                            STEPPERS[case.stepper], (C.c_double * 6)(*ALPH), _lib.ptr(z), _lib.ptr(tab), _lib.ptr(sums),
                                            _lib.ptr(s_all), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    _lib.check(rc, "nocf_rollout_record_f64")
    torch.cuda.synchronize()
    return s_all, z, tab, sums


def _mean_bound(col, n):
    """the kernel's fixed-order column sum (256 strided partial sums of ceil(n / 256) terms, an 8-level tree) divided by n, against the
    longdouble mean: at most ceil(n / 256) + 8 roundings of the sum and one of the division, each 2**-53 relative to the sum of |x_i|"""
    return (uf.cdiv(n, 256) + 10) * U * float(np.abs(col).astype(uf.LD).sum() / n)


def _run_rollout(case, knobs, capfd, family):
    knobs(NOCF_DEBUG="1")
    net, prob = uf.make_net(case, DEV), uf.make_prob(case, DEV)
    x = uf.starts(case).to(DEV)
    ts, n, d = list(case.tspan), case.n, case.d
    capfd.readouterr()
    with torch.no_grad():
        Jc, cs = na.OCflow(x, net, prob, ts, case.nt, case.stepper, list(ALPH))
        _, csn = na.OCflow(x, net, prob, ts, case.nt, case.stepper, list(ALPH), noMean=True)
        zF, cF = na.OCflow(x, net, prob, ts, case.nt, case.stepper, list(ALPH), intermediates=True)
    s_all, z, tab2, sums = _record(case, x, net, prob)
    lines = _lines(capfd.readouterr().err, "f64 kernel")
    assert lines == [_want_line(case, ROLLOUT)] * 4, (lines, _want_line(case, ROLLOUT))
    assert _lib.lib().nocf_last_rollout_kernel().decode() == "rollout_f64_kernel"
    tab = torch.cat(csn, 1)
    assert tab.dtype == F64 and torch.equal(tab, tab2), "the recording forward's table differs from the plain one's"
    t, o = uf.truth(case), uf.oracle(case)
    rows = t["rows"]
    tab, s_all, z, zF, cF = _np(tab), _np(s_all), _np(z), _np(zF), _np(cF)
    for a in (tab, s_all, z, zF, cF):
        assert not np.isnan(a).any(), "a row was not written"
    # every row: the existing double-against-double comparison
    assert uf.rows_off_1e9(tab, o["table"]) == 0
    assert float(np.abs(s_all - o["s_all"]).max()) <= 1e-9 * max(1.0, float(np.abs(o["s_all"]).max()))
    assert np.array_equal(z, zF[:, :, -1]) and float(np.abs(cF[:, :, 0]).max()) == 0.0 and np.array_equal(zF[:, :d, 0], _np(x))
    assert not zF[:, d:, 0].any()
    # the truth's rows: the rule
    got = dict(table=tab, s_all=s_all, z=z[rows], zFull=zF[rows], ctrlFull=cF[rows])
    res = uf.compare_rollout(case, got)
    _check({k: v for k, v in res.items() if k != "s_all"}, family, case.id)
    _check({"s_all": res["s_all"]}, "stage inputs", case.id)
    # the means: the kernel's fixed-order sums against the longdouble mean of its own table; Jc against the truth where the truth is the whole batch
    means = np.array([float(c) for c in cs])
    for j in range(7):
        want = tab[:, j].astype(uf.LD).sum() / n
        assert abs(uf.LD(means[j]) - want) <= _mean_bound(tab[:, j], n), (j, means[j], want)
    assert float(sums[7]) == n
    # Jc is formed from those means: five terms, so at most five roundings of 2**-53 relative to the sum of their magnitudes
    terms = [uf.LD(means[0])] + [uf.LD(ALPH[a]) * uf.LD(means[j]) for a, j in ((0, 1), (3, 2), (4, 3), (5, 4))]
    assert abs(uf.LD(float(Jc)) - sum(terms)) <= 6 * U * float(sum(abs(v) for v in terms)), (float(Jc), float(sum(terms)))
    if len(rows) == n and t["keep"].all():
        _check({"Jc": uf.compare(float(Jc), t["Jc"], o["Jc"]), "means": uf.compare(means, t["means"], o["means"])}, family, case.id)


@pytest.mark.parametrize("case", uf.ROLLOUT_CASES, ids=lambda c: c.id)
def test_rollout_at_every_instantiation(case, knobs, capfd):
    _run_rollout(case, knobs, capfd, "rollout values")


@pytest.mark.parametrize("case", uf.PHYSICS_CASES, ids=lambda c: c.id)
def test_physics_at_two_and_four_samples_per_workgroup(case, knobs, capfd):
    _run_rollout(case, knobs, capfd, "rollout values")


def test_rollout_refuses_a_network_beyond_the_lds(knobs):
    case = uf.LDS_REFUSED
    net, prob = uf.make_net(case, DEV), uf.make_prob(case, DEV)
    with torch.no_grad(), pytest.raises(RuntimeError, match="NOCF_E_LDS"):
        na.OCflow(uf.starts(case).to(DEV), net, prob, list(case.tspan), case.nt, case.stepper, list(ALPH))


@pytest.mark.parametrize("n", uf.COST_SUM_N)
def test_cost_sums_are_the_longdouble_mean_of_the_kernels_own_table(n, knobs):
    case = uf.Case("midcross4", n, stepper="rk1", nt=1)
    net, prob = uf.make_net(case, DEV), uf.make_prob(case, DEV)
    x = uf.starts(case).to(DEV)
    _, _, tab, sums = _record(case, x, net, prob)
    tab, sums = _np(tab), _np(sums)
    assert sums[7] == n
    for j in range(7):
        want = tab[:, j].astype(uf.LD).sum() / n
        assert abs(uf.LD(sums[j]) / n - want) <= _mean_bound(tab[:, j], n), (j, sums[j] / n, want)


# ---- Phi and the problem calls
@pytest.mark.parametrize("case", uf.PHI_CASES, ids=lambda c: c.id)
def test_phi_value_and_gradient_at_every_instantiation(case, knobs, capfd):
    knobs(NOCF_DEBUG="1")
    net = uf.make_net(case, DEV)
    s = uf.phi_points(case).to(DEV)
    capfd.readouterr()
    with torch.no_grad():
        val, grad = net(s), net.getGrad(s)
    torch.cuda.synchronize()
    lines = _lines(capfd.readouterr().err, "f64 phi kernel")
    assert lines == [_want_line(case, PHI)] * 2, (lines, _want_line(case, PHI))
    rows, (g, v), (og, ov) = uf.phi_truth(case)
    val, grad = _np(val).reshape(-1), _np(grad)
    assert val.shape == (case.n,) and grad.shape == (case.n, case.d + 1)
    assert float(np.abs(val - ov).max()) <= 1e-11 * max(1.0, float(np.abs(ov).max()))
    assert float(np.abs(grad - og).max()) <= 1e-11 * max(1.0, float(np.abs(og).max()))
    _check({"value": uf.compare(val[rows], v, ov[rows]), "grad": uf.compare(grad[rows], g, og[rows])}, "phi", case.id)


@pytest.mark.parametrize("case", uf.PROB_CASES, ids=lambda c: c.id)
def test_problem_calls_against_the_truth(case):
    prob = uf.make_prob(case, DEV)
    x = uf.starts(case).to(DEV)
    p, t, o, keep = uf.prob_truth(case)
    pd = p.to(DEV)
    L, H, Q, W = prob.calcLHQW(x, pd)
    got = dict(L=L, H=H, Q=Q, W=W, gradpH=prob.calcGradpH(x, pd), ctrls=prob.calcCtrls(x, pd))
    res = {}
    for k, gk in got.items():
        gk = _np(gk).reshape(o[k].shape)
        assert float(np.abs(gk - o[k]).max()) <= 1e-11 * max(1.0, float(np.abs(o[k]).max())), k
        res[k] = uf.compare(gk[keep], t[k][keep], o[k][keep])
    _check(res, "prob", case.id)


# ---- the adjoint
def _run_adjoint(case, knobs, capfd):
    knobs(NOCF_DEBUG="1", **({"NOCF_F64_BWD_T": case.bwd_t} if case.bwd_t else {}))
    if not case.bwd_t:
        assert "NOCF_F64_BWD_T" not in os.environ
    net, prob = uf.make_net(case, DEV, train=True), uf.make_prob(case, DEV)
    xx = uf.starts(case).to(DEV).requires_grad_(True)
    capfd.readouterr()
    Jc, _ = na.OCflow(xx, net, prob, list(case.tspan), case.nt, case.stepper, list(ALPH))
    assert Jc.dtype == F64 and Jc.requires_grad
    Jc.backward()
    torch.cuda.synchronize()
    err = capfd.readouterr().err
    assert _lib.lib().nocf_last_rollout_kernel().decode() == "rollout_bwd_f64_kernel"
    assert _lines(err, "f64 adjoint kernel") == [_want_line(case, ADJOINT)], (err, _want_line(case, ADJOINT))
    assert _lines(err, "f64 kernel") == [_want_line(case, ROLLOUT)]
    grads = {k: _np(p.grad) for k, p in net.named_parameters()}
    grads["x0"] = _np(xx.grad)
    Jo, og = uf.oracle_grads(case)
    assert set(grads) == set(og)
    for k, g in grads.items():                                  # every entry: the existing double-against-double comparison
        assert not np.isnan(g).any()
        assert float(np.abs(g - og[k].reshape(g.shape)).max()) <= 1e-9 * float(np.abs(og[k]).max()) + 1e-12, k
    J, _ = uf.grad_truth(case)
    res = uf.compare_grads(case, grads)
    res["Jc"] = uf.compare(float(Jc), J, Jo)
    _check(res, "gradients", case.id)


@pytest.mark.parametrize("case", [c for c in uf.ADJOINT_CASES if not c.bwd_t], ids=lambda c: c.id)
def test_adjoint_at_its_natural_instantiations(case, knobs, capfd):
    _run_adjoint(case, knobs, capfd)


@pytest.mark.parametrize("case", [c for c in uf.ADJOINT_CASES if c.bwd_t], ids=lambda c: c.id)
def test_adjoint_at_forced_instantiations(case, knobs, capfd):
    _run_adjoint(case, knobs, capfd)


def test_zz_largest_figures_per_family():
    """err / tol / fp64 oracle error of the quantity closest to its bound, per family (what DESIGN.md section 4 quotes)"""
    for fam in ("rollout values", "stage inputs", "gradients", "phi", "prob"):
        if fam in _WORST:
            ratio, name, e, t, e64 = _WORST[fam]
            _FIGURES.append(f"[f64 sweep] {fam}: err {e:.3e} tol {t:.3e} fp64 oracle {e64:.3e} (err/tol {ratio:.3f}; {name})")
