"""CPU: risk-sensitive training.  neuraloc_amd.risk_weights against torch autograd of the risks' definitions (tests/util_risk.py); the weighted
reference at w = 1/n against util_disturb_train's mean; the comparator rejects the mean's gradients under non-uniform weights; the risk cases'
ranking condition; every refusal of weighted_ocflow_train / risk_ocflow_train and of trainOC.py's --risk flags; the three weighted entries'
export, prototypes and refusals -- none of which touches a device."""
import ctypes as C
import os

import pytest
import torch

import __graft_entry__ as entry
import neuraloc_amd as na
from neuraloc_amd import _lib, train
import util_disturb as ud
import util_disturb_train as ut
import util_mono as um
import util_risk as ur

ALPH = [100.0, 50.0, 30.0, 0.5, 0.25, 0.125]


def _table(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 7, generator=g, dtype=torch.float64) * torch.tensor([5.0, 0.1, 2.0, 4.0, 8.0, 1.0, 1.0], dtype=torch.float64)


# (risk, level, n, paths): CVaR at a fractional k (R = 7, level 0.8: k = 1.4) and at integer k (R = 5: k = 1; R = 35: k = 7)
WEIGHT_CASES = [("cvar", 0.8, 35, 7), ("cvar", 0.8, 35, 5), ("cvar", 0.8, 35, None), ("cvar", 0.37, 35, None), ("cvar", 0.0, 35, 7),
                ("entropic", 0.05, 35, 7), ("entropic", 0.3, 35, None), ("mean", 0.0, 35, 7), ("mean", 0.0, 35, None)]


@pytest.mark.parametrize("risk, level, n, paths", WEIGHT_CASES)
@pytest.mark.parametrize("mix", [0.0, 0.3, 1.0])
def test_risk_weights_are_the_gradient_of_the_value(risk, level, n, paths, mix):
    tab = _table(n)
    w, v = na.risk_weights(tab, ALPH, risk, level, paths=paths, mix=mix)
    J = ur.row_costs(tab, ALPH)
    g, vref = ur.autograd_weights(J, risk, level, paths, mix)
    assert w.shape == (n,) and w.dtype == torch.float64
    assert float((w - g).abs().max()) <= 1e-12
    assert abs(float(v) - float(vref)) <= 1e-12 * abs(float(vref))
    assert abs(float(w.sum()) - 1.0) <= 1e-12
    if mix == 0.0 or risk == "mean" or (risk == "cvar" and level == 0.0):
        assert float((w - 1.0 / n).abs().max()) <= 1e-15                   # mix = 0 and level = 0 are the mean: 1 / n on every row
        assert abs(float(v) - float(J.mean())) <= 1e-12 * abs(float(J.mean()))
    elif risk == "cvar":
        R = n if paths is None else paths
        k, kf, frac = ur.tail_counts(level, R)
        u = (w * (n // R) - (1.0 - mix) / R) / mix                           # the risk's own share of the weights
        srt = torch.sort(u.reshape(-1, R), dim=1, descending=True).values
        assert float((srt[:, :kf] - 1.0 / k).abs().max()) <= 1e-12
        if kf < R:
            assert float((srt[:, kf] - frac / k).abs().max()) <= 1e-12 and float(srt[:, kf + 1:].abs().max() if kf + 1 < R else 0.0) <= 1e-12
        # the weighted rows are the largest costs of their group
        Jg, ug = J.reshape(-1, R), u.reshape(-1, R)
        for g_ in range(Jg.shape[0]):
            inside = ug[g_] > 1e-12
            assert float(Jg[g_][inside].min()) >= float(Jg[g_][~inside].max()) if bool((~inside).any()) else True


def test_risk_weights_argument_checks():
    tab = _table(12)
    rw = na.risk_weights
    for bad in (dict(risk="var", level=0.5), dict(risk="cvar", level=1.0), dict(risk="cvar", level=-0.1), dict(risk="entropic", level=0.0),
                dict(risk="entropic", level=float("inf")), dict(risk="cvar", level=0.5, paths=5), dict(risk="cvar", level=0.5, paths=0),
                dict(risk="cvar", level=0.5, mix=1.5), dict(risk="cvar", level=0.5, mix=-0.1)):
        with pytest.raises(ValueError):
            rw(tab, ALPH, **bad)
    with pytest.raises(ValueError):
        rw(tab[:, :6], ALPH, "mean", 0.0)
    with pytest.raises(ValueError):
        rw(tab, ALPH[:5], "mean", 0.0)
    # float32 tables stay float32; the weights need no gradient
    w, v = rw(tab.float(), ALPH, "cvar", 0.5, paths=4)
    assert w.dtype == torch.float32 and not w.requires_grad and not v.requires_grad


def _as_got(r):
    return {k: (torch.zeros(1) if v is None else v) for k, v in r.items()}


@pytest.mark.parametrize("fc", [ud.CASES[0], ud.CASES[8]], ids=ud.case_id)
def test_uniform_weights_reproduce_the_mean_and_nonuniform_ones_are_told_apart(fc):
    family, case = fc
    n = case.n
    uni = torch.full((n,), 1.0 / n, dtype=torch.float64)
    mean64, mean32 = ut.case_grads(case, torch.float64), ut.case_grads(case, torch.float32)
    w64 = ur.weighted_grads(case, torch.float64, weights=uni)
    assert abs(w64["Jw"] - mean64["Jc"]) <= 1e-12 * abs(mean64["Jc"])
    ref = ut.with_x(mean64)
    for k, v in ref.items():
        if v is None:
            assert w64["grads"][k] is None
        else:
            assert float((w64["grads"][k] - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max())), k
    # the fp32 restatement passes the rule against its own fp64 reference under the case's non-uniform weights ...
    r64, r32 = ur.weighted_grads(case, torch.float64)["grads"], ur.weighted_grads(case, torch.float32)["grads"]
    res = ur.compare_grads(_as_got(r32), r64, r32)
    assert not ur.failures(res), (case.id, ur.failures(res))
    # ... and the gradient of the MEAN does not: a weighted entry that ignored its weights would be caught
    res = ur.compare_grads(_as_got(ut.with_x(mean32)), r64, r32)
    fails = ur.failures(res)
    assert "x" in fails and len(fails) >= len(res) - 2, (case.id, sorted(fails))
    # the weights themselves: both signs, an exact zero, a range of about 100
    w = ur.case_weights(case)
    nz = w[w != 0].abs()
    assert int((w == 0).sum()) == 1 and bool((w < 0).any()) and bool((w > 0).any()) and 50.0 <= float(nz.max() / nz.min()) <= 200.0


@pytest.mark.parametrize("fc", ur.FAMILY_CASES[:1], ids=ud.case_id)
@pytest.mark.parametrize("risk, level", ur.RISK_LEVELS)
def test_risk_cases_rank_alike_in_fp32_and_fp64(fc, risk, level):
    """building the case asserts the ranking condition; here also that risk_weights on the fp64 costs IS the autograd reference, and that the
    gradient of the value differs from the mean's (the GPU comparison has something to find)"""
    family, case = fc
    rc = ur.risk_case(case, risk, level)
    tab = ud.case_restate(case, rc["x"].double(), rc["W"], torch.float64)["table"]
    w, v = na.risk_weights(tab, case.alph, risk, rc["level"], paths=ur.RISK_PATHS)
    assert float((w - rc["r64"]["weights"]).abs().max()) <= 1e-12
    assert abs(float(v) - float(rc["r64"]["value"])) <= 1e-12 * abs(float(v))
    assert float((w - 1.0 / w.numel()).abs().max()) >= 0.2 / w.numel()
    res = ur.compare_grads(_as_got(rc["r32"]["grads"]), rc["r64"]["grads"], rc["r32"]["grads"])
    assert not ur.failures(res)


def test_python_refusals_need_no_device():
    case = ud.CASES[0][1]
    net = um.make_net(case, "cpu")
    prob = um.make_problem(case)
    n, nt, d = 4, case.nt, case.d
    ts = list(case.tspan)
    x = um.candidates(case, n)
    W = torch.zeros(nt, n, d)
    w = torch.full((n,), 0.25)
    net64 = um.make_net(case, "cpu").double()
    ens = na.PhiEnsemble.from_members([um.make_net(case, "cpu"), um.make_net(case, "cpu")])
    for p in net.parameters():
        p.grad = torch.ones_like(p)
    wt, rk = na.weighted_ocflow_train, na.risk_ocflow_train

    def refused(exc, match, f, *a, **kw):
        with pytest.raises(exc, match=match):
            f(*a, **kw)
        assert all(bool((p.grad == 1).all()) for p in net.parameters())

    for f, lead in ((wt, (w,)), (rk, ("cvar", 0.5))):
        # float64 anywhere
        refused(RuntimeError, "single precision only", f, x.double(), net, prob, ts, nt, *lead, W=W)
        refused(RuntimeError, "single precision only", f, x, net, prob, ts, nt, *lead, W=W.double())
        refused(RuntimeError, "single precision only", f, x, net64, prob, ts, nt, *lead, W=W)
        refused(RuntimeError, "single precision only", f, x, net, prob, ts, nt, *lead, sigma=torch.ones(d, dtype=torch.float64), seed=1)
        refused(NotImplementedError, "float64", f, x.double(), net, prob, ts, nt, *lead, sigma=0.1, seed=1)
        # sharded batches and ensembles
        refused(NotImplementedError, "n_total / group", f, x, net, prob, ts, nt, *lead, W=W, n_total=8)
        refused(NotImplementedError, "n_total / group", f, x, net, prob, ts, nt, *lead, W=W, group=True)
        refused(NotImplementedError, "ensembles are not supported", f, x, ens, prob, ts, nt, *lead, W=W)
        # one disturbance, and only one
        refused(ValueError, "exactly one of W and sigma", f, x, net, prob, ts, nt, *lead)
        refused(ValueError, "exactly one of W and sigma", f, x, net, prob, ts, nt, *lead, W=W, sigma=0.1, seed=1)
        refused(ValueError, "needs a seed", f, x, net, prob, ts, nt, *lead, sigma=0.1)
        refused(ValueError, "seed", f, x, net, prob, ts, nt, *lead, sigma=0.1, seed=-1)
        refused(ValueError, "seed belongs to sigma", f, x, net, prob, ts, nt, *lead, W=W, seed=1)
        refused(NotImplementedError, "dJ/dW together with weights", f, x, net, prob, ts, nt, *lead, W=W.clone().requires_grad_(True))
        # the checks of the disturbed and noisy calls
        for bad in (W[:-1], W[:, :-1], W[:, :, :-1], W[0]):
            refused(ValueError, "nt-by-nex-by-d", f, x, net, prob, ts, nt, *lead, W=bad)
        refused(ValueError, "nex-by-d", f, x[0], net, prob, ts, nt, *lead, W=W)
        refused(ValueError, "nt must be", f, x, net, prob, ts, 0, *lead, W=W)
        refused(ValueError, "stepper", f, x, net, prob, ts, nt, *lead, W=W, stepper="rk2")
        refused(ValueError, "alph", f, x, net, prob, ts, nt, *lead, W=W, alph=[1.0] * 5)
        refused(ValueError, "mask", f, x, net, prob, ts, nt, *lead, sigma=0.1, seed=1, mask=torch.ones(d + 1))
        refused(ValueError, "row_offset", f, x, net, prob, ts, nt, *lead, sigma=0.1, seed=1, row_offset=-1)
        # CPU tensors: the last refusal, behind every argument check
        refused(RuntimeError, "no CPU fallback", f, x, net, prob, ts, nt, *lead, W=W)
        refused(RuntimeError, "no CPU fallback", f, x, net, prob, ts, nt, *lead, sigma=0.0, seed=1)
    # the weights
    for bad in (w.double(), w[:-1], w.reshape(2, 2), w.clone().requires_grad_(True), w.to(torch.float16)):
        refused(NotImplementedError, "not supported", wt, x, net, prob, ts, nt, bad, W=W)
    refused(TypeError, "weights", wt, x, net, prob, ts, nt, [0.25] * n, W=W)
    refused(TypeError, "weights", wt, x, net, prob, ts, nt, None, W=W)
    # the risk's own arguments
    refused(ValueError, "risk must be", rk, x, net, prob, ts, nt, "var", 0.5, W=W)
    refused(ValueError, "level", rk, x, net, prob, ts, nt, "cvar", 1.0, W=W)
    refused(ValueError, "level", rk, x, net, prob, ts, nt, "entropic", 0.0, W=W)
    refused(ValueError, "paths", rk, x, net, prob, ts, nt, "cvar", 0.5, W=W, paths=3)
    refused(ValueError, "mix", rk, x, net, prob, ts, nt, "cvar", 0.5, W=W, mix=2.0)
    # the float64 refusals of the disturbed and noisy calls stay
    with pytest.raises(RuntimeError, match="single precision only"):
        na.disturbed_ocflow_train(x.double(), net, prob, ts, nt, W)
    with pytest.raises(RuntimeError, match="single precision only"):
        na.noisy_ocflow_train(x.double(), net, prob, ts, nt, 0.1, 1)


@pytest.mark.parametrize("flags, match", [
    (["--risk", "cvar", "--risk_level", "0.8"], "--risk needs --noise"),
    (["--risk", "cvar", "--risk_level", "0.8", "--noise", "0.1"], "--noise_rng counter"),
    (["--risk", "cvar", "--risk_level", "0.8", "--noise", "0.1", "--noise_rng", "torch"], "--noise_rng counter"),
    (["--risk", "cvar", "--risk_level", "0.8", "--noise", "0.1", "--noise_rng", "counter", "--members", "2"], "excludes --members"),
    (["--risk", "cvar", "--risk_level", "0.8", "--adv", "0.5"], "--risk"),
    (["--risk", "cvar", "--risk_level", "0.8", "--prec", "double"], "single precision"),
    (["--risk", "cvar", "--risk_level", "0.8", "--noise", "0.1", "--noise_rng", "counter", "--prec", "double"], "single precision"),
    (["--risk", "cvar", "--risk_level", "1.0", "--noise", "0.1", "--noise_rng", "counter"], "--risk_level"),
    (["--risk", "entropic", "--risk_level", "0", "--noise", "0.1", "--noise_rng", "counter"], "--risk_level"),
    (["--risk", "cvar", "--noise", "0.1", "--noise_rng", "counter"], "--risk_level"),
    (["--risk", "cvar", "--risk_level", "0.8", "--risk_paths", "0", "--noise", "0.1", "--noise_rng", "counter"], "--risk_paths"),
    (["--risk", "cvar", "--risk_level", "0.8", "--risk_mix", "1.5", "--noise", "0.1", "--noise_rng", "counter"], "--risk_mix"),
    (["--risk_level", "0.8"], "needs --risk"),
])
def test_trainOC_risk_refusals_come_before_anything_runs(tmp_path, capsys, flags, match):
    import trainOC
    save = os.path.join(str(tmp_path), "run")
    with pytest.raises(SystemExit, match=match):
        trainOC.main(["--data", "softcorridor", "--niters", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save, *flags])
    assert not os.path.exists(save) and capsys.readouterr().out == ""


def test_trainOC_risk_refuses_more_than_one_rank(tmp_path, capsys, monkeypatch):
    import trainOC
    monkeypatch.setenv("WORLD_SIZE", "2")
    save = os.path.join(str(tmp_path), "run")
    with pytest.raises(SystemExit, match="one rank"):
        trainOC.main(["--data", "softcorridor", "--niters", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save,
                      "--risk", "cvar", "--risk_level", "0.8", "--noise", "0.1", "--noise_rng", "counter"])
    assert not os.path.exists(save) and capsys.readouterr().out == ""


def test_trainOC_risk_flag_defaults():
    import trainOC
    a = trainOC.parse_args([])
    assert a.risk is None and a.risk_level is None and a.risk_paths >= 1 and a.risk_mix == 1.0
    with pytest.raises(SystemExit):
        trainOC.parse_args(["--risk", "var"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    entry.build()
    return _lib.lib()


def _norm(s):
    return " ".join(s.split())


def test_symbols_are_exported_and_declared(L):
    f = train._weighted_entries(L)
    assert f is not None
    small, mid, act = f
    for new, old in ((small, L.nocf_rollout_bwd_small_f32), (mid, L.nocf_rollout_bwd_mid_f32), (act, L.nocf_rollout_bwd_act_f32)):
        # the existing entry's argument list with a pointer where `double inv_n` stands (argument 7)
        assert new.restype is C.c_int and len(new.argtypes) == len(old.argtypes)
        assert old.argtypes[7] is C.c_double and new.argtypes[7] is C.c_void_p
        assert list(new.argtypes[:7]) == list(old.argtypes[:7]) and list(new.argtypes[8:]) == list(old.argtypes[8:])
    with open(entry.REPO + "/include/nocf.h") as fh:
        text = _norm(fh.read())
    head = ("(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1, "
            "const float* alph, const float* wrow, const float* s_all, const float* z_final, const float* hs, ")
    old_head = head.replace("const float* wrow", "double inv_n")
    tails = {"small": "float* gpart, float* lam0, void* stream);",
             "mid": "const float* act_rec, float* gpart, int64_t gpart_rows, float* lam0, void* workspace, size_t workspace_bytes, void* stream);",
             "act": ("float* Y, float* Ob, float* V, float* Ab, float* Qb, float* U0, float* Wb, float* Gb, float* Sx, float* PHIb, float* lam0, "
                     "const float* act_rec, void* workspace, size_t workspace_bytes, void* stream);")}
    for fam, tail in tails.items():
        assert f"int nocf_rollout_bwd_{fam}_rw_f32" + head + tail in text, fam
        assert f"int nocf_rollout_bwd_{fam}_f32" + old_head + tail in text, fam        # the existing prototypes stay
    assert L.nocf_version() == 113                                                  # ... and so does the version: callers probe for the symbols


def _phi(d, m, nTh=2, r=5):
    phi = _lib.NocfPhi()
    phi.d, phi.m, phi.nTh, phi.r = d, m, nTh, r
    for k in ("K0", "b0", "K", "b", "w", "A", "cw", "cb_dev"):
        setattr(phi, k, 0x1000)
    return phi


def _calls(L, fam, phi, prob, n=4, nt=2, stepper=4, alph=1, s_all=1, z=1, hs=1, out=1, wrow=1, ws=1, wsb=1 << 30):
    """(existing entry's answer, weighted entry's answer) of family fam (0 lane, 1 one-CU, 2 per-tile) on the same arguments.  Every caller
    passes arguments that family refuses: the pointers are fakes and are never dereferenced"""
    p = C.c_void_p(0x1000)
    nz = lambda f: p if f else None                                  # noqa: E731
    a = (C.c_float * 6)(1, 1, 1, 1, 1, 1) if alph else None
    small, mid, act = train._weighted_entries(L)
    h0 = (C.byref(phi) if phi is not None else None, C.byref(prob) if prob is not None else None, n, nt, stepper, 1.0, a)
    h1 = (nz(s_all), nz(z), nz(hs))
    if fam == 0:
        return L.nocf_rollout_bwd_small_f32(*h0, 1.0, *h1, nz(out), p, None), small(*h0, nz(wrow), *h1, nz(out), p, None)
    if fam == 1:
        return (L.nocf_rollout_bwd_mid_f32(*h0, 1.0, *h1, None, nz(out), 1 << 20, p, nz(ws), wsb, None),
                mid(*h0, nz(wrow), *h1, None, nz(out), 1 << 20, p, nz(ws), wsb, None))
    return (L.nocf_rollout_bwd_act_f32(*h0, 1.0, *h1, *([nz(out)] * 10), p, None, nz(ws), wsb, None),
            act(*h0, nz(wrow), *h1, *([nz(out)] * 10), p, None, nz(ws), wsb, None))


def test_abi_refusals_are_the_existing_entries(L):
    """every refusal of a weighted entry is the answer the existing entry gives to the same arguments and returns before a launch; wrow == NULL
    is NOCF_E_NULL.  One shape per family: lane (m = 16), one-CU (m = 64), per-tile (m = 129)"""
    prob, keep = na.Cross2D(torch.zeros(4))._c_struct("cpu")
    prob6, keep6 = na.Cross2D(torch.zeros(6))._c_struct("cpu")
    for fam, m in enumerate((16, 64, 129)):
        phi = _phi(4, m)
        for kw, want in ((dict(alph=0), -1), (dict(s_all=0), -1), (dict(z=0), -1), (dict(hs=0), -1), (dict(out=0), -1),
                         (dict(n=0), -2), (dict(nt=0), -2), (dict(stepper=3), -5)):
            old, new = _calls(L, fam, phi, prob, **kw)
            assert old == new == want, (m, kw, old, new)
        assert _calls(L, fam, None, prob) == (-1, -1)
        assert _calls(L, fam, _phi(4, m), prob6) == (-3, -3)               # NOCF_E_PROB: the problem's agents do not match d
        if fam:                                                            # (the lane kernel needs no workspace)
            assert _calls(L, fam, phi, prob, ws=0) == (-1, -1)
            assert _calls(L, fam, phi, prob, wsb=16) == (-4, -4)           # NOCF_E_WORKSPACE
        # wrow == NULL: NOCF_E_NULL from the weighted entry alone, also together with another refusal's arguments
        _, new = _calls(L, fam, phi, prob, wrow=0, n=0)
        assert new == -1
    # a shape that is not the family's own: NOCF_E_SHAPE hands it on, as the existing entries do
    for fam in (0, 1):
        assert _calls(L, fam, _phi(4, 129), prob) == (-2, -2)
