"""Risk-sensitive ensembles (neuraloc_amd/ensemble_risk.py, trainOC.py --members_risk) without a GPU: ensemble_risk_weights against risk_weights
per member, every refusal -- raised with CPU tensors in front of the device check, with every .grad untouched and, in the driver, before
anything is written --, the two C entries' prototypes and argument codes, and the case lists' geometry."""
import ctypes as C
import os
import re

import pytest
import torch

import __graft_entry__ as entry
import neuraloc_amd as na
from neuraloc_amd import _lib, ensemble, ensemble_risk

import util_ensemble as ue
import util_ensemble_mid as uem
import util_ensemble_noise as uen
import util_ensemble_risk as uer
import util_lane as ul
import util_mono as um

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS, NT = [0.0, 1.0], 2
SYMBOLS = ["nocf_rollout_bwd_small_ensemble_rw_f32", "nocf_rollout_bwd_mid_ensemble_rw_f32"]
SIBLINGS = ["nocf_rollout_bwd_small_ensemble_f32", "nocf_rollout_bwd_mid_ensemble_f32"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the weights
# ---------------------------------------------------------------------------------------------------------------------------------
def _table(E, n, seed=3):
    g = torch.Generator().manual_seed(seed)
    tab = torch.rand(E, n, 7, generator=g) * torch.tensor([5.0, 0.1, 1.0, 1.0, 1.0, 3.0, 2.0])
    tab[0, 4:6] = tab[0, 1:3]                                   # (a tie inside a group of member 0)
    return tab


@pytest.mark.parametrize("paths", [None, 3])
def test_weights_are_risk_weights_per_member(paths):
    E, n = 3, 12
    tab = _table(E, n)
    rows = ue.ALPH_ROWS
    for risk, level, mix in (("cvar", 0.5, 1.0),                                          # one value for all members
                             ("entropic", 0.7, 0.25),
                             ("mean", 0.0, 1.0),
                             ("cvar", [0.0, 0.5, 0.8], 1.0),                               # a level sweep
                             (["cvar", "entropic", "mean"], [0.5, 1.5, 0.0], [1.0, 0.5, 0.0]),
                             ("cvar", 0.25, [0.0, 0.5, 1.0])):
        w, value, rho = na.ensemble_risk_weights(tab, rows, risk, level, paths, mix)
        G = 1 if paths is None else n // paths
        assert tuple(w.shape) == (E, n) and tuple(value.shape) == (E,) and tuple(rho.shape) == (E, G)
        assert w.dtype == value.dtype == rho.dtype == torch.float32
        for e in range(E):
            pick = lambda v: v[e] if isinstance(v, list) else v                           # noqa: E731
            keep = []
            w1, v1 = na.risk_weights(tab[e], rows[e], pick(risk), pick(level), paths, pick(mix), _rho=keep)
            assert torch.equal(w[e], w1) and torch.equal(value[e], v1) and torch.equal(rho[e], keep[0]), (risk, level, mix, e)
    # one row of multipliers for all members; the members differ by their tables alone
    w, value, rho = na.ensemble_risk_weights(tab, rows[0], "cvar", 0.5, paths)
    assert torch.equal(w[2], na.risk_weights(tab[2], rows[0], "cvar", 0.5, paths)[0]) and not torch.equal(w[0], w[1])


def test_weights_argument_checks():
    tab = _table(3, 12)
    rows = ue.ALPH_ROWS
    for bad in (tab[0], tab[:, :, :6], torch.zeros(0, 12, 7), [[1.0] * 7]):
        with pytest.raises(ValueError, match="E-by-n-by-7"):
            na.ensemble_risk_weights(bad, rows, "cvar", 0.5)
    with pytest.raises(ValueError, match="alph must be"):
        na.ensemble_risk_weights(tab, rows[:2], "cvar", 0.5)
    for kw, text in ((dict(risk=["cvar", "cvar"], level=0.5), "risk must be one value"), (dict(risk="cvar", level=[0.5] * 4), "level must be one value"),
                     (dict(risk="cvar", level=0.5, mix=[1.0]), "mix must be one value")):
        with pytest.raises(ValueError, match=text):
            na.ensemble_risk_weights(tab, rows, **kw)
    with pytest.raises(ValueError, match="risk must be one of"):
        na.ensemble_risk_weights(tab, rows, ["cvar", "var", "mean"], 0.5)
    with pytest.raises(ValueError, match="level"):
        na.ensemble_risk_weights(tab, rows, "cvar", [0.5, 1.0, 0.0])
    with pytest.raises(ValueError, match="level"):
        na.ensemble_risk_weights(tab, rows, ["cvar", "entropic", "mean"], [0.5, 0.0, 0.0])
    with pytest.raises(ValueError, match="whole number of groups"):
        na.ensemble_risk_weights(tab, rows, "cvar", 0.5, paths=5)
    with pytest.raises(ValueError, match="mix must lie"):
        na.ensemble_risk_weights(tab, rows, "cvar", 0.5, mix=[1.0, 0.5, 1.5])


# ---------------------------------------------------------------------------------------------------------------------------------
# the refusals of the two training calls
# ---------------------------------------------------------------------------------------------------------------------------------
class _Complete:
    """a library that exports the two weighted ensemble entries and nothing else: any other use of the HIP library fails the test"""
    nocf_rollout_bwd_small_ensemble_rw_f32 = None
    nocf_rollout_bwd_mid_ensemble_rw_f32 = None

    def __init__(self):
        class Fn:
            argtypes = None
        self.nocf_rollout_bwd_small_ensemble_rw_f32, self.nocf_rollout_bwd_mid_ensemble_rw_f32 = Fn(), Fn()


@pytest.fixture
def symbols_only(monkeypatch):
    def reached(*a, **k):
        raise AssertionError("the HIP library was reached")
    stub = _Complete()
    monkeypatch.setattr(_lib, "lib", lambda: stub)
    monkeypatch.setattr(_lib, "lib_for", reached)


def _valid(family):
    u, case = (ue, ue.TRAIN[0]) if family == "lane" else (uem, uem.TRAIN[1])
    ens = na.PhiEnsemble.from_members(u.member_nets(case, "cpu"), alph=u.member_rows())
    x = u.starts(case, n=6)
    return u, case, ens, u.member_problem(case, 0, "cpu"), x


@pytest.mark.parametrize("family", ["lane", "mid"])
def test_python_refusals_need_no_device(symbols_only, monkeypatch, family):
    u, case, ens, prob, x = _valid(family)
    E, n, d = x.shape
    w = torch.full((E, n), 1.0 / n)
    for p in ens.parameters():
        p.grad = torch.ones_like(p)
    wt, rk = na.ensemble_weighted_ocflow_train, na.ensemble_risk_ocflow_train
    nz = dict(sigma=[[0.1], [0.0], [0.2]], seed=5)

    def refused(exc, match, f, *a, **kw):
        with pytest.raises(exc, match=match):
            f(*a, **{**dict(family=family), **kw})
        assert all(bool((p.grad == 1).all()) for p in ens.parameters())

    for f, lead in ((wt, (w,)), (rk, ("cvar", 0.5))):
        # float64 anywhere
        refused(RuntimeError, "single precision only", f, x.double(), ens, prob, TS, NT, *lead, **nz)
        e64 = na.PhiEnsemble.from_members(u.member_nets(case, "cpu"), alph=u.member_rows()).double()
        with pytest.raises(RuntimeError, match="single precision only"):
            f(x, e64, prob, TS, NT, *lead, family=family, **nz)
        p64 = u.member_problem(case, 0, "cpu")
        p64.xtarget = p64.xtarget.double()
        refused(RuntimeError, "single precision only", f, x, ens, p64, TS, NT, *lead, **nz)
        refused(RuntimeError, "sigma is float64", f, x, ens, prob, TS, NT, *lead, sigma=torch.ones(E, 1, dtype=torch.float64), seed=5)
        # a disturbance tensor, sharded batches
        refused(NotImplementedError, "disturbance tensor W", f, x, ens, prob, TS, NT, *lead, W=torch.zeros(NT, n, d), **nz)
        refused(NotImplementedError, "n_total / group", f, x, ens, prob, TS, NT, *lead, n_total=8, **nz)
        refused(NotImplementedError, "n_total / group", f, x, ens, prob, TS, NT, *lead, group=True, **nz)
        # shapes outside the family: ensemble._refuse's rules with train=True
        refused(ValueError, "family must be", f, x, ens, prob, TS, NT, *lead, family="duo", **nz)
        refused(TypeError, "PhiEnsemble", f, x[0], ens.member(0), prob, TS, NT, *lead, **nz)
        refused(ValueError, "nex-by-d", f, torch.zeros(2, n, d), ens, prob, TS, NT, *lead, **nz)
        refused(ValueError, "nt must be", f, x, ens, prob, TS, 0, *lead, **nz)
        refused(ValueError, "stepper", f, x, ens, prob, TS, NT, *lead, stepper="rk2", **nz)
        refused(NotImplementedError, "requires_grad", f, x[0].clone().requires_grad_(), ens, prob, TS, NT,
                *((w,) if f is wt else lead), **nz)
        # the noise: sequences whose length is not E, and the checks of the noisy ensemble
        refused(ValueError, r"\[E, 1\] or \[E, d\]", f, x, ens, prob, TS, NT, *lead, sigma=[[0.1]] * 2, seed=5)
        refused(ValueError, "seed must be", f, x, ens, prob, TS, NT, *lead, sigma=0.1, seed=[1, 2])
        refused(ValueError, "seed must be", f, x, ens, prob, TS, NT, *lead, sigma=0.1, seed=-1)
        refused(ValueError, "mask must have d entries", f, x, ens, prob, TS, NT, *lead, mask=[1.0] * (d + 1), **nz)
        refused(ValueError, "row_offset", f, x, ens, prob, TS, NT, *lead, row_offset=-1, **nz)
        # CPU tensors: the last refusal, behind every argument check
        refused(RuntimeError, "no CPU fallback", f, x, ens, prob, TS, NT, *lead, **nz)
        refused(RuntimeError, "no CPU fallback", f, x[0].contiguous(), ens, prob, TS, NT, *((w,) if f is wt else lead), **nz)
    # the weights
    for bad in (w[:2], w[:, :-1], w.reshape(-1), w.clone().requires_grad_(True), w.to(torch.float16)):
        refused(NotImplementedError, "not supported", wt, x, ens, prob, TS, NT, bad, **nz)
    refused(RuntimeError, "weights is float64", wt, x, ens, prob, TS, NT, w.double(), **nz)
    refused(TypeError, "weights", wt, x, ens, prob, TS, NT, [[1.0 / n] * n] * E, **nz)
    refused(TypeError, "weights", wt, x, ens, prob, TS, NT, None, **nz)
    # the risk's own arguments, per member
    refused(ValueError, "risk must be one of", rk, x, ens, prob, TS, NT, "var", 0.5, **nz)
    refused(ValueError, "risk must be one of", rk, x, ens, prob, TS, NT, ["cvar", "var", "mean"], 0.5, **nz)
    refused(ValueError, "risk must be one value", rk, x, ens, prob, TS, NT, ["cvar", "cvar"], 0.5, **nz)
    refused(ValueError, "level must be one value", rk, x, ens, prob, TS, NT, "cvar", [0.0, 0.5, 0.8, 0.95], **nz)
    refused(ValueError, "mix must be one value", rk, x, ens, prob, TS, NT, "cvar", 0.5, mix=[1.0, 0.5], **nz)
    refused(ValueError, "level", rk, x, ens, prob, TS, NT, "cvar", [0.5, 1.0, 0.0], **nz)
    refused(ValueError, "level", rk, x, ens, prob, TS, NT, ["cvar", "entropic", "mean"], [0.5, 0.0, 0.0], **nz)
    refused(ValueError, "whole number of groups", rk, x, ens, prob, TS, NT, "cvar", 0.5, paths=4, **nz)
    refused(ValueError, "paths must be", rk, x, ens, prob, TS, NT, "cvar", 0.5, paths=0, **nz)
    refused(ValueError, "mix must lie", rk, x, ens, prob, TS, NT, "cvar", 0.5, mix=[1.0, 0.5, 2.0], **nz)
    with pytest.raises(TypeError):
        rk(x, ens, prob, TS, NT, "cvar", 0.5, family=family)                           # sigma and seed are required
    # a library without the two symbols, named in front of the device check
    class Old:
        pass
    monkeypatch.setattr(_lib, "lib", lambda: Old())
    for f, lead in ((wt, (w,)), (rk, ("cvar", 0.5))):
        with pytest.raises(RuntimeError) as ex:
            f(x, ens, prob, TS, NT, *lead, family=family, **nz)
        assert all(name in str(ex.value) for name in SYMBOLS) and "rebuild" in str(ex.value)
        assert all(bool((p.grad == 1).all()) for p in ens.parameters())


def test_shapes_outside_the_family_are_refused(symbols_only):
    w3 = torch.full((3, 5), 0.2)
    sw = ue.FORWARD[1]                                          # the lane adjoint takes Cross2D agents
    e2 = na.PhiEnsemble.from_members(ue.member_nets(sw, "cpu"), alph=ue.member_rows())
    with pytest.raises(ValueError, match="Cross2D"):
        na.ensemble_weighted_ocflow_train(ue.starts(sw), e2, ue.member_problem(sw, 0, "cpu"), TS, NT, w3, sigma=0.1, seed=5)
    quad = na.Quadcopter(torch.zeros(12), obstacle=None, alph_Q=1.0, alph_W=1.0, r=0.5)
    with pytest.raises(ValueError, match="32 < m"):
        na.ensemble_risk_ocflow_train(torch.zeros(2, 3, 12), na.PhiEnsemble(2, 2, 32, 12), quad, TS, NT, "cvar", 0.5, sigma=0.1, seed=5,
                                      family="mid")
    with pytest.raises(ValueError, match="small-network lane kernels only"):
        na.ensemble_risk_ocflow_train(torch.zeros(2, 3, 12), na.PhiEnsemble(2, 2, 64, 12), quad, TS, NT, "cvar", 0.5, sigma=0.1, seed=5)


def test_the_single_network_calls_still_refuse_an_ensemble():
    u, case, ens, prob, x = _valid("lane")
    with pytest.raises(NotImplementedError, match="ensembles are not supported; the weighted adjoint takes one network"):
        na.weighted_ocflow_train(x[0], ens, prob, TS, NT, torch.full((6,), 1 / 6), sigma=0.1, seed=1)
    with pytest.raises(NotImplementedError, match="ensembles are not supported; the weighted adjoint takes one network"):
        na.risk_ocflow_train(x[0], ens, prob, TS, NT, "cvar", 0.5, sigma=0.1, seed=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------------------
_M = ["--members", "2", "--members_sigma", "0.05,0.1"]


@pytest.mark.parametrize("flags, match", [
    (["--members_risk", "cvar", "--members_risk_level", "0.5"], "--members_risk needs --members E --members_sigma"),
    (["--members", "2", "--members_risk", "cvar", "--members_risk_level", "0.5"], "--members_risk needs --members E --members_sigma"),
    (["--members_risk_level", "0.5"], "--members_risk_level needs --members_risk"),
    (_M + ["--members_risk_level", "0.5"], "--members_risk_level needs --members_risk"),
    (_M + ["--members_risk", "cvar"], "needs --members_risk_level"),
    (_M + ["--members_risk", "cvar", "--members_risk_level", "0.5,0.8,0.9"], "one level for all members or one per member"),
    (_M + ["--members_risk", "cvar", "--members_risk_level", "0.5,x"], "comma-separated list of numbers"),
    (_M + ["--members_risk", "cvar", "--members_risk_level", "0.5,1.0"], "0 <= --members_risk_level < 1"),
    (_M + ["--members_risk", "cvar", "--members_risk_level", "-0.1"], "0 <= --members_risk_level < 1"),
    (_M + ["--members_risk", "entropic", "--members_risk_level", "2.0,0"], "--members_risk_level \\(theta\\) > 0"),
    (_M + ["--members_risk", "entropic", "--members_risk_level", "inf"], "--members_risk_level \\(theta\\) > 0"),
    (_M + ["--members_risk", "cvar", "--members_risk_level", "0.5", "--members_risk_paths", "0"], "--members_risk_paths"),
    (_M + ["--members_risk", "cvar", "--members_risk_level", "0.5", "--members_risk_mix", "1.5"], "--members_risk_mix"),
    (_M + ["--members_risk", "cvar", "--members_risk_level", "0.5", "--prec", "double"], "single precision"),
    (_M + ["--members_risk", "cvar", "--members_risk_level", "0.5", "--noise", "0.1"], "--members excludes --noise"),
    # --risk with --members stays refused, with its message: --members_risk is the way in
    (_M + ["--risk", "cvar", "--risk_level", "0.8", "--noise", "0.1", "--noise_rng", "counter"], "--risk excludes --members: the weighted adjoint takes one network"),
    (_M + ["--members_risk", "cvar", "--members_risk_level", "0.5", "--risk", "cvar", "--risk_level", "0.8", "--noise", "0.1", "--noise_rng",
           "counter"], "--risk excludes --members"),
])
def test_driver_refusals_come_before_anything_runs(symbols_only, tmp_path, capsys, monkeypatch, flags, match):
    import trainOC
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    save = os.path.join(str(tmp_path), "run")
    with pytest.raises(SystemExit, match=match):
        trainOC.main(["--data", "softcorridor", "--niters", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save, *flags])
    assert not os.path.exists(save) and capsys.readouterr().out == ""


def test_driver_flags():
    import trainOC
    a = trainOC.parse_args([])
    assert a.members_risk is None and a.members_risk_level is None and a.members_risk_paths == 8 and a.members_risk_mix == 1.0
    assert trainOC.members_risk_spec(a, None) is None
    with pytest.raises(SystemExit):
        trainOC.parse_args(["--members_risk", "var"])
    a = trainOC.parse_args(["--members", "4", "--members_sigma", "0.1,0.1,0.1,0.1", "--members_risk", "cvar", "--members_risk_level",
                            "0, 0.5,0.8,0.95"])
    assert trainOC.members_risk_spec(a, trainOC.members_sigma_levels(a)) == ("cvar", [0.0, 0.5, 0.8, 0.95], 8, 1.0)
    a = trainOC.parse_args(_M + ["--members_risk", "entropic", "--members_risk_level", "2.5", "--members_risk_paths", "3", "--members_risk_mix", "0.5"])
    assert trainOC.members_risk_spec(a, trainOC.members_sigma_levels(a)) == ("entropic", [2.5, 2.5], 3, 0.5)
    a = trainOC.parse_args(_M + ["--members_risk", "mean"])
    assert trainOC.members_risk_spec(a, trainOC.members_sigma_levels(a)) == ("mean", [0.0, 0.0], 8, 1.0)
    assert "--members_risk" in trainOC.__doc__ and "3.16" in trainOC.__doc__


# ---------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    entry.build()
    return _lib.lib()


def test_symbols_are_exported_and_declared(L):
    assert list(ensemble_risk.SYMBOLS) == SYMBOLS
    flat = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "nocf.h")).read())
    for family, name, sib in zip(("lane", "mid"), SYMBOLS, SIBLINGS):
        assert hasattr(L, name), name
        f = ensemble.weighted_entry(L, family)
        old = _lib.PROTOTYPES[sib][1]
        # the sibling's argument list with a pointer where `double inv_n` stands (argument 8)
        assert f.restype is C.c_int and len(f.argtypes) == len(old)
        assert old[8] is C.c_double and f.argtypes[8] is C.c_void_p
        assert list(f.argtypes[:8]) == list(old[:8]) and list(f.argtypes[9:]) == list(old[9:])
        args = re.search(r"int " + name + r"\(([^;]*)\);", flat).group(1)
        sargs = re.search(r"int " + sib + r"\(([^;]*)\);", flat).group(1)
        assert args == sargs.replace("double inv_n", "const float* wrow"), name
        assert len(args.split(",")) == len(f.argtypes)
    assert L.nocf_version() == 113                              # callers probe for the symbols; the number did not move


def test_a_library_without_the_symbols_is_named():
    class Old:
        pass
    for family in ("lane", "mid"):
        with pytest.raises(RuntimeError) as ex:
            ensemble.weighted_entry(Old(), family)
        assert all(name in str(ex.value) for name in SYMBOLS) and "rebuild" in str(ex.value)
        half = Old()
        setattr(half, SYMBOLS[0], object())
        with pytest.raises(RuntimeError) as ex:
            ensemble.weighted_entry(half, family)
        assert SYMBOLS[1] in str(ex.value) and SYMBOLS[0] not in str(ex.value)


def _phi(d, m, nTh=2, r=5):
    phi = _lib.NocfPhi()
    phi.d, phi.m, phi.nTh, phi.r = d, m, nTh, r
    for k in ("K0", "b0", "K", "b", "w", "A", "cw", "cb_dev"):
        setattr(phi, k, 0x1000)
    return phi


def _calls(L, fam, phi, prob, n=5, members=3, nt=2, stepper=4, alph=1, s_all=1, z=1, hs=1, out=1, wrow=1, ws=1, wsb=1 << 30, rows=None,
           sibling=True):
    """(unweighted ensemble entry's answer, weighted entry's answer) of family fam (0 lane, 1 one-CU) on the same arguments.  Every caller
    passes arguments the entries it calls refuse: the pointers are fakes and are never dereferenced.  sibling=False: the weighted entry alone"""
    p = C.c_void_p(0x1000)
    nz = lambda f: p if f else None                                  # noqa: E731
    h0 = (C.byref(phi) if phi is not None else None, C.byref(prob) if prob is not None else None, n, members, nt, stepper, 1.0, nz(alph))
    h1 = (nz(s_all), nz(z), nz(hs))
    if fam == 0:
        old = ensemble._entries(L)[2]
        new = ensemble.weighted_entry(L, "lane")
        return old(*h0, 0.2, *h1, nz(out), p, None) if sibling else None, new(*h0, nz(wrow), *h1, nz(out), p, None)
    old = ensemble._entries_mid(L)[2]
    new = ensemble.weighted_entry(L, "mid")
    if rows is None:
        rows = int(L.nocf_mid_grad_rows(phi.d, phi.m, phi.nTh, phi.r, 2, n)) if phi is not None else 1
    return (old(*h0, 0.2, *h1, None, nz(out), rows, p, nz(ws), wsb, None) if sibling else None,
            new(*h0, nz(wrow), *h1, None, nz(out), rows, p, nz(ws), wsb, None))


def test_abi_refusals_are_the_unweighted_ensemble_entries(L):
    """every refusal of a weighted ensemble entry is the answer its unweighted sibling gives to the same arguments, and wrow == NULL is
    NOCF_E_NULL: all of them return before a device is touched (nothing here has one).  One shape per family: lane (m = 16), one-CU (m = 64)"""
    prob, keep = na.Cross2D(torch.zeros(4))._c_struct("cpu")
    prob6, keep6 = na.Cross2D(torch.zeros(6))._c_struct("cpu")
    for fam, m in enumerate((16, 64)):
        phi = _phi(4, m)
        for kw, want in ((dict(alph=0), -1), (dict(s_all=0), -1), (dict(z=0), -1), (dict(hs=0), -1), (dict(out=0), -1),
                         (dict(n=0), -2), (dict(nt=0), -2), (dict(members=0), -2), (dict(n=2 ** 30, members=4), -2), (dict(stepper=3), -5)):
            old, new = _calls(L, fam, phi, prob, **kw)
            assert old == new == want, (m, kw, old, new)
        assert _calls(L, fam, None, prob) == (-1, -1)
        nocb = _phi(4, m)
        nocb.cb_dev = None
        assert _calls(L, fam, nocb, prob) == (-1, -1)                      # (c.bias [E] is read on the device)
        assert _calls(L, fam, _phi(4, m), prob6) == (-3, -3)               # NOCF_E_PROB: the problem's agents do not match d
        if fam:
            assert _calls(L, fam, phi, prob, ws=0) == (-1, -1)
            assert _calls(L, fam, phi, prob, wsb=16) == (-4, -4)           # NOCF_E_WORKSPACE
            assert _calls(L, fam, phi, prob, rows=7) == (-4, -4)           # gpart_rows must be the query's
        # wrow == NULL: NOCF_E_NULL from the weighted entry alone (its sibling, which would launch on these fakes, is not called)
        assert _calls(L, fam, phi, prob, wrow=0, sibling=False) == (None, -1)
    # a shape that is not the family's own
    for fam in (0, 1):
        assert _calls(L, fam, _phi(4, 129), prob) == (-2, -2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the case lists
# ---------------------------------------------------------------------------------------------------------------------------------
def test_cases_meet_their_conditions():
    lane, mid = [c for c in uer.GIVEN if c.family == "lane"], [c for c in uer.GIVEN if c.family == "mid"]
    assert uer.GIVEN == uen.TRAIN and len(lane) == len(mid) == 6 and uer.E == 3
    assert [c.base.shape for c in lane] == ul.INSTANTIATIONS and [c.base.shape for c in mid] == um.ADJOINT_SHAPES
    assert all(c.own_x for c in uer.GIVEN) and any(0.0 in [row[0] for row in c.sigma] for c in lane) and any(0.0 in [row[0] for row in c.sigma] for c in mid)
    # given weights.  lane: 15 rows in 4 workgroups, two of them hold rows of two members, the last one a tail wave
    assert all(c.base.n == 5 and c.base.nt == 2 for c in lane)
    groups, tail = uer.lane_workgroups(uer.E, 5)
    assert len(groups) == 4 and [len(g) for g in groups] == [1, 2, 2, 1] and tail == 1
    # one-CU: two tiles per member, the second with one valid row
    assert all(c.base.n == 17 and c.base.nt == 2 for c in mid) and uer.mid_tiles(17) == (2, 1)
    # the weights: both signs, one exact zero, a range of about 100, of the order of 1 / n, different per member
    for nc in (lane[0], mid[0]):
        w = uer.weights(nc)
        n = nc.base.n
        assert tuple(w.shape) == (uer.E, n) and w.dtype == torch.float32 and w.is_contiguous()
        for e in range(uer.E):
            assert bool((w[e] > 0).any()) and bool((w[e] < 0).any()) and int((w[e] == 0).sum()) == 1 and float(w[e, n // 2]) == 0.0
            nzw = w[e][w[e] != 0].abs()
            assert 99.0 <= float(nzw.max() / nzw.min()) <= 101.0 and abs(float(nzw.max()) * n - 1.0) < 1e-6
        assert not torch.equal(w[0], w[1]) and not torch.equal(w[1], w[2])
        assert torch.equal(w, uer.weights(nc))
    # risk.  paths divide the rows; lane: 18 rows, a workgroup holds rows of two members and tail waves exist
    assert uer.PATHS == 3 and all(n % uer.PATHS == 0 for n in uer.RISK_N.values())
    groups, tail = uer.lane_workgroups(uer.E, uer.RISK_N["lane"])
    assert uer.RISK_N["lane"] == 6 and any(len(g) == 2 for g in groups) and tail >= 1
    # one-CU: the group of rows 15 .. 17 lies across the tile boundary, the tail tile has 2 valid rows
    n = uer.RISK_N["mid"]
    assert n == 18 and uer.mid_tiles(n) == (2, 2)
    assert any(g * uer.PATHS < 16 < (g + 1) * uer.PATHS for g in range(n // uer.PATHS))
    # the members' measures: a fractional boundary row, the entropic risk, the mean blended with itself at level 0
    assert [s[0] for s in uer.RISK_SPECS] == ["cvar", "entropic", "cvar"]
    k = (1.0 - uer.RISK_SPECS[0][1]) * uer.PATHS
    assert k == 1.5 and uer.RISK_SPECS[1][1] is None and uer.RISK_SPECS[2][1:] == (0.0, 0.5)
    # the undisturbed member is one whose risk is CVaR (its paths tie: the stable sort decides, the same way in both legs); the entropic
    # member is disturbed (its theta is set from the spread of its costs)
    assert [row[0] > 0 for row in uer.RISK_SIGMA] == [False, True, True]
    # one case per family at the smallest and at the largest instantiation
    assert [c.base.shape for c in uer.RISK if c.family == "lane"] == [(16, 8), (32, 32)]
    assert [c.base.shape for c in uer.RISK if c.family == "mid"] == [(4, 1), (8, 2)]
    x = uer.risk_starts(uer.RISK[0])
    assert tuple(x.shape) == (uer.E, 6, uer.RISK[0].base.d) and torch.equal(x[:, 0], x[:, 2]) and not torch.equal(x[:, 2], x[:, 3])
    # the capped grid
    b = uer.CAPPED.base
    assert uer.CAPPED.family == "mid" and b.n == 16385 and b.nt == 1 and b.stepper == "rk1" and uer.CAPPED_E == 2 and um.cdiv(b.n, 16) > 1024
    # theta: 2 / the mean spread
    tab = torch.zeros(6, 7)
    tab[:, 0] = torch.tensor([1.0, 2.0, 3.0, 5.0, 5.0, 9.0])
    assert uer.theta_of(tab, [1.0] * 6) == 2.0 / 3.0
