"""Adversarial ensembles (neuraloc_amd/ensemble_minmax.py, trainOC.py --members_adv) without a GPU: every refusal -- each raised before the HIP
library is reached and, in the driver, before anything is written --, the C prototypes and exported symbols, the case lists' coverage.  What
the undisturbed ensembles and the driver refused before stays refused, with its message."""
import ctypes as C
import os
import re

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, ensemble_minmax as em

import util_ensemble as ue
import util_ensemble_mid as uem
import util_ensemble_minmax as uea
import util_lane as ul
import util_mono as um

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TS, NT = [0.0, 1.0], 2
SYMBOLS = ["nocf_rollout_disturbed_ensemble_f32", "nocf_rollout_record_disturbed_ensemble_f32",
           "nocf_rollout_disturbed_mid_ensemble_f32", "nocf_rollout_record_disturbed_mid_ensemble_f32",
           "nocf_rollout_bwd_small_ensemble_w_f32", "nocf_rollout_bwd_mid_ensemble_w_f32",
           "nocf_rollout_bwd_small_ensemble_states_f32", "nocf_rollout_bwd_mid_ensemble_states_f32",
           "nocf_disturbance_ascent_ensemble_f32"]


@pytest.fixture
def no_library(monkeypatch):
    """any attempt to load or use the HIP library fails the test"""
    def reached(*a, **k):
        raise AssertionError("the HIP library was reached")
    monkeypatch.setattr(_lib, "lib", reached)
    monkeypatch.setattr(_lib, "lib_for", reached)


def _valid(family):
    u, case = (ue, ue.TRAIN[0]) if family == "lane" else (uem, uem.TRAIN[1])
    ens = na.PhiEnsemble.from_members(u.member_nets(case, "cpu"), alph=u.member_rows())
    return u, case, ens, u.member_problem(case, 0, "cpu"), u.starts(case)


def _calls(W, family):
    """every public call that takes (x, ens, prob, ..., W) as a function of its first three arguments and the stepper"""
    kw = dict(family=family)
    return [
        lambda x, ens, prob, nt=NT, stepper="rk4", W=W, **k: na.ensemble_disturbed_rollout(x, ens, prob, TS, nt, W, stepper, **dict(kw, **k)),
        lambda x, ens, prob, nt=NT, stepper="rk4", W=W, **k: na.ensemble_disturbed_ocflow_train(x, ens, prob, TS, nt, W, stepper, **dict(kw, **k)),
        lambda x, ens, prob, nt=NT, stepper="rk4", W=W, **k: na.ensemble_minmax_ocflow_train(x, ens, prob, TS, nt, W, stepper, **dict(kw, **k)),
        lambda x, ens, prob, nt=NT, stepper="rk4", W=W, **k: na.ensemble_disturbance_gradient(x, ens, prob, nt, W, stepper=stepper, **dict(kw, **k)),
        lambda x, ens, prob, nt=NT, stepper="rk4", W=W, **k: na.ensemble_adversarial_step(
            x, ens, prob, TS, nt, W.clone().requires_grad_(True) if isinstance(W, torch.Tensor) and W.is_floating_point() else W, 0.1, 0.05,
            stepper=stepper, **dict(kw, **k)),
    ]


@pytest.mark.parametrize("family", ["lane", "mid"])
def test_refusals_before_the_library(no_library, family):
    u, case, ens, prob, x = _valid(family)
    E, n, d = x.shape
    W = torch.zeros(E, NT, n, d)
    for fn in _calls(W, family):
        # what the undisturbed calls refuse, with their messages: CPU tensors, float64 anywhere, shapes, nt, stepper, the family
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, ens, prob)
        with pytest.raises(RuntimeError, match="single precision only"):
            fn(x.double(), ens, prob)
        e64 = na.PhiEnsemble.from_members(u.member_nets(case, "cpu"), alph=u.member_rows()).double()
        with pytest.raises(RuntimeError, match="single precision only"):
            fn(x, e64, prob)
        with pytest.raises(ValueError, match="nex-by-d"):
            fn(torch.zeros(2, n, d), ens, prob)
        with pytest.raises(ValueError, match="nt must be"):
            fn(x, ens, prob, nt=0)
        with pytest.raises(ValueError, match="stepper"):
            fn(x, ens, prob, stepper="rk2")
        with pytest.raises(ValueError, match="family must be"):
            fn(x, ens, prob, family="duo")
        with pytest.raises(TypeError, match="PhiEnsemble"):
            fn(x, ens.member(0), prob)
    # W: a tensor, float32, [E, nt, nex, d] (or shared [nt, nex, d]), contiguous, on x's device
    bad_shapes = [torch.zeros(E, NT + 1, n, d), torch.zeros(E + 1, NT, n, d), torch.zeros(E, NT, n, d + 1), torch.zeros(NT, n + 1, d),
                  torch.zeros(NT, E, n, d), torch.zeros(n, d)]
    for bad in bad_shapes:
        for fn in _calls(bad, family):
            with pytest.raises(ValueError, match="E-by-nt-by-nex-by-d"):
                fn(x, ens, prob)
    for fn in _calls(W.double(), family):
        with pytest.raises(RuntimeError, match="W is float64"):
            fn(x, ens, prob)
    for fn in _calls(W.half(), family)[:4]:
        with pytest.raises(RuntimeError, match="fp32 only"):
            fn(x, ens, prob)
    for fn in _calls(torch.zeros(E, NT, d, n).transpose(2, 3), family):
        with pytest.raises(ValueError, match="contiguous"):
            fn(x, ens, prob)
    for fn in _calls(torch.zeros(E, NT, n, d, device="meta"), family)[:4]:
        with pytest.raises(ValueError, match="same device"):
            fn(x, ens, prob)
    for fn in _calls([[0.0]], family):
        with pytest.raises(TypeError, match="W must be a torch.Tensor"):
            fn(x, ens, prob)
    # a shared W takes no gradient: the members' dJ/dW are not summed (the rule for a shared x, which stays)
    with pytest.raises(NotImplementedError, match="W.requires_grad needs every member's own disturbance"):
        na.ensemble_minmax_ocflow_train(x, ens, prob, TS, NT, torch.zeros(NT, n, d, requires_grad=True), family=family)
    with pytest.raises(NotImplementedError, match="x.requires_grad needs every member's own starts"):
        na.ensemble_minmax_ocflow_train(x[0].clone().requires_grad_(), ens, prob, TS, NT, W, family=family)
    with pytest.raises(ValueError, match="objective must be"):
        na.ensemble_disturbance_gradient(x, ens, prob, NT, W, objective="L", family=family)
    with pytest.raises(ValueError, match="leaf tensor that requires a gradient"):
        na.ensemble_adversarial_step(x, ens, prob, TS, NT, W, 0.1, 0.05, family=family)


def test_budgets_and_step_lengths_are_checked_before_the_library(no_library):
    u, case, ens, prob, x = _valid("lane")
    E, n, d = x.shape
    W, g = torch.zeros(E, NT, n, d), torch.ones(E, NT, n, d)
    Wg = W.clone().requires_grad_(True)
    for bad in ([0.1, 0.2], [0.1] * 4, -0.1, [0.1, 0.2, -0.3], float("inf"), float("nan"), [0.1, float("nan"), 0.2], "x", [0.1, None, 0.2]):
        for call in (lambda: na.ensemble_ascend_disturbances(W, g, bad, 0.1), lambda: na.ensemble_ascend_disturbances(W, g, 0.1, bad),
                     lambda: na.ensemble_worst_case_disturbances(x, ens, prob, NT, bad),
                     lambda: na.ensemble_worst_case_disturbances(x, ens, prob, NT, 0.1, step_size=bad),
                     lambda: na.ensemble_adversarial_step(x, ens, prob, TS, NT, Wg, bad, 0.1),
                     lambda: na.ensemble_adversarial_step(x, ens, prob, TS, NT, Wg, 0.1, bad)):
            with pytest.raises(ValueError, match="eps must be|step_size must be|every eps|every step_size"):
                call()
    assert em._per_member("f", "eps", 0.25, 3) == [0.25] * 3 and em._per_member("f", "eps", (0, 0.5, 1), 3) == [0.0, 0.5, 1.0]
    assert em._per_member("f", "eps", torch.tensor([0.5, 0.25, 0.0]), 3) == [0.5, 0.25, 0.0]
    # the ascent step's own refusals
    with pytest.raises(ValueError, match="E-by-nt-by-nex-by-d"):
        na.ensemble_ascend_disturbances(W[0], g[0], 0.1, 0.1)
    with pytest.raises(ValueError, match="g must have W's shape"):
        na.ensemble_ascend_disturbances(W, g[:, :1], 0.1, 0.1)
    with pytest.raises(RuntimeError, match="float64"):
        na.ensemble_ascend_disturbances(W.double(), g.double(), 0.1, 0.1)
    with pytest.raises(TypeError, match="torch.Tensor"):
        na.ensemble_ascend_disturbances(W, None, 0.1, 0.1)
    with pytest.raises(ValueError, match="mask must have d entries"):
        na.ensemble_ascend_disturbances(W, g, 0.1, 0.1, mask=[1.0] * (d + 1))
    with pytest.raises(RuntimeError, match="no_grad"):
        na.ensemble_ascend_disturbances(Wg, g, 0.1, 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.ensemble_ascend_disturbances(W, g, 0.1, 0.1)
    # the search's own
    with pytest.raises(ValueError, match="steps must be"):
        na.ensemble_worst_case_disturbances(x, ens, prob, NT, 0.1, steps=-1)
    with pytest.raises(ValueError, match="objective must be"):
        na.ensemble_worst_case_disturbances(x, ens, prob, NT, 0.1, objective="L")
    with pytest.raises(ValueError, match="mask must have d entries"):
        na.ensemble_worst_case_disturbances(x, ens, prob, NT, 0.1, mask=[1.0] * (d + 1))
    with pytest.raises(ValueError, match="W0 must be E-by-nt-by-nex-by-d"):
        na.ensemble_worst_case_disturbances(x, ens, prob, NT, 0.1, W0=torch.zeros(NT, n, d))
    with pytest.raises(RuntimeError, match="W0 is float64"):
        na.ensemble_worst_case_disturbances(x, ens, prob, NT, 0.1, W0=W.double())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.ensemble_worst_case_disturbances(x, ens, prob, NT, [0.0, 0.1, 0.2], W0=W)


@pytest.mark.parametrize("fn", [na.ensemble_rollout, na.ensemble_ocflow_train])
def test_the_undisturbed_calls_still_refuse_a_disturbance(no_library, fn):
    for family in ("lane", "mid"):
        u, case, ens, prob, x = _valid(family)
        with pytest.raises(NotImplementedError, match="disturbed, noisy and min-max rollouts take one network"):
            fn(x, ens, prob, TS, NT, W=torch.zeros(NT, x.shape[1], x.shape[2]), family=family)


def test_a_library_without_the_symbols_is_named():
    class Old:                                                  # a library built before the entries existed; one that has some of them
        pass
    with pytest.raises(RuntimeError) as ex:
        em._entries(Old())
    assert all(name in str(ex.value) for name in SYMBOLS) and "rebuild" in str(ex.value)
    half = Old()
    for name in SYMBOLS[:4]:
        setattr(half, name, object())
    with pytest.raises(RuntimeError) as ex:
        em._entries(half)
    assert all(name in str(ex.value) for name in SYMBOLS[4:]) and not any(name + " " in str(ex.value) + " " for name in SYMBOLS[:4])
    with pytest.raises(RuntimeError, match="rebuild"):
        em._Disturbance(torch.zeros(1, 1, 1, 1), False).entries(half, "lane")
    assert list(em.SYMBOLS) == SYMBOLS


def test_prototypes_are_in_the_header_and_the_library_exports_them():
    flat = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "nocf.h")).read())

    def args_of(name):
        return re.search(r"int " + name + r"\(([^;]*)\);", flat).group(1)

    protos = {name: _lib.PROTOTYPES[name][1] for name in em.SYMBOLS}
    assert list(protos) == SYMBOLS
    # forwards: the undisturbed sibling's argument list with W and its member stride behind x_member_stride
    sibling = {SYMBOLS[0]: "nocf_rollout_ensemble_f32", SYMBOLS[1]: "nocf_rollout_record_ensemble_f32",
               SYMBOLS[2]: "nocf_rollout_mid_ensemble_f32", SYMBOLS[3]: "nocf_rollout_record_mid_ensemble_f32"}
    for name, sib in sibling.items():
        args = args_of(name)
        assert args == args_of(sib).replace("int64_t x_member_stride, ", "int64_t x_member_stride, const float* W, int64_t w_member_stride, "), name
        assert len(protos[name]) == len(args.split(",")), name
        at = args.split(", ").index("int64_t w_member_stride")
        assert protos[name][at - 1:at + 1] == [C.c_void_p, C.c_int64]
    # joint adjoints: the ensemble adjoint's with lamW behind lam0; state-only: the same without gpart (and gpart_rows)
    for name, sib in ((SYMBOLS[4], "nocf_rollout_bwd_small_ensemble_f32"), (SYMBOLS[5], "nocf_rollout_bwd_mid_ensemble_f32")):
        assert args_of(name) == args_of(sib).replace("float* lam0, ", "float* lam0, float* lamW, "), name
        assert len(protos[name]) == len(args_of(name).split(",")), name
    for name, sib in ((SYMBOLS[6], "nocf_rollout_bwd_small_ensemble_f32"), (SYMBOLS[7], "nocf_rollout_bwd_mid_ensemble_f32")):
        want = args_of(sib).replace("float* gpart, int64_t gpart_rows, ", "").replace("float* gpart, ", "").replace("float* lam0, ", "float* lam0, float* lamW, ")
        assert args_of(name) == want, name
        assert len(protos[name]) == len(want.split(",")), name
    assert args_of(SYMBOLS[8]) == ("float* W, const float* g, const float* mask, int64_t n, int32_t members, int32_t nt, int32_t d, "
                                   "const float* steps, const float* epss, void* stream")
    assert len(protos[SYMBOLS[8]]) == 10
    for name in SYMBOLS + ["rollout_lane_kernel<ens,disturbed>", "rollout_mono_kernel<ens,disturbed>", "rollout_lane_bwd_kernel<ens,joint>",
                           "rollout_mono_bwd_kernel<ens,joint>"]:
        assert name in flat, name
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
    f = em._entries(L)
    assert list(f) == SYMBOLS
    for name in SYMBOLS:
        assert f[name].restype is C.c_int and len(f[name].argtypes) == len(protos[name]), name
    assert L.nocf_version() == 113                              # callers probe for the symbols; the number did not move


def test_null_and_misshapen_arguments_are_refused_by_the_abi():
    """NOCF_E_NULL / NOCF_E_SHAPE come back before any device is touched (every pointer here is a null or a host dummy nobody reads)"""
    L = _lib.lib()
    f = em._entries(L)
    one = C.c_void_p(16)
    # a NULL W is refused in front of everything else, on all four forwards
    phi, prob = _lib.NocfPhi(), _lib.NocfProb()
    for name, outs in ((SYMBOLS[0], [one] * 6), (SYMBOLS[1], [one] * 4), (SYMBOLS[2], [one] * 6), (SYMBOLS[3], [one] * 5 + [None])):
        assert f[name](C.byref(phi), C.byref(prob), one, 5, 3, 0, None, 0, 0.0, 1.0, 2, 4, one, *outs, one, 1 << 20, None) == -1, name
    asc = f[SYMBOLS[8]]
    assert asc(None, one, None, 5, 3, 2, 4, one, one, None) == -1 and asc(one, None, None, 5, 3, 2, 4, one, one, None) == -1
    assert asc(one, one, None, 5, 3, 2, 4, None, one, None) == -1 and asc(one, one, None, 5, 3, 2, 4, one, None, None) == -1
    for bad in ((0, 3, 2, 4), (5, 0, 2, 4), (5, 3, 0, 4), (5, 3, 2, 0), (2 ** 30, 4, 2, 4)):
        assert asc(one, one, None, *bad, one, one, None) == -2, bad


def _driver():
    import importlib.util
    spec = importlib.util.spec_from_file_location("trainOC_under_test", os.path.join(REPO, "trainOC.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("argv, text", [
    (["--members_adv", "0.1,0.2"], "--members_adv needs --members"),
    (["--members", "2", "--members_adv", "0.1"], "one budget per member"),
    (["--members", "2", "--members_adv", "0.1,0.2,0.3"], "one budget per member"),
    (["--members", "2", "--members_adv", "0.1,-0.2"], "finite number >= 0"),
    (["--members", "2", "--members_adv", "0.1,inf"], "finite number >= 0"),
    (["--members", "2", "--members_adv", "0.1,nan"], "finite number >= 0"),
    (["--members", "2", "--members_adv", "0.1,x"], "comma-separated list of numbers"),
    (["--members", "2", "--members_adv", "0.1,0.2", "--members_sigma", "0.1,0.2"], "--members_adv excludes --members_sigma and --members_risk"),
    (["--members", "2", "--members_adv", "0.1,0.2", "--members_sigma", "0.1,0.2", "--members_risk", "mean"],
     "--members_adv excludes --members_sigma and --members_risk"),
    (["--members", "2", "--members_adv", "0.1,0.2", "--noise", "0.1"], "--members_adv excludes --noise and --adv"),
    (["--members", "2", "--members_adv", "0.1,0.2", "--adv", "0.1"], "--members_adv excludes --noise and --adv"),
    (["--members", "2", "--members_adv", "0.1,0.2", "--adv_steps", "0"], "--adv_steps K must be >= 1"),
    (["--members", "2", "--adv", "0.1"], "--members excludes --noise and --adv"),            # the pinned refusal: this flag is the way in
    (["--members", "2", "--members_adv", "0.1,0.2", "--prec", "double"], "single precision"),
    (["--members", "2", "--members_adv", "0.1,0.2", "--m", "64"], "outside the small-network kernels"),
    (["--members", "2", "--members_adv", "0.1,0.2", "--members_family", "mid", "--data", "singlequad", "--m", "32"], "outside the one-CU kernels"),
])
def test_driver_refusals_write_nothing(no_library, tmp_path, monkeypatch, argv, text):
    drv = _driver()
    save = tmp_path / "out"
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as ex:
        drv.main(argv + ["--niters", "1", "--save", str(save)] + ([] if "--data" in argv else ["--data", "softcorridor"]))
    assert text in str(ex.value)
    assert not save.exists()


def test_driver_accepts_the_budgets(no_library):
    drv = _driver()
    args = drv.parse_args(["--members", "3", "--members_adv", "0, 0.05,1e-1", "--adv_steps", "2"])
    assert drv.members_adv_budgets(args, None, None) == [0.0, 0.05, 0.1] and len(drv.members_refusals(args, 1)) == 3
    assert drv.members_adv_budgets(drv.parse_args(["--members", "3"]), None, None) is None
    assert "--members_adv" in drv.__doc__ and "3.17" in drv.__doc__


def test_cases_cover_every_instantiation_once():
    lane_f, mid_f = [c for c in uea.FORWARD if c.family == "lane"], [c for c in uea.FORWARD if c.family == "mid"]
    lane_t, mid_t = [c for c in uea.TRAIN if c.family == "lane"], [c for c in uea.TRAIN if c.family == "mid"]
    assert [c.case for c in lane_f] == ue.FORWARD and [c.case for c in mid_f] == uem.FORWARD        # the existing lists, unchanged
    assert [c.case for c in lane_t] == ue.TRAIN and [c.case for c in mid_t] == uem.TRAIN
    assert [c.base.shape for c in lane_f] == ul.INSTANTIATIONS == [c.base.shape for c in lane_t]    # every (MP, DP) pair, once
    assert [c.base.shape for c in mid_f] == um.FORWARD_SHAPES and [c.base.shape for c in mid_t] == um.ADJOINT_SHAPES
    # each forward case runs as evaluation and as recording forward, each adjoint case as joint and as state-only adjoint
    assert 2 * len(lane_f) == 12 and 2 * len(mid_f) == 14 and len(lane_t) == 6 and len(mid_t) == 6
    assert all(c.base.n == 5 and c.base.nt == 2 for c in lane_f + lane_t) and all(c.base.n == 17 and c.base.nt == 2 for c in mid_f + mid_t)
    assert {c.base.stepper for c in lane_f} == {"rk4", "rk1"} == {c.base.stepper for c in mid_t}
    assert uea.E == 3 and len(uea.GJ) == 3 and uea.EPS[0] == 0.0 and all(v > 0 for v in uea.EPS[1:])
    for cases in (lane_f, mid_f, lane_t, mid_t):
        assert [c.masked for c in cases[:2]] in ([False, True], [True, False]) and {c.masked for c in cases} == {True, False}
    assert all(c.own_x for c in uea.TRAIN) and {c.own_x for c in uea.FORWARD} == {True, False}
    assert len(ids := [c.id for c in uea.FORWARD + uea.TRAIN]) == len(set(ids))
    # the disturbances: a slice per member from its own seed, the stated magnitude, masked coordinates exactly zero
    for ac in (lane_f[0], lane_f[1], mid_t[0], mid_t[1]):
        b = ac.base
        W = uea.disturbance(ac)
        assert tuple(W.shape) == (3, b.nt, b.n, b.d) and W.dtype == torch.float32 and W.is_contiguous()
        assert not torch.equal(W[0], W[1]) and not torch.equal(W[1], W[2]) and 0.5 * uea.SCALE < float(W[W != 0].std()) < 2 * uea.SCALE
        assert torch.equal(W, uea.disturbance(ac)) and not torch.equal(W, uea.disturbance(ac, salt=1))
        off = [i for i in range(b.d) if i % 3 == 1]
        assert bool((W[..., off] == 0).all()) == ac.masked
    # the cases the GPU tests pick by property exist
    assert uea.first(uea.TRAIN, "lane", masked=True) and uea.first(uea.TRAIN, "mid", masked=False)
    assert uea.first(uea.FORWARD, "lane", own_x=True) and uea.first(uea.FORWARD, "mid", own_x=False)
