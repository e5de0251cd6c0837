"""Ensembles under in-kernel noise (neuraloc_amd/ensemble_noise.py, trainOC.py --members_sigma) without a GPU: every refusal -- each raised
before the HIP library is reached and, in the driver, before anything is written --, the C prototypes and exported symbols, the sigma / seed
normalisation and the case lists' coverage.  What the undisturbed ensembles refuse stays refused, with its message."""
import ctypes as C
import os
import re

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, ensemble_noise
from neuraloc_amd.noise import noise_scale

import util_ensemble as ue
import util_ensemble_mid as uem
import util_ensemble_noise as uen
import util_lane as ul
import util_mono as um

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNS = [na.ensemble_noisy_rollout, na.ensemble_noisy_ocflow_train]
TS, NT = [0.0, 1.0], 2
SYMBOLS = ["nocf_rollout_noisy_ensemble_f32", "nocf_rollout_record_noisy_ensemble_f32",
           "nocf_rollout_noisy_mid_ensemble_f32", "nocf_rollout_record_noisy_mid_ensemble_f32"]


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


@pytest.mark.parametrize("family", ["lane", "mid"])
@pytest.mark.parametrize("fn", FNS)
def test_refusals_before_the_library(no_library, fn, family):
    u, case, ens, prob, x = _valid(family)
    d = case.base.d
    kw = dict(family=family)
    ok = (0.1, 5)
    # what the undisturbed calls refuse, with their messages: CPU tensors, float64 anywhere, shapes, nt, stepper, the family
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(x, ens, prob, TS, NT, *ok, **kw)
    with pytest.raises(RuntimeError, match="single precision only"):
        fn(x.double(), ens, prob, TS, NT, *ok, **kw)
    e64 = na.PhiEnsemble.from_members(u.member_nets(case, "cpu"), alph=u.member_rows()).double()
    with pytest.raises(RuntimeError, match="single precision only"):
        fn(x, e64, prob, TS, NT, *ok, **kw)
    p64 = u.member_problem(case, 0, "cpu")
    p64.xtarget = p64.xtarget.double()
    with pytest.raises(RuntimeError, match="single precision only"):
        fn(x, ens, p64, TS, NT, *ok, **kw)
    with pytest.raises(ValueError, match="nex-by-d"):
        fn(torch.zeros(2, 5, d), ens, prob, TS, NT, *ok, **kw)
    with pytest.raises(ValueError, match="nt must be"):
        fn(x, ens, prob, TS, 0, *ok, **kw)
    with pytest.raises(ValueError, match="stepper"):
        fn(x, ens, prob, TS, NT, *ok, "rk2", **kw)
    with pytest.raises(ValueError, match="family must be"):
        fn(x, ens, prob, TS, NT, *ok, family="duo")
    with pytest.raises(TypeError, match="PhiEnsemble"):
        fn(x, ens.member(0), prob, TS, NT, *ok, **kw)
    # sigma: [E] against [d] is ambiguous; 2-D must be [E, 1] or [E, d]
    for bad in ([0.1] * (d + 1), [0.1] * 3 if d != 3 else [0.1] * 2, torch.zeros(d - 1)):
        with pytest.raises(ValueError, match="1-D sequence must have d"):
            fn(x, ens, prob, TS, NT, bad, 5, **kw)
    for bad in ([[0.1]] * 2, [[0.1, 0.2]] * 3, torch.zeros(3, d + 1), torch.zeros(3, 1, 1)):
        with pytest.raises(ValueError, match=r"\[E, 1\] or \[E, d\]"):
            fn(x, ens, prob, TS, NT, bad, 5, **kw)
    # seed: a Python int in [0, 2**64) or E of them
    for bad in (-1, 2 ** 64, 1.0, True, None, [1, 2], [1, 2, 3, 4], [1, 2, -1], [1, 2, 2 ** 64], [1, 2, 3.0]):
        with pytest.raises(ValueError, match="seed must be"):
            fn(x, ens, prob, TS, NT, 0.1, bad, **kw)
    # mask, row_offset: as in noisy_rollout
    with pytest.raises(ValueError, match="mask must have d entries"):
        fn(x, ens, prob, TS, NT, *ok, mask=[1.0] * (d + 1), **kw)
    for bad in (-1, 1.0, 2 ** 62):
        with pytest.raises(ValueError, match="row_offset"):
            fn(x, ens, prob, TS, NT, *ok, row_offset=bad, **kw)


def test_training_and_study_refusals_before_the_library(no_library):
    u, case, ens, prob, x = _valid("lane")
    with pytest.raises(NotImplementedError, match="requires_grad"):
        na.ensemble_noisy_ocflow_train(x[0].clone().requires_grad_(), ens, prob, TS, NT, 0.1, 5)
    sw = ue.FORWARD[1]                                          # the lane adjoint takes Cross2D agents
    e2 = na.PhiEnsemble.from_members(ue.member_nets(sw, "cpu"), alph=ue.member_rows())
    with pytest.raises(ValueError, match="Cross2D"):
        na.ensemble_noisy_ocflow_train(ue.starts(sw), e2, ue.member_problem(sw, 0, "cpu"), TS, NT, 0.1, 5)
    quad = na.Quadcopter(torch.zeros(12), obstacle=None, alph_Q=1.0, alph_W=1.0, r=0.5)
    with pytest.raises(ValueError, match="32 < m"):
        na.ensemble_noisy_ocflow_train(torch.zeros(2, 3, 12), na.PhiEnsemble(2, 2, 32, 12), quad, TS, NT, 0.1, 5, family="mid")
    with pytest.raises(ValueError, match="point-agent"):
        na.ensemble_noisy_rollout(torch.zeros(2, 3, 12), na.PhiEnsemble(2, 2, 9, 12), quad, TS, NT, 0.1, 5)
    # the study: its own two, then the rollout's
    with pytest.raises(ValueError, match="paths must be"):
        na.ensemble_noise_study(x, ens, prob, NT, 0.1, 0, 5)
    with pytest.raises(ValueError, match="holds no whole start"):
        na.ensemble_noise_study(x, ens, prob, NT, 0.1, 4, 5, max_rows=3)
    with pytest.raises(ValueError, match="1-D sequence must have d"):
        na.ensemble_noise_study(x, ens, prob, NT, [0.1] * 3, 4, 5)
    with pytest.raises(ValueError, match="seed must be"):
        na.ensemble_noise_study(x, ens, prob, NT, 0.1, 4, [1, 2])
    with pytest.raises(RuntimeError, match="single precision only"):
        na.ensemble_noise_study(x.double(), ens, prob, NT, 0.1, 4, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.ensemble_noise_study(x, ens, prob, NT, 0.1, 4, 5)


@pytest.mark.parametrize("fn", [na.ensemble_rollout, na.ensemble_ocflow_train])
def test_the_undisturbed_calls_still_refuse_a_disturbance(no_library, fn):
    for family in ("lane", "mid"):
        u, case, ens, prob, x = _valid(family)
        with pytest.raises(NotImplementedError, match="disturbed, noisy and min-max rollouts take one network"):
            fn(x, ens, prob, TS, NT, W=torch.zeros(NT, x.shape[1], x.shape[2]), family=family)


def test_a_library_without_the_symbols_is_named():
    class Old:                                                  # a library built before the entries existed; one that has half of them
        pass
    for family, names in (("lane", SYMBOLS[:2]), ("mid", SYMBOLS[2:])):
        with pytest.raises(RuntimeError) as ex:
            ensemble_noise._entries(Old(), family)
        assert all(name in str(ex.value) for name in names) and "rebuild" in str(ex.value)
        half = Old()
        setattr(half, names[0], object())
        with pytest.raises(RuntimeError) as ex:
            ensemble_noise._entries(half, family)
        assert names[1] in str(ex.value) and names[0] not in str(ex.value)
    assert list(ensemble_noise.SYMBOLS) == SYMBOLS


def test_prototypes_are_in_the_header_and_the_library_exports_them():
    flat = re.sub(r"\s+", " ", open(os.path.join(REPO, "include", "nocf.h")).read())
    sibling = {"nocf_rollout_noisy_ensemble_f32": "nocf_rollout_ensemble_f32", "nocf_rollout_record_noisy_ensemble_f32": "nocf_rollout_record_ensemble_f32",
               "nocf_rollout_noisy_mid_ensemble_f32": "nocf_rollout_mid_ensemble_f32",
               "nocf_rollout_record_noisy_mid_ensemble_f32": "nocf_rollout_record_mid_ensemble_f32"}
    assert list(sibling) == SYMBOLS
    protos = {name: _lib.PROTOTYPES[name][1] for name in ensemble_noise.SYMBOLS}
    assert list(protos) == SYMBOLS
    extra = "const float* scale, const uint64_t* seeds, int64_t row0, "
    for name, sib in sibling.items():
        args = re.search(r"int " + name + r"\(([^;]*)\);", flat).group(1)
        sargs = re.search(r"int " + sib + r"\(([^;]*)\);", flat).group(1)
        # the sibling's argument list with the three noise arguments behind x_member_stride
        assert args == sargs.replace("int64_t x_member_stride, ", "int64_t x_member_stride, " + extra), name
        assert len(protos[name]) == len(args.split(",")), name
        at = args.split(", ").index("int64_t row0")
        assert protos[name][at - 2:at + 1] == [C.c_void_p, C.c_void_p, C.c_int64]
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
    for family in ("lane", "mid"):
        f_eval, f_rec, names = ensemble_noise._entries(L, family)
        assert list(names) == (SYMBOLS[:2] if family == "lane" else SYMBOLS[2:])
        assert f_eval.restype is C.c_int and len(f_eval.argtypes) == len(protos[names[0]]) and len(f_rec.argtypes) == len(protos[names[1]])
    assert L.nocf_version() == 113                              # callers probe for the symbols; the number did not move


def test_null_tables_and_a_negative_row_are_refused_by_the_abi():
    """NOCF_E_NULL / NOCF_E_SHAPE come back before any device is touched (every pointer here is a null or a host dummy nobody reads)"""
    L = _lib.lib()
    phi, prob = _lib.NocfPhi(), _lib.NocfProb()
    one = C.c_void_p(16)
    for family in ("lane", "mid"):
        f_eval, f_rec, _ = ensemble_noise._entries(L, family)
        # the outputs behind alph: six buffers (evaluation); z_out, persample, sums, s_all and, one-CU, the record and its flag (recording)
        for f, outs in ((f_eval, [one] * 6), (f_rec, [one] * 4 if family == "lane" else [one] * 5 + [None])):
            def call(scale, seeds, row0, f=f, outs=outs):
                return f(C.byref(phi), C.byref(prob), one, 5, 3, 0, scale, seeds, row0, 0.0, 1.0, 2, 4, one, *outs, one, 1 << 20, None)
            assert call(None, one, 0) == -1 and call(one, None, 0) == -1
            assert call(one, one, -1) == -2


def test_sigma_and_seed_normalisation():
    E, d, nt = 3, 4, 5
    ts = (0.0, 2.0)
    # shared: E equal rows, each noise_scale's
    for shared in (0.25, [0.1, 0.2, 0.3, 0.4], torch.tensor([0.1, 0.2, 0.3, 0.4]), torch.tensor(0.25, dtype=torch.float64)):
        t = ensemble_noise.scale_table(shared, E, nt, d, ts)
        assert t.dtype == torch.float32 and tuple(t.shape) == (E, d) and t.is_contiguous()
        for e in range(E):
            assert torch.equal(t[e], noise_scale(shared, nt, d, ts)), e
    # [E, 1] broadcasts over the coordinates, [E, d] is taken row by row; nested lists and tensors alike
    lv = [[0.05], [0.0], [0.2]]
    for arg in (lv, torch.tensor(lv), torch.tensor(lv, dtype=torch.float64)):
        t = ensemble_noise.scale_table(arg, E, nt, d, ts)
        for e in range(E):
            assert torch.equal(t[e], noise_scale(float(arg[e][0]), nt, d, ts)), e           # (a float32 tensor's level is its float32 value)
    assert bool((t[1] == 0).all()) and bool((t[0] > 0).all()) and len({float(v) for v in t[2]}) == 1
    tab = uen.sigma_rows(d)[2]
    t = ensemble_noise.scale_table(tab, E, nt, d, ts)
    for e in range(E):
        assert torch.equal(t[e], noise_scale(tab[e], nt, d, ts)), e
    assert len({float(v) for v in t[0]}) > 1 and not torch.equal(t[0], t[1])
    # d == E: a 1-D [d] stays a level per coordinate
    t = ensemble_noise.scale_table([0.1, 0.2, 0.3], 3, nt, 3, ts)
    assert torch.equal(t[0], t[2]) and torch.equal(t[0], noise_scale([0.1, 0.2, 0.3], nt, 3, ts))
    # the mask zeroes columns of every row
    mask = [1.0, 0.0, 1.0, 0.0]
    t = ensemble_noise.scale_table(tab, E, nt, d, ts, mask)
    assert bool((t[:, 1] == 0).all()) and bool((t[:, 3] == 0).all()) and bool((t[:, 0] > 0).all())
    for e in range(E):
        assert torch.equal(t[e], noise_scale(tab[e], nt, d, ts, mask)), e
    # seeds
    assert ensemble_noise.seed_list(7, E) == [7, 7, 7] and ensemble_noise.seed_list((1, 2, 2 ** 64 - 1), E) == [1, 2, 2 ** 64 - 1]
    assert uen.SEEDS_OWN[1] >= 2 ** 63 and len(uen.SEEDS_OWN) == E and 0 <= uen.SEED_SHARED < 2 ** 64
    assert max(uen.ROW_OFFSETS) > 2 ** 32 and uen.ROW_OFFSETS[0] == 0


def _driver():
    import importlib.util
    spec = importlib.util.spec_from_file_location("trainOC_under_test", os.path.join(REPO, "trainOC.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("argv, text", [
    (["--members_sigma", "0.1,0.2"], "--members_sigma needs --members"),
    (["--members", "2", "--members_sigma", "0.1"], "one level per member"),
    (["--members", "2", "--members_sigma", "0.1,0.2,0.3"], "one level per member"),
    (["--members", "2", "--members_sigma", "0.1,-0.2"], "finite number >= 0"),
    (["--members", "2", "--members_sigma", "0.1,inf"], "finite number >= 0"),
    (["--members", "2", "--members_sigma", "0.1,nan"], "finite number >= 0"),
    (["--members", "2", "--members_sigma", "0.1,x"], "comma-separated list of numbers"),
    (["--members", "2", "--members_sigma", "0.1,0.2", "--noise_seed", "-1"], "--noise_seed < 2**32"),
    (["--members", "2", "--members_sigma", "0.1,0.2", "--noise_seed", str(2 ** 32)], "--noise_seed < 2**32"),
    (["--members", "2", "--members_sigma", "0.1,0.2", "--noise", "0.1"], "--members excludes --noise"),
    (["--members", "2", "--noise", "0.1"], "--members excludes --noise"),
    (["--members", "2", "--members_sigma", "0.1,0.2", "--prec", "double"], "single precision"),
    (["--members", "2", "--members_sigma", "0.1,0.2", "--m", "64"], "outside the small-network kernels"),
    (["--members", "2", "--members_sigma", "0.1,0.2", "--members_family", "mid", "--data", "singlequad", "--m", "32"], "outside the one-CU kernels"),
])
def test_driver_refusals_write_nothing(no_library, tmp_path, monkeypatch, argv, text):
    drv = _driver()
    save = tmp_path / "out"
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as ex:
        drv.main(argv + ["--niters", "1", "--save", str(save)] + ([] if "--data" in argv else ["--data", "softcorridor"]))
    assert text in str(ex.value)
    assert not save.exists()


def test_driver_accepts_the_levels(no_library):
    drv = _driver()
    args = drv.parse_args(["--members", "3", "--members_sigma", "0, 0.05,1e-1", "--noise_seed", str(2 ** 32 - 1)])
    assert drv.members_sigma_levels(args) == [0.0, 0.05, 0.1] and len(drv.members_refusals(args, 1)) == 3
    assert drv.members_sigma_levels(drv.parse_args(["--members", "3"])) is None
    assert "--members_sigma" in drv.__doc__ and "3.14" in drv.__doc__


def test_cases_cover_every_instantiation_once():
    lane_f, mid_f = [c for c in uen.FORWARD if c.family == "lane"], [c for c in uen.FORWARD if c.family == "mid"]
    lane_t, mid_t = [c for c in uen.TRAIN if c.family == "lane"], [c for c in uen.TRAIN if c.family == "mid"]
    assert [c.case for c in lane_f] == ue.FORWARD and [c.case for c in mid_f] == uem.FORWARD
    assert [c.case for c in lane_t] == ue.TRAIN and [c.case for c in mid_t] == uem.TRAIN
    assert [c.base.shape for c in lane_f] == ul.INSTANTIATIONS == [c.base.shape for c in lane_t]          # every (MP, DP) pair, once
    assert [c.base.shape for c in mid_f] == um.FORWARD_SHAPES and [c.base.shape for c in mid_t] == um.ADJOINT_SHAPES
    assert len(set(um.FORWARD_SHAPES)) == len(um.FORWARD_SHAPES) == 7                                     # every MONO_SHAPES entry, once
    assert all(c.base.n == 5 and c.base.nt == 2 for c in lane_f + lane_t) and all(c.base.n == 17 and c.base.nt == 2 for c in mid_f + mid_t)
    assert uen.E == 3
    for cases in (lane_f, mid_f, lane_t, mid_t):
        assert {c.isigma for c in cases} == {0, 1, 2} and {c.row_offset for c in cases} == set(uen.ROW_OFFSETS)
        assert {c.masked for c in cases} == {True, False}
    assert all(c.own_x for c in uen.TRAIN) and {c.own_x for c in uen.FORWARD} == {True, False}
    # shared starts: one seed; own starts: a seed per member
    assert all((c.seed == uen.SEED_SHARED) != c.own_x for c in uen.FORWARD + uen.TRAIN)
    assert all(c.seed == uen.SEEDS_OWN for c in uen.FORWARD + uen.TRAIN if c.own_x)
    # the sigma rows: three different levels; one member at 0; an [E, d] table with unequal components
    for d in (4, 12, 30):
        r0, r1, r2 = uen.sigma_rows(d)
        assert len({v[0] for v in r0}) == 3 and all(v[0] > 0 for v in r0)
        assert [v[0] > 0 for v in r1] == [True, False, True]
        assert all(len(row) == d and len(set(row)) > 1 and min(row) > 0 for row in r2) and r2[0] != r2[1]
        assert uen.member_sigma(r0, 1) == 0.1 and uen.member_sigma(r2, 2) == r2[2]
        assert 0.0 in uen.mask_of(d) and 1.0 in uen.mask_of(d)
    assert len(ids := [c.id for c in uen.FORWARD + uen.TRAIN]) == len(set(ids))
    # the cases the GPU tests pick by property exist
    for fam in ("lane", "mid"):
        assert uen.first(uen.FORWARD, fam, isigma=1) and uen.first(uen.FORWARD, fam, own_x=False) and uen.first(uen.FORWARD, fam, own_x=True)
    assert uen.first(uen.FORWARD, "lane", own_x=True, isigma=0) and uen.first(uen.FORWARD, "mid", own_x=True, isigma=2)
