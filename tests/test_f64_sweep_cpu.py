"""The double-precision sweep's mirror, truth and case lists (tests/util_f64.py) without a GPU: the Python mirror of the three
samples-per-workgroup choices equals the library's nocf_debug_f64_plan field by field over a grid (NOCF_F64_BWD_T and the NOCF_E_LDS boundary
included); the case lists of tests/test_f64_sweep_gpu.py reach every instantiation and product form they claim, asserted from the mirror;
the extended-precision truth agrees with the torch-fp64 oracle on every case (values and complex-step directional derivatives, 1e-9: a
sanity bound on the restatement, not the rule) and the screen's cap holds; and the rule rejects each wrong restatement, among them the
adjoint without the eval-mode soft-corridor term, while the 1e-9 comparison accepts a covariance off by 1e-11; the second fp64 restatement
is a correct gradient, and for every entry of util_f64.SECOND it is as far from the truth as the kernels were measured."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as entry
import util_f64 as uf
from neuraloc_amd import _lib
from util_f64 import ADJOINT, PHI, ROLLOUT


@pytest.fixture(scope="module")
def L():
    entry.build()
    lib = _lib.lib()
    assert hasattr(lib, "nocf_debug_f64_plan")
    return lib


@pytest.fixture
def bwd_t(L):
    """set NOCF_F64_BWD_T through nocf_set_knob; cleared afterwards"""
    def put(v):
        assert L.nocf_set_knob(b"NOCF_F64_BWD_T", v, 0 if v else 1) == 0
    yield put
    put(0)


def _lib_plan(L, d, m, nTh, r, n_agents, n, which):
    out = (C.c_int32 * 12)()
    rc = L.nocf_debug_f64_plan(d, m, nTh, r, n_agents, n, which, out)
    return dict(zip(uf.FIELDS, out), rc=rc)


# ---- the mirror equals the library
def test_mirror_equals_the_library_over_the_grid(L, bwd_t):
    dims = sorted({uf.dim_of(p) for p in uf.ALL_PROBLEMS} | {1, 4, 127, 128, 255})
    codes, count = set(), 0
    for t in (0, 1, 2, 4):
        bwd_t(t)
        for d in dims:
            for m in (1, 16, 255, 256, 257, 260, 511, 512, 513, 520, 1024):
                for nTh in range(2, 13):
                    for n in (1, 511, 512, 1023, 1024):
                        for which in (ROLLOUT, ADJOINT, PHI):
                            if which != ADJOINT and t:
                                continue                                    # (the knob is the adjoint's)
                            r, nag = min(10, d + 1), max(1, d // 3)
                            want = _lib_plan(L, d, m, nTh, r, nag, n, which)
                            assert uf.f64_plan(d, m, nTh, r, nag, n, which, t) == want, (d, m, nTh, n, which, t)
                            codes.add(want["rc"])
                            count += 1
    assert codes == {0, uf.E_LDS} and count == len(dims) * 11 * 11 * 5 * (2 + 4)


def test_mirror_equals_the_library_at_the_refusals(L, bwd_t):
    bwd_t(0)
    for args in ((0, 64, 2, 1, 1, 5), (12, 0, 2, 10, 1, 5), (12, 64, 1, 10, 1, 5), (12, 64, 2, 0, 1, 5), (12, 64, 2, 17, 1, 5), (12, 64, 2, 10, 1, 0)):
        for which in (ROLLOUT, ADJOINT, PHI, 3):
            want = _lib_plan(L, *args, which)
            assert want["rc"] == uf.E_SHAPE and uf.f64_plan(*args, which) == want, args
    assert _lib_plan(L, 12, 64, 2, 10, 1, 5, 3)["rc"] == uf.E_SHAPE
    # the NOCF_E_LDS boundary in each direction: the last depth and width that fit, the first that do not, per entry and forced T
    for which in (ROLLOUT, ADJOINT, PHI):
        for t in ((0, 1, 2, 4) if which == ADJOINT else (0,)):
            bwd_t(t)
            for d, nag in ((8, 4), (150, 50)):
                nTh = next(k for k in range(2, 200) if uf.f64_plan(d, 512, k, 10, nag, 1025, which, t)["rc"] == uf.E_LDS)
                for k in (nTh - 1, nTh):
                    want = _lib_plan(L, d, 512, k, 10, nag, 1025, which)
                    assert want["rc"] == (uf.E_LDS if k == nTh else 0) and uf.f64_plan(d, 512, k, 10, nag, 1025, which, t) == want
                m = next(k for k in range(256, 20000) if uf.f64_plan(d, k, 3, 10, nag, 1025, which, t)["rc"] == uf.E_LDS)
                for k in (m - 1, m):
                    want = _lib_plan(L, d, k, 3, 10, nag, 1025, which)
                    assert want["rc"] == (uf.E_LDS if k == m else 0) and uf.f64_plan(d, k, 3, 10, nag, 1025, which, t) == want
                # ... and the steps 4 -> 2 -> 1 on the way there
                Ts = [uf.f64_plan(d, 512, k, 10, nag, 1025, which, t)["T"] for k in range(2, nTh)]
                assert Ts == sorted(Ts, reverse=True) and Ts[-1] == 1
    bwd_t(0)


# ---- the case lists reach what tests/test_f64_sweep_gpu.py claims
def _has(cases, which=ROLLOUT, **want):
    return [c for c in cases if all((getattr(c, k) if hasattr(c, k) else c.plan(which)[k]) == v for k, v in want.items())]


def test_the_problem_list_is_initprobs():
    assert list(uf.ALL_PROBLEMS) == uf.problem_names()


def test_rollout_cases_reach_every_instantiation_and_product_form():
    R = uf.ROLLOUT_CASES
    assert all(c.nt <= 3 and c.plan(ROLLOUT)["rc"] == 0 for c in R)
    assert {(c.plan(ROLLOUT)["T"], c.plan(ROLLOUT)["wide"]) for c in R} == {(T, w) for T in (1, 2, 4) for w in (0, 1)}
    assert {c.stepper for c in R} == {"rk1", "rk4"}
    seg = [c for c in R if c.tspan != (0.0, 1.0)]                                                  # a time segment, both steppers
    assert {c.stepper for c in seg} == {"rk1", "rk4"} and all(c.tspan[0] != 0.0 and c.id.endswith("-seg") for c in seg)
    assert [c for c in uf.ADJOINT_CASES if c.tspan != (0.0, 1.0)]
    assert _has(R, n=1, m=24, T=1) and _has(R, n=3, m=24, T=1) and _has(R, n=513, m=24, T=2)
    assert _has(R, n=1026, m=24, T=4) and _has(R, n=1025, m=130, T=4, wide=0)                    # tails of 2 and of 1
    for n, T in ((3, 1), (513, 2)):                                                                # the register-tiled forms
        assert _has(R, n=n, m=260, T=T, f_open=uf.GEMM2, f_layer=uf.GEMM2, f_close=uf.GEMM1, trips_m=1)
        assert _has(R, n=n, m=520, T=T, f_layer=uf.GEMM2, f_close=uf.GEMM1, trips_m=2)             # second i0 trip, closing K > 256
    pipe = [c for c in R if c.plan(ROLLOUT)["f_layer"] == uf.PIPE]
    assert all(c.n == 1025 and c.plan(ROLLOUT)["T"] == 4 for c in pipe)
    assert _has(pipe, m=260, rg_m=8, pass_m=1) and uf.cdiv(260, 16) == 17                          # 17 row groups, one pass
    assert _has(pipe, m=520, rg_m=8, pass_m=2)                                                     # two passes
    assert [c for c in pipe if c.d + 1 == 5 and uf.cdiv(c.d + 1, 4) < 4 and (c.d + 1) % 4 == 1]    # fewer k-steps than the ring is deep
    assert [c for c in pipe if c.plan(ROLLOUT)["rg_d1"] == 4 and (c.d + 1) % 4 == 3 and c.prob == "swarm50"]      # closing RG = 4
    assert _has(pipe, m=258) and 258 % 4 == 2
    assert {c.plan(ROLLOUT)["rg_d1"] for c in pipe} == {2, 4}
    # a closing product at RG = 8 needs d + 1 > 256: no initProb problem has it
    assert max(uf.dim_of(p) for p in uf.ALL_PROBLEMS) + 1 <= 256 and uf.img_rg(256) == 4 and uf.img_rg(257) == 8
    # LDS fallbacks at n >= 1024, and the refusal one step beyond
    assert [c for c in R if c.n >= 1024 and c.plan(ROLLOUT)["T"] == 2 and uf.fwd_lds(c.d, c.m, c.nTh, c.n_agents, 4) * 8 > uf.LDS_BYTES]
    one = [c for c in R if c.n >= 1024 and c.plan(ROLLOUT)["T"] == 1]
    assert one and uf.fwd_lds(one[0].d, one[0].m, one[0].nTh, one[0].n_agents, 2) * 8 > uf.LDS_BYTES
    c = uf.LDS_REFUSED
    assert c.plan(ROLLOUT)["rc"] == uf.E_LDS and dataclass_replace(c, nTh=c.nTh - 1).plan(ROLLOUT)["T"] == 1


def dataclass_replace(c, **kw):
    import dataclasses
    return dataclasses.replace(c, **kw)


def test_physics_phi_and_prob_cases_reach_what_they_claim():
    P = uf.PHYSICS_CASES
    assert {(c.prob, c.training, c.plan(ROLLOUT)["T"]) for c in P} == {(p, tr, T) for p in uf.ALL_PROBLEMS for tr in (True, False) for T in (2, 4)}
    assert all(c.plan(ROLLOUT)["wide"] == 0 and c.nt <= 3 for c in P)
    assert {(c.plan(PHI)["T"], c.plan(PHI)["wide"]) for c in uf.PHI_CASES} == {(T, w) for T in (1, 2, 4) for w in (0, 1)}
    assert {(c.n, c.m) for c in uf.PHI_CASES} == {(n, m) for n in (3, 513, 1025) for m in (24, 520)}
    assert {(c.prob, c.n, c.training) for c in uf.PROB_CASES} == {(p, n, tr) for p in uf.ALL_PROBLEMS for n in (1, 19) for tr in (True, False)}


def test_adjoint_cases_reach_every_instantiation_naturally_and_forced():
    A = uf.ADJOINT_CASES
    assert all(c.nt <= 3 and c.plan(ADJOINT)["rc"] == 0 for c in A)
    five = {(4, 0), (2, 0), (1, 0), (2, 1), (1, 1)}
    key = lambda c: (c.plan(ADJOINT)["T"], c.plan(ADJOINT)["wide"])
    assert {key(c) for c in A if not c.bwd_t} == five and {key(c) for c in A if c.bwd_t} == five
    forced = [c for c in A if c.bwd_t]
    assert all(c.plan(ADJOINT)["T"] == c.bwd_t for c in forced)                                    # the knob is honoured exactly
    below = [c for c in forced if dataclass_replace(c, bwd_t=0).plan(ADJOINT)["T"] > c.bwd_t]      # ... and decides where the LDS would take more
    assert {key(c) for c in below} == {(2, 0), (1, 0), (1, 1)}
    assert any(c.n % c.plan(ADJOINT)["T"] for c in A) and any(c.n == 1 for c in A)
    assert {c.stepper for c in A} == {"rk1", "rk4"}
    kinds = {"cross2d": [c for c in A if c.training and c.prob not in ("swarm", "swarm50", "singlequad")],
             "swarm": _has(A, prob="swarm", training=True), "quad": _has(A, prob="singlequad", training=True)}
    assert all(kinds.values())
    assert _has(A, prob="softcorridor", training=False) and _has(A, prob="swap2", training=False) and _has(A, prob="singlequad", training=False)
    assert _has(A, prob="softcorridor", training=True) and _has(A, prob="swap2", training=True)
    assert uf.EVAL_SOFT_ADJOINT in A


# ---- the truth against the torch-fp64 oracle (sanity bounds on the restatement, not the rule), and the screen
VALUE_CASES = uf.ROLLOUT_CASES + uf.PHYSICS_CASES + uf.ADJOINT_CASES


@pytest.mark.parametrize("case", VALUE_CASES, ids=lambda c: c.id)
def test_truth_agrees_with_the_oracle_and_the_screen_cap_holds(case):
    t, o = uf.truth(case), uf.oracle(case)
    rows = np.asarray(t["rows"])
    assert uf.screen_ok(case), (t["rows"], t["keep"])
    keep = t["keep"]
    assert uf.rows_off_1e9(o["table"][rows][keep], t["table"][keep].astype(np.float64)) == 0
    for k, sel in (("z", o["z"][keep]), ("zFull", o["zFull"][keep]), ("ctrlFull", o["ctrlFull"][keep]), ("s_all", o["s_all"][:, rows][:, keep])):
        want = t[k][keep] if k != "s_all" else t[k][:, keep]
        assert float(np.abs(sel - want).max()) <= 1e-9 * max(1.0, float(np.abs(want).max())), k
    assert float(np.abs(t["ctrlFull"][:, :, 0]).max()) == 0.0
    # the case exercises its physics: with an obstacle the truth's Q column is nonzero on a row the rule judges, without one it is exactly 0
    S = uf.spec_of(case)
    if S.obstacle is None or (S.kind == "swarmtraj" and S.alph_Q <= 0):
        assert not t["table"][:, 5].any()
    else:
        assert t["table"][keep][:, 5].any(), "Q is 0 on every judged row"
    # the time column of the stage inputs starts at the segment's t0 and the final evaluation sits at t1
    assert float(t["s_all"][0, 0, -1]) == case.tspan[0] and float(t["final"][0, -1]) == case.tspan[1]


@pytest.mark.parametrize("case", uf.ADJOINT_CASES, ids=lambda c: c.id)
def test_complex_step_agrees_with_fp64_autograd(case):
    assert len(uf.truth_rows(case)) == case.n                   # (Jc and its derivatives are the whole batch's)
    Jo, og = uf.oracle_grads(case)
    J, dirs = uf.grad_truth(case)
    assert abs(Jo - float(J)) <= 1e-9 * abs(Jo)
    names = {name for name, *_ in dirs}
    assert names == set(uf.param_names(case)) | {"x0"}
    for name, label, v, want, scale in dirs:
        got = float(uf.dot(og[name], v))
        assert abs(got - float(want)) <= 1e-9 * max(scale, 1e-300), (name, label, got, float(want), scale)


@pytest.mark.parametrize("case", uf.PHI_CASES, ids=lambda c: c.id)
def test_phi_truth_agrees_with_the_oracle(case):
    rows, (g, v), (og, ov) = uf.phi_truth(case)
    assert float(np.abs(og[rows] - g).max()) <= 1e-11 * max(1.0, float(np.abs(g).max()))
    assert float(np.abs(ov[rows] - v).max()) <= 1e-11 * max(1.0, float(np.abs(v).max()))


@pytest.mark.parametrize("case", uf.PROB_CASES, ids=lambda c: c.id)
def test_prob_truth_agrees_with_the_oracle(case):
    p, t, o, keep = uf.prob_truth(case)
    assert keep.sum() >= 0.9 * case.n
    for k in t:
        assert float(np.abs(o[k][keep] - t[k][keep]).max()) <= 1e-11 * max(1.0, float(np.abs(t[k][keep]).max())), k


# ---- the rule has teeth
def _stand_in(case, mut=None, kernel_forms=True):
    """the fp64 numpy restatement in the kernel's activation forms (a stand-in for a kernel), on all rows of the truth subset"""
    t = uf.truth(case)
    got = uf.restate(case, np.float64, t["rows"], mut=mut, kernel_forms=kernel_forms and mut != "log1p_f32", intermediates=True)
    full = {}
    n, rows = case.n, np.asarray(t["rows"])
    tab = np.full((n, 7), np.nan)
    tab[rows] = got["table"]
    s_all = np.full((got["s_all"].shape[0], n, case.d + 1), np.nan)
    s_all[:, rows] = got["s_all"]
    full.update(table=tab, s_all=s_all, z=got["z"], zFull=got["zFull"], ctrlFull=got["ctrlFull"])
    return full


def _pick(cases, **want):
    out = _has(cases, **want)
    assert out, want
    return out[0]


MUTATION_CASES = {
    "two_pi_f32": lambda: _pick(uf.PHYSICS_CASES, prob="softcorridor", n=513, training=False),
    "hN_f32": lambda: _pick(uf.ADJOINT_CASES, nTh=4),
    "stage_time_f32": lambda: _pick(uf.ROLLOUT_CASES, stepper="rk4", nt=3),
    "log1p_f32": lambda: _pick(uf.ROLLOUT_CASES, n=1),
    "drop_last_k": lambda: _pick(uf.ROLLOUT_CASES, m=258),
    "lost_second_pass": lambda: _pick(uf.ROLLOUT_CASES, m=520, n=1025),
    "row_alias_256": lambda: _pick(uf.ROLLOUT_CASES, m=260, n=3),
    "reduce_64": lambda: _pick(uf.PHYSICS_CASES, prob="swarm", n=513, training=True),
    "cov_1e-11": lambda: _pick(uf.PHYSICS_CASES, prob="softcorridor", n=513, training=True),
}


def test_every_mutation_has_a_case():
    assert set(MUTATION_CASES) == set(uf.MUTATIONS)
    assert (258 + 0) % 4 != 0 and _pick(uf.PHYSICS_CASES, prob="swarm", n=513, training=True).plan(ROLLOUT)["T"] == 2


@pytest.mark.parametrize("mutation", uf.MUTATIONS)
def test_rule_rejects_a_wrong_restatement(mutation):
    case = MUTATION_CASES[mutation]()
    good = uf.compare_rollout(case, _stand_in(case))
    assert not uf.failures(good), (case.id, uf.failures(good))                 # the rule accepts the restatement without the defect
    bad = uf.failures(uf.compare_rollout(case, _stand_in(case, mutation)))
    assert bad, (case.id, mutation)
    print(case.id, mutation, {k: (f"{e:.3g}", f"{t:.3g}") for k, (_, e, t, _) in bad.items()})
    if mutation == "cov_1e-11":
        # what the new rule adds: the existing double-against-double comparison accepts this defect
        t, o = uf.truth(case), uf.oracle(case)
        rows = np.asarray(t["rows"])
        got = _stand_in(case, mutation)
        assert float(np.abs(t["table"][:, 5]).max()) > 0
        assert uf.rows_off_1e9(got["table"][rows], o["table"][rows]) == 0
        for k in ("z", "zFull", "ctrlFull"):
            assert float(np.abs(got[k] - o[k]).max()) <= 1e-9 * max(1.0, float(np.abs(o[k]).max()))


def test_rule_rejects_the_adjoint_without_the_eval_mode_soft_corridor_term():
    """the double-precision adjoint before its fix: f64_xgrad took the soft corridor's x-gradient in train mode only"""
    case = uf.EVAL_SOFT_ADJOINT
    _, og = uf.oracle_grads(case)
    assert not uf.failures(uf.compare_grads(case, og))
    _, mg = uf.mutated_grads(case)
    bad = uf.failures(uf.compare_grads(case, mg))
    assert bad and any(k.startswith("x0/") for k in bad), bad
    # train mode is not affected by the defect
    train = dataclass_replace(case, training=True)
    _, mg = uf.mutated_grads(train)
    assert not uf.failures(uf.compare_grads(train, mg))


# ---- the second restatement and the entries of util_f64.SECOND, shown without a GPU
@pytest.mark.parametrize("case", uf.ADJOINT_CASES, ids=lambda c: c.id)
def test_second_restatement_of_the_gradient_is_a_correct_gradient(case):
    """util_f64.second_grads (the adjoint as the kernel and train.py form it, float64 numpy) against fp64 autograd: both are double
    evaluations of the same gradient that differ by summation order, bound 1e-12 of each tensor's largest entry (measured: up to 3.5e-14)"""
    _, og = uf.oracle_grads(case)
    sg = uf.second_grads(case)
    assert set(sg) == set(og)
    for k in og:
        assert float(np.abs(sg[k].reshape(og[k].shape) - og[k]).max()) <= 1e-12 * float(np.abs(og[k]).max()) + 1e-300, k


@pytest.mark.parametrize("case", sorted({c for c in VALUE_CASES if any(cid == c.id for cid, _ in uf.SECOND)}, key=lambda c: c.id)
                         + [uf.ROLLOUT_CASES[0], uf.PHYSICS_CASES[-1]], ids=lambda c: c.id)
def test_second_restatement_of_the_values_agrees_with_the_oracle(case):
    """util_f64.second_values against the torch-fp64 oracle on the truth rows: 1e-11 where the existing comparison has 1e-9"""
    t, o, s2 = uf.truth(case), uf.oracle(case), uf.second_values(case)
    rows = np.asarray(t["rows"])
    assert uf.rows_off_1e9(s2["table"], o["table"][rows], rtol=1e-11) == 0
    for k in ("z", "zFull", "ctrlFull"):
        assert float(np.abs(s2[k] - o[k]).max()) <= 1e-11 * max(1.0, float(np.abs(o[k]).max())), k


def _case_of(cid):
    return next(c for c in VALUE_CASES if c.id == cid)


@pytest.mark.parametrize("cid,key", sorted(uf.SECOND), ids=lambda v: str(v))
def test_second_restatement_is_as_far_from_the_truth_as_the_kernels_were_measured(cid, key):
    """every entry of util_f64.SECOND: 4 x the second restatement's error on that quantity reaches the error the kernels were measured at on
    the MI355X, so the larger of the two restatements' errors (factor and floor unchanged) covers it"""
    case, measured = _case_of(cid), uf.SECOND[(cid, key)]
    if key.startswith("table."):
        t = uf.truth(case)
        c = uf.TABLE_COLS.index(key.split(".")[1])
        e2 = float(np.abs(uf.second_values(case)["table"][:, c] - t["table"][:, c])[t["keep"]].max())
    else:
        e2 = uf.compare_grads(case, uf.second_grads(case), second=False)[key][1]
        assert key.rsplit("/", 1)[1] in ("first", "last", "argmax")                                   # unit directions only
    assert uf.TOL_FACTOR * e2 >= measured, (e2, measured)


def test_the_exceptions_are_few_and_name_listed_cases():
    ids = {c.id for c in VALUE_CASES}
    assert all(cid in ids for cid, _ in uf.SECOND) and len(uf.SECOND) <= 40
