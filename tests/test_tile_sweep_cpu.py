"""The per-tile sweep's mirror and case lists (tests/util_tile.py) without a GPU: the Python mirror of plan_layout / choose_sk equals the
library's nocf_debug_tile_plan field by field over a grid of shapes, depths, directions and knobs (the NOCF_E_LDS / NOCF_E_SHAPE boundaries
included); the lists reach every geometry item they claim, asserted from the mirror; every case reaches the per-tile kernel under its knobs
per the dispatcher mirror; every case exercises its physics in fp64 and keeps clear of the screen's margins; and the comparator rejects
the wrong restatements on the cases that can show them."""
import ctypes as C

import pytest
import torch

import __graft_entry__ as entry
import util_mono as um
import util_oracle as uo
import util_tile as ut
from neuraloc_amd import _lib

ALL = ut.FORWARD + ut.FIXED_EVAL + ut.FIXED_TRAIN + ut.ADJOINT
SMALL = [tc for tc in ut.FORWARD if tc.case.n < ut.BIG]
GENERIC = ut.FORWARD                                       # (every case of FORWARD takes the generic instantiation: asserted below)


@pytest.fixture(scope="module")
def L():
    entry.build()
    return _lib.lib()


def _lib_plan(L, d, m, nTh, r, n_agents, bwd):
    out = (C.c_int32 * 12)()
    rc = L.nocf_debug_tile_plan(d, m, nTh, r, n_agents, bwd, out)
    return dict(zip(ut.FIELDS, out), rc=rc)


@pytest.fixture
def lib_knobs(L):
    """set NOCF_NWAVES / NOCF_SUBTILES through nocf_set_knob; cleared afterwards"""
    def put(nw, S):
        for name, v in ((b"NOCF_NWAVES", nw), (b"NOCF_SUBTILES", S)):
            assert L.nocf_set_knob(name, v, 0 if v else 1) == 0
    yield put
    put(0, 0)


# ---- the mirror equals the library
def test_mirror_equals_the_library_over_the_grid(L, lib_knobs):
    codes, n = set(), 0
    for nw in (0, 1, 2, 4, 8):
        for S in (0, 2, 4):
            lib_knobs(nw, S)
            for d in (1, 3, 12, 31, 32, 62, 63, 64, 96, 150, 200):
                for m in (1, 16, 63, 64, 65, 128, 129, 257, 512, 513, 700, 1024, 2048):
                    for nTh in (2, 3, 6, 12):
                        for bwd in (0, 1):
                            for r, nag in ((min(10, d + 1), max(1, d // 3)), (min(16, d + 1), max(1, d // 2))):
                                want = _lib_plan(L, d, m, nTh, r, nag, bwd)
                                assert ut.tile_plan(d, m, nTh, r, nag, bwd, nw, S) == want, (d, m, nTh, r, nag, bwd, nw, S)
                                codes.add(want["rc"])
                                n += 1
    assert codes == {0, ut.E_LDS} and n == 2 * 17160


def test_mirror_equals_the_library_at_the_refusals_and_the_compiled_shapes(L, lib_knobs):
    lib_knobs(0, 0)
    for args in ((0, 64, 2, 1, 1), (12, 0, 2, 10, 1), (12, 64, 1, 10, 1), (12, 64, 13, 10, 1), (12, 64, 2, 0, 1), (12, 64, 2, 14, 1),
                 (30, 64, 2, 17, 1), (12, 64, 2, 10, 256)):
        for bwd in (0, 1):
            want = _lib_plan(L, *args, bwd)
            assert want["rc"] == ut.E_SHAPE and ut.tile_plan(*args, bwd) == want, args
    for nw, S in ((3, 0), (16, 0), (0, 3), (0, 8)):                     # knob values the plan refuses
        lib_knobs(nw, S)
        want = _lib_plan(L, 12, 64, 2, 10, 6, 0)
        assert want["rc"] == ut.E_SHAPE and ut.tile_plan(12, 64, 2, 10, 6, 0, nw, S) == want, (nw, S)
    lib_knobs(0, 0)
    for shape in ut.FIXED_SHAPES + ut.FIXED_SHAPES_TRAIN:
        for bwd in (0, 1):
            want = _lib_plan(L, *shape, bwd)
            assert want["fixed"] == (1 if shape in ut.FIXED_SHAPES else 2) and ut.tile_plan(*shape, bwd) == want, shape
        d, m, nTh, r, nag = shape
        assert _lib_plan(L, d, m, nTh, r, nag + 1, 0)["fixed"] == 0 == ut.tile_plan(d, m, nTh, r, nag + 1)["fixed"]     # (agents are part of a plan)
    for nw, S in ((4, 0), (0, 2)):                                      # ... and so is the geometry: a knob leaves the compiled plans
        lib_knobs(nw, S)
        want = _lib_plan(L, 150, 512, 2, 10, 50, 0)
        assert want["fixed"] == 0 and ut.tile_plan(150, 512, 2, 10, 50, 0, nw, S) == want
    lib_knobs(0, 0)
    # the LDS boundary in m at swarm50's d, both directions: the last width that fits and the first that does not
    for bwd in (0, 1):
        ok = [m for m in range(512, 2049, 64) if _lib_plan(L, 150, m, 2, 10, 50, bwd)["rc"] == 0]
        assert ok and ok == [m for m in range(512, 2049, 64) if ut.tile_plan(150, m, 2, 10, 50, bwd)["rc"] == 0]
        assert _lib_plan(L, 150, ok[-1] + 64, 2, 10, 50, bwd) == ut.tile_plan(150, ok[-1] + 64, 2, 10, 50, bwd)
        assert ut.tile_plan(150, ok[-1] + 64, 2, 10, 50, bwd)["rc"] == ut.E_LDS


def test_every_case_plan_equals_the_library(L, lib_knobs):
    for tc in ALL + ut.DISTURBED:
        lib_knobs(tc.nw, tc.S)
        c = tc.case
        for bwd in (0, 1):
            assert tc.plan(bwd) == _lib_plan(L, c.d, c.m, c.nTh, c.r, c.n_agents, bwd), tc.id


def test_split_k_facts_of_the_mirror():
    """what the case lists rely on: SK1 > 1 needs forced waves; SKm > 1 starts at m = 513; the LDS loop binds where the lists say it does"""
    for d in (12, 31, 62, 96, 150, 200):
        for m in (1, 64, 129, 257, 512, 513, 700, 1024):
            p = ut.tile_plan(d, m, 2, min(10, d + 1), 1)
            assert p["rc"] != 0 or p["SK1"] == 1, (d, m)
    assert ut.tile_plan(96, 32, 2, 10, 32, 0, 4)["SK1"] == 4
    assert [ut.tile_plan(150, m, 2, 10, 50)["SKm"] for m in (512, 513)] == [1, 2]
    assert {ut.tile_plan(150, m, 2, 10, 50)["MB"] for m in (512, 513)} == {8, 9}
    assert ut.tile_plan(150, 520, 2, 10, 50, 1)["cap"] == 1 and ut.tile_plan(12, 700, 2, 10, 6, 1)["cap"] == 1
    assert ut.tile_plan(150, 512, 2, 10, 50, 0, 0, 2)["cap"] == 1 and ut.tile_plan(150, 512, 2, 10, 50)["cap"] == 8
    assert ut.tile_plan(40, 1024, 2, 10, 20, 1)["rc"] == ut.E_LDS and ut.tile_plan(150, 2048, 2, 10, 50)["rc"] == ut.E_LDS
    assert ut.choose_sk(1, 4, 4, 8) == 4 and ut.choose_sk(8, 16, 8, 8) == 1 and ut.choose_sk(9, 17, 8, 8) == 2


# ---- every case reaches the per-tile kernel under its knobs
def test_every_case_reaches_the_tile_kernel():
    for tc in ut.FORWARD + ut.FIXED_EVAL + ut.FIXED_TRAIN:
        assert ut.forward_family(tc.case, tc.env) == "tile" == ut.forward_family(tc.case, tc.env, recording=True), tc.id
        assert tc.plan()["rc"] == 0, tc.id
    for tc in ut.DISTURBED:
        assert ut.forward_family(tc.case, tc.env, dist=True) == "tile" and tc.plan()["rc"] == 0, tc.id
    for tc in ut.ADJOINT:
        assert ut.adjoint_family(tc.case, tc.env) == "tile" and ut.adjoint_rc(tc) == 0, tc.id
        assert ut.forward_family(tc.case, tc.env, recording=True) == tc.fwd, tc.id
    for tc in GENERIC + ut.DISTURBED:
        assert not tc.specialised() and not tc.specialised(recording=True), tc.id
    for tc in ut.FIXED_EVAL:
        assert tc.specialised() and tc.plan()["fixed"] == 1, tc.id
    for tc in ut.FIXED_TRAIN:
        assert tc.specialised(recording=True) and not tc.specialised() and tc.plan()["fixed"] == 2, tc.id
    assert [(tc.case.d, tc.case.m, tc.case.nTh, tc.case.r, tc.case.n_agents) for tc in ut.FIXED_EVAL] == ut.FIXED_SHAPES
    assert [(tc.case.d, tc.case.m, tc.case.nTh, tc.case.r, tc.case.n_agents) for tc in ut.FIXED_TRAIN] == ut.FIXED_SHAPES_TRAIN
    # knobs are set only where they are needed: without them another family would win (or may win: the split-role kernel)
    for tc in ALL:
        for name in ("NOCF_LANE", "NOCF_MONO", "NOCF_DUO"):
            if name in tc.env and tc.fwd == "tile":
                env = {k: v for k, v in tc.env.items() if k != name}
                fam = {ut.forward_family(tc.case, env), ut.forward_family(tc.case, env, recording=True), ut.adjoint_family(tc.case, env)}
                assert fam != {"tile"}, (tc.id, name)
    ids = [tc.id for tc in ALL + ut.DISTURBED]
    assert len(set(ids)) == len(ids)


def test_dispatch_mirror_boundaries():
    from oracle import ocflow_oracle as orc
    c = ut._C("cross2d", 12, 512, 10, None, "eval", 4, "rk4", 1)
    fam = lambda c, rec=False, **kn: ut.forward_family(c, {k: str(v) for k, v in kn.items()}, recording=rec)      # noqa: E731
    import dataclasses
    assert fam(c) == "duo" and fam(c, NOCF_DUO=0) == "tile" and fam(dataclasses.replace(c, m=513)) == "tile"
    assert fam(dataclasses.replace(c, m=129)) == "duo" and fam(dataclasses.replace(c, m=128)) == "mono"
    assert fam(dataclasses.replace(c, m=257), rec=True) == "tile" and fam(dataclasses.replace(c, m=256), rec=True) == "duo"
    assert fam(dataclasses.replace(c, nTh=3)) == "tile" and fam(dataclasses.replace(c, kind="quad")) == "tile"
    assert fam(dataclasses.replace(c, d=160)) == "tile" and fam(dataclasses.replace(c, d=130)) == "tile"          # d + 1 > 160; 65 agents
    assert ut.forward_family(c, {}, dist=True) == "tile"
    s = ut._C("cross2d", 12, 32, 10, None, "train", 4, "rk4", 1)
    assert fam(s) == "lane" and fam(s, NOCF_LANE=0) == "mono" and fam(s, NOCF_LANE=0, NOCF_MONO=0) == "tile"
    assert fam(dataclasses.replace(s, m=64), rec=True, NOCF_MONO_REC=0) == "tile" and fam(dataclasses.replace(s, m=64), NOCF_MONO_REC=0) == "mono"
    assert ut.adjoint_family(s, {}) == "lane" and ut.adjoint_family(s, {"NOCF_LANE": "0"}) == "tile"           # (m <= 32: no one-CU adjoint)
    assert ut.adjoint_family(dataclasses.replace(s, m=64), {}) == "mono"
    assert ut.adjoint_family(dataclasses.replace(s, m=64), {"NOCF_MONO_BWD": "0"}) == "tile"
    assert ut.adjoint_family(c, {}) == "duo" and ut.adjoint_family(c, {"NOCF_DUO_BWD": "0"}) == "tile"
    assert ut.adjoint_family(dataclasses.replace(c, r=11), {}) == "tile"
    assert orc.KIND_QUAD == ut.KINDS["quad"]


# ---- coverage, from the mirror
def test_forward_generic_coverage():
    P = [(tc, tc.plan()) for tc in GENERIC]
    D = [(tc, p) for tc, p in P if not tc.nw and not tc.S]
    assert {p["T"] for _, p in P} == {4, 8, 16} and {tc.S for tc in GENERIC} == {0, 2, 4}
    for T in (4, 8, 16):                                                  # with and without recording (train mode: the recording forward runs too)
        assert {tc.case.mode for tc, p in P if p["T"] == T} == {"eval", "train"}, T
        ns = {tc.case.n for tc, p in P if p["T"] == T and tc.case.n < ut.BIG}
        assert ns >= {1, T - 1, T, T + 1} and any(1 < n < T - 1 for n in ns), (T, ns)
        assert any(n > T + 1 and n % T not in (0, 1, T - 1) for n in ns), (T, ns)                   # a ragged batch of several tiles
    assert any(tc.case.n > 4 * ut.BIG_TILES and tc.case.n % 4 for tc, p in D)
    # waves: the default 1 / 2 / 4 / 8 from MB = 1 / 2 / 3 / 5, and forced on either side of the default
    assert {(p["MB"], p["nwaves"]) for _, p in D} >= {(1, 1), (2, 2), (3, 4), (5, 8)}
    forced = [(tc, p) for tc, p in P if tc.nw]
    assert any(p["nwaves"] > ut.default_waves(tc.case.m) for tc, p in forced) and any(p["nwaves"] < ut.default_waves(tc.case.m) for tc, p in forced)
    assert {p["nwaves"] for _, p in forced} == {1, 2, 4, 8}
    assert {p["MB"] for _, p in P} >= {1, 2, 3, 5, 9, 16} and sum(p["MB"] % p["nwaves"] != 0 for _, p in P) >= 4
    assert any(p["MB"] > p["nwaves"] and p["MB"] % p["nwaves"] for _, p in D)            # a wave walks an uneven share of blocks
    assert {min(p["DB"], 4) for _, p in P} == {1, 2, 3, 4}
    d1 = {tc.case.d + 1 for tc in GENERIC}
    assert {63, 65} <= d1 and {31, 33} <= d1 and any(64 < x <= 96 for x in d1) and any(96 < x <= 128 for x in d1)
    assert {p["KQ1"] for _, p in P} >= {8, 16, 24, 32, 40, 56}
    ms = {tc.case.m for tc in GENERIC}
    assert {1, 63, 64, 65, 128, 129, 130, 257, 513, 1024} <= ms and any(m % 4 for m in ms)
    # split-K
    assert any(p["SK1"] > 1 for _, p in P) and not any(p["SK1"] > 1 for _, p in D)
    assert any(p["SKm"] > 1 for _, p in D)
    sk6 = {p["SK6"] for _, p in P}
    assert {1, 2, 3} <= sk6 and any(s >= 5 for s in sk6)
    two = [tc for tc, p in P if len({s for s in (p["SK1"], p["SK6"], p["SKm"]) if s > 1}) >= 2]
    assert len({(tc.case.d, tc.case.m) for tc in two}) >= 2, [tc.id for tc in two]
    assert any(0 < p["cap"] < 8 for _, p in P)
    assert any(tc.case.d == 150 and tc.case.m == 512 and tc.S == 2 and p["cap"] == 1 for tc, p in P)
    # depth, rank, problems
    assert {tc.case.nTh for tc in GENERIC} >= {2, 3, 4, 6, 12}
    assert {tc.case.r for tc in GENERIC} >= {1, 10, 16} and any(tc.case.r == tc.case.d + 1 <= 16 for tc in GENERIC)
    kinds = {(tc.case.kind, tc.case.obstacle) for tc in GENERIC}
    assert kinds >= {("cross2d", None), ("cross2d", "softcorridor"), ("cross2d", "hardcorridor"), ("swarm", "blocks"), ("quad", None)}
    assert max(tc.case.n_agents for tc in GENERIC if tc.case.kind == "cross2d") == 100
    assert {tc.case.n_agents for tc in GENERIC if tc.case.kind == "swarm"} >= {32, 50}
    quads = [tc.case for tc in GENERIC if tc.case.kind == "quad" and tc.case.angles == "quadrants" and tc.case.n >= 16]
    assert {c.n_agents for c in quads} == {1, 2} and {c.m for c in quads} == {129, 130}
    assert any(tc.case.alph_Q == 0.0 and tc.case.obstacle for tc in GENERIC) and any(tc.case.alph_W == 0.0 and tc.case.n_agents >= 2 for tc in GENERIC)
    for group in (ut.FORWARD_DEFAULT, ut.FORWARD_FORCED):
        assert {tc.case.stepper for tc in group} == {"rk4", "rk1"} and {tc.case.tspan for tc in group} == {ut.T1, ut.T2}
        assert all(1 <= tc.case.nt <= 9 for tc in group) and {tc.case.mode for tc in group} == {"eval", "train"}
    assert all(not tc.nw and not tc.S for tc in ut.FORWARD_DEFAULT) and all(tc.nw or tc.S for tc in ut.FORWARD_FORCED)


def test_disturbed_and_fixed_coverage():
    assert [tc.plan()["T"] for tc in ut.DISTURBED] == [8, 16]
    for tc in ut.DISTURBED:
        assert tc.case.n % tc.plan()["T"] not in (0, 1), tc.id
    for tc in ut.FIXED_EVAL + ut.FIXED_TRAIN:
        assert tc.case.n <= 9
    assert any(tc.case.n % 4 for tc in ut.FIXED_EVAL) and any(tc.case.n % 4 for tc in ut.FIXED_TRAIN)
    assert all(tc.env.get("NOCF_LANE") == "0" for tc in ut.FIXED_TRAIN)


def test_adjoint_coverage():
    P = [(tc, tc.plan(1)) for tc in ut.ADJOINT]
    assert all(p["T"] == 4 and tc.case.mode == "train" for tc, p in P)
    spec = [(tc.case.d, tc.case.m) for tc, p in P if tc.specialised(bwd=1)]
    assert (150, 512) in spec and (12, 128) in spec and sum(p["fixed"] == 2 for tc, p in P if tc.specialised(bwd=1)) >= 2
    assert sum(not tc.specialised(bwd=1) for tc, _ in P) >= 8
    assert {tc.case.nTh for tc in ut.ADJOINT} >= {2, 3, 6, 12}
    assert any(tc.fwd == "mono" and tc.case.act_rec and um.mono_record_eligible(2, tc.case.m, tc.case.d, tc.case.r, tc.case.n_agents) for tc in ut.ADJOINT)
    assert any(tc.fwd == "mono" and not tc.case.act_rec and tc.env.get("NOCF_ACT_REC") == "0" for tc in ut.ADJOINT)
    assert any(p["DB"] >= 2 and tc.case.nTh >= 3 for tc, p in P)
    assert {(tc.case.d, tc.case.m) for tc, p in P if p["cap"] < 4} >= {(150, 520), (12, 700)}
    assert any(p["SK1"] > 1 and tc.nw for tc, p in P) and any(p["SK6"] > 1 for _, p in P) and any(p["SKm"] > 1 for _, p in P)
    assert any(tc.case.n_total not in (None, tc.case.n) for tc in ut.ADJOINT)
    assert {tc.case.n for tc in ut.ADJOINT} >= {1, 3, 5, 17}
    assert any(tc.case.n > 4 * ut.BIG_TILES and tc.case.n % 4 and tc.case.nt == 2 for tc in ut.ADJOINT)
    assert any(tc.case.kind == "quad" and tc.case.n_agents == 2 and tc.case.n >= 16 for tc in ut.ADJOINT)
    assert {tc.case.stepper for tc in ut.ADJOINT} == {"rk4", "rk1"} and {tc.case.tspan for tc in ut.ADJOINT} == {ut.T1, ut.T2}


def test_refusal_list():
    for what, c, kn, bwd, code in ut.REFUSALS:
        tc = ut.TileCase(c, tuple(sorted(kn.items())))
        assert (ut.adjoint_rc(tc) if bwd else tc.plan()["rc"]) == code, what
    assert {code for *_, code in ut.REFUSALS} == {ut.E_SHAPE, ut.E_LDS}
    assert ut.tile_plan(12, 64, 3, 13, 6, 1, 0, 2)["rc"] == 0           # (the plan itself exists: the adjoint has no T = 8 instantiation)


# ---- the cases' physics and the screen
def _unique(tcs):
    seen, out = set(), []
    for tc in tcs:
        if tc.case not in seen:
            seen.add(tc.case)
            out.append(tc)
    return out


@pytest.mark.parametrize("tc", _unique(ALL), ids=lambda tc: tc.id)
def test_cases_exercise_their_physics(tc):
    """Q / W nonzero where on and exactly zero where off, the angle cases visit all eight quadrant / sign pairs; the case finds its n
    starts among n + max(16, n / 2) candidates (util_mono.case_data's rule: it asserts that), none of their evaluated states within the
    screen's margins; the fp32 restatement passes its own comparator"""
    case = tc.case
    D = um.case_data(case)
    assert D["x"].shape == (case.n, case.d)
    assert um.physics_gaps(case, D["r64"]) == []
    assert not bool(um.near_edge(case, D["r64"]["stages"]).any())
    assert um.failures(um.compare_forward(D["r32"], D["r64"], D["r32"])) == {}


def test_two_craft_interact():
    two = [tc.case for tc in ALL if tc.case.kind == "quad" and tc.case.n_agents == 2 and tc.case.n >= 16]
    assert len(two) >= 2
    for c in two:
        assert bool((um.case_data(c)["r64"]["table"][:, 6] > 0).any()), c.id


# ---- the comparator has teeth
def _teeth(mutation, tcs):
    """-> the cases on which the mutated fp64 oracle fails the comparator"""
    caught = []
    for tc in tcs:
        D = um.case_data(tc.case)
        bad = ut.mutated_forward(tc, D["x"], mutation)
        if um.failures(um.compare_forward(bad, D["r64"], D["r32"])):
            caught.append(tc)
    return caught


@pytest.mark.parametrize("mutation", ["rank_minus_one", "last_hidden_dropped", "k_block_dropped", "column_block_dropped", "k_tail_opening", "k_tail_residual",
                                      "k_tail_closing", "residual_layer_skipped", "ragged_row_is_its_neighbour"])
def test_comparator_rejects_a_wrong_geometry_on_every_case_that_can_show_it(mutation):
    """A'A from r - 1 rows, the last hidden unit dropped, the last hidden 16-block dropped, the last 64-column block of hidden units dropped, the last 1 / SK of the opening /
    residual / closing contraction's k-range dropped (SK: the case's own factor, at least 2), the last residual layer skipped, the last
    row of a ragged tile replaced by its neighbour"""
    tcs = [tc for tc in SMALL if ut.mutation_applies(tc, mutation) and (tc.case.r > 1 or mutation != "rank_minus_one")]
    assert len(tcs) >= 6, mutation
    caught = _teeth(mutation, tcs)
    assert caught == tcs, (mutation, [tc.id for tc in tcs if tc not in caught])


def test_comparator_rejects_wrong_time_threshold_and_quadcopter_physics():
    assert _teeth("time_from_zero", [tc for tc in SMALL if tc.case.tspan[0] != 0.0])
    ev = [tc for tc in SMALL if tc.case.mode == "eval" and tc.case.alph_W != 0.0 and tc.case.n_agents >= 2 and tc.case.kind != "quad"]
    assert _teeth("train_threshold_in_eval", ev)
    ang = [tc for tc in SMALL if tc.case.angles == "quadrants"]
    assert ang and _teeth("sin_sign_in_one_quadrant", ang) == ang
    two = [tc for tc in SMALL if tc.case.kind == "quad" and tc.case.n_agents == 2 and tc.case.n >= 16]
    for mutation in ("second_craft_dropped_from_W", "quad_pair_distance_over_all_12"):
        assert _teeth(mutation, two), mutation
    assert set(ut.MUTATIONS) == set(um.MUTATIONS) | {"column_block_dropped", "k_tail_opening", "k_tail_residual", "k_tail_closing",
                                                     "residual_layer_skipped", "ragged_row_is_its_neighbour"}


def test_k_cut():
    assert ut.k_cut(97, 32, 4) == 96 and ut.k_cut(96, 32, 4) is None and ut.k_cut(13, 8, 1) is None and ut.k_cut(41, 16, 1) == 32
    assert ut.k_cut(700, 176, 8) == 616 and ut.k_cut(64, 16, 3) == 42


def test_standalone_references_are_the_oracles():
    tc = next(t for t in ut.ADJOINT if t.case.nTh == 3 and t.case.n <= 8)
    s, g = ut.standalone_inputs(tc.case, 5)
    val, vjp = ut.standalone_grads(tc.case, s, g, torch.float64)
    assert set(val) == set(vjp) and val["x"].shape == s.shape and g.dtype == torch.float64
    from oracle import ocflow_oracle as orc
    P = orc.PhiParams.from_state_dict(um.case_sd(tc.case), dtype=torch.float64)
    assert float((val["x"] - orc.phi_grad(P, s.double())).abs().max()) <= 1e-12 * float(val["x"].abs().max())


def test_second_yardstick_is_a_restatement_of_the_kernels_activations():
    """util_tile.kernel_activations: sigma and tanh as csrc/nocf_dev.h act_pair forms them, within a few ulp of the plain ones in fp32 and
    untouched in fp64; the cases it is a yardstick for exist, and its gradients are a restatement in their own right (they pass the plain
    comparator's rule against fp64 with the plain fp32 run as yardstick, at twice the factor)"""
    from oracle import ocflow_oracle as orc
    o = torch.linspace(-12.0, 12.0, 4001)
    with ut.kernel_activations():
        s32, t32, s64 = orc.sigma(o), torch.tanh(o), orc.sigma(o.double())
    assert torch.equal(s64, orc.sigma(o.double()))
    assert float((s32.double() - orc.sigma(o.double())).abs().max()) <= 4 * 2.0 ** -23 * 12.0
    assert float((t32.double() - torch.tanh(o.double())).abs().max()) <= 4 * 2.0 ** -24
    assert orc.sigma is not None and torch.tanh(o[:1]).dtype == torch.float32
    ids = {tc.id: tc for tc in ut.ADJOINT}
    assert set(ut.SECOND_YARDSTICK) <= set(ids)
    for cid in ut.SECOND_YARDSTICK:
        c = ids[cid].case
        x = um.case_data(c)["x"]
        _, g64, _ = um.oracle_grads(c, x, torch.float64)
        _, g32, _ = um.oracle_grads(c, x, torch.float32)
        _, gk, _ = ut.oracle_grads_kernel_activations(c, x)
        for k in g64:
            if g64[k] is not None:
                tol, _ = uo.tolerance(g64[k], g32[k])
                assert float((gk[k].double() - g64[k]).abs().max()) <= 2 * tol, k
