"""CPU: the case list, the references, the self-agreement screens and the comparator of the quadcopter L-BFGS sweep (util_quad_sweep;
the GPU half is test_baseline_quad_sweep_gpu.py).  No GPU runs here: the fp64 reference is the one the GPU file uses, and util_quad's
fp32 restatement stands in for the GPU's objective in the fp32 screen.

Measured on the CPU with the case list below (93 cases per precision: 11 horizons x 7 caps, 2 with the largest history, 14 exit
settings), as printed by test_screens_leave_out_at_most_one:

  fp64, 1e-14 relative noise on J and dJ/dU, 3 noisy solves: 0 cases left out; largest spread in U 3.1e-9 (7.7e-11 of max|U|, at nt = 65,
        history_size = 3, 12 iterations), against the tolerance of 1e-8 of max|U|.
  fp32, 3 permutations of the unknowns:                      0 cases left out; largest spread in U 1.6e-1 (3.9e-3 of max|U|) at nt = 256,
        history_size = 3, 12 iterations, then 6.3e-4 of max|U| at nt = 256, history_size = 1, and at most 2.3e-4 of max|U| elsewhere.

Each of E = 1, 2, 4, 8, 16 has a case whose ring of 3 pairs has wrapped (12 iterations, 11 pairs) in both precisions."""
import pytest
import torch

import util_quad_sweep as qs
from neuraloc_amd.baseline_quad import MAX_HISTORY, MAX_NT, REASONS

CASES = qs.cases()


class _Screens(dict):
    """{(case id, double): Screened}, each computed when first asked for"""

    def __missing__(self, key):
        c = next(c for c in CASES if qs.case_id(c) == key[0])
        z0, U0 = qs.case_start(c, torch.float64 if key[1] else torch.float32)
        self[key] = qs.screen64(z0, U0, c.settings) if key[1] else qs.screen32_cpu(z0, U0, c.settings)
        return self[key]


@pytest.fixture(scope="module")
def screens():
    return _Screens()


def test_dispatch_rule_and_horizons():
    """lbfgs_E is the table of the host's per_lane rule, and the horizons stand on both sides of each of its boundaries"""
    table = {1: (1, 16), 2: (17, 32), 4: (33, 64), 8: (65, 128), 16: (129, 256)}
    for nt in range(1, MAX_NT + 1):
        E = qs.lbfgs_E(nt)
        assert table[E][0] <= nt <= table[E][1], (nt, E)
        assert 64 * E >= 4 * nt and (E == 1 or 64 * (E // 2) < 4 * nt)       # the smallest build that holds 4 nt elements
    with pytest.raises(ValueError):
        qs.lbfgs_E(MAX_NT + 1)
    for E, (lo, hi) in table.items():
        assert lo in qs.HORIZONS and hi in qs.HORIZONS, (E, lo, hi)
    assert {qs.lbfgs_E(nt) for nt in qs.HORIZONS} == set(qs.BUILDS)
    tails = {nt: 4 * nt % 64 for nt in qs.HORIZONS}
    assert [nt for nt, r in tails.items() if 4 * nt < 64] == [1, 4]
    assert [nt for nt, r in tails.items() if r == 0] == [16, 32, 64, 128, 256]
    assert [nt for nt, r in tails.items() if r and 4 * nt > 64] == [17, 33, 65, 129]


def test_case_list():
    ids = [qs.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    print("\n".join(f"{i}  E={qs.lbfgs_E(c.nt)}  {c.settings}" for i, c in zip(ids, CASES)))
    for nt in qs.HORIZONS:
        mine = [c.settings for c in CASES if c.nt == nt and c.want_reason is None and c.settings["history_size"] != MAX_HISTORY]
        for mi in (1, 2, 3, 5):
            assert dict(qs.REF_SETTINGS, max_iter=mi) in mine
        assert dict(qs.REF_SETTINGS, max_iter=12, history_size=3) in mine and dict(qs.REF_SETTINGS, max_iter=12, history_size=1) in mine
        assert dict(qs.REF_SETTINGS, max_iter=16000, max_eval=7) in mine
    big = [c.nt for c in CASES if c.settings["history_size"] == MAX_HISTORY]
    assert sorted(big) == [64, 256] and all(c.settings["max_iter"] == 5 for c in CASES if c.settings["history_size"] == MAX_HISTORY)
    reasons = {(c.nt, c.want_reason) for c in CASES if c.want_reason is not None}
    assert reasons == {(nt, r) for nt in qs.REASON_HORIZONS for r in REASONS if r != 0}
    a, b = (qs.lbfgs_E(nt) for nt in qs.REASON_HORIZONS)
    assert a <= qs.PF_E < b                                     # one prefetch build, and the one without
    z0, U0 = qs.start(33)
    assert torch.equal(z0, torch.tensor([-1.5, -1.5, -1.5] + [0.] * 9))
    assert torch.equal(U0, 1e-2 * torch.randn(33, 4, generator=torch.Generator().manual_seed(33)))
    assert torch.equal(qs.start(33, torch.float64)[1], U0.double())


def test_reference_is_the_fp64_restatement():
    """torch_lbfgs on objective64 gives the bits of test_baseline_f64_gpu._restated_lbfgs, the fp64 reference the project already has"""
    import test_baseline_f64_gpu as f64
    z0, U0 = qs.start(17, torch.float64)
    kw = dict(qs.REF_SETTINGS, **qs.WRAP_CAP)
    it, ev, U = f64._restated_lbfgs(z0, U0, **kw)
    sol = qs.torch_lbfgs(qs.objective64(z0), U0, **kw)
    assert (sol.n_iter, sol.n_evals) == (it, ev) and torch.equal(sol.U, U)
    assert qs.REL_LBFGS == f64.REL_LBFGS and qs.REF_SETTINGS == f64.REF_SETTINGS


def test_batched_stand_in_has_independent_rows():
    """the fp32 stand-in evaluated side by side: a row's bits depend neither on its place in the batch nor on the other rows, and are
    those of the unbatched call; the permuted solve un-permutes exactly"""
    z0, U0 = qs.start(65)
    J1, g1 = qs.objective32(z0)(U0)
    other = qs.start(65)[1].flip(0) * 3
    J, g = qs.objective32_batched(z0)(torch.stack([U0, other, U0, U0]))
    for r in (0, 2, 3):
        assert torch.equal(J[r], J1) and torch.equal(g[r], g1)
    seen = []
    perm = qs._perm(U0.numel(), 0)

    def fun(U):
        seen.append(U.clone())
        return qs.objective32(z0)(U)
    qs.torch_lbfgs(fun, U0, perm=perm, **dict(qs.REF_SETTINGS, max_iter=1))
    assert torch.equal(seen[0], U0) and not torch.equal(perm, torch.arange(U0.numel()))


def test_screens_leave_out_at_most_one(screens):
    """both screens over the final case list; the figures of this file's docstring and of DESIGN section 3.7 are this test's output"""
    for double in (True, False):
        left, worst, worst_rel, worst_id = [], 0.0, 0.0, None
        for c in CASES:
            s = screens[qs.case_id(c), double]
            scale = float(s.ref.U.abs().max())
            print(f"{'fp64' if double else 'fp32'} {qs.case_id(c):44s} E={qs.lbfgs_E(c.nt):2d} counts {s.counts[0]} exit {s.ref.reason} pairs "
                  f"{s.ref.pairs:3d}{' wrapped' if qs.wrapped(s.ref, c.settings) else ''}  spread {s.spread:.3e} ({s.spread / scale:.1e} of max|U|)"
                  f"{'' if s.ok else '  LEFT OUT: counts ' + str(s.counts)}")
            if not s.ok:
                left.append(qs.case_id(c))
            elif s.spread > worst:
                worst, worst_rel, worst_id = s.spread, s.spread / scale, qs.case_id(c)
        print(f"{'fp64' if double else 'fp32'}: {len(CASES)} cases, {len(left)} left out {left}; largest spread in U {worst:.3e} ({worst_rel:.1e} of "
              f"max|U|) at {worst_id}")
        assert len(left) <= qs.MAX_LEFT_OUT, left
        if double:                                              # the noise must stay far inside the fp64 tolerance for the screen to mean anything
            assert worst_rel <= 0.1 * qs.REL_LBFGS, (worst_id, worst_rel)


def test_every_build_has_a_wrapped_case(screens):
    for double in (True, False):
        have = {qs.lbfgs_E(c.nt) for c in CASES if screens[qs.case_id(c), double].ok and qs.wrapped(screens[qs.case_id(c), double].ref, c.settings)
                and c.settings["history_size"] == 3}
        assert have == set(qs.BUILDS), (double, have)
        for c in CASES:                                         # head = (pairs stored - ring) mod ring != 0 at the last direction
            s = screens[qs.case_id(c), double]
            if c.settings == dict(qs.REF_SETTINGS, **qs.WRAP_CAP) and s.ok and s.ref.n_iter == 12:
                assert (s.ref.n_iter - 1 - 3) % 3 != 0


def test_expected_reason_on_each_setting(screens):
    """each exit of torch.optim.LBFGS on its setting, at a prefetch horizon and at E = 16, in fp64 (where the settings were found)"""
    for c in CASES:
        if c.want_reason is not None:
            s64, s32 = screens[qs.case_id(c), True], screens[qs.case_id(c), False]
            print(f"{qs.case_id(c)}: fp64 exit {s64.ref.reason} ({REASONS[s64.ref.reason]}) after {s64.counts[0]}; fp32 stand-in {s32.ref.reason}")
            assert s64.ok and s64.ref.reason == c.want_reason, (qs.case_id(c), s64.ref.reason, s64.counts)
    c1 = next(c for c in CASES if c.want_reason == 1)
    assert screens[qs.case_id(c1), True].counts[0] == (0, 1)
    c2 = next(c for c in CASES if c.want_reason == 2)
    assert screens[qs.case_id(c2), True].counts[0] == (1, 1)


@pytest.mark.parametrize("nt", (17, 129))
def test_comparator_rejects_wrong_restatements(screens, nt):
    """on the wrapping case of a ragged horizon (E = 2 with prefetch, E = 16 without): one pair fewer in the ring, one evaluation more
    allowed, and a tail slot whose gradient never arrives all fail the rule, in both precisions; a self-agreeing solve passes it"""
    wrap = next(c for c in CASES if c.nt == nt and c.settings == dict(qs.REF_SETTINGS, **qs.WRAP_CAP))
    for double in (True, False):
        dt = torch.float64 if double else torch.float32
        z0, U0 = qs.case_start(wrap, dt)
        fun = qs.objective64(z0) if double else qs.objective32(z0)
        s = screens[qs.case_id(wrap), double]
        assert s.ok and qs.wrapped(s.ref, wrap.settings)
        tol = qs.tolerance(double, s.ref.U, s.spread)

        def verdict(sol, ref=s.ref, tol=tol):
            return qs.compare_solve(sol.U, (sol.n_iter, sol.n_evals), ref, tol)

        assert verdict(s.ref)[0]
        good = qs.torch_lbfgs(qs.noisy(fun, 5) if double else fun, U0, perm=None if double else qs._perm(U0.numel(), 7), **wrap.settings)
        assert verdict(good)[0], verdict(good)
        short = qs.torch_lbfgs(fun, U0, **dict(wrap.settings, history_size=2))
        dead = qs.torch_lbfgs(qs.dead_tail(fun, nt), U0, **wrap.settings)
        for name, sol in (("history_size - 1", short), ("dead tail slot", dead)):
            ok, err, why = verdict(sol)
            print(f"nt={nt} {'fp64' if double else 'fp32'} {name}: {why} (tol {tol:.3e})")
            assert not ok, name
        # the evaluation cap on the same wrapping solve, set to the evaluations its first 8 iterations take: the reference ends there with
        # exit 4, a solve allowed one evaluation more goes on into iteration 9
        base = qs.torch_lbfgs(fun, U0, **dict(wrap.settings, max_iter=8))
        capped = dict(wrap.settings, max_iter=16000, max_eval=base.n_evals)
        ref = qs.torch_lbfgs(fun, U0, **capped)
        assert ref.reason == 4 and (ref.n_iter, ref.n_evals) == (8, base.n_evals) and torch.equal(ref.U, base.U)
        more = qs.torch_lbfgs(fun, U0, **dict(capped, max_eval=base.n_evals + 1))
        ok, err, why = verdict(more, ref, qs.tolerance(double, ref.U, s.spread))
        print(f"nt={nt} {'fp64' if double else 'fp32'} max_eval + 1: {why}")
        assert not ok


def test_limits_match_the_package():
    assert max(qs.HORIZONS) == MAX_NT and qs.BIG_HISTORY["history_size"] == MAX_HISTORY
    assert qs.TOL_FACTOR == 4.0 and qs.REL32 == 1e-4 and qs.REL_LBFGS == 1e-8
