"""GPU: time-correlated (Ornstein-Uhlenbeck) noise drawn inside the rollout kernels.  Every check is an equality:
the fill kernel against the float32 recursion in numpy over two white fills; the <noise-corr> instantiation of every kernel family against
the <dist> instantiation on the filled tensor (evaluation, intermediates, training with its gradients); rho = 0.0 against rho = None; a row
of a ragged batch against that row alone; noise_study in two chunks against one; the risk route against given weights on the tensor; guard
bands around every output buffer of the three new C entries.  Shapes: tests/util_noise_corr.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, noise, train
import util_disturb as ud
import util_mono as um
import util_noise_corr as uc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SEED = 0xDEADBEEFCAFEF00D
ROW0 = 2 ** 32 + 7                                                   # row keys with a high word


def last_kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def sigma_of(case):
    return ud.SIGMA_REL * case.rad * (1.0 + 0.25 * torch.arange(case.d, dtype=torch.float64) / case.d)


def rho_of(case):
    return torch.from_numpy(uc.rho_of(case)).float()


def mask_of(case):
    return (torch.arange(case.d) % 5 != 2).long()


_STARTS = {}


def starts(case, n=None):
    n = n or case.n
    if (case, n) not in _STARTS:
        _STARTS[(case, n)] = um.candidates(case, n).contiguous()
    return _STARTS[(case, n)].to(DEV)


def _specialised_or_skip(family, kernel):
    """the only admissible skip: the shape-specialised per-tile instantiation when the library at hand runs this shape on the generic one"""
    if family == "tile-fixed" and kernel == uc.KERNEL["tile"]:
        pytest.skip("this library has no shape-specialised build of swarm50's shape (NOCF_FIXED=0 or a per-shape build): the generic case ran")
    assert kernel == uc.KERNEL[family], kernel


# ---------------------------------------------------------------- 1. the fill
def _white_fill(nt, n, d, scale, seed, row0):
    W = torch.empty(nt, n, d, device=DEV)
    _, f = noise._entry_for(_lib.lib(), "nocf_noise_fill_f32", "test")
    with torch.cuda.device(DEV):
        rc = f(_lib.ptr(W), n, nt, d, _lib.ptr(scale.to(DEV)), seed, row0, _lib.stream_ptr(torch.device(DEV)))
    assert rc == 0
    return W


@pytest.mark.parametrize("shape", [(4, 257, 7), (3, 2, 150), (1, 5, 4)], ids=str)
def test_fill_is_the_float32_recursion_over_two_white_fills(shape):
    """step 0 from counter_disturbances (scale s0), steps k >= 1 from the white fill with the table s1; d no multiple of the block size, n of
    one block of (row, i) threads plus one, row keys above 2^32, a per-component rho and a mask"""
    nt, n, d = shape
    tspan = (0.25, 1.0)
    sigma = 0.3 * (1.0 + torch.arange(d, dtype=torch.float64) / d)
    rho = 0.05 + 0.9 * torch.arange(d, dtype=torch.float32) / d
    mask = (torch.arange(d) % 3 != 1).long()
    s0, s1, r = na.noise_corr_scales(sigma, rho, nt, d, tspan, mask)
    got = na.counter_disturbances(nt, n, d, sigma, SEED, tspan=tspan, mask=mask, row_offset=ROW0, device=DEV, rho=rho)
    A = na.counter_disturbances(nt, n, d, sigma, SEED, tspan=tspan, mask=mask, row_offset=ROW0, device=DEV)
    B = _white_fill(nt, n, d, s1, SEED, ROW0)
    torch.cuda.synchronize()
    ref = torch.from_numpy(uc.recursion(A.cpu().numpy(), B.cpu().numpy(), r.numpy()))
    assert torch.equal(got.cpu(), ref)
    assert bool((got[:, :, mask.to(DEV) == 0] == 0).all()) and bool((got[:, :, mask.to(DEV) != 0] != 0).all())
    if nt > 1:
        assert not torch.equal(got, A)                               # (the path is not the white tensor)
    # the path of a row does not depend on the batch it is filled in
    part = na.counter_disturbances(nt, 1, d, sigma, SEED, tspan=tspan, mask=mask, row_offset=ROW0 + n - 1, device=DEV, rho=rho)
    assert torch.equal(part[:, 0], got[:, n - 1])


def test_fill_at_rho_zero_is_the_white_tensor():
    sig = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    for rho in (0.0, torch.zeros(6)):
        a = na.counter_disturbances(4, 33, 6, sig, SEED, mask=[1, 1, 0, 1, 1, 1], row_offset=ROW0, device=DEV, rho=rho)
        b = na.counter_disturbances(4, 33, 6, sig, SEED, mask=[1, 1, 0, 1, 1, 1], row_offset=ROW0, device=DEV)
        assert torch.equal(a, b)
    # a prefix in nt stays a prefix (the same step h): nt = 5 on [0, 1] and nt = 3 on [0, 0.6]
    a5 = na.counter_disturbances(5, 9, 6, sig, 11, tspan=(0.0, 1.0), device=DEV, rho=0.7)
    a3 = na.counter_disturbances(3, 9, 6, sig, 11, tspan=(0.0, 0.6), device=DEV, rho=0.7)
    assert torch.equal(a5[:3], a3)


# ---------------------------------------------------------------- 2. the mode in the kernels
def _noise_kw(case, masked=True):
    return dict(tspan=case.tspan, mask=mask_of(case) if masked else None)


def _pair(case, x, intermediates, rho):
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    kw = dict(tspan=case.tspan, alph=case.alph, stepper=case.stepper, intermediates=intermediates)
    with torch.no_grad():
        a = na.noisy_rollout(x, net, prob, case.nt, sigma_of(case), SEED, row_offset=ROW0, mask=mask_of(case), rho=rho, **kw)
        ka = last_kernel()
        W = na.counter_disturbances(case.nt, x.shape[0], case.d, sigma_of(case), SEED, row_offset=ROW0, device=DEV, rho=rho, **_noise_kw(case))
        b = na.disturbed_rollout(x, net, prob, case.nt, W, **kw)
        kb = last_kernel()
    torch.cuda.synchronize()
    return a, b, ka, kb, W


def _assert_same(a, b, keys):
    for k in keys:
        if k == "cs":
            assert all(torch.equal(p, q) for p, q in zip(a[k], b[k])), k
        else:
            assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))
        assert not bool(torch.isnan(a[k] if k != "cs" else torch.stack(list(a[k]))).any()), k


@pytest.mark.parametrize("fc", uc.CASES, ids=uc.case_id)
def test_noisy_rollout_is_the_disturbed_rollout_on_the_filled_tensor(fc):
    family, case = fc
    assert case.n == uc.TILE[family] + 1 and case.nt == 3
    x = starts(case)
    for intermediates in (True, False):
        a, b, ka, kb, W = _pair(case, x, intermediates, rho_of(case))
        _specialised_or_skip(family, ka)
        assert kb == ud.KERNEL[family], kb
        _assert_same(a, b, ("persample", "z_final", "Jc", "cs") + (("traj", "ctrl") if intermediates else ()))
    white = na.counter_disturbances(case.nt, case.n, case.d, sigma_of(case), SEED, row_offset=ROW0, device=DEV, **_noise_kw(case))
    assert float(W.abs().max()) > 0 and not torch.equal(W, white) and torch.equal(W[0], white[0])


# ---------------------------------------------------------------- 3. training
def _train(case, x, fn):
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    xx = x.clone().requires_grad_(True)
    out = fn(xx, net, prob)
    Jc, cs = out[0], out[1]
    kf = last_kernel()
    Jc.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    got["x"] = xx.grad.clone()
    return Jc.detach(), torch.stack(list(cs)).detach(), got, kf, out


@pytest.mark.parametrize("fc", uc.FAMILY_FIRST, ids=uc.case_id)
def test_training_is_disturbed_training_on_the_filled_tensor(fc):
    """the recording forward leaves the same record, and the adjoint is unchanged code on it: the value, every parameter gradient and x.grad
    are equal (two tiles: the adjoint's two partial sums meet in one commutative addition)"""
    family, case = fc
    x = starts(case)
    sig, rho, ts = sigma_of(case), rho_of(case), list(case.tspan)
    W = na.counter_disturbances(case.nt, case.n, case.d, sig, SEED, row_offset=ROW0, device=DEV, rho=rho, **_noise_kw(case))
    dist = lambda xx, net, prob: na.disturbed_ocflow_train(xx, net, prob, ts, case.nt, W, case.stepper, case.alph)          # noqa: E731
    nois = lambda xx, net, prob: na.noisy_ocflow_train(xx, net, prob, ts, case.nt, sig, SEED, case.stepper, case.alph,      # noqa: E731
                                                       mask=mask_of(case), row_offset=ROW0, rho=rho)
    J1, c1, g1, k1, _ = _train(case, x, dist)
    J3, c3, g3, k3, _ = _train(case, x, nois)
    _specialised_or_skip(family, k3)
    assert k1 == ud.KERNEL[family], k1
    assert torch.equal(J1, J3) and torch.equal(c1, c3)
    for k in g1:
        print(case.id, k, "noisy - disturbed", float((g3[k] - g1[k]).abs().max()))
        assert bool(torch.isfinite(g3[k]).all()) and float(g3[k].abs().max()) > 0
        assert torch.equal(g3[k], g1[k]), k


# ---------------------------------------------------------------- 4. rho = 0.0 against rho = None
@pytest.mark.parametrize("fc", uc.FAMILY_FIRST, ids=uc.case_id)
def test_rho_zero_is_the_white_path(fc):
    family, case = fc
    x = starts(case)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    sig, ts = sigma_of(case), list(case.tspan)
    kw = dict(tspan=case.tspan, alph=case.alph, stepper=case.stepper, mask=mask_of(case), row_offset=ROW0)
    for intermediates in (True, False):
        with torch.no_grad():
            a = na.noisy_rollout(x, net, prob, case.nt, sig, SEED, intermediates=intermediates, rho=0.0, **kw)
            ka = last_kernel()
            b = na.noisy_rollout(x, net, prob, case.nt, sig, SEED, intermediates=intermediates, **kw)
            kb = last_kernel()
        _specialised_or_skip(family, ka)
        assert kb == ka.replace("noise-corr", "noise")
        _assert_same(a, b, ("persample", "z_final", "Jc", "cs") + (("traj", "ctrl") if intermediates else ()))
    corr = lambda xx, net, prob: na.noisy_ocflow_train(xx, net, prob, ts, case.nt, sig, SEED, case.stepper, case.alph,      # noqa: E731
                                                       mask=mask_of(case), row_offset=ROW0, rho=0.0)
    whit = lambda xx, net, prob: na.noisy_ocflow_train(xx, net, prob, ts, case.nt, sig, SEED, case.stepper, case.alph,      # noqa: E731
                                                       mask=mask_of(case), row_offset=ROW0)
    J1, c1, g1, k1, _ = _train(case, x, corr)
    J2, c2, g2, k2, _ = _train(case, x, whit)
    assert k1 == uc.KERNEL[family] and k2 == k1.replace("noise-corr", "noise")
    assert torch.equal(J1, J2) and torch.equal(c1, c2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


# ---------------------------------------------------------------- 5. rows are independent
@pytest.mark.parametrize("fc", uc.FAMILY_FIRST, ids=uc.case_id)
def test_a_row_of_a_ragged_batch_is_that_row_alone(fc):
    """n = tile + 3: the last tile holds three rows, and the per-tile and one-CU kernels fill it up with copies of row n - 1.  The copies
    must neither advance nor disturb a real row's carried state: every row equals the same row rolled out alone under its row_offset"""
    family, case = fc
    n = uc.TILE[family] + 3
    x = starts(case, n)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    kw = dict(tspan=case.tspan, alph=case.alph, stepper=case.stepper, mask=mask_of(case), rho=rho_of(case), intermediates=True)
    with torch.no_grad():
        whole = na.noisy_rollout(x, net, prob, case.nt, sigma_of(case), SEED, row_offset=ROW0, **kw)
        _specialised_or_skip(family, last_kernel())
        for j in (0, uc.TILE[family] - 1, uc.TILE[family], n - 1):   # first tile's ends, the ragged tile's ends
            one = na.noisy_rollout(x[j:j + 1].contiguous(), net, prob, case.nt, sigma_of(case), SEED, row_offset=ROW0 + j, **kw)
            for k in ("persample", "z_final", "traj", "ctrl"):
                assert torch.equal(one[k][0], whole[k][j]), (j, k)
        wrong = na.noisy_rollout(x[n - 1:].contiguous(), net, prob, case.nt, sigma_of(case), SEED, row_offset=ROW0, **kw)
    assert not torch.equal(wrong["z_final"][0], whole["z_final"][n - 1])         # (the offset is what ties a row to its path)


# ---------------------------------------------------------------- 6. noise_study
def test_noise_study_does_not_depend_on_the_chunking():
    family, case = uc.CASES[0]
    x = starts(case)[:3].contiguous()
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    paths, sigma, rho = 8, ud.SIGMA_REL * case.rad, rho_of(case)
    kw = dict(tspan=case.tspan, alph=case.alph, stepper=case.stepper)
    with torch.no_grad():
        two = na.noise_study(x, net, prob, case.nt, sigma, paths, rng="counter", seed=SEED, max_rows=2 * paths, rho=rho, **kw)
        assert last_kernel() == uc.KERNEL[family]
        one = na.noise_study(x, net, prob, case.nt, sigma, paths, rng="counter", seed=SEED, rho=rho, **kw)
        assert two["persample"].shape == (3, paths, 7) and torch.equal(two["persample"], one["persample"])
        for q in ("L+G", "G", "Q", "W"):
            for s in ("mean", "std", "q05", "q50", "q95"):
                assert torch.equal(two[q][s], one[q][s])
        ref = na.noisy_rollout(x.repeat_interleave(paths, 0).contiguous(), net, prob, case.nt, sigma, SEED, rho=rho, **kw)
        assert torch.equal(ref["persample"].view(3, paths, 7), one["persample"])
        white = na.noise_study(x, net, prob, case.nt, sigma, paths, rng="counter", seed=SEED, **kw)
        assert not torch.equal(white["persample"], one["persample"])
        # rng="torch" takes rho too (brownian_disturbances' recursion): finite, and not the white study of the same generator
        gen = lambda: torch.Generator(device=DEV).manual_seed(5)                          # noqa: E731
        t1 = na.noise_study(x, net, prob, case.nt, sigma, paths, generator=gen(), rho=0.9, **kw)
        t2 = na.noise_study(x, net, prob, case.nt, sigma, paths, generator=gen(), **kw)
        assert bool(torch.isfinite(t1["persample"]).all()) and not torch.equal(t1["persample"], t2["persample"])


# ---------------------------------------------------------------- 7. the risk route
@pytest.mark.parametrize("fc", [uc.CASES[0], uc.CASES[1]], ids=uc.case_id)
def test_risk_training_is_weighted_training_on_the_filled_tensor(fc):
    """CVaR over small groups of paths, rho given.  The gradients and the 7 means are weighted_ocflow_train's with the same weights on the
    filled tensor; the value is risk_ocflow_train's on that tensor (the same formula on an equal table: risk_weights' value and the weighted
    sum of the rows are two roundings of one number, so the weighted call's value is held to its own noise route instead)"""
    family, case = fc
    paths = 3
    x = starts(case, 2).repeat_interleave(paths, 0).contiguous()    # 6 rows: two starts of three paths, a full tile and a ragged one (lane)
    sig, rho, ts = sigma_of(case).float(), rho_of(case), list(case.tspan)       # (the risk calls refuse a float64 sigma tensor)
    kw = dict(stepper=case.stepper, alph=case.alph)
    risk = lambda xx, net, prob: na.risk_ocflow_train(xx, net, prob, ts, case.nt, "cvar", 0.5, paths=paths, sigma=sig, seed=SEED,  # noqa: E731
                                                      mask=mask_of(case), row_offset=ROW0, rho=rho, **kw)
    J1, c1, g1, k1, out = _train(case, x, risk)
    assert k1 == uc.KERNEL[family], k1
    w = out[2]["weights"]
    assert w.shape == (x.shape[0],) and float(w.sum()) > 0
    W = na.counter_disturbances(case.nt, x.shape[0], case.d, sig, SEED, row_offset=ROW0, device=DEV, rho=rho, **_noise_kw(case))
    given = lambda xx, net, prob: na.weighted_ocflow_train(xx, net, prob, ts, case.nt, w, W=W, **kw)                          # noqa: E731
    J2, c2, g2, k2, _ = _train(case, x, given)
    assert k2 == ud.KERNEL[family], k2
    print(case.id, "risk value", float(J1), "weighted sum", float(J2))
    # (two float32 evaluations of one positive sum of 6 products: each within (rows + 2) half-ulps of it)
    assert torch.equal(c1, c2) and abs(float(J1) - float(J2)) <= 2 * (x.shape[0] + 2) * 2.0 ** -24 * abs(float(J2))
    for k in g1:
        assert float(g1[k].abs().max()) > 0 and torch.equal(g1[k], g2[k]), k
    onW = lambda xx, net, prob: na.risk_ocflow_train(xx, net, prob, ts, case.nt, "cvar", 0.5, paths=paths, W=W, **kw)         # noqa: E731
    J4, c4, g4, k4, out4 = _train(case, x, onW)
    assert torch.equal(J4, J1) and torch.equal(out4[2]["weights"], w) and torch.equal(out4[2]["persample"], out[2]["persample"])
    assert all(torch.equal(g4[k], g1[k]) for k in g1)
    # ... and weighted_ocflow_train's own sigma / seed / rho route
    own = lambda xx, net, prob: na.weighted_ocflow_train(xx, net, prob, ts, case.nt, w, sigma=sig, seed=SEED, mask=mask_of(case),  # noqa: E731
                                                         row_offset=ROW0, rho=rho, **kw)
    J3, c3, g3, k3, _ = _train(case, x, own)
    assert k3 == uc.KERNEL[family] and torch.equal(J3, J2) and all(torch.equal(g3[k], g2[k]) for k in g2)


# ---------------------------------------------------------------- 8. guard bands
def _banded(counts):
    bufs = [torch.full((c + 2 * GUARD,), float("nan"), device=DEV) for c in counts]
    return bufs, [C.c_void_p(b.data_ptr() + 4 * GUARD) for b in bufs]


def _bands_intact(bufs, counts):
    for b, c in zip(bufs, counts):
        assert bool(b[:GUARD].isnan().all()) and bool(b[GUARD + c:].isnan().all()) and not bool(b[GUARD:GUARD + c].isnan().any())


def test_fill_entry_writes_only_its_tensor():
    nt, n, d = 3, 33, 14
    s0, s1, r = (t.to(DEV) for t in na.noise_corr_scales(0.3, 0.6, nt, d))
    bufs, (w,) = _banded([nt * n * d])
    _, f = noise._entry_for(_lib.lib(), "nocf_noise_fill_corr_f32", "test")
    with torch.cuda.device(DEV):
        rc = f(w, n, nt, d, _lib.ptr(s0), _lib.ptr(s1), _lib.ptr(r), 5, 0, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    _bands_intact(bufs, [nt * n * d])
    assert torch.equal(bufs[0][GUARD:GUARD + nt * n * d].view(nt, n, d), na.counter_disturbances(nt, n, d, 0.3, 5, device=DEV, rho=0.6))


@pytest.mark.parametrize("fc", uc.FAMILY_FIRST, ids=uc.case_id)
def test_rollout_entries_write_only_their_rows(fc):
    family, case = fc
    x = starts(case)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    n, d, nt = case.n, case.d, case.nt
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(x.device)
    cdim = _lib.lib().nocf_ctrl_dim(C.byref(prob_st), d)
    s0, s1, r = (t.to(DEV) for t in na.noise_corr_scales(sigma_of(case), rho_of(case), nt, d, case.tspan, mask_of(case)))
    alph_c = (C.c_float * 6)(*case.alph)
    head = (C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), _lib.ptr(s0), _lib.ptr(s1), _lib.ptr(r), SEED, ROW0, n,
            float(case.tspan[0]), float(case.tspan[1]), nt, train._STEPPERS[case.stepper], alph_c)
    tail = (_lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_ptr(x.device))
    with torch.no_grad():
        ref = na.noisy_rollout(x, net, prob, nt, sigma_of(case), SEED, tspan=case.tspan, alph=case.alph, stepper=case.stepper,
                               intermediates=True, mask=mask_of(case), row_offset=ROW0, rho=rho_of(case))
    # the evaluation entry
    counts = [n * (d + 4), n * 7, (nt + 1) * n * (d + 4), (nt + 1) * n * cdim, 8, 8]
    bufs, (z, tab, zF, cF, sums, means) = _banded(counts)
    f = noise._entry(_lib.lib(), "nocf_rollout_noisy_corr_f32")
    with torch.cuda.device(x.device):
        rc = f(*head, z, tab, sums, means, zF, cF, *tail)
    torch.cuda.synchronize()
    assert rc == 0
    _specialised_or_skip(family, last_kernel())
    _bands_intact(bufs, counts)
    assert torch.equal(bufs[1][GUARD:GUARD + counts[1]].view(n, 7), ref["persample"])
    assert torch.equal(bufs[2][GUARD:GUARD + counts[2]].view(nt + 1, n, d + 4).permute(1, 2, 0), ref["traj"])
    # the recording entry
    E = nt * (4 if case.stepper == "rk4" else 1)
    nact = int(_lib.lib().nocf_activation_record_floats(d, case.m, case.nTh, n, nt, train._STEPPERS[case.stepper])) if family == "mono" else 0
    counts = [E * n * (d + 1), n * (d + 4), n * 7, 8] + ([nact] if nact else [])
    bufs, ptrs = _banded(counts)
    s_all, z, tab, sums = ptrs[:4]
    act = ptrs[4] if nact else None
    rec = C.c_int32(-1)
    f = noise._entry(_lib.lib(), "nocf_rollout_record_noisy_corr_f32")
    with torch.cuda.device(x.device):
        rc = f(*head, z, tab, sums, s_all, act, C.byref(rec), *tail)
    torch.cuda.synchronize()
    assert rc == 0 and last_kernel() == uc.KERNEL[family] and rec.value == (1 if nact else 0)
    _bands_intact(bufs, counts)
    # (against the call without intermediates: swarm50's shape accumulates its cost integrals in another order when no trajectory is asked for)
    with torch.no_grad():
        ref = na.noisy_rollout(x, net, prob, nt, sigma_of(case), SEED, tspan=case.tspan, alph=case.alph, stepper=case.stepper,
                               mask=mask_of(case), row_offset=ROW0, rho=rho_of(case))
    assert torch.equal(bufs[2][GUARD:GUARD + counts[2]].view(n, 7), ref["persample"])
    assert torch.equal(bufs[1][GUARD:GUARD + counts[1]].view(n, d + 4), ref["z_final"])


# ---------------------------------------------------------------- 9. the drivers
def _train_lines(capsys, tmp_path, name, *flags):
    import trainOC
    save = str(tmp_path / name)
    trainOC.main(["--data", "softcorridor", "--niters", "2", "--val_freq", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save,
                  "--seed", "1", "--lr", "0.02", "--noise", "0.1", "--noise_seed", "3", *flags])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln[:5].isdigit()]
    assert len(lines) == 2
    return [ln.split()[:2] + ln.split()[3:] for ln in lines]         # (column 2 is the wall time)


def test_trainOC_noise_rho(tmp_path, capsys):
    a = _train_lines(capsys, tmp_path, "a", "--noise_rng", "counter", "--noise_rho", "0.8")
    b = _train_lines(capsys, tmp_path, "b", "--noise_rng", "counter", "--noise_rho", "0.8")
    w = _train_lines(capsys, tmp_path, "w", "--noise_rng", "counter")
    z = _train_lines(capsys, tmp_path, "z", "--noise_rng", "counter", "--noise_rho", "0")
    t = _train_lines(capsys, tmp_path, "t", "--noise_rho", "0.8")
    r = _train_lines(capsys, tmp_path, "r", "--noise_rng", "counter", "--noise_rho", "0.8", "--risk", "cvar", "--risk_level", "0.5",
                     "--risk_paths", "2")
    assert a == b and w == z and a[0][2] != w[0][2] and a[0][2] != t[0][2] and a[0][2] != r[0][2]
    for run in (a, t, r):
        assert all(np.isfinite(float(v)) for ln in run for v in ln[2:]) and [len(ln) for ln in run] == [10, 18]


def test_evalOC_noise_rho(tmp_path, capsys):
    import argparse
    import os
    import evalOC
    from neuraloc_amd.checkpoint import save_checkpoint
    from conftest import load_golden
    g = load_golden("softcorridor")
    m = g.meta
    net = na.Phi(nTh=m["nTh"], m=m["m"], d=m["d"], alph=m["alph"])
    net.load_state_dict(g.state_dict())
    ck = str(tmp_path / "softcorridor_nn_checkpt.pth")
    save_checkpoint(ck, net, argparse.Namespace(data="softcorridor", m=m["m"], nTh=m["nTh"], alph=m["alph"], n_train=64, var0=1.0))
    nt = int(g["xinit_eval/nt"])
    outs = {}
    for name, flags in (("c1", ["--noise_rng", "counter", "--noise_rho", "0.8"]), ("c2", ["--noise_rng", "counter", "--noise_rho", "0.8"]),
                        ("w", ["--noise_rng", "counter"]), ("t", ["--noise_rho", "0.8"])):
        save = str(tmp_path / name)
        evalOC.main(["--resume", ck, "--nt", str(nt), "--save", save, "--batch", "16", "--noise", "0.1", "--noise_paths", "8",
                     "--noise_seed", "3", *flags])
        capsys.readouterr()
        z = np.load(os.path.join(save, "figs", "eval_softcorridor_nn_noise.npz"))
        assert z["persample"].shape == (1, 8, 7) and np.isfinite(z["persample"]).all()
        outs[name] = z["persample"]
    assert np.array_equal(outs["c1"], outs["c2"]) and not np.array_equal(outs["c1"], outs["w"]) and not np.array_equal(outs["t"], outs["w"])
