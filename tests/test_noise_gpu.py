"""GPU: Brownian disturbances drawn inside the rollout kernels.  The fill kernel against the float64 restatement
of tests/util_noise.py element by element; its invariances bitwise; the <noise> instantiation of every kernel family against the <dist>
instantiation on the filled tensor bitwise (evaluation and recording forward, all cases of util_disturb.CASES), which carries the parity of
the disturbed path over to the new mode without a second tolerance; invariance under cutting the batch; bounds; the drivers."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, noise, train
import util_disturb as ud
import util_mono as um
import util_noise as un

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64

# Relative error of the fill kernel against the float64 restatement: four times the largest error measured on the grid 64 x 1024 x 64
# (tools/noise_accuracy.py, profiles/noise/noise_accuracy.txt: MEASURED, at most 2^-20 by the specification); the margin covers inputs
# the grid did not visit.
MEASURED = 2.509111e-07                                              # = 2.1 * 2^-23, at (row 859, k 4, i 42)
TOL = 4.0 * MEASURED

KERNEL = {"lane": "rollout_lane_kernel<noise>", "mono": "rollout_mono_kernel<noise>", "tile": "rollout_kernel<generic, noise>",
          "tile-fixed": "rollout_kernel<shape-specialised, noise>"}
SEED = 0xDEADBEEFCAFEF00D
ROW0 = 2 ** 32 + 7


def last_kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def sigma_of(case):
    """per component, so that a swapped scale index shows"""
    return ud.SIGMA_REL * case.rad * (1.0 + 0.25 * torch.arange(case.d, dtype=torch.float64) / case.d)


_STARTS = {}


def starts(case, n=None):
    n = n or case.n
    if (case, n) not in _STARTS:
        _STARTS[(case, n)] = um.candidates(case, n).contiguous()
    return _STARTS[(case, n)].to(DEV)


# ---------------------------------------------------------------- 1. the fill against the restatement
@pytest.mark.parametrize("shape", [(3, 5, 4), (2, 33, 14), (2, 16, 150)], ids=str)
@pytest.mark.parametrize("row0", [0, ROW0])
@pytest.mark.parametrize("seed", [0, SEED])
def test_fill_against_the_restatement(shape, row0, seed):
    assert MEASURED < 2.0 ** -20
    nt, n, d = shape
    tspan = (0.25, 1.0)
    per = 0.3 * (1.0 + np.arange(d) / d)
    mask = (np.arange(d) % 3 != 1).astype(np.int64)
    for sigma, mk in ((0.7, None), (per, None), (per, mask)):
        sg = sigma if np.isscalar(sigma) else torch.from_numpy(sigma)
        W = na.counter_disturbances(nt, n, d, sg, seed, tspan=tspan, mask=None if mk is None else torch.from_numpy(mk),
                                    row_offset=row0, device=DEV)
        torch.cuda.synchronize()
        got = W.cpu().numpy().astype(np.float64)
        ref, sc, g = un.disturbances(seed, nt, n, d, sigma, tspan, mk, row0)
        bound = TOL * sc.astype(np.float64)[None, None, :] * np.maximum(np.abs(g), 1e-3)
        err = np.abs(got - ref)
        print(shape, row0, hex(seed), "largest error / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
        if mk is not None:
            assert (got[:, :, mk == 0] == 0.0).all() and (got[:, :, mk != 0] != 0.0).all()


# ---------------------------------------------------------------- 2. the fill's invariances
def test_fill_invariances_bitwise():
    sig = torch.tensor([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    full = na.counter_disturbances(3, 33, 6, sig, SEED, row_offset=ROW0, device=DEV)
    part = na.counter_disturbances(3, 5, 6, sig, SEED, row_offset=ROW0 + 7, device=DEV)
    assert torch.equal(full[:, 7:12], part)
    # a prefix in nt stays a prefix at the same scale: nt = 5 on [0, 1] and nt = 3 on [0, 0.6] have the step 0.2
    a5 = na.counter_disturbances(5, 9, 6, sig, 11, tspan=(0.0, 1.0), device=DEV)
    a3 = na.counter_disturbances(3, 9, 6, sig, 11, tspan=(0.0, 0.6), device=DEV)
    assert np.array_equal(un.scale_of(sig.numpy(), 6, 5, (0.0, 1.0)), un.scale_of(sig.numpy(), 6, 3, (0.0, 0.6)))
    assert torch.equal(a5[:3], a3)
    again = na.counter_disturbances(5, 9, 6, sig, 11, device=DEV)
    other = na.counter_disturbances(5, 9, 6, sig, 12, device=DEV)
    assert torch.equal(a5, again) and not torch.equal(a5, other)
    assert float((a5 == other).float().mean()) < 0.01
    # guard floats in front of and behind W stay NaN
    nt, n, d = 2, 33, 14
    buf = torch.full((nt * n * d + 2 * GUARD,), float("nan"), device=DEV)
    scale = noise.noise_scale(0.3, nt, d).to(DEV)
    L, f = noise._entry_for(_lib.lib(), "nocf_noise_fill_f32", "test")
    with torch.cuda.device(DEV):
        rc = f(C.c_void_p(buf.data_ptr() + 4 * GUARD), n, nt, d, _lib.ptr(scale), 5, 0, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == 0
    mid = buf[GUARD:GUARD + nt * n * d]
    assert bool(buf[:GUARD].isnan().all()) and bool(buf[GUARD + nt * n * d:].isnan().all()) and bool(torch.isfinite(mid).all())
    assert torch.equal(mid.view(nt, n, d), na.counter_disturbances(nt, n, d, 0.3, 5, device=DEV))


# ---------------------------------------------------------------- 3. the mode in the kernels
def _pair(case, x, sigma, seed, row0, intermediates):
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    kw = dict(tspan=case.tspan, alph=case.alph, stepper=case.stepper, intermediates=intermediates)
    with torch.no_grad():
        a = na.noisy_rollout(x, net, prob, case.nt, sigma, seed, row_offset=row0, **kw)
        ka = last_kernel()
        W = na.counter_disturbances(case.nt, x.shape[0], case.d, sigma, seed, tspan=case.tspan, row_offset=row0, device=DEV)
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


@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
def test_noisy_rollout_is_the_disturbed_rollout_on_the_filled_tensor_bitwise(fc):
    family, case = fc
    x = starts(case)
    for intermediates in (True, False):
        a, b, ka, kb, W = _pair(case, x, sigma_of(case), SEED, ROW0, intermediates)
        assert ka == KERNEL[family] and kb == ud.KERNEL[family], (ka, kb)
        _assert_same(a, b, ("persample", "z_final", "Jc", "cs") + (("traj", "ctrl") if intermediates else ()))
    # the noise arrives: the terminal state is not the undisturbed one
    z0 = _pair(case, x, 0.0, SEED, ROW0, False)
    assert float(W.abs().max()) > 0 and not torch.equal(a["z_final"], z0[0]["z_final"])
    # sigma = 0 is the disturbed call on a zero W
    assert z0[2] == KERNEL[family] and float(z0[4].abs().max()) == 0.0
    _assert_same(z0[0], z0[1], ("persample", "z_final", "Jc", "cs"))


# ---------------------------------------------------------------- 4. the recording forward and training
def _record(case, x, family, W=None, scale=None, seed=0, row0=0):
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    n, d, nt, m = x.shape[0], case.d, case.nt, case.m
    E = nt * (4 if case.stepper == "rk4" else 1)
    L = _lib.lib()
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(x.device)
    nan = float("nan")
    bufs = [torch.full((c + 2 * GUARD,), nan, device=DEV) for c in (E * n * (d + 1), n * (d + 4), n * 7)]
    s_all, z, tab = (b[GUARD:b.numel() - GUARD] for b in bufs)
    sums = torch.full((8,), nan, device=DEV)
    nact = int(L.nocf_activation_record_floats(d, m, case.nTh, n, nt, train._STEPPERS[case.stepper])) if family == "mono" else 0
    act = torch.full((nact,), nan, device=DEV) if nact else None
    rec = C.c_int32(-1)
    alph_c = (C.c_float * 6)(*case.alph)
    tail = (n, float(case.tspan[0]), float(case.tspan[1]), nt, train._STEPPERS[case.stepper], alph_c, _lib.ptr(z), _lib.ptr(tab),
            _lib.ptr(sums), _lib.ptr(s_all), _lib.ptr(act), C.byref(rec), _lib.ptr(ws), ws.numel() * ws.element_size(),
            _lib.stream_ptr(x.device))
    with torch.cuda.device(x.device):
        if W is None:
            rc = noise._entry(L, "nocf_rollout_record_noisy_f32")(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), _lib.ptr(scale), seed, row0, *tail)
        else:
            rc = train._disturbed_entry(L)(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), _lib.ptr(W), *tail)
    torch.cuda.synchronize()
    assert rc == 0
    for b, mid in zip(bufs, (s_all, z, tab)):                        # 6. bounds: only rows < n are written
        assert bool(b[:GUARD].isnan().all()) and bool(b[GUARD + mid.numel():].isnan().all()) and not bool(mid.isnan().any())
    return dict(s_all=s_all, z=z, tab=tab, sums=sums, act=act, rec=rec.value, kernel=last_kernel())


@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
def test_recording_forward_bitwise(fc):
    family, case = fc
    x = starts(case)
    sig = sigma_of(case)
    scale = noise.noise_scale(sig, case.nt, case.d, case.tspan).to(DEV)
    W = na.counter_disturbances(case.nt, case.n, case.d, sig, SEED, tspan=case.tspan, row_offset=ROW0, device=DEV)
    a = _record(case, x, family, scale=scale, seed=SEED, row0=ROW0)
    b = _record(case, x, family, W=W)
    assert a["kernel"] == KERNEL[family] and b["kernel"] == ud.KERNEL[family]
    assert a["rec"] == b["rec"] == (1 if a["act"] is not None else 0)
    for k in ("s_all", "z", "tab", "sums"):
        assert torch.equal(a[k], b[k]), k
    if a["act"] is not None:
        assert not bool(a["act"].isnan().any()) and torch.equal(a["act"], b["act"])


def _train(case, x, fn):
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    xx = x.clone().requires_grad_(True)
    Jc, cs = fn(xx, net, prob)
    kf = last_kernel()
    Jc.backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    got["x"] = xx.grad.clone()
    return Jc.detach(), torch.stack(list(cs)).detach(), got, kf


@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
def test_training_is_disturbed_training_on_the_filled_tensor(fc):
    """the adjoint is unchanged code on equal inputs: a gradient may differ from disturbed_ocflow_train's by no more than twice what two
    runs of disturbed_ocflow_train on the same W differ by from each other (atomics), and by nothing where those two are equal"""
    family, case = fc
    x = starts(case)
    sig = sigma_of(case)
    ts = list(case.tspan)
    W = na.counter_disturbances(case.nt, case.n, case.d, sig, SEED, tspan=case.tspan, row_offset=ROW0, device=DEV)
    dist = lambda xx, net, prob: na.disturbed_ocflow_train(xx, net, prob, ts, case.nt, W, case.stepper, case.alph)          # noqa: E731
    nois = lambda xx, net, prob: na.noisy_ocflow_train(xx, net, prob, ts, case.nt, sig, SEED, case.stepper, case.alph,      # noqa: E731
                                                       row_offset=ROW0)
    J1, c1, g1, k1 = _train(case, x, dist)
    J2, c2, g2, k2 = _train(case, x, dist)
    J3, c3, g3, k3 = _train(case, x, nois)
    assert k1 == ud.KERNEL[family] and k3 == KERNEL[family], (k1, k3)
    assert torch.equal(J1, J3) and torch.equal(c1, c3)
    for k in g1:
        spread = float((g1[k] - g2[k]).abs().max())
        diff = float((g3[k] - g1[k]).abs().max())
        print(case.id, k, "two disturbed runs differ by", spread, "noisy - disturbed", diff)
        assert bool(torch.isfinite(g3[k]).all()) and diff <= 2.0 * spread, (k, diff, spread)


# ---------------------------------------------------------------- 5. cutting the batch
CUTS = [(ud.CASES[1], 7, 3), (ud.CASES[3], 33, 16), (ud.CASES[5], 17, 9)]


@pytest.mark.parametrize("fc,n,cut", CUTS, ids=[ud.case_id(c[0]) for c in CUTS])
def test_rows_do_not_depend_on_how_the_batch_is_cut(fc, n, cut):
    family, case = fc
    x = starts(case, n)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    kw = dict(tspan=case.tspan, alph=case.alph, stepper=case.stepper)
    with torch.no_grad():
        whole = na.noisy_rollout(x, net, prob, case.nt, sigma_of(case), SEED, row_offset=ROW0, **kw)
        assert last_kernel() == KERNEL[family]
        parts = [na.noisy_rollout(x[a:b].contiguous(), net, prob, case.nt, sigma_of(case), SEED, row_offset=ROW0 + a, **kw)
                 for a, b in ((0, cut), (cut, n))]
        wrong = na.noisy_rollout(x[cut:].contiguous(), net, prob, case.nt, sigma_of(case), SEED, row_offset=ROW0, **kw)
    torch.cuda.synchronize()
    for k in ("persample", "z_final"):
        assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), k
    assert not torch.equal(wrong["z_final"], whole["z_final"][cut:])             # (the offset is what ties a row to its noise)


def test_noise_study_does_not_depend_on_the_chunking():
    family, case = ud.CASES[1]
    x = starts(case)[:3].contiguous()
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    paths, sigma = 8, ud.SIGMA_REL * case.rad
    kw = dict(tspan=case.tspan, alph=case.alph, stepper=case.stepper)
    with torch.no_grad():
        one = na.noise_study(x, net, prob, case.nt, sigma, paths, rng="counter", seed=SEED, max_rows=paths, **kw)
        assert last_kernel() == KERNEL[family]
        dflt = na.noise_study(x, net, prob, case.nt, sigma, paths, rng="counter", seed=SEED, **kw)
        assert one["persample"].shape == (3, paths, 7) and torch.equal(one["persample"], dflt["persample"])
        for q in ("L+G", "G", "Q", "W"):
            for s in ("mean", "std", "q05", "q50", "q95"):
                assert torch.equal(one[q][s], dflt[q][s])
        # start i, path p is global row i * paths + p
        ref = na.noisy_rollout(x.repeat_interleave(paths, 0).contiguous(), net, prob, case.nt, sigma, SEED, **kw)
        assert torch.equal(ref["persample"].view(3, paths, 7), dflt["persample"])
        # the reason the option exists: torch's generator is consumed chunk by chunk, so the same two calls differ
        gen = lambda: torch.Generator(device=DEV).manual_seed(5)                          # noqa: E731
        t1 = na.noise_study(x, net, prob, case.nt, sigma, paths, generator=gen(), max_rows=paths, **kw)
        t2 = na.noise_study(x, net, prob, case.nt, sigma, paths, generator=gen(), **kw)
        assert not torch.equal(t1["persample"], t2["persample"])


# ---------------------------------------------------------------- 6. bounds of the evaluation entry
@pytest.mark.parametrize("fc", [ud.CASES[1], ud.CASES[4], ud.CASES[5]], ids=ud.case_id)
def test_evaluation_entry_writes_only_its_rows(fc):
    family, case = fc
    x = starts(case)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    n, d, nt = case.n, case.d, case.nt
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(x.device)
    cdim = _lib.lib().nocf_ctrl_dim(C.byref(prob_st), d)
    counts = (n * (d + 4), n * 7, (nt + 1) * n * (d + 4), (nt + 1) * n * cdim)
    bufs = [torch.full((c + 2 * GUARD,), float("nan"), device=DEV) for c in counts]
    z, tab, zF, cF = (C.c_void_p(b.data_ptr() + 4 * GUARD) for b in bufs)
    sums, means = torch.empty(8, device=DEV), torch.empty(8, device=DEV)
    scale = noise.noise_scale(sigma_of(case), nt, d, case.tspan).to(DEV)
    alph_c = (C.c_float * 6)(*case.alph)
    f = noise._entry(_lib.lib(), "nocf_rollout_noisy_f32")
    with torch.cuda.device(x.device):
        rc = f(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), _lib.ptr(scale), SEED, ROW0, n, float(case.tspan[0]), float(case.tspan[1]), nt,
               train._STEPPERS[case.stepper], alph_c, z, tab, _lib.ptr(sums), _lib.ptr(means), zF, cF,
               _lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == 0 and last_kernel() == KERNEL[family]
    for b, c in zip(bufs, counts):
        assert bool(b[:GUARD].isnan().all()) and bool(b[GUARD + c:].isnan().all()) and not bool(b[GUARD:GUARD + c].isnan().any())
    with torch.no_grad():
        ref = na.noisy_rollout(x, net, prob, nt, sigma_of(case), SEED, tspan=case.tspan, alph=case.alph, stepper=case.stepper,
                               intermediates=True, row_offset=ROW0)
    assert torch.equal(bufs[1][GUARD:GUARD + counts[1]].view(n, 7), ref["persample"])
    assert torch.equal(bufs[2][GUARD:GUARD + counts[2]].view(nt + 1, n, d + 4).permute(1, 2, 0), ref["traj"])


# ---------------------------------------------------------------- 7. the drivers
def _train_lines(capsys, tmp_path, name, *flags):
    import trainOC
    save = os.path.join(str(tmp_path), name)
    trainOC.main(["--data", "softcorridor", "--niters", "2", "--val_freq", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save,
                  "--seed", "1", "--lr", "0.02", *flags])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln[:5].isdigit()]
    assert len(lines) == 2
    return [ln.split()[:2] + ln.split()[3:] for ln in lines]         # (column 2 is the wall time)


def test_trainOC_counter_noise(tmp_path, capsys):
    a = _train_lines(capsys, tmp_path, "a", "--noise", "0.1", "--noise_seed", "3", "--noise_rng", "counter")
    b = _train_lines(capsys, tmp_path, "b", "--noise", "0.1", "--noise_seed", "3", "--noise_rng", "counter")
    c = _train_lines(capsys, tmp_path, "c", "--noise", "0.1", "--noise_seed", "4", "--noise_rng", "counter")
    t = _train_lines(capsys, tmp_path, "t", "--noise", "0.1", "--noise_seed", "3")
    assert last_kernel().startswith("rollout_lane")
    assert a == b and a[0][2] != c[0][2] and a[0][2] != t[0][2]      # one seed: identical log lines; the loss follows the seed and the generator
    assert all(np.isfinite(float(v)) for ln in a for v in ln[2:])
    assert [len(ln) for ln in a] == [10, 18]


def test_evalOC_counter_noise(tmp_path, capsys):
    import evalOC
    from neuraloc_amd.checkpoint import save_checkpoint
    from conftest import load_golden
    g = load_golden("softcorridor")
    m = g.meta
    net = na.Phi(nTh=m["nTh"], m=m["m"], d=m["d"], alph=m["alph"])
    net.load_state_dict(g.state_dict())
    ck = os.path.join(str(tmp_path), "softcorridor_nn_checkpt.pth")
    save_checkpoint(ck, net, argparse.Namespace(data="softcorridor", m=m["m"], nTh=m["nTh"], alph=m["alph"], n_train=64, var0=1.0))
    nt = int(g["xinit_eval/nt"])
    outs = []
    for name in ("e1", "e2"):
        save = os.path.join(str(tmp_path), name)
        out = evalOC.main(["--resume", ck, "--nt", str(nt), "--save", save, "--batch", "16", "--noise", "0.1", "--noise_paths", "8",
                           "--noise_seed", "3", "--noise_rng", "counter"])
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("noise ")]
        assert [ln.split()[1] for ln in lines[1:]] == ["L+G", "G", "Q", "W"], lines
        z = np.load(os.path.join(save, "figs", "eval_softcorridor_nn_noise.npz"))
        assert z["persample"].shape == (1, 8, 7) and np.isfinite(z["persample"]).all() and int(z["seed"]) == 3
        assert out["noise"]["L+G"]["std"] > 0
        outs.append(z["persample"])
    assert np.array_equal(outs[0], outs[1])
