"""GPU: the disturbed rollout (nocf_rollout_disturbed_f32, neuraloc_amd.disturb) on every new kernel instantiation against the fp64
restatement of tests/util_disturb.py under util_oracle's rule; W = 0 against the undisturbed call bitwise; one nonzero step against two
chained existing rollouts; row independence in a 1027-row batch; the refusals; noise_study; the evalOC flag."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib
import util_disturb as ud
import util_lane as ul
import util_mono as um

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def last_kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def run(case, x, W, intermediates=True):
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    with torch.no_grad():
        out = na.disturbed_rollout(x.to(DEV), net, prob, case.nt, W.to(DEV), tspan=case.tspan, alph=case.alph, stepper=case.stepper,
                                   intermediates=intermediates)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
def test_against_fp64_on_every_instantiation(fc):
    family, case = fc
    data = ud.case_data(case)
    out = run(case, data["x"], data["W"])
    kern = last_kernel()
    assert kern == ud.KERNEL[family] and not kern.startswith("rollout_duo"), kern
    got = dict(table=out["persample"], z=out["z_final"], zFull=out["traj"], ctrlFull=out["ctrl"])
    res = ud.compare(got, data["r64"], data["r32"])
    for k, v in res.items():
        print(f"{case.id} {k}: err {v[1]:.3e} tol {v[2]:.3e} fp32 restatement {v[3]:.3e}")
    assert not ul.failures(res), ul.failures(res)
    # the means are the table's, and the run without intermediates returns the same table and final state
    tab = out["persample"].double().cpu()
    a = case.alph
    for c in range(7):
        assert abs(float(out["cs"][c]) - float(tab[:, c].mean())) <= 1e-5 * (abs(float(tab[:, c].mean())) + 1e-30) + 1e-30
    jc = tab[:, 0].mean() + a[0] * tab[:, 1].mean() + a[3] * tab[:, 2].mean() + a[4] * tab[:, 3].mean() + a[5] * tab[:, 4].mean()
    assert abs(float(out["Jc"]) - float(jc)) <= 1e-5 * abs(float(jc))
    plain = run(case, data["x"], data["W"], intermediates=False)
    assert last_kernel() == ud.KERNEL[family]
    assert "traj" not in plain
    got2 = dict(table=plain["persample"], z=plain["z_final"])
    assert not ul.failures(ud.compare(got2, data["r64"], data["r32"]))


FAMILY_CASES = [ud.CASES[1], ud.CASES[3], ud.CASES[4], ud.CASES[5], ud.CASES[7]]


@pytest.mark.parametrize("fc", FAMILY_CASES, ids=ud.case_id)
def test_zero_disturbance_equals_the_undisturbed_call_on_the_same_kernel(fc, monkeypatch):
    family, case = fc
    monkeypatch.setenv("NOCF_DUO", "0")                              # (the undisturbed m = 512 call then takes the per-tile kernel too)
    data = ud.case_data(case)
    x = data["x"].to(DEV)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    W = torch.zeros(case.nt, case.n, case.d, device=DEV)
    # like with like: the call without intermediates against noMean and the means, the call with them against the trajectories (the
    # per-tile kernel defers its cost side when no trajectory is kept, so the two kinds of call differ in the last bit with or without W)
    with torch.no_grad():
        plain = na.disturbed_rollout(x, net, prob, case.nt, W, tspan=case.tspan, alph=case.alph, stepper=case.stepper)
        out = na.disturbed_rollout(x, net, prob, case.nt, W, tspan=case.tspan, alph=case.alph, stepper=case.stepper, intermediates=True)
        k1 = last_kernel()
        Jc, cs = na.OCflow(x, net, prob, list(case.tspan), case.nt, case.stepper, case.alph, noMean=True)
        k2 = last_kernel()
        zF, cF = na.OCflow(x, net, prob, list(case.tspan), case.nt, case.stepper, case.alph, intermediates=True)
        Jm, csm = na.OCflow(x, net, prob, list(case.tspan), case.nt, case.stepper, case.alph)
    assert k1 == ud.KERNEL[family] and k1.replace("<dist>", "").replace(", dist>", ">") == k2, (k1, k2)
    tab = torch.cat(cs, 1)
    print(case.id, "max |table difference|", float((plain["persample"] - tab).abs().max()), "max |traj difference|", float((out["traj"] - zF).abs().max()))
    assert torch.equal(plain["persample"], tab)
    assert torch.equal(plain["z_final"][:, :case.d], zF[:, :case.d, -1])
    assert torch.equal(out["traj"], zF) and torch.equal(out["ctrl"], cF)
    assert torch.equal(out["z_final"], zF[:, :, -1])
    assert torch.equal(plain["Jc"], Jm) and all(torch.equal(a, b) for a, b in zip(plain["cs"], csm))


@pytest.mark.parametrize("fc", [ud.CASES[0], ud.CASES[3], ud.CASES[6]], ids=ud.case_id)
def test_one_nonzero_step_equals_two_chained_rollouts(fc):
    """independent of the restatement: the existing OCflow(intermediates=True) twice, the state displaced in between"""
    family, case = fc
    data = ud.case_data(case)
    x = data["x"].to(DEV)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    d, nt = case.d, case.nt
    t0, t1 = case.tspan
    h = (t1 - t0) / nt
    for k in range(nt):
        W = torch.zeros(nt, case.n, d, device=DEV)
        W[k] = 4.0 * data["W"][k].to(DEV)
        with torch.no_grad():
            out = na.disturbed_rollout(x, net, prob, nt, W, tspan=case.tspan, alph=case.alph, stepper=case.stepper, intermediates=True)
            ts = t0 + (k + 1) * h
            z1, c1 = na.OCflow(x, net, prob, [t0, ts], k + 1, case.stepper, case.alph, intermediates=True)
            want = torch.zeros_like(out["traj"])
            want[:, :, :k + 2] = z1
            want[:, :d, k + 1] += W[k]
            if k + 1 < nt:
                z2, c2 = na.OCflow(want[:, :d, k + 1].contiguous(), net, prob, [ts, t1], nt - k - 1, case.stepper, case.alph, intermediates=True)
                want[:, :, k + 2:] = z2[:, :, 1:]
                want[:, d:, k + 2:] += want[:, d:, k + 1:k + 2]
                assert ud.state_close(out["ctrl"][:, :, k + 2:].cpu(), c2[:, :, 1:].cpu())
            assert ud.state_close(out["ctrl"][:, :, 1:k + 1].cpu(), c1[:, :, 1:k + 1].cpu())
        assert ud.state_close(out["traj"].cpu(), want.cpu()), (case.id, k)
        assert ud.state_close(out["z_final"].cpu(), want[:, :, -1].cpu())


@pytest.mark.parametrize("fc", [ud.CASES[1], ud.CASES[3], ud.CASES[4]], ids=ud.case_id)
def test_a_row_of_a_large_batch_equals_the_row_alone_bitwise(fc):
    family, case = fc
    n = 1027
    x = um.candidates(case, n)
    W = ud.disturbances(case, n, seed_offset=1)
    big = run(case, x, W)
    assert last_kernel() == ud.KERNEL[family]
    for i in (0, 15, 16, 513, 1024, 1026):
        one = run(case, x[i:i + 1], W[:, i:i + 1].contiguous())
        assert torch.equal(one["persample"], big["persample"][i:i + 1]), i
        assert torch.equal(one["z_final"], big["z_final"][i:i + 1])
        assert torch.equal(one["traj"], big["traj"][i:i + 1]) and torch.equal(one["ctrl"], big["ctrl"][i:i + 1])
    # ... and the other rows' disturbances matter to them: a different W on row 1 changes row 1 only
    W2 = W.clone()
    W2[:, 1] = -W2[:, 1]
    big2 = run(case, x, W2)
    assert not torch.equal(big2["z_final"][1], big["z_final"][1])
    keep = torch.arange(n) != 1
    assert torch.equal(big2["z_final"][keep], big["z_final"][keep]) and torch.equal(big2["persample"][keep], big["persample"][keep])


def test_refusals_leave_the_outputs_untouched():
    import ctypes as C
    from neuraloc_amd import disturb
    case = ud.CASES[0][1]
    data = ud.case_data(case)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x, W = data["x"].to(DEV), data["W"].to(DEV)
    n, d, nt = case.n, case.d, case.nt
    # float64 tensors
    with pytest.raises(RuntimeError, match="single precision only"):
        na.disturbed_rollout(x.double(), net, prob, nt, W)
    with pytest.raises(RuntimeError, match="single precision only"):
        na.disturbed_rollout(x, net, prob, nt, W.double())
    # under autograd (the network's parameters, or x, require a gradient and grad mode is on): like noMean
    with pytest.raises(NotImplementedError):
        na.disturbed_rollout(x, net, prob, nt, W)
    for p_ in net.parameters():
        p_.requires_grad_(False)
    with pytest.raises(NotImplementedError):
        na.disturbed_rollout(x.clone().requires_grad_(True), net, prob, nt, W)
    assert torch.isfinite(na.disturbed_rollout(x, net, prob, nt, W)["Jc"])
    # shapes
    with pytest.raises(ValueError):
        na.disturbed_rollout(x, net, prob, nt, W[:-1])
    with pytest.raises(ValueError):
        na.disturbed_rollout(x, net, prob, nt, W[:, :-1])
    with pytest.raises(ValueError):
        na.disturbed_rollout(x, net, prob, 0, W)
    with pytest.raises(ValueError):
        na.disturbed_rollout(x, net, prob, nt, W, stepper="rk2")
    # the C entry point with real device buffers: every refusal leaves the sentinel-filled outputs as they were
    L = _lib.lib()
    f = disturb._entry(L)
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(x.device)
    SENT = 12345.0
    bufs = dict(z=torch.full((n, d + 4), SENT, device=DEV), tab=torch.full((n, 7), SENT, device=DEV), sums=torch.full((8,), SENT, device=DEV),
                means=torch.full((8,), SENT, device=DEV), zF=torch.full((nt + 1, n, d + 4), SENT, device=DEV),
                cF=torch.full((nt + 1, n, d), SENT, device=DEV))
    alph_c = (C.c_float * 6)(*case.alph)
    wsb = ws.numel() * ws.element_size()

    def call(xp=x, Wp=W, n_=n, nt_=nt, stp=4, sums=True, cF=True, wsb_=wsb):
        return f(C.byref(phi_st), C.byref(prob_st), _lib.ptr(xp), _lib.ptr(Wp), n_, 0.0, 1.0, nt_, stp, alph_c,
                 _lib.ptr(bufs["z"]), _lib.ptr(bufs["tab"]), _lib.ptr(bufs["sums"]) if sums else None, _lib.ptr(bufs["means"]),
                 _lib.ptr(bufs["zF"]), _lib.ptr(bufs["cF"]) if cF else None, _lib.ptr(ws), wsb_, _lib.stream_ptr(x.device))

    with torch.cuda.device(x.device):
        assert call(Wp=None) == -1
        assert call(xp=None) == -1
        assert call(sums=False) == -1
        assert call(cF=False) == -1
        assert call(n_=0) == -2
        assert call(nt_=0) == -2
        assert call(stp=2) == -5
        assert call(wsb_=8) == -4
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert bool((b == SENT).all()), k
    with torch.cuda.device(x.device):
        assert call() == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert not bool((b == SENT).any()), k


def test_noise_study_equals_statistics_by_hand():
    case = ud.CASES[1][1]
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x = ud.case_data(case)["x"][:3].to(DEV)
    paths, sigma, nt = 8, ud.SIGMA_REL * case.rad, 4
    mask = torch.tensor([1, 1, 0, 1])
    g = torch.Generator(device=DEV).manual_seed(11)
    with torch.no_grad():
        st = na.noise_study(x, net, prob, nt, sigma, paths, alph=case.alph, generator=g, mask=mask)
    assert last_kernel() == ud.KERNEL["lane"]
    g = torch.Generator(device=DEV).manual_seed(11)
    W = na.brownian_disturbances(nt, 3 * paths, case.d, sigma, generator=g, device=DEV, mask=mask)
    assert W.is_cuda and not W[..., 2].any() and W[..., 0].any()
    with torch.no_grad():
        tab = na.disturbed_rollout(x.repeat_interleave(paths, 0), net, prob, nt, W, alph=case.alph)["persample"].view(3, paths, 7)
    assert torch.equal(st["persample"], tab)
    cols = {"L+G": tab[:, :, 0] + case.alph[0] * tab[:, :, 1], "G": tab[:, :, 1], "Q": tab[:, :, 5], "W": tab[:, :, 6]}
    for name, v in cols.items():
        v = v.double().cpu()
        assert set(st[name]) == {"mean", "std", "q05", "q50", "q95"}
        for k, want in (("mean", v.mean(1)), ("std", v.std(1)), ("q05", torch.quantile(v, 0.05, dim=1)),
                        ("q50", torch.quantile(v, 0.5, dim=1)), ("q95", torch.quantile(v, 0.95, dim=1))):
            got = st[name][k].double().cpu()
            assert got.shape == (3,) and bool(torch.isfinite(got).all())
            assert torch.allclose(got, want, rtol=1e-5, atol=1e-6 * float(v.abs().max()) + 1e-30), (name, k)
    assert float(st["L+G"]["std"].min()) > 0.0                      # the disturbances reach the costs
    # chunked: two starts in the first launch, one in the second, the disturbances drawn chunk by chunk
    g = torch.Generator(device=DEV).manual_seed(11)
    with torch.no_grad():
        st2 = na.noise_study(x, net, prob, nt, sigma, paths, alph=case.alph, generator=g, mask=mask, max_rows=2 * paths)
        g = torch.Generator(device=DEV).manual_seed(11)
        tabs = []
        for xs in (x[:2], x[2:]):
            Wc = na.brownian_disturbances(nt, xs.shape[0] * paths, case.d, sigma, generator=g, device=DEV, mask=mask)
            tabs.append(na.disturbed_rollout(xs.repeat_interleave(paths, 0), net, prob, nt, Wc, alph=case.alph)["persample"])
    assert torch.equal(st2["persample"], torch.cat(tabs).view(3, paths, 7))
    with pytest.raises(ValueError, match="max_rows"):               # a chunk holds whole starts: none fits
        na.noise_study(x, net, prob, nt, sigma, paths, alph=case.alph, max_rows=paths - 1)
    with pytest.raises(ValueError, match="nex-by-d"):
        na.noise_study(x[0], net, prob, nt, sigma, paths, alph=case.alph)


def test_evalOC_noise_flag(tmp_path, capsys):
    """evalOC.py --noise on the shipped softcorridor fixture, the way tests/test_drivers_gpu.py runs the driver"""
    import evalOC
    from neuraloc_amd.checkpoint import save_checkpoint
    from conftest import load_golden
    g = load_golden("softcorridor")
    m = g.meta
    net = na.Phi(nTh=m["nTh"], m=m["m"], d=m["d"], alph=m["alph"])
    net.load_state_dict(g.state_dict())
    ck = os.path.join(str(tmp_path), "softcorridor_nn_checkpt.pth")
    save_checkpoint(ck, net, argparse.Namespace(data="softcorridor", m=m["m"], nTh=m["nTh"], alph=m["alph"], n_train=64, var0=1.0))
    save = os.path.join(str(tmp_path), "eval")
    nt = int(g["xinit_eval/nt"])
    out = evalOC.main(["--resume", ck, "--nt", str(nt), "--save", save, "--batch", "16", "--noise", "0.1", "--noise_paths", "32", "--noise_seed", "3"])
    text = capsys.readouterr().out
    lines = [ln for ln in text.splitlines() if ln.startswith("noise ")]
    assert [ln.split()[1] for ln in lines[1:]] == ["L+G", "G", "Q", "W"], lines
    z = np.load(os.path.join(save, "figs", "eval_softcorridor_nn_noise.npz"))
    assert z["persample"].shape == (1, 32, 7) and np.isfinite(z["persample"]).all() and int(z["paths"]) == 32 and int(z["seed"]) == 3
    assert abs(float(z["L+G/mean"][0]) - out["noise"]["L+G"]["mean"]) <= 1e-6 * abs(out["noise"]["L+G"]["mean"])
    assert out["noise"]["L+G"]["std"] > 0 and z["L+G/q05"][0] <= z["L+G/q50"][0] <= z["L+G/q95"][0]
    # the undisturbed evaluation next to it is the one without the flag
    want_J = float(g["xinit_eval/Jc"])
    assert abs(out["Jc"] - want_J) <= 1e-4 * abs(want_J)
    # without --noise nothing of it is printed or written
    save3 = os.path.join(str(tmp_path), "eval3")
    out3 = evalOC.main(["--resume", ck, "--nt", str(nt), "--save", save3, "--batch", "16"])
    text3 = capsys.readouterr().out
    assert "noise" not in out3 and not any(ln.startswith("noise") for ln in text3.splitlines())
    assert sorted(os.listdir(os.path.join(save3, "figs"))) == ["eval_softcorridor_nn.npz"]
    # --noise with --prec double is refused before anything runs or is written
    save4 = os.path.join(str(tmp_path), "eval4")
    with pytest.raises(SystemExit, match="single precision"):
        evalOC.main(["--resume", ck, "--nt", str(nt), "--save", save4, "--batch", "16", "--prec", "double", "--noise", "0.1"])
    assert not os.path.exists(save4) and "loading model" not in capsys.readouterr().out
