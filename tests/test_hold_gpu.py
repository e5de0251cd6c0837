"""GPU: the zero-order-hold rollout (nocf_rollout_held_f32, neuraloc_amd.hold) on every new kernel instantiation against the fp64 restatement of
tests/util_hold.py under util_oracle's rule, for K in {1, 2, nt, nt + 3} with and without W; the HJB column exactly 0; W = 0 against W = None
and K = nt against K = nt + 3 bitwise; row independence in a 1027-row batch; NaN guard bands around every output buffer; hold_study's shared
W; the C entry's refusals; the evalOC flag."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, hold as nh
import util_hold as uh
import util_lane as ul
import util_mono as um

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                                      # floats of NaN in front of and behind every output buffer


def last_kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def _banded(*shape):
    """an output buffer inside NaN guard bands -> (whole allocation, the buffer as a view of its middle)"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def c_held(case, net, prob, x, W, hold, intermediates=True, expect=0, **over):
    """nocf_rollout_held_f32 itself, every output inside guard bands that must come back intact -> dict table, z, zFull, ctrlFull, sums,
    means (expect = 0), or the untouched buffers after a refusal.  over: null_x / n / nt / ws_bytes / ctrl replaced for the refusals"""
    n, d, nt = x.shape[0], case.d, case.nt
    f = nh._entry(_lib.lib())
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(x.device)
    cdim = _lib.lib().nocf_ctrl_dim(C.byref(prob_st), d)
    bufs = {"z": _banded(n, d + 4), "table": _banded(n, 7), "sums": _banded(8), "means": _banded(8)}
    if intermediates:
        bufs.update(zFull=_banded(nt + 1, n, d + 4), ctrlFull=_banded(nt + 1, n, cdim))
    alph_c = (C.c_float * 6)(*case.alph)
    ptr = lambda k: _lib.ptr(bufs[k][1]) if k in bufs else None      # noqa: E731
    with torch.cuda.device(x.device):
        rc = f(C.byref(phi_st), C.byref(prob_st), _lib.ptr(None if over.get("null_x") else x), _lib.ptr(W), hold,
               over.get("n", n), float(case.tspan[0]), float(case.tspan[1]), over.get("nt", nt), 4 if case.stepper == "rk4" else 1, alph_c,
               ptr("z"), ptr("table"), ptr("sums"), ptr("means"), ptr("zFull"), None if over.get("ctrl") is False else ptr("ctrlFull"),
               _lib.ptr(ws), over.get("ws_bytes", ws.numel() * ws.element_size()), _lib.stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    for k, (whole, view) in bufs.items():
        assert bool(torch.isnan(whole[:GUARD]).all()) and bool(torch.isnan(whole[-GUARD:]).all()), f"guard band of {k} overwritten"
        if expect == 0:
            assert not bool(torch.isnan(view).any()), f"{k} holds an unwritten entry"
        else:
            assert bool(torch.isnan(view).all()), f"{k} was written by a refused call"
    out = {k: v[1] for k, v in bufs.items()}
    if intermediates and expect == 0:
        out["zFull"], out["ctrlFull"] = out["zFull"].permute(1, 2, 0), out["ctrlFull"].permute(1, 2, 0)
    return out


def py_held(case, net, prob, x, W, hold, intermediates=True):
    with torch.no_grad():
        out = na.held_rollout(x, net, prob, list(case.tspan), case.nt, hold, W=W, stepper=case.stepper, alph=case.alph, intermediates=intermediates)
    torch.cuda.synchronize()
    keys = ("Jc", "cs", "table", "z", "zFull", "ctrlFull")
    return dict(zip(keys, out))


@pytest.mark.parametrize("fc", uh.CASES, ids=uh.case_id)
def test_against_fp64_on_every_instantiation(fc):
    family, case = fc
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    d = case.d
    for ki, dist in uh.COMBOS:
        K = uh.holds(case)[ki]
        data = uh.case_data(case, K, dist)
        x, W = data["x"].to(DEV), data["W"].to(DEV) if dist else None
        got = c_held(case, net, prob, x, W, K)
        assert last_kernel() == uh.KERNEL[(family, dist)], last_kernel()
        res = uh.compare(got, data["r64"], data["r32"])
        for k, v in res.items():
            print(f"{case.id} K={K} W={dist} {k}: err {v[1]:.3e} tol {v[2]:.3e} fp32 restatement {v[3]:.3e}")
        assert not ul.failures(res), (K, dist, ul.failures(res))
        # a held control has no HJB residual: exactly 0, at every step
        assert bool((got["table"][:, 2] == 0).all()) and bool((got["z"][:, d + 1] == 0).all()) and bool((got["zFull"][:, d + 1] == 0).all())
        assert bool((got["ctrlFull"][:, :, 0] == 0).all())
        # the Python call returns the same bits, the means are the table's, and the run without intermediates gives the same table and state
        py = py_held(case, net, prob, x, W, K)
        for k in ("table", "z", "zFull", "ctrlFull"):
            assert torch.equal(py[k], got[k]), k
        tab = got["table"].double().cpu()
        a = case.alph
        for c in range(7):
            assert abs(float(py["cs"][c]) - float(tab[:, c].mean())) <= 1e-5 * (abs(float(tab[:, c].mean())) + 1e-30) + 1e-30
        jc = tab[:, 0].mean() + a[0] * tab[:, 1].mean() + a[3] * tab[:, 2].mean() + a[4] * tab[:, 3].mean() + a[5] * tab[:, 4].mean()
        assert abs(float(py["Jc"]) - float(jc)) <= 1e-5 * abs(float(jc))
        plain = c_held(case, net, prob, x, W, K, intermediates=False)
        assert last_kernel() == uh.KERNEL[(family, dist)]
        assert not ul.failures(uh.compare(plain, data["r64"], data["r32"]))


FAMILY_CASES = [uh.GROUP_I[1], uh.GROUP_I[3], uh.GROUP_I[4]]            # lane with obstacle and W; singlequad; one-CU point agents


@pytest.mark.parametrize("fc", FAMILY_CASES, ids=uh.case_id)
def test_zero_W_equals_no_W_and_the_open_loop_limit_is_one_rollout(fc):
    family, case = fc
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x = uh.case_data(case, 1, False)["x"].to(DEV)
    Z = torch.zeros(case.nt, case.n, case.d, device=DEV)
    for K in uh.holds(case):
        a, b = py_held(case, net, prob, x, None, K), py_held(case, net, prob, x, Z, K)
        assert last_kernel() == uh.KERNEL[(family, True)]
        for k in ("table", "z", "zFull", "ctrlFull", "Jc"):
            assert torch.equal(a[k], b[k]), (K, k)
    W = uh.case_data(case, 1, True)["W"].to(DEV)
    for Wk in (None, W):
        a, b = py_held(case, net, prob, x, Wk, case.nt), py_held(case, net, prob, x, Wk, case.nt + 3)
        for k in ("table", "z", "zFull", "ctrlFull", "Jc"):
            assert torch.equal(a[k], b[k]), k
        c1 = a["ctrlFull"][:, :, 1:2]
        assert torch.equal(a["ctrlFull"][:, :, 1:], c1.expand(-1, -1, case.nt)) and bool((c1 != 0).any())
        # ... and the refresh rate matters: K = 1 is another rollout
        assert not torch.equal(py_held(case, net, prob, x, Wk, 1)["z"], a["z"])


@pytest.mark.parametrize("fc", FAMILY_CASES, ids=uh.case_id)
def test_a_row_of_a_large_batch_equals_the_row_alone_bitwise(fc):
    """tail waves of the lane kernel (1027 = 4 * 256 + 3), the ragged last tile of the one-CU kernel (1027 = 16 * 64 + 3)"""
    import util_disturb as ud
    family, case = fc
    n = 1027
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x = um.candidates(case, n).to(DEV)
    W = ud.disturbances(case, n, seed_offset=1).to(DEV)
    for Wk in (None, W):
        big = py_held(case, net, prob, x, Wk, 2)
        assert last_kernel() == uh.KERNEL[(family, Wk is not None)]
        assert bool(torch.isfinite(big["table"]).all())
        for i in (0, 15, 16, 513, 1024, 1026):
            one = py_held(case, net, prob, x[i:i + 1].contiguous(), None if Wk is None else Wk[:, i:i + 1].contiguous(), 2)
            for k in ("table", "z", "zFull", "ctrlFull"):
                assert torch.equal(one[k], big[k][i:i + 1]), (i, k)


def test_hold_study_pairs_every_K_with_one_W():
    family, case = uh.GROUP_I[1]
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x = uh.case_data(case, 1, False)["x"][:3].to(DEV)
    paths, sigma, nt, seed = 8, 0.05 * case.rad, 4, 11
    for p_ in net.parameters():                                        # (an evaluation: refused in grad mode with trainable parameters)
        p_.requires_grad_(False)
    st = na.hold_study(x, net, prob, nt, holds=(1, 2, 4), sigma=sigma, seed=seed, paths=paths, alph=case.alph)
    assert sorted(st) == [0, 1, 2, 4]
    W = na.counter_disturbances(nt, 3 * paths, case.d, sigma, seed, device=DEV)
    xs = x.repeat_interleave(paths, 0).contiguous()
    with torch.no_grad():
        for K in (1, 2, 4):
            tab = na.held_rollout(xs, net, prob, [0.0, 1.0], nt, K, W=W, alph=case.alph)[2]
            assert last_kernel() == uh.KERNEL[("lane", True)]
            assert torch.equal(st[K]["persample"], tab.view(3, paths, 7)), K
        ref = na.disturbed_rollout(xs, net, prob, nt, W, alph=case.alph)["persample"]
    assert torch.equal(st[0]["persample"], ref.view(3, paths, 7))
    tab = st[1]["persample"].double().cpu()
    want = {"L+G": tab[:, :, 0] + case.alph[0] * tab[:, :, 1], "G": tab[:, :, 1], "L": tab[:, :, 0], "Q": tab[:, :, 5], "W": tab[:, :, 6]}
    for name, v in want.items():
        assert set(st[1][name]) == {"mean", "std", "q05", "q50", "q95"}
        assert torch.allclose(st[1][name]["mean"].double().cpu(), v.mean(1), rtol=1e-5, atol=1e-6 * float(v.abs().max()) + 1e-30)
        assert torch.allclose(st[1][name]["q50"].double().cpu(), torch.quantile(v, 0.5, dim=1), rtol=1e-5, atol=1e-6 * float(v.abs().max()) + 1e-30)
    assert float(st[1]["L+G"]["std"].min()) > 0.0                     # the disturbances reach the costs
    # chunked: the noise of a global row does not depend on the chunking, so neither does any figure
    st2 = na.hold_study(x, net, prob, nt, holds=(2,), sigma=sigma, seed=seed, paths=paths, alph=case.alph, max_rows=2 * paths)
    assert torch.equal(st2[2]["persample"], st[2]["persample"]) and torch.equal(st2[0]["persample"], st[0]["persample"])
    # without sigma: one undisturbed row per start, hold 0 is OCflow's own table
    st3 = na.hold_study(x, net, prob, nt, holds=(1, 4), alph=case.alph)
    with torch.no_grad():
        _, cs = na.OCflow(x, net, prob, [0.0, 1.0], nt, "rk4", case.alph, noMean=True)
        t4 = na.held_rollout(x, net, prob, [0.0, 1.0], nt, 4, alph=case.alph)[2]
    assert torch.equal(st3[0]["persample"][:, 0], torch.cat(cs, 1)) and torch.equal(st3[4]["persample"][:, 0], t4)
    assert st3[4]["L+G"].shape == (3,) and torch.equal(st3[4]["L"], t4[:, 0])
    with pytest.raises(ValueError, match="pass sigma"):
        na.hold_study(x, net, prob, nt, paths=4)


def test_the_C_entry_refuses_with_nothing_enqueued():
    family, case = uh.GROUP_I[0]
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x = uh.case_data(case, 1, False)["x"].to(DEV)
    c_held(case, net, prob, x, None, 0, expect=-2)
    c_held(case, net, prob, x, None, -3, expect=-2)
    c_held(case, net, prob, x, None, 1, expect=-1, null_x=True)
    c_held(case, net, prob, x, None, 1, expect=-1, ctrl=False)         # zFull without ctrlFull
    c_held(case, net, prob, x, None, 1, expect=-2, n=0)
    c_held(case, net, prob, x, None, 1, expect=-2, nt=0)
    c_held(case, net, prob, x, None, 1, expect=-4, ws_bytes=8)
    before = last_kernel()
    # an m = 129 network: the per-tile / split-role families take no held control
    wide = um.MonoCase("cross2d", 4, 129, 5, "softcorridor", "eval", 5, "rk4", 3)
    c_held(wide, um.make_net(wide, DEV), um.make_problem(wide, DEV), um.candidates(wide, 5).to(DEV), None, 1, expect=-2)
    # three layers, and a quadcopter problem of two craft
    deep = um.MonoCase("cross2d", 6, 48, 5, None, "eval", 5, "rk4", 3, nTh=3)
    c_held(deep, um.make_net(deep, DEV), um.make_problem(deep, DEV), um.candidates(deep, 5).to(DEV), None, 1, expect=-2)
    two = um.MonoCase("quad", 24, 64, 10, None, "eval", 5, "rk4", 3)
    c_held(two, um.make_net(two, DEV), um.make_problem(two, DEV), um.candidates(two, 5).to(DEV), None, 2, expect=-2)
    assert last_kernel() == before                                     # nothing was launched by a refused call
    with pytest.raises(NotImplementedError, match="2 craft"):
        na.held_rollout(um.candidates(two, 5).to(DEV), um.make_net(two, DEV).eval(), um.make_problem(two, DEV), [0.0, 1.0], 3, 2)
    # ... and the same buffers take a valid call
    c_held(case, net, prob, x, None, 1)
    assert last_kernel() == uh.KERNEL[("lane", False)]


def test_evalOC_hold_flag(tmp_path, capsys):
    """evalOC.py --hold on the shipped softcorridor fixture, the way tests/test_drivers_gpu.py runs the driver"""
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
    out = evalOC.main(["--resume", ck, "--nt", str(nt), "--save", save, "--batch", "16", "--hold", "1,5"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("hold ")]
    assert [ln.split()[1] for ln in lines] == ["K", "0", "1", "5"], lines
    z = np.load(os.path.join(save, "figs", "eval_softcorridor_nn_hold.npz"))
    assert list(z["holds"]) == [0, 1, 5] and z["5/persample"].shape == (1, 1, 7) and np.isfinite(z["5/persample"]).all()
    assert abs(float(z["5/L+G"][0]) - out["hold"][5]["L+G"]) <= 1e-6 * abs(out["hold"][5]["L+G"])
    assert float(z["5/persample"][0, 0, 2]) == 0.0 and float(z["0/persample"][0, 0, 2]) > 0.0
    want_J = float(g["xinit_eval/Jc"])                                  # the evaluation next to it is the one without the flag
    assert abs(out["Jc"] - want_J) <= 1e-4 * abs(want_J)
    # with --noise: statistics over paths, the same for every K
    save2 = os.path.join(str(tmp_path), "eval2")
    out2 = evalOC.main(["--resume", ck, "--nt", str(nt), "--save", save2, "--batch", "16", "--hold", "2", "--noise", "0.1", "--noise_paths", "16",
                        "--noise_seed", "3", "--noise_rho", "0.5"])
    z2 = np.load(os.path.join(save2, "figs", "eval_softcorridor_nn_hold.npz"))
    assert z2["2/persample"].shape == (1, 16, 7) and int(z2["paths"]) == 16 and out2["hold"][2]["L+G"]["std"] > 0
    assert z2["2/L+G/q05"][0] <= z2["2/L+G/q50"][0] <= z2["2/L+G/q95"][0]
    assert [ln.split()[1] for ln in capsys.readouterr().out.splitlines() if ln.startswith("hold ")][-2:] == ["0", "2"]
    # without --hold nothing of it is printed or written
    save3 = os.path.join(str(tmp_path), "eval3")
    out3 = evalOC.main(["--resume", ck, "--nt", str(nt), "--save", save3, "--batch", "16"])
    text3 = capsys.readouterr().out
    assert "hold" not in out3 and not any(ln.startswith("hold") for ln in text3.splitlines())
    assert sorted(os.listdir(os.path.join(save3, "figs"))) == ["eval_softcorridor_nn.npz"]
