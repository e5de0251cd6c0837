"""GPU: min-max training (neuraloc_amd.minmax_ocflow_train / adversarial_step / pgd_ocflow_train, nocf_rollout_bwd_*_w_f32).  The parameter
gradients, dJc/dx and dJc/dW of ONE joint adjoint launch against the existing fp64 autograd yardsticks (tests/util_minmax.py) on every case
of util_disturb.CASES under util_oracle's rule; the three C entries inside NaN-guarded buffers at ragged sizes; shards with n_total; the free
iteration against its hand composition and, with frozen parameters, against the fp64 projected-ascent search; the K-step composition;
trainOC.py --adv."""
import ctypes as C
import os

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, adversary, train
import util_adversary as ua
import util_disturb as ud
import util_hip
import util_minmax as umm
import util_mono as um
import util_oracle as uo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def last_kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def _check(res, what):
    for k, v in res.items():
        print(f"{what} {k}: err {v[1]:.3e} tol {v[2]:.3e} fp32 restatement {v[3]:.3e}")
    assert not umm.failures(res), (what, umm.failures(res))


def _run(case, x, W, n_total=None, family=None, scale=None, w_grad=True):
    """one minmax_ocflow_train call and its backward -> (Jc, {name: gradient, "x": dJc/dx, "W": dJc/dW}) on the CPU"""
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    xx = x.to(DEV).clone().requires_grad_(True)
    WW = W.to(DEV).clone().requires_grad_(w_grad)
    Jc, cs = na.minmax_ocflow_train(xx, net, prob, list(case.tspan), case.nt, WW, case.stepper, case.alph, n_total=n_total)
    kf = last_kernel()
    (Jc if scale is None else scale * Jc).backward()
    torch.cuda.synchronize()
    kb = last_kernel()
    if family is not None:
        assert kf == ud.KERNEL[family], kf
        assert kb == (umm.JOINT_KERNEL if w_grad else umm.FULL_KERNEL)[family], kb
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    got["x"] = xx.grad.cpu()
    if w_grad:
        got["W"] = WW.grad.cpu()
    else:
        assert WW.grad is None
    return Jc.detach().cpu(), got


@pytest.mark.parametrize("fc", ud.CASES, ids=ud.case_id)
def test_joint_gradients_against_fp64_autograd(fc):
    """every parameter gradient, x.grad and W.grad of one forward and one joint adjoint pass the rule; both kernels are the family's; a
    second run is bitwise equal"""
    family, case = fc
    data = ud.case_data(case)
    Jc, got = _run(case, data["x"], data["W"], family=family)
    assert got["W"].shape == data["W"].shape and got["x"].shape == data["x"].shape
    _check(umm.compare(got, umm.references(case, torch.float64), umm.references(case, torch.float32)), case.id)
    Jc2, got2 = _run(case, data["x"], data["W"], family=family)
    assert torch.equal(Jc, Jc2)
    for k in got:
        assert torch.equal(got[k], got2[k]), k


SCALE_CASES = [ud.CASES[1], ud.CASES[3], ud.CASES[6], ud.CASES[7]]


@pytest.mark.parametrize("fc", SCALE_CASES, ids=ud.case_id)
def test_scaled_backward_and_a_constant_W(fc):
    """(3 Jc).backward() scales all three gradients (gJ multiplies the adjoint's outputs: 3 g in fp32, bit for bit); a W that does not
    require a gradient gives disturbed_ocflow_train's gradients bitwise on the existing (mode-0) kernel"""
    family, case = fc
    data = ud.case_data(case)
    _, g1 = _run(case, data["x"], data["W"], family=family)
    _, g3 = _run(case, data["x"], data["W"], family=family, scale=3.0)
    for k in g1:
        assert torch.equal(g3[k], 3.0 * g1[k]), k
    _, gc = _run(case, data["x"], data["W"], family=family, w_grad=False)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    xx = data["x"].to(DEV).clone().requires_grad_(True)
    Jc, _ = na.disturbed_ocflow_train(xx, net, prob, list(case.tspan), case.nt, data["W"].to(DEV), case.stepper, case.alph)
    Jc.backward()
    torch.cuda.synchronize()
    assert last_kernel() == umm.FULL_KERNEL[family]
    for k, p in net.named_parameters():
        assert torch.equal(gc[k], p.grad.cpu()), k
    assert torch.equal(gc["x"], xx.grad.cpu())
    # the joint kernel's parameter gradients against the mode-0 kernel's: the same statements, compiled separately -- the rule, not the bits
    r64, r32 = umm.references(case, torch.float64), umm.references(case, torch.float32)
    _check(umm.compare(gc, {k: v for k, v in r64.items() if k != "W"}, r32), case.id + " (mode 0)")


ABI_CASES = [ud.CASES[0], ud.CASES[1], ud.CASES[3], ud.CASES[4], ud.CASES[5], ud.CASES[7]]          # n = 5, 7, 17, 33, 17, 16
POISONED = {ud.CASES[1][1].id, ud.CASES[3][1].id, ud.CASES[5][1].id, ud.CASES[7][1].id}
GUARD = 1024


def _guarded(count):
    """a NaN-filled buffer with GUARD floats on either side of `count` floats -> (buffer, the view in the middle)"""
    buf = torch.full((count + 2 * GUARD,), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + count]


def _guards_intact(buf, mid):
    return bool(buf[:GUARD].isnan().all()) and bool(buf[GUARD + mid.numel():].isnan().all())


@pytest.mark.parametrize("fc", ABI_CASES, ids=ud.case_id)
def test_joint_entries_at_the_abi(fc):
    """nocf_rollout_bwd_small_w_f32 / _mid_w_f32 / _act_w_f32 with lamW and lam0 inside larger NaN-filled buffers: every
    [k < nt, row < n, i < d] is finite afterwards, passes the rule, and every guard float is still NaN; a NaN-filled workspace (the entry
    packs what it reads) changes nothing; lamW == NULL gives the existing entry's outputs bitwise on the existing kernel"""
    family, case = fc
    data = ud.case_data(case)
    n, d, nt, m = case.n, case.d, case.nt, case.m
    if case.id in POISONED:
        util_hip.poison_allocator(torch.device(DEV), big=1)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x, W = data["x"].to(DEV), data["W"].to(DEV)
    nstage = 4 if case.stepper == "rk4" else 1
    E = nt * nstage
    L = _lib.lib()
    rec_f = adversary._entries(L)[0]
    joint = train._joint_entries(L)
    assert joint is not None
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(x.device)
    nan = float("nan")
    s_all, z = torch.full((E, n, d + 1), nan, device=DEV), torch.full((n, d + 4), nan, device=DEV)
    tab, sums = torch.full((n, 7), nan, device=DEV), torch.full((8,), nan, device=DEV)
    nact = int(L.nocf_activation_record_floats(d, m, case.nTh, n, nt, train._STEPPERS[case.stepper])) if family == "mono" else 0
    act = torch.full((nact,), nan, device=DEV) if nact else None
    rec = C.c_int32(-1)
    alph_c = (C.c_float * 6)(*case.alph)
    hs = train._step_sizes(case.tspan, nt).to(DEV)
    st = train._STEPPERS[case.stepper]
    wsb = ws.numel() * ws.element_size()
    with torch.cuda.device(x.device):
        rc = rec_f(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), _lib.ptr(W), n, float(case.tspan[0]), float(case.tspan[1]), nt,
                   st, alph_c, _lib.ptr(z), _lib.ptr(tab), _lib.ptr(sums), _lib.ptr(s_all), _lib.ptr(act),
                   C.byref(rec), _lib.ptr(ws), wsb, _lib.stream_ptr(x.device))
    torch.cuda.synchronize()
    assert rc == 0 and last_kernel() == ud.KERNEL[family]
    act_p = act if rec.value else None
    P = int(L.nocf_small_grad_floats(d, m))
    mid_rows = int(L.nocf_mid_grad_rows(d, m, case.nTh, phi_st.r, prob_st.n_agents, n)) if family == "mono" else 0
    rows, Lr = (E + 2) * n, case.nTh - 1
    head = (C.byref(phi_st), C.byref(prob_st), n, nt, st, float(case.tspan[1]), alph_c, 1.0 / n, _lib.ptr(s_all), _lib.ptr(z), _lib.ptr(hs))

    def adjoint(lam0, lamW, existing=False):
        """one call of the family's joint entry (existing: of the entry it extends, which takes no lamW) -> its gradient buffers"""
        if case.id in POISONED:
            ws.fill_(255)                                            # every float of the workspace a NaN: the entry packs what it reads
        w = () if existing else (_lib.ptr(lamW),)
        sp = _lib.stream_ptr(x.device)
        with torch.cuda.device(x.device):
            if family == "lane":
                out = [torch.zeros(n, P, device=DEV)]
                f = L.nocf_rollout_bwd_small_f32 if existing else joint[0]
                rc = f(*head, _lib.ptr(out[0]), _lib.ptr(lam0), *w, sp)
            elif family == "mono":
                out = [torch.zeros(mid_rows, P, device=DEV)]
                f = L.nocf_rollout_bwd_mid_f32 if existing else joint[1]
                rc = f(*head, _lib.ptr(act_p), _lib.ptr(out[0]), mid_rows, _lib.ptr(lam0), *w, _lib.ptr(ws), wsb, sp)
            else:
                out = [torch.zeros(rows, m, device=DEV) for _ in range(3)] + [torch.zeros(Lr, rows, m, device=DEV) for _ in range(4)] + \
                      [torch.zeros(rows, d + 1, device=DEV) for _ in range(2)] + [torch.zeros(n, device=DEV)]
                Y, Ob, Wb, V, Ab, Qb, U0, Gb, Sx, PHIb = out
                f = L.nocf_rollout_bwd_act_f32 if existing else joint[2]
                rc = f(*head, *[_lib.ptr(t) for t in (Y, Ob, V, Ab, Qb, U0, Wb, Gb, Sx, PHIb)], _lib.ptr(lam0), *w, _lib.ptr(None),
                       _lib.ptr(ws), wsb, sp)
        torch.cuda.synchronize()
        assert rc == 0, rc
        assert last_kernel() == (umm.FULL_KERNEL if (existing or lamW is None) else umm.JOINT_KERNEL)[family], last_kernel()
        return out

    bufW, lamW = _guarded(nt * n * d)
    buf0, lam0 = _guarded(n * d)
    out = adjoint(lam0, lamW)
    for buf, mid in ((bufW, lamW), (buf0, lam0)):
        assert bool(torch.isfinite(mid).all()) and _guards_intact(buf, mid)
    assert all(bool(torch.isfinite(t).all()) for t in out)
    r64, r32 = umm.references(case, torch.float64), umm.references(case, torch.float32)
    _check({"lamW": uo.compare(lamW.view(nt, n, d), r64["W"], r32["W"]), "lam0": uo.compare(lam0.view(n, d), r64["x"], r32["x"])}, case.id)
    # without lam0: the same lamW, bit for bit
    bufW2, lamW2 = _guarded(nt * n * d)
    out2 = adjoint(None, lamW2)
    assert torch.equal(lamW2, lamW) and _guards_intact(bufW2, lamW2)
    for a, b in zip(out, out2):
        assert torch.equal(a, b)
    # lamW == NULL is the existing entry: its kernel, its bits
    buf03, lam03 = _guarded(n * d)
    out3 = adjoint(lam03, None)
    buf04, lam04 = _guarded(n * d)
    out4 = adjoint(lam04, None, existing=True)
    assert torch.equal(lam03, lam04) and _guards_intact(buf03, lam03)
    for a, b in zip(out3, out4):
        assert torch.equal(a, b)
    _check({"lam0 (mode 0)": uo.compare(lam03.view(n, d), r64["x"], r32["x"])}, case.id)


def test_two_shards_with_n_total():
    """the halves' W.grad concatenated (rows are independent, each carries 1 / n_total) and the summed parameter gradients against the
    whole batch's yardstick"""
    family, case = ud.CASES[3]
    data = ud.case_data(case)
    n = case.n
    parts = [_run(case, data["x"][sl], data["W"][:, sl].contiguous(), n_total=n, family=family)[1] for sl in (slice(0, 8), slice(8, n))]
    got = {k: parts[0][k] + parts[1][k] for k in parts[0] if k not in ("x", "W")}
    got["x"] = torch.cat([parts[0]["x"], parts[1]["x"]], 0)
    got["W"] = torch.cat([parts[0]["W"], parts[1]["W"]], 1)
    _check(umm.compare(got, umm.references(case, torch.float64), umm.references(case, torch.float32)), case.id + " (two shards)")
    sl = slice(0, 8)
    _check(umm.compare(parts[0], umm.references(case, torch.float64, n_total=n, rows=sl), umm.references(case, torch.float32, n_total=n, rows=sl)),
           case.id + " (first shard of n_total)")


STEP_CASES = [ud.CASES[1], ud.CASES[3], ud.CASES[5]]


@pytest.mark.parametrize("fc", STEP_CASES, ids=ud.case_id)
def test_adversarial_step_is_its_hand_composition(fc):
    """adversarial_step against minmax_ocflow_train, backward, ascend_disturbances written out: Jc, the parameter gradients and the updated W
    bitwise; W.grad cleared; the ascent against util_adversary.ascent_reference under the existing ascent test's per-element bound
    (nt d + 16) 2^-23 max(eps, |W|_inf); every row inside the ball"""
    family, case = fc
    data = ud.case_data(case)
    nt, d = case.nt, case.d
    eps = ua.median_path_norm(data["W"])                             # the rows start on either side of the ball's surface
    step = 2.5 * eps / 3
    ts = list(case.tspan)
    x = data["x"].to(DEV)

    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    Wa = data["W"].to(DEV).clone().requires_grad_(True)
    Ja, csa = na.adversarial_step(x, net, prob, ts, nt, Wa, eps, step, stepper=case.stepper, alph=case.alph)
    torch.cuda.synchronize()
    assert Wa.grad is None and Wa.requires_grad and last_kernel() == umm.JOINT_KERNEL[family]

    net2, prob2 = um.make_net(case, DEV), um.make_problem(case, DEV)
    Wb = data["W"].to(DEV).clone().requires_grad_(True)
    Jb, csb = na.minmax_ocflow_train(x, net2, prob2, ts, nt, Wb, case.stepper, case.alph)
    Jb.backward()
    g = Wb.grad.clone()
    with torch.no_grad():
        ret = na.ascend_disturbances(Wb, Wb.grad, eps, step)
    torch.cuda.synchronize()
    assert ret is Wb and torch.equal(Wb.grad, g)                     # (the direction is not modified)
    assert torch.equal(Ja, Jb.detach()) and all(torch.equal(a, b) for a, b in zip(csa, csb))
    assert torch.equal(Wa.detach(), Wb.detach())
    for (k, p), (_, q) in zip(net.named_parameters(), net2.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    want = ua.ascent_reference(data["W"], g.cpu(), None, step, eps)
    tol = (nt * d + 16) * 2.0 ** -23 * max(eps, float(data["W"].abs().max()))
    err = float((Wa.detach().cpu().double() - want).abs().max())
    print(f"{case.id}: ascent err {err:.3e} tol {tol:.3e}")
    assert err <= tol
    norms = Wa.detach().double().pow(2).sum((0, 2)).sqrt()
    assert bool((norms <= eps * (1 + 1e-5)).all()), float(norms.max())
    assert not torch.equal(Wa.detach().cpu(), data["W"])
    # a masked step leaves the masked components of a row it does not project bit for bit (eps large: no projection)
    mask = (torch.arange(d) % 2 == 0).float()
    Wm = data["W"].to(DEV).clone()
    na.ascend_disturbances(Wm, g, 1e6, step, mask=mask)
    torch.cuda.synchronize()
    assert torch.equal(Wm.cpu()[:, :, mask == 0], data["W"][:, :, mask == 0]) and not torch.equal(Wm.cpu(), data["W"])


SEARCH_CASES = [ud.CASES[0], ud.CASES[3], ud.CASES[5], ud.CASES[7]]      # tests/test_adversary_gpu.py's
SEARCH_STEPS = 3
_SEARCH = {}


def _search_refs(case):
    """the search on the training loss restated on the CPU in fp64 and fp32 (the rule's own error), once per case"""
    if case not in _SEARCH:
        data = ud.case_data(case)
        eps = ua.median_path_norm(data["W"])
        _SEARCH[case] = (eps, ua.search(case, torch.float64, data["x"], eps, SEARCH_STEPS, objective="Jc"),
                         ua.search(case, torch.float32, data["x"], eps, SEARCH_STEPS, objective="Jc"))
    return _SEARCH[case]


@pytest.mark.parametrize("fc", SEARCH_CASES, ids=ud.case_id)
def test_free_mode_is_projected_ascent_when_the_parameters_are_frozen(fc):
    """three adversarial_steps from W = 0 without an optimizer step: the per-row objective of a disturbed rollout at the resulting W against
    iterate 3 of the fp64 search on Jc (the normalised step does not see the mean's 1 / n), the fp32 search supplying the rule's own error;
    rows the fp64 search flags are left out, at most one in eight"""
    family, case = fc
    data = ud.case_data(case)
    eps, s64, s32 = _search_refs(case)
    n = case.n
    bad = s64["bad"]
    print(f"{case.id}: eps {eps:.4f}, the screen drops {int(bad.sum())} of {n} rows")
    assert 8 * int(bad.sum()) <= n
    assert bool((s64["objective"] > s64["nominal"]).all())           # the fp64 search gains on every start
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    x = data["x"].to(DEV)
    W = torch.zeros(case.nt, n, case.d, device=DEV, requires_grad=True)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    for _ in range(SEARCH_STEPS):
        na.adversarial_step(x, net, prob, list(case.tspan), case.nt, W, eps, 2.5 * eps / SEARCH_STEPS, stepper=case.stepper, alph=case.alph)
    assert last_kernel() == umm.JOINT_KERNEL[family]
    with torch.no_grad():
        out = na.disturbed_rollout(x, net, prob, case.nt, W.detach(), tspan=case.tspan, alph=case.alph, stepper=case.stepper)
    torch.cuda.synchronize()
    na.check_errors(sync=True)
    for k, p in net.named_parameters():
        assert torch.equal(p.detach(), before[k]), k                 # (nothing stepped the parameters)
    norms = W.detach().double().pow(2).sum((0, 2)).sqrt()
    assert bool((norms <= eps * (1 + 1e-5)).all()) and bool((norms > 0).all())
    obj = umm.row_objective(out["persample"].cpu(), case.alph)
    _check({"objective after 3 free steps": uo.compare(obj[~bad], s64["history"][SEARCH_STEPS][~bad], s32["history"][SEARCH_STEPS][~bad])},
           case.id)


PGD_CASES = [ud.CASES[0], ud.CASES[3]]


@pytest.mark.parametrize("objective", ua.OBJECTIVES)
@pytest.mark.parametrize("fc", PGD_CASES, ids=ud.case_id)
def test_pgd_is_its_two_call_composition(fc, objective):
    family, case = fc
    data = ud.case_data(case)
    eps = ua.median_path_norm(data["W"])
    ts = list(case.tspan)
    x = data["x"].to(DEV)
    net, prob = um.make_net(case, DEV), um.make_problem(case, DEV)
    Jc, cs, W = na.pgd_ocflow_train(x, net, prob, ts, case.nt, eps, 2, objective=objective, stepper=case.stepper, alph=case.alph)
    Jc.backward()
    net2, prob2 = um.make_net(case, DEV), um.make_problem(case, DEV)
    W2 = na.worst_case_disturbances(x, net2, prob2, case.nt, eps, steps=2, objective=objective, mask=None, W0=None, tspan=case.tspan,
                                    alph=case.alph, stepper=case.stepper)["W"]
    J2, cs2 = na.disturbed_ocflow_train(x, net2, prob2, ts, case.nt, W2, case.stepper, case.alph)
    J2.backward()
    torch.cuda.synchronize()
    assert last_kernel() == umm.FULL_KERNEL[family]
    assert torch.equal(W, W2) and torch.equal(Jc.detach(), J2.detach()) and all(torch.equal(a, b) for a, b in zip(cs, cs2))
    for (k, p), (_, q) in zip(net.named_parameters(), net2.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    assert bool((W.double().pow(2).sum((0, 2)).sqrt() <= eps * (1 + 1e-5)).all()) and bool((W != 0).any())


def _train_lines(capsys, tmp_path, name, *flags):
    import trainOC
    save = os.path.join(str(tmp_path), name)
    trainOC.main(["--data", "softcorridor", "--niters", "3", "--val_freq", "3", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save,
                  "--seed", "1", "--lr", "0.02", *flags])
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln[:5].isdigit()]
    assert len(lines) == 3
    return lines, save


def test_trainOC_adv_flag(tmp_path, capsys):
    """trainOC.py --adv EPS --niters 3 in both modes on the problem tests/test_drivers_gpu.py trains (softcorridor, m = 16, 16 samples): a
    checkpoint, finite losses, the unchanged log line; the free mode's W starts at zero, so its first loss is the plain run's"""
    loss = lambda lines: [ln.split()[3] for ln in lines]             # noqa: E731
    free, sf = _train_lines(capsys, tmp_path, "free", "--adv", "0.5", "--adv_steps", "2")
    pgd, sp = _train_lines(capsys, tmp_path, "pgd", "--adv", "0.5", "--adv_mode", "pgd", "--adv_steps", "2")
    ctl, sc = _train_lines(capsys, tmp_path, "ctl", "--adv", "0.5", "--adv_mode", "pgd", "--adv_steps", "2", "--adv_objective", "control")
    plain, _ = _train_lines(capsys, tmp_path, "plain")
    for lines in (free, pgd, ctl, plain):
        assert all(float(v) == float(v) and abs(float(v)) < float("inf") for ln in lines for v in ln.split()[3:])
        assert [len(ln.split()) for ln in lines] == [11, 11, 19]
    for save in (sf, sp, sc):
        assert any(f.endswith("_checkpt.pth") for f in os.listdir(save))
    assert loss(free)[0] == loss(plain)[0] and loss(free)[1] != loss(plain)[1]
    assert loss(pgd)[0] != loss(plain)[0] and loss(ctl)[0] != loss(plain)[0]
    # validation is undisturbed: with a learning rate of 0 the validation costs are the plain run's
    f0, _ = _train_lines(capsys, tmp_path, "f0", "--adv", "0.5", "--adv_steps", "2", "--lr", "0")
    p0, _ = _train_lines(capsys, tmp_path, "p0", "--lr", "0")
    assert f0[2].split()[11:] == p0[2].split()[11:] and f0[2].split()[3] != p0[2].split()[3]
