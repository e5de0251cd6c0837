"""Ensembles on the MI355X: member e of one ensemble launch against the single-network call on that member alone -- bit for bit, forward and
gradients, at every (MP, DP) instantiation of the lane kernels (cases and shapes: tests/util_ensemble.py)."""
import contextlib
import os

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, ensemble
from neuraloc_amd.OCflow import _launch as single_launch
from neuraloc_amd.train import ocflow_train

import util_ensemble as ue

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024


def _kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def _guarded(*shape):
    """a NaN-filled buffer with GUARD floats on either side of a tensor of `shape` -> (buffer, the view in the middle)"""
    count = 1
    for v in shape:
        count *= v
    buf = torch.full((count + 2 * GUARD,), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + count].view(*shape)


def _setup(case, members=ue.E, first=0):
    nets = ue.member_nets(case, DEV, members, first)
    rows = ue.member_rows(members, first)
    ens = na.PhiEnsemble.from_members(nets, alph=rows)
    x = ue.starts(case, members, first=first).to(DEV)
    prob = ue.member_problem(case, 0, DEV, first)          # (its alph_Q / alph_W are not read by an ensemble call)
    return ens, rows, x, prob


def _member_x(case, x, e):
    return (x[e] if case.own_x else x[0]).contiguous()


@pytest.mark.parametrize("case", ue.FORWARD, ids=lambda c: c.id)
def test_forward_members_equal_the_single_network_call(case):
    b = case.base
    E, n, d, nt = ue.E, b.n, b.d, b.nt
    ens, rows, x, prob = _setup(case)
    xe = x if case.own_x else x[0]
    cdim = d
    bufs, guards = {}, {}
    for key, shape in (("persample", (E * n, 7)), ("z_out", (E * n, d + 4)), ("sums", (E, 8)), ("means", (E, 8)),
                       ("zFull", (nt + 1, E * n, d + 4)), ("ctrlFull", (nt + 1, E * n, cdim))):
        guards[key], bufs[key] = _guarded(*shape)
    with torch.no_grad():
        out = ensemble._launch(xe, ens, prob, b.tspan, nt, b.stepper, None, intermediates=True, bufs=bufs)
        assert _kernel() == "rollout_lane_kernel<ens>"
        Jc, cs = na.ensemble_rollout(xe, ens, prob, b.tspan, nt, b.stepper)
        assert _kernel() == "rollout_lane_kernel<ens>"
        Jc2, cs2, traj, ctrl = na.ensemble_rollout(xe, ens, prob, b.tspan, nt, b.stepper, intermediates=True)
    torch.cuda.synchronize()
    # nothing outside the stated rows is written, every stated row is
    for key, g in guards.items():
        mid = bufs[key].numel()
        assert bool(g[:GUARD].isnan().all()) and bool(g[GUARD + mid:].isnan().all()), key
        assert bool(torch.isfinite(out[key]).all()), key
    assert tuple(Jc.shape) == (E,) and tuple(cs.shape) == (E, 7)
    assert tuple(traj.shape) == (E, n, d + 4, nt + 1) and tuple(ctrl.shape) == (E, n, cdim, nt + 1)
    assert torch.equal(Jc, out["means"][:, 7]) and torch.equal(cs, out["means"][:, :7]) and torch.equal(Jc2, Jc) and torch.equal(cs2, cs)
    zF = out["zFull"].view(nt + 1, E, n, d + 4)
    cF = out["ctrlFull"].view(nt + 1, E, n, cdim)
    assert torch.equal(traj, zF.permute(1, 2, 3, 0)) and torch.equal(ctrl, cF.permute(1, 2, 3, 0))
    differ = 0
    for e in range(E):
        net, pe, x1 = ens.member(e), ue.member_problem(case, e, DEV), _member_x(case, x, e)
        assert (pe.alph_Q, pe.alph_W) == (rows[e][1], rows[e][2]) and net.alph == rows[e]
        with torch.no_grad():
            means = torch.empty(8, device=DEV)
            tab, sums, zF1, cF1 = single_launch(x1, net, pe, list(b.tspan), nt, b.stepper, rows[e], True, means)
            assert _kernel() == "rollout_lane_kernel"           # the yardstick ran the single-network lane kernel
            J1, c1 = na.OCflow(x1, net, pe, list(b.tspan), nt, b.stepper, rows[e])
            assert _kernel() == "rollout_lane_kernel"
            t1, u1 = na.OCflow(x1, net, pe, list(b.tspan), nt, b.stepper, rows[e], intermediates=True)
        sl = slice(e * n, (e + 1) * n)
        assert torch.equal(out["persample"][sl], tab), e
        assert torch.equal(out["z_out"][sl], zF1[nt]), e
        assert torch.equal(out["sums"][e], sums), e
        assert torch.equal(out["means"][e], means), e
        assert torch.equal(zF[:, e], zF1) and torch.equal(cF[:, e], cF1), e
        assert torch.equal(Jc[e], J1) and torch.equal(cs[e], torch.stack(c1)), e
        assert torch.equal(traj[e], t1) and torch.equal(ctrl[e], u1), e
        differ += int(not torch.equal(out["persample"][sl], out["persample"][:n]))
    assert differ == E - 1                                      # the members are different networks: a launch that read member 0 thrice fails
    # the want_W branch differs between the members: no interaction cost where alph_W = 0, one where it is not
    if b.n_agents >= 2:
        assert bool((out["persample"][n:2 * n, 6] == 0).all()) and bool((out["persample"][:n, 6] != 0).any())


def test_one_member_one_row_equals_the_plain_call():
    case = ue.FORWARD[3]
    b = case.base
    ens, rows, x, prob = _setup(case, members=1)
    x1 = x[0, :1].contiguous()
    net, pe = ens.member(0), ue.member_problem(case, 0, DEV)
    with torch.no_grad():
        Jc, cs, traj, ctrl = na.ensemble_rollout(x1, ens, prob, b.tspan, b.nt, b.stepper, intermediates=True)
        assert _kernel() == "rollout_lane_kernel<ens>"
        J1, c1 = na.OCflow(x1, net, pe, list(b.tspan), b.nt, b.stepper, rows[0])
        t1, u1 = na.OCflow(x1, net, pe, list(b.tspan), b.nt, b.stepper, rows[0], intermediates=True)
        Jo, co = na.ensemble_rollout(x1[None], ens, prob, b.tspan, b.nt, b.stepper)       # the same row as the member's own
    assert torch.equal(Jc[0], J1) and torch.equal(cs[0], torch.stack(c1)) and torch.equal(traj[0], t1) and torch.equal(ctrl[0], u1)
    assert torch.equal(Jo, Jc) and torch.equal(co, cs)


@pytest.mark.parametrize("own", [False, True])
def test_a_member_does_not_depend_on_its_position(own):
    """the member at index 2 of E = 3 is the member at index 0 of E = 7, bitwise"""
    case = ue.FORWARD[4]
    b = case.base
    n = b.n
    nets3, rows3 = ue.member_nets(case, DEV, 3), ue.member_rows(3)
    nets7 = [nets3[2]] + ue.member_nets(case, DEV, 6, first=3)
    rows7 = [rows3[2]] + ue.member_rows(6, first=3)
    e3, e7 = na.PhiEnsemble.from_members(nets3, alph=rows3), na.PhiEnsemble.from_members(nets7, alph=rows7)
    x3 = ue.starts(case, 3).to(DEV)
    x7 = torch.cat([x3[2:3], ue.starts(case, 6, first=3).to(DEV)])
    prob = ue.member_problem(case, 0, DEV)
    with torch.no_grad():
        o3 = ensemble._launch(x3 if own else x3[2], e3, prob, b.tspan, b.nt, b.stepper, None, intermediates=True)
        o7 = ensemble._launch(x7 if own else x3[2], e7, prob, b.tspan, b.nt, b.stepper, None, intermediates=True)
    for key in ("persample", "z_out"):
        assert torch.equal(o3[key][2 * n:3 * n], o7[key][:n]), key
    assert torch.equal(o3["sums"][2], o7["sums"][0]) and torch.equal(o3["means"][2], o7["means"][0])
    for key in ("zFull", "ctrlFull"):
        assert torch.equal(o3[key][:, 2 * n:3 * n], o7[key][:, :n]), key
    assert not torch.equal(o3["persample"][:n], o7["persample"][n:2 * n])


@contextlib.contextmanager
def _saved(into):
    """collects the tensors an autograd.Function saves for its backward (the recorded stage inputs and the final states)"""
    def pack(t):
        into.append(t)
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        yield


def _single_train(case, ens, rows, x, e, gj=None):
    """ocflow_train + backward() on member e alone -> (Jc, cs, s_all, {name: grad}, x.grad)"""
    b = case.base
    net, pe = ens.member(e), ue.member_problem(case, e, DEV)
    x1 = _member_x(case, x, e).clone().requires_grad_(True)
    saved = []
    with _saved(saved):
        J1, c1 = ocflow_train(x1, net, pe, list(b.tspan), b.nt, b.stepper, rows[e])
    assert _kernel() == "rollout_lane_kernel"
    (J1 if gj is None else gj * J1).backward()
    assert _kernel() == "rollout_lane_bwd_kernel"
    s_all = next(t for t in saved if t.dim() == 3)
    return J1.detach(), torch.stack(c1), s_all, {k: p.grad for k, p in net.named_parameters()}, x1.grad


@pytest.mark.parametrize("case", ue.TRAIN, ids=lambda c: c.id)
def test_training_members_equal_the_single_network_adjoint(case):
    b = case.base
    E, n, d = ue.E, b.n, b.d
    ens, rows, x, prob = _setup(case)
    xe = x.clone().requires_grad_(True)
    saved = []
    with _saved(saved):
        Jc, cs = na.ensemble_ocflow_train(xe, ens, prob, b.tspan, b.nt, b.stepper)
    assert _kernel() == "rollout_lane_kernel<ens>"
    assert tuple(Jc.shape) == (E,) and tuple(cs.shape) == (E, 7) and Jc.requires_grad and not cs.requires_grad
    Jc.sum().backward()                                         # upstream gradient 1 for every member
    assert _kernel() == "rollout_lane_bwd_kernel<ens>"
    s_all = next(t for t in saved if t.dim() == 3)
    nstage = 4 if b.stepper == "rk4" else 1
    assert tuple(s_all.shape) == (b.nt * nstage, E * n, d + 1)
    for e in range(E):
        J1, c1, s1, g1, gx1 = _single_train(case, ens, rows, x, e)
        assert torch.equal(Jc[e].detach(), J1) and torch.equal(cs[e], c1), e
        assert torch.equal(s_all[:, e * n:(e + 1) * n], s1), e
        assert torch.equal(xe.grad[e], gx1), e
        for name, p in ens.named_parameters():
            assert p.grad is not None and torch.equal(p.grad[e], g1[name]), (e, name)
    assert all(bool((p.grad[e] != 0).any()) for e in range(E) for _, p in ens.named_parameters())


def test_a_non_unit_upstream_gradient_scales_each_member():
    case = ue.TRAIN[1]
    b = case.base
    E = ue.E
    ens, rows, x, prob = _setup(case)
    gJ = torch.tensor([1.0, 0.5, -2.0], device=DEV)
    xs = x[0].contiguous()                                      # one batch shared by the members (no x gradient)
    shared = ue.EnsCase(b, False)
    Jc, _ = na.ensemble_ocflow_train(xs, ens, prob, b.tspan, b.nt, b.stepper)
    Jc.sum().backward()
    unit = {k: p.grad.clone() for k, p in ens.named_parameters()}
    ens.zero_grad(set_to_none=True)
    Jc, _ = na.ensemble_ocflow_train(xs, ens, prob, b.tspan, b.nt, b.stepper)
    (gJ * Jc).sum().backward()
    for e in range(E):
        _, _, _, g1, _ = _single_train(shared, ens, rows, x, e, gj=gJ[e])
        for name, p in ens.named_parameters():
            assert torch.equal(p.grad[e], gJ[e] * unit[name][e]), (e, name)        # (a power of two: exact)
            assert torch.equal(p.grad[e], g1[name]), (e, name)


def test_two_adam_steps_equal_three_separate_optimisers():
    case = ue.TRAIN[0]
    b = case.base
    E = ue.E
    ens, rows, x, prob = _setup(case)
    xs = x[0].contiguous()
    nets = [ens.member(e) for e in range(E)]
    probs = [ue.member_problem(case, e, DEV) for e in range(E)]
    opt = torch.optim.Adam(ens.parameters(), lr=0.01)
    opts = [torch.optim.Adam(q.parameters(), lr=0.01) for q in nets]
    for _ in range(2):
        opt.zero_grad()
        Jc, _ = na.ensemble_ocflow_train(xs, ens, prob, b.tspan, b.nt, b.stepper)
        Jc.sum().backward()
        opt.step()
        for e in range(E):
            opts[e].zero_grad()
            J1, _ = ocflow_train(xs, nets[e], probs[e], list(b.tspan), b.nt, b.stepper, rows[e])
            J1.backward()
            opts[e].step()
    for e in range(E):
        for (name, p), (_, q) in zip(ens.named_parameters(), nets[e].named_parameters()):
            assert torch.equal(p[e], q), (e, name)
    assert not torch.equal(ens.A[0], na.PhiEnsemble.from_members(ue.member_nets(case, DEV), alph=rows).A[0])      # the steps moved the weights


def test_the_abi_refuses_what_the_lane_family_does_not_take():
    import ctypes as C
    case = ue.TRAIN[0]
    b = case.base
    ens, rows, x, prob = _setup(case)
    L, (f_eval, f_rec, f_bwd) = ensemble._shipped()
    phi_st, keep = ens._c_struct()
    prob_st, keep2 = prob._c_struct(torch.device(DEV))
    table = ens.alph_table()
    n, d = b.n, b.d
    tab, sums = torch.empty(ue.E * n, 7, device=DEV), torch.empty(ue.E, 8, device=DEV)

    def call(members=ue.E, stride=0, phi=phi_st, pr=prob_st):
        return f_eval(C.byref(phi), C.byref(pr), _lib.ptr(x), n, members, stride, 0.0, 1.0, 2, _lib.NOCF_RK4, _lib.ptr(table),
                      None, _lib.ptr(tab), _lib.ptr(sums), None, None, None, None, 0, _lib.stream_ptr(torch.device(DEV)))
    assert call() == 0 and call(stride=n * d) == 0
    assert call(members=0) == -2 and call(stride=d) == -2
    for field, value in (("nTh", 3), ("m", 33), ("d", 32)):
        ph = _lib.NocfPhi.from_buffer_copy(phi_st)
        setattr(ph, field, value)
        assert call(phi=ph) in (-2, -3), field
    os.environ["NOCF_LANE"] = "0"
    try:
        _lib.lib()                                              # (NOCF_ENV_WATCH: the library re-reads its knobs)
        assert call() == -2
    finally:
        del os.environ["NOCF_LANE"]
        _lib.lib()
    assert call() == 0
    torch.cuda.synchronize()


def _run_driver(argv, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("trainOC_under_test", os.path.join(REPO, "trainOC.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    capsys.readouterr()
    mod.main(argv)
    return capsys.readouterr().out.splitlines()


def test_driver_members(tmp_path, capsys):
    from neuraloc_amd.checkpoint import load_checkpoint
    common = ["--data", "softcorridor", "--m", "16", "--nt", "4", "--niters", "3", "--n_train", "32", "--val_freq", "2", "--seed", "5",
              "--alph", "100.0, 10000.0, 300.0, 0.25, 0.25, 0.25"]
    rows = tmp_path / "alph.txt"
    rows.write_text("100.0, 10000.0, 300.0, 0.25, 0.25, 0.25\n50.0, 5000.0, 0.0, 0.5, 0.25, 0.125\n")
    ens_out = _run_driver(common + ["--members", "2", "--members_alph", str(rows), "--save", str(tmp_path / "ens")], capsys)
    one_out = _run_driver(common + ["--save", str(tmp_path / "one")], capsys)
    first_m0 = next(ln for ln in ens_out if ln.startswith("m0 ") and ln.split()[1] == "00001")
    first_m1 = next(ln for ln in ens_out if ln.startswith("m1 ") and ln.split()[1] == "00001")
    first_one = next(ln for ln in one_out if ln.split() and ln.split()[0] == "00001")
    # the usual line prefixed by the member; the third column of it is wall-clock time
    strip = lambda cols: cols[:2] + cols[3:]                   # noqa: E731
    assert strip(first_m0.split()[1:]) == strip(first_one.split())
    assert strip(first_m1.split()[1:]) != strip(first_one.split())
    assert sum(ln.startswith("m0 ") for ln in ens_out) == 3 + 1 and sum(ln.startswith("m1 ") for ln in ens_out) == 3 + 1     # header line + 3
    files = sorted(os.listdir(tmp_path / "ens"))
    assert len(files) == 2 and files[0].endswith("_m0_checkpt.pth") and files[1].endswith("_m1_checkpt.pth")
    for f, want in zip(files, ("10000.0", "5000.0")):
        net, prob, x0, x0v, xInit, a = load_checkpoint(str(tmp_path / "ens" / f), device=DEV, n_train=8, n_val=8)
        assert isinstance(net, na.Phi) and net.m == 16 and float(prob.alph_Q) == float(want)
        with torch.no_grad():
            Jc, _ = na.OCflow(x0, net, prob, [0.0, 1.0], 4, "rk4", net.alph)
        assert bool(torch.isfinite(Jc))
