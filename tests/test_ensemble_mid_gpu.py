"""Ensembles on the one-CU kernels, on the MI355X: member e of one ensemble launch (family="mid") against the single-network call on that
member alone -- bit for bit, forward, recording forward and gradients, at every instantiation (cases and shapes: tests/util_ensemble_mid.py).
Nothing here carries a tolerance: the ensemble kernels run the single-network statements on the member's blocks."""
import contextlib
import ctypes as C
import dataclasses
import os

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, ensemble
from neuraloc_amd.OCflow import _launch as single_launch
from neuraloc_amd.train import _STEPPERS, ocflow_train

import util_ensemble_mid as uem
import util_mono as um

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024
FWD, REC, BWD = "rollout_mono_kernel", "rollout_mono_kernel", "rollout_mono_bwd_kernel"
GJ = [1.0, 0.5, -2.0]


def _kernel():
    return _lib.lib().nocf_last_rollout_kernel().decode()


def _guarded(*shape):
    """a NaN-filled buffer with GUARD floats on either side of a tensor of `shape` -> (buffer, the view in the middle)"""
    count = 1
    for v in shape:
        count *= v
    buf = torch.full((count + 2 * GUARD,), float("nan"), device=DEV)
    return buf, buf[GUARD:GUARD + count].view(*shape)


def _guards_intact(guards, bufs):
    for key, g in guards.items():
        mid = bufs[key].numel()
        assert bool(g[:GUARD].isnan().all()) and bool(g[GUARD + mid:].isnan().all()), key


def _setup(case, members=uem.E, first=0, n=None):
    nets = uem.member_nets(case, DEV, members, first)
    rows = uem.member_rows(members, first)
    ens = na.PhiEnsemble.from_members(nets, alph=rows)
    x = uem.starts(case, members, n=n, first=first).to(DEV)
    prob = uem.member_problem(case, 0, DEV, first)         # (its alph_Q / alph_W are not read by an ensemble call)
    return ens, rows, x, prob


def _member_x(case, x, e):
    return (x[e] if case.own_x else x[0]).contiguous()


def _cdim(b):
    return 4 * b.n_agents if b.kind == "quad" else b.d


def _act_floats(b, n):
    """(floats of the single-network record, the ensemble's member stride)"""
    nact = int(_lib.lib().nocf_activation_record_floats(b.d, b.m, 2, n, b.nt, _STEPPERS[b.stepper]))
    return nact, (nact + 3) // 4 * 4


def _single_record(net, prob, x, b, alph):
    """nocf_rollout_record_act_f32 on one network: what ocflow_train's forward calls -> dict persample, z_out, sums, s_all, act, recorded"""
    n, d = x.shape
    L = _lib.lib()
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(torch.device(DEV))
    nstage = 4 if b.stepper == "rk4" else 1
    nact, _ = _act_floats(b, n)
    out = dict(persample=torch.empty(n, 7, device=DEV), z_out=torch.empty(n, d + 4, device=DEV), sums=torch.empty(8, device=DEV),
               s_all=torch.empty(b.nt * nstage, n, d + 1, device=DEV), act=torch.full((nact,), float("nan"), device=DEV) if nact else None)
    recorded = C.c_int32(0)
    alph_c = (C.c_float * 6)(*[float(a) for a in alph[:6]])
    with torch.cuda.device(DEV):
        rc = L.nocf_rollout_record_act_f32(C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), n, float(b.tspan[0]), float(b.tspan[1]), int(b.nt),
                                           _STEPPERS[b.stepper], alph_c, _lib.ptr(out["z_out"]), _lib.ptr(out["persample"]), _lib.ptr(out["sums"]),
                                           _lib.ptr(out["s_all"]), _lib.ptr(out["act"]), C.byref(recorded),
                                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr(torch.device(DEV)))
    assert rc == 0
    out["recorded"] = bool(recorded.value)
    return out


@pytest.mark.parametrize("case", uem.FORWARD, ids=lambda c: c.id)
def test_evaluation_members_equal_the_single_network_call(case):
    b = case.base
    E, n, d, nt = uem.E, b.n, b.d, b.nt
    ens, rows, x, prob = _setup(case)
    xe = x if case.own_x else x[0]
    cdim = _cdim(b)
    bufs, guards = {}, {}
    for key, shape in (("persample", (E, n, 7)), ("z_out", (E, n, d + 4)), ("sums", (E, 8)), ("means", (E, 8)),
                       ("zFull", (E, nt + 1, n, d + 4)), ("ctrlFull", (E, nt + 1, n, cdim))):
        guards[key], bufs[key] = _guarded(*shape)
    with torch.no_grad():
        out = ensemble._launch_mid(xe, ens, prob, b.tspan, nt, b.stepper, None, intermediates=True, bufs=bufs)
        assert _kernel() == "rollout_mono_kernel<ens>"
        Jc, cs = na.ensemble_rollout(xe, ens, prob, b.tspan, nt, b.stepper, family="mid")
        assert _kernel() == "rollout_mono_kernel<ens>"
        Jc2, cs2, traj, ctrl = na.ensemble_rollout(xe, ens, prob, b.tspan, nt, b.stepper, intermediates=True, family="mid")
    torch.cuda.synchronize()
    _guards_intact(guards, bufs)                                # nothing outside the stated rows is written, every stated row is
    for key in guards:
        assert bool(torch.isfinite(out[key]).all()), key
    assert tuple(Jc.shape) == (E,) and tuple(cs.shape) == (E, 7)
    assert tuple(traj.shape) == (E, n, d + 4, nt + 1) and tuple(ctrl.shape) == (E, n, cdim, nt + 1)
    assert torch.equal(Jc, out["means"][:, 7]) and torch.equal(cs, out["means"][:, :7]) and torch.equal(Jc2, Jc) and torch.equal(cs2, cs)
    assert torch.equal(traj, out["zFull"].permute(0, 2, 3, 1)) and torch.equal(ctrl, out["ctrlFull"].permute(0, 2, 3, 1))
    differ = 0
    for e in range(E):
        net, pe, x1 = ens.member(e), uem.member_problem(case, e, DEV), _member_x(case, x, e)
        assert (pe.alph_Q, pe.alph_W) == (rows[e][1], rows[e][2]) and net.alph == rows[e]
        with torch.no_grad():
            means = torch.empty(8, device=DEV)
            tab, sums, zF1, cF1 = single_launch(x1, net, pe, list(b.tspan), nt, b.stepper, rows[e], True, means)
            assert _kernel() == FWD                             # the yardstick ran the single-network one-CU kernel
            J1, c1 = na.OCflow(x1, net, pe, list(b.tspan), nt, b.stepper, rows[e])
            assert _kernel() == FWD
            t1, u1 = na.OCflow(x1, net, pe, list(b.tspan), nt, b.stepper, rows[e], intermediates=True)
        assert torch.equal(out["persample"][e], tab), e
        assert torch.equal(out["z_out"][e], zF1[nt]), e
        assert torch.equal(out["sums"][e], sums), e
        assert torch.equal(out["means"][e], means), e
        assert torch.equal(out["zFull"][e], zF1) and torch.equal(out["ctrlFull"][e], cF1), e
        assert torch.equal(Jc[e], J1) and torch.equal(cs[e], torch.stack(c1)), e
        assert torch.equal(traj[e], t1) and torch.equal(ctrl[e], u1), e
        differ += int(not torch.equal(out["persample"][e], out["persample"][0]))
    assert differ == E - 1                                      # the members are different networks: a launch that read member 0 thrice fails
    # the want_W decision differs between the members: no interaction cost where alph_W = 0, one where it is not
    if b.n_agents >= 2:
        assert bool((out["persample"][1, :, 6] == 0).all()) and bool((out["persample"][0, :, 6] != 0).any())


@pytest.mark.parametrize("case", uem.FORWARD, ids=lambda c: c.id)
def test_recording_forward_members_equal_the_single_network_call(case):
    b = case.base
    E, n, d, nt = uem.E, b.n, b.d, b.nt
    nstage = 4 if b.stepper == "rk4" else 1
    ens, rows, x, prob = _setup(case)
    xe = x if case.own_x else x[0]
    nact, stride = _act_floats(b, n)
    assert (nact > 0) == um.mono_record_eligible(2, b.m, d, b.r, b.n_agents)
    bufs, guards = {}, {}
    for key, shape in (("persample", (E, n, 7)), ("z_out", (E, n, d + 4)), ("sums", (E, 8)), ("s_all", (E, nt * nstage, n, d + 1))) \
            + ((("act", (E, stride)),) if nact else ()):
        guards[key], bufs[key] = _guarded(*shape)
    out = ensemble._launch_mid(xe, ens, prob, b.tspan, nt, b.stepper, None, record=True, bufs=bufs)
    assert _kernel() == "rollout_mono_kernel<ens>"
    torch.cuda.synchronize()
    _guards_intact(guards, bufs)
    assert out["recorded"] == (nact > 0) and (out["act"] is not None) == (nact > 0)
    for key in ("persample", "z_out", "sums", "s_all"):
        assert bool(torch.isfinite(out[key]).all()), key
    trainable = b.m > 32
    if trainable:
        Jc, cs = na.ensemble_ocflow_train(xe, ens, prob, b.tspan, nt, b.stepper, family="mid")
        assert _kernel() == "rollout_mono_kernel<ens>"
        assert torch.equal(cs, out["sums"][:, :7] / out["sums"][:, 7:8])
    else:
        with pytest.raises(ValueError, match="32 < m"):
            na.ensemble_ocflow_train(xe, ens, prob, b.tspan, nt, b.stepper, family="mid")
    for e in range(E):
        net, pe, x1 = ens.member(e), uem.member_problem(case, e, DEV), _member_x(case, x, e)
        one = _single_record(net, pe, x1, b, rows[e])
        assert _kernel() == REC
        for key in ("persample", "z_out", "sums", "s_all"):
            assert torch.equal(out[key][e], one[key]), (e, key)
        assert one["recorded"] == out["recorded"]
        if nact:
            assert torch.equal(out["act"][e, :nact], one["act"]), e
            assert bool(out["act"][e, nact:].isnan().all())     # (the padding up to whole 16-byte pieces is not written)
        if trainable:
            J1, c1 = ocflow_train(x1, net, pe, list(b.tspan), nt, b.stepper, rows[e])
            assert _kernel() == REC
            assert torch.equal(Jc[e].detach(), J1.detach()) and torch.equal(cs[e], torch.stack(c1)), e


@pytest.mark.parametrize("own", [False, True])
def test_whole_tiles_no_tail(own):
    """n = 16: every member is exactly one tile"""
    case = dataclasses.replace(uem.FORWARD[2], own_x=own)
    b = case.base
    ens, rows, x, prob = _setup(case, n=16)
    xe = x if own else x[0]
    with torch.no_grad():
        out = ensemble._launch_mid(xe, ens, prob, b.tspan, b.nt, b.stepper, None, intermediates=True)
        for e in range(uem.E):
            net, pe, x1 = ens.member(e), uem.member_problem(case, e, DEV), _member_x(case, x, e)
            means = torch.empty(8, device=DEV)
            tab, sums, zF1, cF1 = single_launch(x1, net, pe, list(b.tspan), b.nt, b.stepper, rows[e], True, means)
            assert torch.equal(out["persample"][e], tab) and torch.equal(out["means"][e], means), e
            assert torch.equal(out["zFull"][e], zF1) and torch.equal(out["ctrlFull"][e], cF1), e


def test_one_member_one_row_equals_the_plain_call():
    case = uem.FORWARD[0]                                       # singlequad's shape
    b = case.base
    ens, rows, x, prob = _setup(case, members=1)
    x1 = x[0, :1].contiguous()
    net, pe = ens.member(0), uem.member_problem(case, 0, DEV)
    with torch.no_grad():
        Jc, cs, traj, ctrl = na.ensemble_rollout(x1, ens, prob, b.tspan, b.nt, b.stepper, intermediates=True, family="mid")
        assert _kernel() == "rollout_mono_kernel<ens>"
        J1, c1 = na.OCflow(x1, net, pe, list(b.tspan), b.nt, b.stepper, rows[0])
        assert _kernel() == FWD
        t1, u1 = na.OCflow(x1, net, pe, list(b.tspan), b.nt, b.stepper, rows[0], intermediates=True)
        Jo, co = na.ensemble_rollout(x1[None], ens, prob, b.tspan, b.nt, b.stepper, family="mid")        # the same row as the member's own
    assert torch.equal(Jc[0], J1) and torch.equal(cs[0], torch.stack(c1)) and torch.equal(traj[0], t1) and torch.equal(ctrl[0], u1)
    assert torch.equal(Jo, Jc) and torch.equal(co, cs)


@pytest.mark.parametrize("own", [False, True])
def test_a_member_does_not_depend_on_its_position(own):
    """the member at index 2 of E = 3 is the member at index 0 of E = 7, bitwise"""
    case = uem.FORWARD[4]
    b = case.base
    nets3, rows3 = uem.member_nets(case, DEV, 3), uem.member_rows(3)
    nets7 = [nets3[2]] + uem.member_nets(case, DEV, 6, first=3)
    rows7 = [rows3[2]] + uem.member_rows(6, first=3)
    e3, e7 = na.PhiEnsemble.from_members(nets3, alph=rows3), na.PhiEnsemble.from_members(nets7, alph=rows7)
    x3 = uem.starts(case, 3).to(DEV)
    x7 = torch.cat([x3[2:3], uem.starts(case, 6, first=3).to(DEV)])
    prob = uem.member_problem(case, 0, DEV)
    with torch.no_grad():
        o3 = ensemble._launch_mid(x3 if own else x3[2], e3, prob, b.tspan, b.nt, b.stepper, None, intermediates=True)
        o7 = ensemble._launch_mid(x7 if own else x3[2], e7, prob, b.tspan, b.nt, b.stepper, None, intermediates=True)
    for key in ("persample", "z_out", "sums", "means", "zFull", "ctrlFull"):
        assert torch.equal(o3[key][2], o7[key][0]), key
    assert not torch.equal(o3["persample"][0], o7["persample"][1])


@contextlib.contextmanager
def _saved(into):
    """collects the tensors an autograd.Function saves for its backward (the recorded stage inputs and the final states)"""
    def pack(t):
        into.append(t)
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        yield


def _single_train(case, ens, rows, x, e, gj):
    """ocflow_train + backward() on member e alone -> (Jc, cs, s_all, {name: grad}, x.grad)"""
    b = case.base
    net, pe = ens.member(e), uem.member_problem(case, e, DEV)
    x1 = _member_x(case, x, e).clone().requires_grad_(case.own_x)
    saved = []
    with _saved(saved):
        J1, c1 = ocflow_train(x1, net, pe, list(b.tspan), b.nt, b.stepper, rows[e])
    assert _kernel() == REC
    (gj * J1).backward()
    assert _kernel() == BWD
    s_all = next(t for t in saved if t.dim() == 3)
    return J1.detach(), torch.stack(c1), s_all, {k: p.grad for k, p in net.named_parameters()}, x1.grad


@pytest.mark.parametrize("case", uem.TRAIN, ids=lambda c: c.id)
def test_training_members_equal_the_single_network_adjoint(case):
    b = case.base
    E, n, d = uem.E, b.n, b.d
    ens, rows, x, prob = _setup(case)
    gJ = torch.tensor(GJ, device=DEV)
    xe = x.clone().requires_grad_(True)
    saved = []
    with _saved(saved):
        Jc, cs = na.ensemble_ocflow_train(xe, ens, prob, b.tspan, b.nt, b.stepper, family="mid")
    assert _kernel() == "rollout_mono_kernel<ens>"
    assert tuple(Jc.shape) == (E,) and tuple(cs.shape) == (E, 7) and Jc.requires_grad and not cs.requires_grad
    (gJ * Jc).sum().backward()
    assert _kernel() == "rollout_mono_bwd_kernel<ens>"
    s_all = next(t for t in saved if t.dim() == 4)
    nstage = 4 if b.stepper == "rk4" else 1
    assert tuple(s_all.shape) == (E, b.nt * nstage, n, d + 1)
    for e in range(E):
        J1, c1, s1, g1, gx1 = _single_train(case, ens, rows, x, e, gJ[e])
        assert torch.equal(Jc[e].detach(), J1) and torch.equal(cs[e], c1), e
        assert torch.equal(s_all[e], s1), e
        assert torch.equal(xe.grad[e], gx1), e
        for name, p in ens.named_parameters():
            assert p.grad is not None and torch.equal(p.grad[e], g1[name]), (e, name)
    assert all(bool((p.grad[e] != 0).any()) for e in range(E) for _, p in ens.named_parameters())


@pytest.mark.parametrize("case", [uem.TRAIN[2], uem.TRAIN[5]], ids=lambda c: c.id)       # m % 16 == 0: the record is read; m = 33: recomputed
def test_two_adam_steps_equal_three_separate_optimisers(case):
    b = case.base
    E = uem.E
    ens, rows, x, prob = _setup(case)
    fresh = ens.A.detach().clone()
    xs = x[0].contiguous()
    nets = [ens.member(e) for e in range(E)]
    probs = [uem.member_problem(case, e, DEV) for e in range(E)]
    opt = torch.optim.Adam(ens.parameters(), lr=0.01)
    opts = [torch.optim.Adam(q.parameters(), lr=0.01) for q in nets]
    for _ in range(2):
        opt.zero_grad()
        Jc, _ = na.ensemble_ocflow_train(xs, ens, prob, b.tspan, b.nt, b.stepper, family="mid")
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
    assert not torch.equal(ens.A, fresh)                        # the steps moved the weights


def test_capped_adjoint_grid_walks_the_members_tiles():
    """E = 2 members of more than 1024 tiles: workgroup j of member e walks tiles j, j + 1024 of THAT member"""
    case = uem.CAPPED
    b = case.base
    E = 2
    ens, rows, x, prob = _setup(case, members=E)
    xs = x[0].contiguous()
    assert um.cdiv(b.n, 16) > um.mid_grad_rows(b.n) == 1024
    Jc, cs = na.ensemble_ocflow_train(xs, ens, prob, b.tspan, b.nt, b.stepper, family="mid")
    Jc.sum().backward()
    assert _kernel() == "rollout_mono_bwd_kernel<ens>"
    for e in range(E):
        net, pe = ens.member(e), uem.member_problem(case, e, DEV)
        J1, c1 = ocflow_train(xs, net, pe, list(b.tspan), b.nt, b.stepper, rows[e])
        J1.backward()
        assert _kernel() == BWD
        assert torch.equal(Jc[e].detach(), J1.detach()) and torch.equal(cs[e], torch.stack(c1)), e
        for (name, p), (_, q) in zip(ens.named_parameters(), net.named_parameters()):
            assert torch.equal(p.grad[e], q.grad), (e, name)


def test_the_abi_refuses_before_anything_is_enqueued():
    case = uem.TRAIN[5]
    b = case.base
    E, n, d, nt = uem.E, b.n, b.d, b.nt
    dev = torch.device(DEV)
    ens, rows, x, prob = _setup(case)
    L, (f_eval, f_rec, f_bwd) = ensemble._shipped_mid()
    phi_st, keep = ens._c_struct()
    prob_st, keep2 = prob._c_struct(dev)
    table = ens.alph_table()
    nbytes = int(L.nocf_mid_ensemble_workspace_bytes(d, b.m, 2, b.r, E))
    assert nbytes > 0 and nbytes % E == 0
    assert int(L.nocf_mid_ensemble_workspace_bytes(d, 129, 2, b.r, E)) == 0 and int(L.nocf_mid_ensemble_workspace_bytes(d, b.m, 3, b.r, E)) == 0
    assert int(L.nocf_mid_ensemble_workspace_bytes(d, b.m, 2, b.r, 0)) == 0
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    tab, sums = torch.full((E, n, 7), float("nan"), device=DEV), torch.full((E, 8), float("nan"), device=DEV)
    s_all, z_out = torch.full((E, nt * 4, n, d + 1), float("nan"), device=DEV), torch.full((E, n, d + 4), float("nan"), device=DEV)
    P = int(L.nocf_small_grad_floats(d, b.m))
    grows = int(L.nocf_mid_grad_rows(d, b.m, 2, b.r, b.n_agents, n))
    gpart = torch.full((E, grows, P), float("nan"), device=DEV)
    hs = torch.full((nt,), 1.0 / nt, device=DEV)

    def ev(members=E, stride=0, phi=phi_st, pr=prob_st, wbytes=nbytes):
        return f_eval(C.byref(phi), C.byref(pr), _lib.ptr(x), n, members, stride, 0.0, 1.0, nt, _lib.NOCF_RK4, _lib.ptr(table),
                      None, _lib.ptr(tab), _lib.ptr(sums), None, None, None, _lib.ptr(ws), wbytes, _lib.stream_ptr(dev))

    def rec(members=E, stride=0, phi=phi_st, wbytes=nbytes):
        return f_rec(C.byref(phi), C.byref(prob_st), _lib.ptr(x), n, members, stride, 0.0, 1.0, nt, _lib.NOCF_RK4, _lib.ptr(table),
                     _lib.ptr(z_out), _lib.ptr(tab), _lib.ptr(sums), _lib.ptr(s_all), None, None, _lib.ptr(ws), wbytes, _lib.stream_ptr(dev))

    def bwd(members=E, phi=phi_st, pr=prob_st, wbytes=nbytes, rows_=grows):
        return f_bwd(C.byref(phi), C.byref(pr), n, members, nt, _lib.NOCF_RK4, 1.0, _lib.ptr(table), 1.0 / n, _lib.ptr(s_all), _lib.ptr(z_out),
                     _lib.ptr(hs), None, _lib.ptr(gpart), rows_, None, _lib.ptr(ws), wbytes, _lib.stream_ptr(dev))

    # a workspace that is too small: NOCF_E_WORKSPACE, and nothing is written -- not the outputs, not the workspace
    assert ev(wbytes=nbytes - 1) == -4 and rec(wbytes=nbytes - 1) == -4 and bwd(wbytes=nbytes - 1) == -4 and bwd(rows_=grows + 1) == -4
    torch.cuda.synchronize()
    assert bool(tab.isnan().all()) and bool(sums.isnan().all()) and bool(s_all.isnan().all()) and bool(z_out.isnan().all())
    assert bool(gpart.isnan().all()) and bool((ws == 0).all())
    # members, strides, the row count
    for call in (ev, rec, bwd):
        assert call(members=0) == -2 and call(members=2 ** 31 // n + 1) == -2, call.__name__
    for call in (ev, rec):
        assert call(stride=d) == -2 and call(stride=n * d + 1) == -2, call.__name__
    # shapes without a one-CU plan; the adjoint: without an adjoint instantiation (m <= 32)
    for field, value in (("nTh", 3), ("m", 129), ("r", 17)):
        ph = _lib.NocfPhi.from_buffer_copy(phi_st)
        setattr(ph, field, value)
        for call in (ev, rec, bwd):
            assert call(phi=ph) == -2, (field, call.__name__)
    ph = _lib.NocfPhi.from_buffer_copy(phi_st)
    ph.m = 32
    assert bwd(phi=ph) == -2
    # c.bias is read on the device
    ph = _lib.NocfPhi.from_buffer_copy(phi_st)
    ph.cb_dev = None
    for call in (ev, rec, bwd):
        assert call(phi=ph) == -1, call.__name__
    os.environ["NOCF_MONO"] = "0"
    try:
        _lib.lib()                                              # (NOCF_ENV_WATCH: the library re-reads its knobs)
        assert ev() == -2 and rec() == -2 and bwd() == -2
    finally:
        del os.environ["NOCF_MONO"]
        _lib.lib()
    torch.cuda.synchronize()
    assert bool(tab.isnan().all()) and bool(gpart.isnan().all()) and bool((ws == 0).all())       # every refusal above came before a launch
    # ... and the accepted calls
    assert ev() == 0 and ev(stride=n * d) == 0 and rec() == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(tab).all()) and bool(torch.isfinite(gpart).all())


def _run_driver(argv, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("trainOC_under_test", os.path.join(REPO, "trainOC.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    capsys.readouterr()
    mod.main(argv)
    return capsys.readouterr().out.splitlines()


def test_driver_members_family_mid_singlequad(tmp_path, capsys):
    from neuraloc_amd.checkpoint import load_checkpoint
    common = ["--data", "singlequad", "--m", "64", "--nt", "4", "--niters", "2", "--n_train", "32", "--val_freq", "2", "--seed", "5"]
    ens_out = _run_driver(common + ["--members", "2", "--members_family", "mid", "--save", str(tmp_path / "ens")], capsys)
    assert _kernel() == "rollout_mono_kernel<ens>"              # (the last launch: the validation rollout)
    one_out = _run_driver(common + ["--save", str(tmp_path / "one")], capsys)
    first_m0 = next(ln for ln in ens_out if ln.startswith("m0 ") and ln.split()[1] == "00001")
    first_m1 = next(ln for ln in ens_out if ln.startswith("m1 ") and ln.split()[1] == "00001")
    first_one = next(ln for ln in one_out if ln.split() and ln.split()[0] == "00001")
    # the usual line prefixed by the member; the third column of it is wall-clock time
    strip = lambda cols: cols[:2] + cols[3:]                   # noqa: E731
    assert strip(first_m0.split()[1:]) == strip(first_one.split())
    assert strip(first_m1.split()[1:]) != strip(first_one.split())
    files = sorted(os.listdir(tmp_path / "ens"))
    assert len(files) == 2 and files[0].endswith("_m0_checkpt.pth") and files[1].endswith("_m1_checkpt.pth")
    for f in files:
        net, prob, x0, x0v, xInit, a = load_checkpoint(str(tmp_path / "ens" / f), device=DEV, n_train=8, n_val=8)
        assert isinstance(net, na.Phi) and net.m == 64 and isinstance(prob, na.Quadcopter)
        with torch.no_grad():
            Jc, _ = na.OCflow(x0, net, prob, [0.0, 1.0], 4, "rk4", net.alph)
        assert bool(torch.isfinite(Jc))
