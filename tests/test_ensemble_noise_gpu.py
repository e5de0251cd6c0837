"""Ensembles under in-kernel Brownian noise, on the MI355X: member e of one noisy ensemble launch against noisy_rollout / noisy_ocflow_train on
that member alone with its sigma row, seed, mask and row offset -- bit for bit, evaluation, recording forward and gradients, at every
instantiation of both families (cases: tests/util_ensemble_noise.py).  Nothing here carries a tolerance: the kernels run the single-network
DIST == 2 statements on the member's blocks, scale row and seed.  Every comparison is torch.equal."""
import contextlib
import ctypes as C
import os

import pytest
import torch

import neuraloc_amd as na
from neuraloc_amd import _lib, ensemble, ensemble_noise, noise
from neuraloc_amd.train import _STEPPERS

import util_ensemble_noise as uen

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024
E = uen.E
GJ = [1.0, 0.5, -2.0]
ENS_KERNEL = {"lane": "rollout_lane_kernel<ens,noisy>", "mid": "rollout_mono_kernel<ens,noisy>"}
ONE_KERNEL = {"lane": "rollout_lane_kernel<noise>", "mid": "rollout_mono_kernel<noise>"}
ENS_BWD = {"lane": "rollout_lane_bwd_kernel<ens>", "mid": "rollout_mono_bwd_kernel<ens>"}
ONE_BWD = {"lane": "rollout_lane_bwd_kernel", "mid": "rollout_mono_bwd_kernel"}


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


def _setup(nc, members=E, n=None):
    u, case = nc.util, nc.case
    nets = u.member_nets(case, DEV, members)
    rows = u.member_rows(members)
    ens = na.PhiEnsemble.from_members(nets, alph=rows)
    x = (u.starts(case, members) if n is None else u.starts(case, members, n=n)).to(DEV)
    prob = u.member_problem(case, 0, DEV)                       # (its alph_Q / alph_W are not read by an ensemble call)
    return ens, rows, x, prob


def _member_x(nc, x, e):
    return (x[e] if nc.own_x else x[0]).contiguous()


def _cdim(b):
    return 4 * b.n_agents if getattr(b, "kind", "") == "quad" else b.d


def _noise_of(nc, members=E, sigma=None, seed=None, row_offset=None):
    b = nc.base
    return ensemble_noise._Noise(ensemble_noise.scale_table(nc.sigma if sigma is None else sigma, members, b.nt, b.d, b.tspan, nc.mask),
                                 ensemble_noise.seed_list(nc.seed if seed is None else seed, members),
                                 nc.row_offset if row_offset is None else row_offset)


def _launch(nc, xe, ens, prob, **kw):
    """the ensemble launch of the case's family -> its buffers, MEMBER-MAJOR views for both families (the lane family's are time-major over
    E * n rows: member e's block is rows [e n, (e + 1) n))"""
    b = nc.base
    fn = ensemble._launch if nc.family == "lane" else ensemble._launch_mid
    return fn(xe, ens, prob, b.tspan, b.nt, b.stepper, None, **kw)


def _member(nc, out, key, e, n):
    """member e's block of buffer `key` in the single-network layout"""
    t = out[key]
    if nc.family == "mid" or key in ("sums", "means"):
        return t[e]
    if key in ("persample", "z_out"):
        return t[e * n:(e + 1) * n]
    return t[:, e * n:(e + 1) * n]                              # zFull, ctrlFull, s_all: time-major


def _shapes(nc, n, record):
    b = nc.base
    d, nt = b.d, b.nt
    nstage = 4 if b.stepper == "rk4" else 1
    if nc.family == "lane":
        s = {"persample": (E * n, 7), "z_out": (E * n, d + 4), "sums": (E, 8)}
        s.update({"s_all": (nt * nstage, E * n, d + 1)} if record else
                 {"means": (E, 8), "zFull": (nt + 1, E * n, d + 4), "ctrlFull": (nt + 1, E * n, _cdim(b))})
    else:
        s = {"persample": (E, n, 7), "z_out": (E, n, d + 4), "sums": (E, 8)}
        s.update({"s_all": (E, nt * nstage, n, d + 1)} if record else
                 {"means": (E, 8), "zFull": (E, nt + 1, n, d + 4), "ctrlFull": (E, nt + 1, n, _cdim(b))})
    return s


def _single(nc, net, prob, x, alph, sigma, seed, record):
    """nocf_rollout_noisy_f32 (or nocf_rollout_record_noisy_f32 with record) on one network, called as noisy_rollout / noisy_ocflow_train call
    it, into NaN-guarded buffers -> dict of the buffers (+ "recorded")"""
    b = nc.base
    n, d = x.shape
    dev = torch.device(DEV)
    L = _lib.lib()
    phi_st, keep1, ws = net._c_struct(n)
    prob_st, keep2 = prob._c_struct(dev)
    scale = noise.noise_scale(sigma, b.nt, d, b.tspan, nc.mask).to(DEV)
    nstage = 4 if b.stepper == "rk4" else 1
    alph_c = (C.c_float * 6)(*[float(a) for a in alph[:6]])
    guards, out = {}, {}
    shapes = {"persample": (n, 7), "z_out": (n, d + 4), "sums": (8,)}
    nact = 0
    if record:
        shapes["s_all"] = (b.nt * nstage, n, d + 1)
        nact = int(L.nocf_activation_record_floats(d, b.m, 2, n, b.nt, _STEPPERS[b.stepper])) if nc.family == "mid" else 0
        if nact:
            shapes["act"] = (nact,)
    else:
        shapes.update({"means": (8,), "zFull": (b.nt + 1, n, d + 4), "ctrlFull": (b.nt + 1, n, _cdim(b))})
    for key, shape in shapes.items():
        guards[key], out[key] = _guarded(*shape)
    head = (C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), _lib.ptr(scale), seed, nc.row_offset, n,
            float(b.tspan[0]), float(b.tspan[1]), int(b.nt), _STEPPERS[b.stepper], alph_c)
    tail = (_lib.ptr(ws), ws.numel() * ws.element_size(), _lib.stream_ptr(dev))
    with torch.cuda.device(dev):
        if record:
            recorded = C.c_int32(0)
            f = noise._entry(L, "nocf_rollout_record_noisy_f32")
            rc = f(*head, _lib.ptr(out["z_out"]), _lib.ptr(out["persample"]), _lib.ptr(out["sums"]), _lib.ptr(out["s_all"]),
                   _lib.ptr(out.get("act")), C.byref(recorded), *tail)
            out["recorded"] = bool(recorded.value)
        else:
            f = noise._entry(L, "nocf_rollout_noisy_f32")
            rc = f(*head, _lib.ptr(out["z_out"]), _lib.ptr(out["persample"]), _lib.ptr(out["sums"]), _lib.ptr(out["means"]),
                   _lib.ptr(out["zFull"]), _lib.ptr(out["ctrlFull"]), *tail)
    assert rc == 0
    assert _kernel() == ONE_KERNEL[nc.family]                   # the yardstick ran the single-network kernel of the same family
    torch.cuda.synchronize()
    _guards_intact(guards, out)
    return out


# ---- 1. evaluation
@pytest.mark.parametrize("nc", uen.FORWARD, ids=lambda c: c.id)
def test_evaluation_members_equal_noisy_rollout_on_the_member(nc):
    b = nc.base
    n, d, nt = b.n, b.d, b.nt
    ens, rows, x, prob = _setup(nc)
    xe = x if nc.own_x else x[0]
    bufs, guards = {}, {}
    for key, shape in _shapes(nc, n, False).items():
        guards[key], bufs[key] = _guarded(*shape)
    kw = dict(mask=nc.mask, row_offset=nc.row_offset, family=nc.family)
    with torch.no_grad():
        out = _launch(nc, xe, ens, prob, intermediates=True, bufs=bufs, noise=_noise_of(nc))
        assert _kernel() == ENS_KERNEL[nc.family]
        Jc, cs = na.ensemble_noisy_rollout(xe, ens, prob, b.tspan, nt, nc.sigma, nc.seed, b.stepper, **kw)
        assert _kernel() == ENS_KERNEL[nc.family]
        Jc2, cs2, traj, ctrl = na.ensemble_noisy_rollout(xe, ens, prob, b.tspan, nt, nc.sigma, nc.seed, b.stepper, intermediates=True, **kw)
    torch.cuda.synchronize()
    _guards_intact(guards, bufs)                                # nothing outside the stated rows is written, every stated row is
    for key in guards:
        assert bool(torch.isfinite(out[key]).all()), key
    assert tuple(Jc.shape) == (E,) and tuple(cs.shape) == (E, 7)
    assert tuple(traj.shape) == (E, n, d + 4, nt + 1) and tuple(ctrl.shape) == (E, n, _cdim(b), nt + 1)
    assert torch.equal(Jc, out["means"][:, 7]) and torch.equal(cs, out["means"][:, :7]) and torch.equal(Jc2, Jc) and torch.equal(cs2, cs)
    for e in range(E):
        net, pe, x1 = ens.member(e), nc.util.member_problem(nc.case, e, DEV), _member_x(nc, x, e)
        sg, sd = uen.member_sigma(nc.sigma, e), nc.member_seed(e)
        with torch.no_grad():
            one = _single(nc, net, pe, x1, rows[e], sg, sd, record=False)
            ref = na.noisy_rollout(x1, net, pe, nt, sg, sd, tspan=b.tspan, alph=rows[e], stepper=b.stepper, intermediates=True,
                                   mask=nc.mask, row_offset=nc.row_offset)
            assert _kernel() == ONE_KERNEL[nc.family]
        for key in ("persample", "z_out", "sums", "means", "zFull", "ctrlFull"):
            assert torch.equal(_member(nc, out, key, e, n), one[key]), (e, key)
        assert torch.equal(Jc[e], ref["Jc"]) and torch.equal(cs[e], torch.stack(ref["cs"])), e
        assert torch.equal(_member(nc, out, "persample", e, n), ref["persample"]) and torch.equal(_member(nc, out, "z_out", e, n), ref["z_final"]), e
        assert torch.equal(traj[e], ref["traj"]) and torch.equal(ctrl[e], ref["ctrl"]), e


# ---- 2. not vacuous
@pytest.mark.parametrize("nc", [uen.first(uen.FORWARD, "lane", isigma=1), uen.first(uen.FORWARD, "mid", isigma=1)], ids=lambda c: c.id)
def test_a_positive_level_moves_a_member_and_level_zero_does_not(nc):
    b = nc.base
    n = b.n
    assert [row[0] > 0 for row in nc.sigma] == [True, False, True]
    ens, rows, x, prob = _setup(nc)
    xe = x if nc.own_x else x[0]
    with torch.no_grad():
        noisy = _launch(nc, xe, ens, prob, intermediates=True, noise=_noise_of(nc))
        plain = _launch(nc, xe, ens, prob, intermediates=True)
        assert _kernel() == ENS_KERNEL[nc.family].replace(",noisy", "")
    for e in range(E):
        same = [torch.equal(_member(nc, noisy, key, e, n), _member(nc, plain, key, e, n))
                for key in ("persample", "z_out", "sums", "means", "zFull", "ctrlFull")]
        assert same == [nc.sigma[e][0] == 0] * 6, (e, same)


# ---- 3. recording forward and gradients
@contextlib.contextmanager
def _saved(into):
    """collects the tensors an autograd.Function saves for its backward (the recorded stage inputs and the final states)"""
    def pack(t):
        into.append(t)
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        yield


@pytest.mark.parametrize("nc", uen.TRAIN, ids=lambda c: c.id)
def test_recording_forward_and_gradients_equal_noisy_ocflow_train_on_the_member(nc):
    b = nc.base
    n, d, nt = b.n, b.d, b.nt
    assert nc.own_x
    ens, rows, x, prob = _setup(nc)
    # the recording launch itself, into guarded buffers: s_all, z_out and, where the one-CU kernel writes one, the activation record
    bufs, guards = {}, {}
    for key, shape in _shapes(nc, n, True).items():
        guards[key], bufs[key] = _guarded(*shape)
    stride = ensemble._act_stride(_lib.lib(), ens, n, nt, b.stepper) if nc.family == "mid" else 0
    if stride:
        guards["act"], bufs["act"] = _guarded(E, stride)
    out = _launch(nc, x, ens, prob, record=True, bufs=bufs, noise=_noise_of(nc))
    assert _kernel() == ENS_KERNEL[nc.family]
    torch.cuda.synchronize()
    _guards_intact(guards, bufs)
    for key in ("persample", "z_out", "sums", "s_all"):
        assert bool(torch.isfinite(out[key]).all()), key
    # ... and the public call with its backward
    gJ = torch.tensor(GJ, device=DEV)
    xe = x.clone().requires_grad_(True)
    saved = []
    with _saved(saved):
        Jc, cs = na.ensemble_noisy_ocflow_train(xe, ens, prob, b.tspan, nt, nc.sigma, nc.seed, b.stepper, mask=nc.mask,
                                                row_offset=nc.row_offset, family=nc.family)
    assert _kernel() == ENS_KERNEL[nc.family]
    assert tuple(Jc.shape) == (E,) and tuple(cs.shape) == (E, 7) and Jc.requires_grad and not cs.requires_grad
    assert torch.equal(cs, out["sums"][:, :7] / out["sums"][:, 7:8])
    (gJ * Jc).sum().backward()
    assert _kernel() == ENS_BWD[nc.family]
    s_ens = next(t for t in saved if t.dim() == out["s_all"].dim())
    assert torch.equal(s_ens, out["s_all"])
    for e in range(E):
        net, pe = ens.member(e), nc.util.member_problem(nc.case, e, DEV)
        sg, sd = uen.member_sigma(nc.sigma, e), nc.member_seed(e)
        x1 = x[e].clone().requires_grad_(True)
        one = _single(nc, net, pe, x[e].contiguous(), rows[e], sg, sd, record=True)
        for key in ("persample", "z_out", "sums", "s_all"):
            assert torch.equal(_member(nc, out, key, e, n), one[key]), (e, key)
        if nc.family == "mid":
            assert one["recorded"] == out["recorded"] == ("act" in one)
            if "act" in one:
                nact = one["act"].numel()
                assert torch.equal(out["act"][e, :nact], one["act"]), e
        got = []
        with _saved(got):
            J1, c1 = na.noisy_ocflow_train(x1, net, pe, list(b.tspan), nt, sg, sd, b.stepper, rows[e], mask=nc.mask, row_offset=nc.row_offset)
        assert _kernel() == ONE_KERNEL[nc.family]
        (gJ[e] * J1).backward()
        assert _kernel() == ONE_BWD[nc.family]
        s1 = next(t for t in got if t.dim() == 3)
        assert torch.equal(_member(nc, out, "s_all", e, n), s1), e
        assert torch.equal(Jc[e].detach(), J1.detach()) and torch.equal(cs[e], torch.stack(c1)), e
        assert torch.equal(xe.grad[e], x1.grad), e
        for name, p in ens.named_parameters():
            assert p.grad is not None and torch.equal(p.grad[e], dict(net.named_parameters())[name].grad), (e, name)
    assert all(bool((p.grad[e] != 0).any()) for e in range(E) for _, p in ens.named_parameters())


# ---- 4. the key of a row
@pytest.mark.parametrize("nc", [uen.first(uen.FORWARD, "lane", own_x=True, isigma=0), uen.first(uen.FORWARD, "mid", own_x=True, isigma=2)],
                         ids=lambda c: c.id)
def test_rows_keep_their_noise_when_a_member_is_cut_in_two(nc):
    b = nc.base
    n, a = b.n, 3                                               # (a = 3: neither a workgroup's four waves nor a 16-row tile)
    ens, rows, x, prob = _setup(nc)
    r0 = nc.row_offset
    with torch.no_grad():
        whole = _launch(nc, x, ens, prob, noise=_noise_of(nc))
        lo = _launch(nc, x[:, :a].contiguous(), ens, prob, noise=_noise_of(nc))
        hi = _launch(nc, x[:, a:].contiguous(), ens, prob, noise=_noise_of(nc, row_offset=r0 + a))
        moved = _launch(nc, x[:, a:].contiguous(), ens, prob, noise=_noise_of(nc, row_offset=r0 + a + 1))
    for e in range(E):
        for key in ("persample", "z_out"):
            w = _member(nc, whole, key, e, n)
            assert torch.equal(w[:a], _member(nc, lo, key, e, a)) and torch.equal(w[a:], _member(nc, hi, key, e, n - a)), (e, key)
            assert not torch.equal(w[a:], _member(nc, moved, key, e, n - a)), (e, key)      # (another key: another noise)


@pytest.mark.parametrize("nc", [uen.first(uen.FORWARD, "lane", own_x=False), uen.first(uen.FORWARD, "mid", own_x=False)], ids=lambda c: c.id)
def test_one_seed_is_one_noise_scaled_by_each_members_level(nc):
    """shared starts, one seed: behind step 0 member e stands at its undisturbed state + fl(scale_e * g) with ONE g for all members --
    counter_disturbances with the member's scale (nocf_noise_fill_f32) is that product.  Not a tolerance: the kernel's z += w is one
    rounded addition, torch's is the same one."""
    b = nc.base
    n, d = b.n, b.d
    sigma = [[0.05], [0.1], [0.2]]                              # powers of two apart: W_1 = 2 W_0, W_2 = 4 W_0 exactly
    ens, rows, x, prob = _setup(nc)
    xs = x[0].contiguous()
    with torch.no_grad():
        noisy = _launch(nc, xs, ens, prob, intermediates=True, noise=_noise_of(nc, sigma=sigma, seed=uen.SEED_SHARED))
        plain = _launch(nc, xs, ens, prob, intermediates=True)
    W = [na.counter_disturbances(b.nt, n, d, sigma[e][0], uen.SEED_SHARED, tspan=b.tspan, mask=nc.mask, row_offset=nc.row_offset, device=DEV)
         for e in range(E)]
    assert torch.equal(W[1], 2 * W[0]) and torch.equal(W[2], 4 * W[0]) and bool((W[0] != 0).any())
    for e in range(E):
        zn, zp = _member(nc, noisy, "zFull", e, n), _member(nc, plain, "zFull", e, n)      # [nt + 1, n, d + 4]
        assert torch.equal(zn[0], zp[0])
        assert torch.equal(zn[1, :, :d], zp[1, :, :d] + W[e][0]), e
        assert torch.equal(zn[1, :, d:], zp[1, :, d:]), e      # (the four cost components are not displaced)


# ---- 5. the study
@pytest.mark.parametrize("nc", [uen.first(uen.FORWARD, "lane", own_x=True), uen.first(uen.FORWARD, "mid", own_x=False)], ids=lambda c: c.id)
def test_noise_study_members_equal_noise_study_on_the_member(nc):
    b = nc.base
    members, nex, paths = 2, 3, 4
    ens, rows, x, prob = _setup(nc, members=members, n=nex)
    xe = x if nc.own_x else x[0]
    sigma, seed = nc.sigma[:members], (nc.seed[:members] if nc.own_x else nc.seed)
    kw = dict(tspan=b.tspan, stepper=b.stepper, mask=nc.mask, max_rows=2 * paths)          # two starts per launch: two chunks
    with torch.no_grad():
        got = na.ensemble_noise_study(xe, ens, prob, b.nt, sigma, paths, seed, family=nc.family, **kw)
        assert _kernel() == ENS_KERNEL[nc.family]
        assert tuple(got["persample"].shape) == (members, nex, paths, 7)
        for e in range(members):
            net, pe, x1 = ens.member(e), nc.util.member_problem(nc.case, e, DEV), _member_x(nc, x, e)
            want = na.noise_study(x1, net, pe, b.nt, uen.member_sigma(sigma, e), paths, alph=rows[e], rng="counter", seed=nc.member_seed(e), **kw)
            assert _kernel() == ONE_KERNEL[nc.family]
            assert torch.equal(got["persample"][e], want["persample"]), e
            for q in ("L+G", "G", "Q", "W"):
                for stat in ("mean", "std", "q05", "q50", "q95"):
                    assert torch.equal(got[q][stat][e], want[q][stat]), (e, q, stat)
    assert not torch.equal(got["persample"][0], got["persample"][1])


# ---- 6. the driver
def _run_driver(argv, capsys):
    import importlib.util
    spec = importlib.util.spec_from_file_location("trainOC_under_test", os.path.join(REPO, "trainOC.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    capsys.readouterr()
    mod.main(argv)
    lines = [ln.split() for ln in capsys.readouterr().out.splitlines()]
    # the members' iteration lines without their wall-clock column
    return [cols[:3] + cols[4:] for cols in lines if len(cols) > 4 and cols[0] in ("m0", "m1") and cols[1].isdigit()]


@pytest.mark.parametrize("family, common", [
    ("lane", ["--data", "softcorridor", "--m", "16"]),
    ("mid", ["--data", "singlequad", "--m", "64", "--members_family", "mid"]),
])
def test_driver_members_sigma(family, common, tmp_path, capsys):
    common = common + ["--nt", "4", "--niters", "2", "--n_train", "32", "--val_freq", "2", "--seed", "5", "--members", "2",
                       "--save", str(tmp_path / "out")]
    noisy = ["--members_sigma", "0.1,0.2"]
    first = _run_driver(common + noisy + ["--noise_seed", "11"], capsys)
    assert _kernel() == ENS_KERNEL[family].replace(",noisy", "")                           # (the last launch: the undisturbed validation)
    again = _run_driver(common + noisy + ["--noise_seed", "11"], capsys)
    other = _run_driver(common + noisy + ["--noise_seed", "12"], capsys)
    zero = _run_driver(common + ["--members_sigma", "0,0"], capsys)
    plain = _run_driver(common, capsys)
    assert len(first) == 4 and first == again                   # two members, two iterations
    assert len(other) == 4 and other != first
    assert zero == plain and first != plain
