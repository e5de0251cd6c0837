"""Ensembles of small value networks: E networks of one shape rolled out, and trained, in one launch each.

The lane kernels (csrc/nocf_lane.inc, csrc/nocf_lane_bwd.inc: nTh = 2, m <= 32, d+1 <= 32, point agents) integrate one sample per wavefront
with the whole network in registers.  A single rollout of such a network is a latency chain that leaves the machine almost empty; what users
of these problems do is run the same shape many times -- seeds, the `alph` multipliers, checkpoints.  Here the launch is one batch of E * n
rows and wave g reads network g // n; nothing else in the rollout changes, so member e's results carry the bits of the single-network call
(OCflow / ocflow_train) on that member alone.

    ens = PhiEnsemble(E, nTh, m, d, alph=..., seeds=[...])           # or PhiEnsemble.from_members([phi_0, ...])
    Jc, cs = ensemble_rollout(x, ens, prob, tspan, nt)                # Jc [E], cs [E, 7]
    Jc, cs = ensemble_ocflow_train(x, ens, prob, tspan, nt)           # Jc.sum().backward(): E independent gradients from one adjoint launch

Single precision, one device, undisturbed rollouts (under in-kernel Brownian noise: ensemble_noise.py, which launches through this module).
There is no CPU or eager-torch fallback behind these calls: everything else is refused before a launch.

family="mid"  selects the one-CU weight-stationary kernels instead (csrc/nocf_mono.inc, csrc/nocf_mono_bwd.inc: nTh = 2,
m <= 128, d+1 <= 32, all three problem classes -- singlequad among them).  There a 16-sample tile sits on one CU with the whole network in its
registers, a rollout of n = 1024 rows occupies 64 of 256 CUs, and an ensemble fills the idle ones: member e takes workgroups [e * tiles,
(e + 1) * tiles) of the launch and every buffer is member-major.  The default, family="lane", is the lane family and nothing else."""
import ctypes as C
import os

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .Phi import Phi
from .train import _STEPPERS, _step_sizes, _unpack_partials

LANE_LIMITS = "nTh = 2, m <= 32, d + 1 <= 32, rank of A <= 16, a point-agent problem (Cross2D / SwarmTraj) with at most 16 agents"

MID_LIMITS = ("nTh = 2, a width with a one-CU instantiation (m <= 128; training: 32 < m), d + 1 <= 32, rank of A <= 16, Cross2D / SwarmTraj / "
              "Quadcopter with at most 8 agents when d + 1 <= 16 and at most 16 beyond (MONO_NAG)")
FAMILIES = ("lane", "mid")

_LANE = ("nocf_rollout_ensemble_f32", "nocf_rollout_record_ensemble_f32", "nocf_rollout_bwd_small_ensemble_f32")
_MID = ("nocf_rollout_mid_ensemble_f32", "nocf_rollout_record_mid_ensemble_f32", "nocf_rollout_bwd_mid_ensemble_f32")
_MID_WORKSPACE = ("nocf_mid_ensemble_workspace_bytes",)
# the weighted ensemble adjoints (ensemble_risk.py): the two adjoint entries above with `const float* wrow` [E, n] in place of `double inv_n`
_WEIGHTED = {"lane": "nocf_rollout_bwd_small_ensemble_rw_f32", "mid": "nocf_rollout_bwd_mid_ensemble_rw_f32"}


def weighted_entry(L, family):
    """the weighted ensemble adjoint of a family in library L; RuntimeError when L does not export BOTH (a library is rebuilt as a whole)"""
    f = _lib.require(L, tuple(_WEIGHTED.values()), "ensemble")
    return f[list(_WEIGHTED).index(family)]


def _entries_mid(L):
    """the three entries _MID of library L, or None when L lacks one of them or nocf_mid_ensemble_workspace_bytes"""
    f = _lib.entries(L, _MID_WORKSPACE + _MID)
    return f and f[1:]


def _shipped_mid():
    """the shipped library and its three one-CU ensemble entries"""
    L = _lib.lib()
    return L, _lib.require(L, _MID_WORKSPACE + _MID, "ensemble")[1:]


def _mid_eligible(nTh, m, d, r, n_agents, train=False):
    """the shape has a one-CU plan (make_mono_plan of csrc/nocf_kernels.hip); train: and an adjoint instantiation (nocf_mid_grad_rows != 0)"""
    kbd = -(-(d + 1) // 16)
    return (nTh == 2 and 1 <= m <= 128 and 1 <= d and d + 1 <= 32 and 1 <= r <= min(16, d + 1) and 1 <= n_agents <= (8 if kbd == 1 else 16)
            and (m > 32 or not train))


def _entries(L):
    """the three entries _LANE of library L, or None when L lacks one of them"""
    return _lib.entries(L, _LANE)


def _shipped():
    """the shipped library and its three ensemble entries (the lane family needs no per-shape library)"""
    L = _lib.lib()
    return L, _lib.require(L, _LANE, "ensemble")


class _Stacked(nn.Module):
    """the parameters of E nn.Linear layers under nn.Linear's names, with a leading member axis"""

    def __init__(self, weight, bias=None):
        super().__init__()
        self.weight = nn.Parameter(weight)
        if bias is not None:
            self.bias = nn.Parameter(bias)


class _StackedResNN(nn.Module):
    def __init__(self, layers):
        super().__init__()
        self.layers = nn.ModuleList(layers)


def _alph_rows(alph, members):
    """one list of six or E rows of six -> E lists of six floats"""
    if isinstance(alph, torch.Tensor):
        alph = alph.detach().cpu().tolist()
    rows = list(alph)
    if rows and not isinstance(rows[0], (list, tuple)):
        rows = [rows] * members
    rows = [[float(v) for v in r_[:6]] for r_ in rows]
    if len(rows) != members or any(len(r_) < 6 for r_ in rows):
        raise ValueError(f"alph must be one list of 6 multipliers or {members} rows of 6")
    return rows


class PhiEnsemble(nn.Module):
    """E value networks Phi of one shape.  The parameters carry Phi's names (A, c.weight, c.bias, w.weight, N.layers.{i}.weight / .bias)
    with a leading member axis, so ONE optimiser over this module is E independent elementwise optimisers.

    :param members: E
    :param alph:    one list of six multipliers, or E rows of six (member e's row: its OCflow multipliers AND its alph_Q / alph_W)
    :param seeds:   E seeds: member e is exactly Phi(nTh, m, d, r) built under torch.manual_seed(seeds[e]) (the global generator is left as
                    it was).  None: the members are drawn one after the other from the global generator"""

    def __init__(self, members, nTh, m, d, r=10, alph=[1.0] * 6, seeds=None):
        super().__init__()
        members = int(members)
        if members < 1:
            raise ValueError("an ensemble needs at least one member")
        if seeds is not None and len(seeds) != members:
            raise ValueError(f"seeds must hold {members} entries")
        rows = _alph_rows(alph, members)
        nets = []
        for e in range(members):
            if seeds is None:
                nets.append(Phi(nTh, m, d, r=r, alph=rows[e]))
            else:
                with torch.random.fork_rng(devices=[]):
                    torch.manual_seed(int(seeds[e]))
                    nets.append(Phi(nTh, m, d, r=r, alph=rows[e]))
        self._adopt(nets, rows)

    def _adopt(self, nets, rows):
        p0 = nets[0]
        for q in nets[1:]:
            if (q.nTh, q.m, q.d, tuple(q.A.shape)) != (p0.nTh, p0.m, p0.d, tuple(p0.A.shape)):
                raise ValueError("the members of an ensemble must have one shape (nTh, m, d, rank of A)")
        self.members, self.nTh, self.m, self.d, self.r = len(nets), p0.nTh, p0.m, p0.d, p0.A.shape[0]
        self.alph = [list(r_) for r_ in rows]

        def st(get):
            return torch.stack([get(q).detach() for q in nets]).contiguous()

        # (registration order = Phi's, so named_parameters() lists the same names in the same order)
        self.A = nn.Parameter(st(lambda q: q.A))
        self.c = _Stacked(st(lambda q: q.c.weight), st(lambda q: q.c.bias))
        self.w = _Stacked(st(lambda q: q.w.weight))
        self.N = _StackedResNN([_Stacked(st(lambda q, i=i: q.N.layers[i].weight), st(lambda q, i=i: q.N.layers[i].bias))
                                for i in range(p0.nTh)])
        self._tables = {}
        self._plist = None
        self._mid_ws = {}

    def _params(self):
        """[(name, parameter)] in named_parameters() order, cached: the walk over the module tree costs more than a small rollout's launch"""
        pl = self._plist
        if pl is None or pl[0][1] is not self.A:
            pl = self._plist = list(self.named_parameters())
        return pl

    @classmethod
    def from_members(cls, nets, alph=None):
        """an ensemble holding exact copies of the given Phi (alph: as for the constructor; default: every member's own .alph)"""
        nets = list(nets)
        if not nets:
            raise ValueError("an ensemble needs at least one member")
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self._adopt(nets, _alph_rows([list(q.alph) for q in nets] if alph is None else alph, len(nets)))
        return self.to(nets[0].A.device)

    def member_state_dict(self, e):
        """member e's parameters in the reference's checkpoint layout (Phi.state_dict()'s keys and shapes)"""
        return {name: p[e].detach().clone() for name, p in self._params()}

    def member(self, e):
        """member e as a Phi on this module's device: an exact copy (Phi.alph = the member's row)"""
        q = Phi(self.nTh, self.m, self.d, r=self.r, alph=list(self.alph[e]))
        q.load_state_dict(self.member_state_dict(e))
        return q.to(self.A.device)

    def alph_table(self, alph=None):
        """the multipliers as the device table [E, 6] the kernels index by member (cached per device and value)"""
        rows = self.alph if alph is None else _alph_rows(alph, self.members)
        key = (self.A.device, tuple(tuple(r_) for r_ in rows))
        t = self._tables.get(key)
        if t is None:
            if len(self._tables) > 8:
                self._tables.clear()
            t = self._tables[key] = torch.tensor(rows, dtype=torch.float32).to(self.A.device)
        return t

    def mid_workspace(self, L, dev):
        """the workspace of the one-CU family (nocf_mid_ensemble_workspace_bytes: every member's images, padded vectors and plan record), one
        per device and stream (as Phi's), cached: the launches of one stream are ordered, and every launch packs it anew"""
        key = (dev, torch.cuda.current_stream(dev).cuda_stream)
        ws = self._mid_ws.get(key)
        if ws is None:
            if len(self._mid_ws) > 8:
                self._mid_ws.clear()
            nbytes = int(L.nocf_mid_ensemble_workspace_bytes(self.d, self.m, self.nTh, self.r, self.members))
            if nbytes == 0:
                raise RuntimeError(f"ensemble: no one-CU plan for nTh = {self.nTh}, m = {self.m}, d = {self.d}, rank {self.r}")
            ws = self._mid_ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        return ws

    def forward(self, x):
        raise NotImplementedError("PhiEnsemble is evaluated inside the ensemble rollouts (ensemble_rollout / ensemble_ocflow_train); "
                                  "ens.member(e) is a Phi")

    def _c_struct(self):
        """(NocfPhi over the stacked tensors, keep-alive list)"""
        pl = self._params()
        ptr = {}
        for name, p in pl:                               # (the stacked tensors are read in place: they must be what _refuse has checked)
            if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
                raise RuntimeError(f"{name} must be a contiguous float32 tensor on the MI355X")
            ptr[name] = p.data_ptr()
        st = _lib.NocfPhi()
        st.d, st.m, st.nTh, st.r = self.d, self.m, self.nTh, self.r
        st.K0, st.b0 = ptr["N.layers.0.weight"], ptr["N.layers.0.bias"]
        st.K, st.b = ptr["N.layers.1.weight"], ptr["N.layers.1.bias"]
        st.w, st.A, st.cw = ptr["w.weight"], ptr["A"], ptr["c.weight"]
        st.cb = 0.0
        st.cb_dev = ptr["c.bias"]
        return st, pl


def _refuse(fn, x, ens, prob, nt, stepper, train, noMean=False, W=None, family="lane"):
    """every refusal of an ensemble call, raised before the library is reached.  -> (E, n, d, own)"""
    if family not in FAMILIES:
        raise ValueError(f"{fn}: family must be 'lane' (the small-network lane kernels) or 'mid' (the one-CU kernels), got {family!r}")
    if not isinstance(ens, PhiEnsemble):
        raise TypeError(f"{fn}: ens must be a PhiEnsemble")
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    xt = getattr(prob, "xtarget", None)
    params = ens._params()
    for name, t in [("x", x), ("prob.xtarget", xt)] + params:
        if isinstance(t, torch.Tensor) and t.dtype == torch.float64:
            raise RuntimeError(f"{fn}: {name} is float64; ensembles are single precision only (the double-precision kernels take one network)")
    kind, n_agents = getattr(prob, "KIND", None), int(getattr(prob, "nAgents", 0))
    if family == "mid":
        if not (kind in (_lib.PROB_CROSS2D, _lib.PROB_SWARMTRAJ, _lib.PROB_QUADCOPTER)
                and _mid_eligible(ens.nTh, ens.m, ens.d, ens.r, n_agents, train)):
            raise ValueError(f"{fn}: family='mid' runs on the one-CU kernels only: {MID_LIMITS}; got nTh = {ens.nTh}, m = {ens.m}, "
                             f"d = {ens.d}, rank {ens.r}, {type(prob).__name__} with {n_agents} agents" + (", training" if train else ""))
    elif not (ens.nTh == 2 and 1 <= ens.m <= 32 and ens.d + 1 <= 32 and 1 <= ens.r <= 16
            and kind in (_lib.PROB_CROSS2D, _lib.PROB_SWARMTRAJ) and 1 <= n_agents <= 16):
        raise ValueError(f"{fn}: an ensemble runs on the small-network lane kernels only: {LANE_LIMITS}; got nTh = {ens.nTh}, m = {ens.m}, "
                         f"d = {ens.d}, rank {ens.r}, {type(prob).__name__} with {n_agents} agents")
    if family == "lane" and train and not (kind == _lib.PROB_CROSS2D and 2 * n_agents == ens.d):
        raise ValueError(f"{fn}: the lane adjoint takes Cross2D agents only ({LANE_LIMITS}); got {type(prob).__name__}")
    if noMean:
        raise NotImplementedError(f"{fn}: noMean is not built for ensembles (per-sample costs: OCflow on ens.member(e))")
    if W is not None:
        raise NotImplementedError(f"{fn}: disturbed, noisy and min-max rollouts take one network (disturbed_rollout, noisy_rollout, ...)")
    if stepper not in _STEPPERS:
        raise ValueError(f"stepper must be 'rk4' or 'rk1', got {stepper!r}")
    if int(nt) < 1:
        raise ValueError("nt must be >= 1")
    E = ens.members
    if x.dim() == 2:
        own, (n, d) = False, x.shape
    elif x.dim() == 3 and x.shape[0] == E:
        own, (n, d) = True, x.shape[1:]
    else:
        raise ValueError(f"x must be nex-by-d (shared by the members) or {E}-by-nex-by-d (every member its own starts)")
    if d != ens.d:
        raise ValueError(f"x has d={d} but the ensemble was built for d={ens.d}")
    pd_ = getattr(prob, "d", None)
    if pd_ is not None and int(pd_) != d:
        raise ValueError(f"the problem object has d={pd_} but x has d={d}")
    if n < 1:
        raise ValueError("x has no rows")
    if E * n >= 2 ** 31:
        raise ValueError("members * nex must stay below 2**31")
    if train and x.requires_grad and not own:
        raise NotImplementedError(f"{fn}: x.requires_grad needs every member's own starts (x of shape [E, nex, d]): the members' dJ/dx of a "
                                  "shared x are not summed")
    _lib.require_device_f32(x, "x")
    for name, p in params:
        if not p.is_cuda or p.dtype != torch.float32:
            _lib.require_device_f32(p, name)
        if p.device != x.device:
            raise ValueError("x and the ensemble must be on the same device")
    return E, int(n), int(d), own


def _launch(x, ens, prob, tspan, nt, stepper, alph=None, intermediates=False, record=False, bufs=None, noise=None, dist=None):
    """one ensemble launch (nocf_rollout_ensemble_f32, or nocf_rollout_record_ensemble_f32 with record) -> dict of its buffers: persample
    [E*n, 7], z_out [E*n, d+4], sums [E, 8], means [E, 8] (evaluation), zFull / ctrlFull (time-major over E*n rows, intermediates), s_all
    [nt*nstage, E*n, d+1] (record).  bufs: buffers to write into instead of fresh ones (same keys).  noise: an ensemble_noise._Noise -- the
    launch is the noisy sibling's (nocf_rollout_noisy_ensemble_f32 / nocf_rollout_record_noisy_ensemble_f32), same buffers.  dist: an
    ensemble_minmax._Disturbance -- the launch is the disturbed sibling's (nocf_rollout_disturbed_ensemble_f32 /
    nocf_rollout_record_disturbed_ensemble_f32) under its tensor W, same buffers; it speaks noise's protocol (entries, args)"""
    if dist is not None:
        noise = dist
    E = ens.members
    own = x.dim() == 3
    n, d = x.shape[-2], x.shape[-1]
    x = _lib.require_device_f32(x.detach(), "x")
    dev = x.device
    _lib.check_errors()
    L, (f_eval, f_rec, _f_bwd) = _shipped()
    names = ("nocf_rollout_ensemble_f32", "nocf_rollout_record_ensemble_f32")
    if noise is not None:
        f_eval, f_rec, names = noise.entries(L, "lane")
    phi_st, keep1 = ens._c_struct()
    prob_st, keep2 = prob._c_struct(dev)
    table = ens.alph_table(alph)
    rows = E * n
    b = dict(bufs or {})
    nstage = 4 if stepper == "rk4" else 1

    def buf(key, *shape):
        t = b.get(key)
        if t is None:
            t = b[key] = torch.empty(*shape, dtype=torch.float32, device=dev)
        if tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.dtype != torch.float32 or t.device != dev:
            raise ValueError(f"{key} must be a contiguous float32 tensor of shape {tuple(shape)} on {dev}")
        return t

    persample, z_out, sums = buf("persample", rows, 7), buf("z_out", rows, d + 4), buf("sums", E, 8)
    head = (C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), n, E, n * d if own else 0) + (noise.args(dev) if noise is not None else ()) + \
           (float(tspan[0]), float(tspan[1]), int(nt), _STEPPERS[stepper], _lib.ptr(table))
    with torch.cuda.device(dev):
        if record:
            s_all = buf("s_all", nt * nstage, rows, d + 1)
            rc = f_rec(*head, _lib.ptr(z_out), _lib.ptr(persample), _lib.ptr(sums), _lib.ptr(s_all), None, 0, _lib.stream_ptr(dev))
            what = names[1]
        else:
            means = buf("means", E, 8)
            zF = cF = None
            if intermediates:
                cdim = L.nocf_ctrl_dim(C.byref(prob_st), d)
                zF, cF = buf("zFull", nt + 1, rows, d + 4), buf("ctrlFull", nt + 1, rows, cdim)
            rc = f_eval(*head, _lib.ptr(z_out), _lib.ptr(persample), _lib.ptr(sums), _lib.ptr(means), _lib.ptr(zF), _lib.ptr(cF),
                        None, 0, _lib.stream_ptr(dev))
            what = names[0]
    _lib.check(rc, what)
    b["table"] = table
    return b


def _act_stride(L, ens, n, nt, stepper):
    """member stride of the one-CU ensemble's activation record, in floats: nocf_activation_record_floats rounded up to whole 16-byte pieces
    (0: the shape records nothing, the adjoint recomputes; NOCF_ACT_REC=0 as for the single-network call)"""
    if os.environ.get("NOCF_ACT_REC", "1") in ("0", ""):
        return 0
    return (int(L.nocf_activation_record_floats(ens.d, ens.m, ens.nTh, int(n), int(nt), _STEPPERS[stepper])) + 3) // 4 * 4


def _launch_mid(x, ens, prob, tspan, nt, stepper, alph=None, intermediates=False, record=False, bufs=None, noise=None, dist=None):
    """one launch of the one-CU family (nocf_rollout_mid_ensemble_f32, or nocf_rollout_record_mid_ensemble_f32 with record) -> dict of its
    buffers, all MEMBER-MAJOR: persample [E, n, 7], z_out [E, n, d+4], sums [E, 8], means [E, 8] (evaluation), zFull [E, nt+1, n, d+4] /
    ctrlFull [E, nt+1, n, a] (intermediates), s_all [E, nt*nstage, n, d+1] and act [E, stride] or None (record; "recorded": the kernel wrote
    it).  bufs: buffers to write into instead of fresh ones (same keys).  noise: as for _launch (nocf_rollout_noisy_mid_ensemble_f32 /
    nocf_rollout_record_noisy_mid_ensemble_f32).  dist: as for _launch (nocf_rollout_disturbed_mid_ensemble_f32 /
    nocf_rollout_record_disturbed_mid_ensemble_f32)"""
    if dist is not None:
        noise = dist
    E = ens.members
    own = x.dim() == 3
    n, d = x.shape[-2], x.shape[-1]
    x = _lib.require_device_f32(x.detach(), "x")
    dev = x.device
    _lib.check_errors()
    L, (f_eval, f_rec, _f_bwd) = _shipped_mid()
    names = ("nocf_rollout_mid_ensemble_f32", "nocf_rollout_record_mid_ensemble_f32")
    if noise is not None:
        f_eval, f_rec, names = noise.entries(L, "mid")
    phi_st, keep1 = ens._c_struct()
    prob_st, keep2 = prob._c_struct(dev)
    table = ens.alph_table(alph)
    ws = ens.mid_workspace(L, dev)
    b = dict(bufs or {})
    nstage = 4 if stepper == "rk4" else 1

    def buf(key, *shape):
        t = b.get(key)
        if t is None:
            t = b[key] = torch.empty(*shape, dtype=torch.float32, device=dev)
        if tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.dtype != torch.float32 or t.device != dev:
            raise ValueError(f"{key} must be a contiguous float32 tensor of shape {tuple(shape)} on {dev}")
        return t

    persample, z_out, sums = buf("persample", E, n, 7), buf("z_out", E, n, d + 4), buf("sums", E, 8)
    head = (C.byref(phi_st), C.byref(prob_st), _lib.ptr(x), n, E, n * d if own else 0) + (noise.args(dev) if noise is not None else ()) + \
           (float(tspan[0]), float(tspan[1]), int(nt), _STEPPERS[stepper], _lib.ptr(table))
    tail = (_lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    with torch.cuda.device(dev):
        if record:
            s_all = buf("s_all", E, nt * nstage, n, d + 1)
            stride = _act_stride(L, ens, n, nt, stepper)
            act = None
            if stride:
                try:
                    act = buf("act", E, stride)
                except torch.OutOfMemoryError:                 # the record is an optimisation: without it the adjoint recomputes
                    act = None
            recorded = C.c_int32(0)
            rc = f_rec(*head, _lib.ptr(z_out), _lib.ptr(persample), _lib.ptr(sums), _lib.ptr(s_all), _lib.ptr(act), C.byref(recorded), *tail)
            what = names[1]
            b["recorded"] = bool(recorded.value)
            b["act"] = act if recorded.value else None
        else:
            means = buf("means", E, 8)
            zF = cF = None
            if intermediates:
                cdim = L.nocf_ctrl_dim(C.byref(prob_st), d)
                zF, cF = buf("zFull", E, nt + 1, n, d + 4), buf("ctrlFull", E, nt + 1, n, cdim)
            rc = f_eval(*head, _lib.ptr(z_out), _lib.ptr(persample), _lib.ptr(sums), _lib.ptr(means), _lib.ptr(zF), _lib.ptr(cF), *tail)
            what = names[0]
    _lib.check(rc, what)
    b["table"] = table
    return b


def ensemble_rollout(x, ens, prob, tspan, nt, stepper="rk4", alph=None, intermediates=False, *, noMean=False, W=None, family="lane"):
    """OCflow for every member of an ensemble in one launch.
    :param x:     nex-by-d (every member integrates the same starts) or E-by-nex-by-d (every member its own), float32 on the MI355X
    :param ens:   PhiEnsemble
    :param prob:  Cross2D / SwarmTraj; its target, obstacle, r and mode are common to the members, its alph_Q / alph_W are NOT read:
                  member e takes entries 1 and 2 of its row of alph
    :param alph:  one list of six or E rows of six (default: ens.alph)
    :param family: "lane" (default): the small-network lane kernels, LANE_LIMITS.  "mid": the one-CU kernels, MID_LIMITS -- also a Quadcopter
                  problem, e.g. singlequad; member e's values are then OCflow's on the one-CU kernel
    :return: (Jc [E], cs [E, 7]); with intermediates also the trajectories [E, nex, d+4, nt+1] and the controls [E, nex, a, nt+1].
             Member e's values are bit for bit OCflow's on ens.member(e) with a problem of that member's alph_Q / alph_W.
             An evaluation: nothing here is differentiable (ensemble_ocflow_train is)."""
    E, n, d, _own = _refuse("ensemble_rollout", x, ens, prob, nt, stepper, False, noMean, W, family)
    if family == "mid":
        b = _launch_mid(x, ens, prob, tspan, int(nt), stepper, alph, intermediates)
        Jc, cs = b["means"][:, 7], b["means"][:, :7]
        if not intermediates:
            return Jc, cs
        # kernel layout is member-major [E, nt+1, nex, .]; the reference's, per member, is [nex, ., nt+1]
        return Jc, cs, b["zFull"].permute(0, 2, 3, 1), b["ctrlFull"].permute(0, 2, 3, 1)
    b = _launch(x, ens, prob, tspan, int(nt), stepper, alph, intermediates)
    Jc, cs = b["means"][:, 7], b["means"][:, :7]
    if not intermediates:
        return Jc, cs
    zF, cF = b["zFull"], b["ctrlFull"]
    # kernel layout is time-major [nt+1, E*nex, .]; the reference's, per member, is [nex, ., nt+1]
    return Jc, cs, zF.view(nt + 1, E, n, d + 4).permute(1, 2, 3, 0), cF.view(nt + 1, E, n, cF.shape[-1]).permute(1, 2, 3, 0)


class _MemberA:
    """what train._unpack_partials reads of a network: A"""

    def __init__(self, A):
        self.A = A


class _EnsembleTrain(torch.autograd.Function):
    """ocflow_train for E networks: one recording forward (nocf_rollout_record_ensemble_f32) and one adjoint launch
    (nocf_rollout_bwd_small_ensemble_f32).  The members do not interact: gJ [E] scales each member's gradient."""

    @staticmethod
    def forward(ctx, x, ens, prob, tspan, nt, stepper, alph, *params):
        return _EnsembleTrain._forward(ctx, x, ens, prob, tspan, nt, stepper, alph)

    @staticmethod
    def _forward(ctx, x, ens, prob, tspan, nt, stepper, alph, noise=None, dist=None):
        """(noise: the recording forward draws its disturbances, ensemble_noise.py; dist: it runs under a tensor disturbance,
        ensemble_minmax.py; everything saved is what the undisturbed forward saves)"""
        ctx.x_needs_grad = bool(x.requires_grad)
        b = _launch(x, ens, prob, tspan, nt, stepper, alph, record=True, noise=noise, dist=dist)
        ctx.ens, ctx.prob, ctx.tspan, ctx.nt, ctx.stepper, ctx.table = ens, prob, tspan, nt, stepper, b["table"]
        ctx.persample = b["persample"]                      # (the weighted calls form their sums and risks from it: ensemble_risk.py)
        ctx.save_for_backward(b["s_all"], b["z_out"])
        # the adjoint re-reads the weights from the module: they must still be the ones this forward ran with
        ctx.param_versions = [p._version for _, p in ens._params()]
        sums, a = b["sums"], b["table"]
        means = sums[:, :7] / sums[:, 7:8]
        Jc = means[:, 0] + a[:, 0] * means[:, 1] + a[:, 3] * means[:, 2] + a[:, 4] * means[:, 3] + a[:, 5] * means[:, 4]
        cs = means.detach()
        ctx.mark_non_differentiable(cs)                     # (only Jc carries a gradient: the logged costs are values)
        return Jc, cs

    @staticmethod
    @once_differentiable
    def backward(ctx, gJ, _gmeans):
        return _EnsembleTrain._adjoint(ctx, gJ)

    @staticmethod
    def _adjoint(ctx, gJ, wrow=None, joint=None):
        """wrow: [E, n] float32 weights (ensemble_risk.py) -- the launch is the weighted entry's, wrow standing where 1 / n stands.
        joint: (entry, its name, lamW [E, nt, n, d]) (ensemble_minmax.py) -- the launch is the joint entry's, which takes lamW behind lam0 and
        fills it with every member's dJ/dW; what is returned does not change"""
        s_all, z_out = ctx.saved_tensors
        ens, prob, nt = ctx.ens, ctx.prob, ctx.nt
        if [p._version for _, p in ens._params()] != ctx.param_versions:
            raise RuntimeError("ensemble backward: a parameter of the ensemble was modified in place (optimizer step, load_state_dict) "
                               "between this forward and its backward; call backward() before changing the parameters.")
        dev = s_all.device
        E, m, d = ens.members, ens.m, ens.d
        D1 = d + 1
        n = z_out.shape[0] // E
        L, (_f_eval, _f_rec, f_bwd) = _shipped()
        what = "nocf_rollout_bwd_small_ensemble_f32"
        if wrow is not None:
            f_bwd, what = weighted_entry(L, "lane"), _WEIGHTED["lane"]
        lamW = ()
        if joint is not None:
            f_bwd, what, lamW = joint[0], joint[1], (_lib.ptr(joint[2]),)
        phi_st, keep1 = ens._c_struct()
        prob_st, keep2 = prob._c_struct(dev)
        hs = _step_sizes(ctx.tspan, nt).to(dev)
        P = int(L.nocf_small_grad_floats(d, m))
        gpart = torch.empty(E * n, P, device=dev)
        lam0 = torch.empty(E * n, d, device=dev) if ctx.x_needs_grad else None
        with torch.cuda.device(dev):
            rc = f_bwd(C.byref(phi_st), C.byref(prob_st), n, E, int(nt), _STEPPERS[ctx.stepper], float(ctx.tspan[1]),
                       _lib.ptr(ctx.table), 1.0 / float(n) if wrow is None else _lib.ptr(wrow), _lib.ptr(s_all), _lib.ptr(z_out), _lib.ptr(hs),
                       _lib.ptr(gpart), _lib.ptr(lam0), *lamW, _lib.stream_ptr(dev))
        _lib.check(rc, what)
        # per member the sum and the products of the single-network adjoint (train._unpack_partials on the member's contiguous [n, P] slice:
        # the same calls on the same shapes, so the same bits); only the exact elementwise scaling by gJ runs on the stacked tensors
        A = ens.A.detach()
        per = [_unpack_partials(gpart[e * n:(e + 1) * n], m, D1, _MemberA(A[e])) for e in range(E)]
        out = []
        for name, p in ens._params():
            g = torch.stack([per[e][name] for e in range(E)])
            out.append(gJ.reshape((E,) + (1,) * (g.dim() - 1)) * g)
        gx = gJ.reshape(E, 1, 1) * lam0.view(E, n, d) if lam0 is not None else None
        return (gx,) + (None,) * 6 + tuple(out)


class _EnsembleTrainMid(torch.autograd.Function):
    """_EnsembleTrain on the one-CU family: one recording forward (nocf_rollout_record_mid_ensemble_f32, with the activation record where the
    single-network call writes one) and one adjoint launch (nocf_rollout_bwd_mid_ensemble_f32, nocf_mid_grad_rows partial vectors per member)"""

    @staticmethod
    def forward(ctx, x, ens, prob, tspan, nt, stepper, alph, *params):
        return _EnsembleTrainMid._forward(ctx, x, ens, prob, tspan, nt, stepper, alph)

    @staticmethod
    def _forward(ctx, x, ens, prob, tspan, nt, stepper, alph, noise=None, dist=None):
        ctx.x_needs_grad = bool(x.requires_grad)
        b = _launch_mid(x, ens, prob, tspan, nt, stepper, alph, record=True, noise=noise, dist=dist)
        ctx.ens, ctx.prob, ctx.tspan, ctx.nt, ctx.stepper, ctx.table = ens, prob, tspan, nt, stepper, b["table"]
        ctx.act = b["act"]
        ctx.persample = b["persample"]
        ctx.save_for_backward(b["s_all"], b["z_out"])
        ctx.param_versions = [p._version for _, p in ens._params()]
        sums, a = b["sums"], b["table"]
        means = sums[:, :7] / sums[:, 7:8]
        Jc = means[:, 0] + a[:, 0] * means[:, 1] + a[:, 3] * means[:, 2] + a[:, 4] * means[:, 3] + a[:, 5] * means[:, 4]
        cs = means.detach()
        ctx.mark_non_differentiable(cs)
        return Jc, cs

    @staticmethod
    @once_differentiable
    def backward(ctx, gJ, _gmeans):
        return _EnsembleTrainMid._adjoint(ctx, gJ)

    @staticmethod
    def _adjoint(ctx, gJ, wrow=None, joint=None):
        """wrow, joint: as for _EnsembleTrain._adjoint"""
        s_all, z_out = ctx.saved_tensors
        ens, prob, nt = ctx.ens, ctx.prob, ctx.nt
        if [p._version for _, p in ens._params()] != ctx.param_versions:
            raise RuntimeError("ensemble backward: a parameter of the ensemble was modified in place (optimizer step, load_state_dict) "
                               "between this forward and its backward; call backward() before changing the parameters.")
        dev = s_all.device
        E, m, d = ens.members, ens.m, ens.d
        D1 = d + 1
        n = z_out.shape[1]
        L, (_f_eval, _f_rec, f_bwd) = _shipped_mid()
        what = "nocf_rollout_bwd_mid_ensemble_f32"
        if wrow is not None:
            f_bwd, what = weighted_entry(L, "mid"), _WEIGHTED["mid"]
        lamW = ()
        if joint is not None:
            f_bwd, what, lamW = joint[0], joint[1], (_lib.ptr(joint[2]),)
        phi_st, keep1 = ens._c_struct()
        prob_st, keep2 = prob._c_struct(dev)
        ws = ens.mid_workspace(L, dev)
        hs = _step_sizes(ctx.tspan, nt).to(dev)
        P = int(L.nocf_small_grad_floats(d, m))
        rows = int(L.nocf_mid_grad_rows(d, m, ens.nTh, ens.r, int(prob_st.n_agents), n))
        if rows == 0:
            raise RuntimeError("ensemble backward: the one-CU adjoint does not take this shape (NOCF_MONO / NOCF_MONO_BWD switched off?)")
        gpart = torch.empty(E, rows, P, device=dev)
        lam0 = torch.empty(E, n, d, device=dev) if ctx.x_needs_grad else None
        with torch.cuda.device(dev):
            rc = f_bwd(C.byref(phi_st), C.byref(prob_st), n, E, int(nt), _STEPPERS[ctx.stepper], float(ctx.tspan[1]),
                       _lib.ptr(ctx.table), 1.0 / float(n) if wrow is None else _lib.ptr(wrow), _lib.ptr(s_all), _lib.ptr(z_out), _lib.ptr(hs),
                       _lib.ptr(ctx.act), _lib.ptr(gpart), rows, _lib.ptr(lam0), *lamW, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, what)
        ctx.act = None
        # per member the sum and the products of the single-network adjoint: train._unpack_partials on the member's contiguous [rows, P] block
        A = ens.A.detach()
        per = [_unpack_partials(gpart[e], m, D1, _MemberA(A[e])) for e in range(E)]
        out = []
        for name, p in ens._params():
            g = torch.stack([per[e][name] for e in range(E)])
            out.append(gJ.reshape((E,) + (1,) * (g.dim() - 1)) * g)
        gx = gJ.reshape(E, 1, 1) * lam0 if lam0 is not None else None
        return (gx,) + (None,) * 6 + tuple(out)


def ensemble_ocflow_train(x, ens, prob, tspan, nt, stepper="rk4", alph=None, *, noMean=False, W=None, family="lane"):
    """(Jc [E], cs [E, 7]) with Jc differentiable in every stacked parameter of `ens` (and in x when every member has its own starts):
    one recording forward and one adjoint launch for all members.  Member e's Jc, gradients and x.grad[e] are bit for bit those of
    ocflow_train + backward() on ens.member(e) alone; an upstream gradient gJ [E] scales each member's, the members do not interact.
    Cross2D problems (the lane adjoint's); family="mid": all three problem classes, 32 < m (the one-CU adjoint's).  Arguments as for
    ensemble_rollout."""
    _refuse("ensemble_ocflow_train", x, ens, prob, nt, stepper, True, noMean, W, family)
    params = [p for _, p in ens._params()]
    fn = _EnsembleTrainMid if family == "mid" else _EnsembleTrain
    Jc, means = fn.apply(x, ens, prob, [float(tspan[0]), float(tspan[1])], int(nt), stepper, alph, *params)
    return Jc, means
