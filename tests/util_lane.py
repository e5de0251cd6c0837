"""oracle-side helpers of the small-network lane sweep (CPU only: nothing here touches a GPU)

The lane kernels (csrc/nocf_lane.inc forward, csrc/nocf_lane_bwd.inc adjoint) run one wavefront per sample with the weights zero-padded
into register arrays of compile-time size (MP, DP).  This module holds a Python mirror of the dispatcher's choice, the case list that
reaches all six instantiations, the problems and weights of a case, the oracle restated in fp32 and fp64 for it (forward and autograd
gradients), the screen that keeps starts off decision edges, and the physics checks every case must pass.  tests/test_lane_sweep_gpu.py
runs the cases on the GPU; tests/test_lane_sweep_cpu.py checks the case list's coverage and that the comparator has teeth on it."""
import contextlib
import dataclasses

import torch

import util_oracle as uo
from oracle import ocflow_oracle as orc
from util_hip import closed_form_normal, synth_state_dict

ALPH = (100.0, 0.0, 0.0, 0.5, 0.25, 0.125)          # OCflow's 6 multipliers; entries 1 and 2 are taken from the case's alph_Q / alph_W
VAR0 = 0.25                                          # start spread around the layout
SPACING = {"cross2d": 1.0, "swarm": 0.7}             # neighbours on the line start this far apart ...
AGENT_R = {"cross2d": 0.6, "swarm": 0.4}             # ... inside the W threshold 2r (eval), 2.2r / 3.2r (train)
LINE_Y = {None: 0.0, "softcorridor": 0.0, "hardcorridor": 2.5}    # Cross2D: the corridor's Gaussians / inside the upper hard disc
SWARM_Z = 3.0                                                      # SwarmTraj: the line runs through both blocks
MAX_RANK = 16                                                      # the rollout plans' limit on the rows of A (ZQLD)


# ---------------------------------------------------------------------------------------------------------------------------------
# the dispatcher, mirrored (csrc/nocf_kernels.hip: rollout_impl and nocf_rollout_bwd_small_f32)
# ---------------------------------------------------------------------------------------------------------------------------------
def lane_shape(m, d):
    """the (MP, DP) instantiation a lane launch of width m and d+1 inputs takes"""
    return (16 if m <= 16 else 32, 8 if d + 1 <= 8 else (16 if d + 1 <= 16 else 32))


def lane_forward_eligible(nTh, m, d, kind, n_agents):
    return nTh == 2 and m <= 32 and d + 1 <= 32 and kind != orc.KIND_QUAD and n_agents <= 16


def lane_adjoint_eligible(nTh, m, d, kind, n_agents):
    return lane_forward_eligible(nTh, m, d, kind, n_agents) and kind == orc.KIND_CROSS2D and 2 * n_agents == d


def agent_pairs(N):
    """the unordered pairs in the order the forward kernel enumerates them (lane q of trip tr takes pair q + 64 tr)"""
    return [(i, j) for i in range(N) for j in range(i + 1, N)]


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class LaneCase:
    kind: str                  # "cross2d" / "swarm"
    d: int
    m: int
    r: int                     # rows of A
    obstacle: object           # None / "softcorridor" / "hardcorridor" / "blocks"
    mode: str                  # "train" / "eval"
    n: int
    stepper: str
    nt: int
    tspan: tuple = (0.0, 1.0)
    alph_Q: float = 50.0
    alph_W: float = 30.0
    n_total: object = None     # adjoint cases: the global batch the gradients are normalised by (None: n)
    seed: int = 0
    nTh: int = 2               # (the lane kernels take nTh = 2 only: other depths are eligibility-boundary cases)

    @property
    def agent_dim(self):
        return 2 if self.kind == "cross2d" else 3

    @property
    def n_agents(self):
        return self.d // self.agent_dim

    @property
    def spec_kind(self):
        return orc.KIND_CROSS2D if self.kind == "cross2d" else orc.KIND_SWARM

    @property
    def shape(self):
        return lane_shape(self.m, self.d)

    @property
    def alph(self):
        return [ALPH[0], self.alph_Q, self.alph_W, ALPH[3], ALPH[4], ALPH[5]]

    @property
    def id(self):
        v = "-Q0" if self.alph_Q == 0.0 else ("-W0" if self.alph_W == 0.0 else "")
        t = "" if self.tspan == (0.0, 1.0) else f"-t{self.tspan[0]:g}_{self.tspan[1]:g}"
        nt = "" if self.n_total is None else f"-of{self.n_total}"
        return (f"{self.kind}{self.d}-m{self.m}-r{self.r}-{self.obstacle or 'free'}{v}-{self.mode}-n{self.n}{nt}-"
                f"{self.stepper}x{self.nt}{t}")


def _F(kind, d, m, r, obstacle, mode, n, stepper, nt, tspan=(0.0, 1.0), **kw):
    return LaneCase(kind, d, m, r, obstacle, mode, n, stepper, nt, tspan, seed=d + 3 * m + r, **kw)


T2 = (0.25, 0.9)
BIG = 4097             # the grid exceeds 1024 workgroups from here on

# (one agent, d = 2: alph_W = 0 -- the reference's interaction cost of a single agent is a row vector that broadcasts L to [n, n])
# forward: per instantiation n = 1, 2, 3 (mod 4), one batch of >= BIG rows; MP = 16 from m in {1, 7, 9, 16}, MP = 32 from {17, 31, 32};
# DP = 8 / 16 / 32 from Cross2D d + 1 in {3, 5, 7} / {9, 15} / {17, 25, 31} and SwarmTraj d + 1 = 16 (fills DP) / 31
FORWARD = [
    # (16, 8)
    _F("cross2d", 2, 1, 1, "softcorridor", "eval", 1, "rk4", 1, alph_W=0.0),
    _F("cross2d", 4, 7, 3, "hardcorridor", "train", 6, "rk1", 9, T2),
    _F("cross2d", 6, 16, 7, None, "eval", 11, "rk4", 7),
    _F("cross2d", 4, 9, 5, "softcorridor", "train", BIG, "rk4", 7),
    # (16, 16)
    _F("cross2d", 8, 9, 1, "hardcorridor", "eval", 2, "rk4", 7, T2),
    _F("swarm", 15, 16, 16, "blocks", "train", 5, "rk4", 1),
    _F("cross2d", 14, 1, 8, "softcorridor", "train", 7, "rk1", 9, alph_W=0.0),
    _F("swarm", 15, 7, 4, "blocks", "eval", BIG + 1, "rk4", 7),
    # (16, 32)
    _F("cross2d", 16, 16, 16, None, "train", 3, "rk4", 7),
    _F("cross2d", 30, 7, 1, None, "eval", 9, "rk4", 1, T2),
    _F("swarm", 30, 9, 8, "blocks", "train", 6, "rk1", 9, alph_Q=0.0),
    _F("cross2d", 24, 16, 12, "hardcorridor", "train", BIG + 2, "rk4", 7),
    # (32, 8)
    _F("cross2d", 2, 17, 3, "hardcorridor", "train", 2, "rk4", 7, alph_W=0.0),
    _F("cross2d", 6, 31, 1, "softcorridor", "eval", 3, "rk1", 9, T2),
    _F("cross2d", 4, 32, 5, "softcorridor", "eval", 5, "rk4", 1, alph_Q=0.0),
    _F("cross2d", 6, 32, 7, None, "train", BIG, "rk4", 7),
    # (32, 16)
    _F("swarm", 15, 17, 1, "blocks", "eval", 1, "rk4", 7),
    _F("cross2d", 14, 32, 15, "hardcorridor", "train", 10, "rk1", 9, T2),
    _F("cross2d", 8, 31, 9, "softcorridor", "train", 7, "rk4", 7),
    _F("cross2d", 14, 17, 4, None, "eval", BIG + 1, "rk4", 1),
    # (32, 32)
    _F("cross2d", 30, 32, 16, "softcorridor", "train", 13, "rk4", 7),
    _F("swarm", 30, 31, 1, "blocks", "train", 2, "rk4", 7, T2),
    _F("cross2d", 24, 17, 12, None, "eval", 3, "rk1", 9),
    _F("cross2d", 16, 32, 6, "hardcorridor", "eval", BIG + 3, "rk4", 7),
]

# adjoint (Cross2D, train mode, Jc.backward()): every instantiation, both steppers, both spans, one sharded normalisation
ADJOINT = [
    _F("cross2d", 4, 16, 1, "hardcorridor", "train", 5, "rk4", 7),
    _F("cross2d", 2, 1, 3, "softcorridor", "train", 2, "rk1", 9, T2, alph_W=0.0),
    _F("cross2d", 8, 9, 9, "softcorridor", "train", 3, "rk4", 7, T2),
    _F("cross2d", 14, 7, 4, "hardcorridor", "train", 6, "rk1", 9, n_total=10),
    _F("cross2d", 30, 16, 16, None, "train", 7, "rk4", 7),
    _F("cross2d", 16, 9, 1, "softcorridor", "train", 1, "rk4", 1),
    _F("cross2d", 6, 32, 7, "softcorridor", "train", 9, "rk4", 7, alph_Q=0.0),
    _F("cross2d", 14, 17, 15, None, "train", 2, "rk4", 7, T2),
    _F("cross2d", 24, 31, 8, "hardcorridor", "train", 3, "rk4", 7),
    _F("cross2d", 30, 32, 1, "softcorridor", "train", 5, "rk1", 9, alph_W=0.0),
]

INSTANTIATIONS = [(mp, dp) for mp in (16, 32) for dp in (8, 16, 32)]


def big_case(shape):
    """the forward case of >= BIG rows of one instantiation"""
    return next(c for c in FORWARD if c.shape == shape and c.n >= BIG)


# ---------------------------------------------------------------------------------------------------------------------------------
# problems, weights, starts
# ---------------------------------------------------------------------------------------------------------------------------------
def layout(case):
    """(xInit [d], xtarget [d]): agents on a line SPACING apart, targets mirrored along it"""
    N, sp = case.n_agents, SPACING[case.kind]
    xx = sp * (torch.arange(N, dtype=torch.float64) - 0.5 * (N - 1))
    if case.kind == "cross2d":
        y0 = LINE_Y[case.obstacle]
        ini = torch.stack([xx, torch.full_like(xx, y0)], 1)
        tgt = torch.stack([xx.flip(0), torch.full_like(xx, -y0 + 1.0)], 1)
    else:
        ini = torch.stack([xx + 0.5, torch.zeros_like(xx), torch.full_like(xx, SWARM_Z)], 1)
        tgt = torch.stack([xx.flip(0) + 0.5, torch.full_like(xx, 0.5), torch.full_like(xx, SWARM_Z + 3.0)], 1)
    return ini.reshape(-1).float(), tgt.reshape(-1).float()


def make_problem(case, device="cpu"):
    """the package's problem object, in the case's mode"""
    import neuraloc_amd as na
    _, xt = layout(case)
    cls = na.Cross2D if case.kind == "cross2d" else na.SwarmTraj
    prob = cls(xt.to(device), obstacle=case.obstacle, alph_Q=case.alph_Q, alph_W=case.alph_W, r=AGENT_R[case.kind])
    prob.train() if case.mode == "train" else prob.eval()
    return prob


def spec(case, mode=None):
    _, xt = layout(case)
    return orc.ProbSpec(kind=case.spec_kind, xtarget=xt, obstacle=case.obstacle, alph_Q=case.alph_Q, alph_W=case.alph_W,
                        r=AGENT_R[case.kind], training=(mode or case.mode) == "train")


def state_dict(m, d, r, seed, nTh=2):
    """util_hip.synth_state_dict with A replaced by a closed-form (r, d+1) matrix"""
    sd = synth_state_dict(nTh, m, d, seed)
    i = torch.arange(r, dtype=torch.float64).unsqueeze(1)
    j = torch.arange(d + 1, dtype=torch.float64).unsqueeze(0)
    sd["A"] = (torch.sin(0.37 * i + 0.11 * j + 0.1 + seed) / (d + 1) ** 0.5).float()
    return sd


def make_net(case, device):
    import neuraloc_amd as na
    net = na.Phi(nTh=case.nTh, m=case.m, d=case.d, r=case.r, alph=case.alph)
    net.load_state_dict(case_sd(case))
    return net.to(device)


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle in fp32 and fp64
# ---------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def recording(stages, steps):
    """while active, every state the oracle's rollout evaluates its right-hand side at (each RK stage) is appended to `stages`, and the
    state after every step to `steps` ([n, d] / [n, d+4] each)"""
    rhs, rk4, rk1 = orc.rhs, orc.step_rk4, orc.step_rk1

    def rec(P, S, z, t):
        stages.append(z[:, :-4].detach().clone())
        return rhs(P, S, z, t)

    def stepper(f):
        def step(*a):
            z = f(*a)
            steps.append(z.detach().clone())
            return z
        return step
    orc.rhs, orc.step_rk4, orc.step_rk1 = rec, stepper(rk4), stepper(rk1)
    try:
        yield
    finally:
        orc.rhs, orc.step_rk4, orc.step_rk1 = rhs, rk4, rk1


@contextlib.contextmanager
def train_threshold_for_W():
    """mutation: the interaction cost takes the train-mode threshold whatever the problem's mode"""
    prob_W = orc.prob_W
    orc.prob_W = lambda S, x: prob_W(dataclasses.replace(S, training=True), x)
    try:
        yield
    finally:
        orc.prob_W = prob_W


MUTATIONS = ("rank_minus_one", "last_hidden_dropped", "time_from_zero", "train_threshold_in_eval")


def _params(sd, dtype, mutation=None):
    P = orc.PhiParams.from_state_dict({k: v.clone() for k, v in sd.items()}, dtype=dtype)
    if mutation == "rank_minus_one":
        P.A = P.A[:-1]
    elif mutation == "last_hidden_dropped":
        P.K[0][-1] = 0.0
        P.b[0][-1] = 0.0
        P.K[1][-1] = 0.0
        P.K[1][:, -1] = 0.0
        P.w[:, -1] = 0.0
    return P


def oracle_forward(case, x, dtype, mutation=None, rows=8):
    """the oracle on starts x in `dtype` -> dict Jc, cs [7] (the means and Jc of src/OCflow.py:78-86 over the table's columns), table
    [n, 7] (persample_table), jc_rows [n] (noMean's Jc), z [n, d+4] (final state), zFull / ctrlFull of the first `rows` rows
    ([rows, ., nt+1]), stages [n, evaluations + 1, d] (every state a cost was evaluated at, the final one last)"""
    P = _params(case_sd(case), dtype, mutation)
    S = spec(case).to(dtype)
    t0, t1 = case.tspan
    tspan = [0.0, t1 - t0] if mutation == "time_from_zero" else [t0, t1]
    x = x.to(dtype)
    ctx = train_threshold_for_W() if mutation == "train_threshold_in_eval" else contextlib.nullcontext()
    stages, steps = [], []
    a = case.alph
    with torch.no_grad(), ctx:
        with recording(stages, steps):
            table = orc.persample_table(x, P, S, tspan, case.nt, case.stepper, a)
        zF, cF = orc.rollout(x[:rows], P, S, tspan, case.nt, case.stepper, a, intermediates=True) if rows else (None, None)
    z = steps[-1]
    return _summary(case, dict(table=table, z=z, zFull=zF, ctrlFull=cF, stages=torch.stack(stages + [z[:, :case.d]], 1)))


def _summary(case, res):
    """adds Jc, cs and jc_rows, formed from the table as src/OCflow.py:66-86 forms them"""
    a, tab = case.alph, res["table"]
    res["jc_rows"] = tab[:, 0] + a[0] * tab[:, 1] + a[3] * tab[:, 2] + a[4] * tab[:, 3] + a[5] * tab[:, 4]
    cs = res["cs"] = tab.mean(0)
    res["Jc"] = cs[0] + a[0] * cs[1] + a[3] * cs[2] + a[4] * cs[3] + a[5] * cs[4]
    return res


def autograd_grads(sd, S, x, tspan, nt, stepper, alph, dtype, scale=1.0):
    """Jc of the oracle in `dtype` and, by torch autograd, scale * dJc/dtheta and scale * dJc/dx -> (Jc, {parameter name: gradient}, x
    gradient).  S: ProbSpec (CPU)"""
    P = orc.PhiParams.from_state_dict({k: v.clone() for k, v in sd.items()}, dtype=dtype)
    for t in [*P.K, *P.b, P.w, P.A, P.cw, P.cb]:
        t.requires_grad_(True)
    xx = x.detach().cpu().to(dtype).clone().requires_grad_(True)
    J, _ = orc.rollout(xx, P, S.to(dtype), list(tspan), nt, stepper, alph)
    (J * scale).backward()
    out = {"A": P.A.grad, "c.weight": P.cw.grad, "c.bias": P.cb.grad, "w.weight": P.w.grad}
    for i in range(P.nTh):
        out[f"N.layers.{i}.weight"], out[f"N.layers.{i}.bias"] = P.K[i].grad, P.b[i].grad
    return float(J.detach()), out, xx.grad


def oracle_grads(case, x, dtype):
    """autograd_grads for a case, normalised like the adjoint: by the case's n_total"""
    return autograd_grads(case_sd(case), spec(case), x, case.tspan, case.nt, case.stepper, case.alph, dtype,
                          x.shape[0] / (case.n_total or x.shape[0]))


def oracle_grads64(x, sd, prob, nt, stepper, alph, nTh=None, tspan=(0.0, 1.0)):
    """the oracle differentiated by torch autograd in fp64 for a package problem object -> (Jc, {parameter name: gradient})"""
    S = orc.ProbSpec.from_object(prob)
    S.xtarget = S.xtarget.cpu()
    J, out, _ = autograd_grads(sd, S, x, tspan, nt, stepper, alph, torch.float64)
    return J, out


def screen_starts(sd, S, cand, tspan, nt, stepper, alph, n):
    """the first n rows of cand [*, d] whose every evaluated state (fp64 oracle) passes util_oracle.near_edge"""
    P = orc.PhiParams.from_state_dict(sd, dtype=torch.float64)
    stages, steps = [], []
    with torch.no_grad(), recording(stages, steps):
        orc.persample_table(cand.double(), P, S.to(torch.float64), list(tspan), nt, stepper, alph)
    d = cand.shape[1]
    keep = (~uo.near_edge(S, torch.stack(stages + [steps[-1][:, :d]], 1))).nonzero().flatten()[:n]
    assert keep.numel() == n, f"only {keep.numel()} of {cand.shape[0]} starts pass the screen"
    return cand[keep].contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# starts and the screen
# ---------------------------------------------------------------------------------------------------------------------------------
def pair_hits(case, stages):
    """stages [B, T, d] -> bool [B, pairs]: the pair came inside the W threshold of the case's mode at some evaluated state"""
    S = spec(case)
    N, ad = case.n_agents, case.agent_dim
    pr = agent_pairs(N)
    if not pr:
        return torch.zeros(stages.shape[0], 0, dtype=torch.bool)
    X = stages.double().reshape(stages.shape[0], stages.shape[1], N, ad)
    i = torch.tensor([p[0] for p in pr])
    j = torch.tensor([p[1] for p in pr])
    dist = (X[:, :, i] - X[:, :, j]).norm(dim=-1)
    fac = (3.2 if (S.kind == orc.KIND_SWARM and N > 2) else 2.2) if S.training else 2.0
    return (dist < fac * S.r).any(1)


def near_edge(case, stages):
    """util_oracle.near_edge on every evaluated state (both modes' W thresholds, the hard-corridor discs, the blocks)"""
    return uo.near_edge(spec(case), stages)


_CACHE = {}


def case_sd(case):
    return state_dict(case.m, case.d, case.r, case.seed, case.nTh)


def case_data(case):
    """-> dict x [n, d] (the first starts that pass the screen), r64 / r32 (oracle_forward in fp64 / fp32); cached per case"""
    if case in _CACHE:
        return _CACHE[case]
    xi, _ = layout(case)
    extra = max(16, case.n // 2)
    cand = (xi + VAR0 * closed_form_normal(case.n + extra, case.d, case.seed)).contiguous()
    r64 = oracle_forward(case, cand.double(), torch.float64, rows=0)
    keep = (~near_edge(case, r64["stages"])).nonzero().flatten()[:case.n]
    assert keep.numel() == case.n, f"{case.id}: only {keep.numel()} of {cand.shape[0]} starts pass the screen"
    x = cand[keep].contiguous()
    # (rows are independent: the screened rows' fp64 results are those of the candidates)
    r64 = _summary(case, {k: r64[k][keep] for k in ("table", "z", "stages")})
    head = oracle_forward(case, x[:8].double(), torch.float64)
    r64["zFull"], r64["ctrlFull"] = head["zFull"], head["ctrlFull"]
    r32 = oracle_forward(case, x, torch.float32)
    _CACHE[case] = out = dict(x=x, r64=r64, r32=r32)
    return out


def physics_gaps(case, r64):
    """-> the reasons the case does not exercise what it should (empty: it does): with an obstacle and alph_Q != 0 the fp64 Q column is
    > 0 in some sample, with alph_W != 0 and N >= 2 so is the W column; switched off: exactly 0.  N >= 12: some pair of enumeration index
    >= 64 (the kernel's second trip) comes inside the W threshold in some sample."""
    out = []
    q, w = r64["table"][:, 5], r64["table"][:, 6]
    if case.obstacle is not None and case.alph_Q != 0.0 and not bool((q > 0).any()):
        out.append("Q is 0 in every sample")
    if case.alph_W != 0.0 and case.n_agents >= 2 and not bool((w > 0).any()):
        out.append("W is 0 in every sample")
    if case.alph_Q == 0.0 and bool((q != 0).any()):
        out.append("alph_Q = 0 but Q != 0")
    if case.alph_W == 0.0 and bool((w != 0).any()):
        out.append("alph_W = 0 but W != 0")
    if case.n_agents >= 12 and case.alph_W != 0.0 and not bool(pair_hits(case, r64["stages"])[:, 64:].any()):
        out.append("no pair of index >= 64 comes inside the W threshold")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparator (util_oracle's rule) over a forward result
# ---------------------------------------------------------------------------------------------------------------------------------
def compare_forward(got, r64, r32, rows=None):
    """got: dict with any of Jc, cs, table, z, zFull, ctrlFull (CPU or device tensors).  Each quantity against fp64 under util_oracle's
    tolerance; a mean (Jc, each of cs) may also be off by its per-sample column's tolerance, the error allowed in every term it averages.
    -> {name: (ok, err, tol, err32)}"""
    out = {}
    tab64, tab32 = r64["table"], r32["table"]
    for k in ("table", "z", "zFull", "ctrlFull"):
        if k in got:
            out[k] = uo.compare(got[k], r64[k], r32[k])
    if "table" in got:
        for c in range(7):
            out[f"table[:, {c}]"] = uo.compare(got["table"][:, c], tab64[:, c], tab32[:, c])
    if "cs" in got:
        for c in range(7):
            tol, e32 = uo.tolerance(r64["cs"][c], r32["cs"][c])
            tol = max(tol, uo.tolerance(tab64[:, c], tab32[:, c])[0])
            err = abs(float(got["cs"][c]) - float(r64["cs"][c]))
            out[f"cs[{c}]"] = (err <= tol, err, tol, e32)
    if "Jc" in got:
        tol, e32 = uo.tolerance(r64["Jc"], r32["Jc"])
        tol = max(tol, uo.tolerance(r64["jc_rows"], r32["jc_rows"])[0])
        err = abs(float(got["Jc"]) - float(r64["Jc"]))
        out["Jc"] = (err <= tol, err, tol, e32)
    return out


def failures(res):
    return {k: v for k, v in res.items() if not v[0]}
