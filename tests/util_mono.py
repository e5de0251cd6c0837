"""oracle-side helpers of the one-CU sweep (CPU only: nothing here touches a GPU)

The one-CU weight-stationary kernels (csrc/nocf_mono.inc forward and recording forward, csrc/nocf_mono_bwd.inc adjoint) keep a two-layer
network of up to 128 hidden units in one workgroup's registers and LDS, the hidden units zero-padded to KBM = 2 / 4 / 6 / 8 blocks of 16 and
the d + 1 inputs to KBD = 1 / 2 blocks.  This module holds a Python mirror of the dispatcher's choice (make_mono_plan, rollout_impl,
nocf_mid_grad_rows, nocf_activation_record_floats of csrc/nocf_kernels.hip), the case lists that reach all 14 forward and 6 adjoint
instantiations, the problems and weights of a case (point agents as in tests/util_lane.py, one and two quadcopters), the oracle restated in
fp32 and fp64 for it (forward, autograd gradients, the five sections of the activation record), the screen that keeps starts off decision
edges (quadcopters: the pair distance over positions, 2r in both modes) and the wrong restatements the comparator must reject.
tests/test_mono_sweep_gpu.py runs the cases on the GPU; tests/test_mono_sweep_cpu.py checks the lists' coverage and the comparator's teeth.

Tolerances are util_oracle's rule unchanged (4 x the fp32 restatement's own error, floor 1e-6 of the scale)."""
import contextlib
import dataclasses
import math

import torch

import util_lane as ul
import util_oracle as uo
from oracle import ocflow_oracle as orc
from util_hip import closed_form_normal
from util_lane import (ALPH, AGENT_R, LINE_Y, MAX_RANK, SPACING, SWARM_Z, T2, VAR0, _summary, autograd_grads, compare_forward,  # noqa: F401
                       failures, recording, screen_starts)

T1 = (0.0, 1.0)
QUAD_R = 0.5                # quadcopters: W's edge is at 2r = 1.0 in both modes
QUAD_GAP = 0.7              # two craft start this far apart along x: inside 2r for most draws of the start spread, outside for some
QUAD_CENTRE = (-1.5, -1.5, -1.5)
ANGLE_STEP = math.sqrt(2.0) / 10.0       # multiples of pi/4 are moved off every reduction boundary by this
BIG_ANGLE = 1000.0                       # mono_sincos takes the library path from |x| = 1000 on
BIG = 16385                              # more than 1024 tiles of 16 rows: an adjoint workgroup walks several tiles


# ---------------------------------------------------------------------------------------------------------------------------------
# the dispatcher, mirrored
# ---------------------------------------------------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def mono_shape(m, d):
    """(KBM, KBD) of make_mono_plan: hidden k-blocks padded up to an instantiated width, input k-blocks"""
    kbm = cdiv(m, 16)
    return (2 if kbm <= 2 else 4 if kbm <= 4 else 6 if kbm <= 6 else 8), cdiv(d + 1, 16)


FORWARD_SHAPES = [(8, 1), (6, 1), (4, 1), (2, 1), (8, 2), (6, 2), (4, 2)]                   # MONO_SHAPES
ADJOINT_SHAPES = [(8, 1), (6, 1), (4, 1), (8, 2), (6, 2), (4, 2)]
FORWARD_INSTANTIATIONS = [(kbm, kbd, rec) for kbm, kbd in FORWARD_SHAPES for rec in (False, True)]


def mono_nag(kbd):
    return 8 if kbd == 1 else 16                                                            # MONO_NAG


def mono_zld(kbd):
    return 20 if kbd == 1 else 36                                                           # MONO_ZLD


def mono_fwd_lds_floats(kbm, kbd):
    """mono_fwd_lds(KBM, KBD).total"""
    T, Z, NA = 16, mono_zld(kbd), mono_nag(kbd)
    return (kbd * 256 + 2 * kbm * 256 + kbd * kbm * 256 + kbd * 256 + 3 * kbm * 16 + kbd * 16 + 4 * 256 + kbd * 4 * 256 + 64 + T * 68 + T * 64
            + T * 16 + 3 * T * Z + 64 + T * NA + 8 + T + T * kbd * 6 + 4 + 4)


def mono_bwd_lds_floats(kbm, kbd):
    """mono_bwd_lds(KBM, KBD).total"""
    T, Z, NA = 16, mono_zld(kbd), mono_nag(kbd)
    return (kbd * 256 + 2 * kbm * 256 + kbd * kbm * 256 + kbd * 256 + 3 * kbm * 16 + kbd * 16 + 1024 + kbd * 1024 + 64 + kbd * 256 + 6 * T * 132
            + T * 68 + T * 64 + T * 16 + T * Z + 64 + T * NA + 8 + T + T * kbd * 6 + 4 + 4 + T * 68 + T * 64 + T * 16 + 4 * T * Z + T * 4 + 8 + 2 * T
            + 3 * kbm * 256)


def mono_plan_ok(nTh, m, d, r, n_agents, bwd=False):
    """make_mono_plan returns 0: an instantiation exists and the shape fits the kernels' compile-time LDS layout"""
    if nTh != 2 or not 1 <= r <= min(MAX_RANK, d + 1) or m < 1 or cdiv(m, 16) > 8:
        return False
    kbm, kbd = mono_shape(m, d)
    if (kbm, kbd) not in FORWARD_SHAPES:
        return False
    if -(-(d + 4) // 4) * 4 > mono_zld(kbd) or n_agents > mono_nag(kbd):
        return False
    return 4 * (mono_bwd_lds_floats(kbm, kbd) if bwd else mono_fwd_lds_floats(kbm, kbd)) <= (160 if bwd else 96) * 1024


def mono_forward_eligible(nTh, m, d, r, kind, n_agents, lane=True, mono=True):
    """rollout_impl takes the one-CU kernel: the lane kernel wins where it is eligible (point agents, m <= 32) unless NOCF_LANE=0"""
    if lane and ul.lane_forward_eligible(nTh, m, d, kind, n_agents):
        return False
    return mono and mono_plan_ok(nTh, m, d, r, n_agents)


def mono_adjoint_eligible(nTh, m, d, r, n_agents):
    """nocf_mid_grad_rows != 0: the one-CU adjoint (KBM in {4, 6, 8}); narrower quadcopter networks take the per-tile adjoint"""
    return m > 32 and mono_plan_ok(nTh, m, d, r, n_agents, bwd=True) and mono_shape(m, d) in ADJOINT_SHAPES


def mono_record_eligible(nTh, m, d, r, n_agents):
    """the recording forward writes the activation record (nocf_activation_record_floats and rollout_impl's mono_rec): whole 16-blocks of
    more than 32 hidden units; otherwise the adjoint recomputes"""
    return m % 16 == 0 and 32 < m <= 128 and d + 1 <= 32 and mono_plan_ok(nTh, m, d, r, n_agents)


def mid_grad_rows(n):
    return min(cdiv(n, 16), 1024)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class MonoCase:
    kind: str                  # "cross2d" / "swarm" / "quad"
    d: int
    m: int
    r: int                     # rows of A
    obstacle: object           # None / "softcorridor" / "hardcorridor" / "blocks"
    mode: str                  # "train" / "eval"
    n: int
    stepper: str
    nt: int
    tspan: tuple = T1
    alph_Q: float = 50.0
    alph_W: float = 30.0
    n_total: object = None     # adjoint cases: the global batch the gradients are normalised by (None: n)
    seed: int = 0
    nTh: int = 2
    mass: float = 1.0          # quadcopters
    grav: float = 9.81
    angles: str = "small"      # quadcopters' start angles: "small" (the start spread) / "quadrants" / "big" (990 ... 1010, both signs)
    act_rec: bool = True       # adjoint cases: False runs with NOCF_ACT_REC=0
    draw: int = 0              # added to the seed of the starts (not of the weights): the segments of one network

    @property
    def agent_dim(self):
        return {"cross2d": 2, "swarm": 3, "quad": 12}[self.kind]

    @property
    def n_agents(self):
        return self.d // self.agent_dim

    @property
    def spec_kind(self):
        return {"cross2d": orc.KIND_CROSS2D, "swarm": orc.KIND_SWARM, "quad": orc.KIND_QUAD}[self.kind]

    @property
    def shape(self):
        return mono_shape(self.m, self.d)

    @property
    def rad(self):
        return QUAD_R if self.kind == "quad" else AGENT_R[self.kind]

    @property
    def alph(self):
        return [ALPH[0], self.alph_Q, self.alph_W, ALPH[3], ALPH[4], ALPH[5]]

    @property
    def id(self):
        v = "-Q0" if self.alph_Q == 0.0 else ("-W0" if self.alph_W == 0.0 else "")
        t = "" if self.tspan == T1 else f"-t{self.tspan[0]:g}_{self.tspan[1]:g}"
        nt = "" if self.n_total is None else f"-of{self.n_total}"
        q = ("" if self.angles == "small" else "-" + self.angles) + ("" if (self.mass, self.grav) == (1.0, 9.81) else f"-M{self.mass:g}g{self.grav:g}")
        return (f"{self.kind}{self.d}-m{self.m}-r{self.r}-{self.obstacle or 'free'}{v}{q}-{self.mode}-n{self.n}{nt}-"
                f"{self.stepper}x{self.nt}{t}" + ("" if self.act_rec else "-norec"))


# per instantiation: the batch, mode, stepper and span of its five small cases and of its batch above 1024 tiles (ragged: BIG + k)
SCHEDULE = [(1, "eval", "rk4", 1, T1), (15, "train", "rk1", 9, T2), (16, "eval", "rk4", 7, T2), (17, "train", "rk4", 7, T1),
            (None, "eval", "rk1", 9, T1), (BIG, "train", "rk4", 7, T1)]
MID_N = {(2, 1): 21, (4, 1): 38, (6, 1): 43, (8, 1): 57, (4, 2): 70, (6, 2): 91, (8, 2): 108}       # n mod 16 = 5, 6, 11, 9, 6, 11, 12

# (kind, d, m, r, obstacle, further fields) in SCHEDULE's order.  Widths on both sides of every padding bound; d + 1 in {13, 15, 16} for
# KBD = 1 and {17, 25, 31} for KBD = 2; r in {1, 10, min(16, d + 1)}; the (2, 1) shape is the quadcopter's alone (point agents of m <= 32
# take the lane kernel)
_SPECS = {
    (2, 1): [("quad", 12, 1, 1, None, {}), ("quad", 12, 16, 10, None, {}), ("quad", 12, 17, 13, None, {}),
             ("quad", 12, 32, 10, None, dict(angles="quadrants")), ("quad", 12, 32, 1, None, dict(mass=1.3, grav=9.0)), ("quad", 12, 17, 10, None, {})],
    (4, 1): [("cross2d", 12, 33, 1, "softcorridor", {}), ("cross2d", 14, 48, 15, "hardcorridor", {}), ("swarm", 15, 49, 16, "blocks", {}),
             ("quad", 12, 64, 13, None, dict(angles="quadrants")), ("cross2d", 14, 64, 10, None, {}), ("swarm", 15, 33, 10, "blocks", {})],
    (6, 1): [("cross2d", 14, 65, 10, "softcorridor", dict(alph_Q=0.0)), ("swarm", 15, 80, 1, "blocks", {}), ("quad", 12, 81, 10, None, {}),
             ("cross2d", 12, 96, 13, "hardcorridor", {}), ("swarm", 15, 96, 16, "blocks", {}), ("cross2d", 14, 80, 15, None, {})],
    (8, 1): [("quad", 12, 97, 10, None, {}), ("cross2d", 14, 100, 1, "hardcorridor", {}), ("swarm", 15, 127, 16, "blocks", {}),
             ("quad", 12, 128, 13, None, dict(angles="big")), ("cross2d", 12, 128, 10, "softcorridor", dict(alph_W=0.0)), ("quad", 12, 128, 10, None, {})],
    (4, 2): [("cross2d", 16, 33, 1, None, {}), ("swarm", 30, 48, 16, "blocks", {}), ("quad", 24, 49, 10, None, {}),
             ("cross2d", 24, 64, 16, "hardcorridor", {}), ("cross2d", 30, 64, 10, "softcorridor", {}), ("cross2d", 24, 48, 10, "softcorridor", {})],
    (6, 2): [("cross2d", 30, 65, 1, "hardcorridor", {}), ("swarm", 30, 80, 10, "blocks", {}), ("cross2d", 16, 81, 16, None, {}),
             ("quad", 24, 96, 16, None, dict(angles="quadrants")), ("cross2d", 24, 96, 10, "softcorridor", {}), ("swarm", 30, 81, 10, "blocks", {})],
    (8, 2): [("swarm", 30, 97, 1, "blocks", {}), ("cross2d", 16, 100, 10, "softcorridor", {}), ("quad", 24, 127, 10, None, dict(mass=0.8, grav=9.0)),
             ("cross2d", 30, 128, 16, "hardcorridor", {}), ("quad", 24, 128, 10, None, {}), ("quad", 24, 100, 16, None, {})],
}


def _forward_cases():
    out = []
    for si, shape in enumerate(FORWARD_SHAPES):
        for k, ((kind, d, m, r, obstacle, kw), (n, mode, stepper, nt, tspan)) in enumerate(zip(_SPECS[shape], SCHEDULE)):
            n = MID_N[shape] if n is None else (n + si if n >= BIG else n)
            out.append(MonoCase(kind, d, m, r, obstacle, mode, n, stepper, nt, tspan, seed=d + 3 * m + r, **kw))
    return out


FORWARD = _forward_cases()


def _A(kind, d, m, r, obstacle, n, stepper, nt, tspan=T1, **kw):
    return MonoCase(kind, d, m, r, obstacle, "train", n, stepper, nt, tspan, seed=d + 3 * m + r + 1, **kw)


# adjoint (train mode, Jc.backward()): per shape a width in whole 16-blocks (the activation record is used) and one that is not (the
# adjoint recomputes); both steppers, both spans, a sharded normalisation, two quadcopters, NOCF_ACT_REC=0, > 1024 tiles at nt = 2
ADJOINT = [
    _A("cross2d", 14, 48, 10, "hardcorridor", 5, "rk4", 7),
    _A("quad", 12, 33, 13, None, 17, "rk1", 9, T2),
    _A("swarm", 15, 96, 16, "blocks", 9, "rk4", 7, T2),
    _A("cross2d", 12, 81, 1, "softcorridor", 3, "rk4", 1, n_total=10),
    _A("quad", 12, 128, 10, None, BIG + 16, "rk4", 2),
    _A("cross2d", 14, 100, 15, None, 21, "rk1", 9),
    _A("cross2d", 24, 64, 16, "softcorridor", 6, "rk4", 7, alph_W=0.0),
    _A("quad", 24, 49, 10, None, 18, "rk4", 7, T2),
    _A("swarm", 30, 80, 10, "blocks", 4, "rk1", 9, act_rec=False),
    _A("cross2d", 16, 65, 1, "hardcorridor", 7, "rk4", 7),
    _A("cross2d", 30, 128, 10, "hardcorridor", 5, "rk4", 7, T2, alph_Q=0.0),
    _A("cross2d", 24, 127, 16, None, 33, "rk4", 1),
]

# nocf_rollout_segments_f32: singlequad's shape, a KBD = 2 point-agent shape, a SwarmTraj shape
SEGMENTS = [
    MonoCase("quad", 12, 128, 10, None, "eval", 0, "rk4", 0, seed=5),
    MonoCase("cross2d", 24, 64, 10, "softcorridor", "eval", 0, "rk4", 0, seed=6),
    MonoCase("swarm", 15, 80, 16, "blocks", "train", 0, "rk1", 0, seed=7),
]
# (number of segments, rows per segment, rows of the ragged last segment): n = (nseg - 1) rows + last is a multiple of neither
SEGMENT_LAYOUTS = [(1, 32, 21), (3, 32, 7), (16, 16, 5)]


def segment_plan(nseg, t1=1.0):
    """-> (t0s, nts, slot0s) of a layout: every segment its own start time and step count, windows that leave gaps between them"""
    t0s = [round(0.05 + 0.9 * k / max(nseg, 2) * t1, 6) for k in range(nseg)]
    nts = [1 + (3 * k + 2) % 5 for k in range(nseg)]
    slot0s = [(2 * k + 1) % 4 for k in range(nseg)]
    return t0s, nts, slot0s


def big_case(shape):
    return next(c for c in FORWARD if c.shape == shape and c.n >= BIG)


# ---------------------------------------------------------------------------------------------------------------------------------
# problems, weights, starts
# ---------------------------------------------------------------------------------------------------------------------------------
def layout(case):
    """(xInit [d], xtarget [d]).  Point agents: tests/util_lane.layout.  Quadcopters: craft k starts at QUAD_CENTRE + k QUAD_GAP e_x at rest,
    its target is (2, 2, 2) - k QUAD_GAP e_x"""
    if case.kind != "quad":
        return ul.layout(case)
    ini, tgt = torch.zeros(case.n_agents, 12), torch.zeros(case.n_agents, 12)
    for k in range(case.n_agents):
        ini[k, :3] = torch.tensor(QUAD_CENTRE) + torch.tensor([k * QUAD_GAP, 0.0, 0.0])
        tgt[k, :3] = torch.tensor([2.0, 2.0, 2.0]) - torch.tensor([k * QUAD_GAP, 0.0, 0.0])
    return ini.reshape(-1), tgt.reshape(-1)


def candidates(case, count):
    """count starts around the layout (spread VAR0); quadcopters with angles "quadrants" / "big" get their angles (and for "big" their
    angular rates) in closed form instead of from the spread"""
    xi, _ = layout(case)
    x = (xi + VAR0 * closed_form_normal(count, case.d, case.seed + case.draw)).contiguous()
    if case.kind == "quad" and case.angles != "small":
        i = torch.arange(count, dtype=torch.float64)
        for c in range(case.n_agents):
            for j in range(3):
                if case.angles == "quadrants":                  # every multiple of pi/4 in [-2 pi, 2 pi) + ANGLE_STEP: 4 quadrants x 2 signs
                    ang = (math.pi / 4) * (((i + 5 * j + 3 * c) % 16) - 8) + ANGLE_STEP
                    x[:, 12 * c + 3 + j] = ang.float()
                else:                                           # 990 ... 1010, odd rows negative; the rate carries the angle across +-1000
                    frac = (i * 0.6180339887498949 + 0.37 * j + 0.21 * c) % 1.0
                    ang = (BIG_ANGLE - 10.0 + 20.0 * frac + ANGLE_STEP * 0.01) * (1.0 - 2.0 * (i % 2))
                    rate = 2.0 * (torch.sign(ang) * BIG_ANGLE - ang)
                    x[:, 12 * c + 3 + j] = ang.float()
                    x[:, 12 * c + 9 + j] = rate.float()
    return x.contiguous()


def make_problem(case, device="cpu"):
    import neuraloc_amd as na
    if case.kind != "quad":
        return ul.make_problem(case, device)
    _, xt = layout(case)
    prob = na.Quadcopter(xt.to(device), obstacle=None, alph_Q=case.alph_Q, alph_W=case.alph_W, mass=case.mass, grav=case.grav, r=QUAD_R)
    prob.train() if case.mode == "train" else prob.eval()
    return prob


def spec(case, mode=None):
    _, xt = layout(case)
    return orc.ProbSpec(kind=case.spec_kind, xtarget=xt, obstacle=case.obstacle, alph_Q=case.alph_Q, alph_W=case.alph_W, r=case.rad,
                        training=(mode or case.mode) == "train", mass=case.mass, grav=case.grav)


def case_sd(case):
    """tests/util_lane.state_dict; with angles "big" the columns of K0 and A that read the angles are scaled by 1e-3, so that an angle of
    1000 enters the network like one of 1 (the case is about the sines and cosines of the physics, not about a saturated network)"""
    sd = ul.state_dict(case.m, case.d, case.r, case.seed, case.nTh)
    if case.kind == "quad" and case.angles == "big":
        for c in range(case.n_agents):
            sd["A"][:, 12 * c + 3:12 * c + 6] *= 1e-3
            sd["N.layers.0.weight"][:, 12 * c + 3:12 * c + 6] *= 1e-3
    return sd


def make_net(case, device):
    import neuraloc_amd as na
    net = na.Phi(nTh=case.nTh, m=case.m, d=case.d, r=case.r, alph=case.alph)
    net.load_state_dict(case_sd(case))
    return net.to(device)


# ---------------------------------------------------------------------------------------------------------------------------------
# the screen
# ---------------------------------------------------------------------------------------------------------------------------------
def quad_pair_distance(stages):
    """stages [B, T, 24] -> [B, T]: the two craft's distance, over positions only"""
    return (stages[..., 0:3].double() - stages[..., 12:15].double()).norm(dim=-1)


def near_edge(case, stages):
    """bool [B]: some evaluated state lies within util_oracle's margins of a decision edge.  Point agents: util_oracle.near_edge.
    Quadcopters: the pair distance over POSITIONS (util_oracle's is over all agent_dim coordinates) against 2r, the edge in both modes"""
    if case.kind != "quad":
        return uo.near_edge(spec(case), stages)
    if case.n_agents < 2 or case.alph_W == 0.0:
        return torch.zeros(stages.shape[0], dtype=torch.bool)
    thr = 2.0 * QUAD_R
    return ((quad_pair_distance(stages) - thr).abs() <= uo.W_REL * thr).any(1)


# ---------------------------------------------------------------------------------------------------------------------------------
# wrong restatements
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ul.MUTATIONS + ("sin_sign_in_one_quadrant", "second_craft_dropped_from_W", "k_block_dropped", "quad_pair_distance_over_all_12")


@contextlib.contextmanager
def _patched(name, fn):
    old = getattr(orc, name)
    setattr(orc, name, fn)
    try:
        yield
    finally:
        setattr(orc, name, old)


def _quad_f_sin_flipped(ang):
    """_quad_f with the sine's sign flipped for angles in the third quadrant, [pi, 3 pi / 2) mod 2 pi"""
    q = torch.floor(torch.remainder(ang, 2 * math.pi) / (math.pi / 2))
    sn = torch.sin(ang) * torch.where(q == 2, -1.0, 1.0).to(ang.dtype)
    cs = torch.cos(ang)
    sps, sth, sph = sn[:, 0], sn[:, 1], sn[:, 2]
    cps, cth, cph = cs[:, 0], cs[:, 1], cs[:, 2]
    return sps * sph + cps * sth * cph, - cps * sph + sps * sth * cph, cth * cph


def _quad_W_all_12(S, x):
    dist = torch.norm(x[:, 0:12] - x[:, 12:24], p=2, dim=1, keepdim=True)
    return (dist < 2 * S.r) * torch.exp(-dist ** 2 / (2 * S.r ** 2))


def _mutation_ctx(mutation):
    if mutation == "train_threshold_in_eval":
        return ul.train_threshold_for_W()
    if mutation == "sin_sign_in_one_quadrant":
        return _patched("_quad_f", _quad_f_sin_flipped)
    if mutation == "second_craft_dropped_from_W":
        return _patched("_quad_W", lambda S, x: (0.0 * x[:, 0]).view(-1, 1))
    if mutation == "quad_pair_distance_over_all_12":
        return _patched("_quad_W", _quad_W_all_12)
    return contextlib.nullcontext()


def _params(sd, dtype, mutation=None):
    if mutation == "k_block_dropped":                              # hidden units 16 k ... of the last (possibly partial) k-block
        P = orc.PhiParams.from_state_dict({k: v.clone() for k, v in sd.items()}, dtype=dtype)
        lo = 16 * (cdiv(P.m, 16) - 1)
        P.K[0][lo:] = 0.0
        P.b[0][lo:] = 0.0
        P.K[1][lo:] = 0.0
        P.K[1][:, lo:] = 0.0
        P.w[:, lo:] = 0.0
        return P
    return ul._params(sd, dtype, mutation)


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle in fp32 and fp64
# ---------------------------------------------------------------------------------------------------------------------------------
def oracle_forward(case, x, dtype, mutation=None, rows=8):
    """tests/util_lane.oracle_forward for a MonoCase: dict table [n, 7], z [n, d+4], zFull / ctrlFull of the first `rows` rows, stages
    [n, evaluations + 1, d] (the final state last), Jc, cs, jc_rows"""
    P = _params(case_sd(case), dtype, mutation)
    S = spec(case).to(dtype)
    t0, t1 = case.tspan
    tspan = [0.0, t1 - t0] if mutation == "time_from_zero" else [t0, t1]
    x = x.to(dtype)
    stages, steps = [], []
    a = case.alph
    with torch.no_grad(), _mutation_ctx(mutation):
        with recording(stages, steps):
            table = orc.persample_table(x, P, S, tspan, case.nt, case.stepper, a)
        zF, cF = orc.rollout(x[:rows], P, S, tspan, case.nt, case.stepper, a, intermediates=True) if rows else (None, None)
    z = steps[-1]
    return _summary(case, dict(table=table, z=z, zFull=zF, ctrlFull=cF, stages=torch.stack(stages + [z[:, :case.d]], 1)))


def oracle_grads(case, x, dtype):
    """fp autograd of the oracle's Jc, normalised like the adjoint: by the case's n_total -> (Jc, {name: gradient}, dJc/dx)"""
    return autograd_grads(case_sd(case), spec(case), x, case.tspan, case.nt, case.stepper, case.alph, dtype,
                          x.shape[0] / (case.n_total or x.shape[0]))


SECTIONS = ("u0", "tanh_o", "tanh_q", "a", "grad")


def oracle_activations(case, s):
    """the five sections of the activation record at the stage inputs s [E, n, d+1] (fp32: the kernel's own recorded inputs), from the
    oracle's grad Phi (ocflow_oracle.phi_grad's intermediates) -> ({section: [E, n, m or d+1]} in fp64, the same in fp32)"""
    out = []
    E, n, D1 = s.shape
    for dtype in (torch.float64, torch.float32):
        P = orc.PhiParams.from_state_dict(case_sd(case), dtype=dtype)
        parts = {}
        with torch.no_grad():
            orc.phi_grad(P, s.reshape(E * n, D1).to(dtype), parts)
        out.append({k: parts[k].reshape(E, n, -1) for k in SECTIONS})
    return tuple(out)


def stage_times(case):
    """the time of every right-hand-side evaluation, in the kernel's order [nt * nstage]"""
    t0, t1 = case.tspan
    h = (t1 - t0) / case.nt
    offs = (0.0, 0.5, 0.5, 1.0) if case.stepper == "rk4" else (0.0,)
    return [t0 + (k + o) * h for k in range(case.nt) for o in offs]


_CACHE = {}


def case_data(case):
    """-> dict x [n, d] (the first n of n + max(16, n / 2) candidates that pass the screen), r64 / r32 (oracle_forward); cached per case"""
    if case in _CACHE:
        return _CACHE[case]
    cand = candidates(case, case.n + max(16, case.n // 2))
    r64 = oracle_forward(case, cand.double(), torch.float64, rows=0)
    keep = (~near_edge(case, r64["stages"])).nonzero().flatten()[:case.n]
    assert keep.numel() == case.n, f"{case.id}: only {keep.numel()} of {cand.shape[0]} starts pass the screen"
    x = cand[keep].contiguous()
    r64 = _summary(case, {k: r64[k][keep] for k in ("table", "z", "stages")})         # (rows are independent)
    head = oracle_forward(case, x[:8].double(), torch.float64)
    r64["zFull"], r64["ctrlFull"] = head["zFull"], head["ctrlFull"]
    r32 = oracle_forward(case, x, torch.float32)
    _CACHE[case] = out = dict(x=x, r64=r64, r32=r32)
    return out


def quadrant_signs(angles):
    """angles [...] -> the set of (quadrant 0..3 of the angle mod 2 pi, angle < 0) pairs present"""
    a = angles.double().flatten()
    q = torch.floor(torch.remainder(a, 2 * math.pi) / (math.pi / 2)).long().clamp(0, 3)
    return {(int(qq), bool(neg)) for qq, neg in zip(q.tolist(), (a < 0).tolist())}


def physics_gaps(case, r64):
    """-> the reasons the case does not exercise what it should (empty: it does): Q > 0 in some sample with an obstacle and alph_Q != 0,
    W > 0 with alph_W != 0 and >= 2 agents, exactly 0 where switched off (quadcopters have no obstacle: Q = 0); two quadcopters: W = 0 in
    some sample too (the 2r edge lies inside the batch); angle cases: all eight quadrant / sign pairs, both sides of 1000"""
    out = []
    q, w = r64["table"][:, 5], r64["table"][:, 6]
    n_small = case.n < 16
    if case.obstacle is not None and case.alph_Q != 0.0 and not bool((q > 0).any()):
        out.append("Q is 0 in every sample")
    if case.alph_W != 0.0 and case.n_agents >= 2 and not bool((w > 0).any()) and not (case.kind == "quad" and n_small):
        out.append("W is 0 in every sample")
    if (case.alph_Q == 0.0 or case.obstacle is None) and bool((q != 0).any()):
        out.append("Q switched off but Q != 0")
    if (case.alph_W == 0.0 or case.n_agents < 2) and bool((w != 0).any()):
        out.append("W switched off but W != 0")
    if case.kind == "quad":
        ang = torch.cat([r64["stages"][..., 12 * c + 3:12 * c + 6] for c in range(case.n_agents)], -1)
        if case.angles == "quadrants" and len(quadrant_signs(ang)) != 8:
            out.append("the angles do not visit all four quadrants with both signs")
        if case.angles == "big":
            for sgn in (1.0, -1.0):
                a = sgn * ang
                if not (bool(((a > 0) & (a < BIG_ANGLE)).any()) and bool((a >= BIG_ANGLE).any())):
                    out.append(f"the angles of sign {sgn:+.0f} do not lie on both sides of 1000")
    return out
