"""oracle-side helpers of the zero-order-hold rollout's tests (CPU only: nothing here touches a GPU)

The reference has no rollout whose control is held between samples, so the yardstick is the contract of nocf_rollout_held_f32
(include/nocf.h) restated with oracle.ocflow_oracle's functions -- phi_grad, prob_ctrls, prob_LHQW, prob_Q, _quad_f and the terminal block
of oracle.rollout -- in the dtype of x, fp32 and fp64.  Cases are util_mono.MonoCase (its make_net / make_problem / candidates serve point
agents and quadcopters of any width); tests/test_hold_gpu.py runs them on the GPU, tests/test_hold_cpu.py checks the restatement, the
screen's cap and that the comparator has teeth on wrong restatements."""
import torch
import torch.nn.functional as F

import util_disturb as ud
import util_lane as ul
import util_mono as um
from oracle import ocflow_oracle as orc

T1, T2 = ud.T1, ud.T2

# wrong restatements: the control sampled from the state before W[k-1] is added; the control re-sampled at every step whatever K is; L formed
# from the costate at the stage state instead of the held control; the HJB column integrated as the closed loop does; the quadcopter's
# f7..f9 frozen at the sampling instant
MUTATIONS = ("ctrl_undisplaced", "resample_every_step", "L_from_current_costate", "hjt_not_zeroed", "f_frozen_at_sample")


def _sample(P, S, x, t):
    """the controller's sample at (x, t) -> dict p [n, d] (grad_x Phi), ctrl (calcCtrls), and for the quadcopter u [n, 1], f (f7, f8, f9)"""
    d = x.shape[1]
    p = orc.phi_grad(P, F.pad(x, [0, 1, 0, 0], value=t))[:, 0:d]
    out = dict(p=p, ctrl=orc.prob_ctrls(S, x, p))
    if S.kind == orc.KIND_QUAD:
        u, f7, f8, f9 = orc._quad_u(S, x, p)
        out.update(u=u, f=(f7, f8, f9))
    return out


def held_rhs(P, S, z, t, smp, mutation=None):
    """the right-hand side [ f(x, c) | L(x, c) | 0 | Q(x) | W(x) ] at the stage state z with the control of sample smp held"""
    n, width = z.shape
    d = width - 4
    x, p = z[:, :d], smp["p"]
    out = torch.zeros(n, d + 4, dtype=z.dtype)
    g = None
    if mutation in ("L_from_current_costate", "hjt_not_zeroed"):
        g = orc.phi_grad(P, F.pad(x, [0, 1, 0, 0], value=t))
    if S.kind != orc.KIND_QUAD:
        out[:, :d] = -p                                                    # f = c = -p
        L, _, Q, W = orc.prob_LHQW(S, x, g[:, :d] if mutation == "L_from_current_costate" else p)
    else:
        assert S.n_agents == 1, "the held rollout takes one craft"
        u = smp["u"]
        f7, f8, f9 = smp["f"] if mutation == "f_frozen_at_sample" else orc._quad_f(x[:, 3:6])
        um_ = u / S.mass
        out[:, 0:6] = x[:, 6:12]
        out[:, 6:9] = torch.cat((um_ * f7.view(-1, 1), um_ * f8.view(-1, 1), um_ * f9.view(-1, 1) - S.grav), 1)
        out[:, 9:12] = -0.5 * p[:, 9:12]                                   # tau
        Q = orc.prob_Q(S, x).view(-1, 1)
        pl = g[:, :d] if mutation == "L_from_current_costate" else p
        ul_ = orc._quad_u(S, x, pl)[0] if mutation == "L_from_current_costate" else u
        sq = (pl[:, 9] ** 2 + pl[:, 10] ** 2 + pl[:, 11] ** 2).view(-1, 1)
        L = S.alph_Q * Q + 2 + ul_ ** 2 + 0.25 * sq                        # 2 + u^2 + |tau|^2
        W = 0.0 * L
    out[:, d] = L.squeeze(1)
    if mutation == "hjt_not_zeroed":
        _, H, _, _ = orc.prob_LHQW(S, x, g[:, :d])
        out[:, d + 1] = torch.abs(g[:, -1] - H.squeeze(1))
    out[:, d + 2] = torch.as_tensor(Q, dtype=z.dtype).reshape(n)
    out[:, d + 3] = torch.as_tensor(W, dtype=z.dtype).reshape(n)
    return out


def restate(P, S, x, W, hold, tspan, nt, stepper, alph, mutation=None, states=None):
    """The held rollout in the dtype of x.  W [nt, n, d] or None.  mutation: one of MUTATIONS, a deliberately wrong restatement.  states:
    a list that receives every sampled, stage and displaced state [n, d].
    -> dict table [n, 7], z [n, d+4], zFull [n, d+4, nt+1], ctrlFull [n, a, nt+1]"""
    n, d = x.shape
    if W is not None:
        W = W.to(x.dtype)
    h = (tspan[1] - tspan[0]) / nt
    z = torch.cat((x, torch.zeros(n, 4, dtype=x.dtype)), 1)
    tk = tspan[0]
    zFull = torch.zeros(n, d + 4, nt + 1, dtype=x.dtype)
    zFull[:, :, 0] = z
    undisplaced = x
    smp = None
    K = 1 if mutation == "resample_every_step" else hold

    def rhs(zz, t):
        if states is not None:
            states.append(zz[:, :d].clone())
        return held_rhs(P, S, zz, t, smp, mutation)

    for k in range(nt):
        if k % K == 0:
            smp = _sample(P, S, undisplaced if mutation == "ctrl_undisplaced" else z[:, :d], tk)
        t1 = tk + h
        hs = t1 - tk                                                       # the steppers re-derive h (src/OCflow.py:170)
        if stepper == "rk4":
            z0 = z
            kk = hs * rhs(z0, tk)
            z = z0 + (1.0 / 6.0) * kk
            kk = hs * rhs(z0 + 0.5 * kk, tk + (hs / 2))
            z = z + (2.0 / 6.0) * kk
            kk = hs * rhs(z0 + 0.5 * kk, tk + (hs / 2))
            z = z + (2.0 / 6.0) * kk
            kk = hs * rhs(z0 + kk, tk + hs)
            z = z + (1.0 / 6.0) * kk
        else:
            z = z + hs * rhs(z, tk)
        undisplaced = z[:, :d].clone()
        if W is not None:
            z = z.clone()
            z[:, :d] += W[k]
        if states is not None:
            states.append(z[:, :d].clone())
        tk += h
        zFull[:, :, k + 1] = z
        if k == 0:
            ctrlFull = torch.zeros(*smp["ctrl"].shape, nt + 1, dtype=x.dtype)
        ctrlFull[:, :, k + 1] = smp["ctrl"]
    # the terminal block of oracle.rollout (src/OCflow.py:58-76)
    resG = z[:, 0:d] - S.xtarget
    cG = 0.5 * torch.sum(resG ** 2, 1, keepdims=True)
    sT = F.pad(z[:, 0:d], [0, 1, 0, 0], value=tspan[1])
    phi1 = orc.phi_value(P, sT)
    gphi1 = orc.phi_grad(P, sT)[:, 0:d]
    cHJf = torch.sum(torch.abs(phi1 - alph[0] * cG), 1).view(-1, 1)
    cHJg = torch.sum(torch.abs(gphi1 - alph[0] * resG), 1).view(-1, 1)
    table = torch.cat([z[:, -4].view(-1, 1), cG.view(-1, 1), z[:, -3].view(-1, 1), cHJf, cHJg, z[:, -2].view(-1, 1), z[:, -1].view(-1, 1)], 1)
    return dict(table=table, z=z, zFull=zFull, ctrlFull=ctrlFull)


def case_restate(case, x, W, hold, dtype, mutation=None):
    """restate() for a MonoCase -> its dict plus stages [n, states, d]: every sampled, stage and displaced state"""
    P = orc.PhiParams.from_state_dict({k: v.clone() for k, v in um.case_sd(case).items()}, dtype=dtype)
    S = um.spec(case).to(dtype)
    states = [x.to(dtype).clone()]
    with torch.no_grad():
        out = restate(P, S, x.to(dtype), W, hold, list(case.tspan), case.nt, case.stepper, case.alph, mutation, states)
    out["stages"] = torch.stack(states, 1)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# cases: (kernel family, MonoCase)
# ---------------------------------------------------------------------------------------------------------------------------------
def _C(kind, d, m, r, obstacle, mode, n, stepper, nt, tspan=T1, **kw):
    return um.MonoCase(kind, d, m, r, obstacle, mode, n, stepper, nt, tspan, seed=d + 3 * m + r, **kw)


# (i) the lane and one-CU entries of util_disturb.CASES (its variants rk1 and tspan = (0.25, 1) among them)
GROUP_I = [fc for fc in ud.CASES if fc[0] in ("lane", "mono")]
# (ii) one small case at each of the 6 lane (MP, DP) and the 7 one-CU (KBM, KBD) instantiations: a ragged tail (n no multiple of 4 / of 16),
# nt = 3 -- with K = 2 the smallest rollout with a ragged last interval.  KBD = 2 from point agents: quadcopters there have two craft
GROUP_II = [
    ("lane", _C("cross2d", 4, 9, 3, "hardcorridor", "eval", 5, "rk4", 3)),                         # (16, 8)
    ("lane", _C("cross2d", 8, 16, 5, "softcorridor", "eval", 6, "rk4", 3)),                        # (16, 16)
    ("lane", _C("cross2d", 16, 7, 4, None, "eval", 7, "rk4", 3)),                                  # (16, 32)
    ("lane", _C("cross2d", 6, 31, 7, "softcorridor", "eval", 5, "rk4", 3)),                        # (32, 8)
    ("lane", _C("swarm", 15, 17, 6, "blocks", "eval", 6, "rk4", 3)),                               # (32, 16)
    ("lane", _C("cross2d", 30, 32, 10, None, "eval", 7, "rk4", 3)),                                # (32, 32), 15 agents
    ("mono", _C("quad", 12, 17, 5, None, "eval", 17, "rk4", 3)),                                   # (2, 1)
    # (seven agents 1.0 apart sit near W's edge 2 r = 1.2: draw 0 of the starts loses 4 of 20 candidates to the screen, draw 1 at most 1)
    ("mono", _C("cross2d", 14, 48, 10, "softcorridor", "eval", 18, "rk4", 3, draw=1)),             # (4, 1)
    ("mono", _C("swarm", 15, 80, 6, "blocks", "eval", 19, "rk4", 3)),                              # (6, 1)
    ("mono", _C("quad", 12, 100, 13, None, "eval", 21, "rk4", 3, angles="quadrants")),             # (8, 1)
    ("mono", _C("cross2d", 16, 33, 5, None, "eval", 17, "rk4", 3)),                                # (4, 2)
    ("mono", _C("swarm", 30, 81, 10, "blocks", "eval", 18, "rk4", 3)),                             # (6, 2)
    ("mono", _C("cross2d", 24, 128, 16, "softcorridor", "eval", 19, "rk4", 3)),                    # (8, 2)
]
# (iii) train mode (W's threshold 2.2 r) on both families, and the quadcopter under rk1
GROUP_III = [
    ("lane", _C("cross2d", 4, 16, 5, "softcorridor", "train", 5, "rk4", 3)),
    ("mono", _C("cross2d", 14, 64, 10, "softcorridor", "train", 17, "rk4", 3, T2)),
    ("mono", _C("quad", 12, 128, 10, None, "train", 17, "rk1", 3)),
]
CASES = GROUP_I + GROUP_II + GROUP_III
KERNEL = {("lane", False): "rollout_lane_kernel<hold>", ("lane", True): "rollout_lane_kernel<hold,dist>",
          ("mono", False): "rollout_mono_kernel<hold>", ("mono", True): "rollout_mono_kernel<hold,dist>"}


def case_id(fc):
    return f"{fc[0]}-{fc[1].id}"


def holds(case):
    """K = 1, 2 (nt = 3: a ragged last interval), nt and nt + 3 (the open-loop limit, twice)"""
    return (1, 2, case.nt, case.nt + 3)


COMBOS = [(k, dist) for k in range(4) for dist in (False, True)]          # (index into holds(case), W given)

_CACHE = {}


def candidates_total(case):
    return case.n + max(2, case.n // 8)


def case_data(case, hold, disturbed):
    """-> dict x [n, d], W [nt, n, d] or None, r64 / r32 (case_restate), screened (candidates the screen dropped), total (candidates).
    Candidates: n + max(2, n // 8) starts with their own disturbances; the screen (util_mono.near_edge over every sampled, stage and
    displaced state of the fp64 run) may drop at most one in eight of them: asserted here.  Cached per (case, hold, disturbed)."""
    key = (case, hold, disturbed)
    if key in _CACHE:
        return _CACHE[key]
    total = candidates_total(case)
    cand = um.candidates(case, total)
    Wc = ud.disturbances(case, total) if disturbed else None
    r64 = case_restate(case, cand.double(), Wc, hold, torch.float64)
    assert all(bool(torch.isfinite(v).all()) for v in r64.values()), f"{case.id}: the fp64 restatement is not finite"
    bad = um.near_edge(case, r64["stages"])
    keep = (~bad).nonzero().flatten()[:case.n]
    assert 8 * int(bad.sum()) <= total and keep.numel() == case.n, f"{case.id} K={hold}: the screen drops {int(bad.sum())} of {total} rows"
    x = cand[keep].contiguous()
    W = Wc[:, keep].contiguous() if disturbed else None
    r64 = {k: v[keep] for k, v in r64.items()}                      # (rows are independent)
    r32 = case_restate(case, x, W, hold, torch.float32)
    _CACHE[key] = out = dict(x=x, W=W, r64=r64, r32=r32, screened=int(bad.sum()), total=total)
    return out


def compare(got, r64, r32):
    """util_lane.compare_forward (util_oracle's rule, factor 4 over the fp32 restatement's own error, floor 1e-6) over table, z, zFull,
    ctrlFull -> {name: (ok, err, tol, e32)}"""
    return ul.compare_forward({k: got[k] for k in ("table", "z", "zFull", "ctrlFull") if k in got}, r64, r32)
