"""oracle-side helpers of the disturbed rollout's tests (CPU only: nothing here touches a GPU)

The reference has no rollout under per-step disturbances, so the yardstick is the pinned oracle composed in a loop: restate() is
nocf_rollout_disturbed_f32's contract (include/nocf.h) written with oracle.ocflow_oracle's steppers, grad Phi, controls and the terminal
block of oracle.rollout, in fp32 and fp64.  Cases are util_mono.MonoCase (its make_net / make_problem / candidates serve point agents and
quadcopters of any width and depth); tests/test_disturb_gpu.py runs them on the GPU, tests/test_disturb_cpu.py checks the restatement, the
screen and that the comparator has teeth on wrong restatements."""
import torch
import torch.nn.functional as F

import util_lane as ul
import util_mono as um
import util_oracle as uo
from oracle import ocflow_oracle as orc

STATE_ATOL, STATE_RTOL = 1e-4, 1e-5          # the stated state tolerance of chained rollouts (tests/test_hip_parity.py: shock sweep)
SIGMA_REL = 0.05                             # disturbance scale: sigma = 0.05 r of the problem
T1, T2 = (0.0, 1.0), (0.25, 1.0)

MUTATIONS = ("w_before_step", "w_on_costs", "ctrl_undisplaced")


def restate(P, S, x, W, tspan, nt, stepper, alph, mutation=None, states=None):
    """The disturbed rollout in the dtype of x: z = step(z); z[:, :d] += W[k]; zFull[k+1] = z; ctrlFull[k+1] = calcCtrls at the displaced
    state and the step's start time; terminal terms at the displaced z(T).  W [nt, n, d].  mutation: one of MUTATIONS, a deliberately wrong
    restatement.  states: a list that receives every displaced state [n, d].
    -> dict table [n, 7], z [n, d+4], zFull [n, d+4, nt+1], ctrlFull [n, a, nt+1]"""
    n, d = x.shape
    W = W.to(x.dtype)
    h = (tspan[1] - tspan[0]) / nt
    z = torch.cat((x, torch.zeros(n, 4, dtype=x.dtype)), 1)
    tk = tspan[0]
    p_init = orc.phi_grad(P, F.pad(x, [0, 1, 0, 0], value=0))[:, 0:d]
    zFull = torch.zeros(n, d + 4, nt + 1, dtype=x.dtype)
    zFull[:, :, 0] = z
    c0 = orc.prob_ctrls(S, z[:, 0:d], p_init)
    ctrlFull = torch.zeros(*c0.shape, nt + 1, dtype=x.dtype)
    for k in range(nt):
        if mutation == "w_before_step":
            z = z.clone()
            z[:, :d] += W[k]
        if stepper == "rk4":
            z = orc.step_rk4(P, S, z, tk, tk + h)
        else:
            z = orc.step_rk1(P, S, z, tk, tk + h)
        undisplaced = z[:, :d].clone()
        z = z.clone()
        if mutation != "w_before_step":
            z[:, :d] += W[k]
        if mutation == "w_on_costs":
            z[:, d:] += W[k][:, :4]
        if states is not None:
            states.append(z[:, :d].clone())
        tk += h
        zFull[:, :, k + 1] = z
        xc = undisplaced if mutation == "ctrl_undisplaced" else z[:, 0:d]
        s = F.pad(xc, [0, 1, 0, 0], value=tk - h)
        ctrlFull[:, :, k + 1] = orc.prob_ctrls(S, xc, orc.phi_grad(P, s)[:, 0:d])
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


def case_restate(case, x, W, dtype, mutation=None):
    """restate() for a MonoCase -> its dict plus stages [n, evaluations + displaced states, d]: every stage state and every displaced state"""
    P = orc.PhiParams.from_state_dict({k: v.clone() for k, v in um.case_sd(case).items()}, dtype=dtype)
    S = um.spec(case).to(dtype)
    stages, steps, disp = [], [], []
    with torch.no_grad(), ul.recording(stages, steps):
        out = restate(P, S, x.to(dtype), W, list(case.tspan), case.nt, case.stepper, case.alph, mutation, disp)
    out["stages"] = torch.stack(stages + disp, 1)
    return out


# the smallest shapes that reach every new instantiation (kernel family, case); the GPU file proves the family by nocf_last_rollout_kernel
def _C(kind, d, m, r, obstacle, mode, n, stepper, nt, tspan=T1, **kw):
    return um.MonoCase(kind, d, m, r, obstacle, mode, n, stepper, nt, tspan, seed=d + 3 * m + r, **kw)


CASES = [
    ("lane", _C("cross2d", 4, 16, 5, None, "eval", 5, "rk4", 3)),                                  # (MP, DP) = (16, 8)
    ("lane", _C("cross2d", 4, 32, 5, "softcorridor", "eval", 7, "rk4", 3)),                        # (32, 8), obstacle and W on
    ("lane", _C("cross2d", 24, 32, 10, None, "eval", 6, "rk4", 2)),                                # (32, 32), 12 agents
    ("mono", _C("quad", 12, 128, 10, None, "eval", 17, "rk4", 3)),                                 # singlequad: one full, one ragged tile
    ("mono", _C("cross2d", 14, 64, 10, "softcorridor", "eval", 33, "rk4", 2)),
    ("tile", _C("cross2d", 4, 129, 5, "softcorridor", "eval", 17, "rk4", 2)),
    ("tile", _C("cross2d", 6, 48, 5, None, "eval", 20, "rk4", 2, nTh=3)),
    # swarm50's shape; 50 agents 0.7 apart meet many W edges: the draw of the starts (chosen on the CPU) whose fp64 run drops no row
    ("tile-fixed", _C("swarm", 150, 512, 10, "blocks", "eval", 16, "rk4", 2, draw=5)),
    # variants: rk1, tspan = [0.25, 1], train mode
    ("lane", _C("cross2d", 4, 16, 5, "softcorridor", "eval", 5, "rk1", 3)),
    ("mono", _C("quad", 12, 128, 10, None, "eval", 17, "rk4", 3, T2)),
    ("tile", _C("cross2d", 4, 129, 5, "hardcorridor", "train", 17, "rk4", 2)),
]
KERNEL = {"lane": "rollout_lane_kernel<dist>", "mono": "rollout_mono_kernel<dist>", "tile": "rollout_kernel<generic, dist>",
          "tile-fixed": "rollout_kernel<shape-specialised, dist>"}


def case_id(fc):
    return f"{fc[0]}-{fc[1].id}"


def disturbances(case, rows, seed_offset=0):
    """W [nt, rows, d] on the CPU: neuraloc_amd.brownian_disturbances with sigma = SIGMA_REL r, seeded by the case"""
    import neuraloc_amd as na
    g = torch.Generator().manual_seed(7919 * case.seed + 31 * case.nt + seed_offset)
    return na.brownian_disturbances(case.nt, rows, case.d, SIGMA_REL * case.rad, case.tspan, generator=g)


_CACHE = {}


def case_data(case):
    """-> dict x [n, d], W [nt, n, d], r64 / r32 (case_restate), screened (rows of the candidates the screen dropped), total (candidates).
    Candidates: n + n // 8 starts with their own disturbances; the screen (util_mono.near_edge over every stage state and every displaced
    state of the fp64 run) may drop at most one in eight of them.  Cached per case."""
    if case in _CACHE:
        return _CACHE[case]
    total = case.n + case.n // 8
    cand = um.candidates(case, total)
    Wc = disturbances(case, total)
    r64 = case_restate(case, cand.double(), Wc, torch.float64)
    bad = um.near_edge(case, r64["stages"])
    keep = (~bad).nonzero().flatten()[:case.n]
    assert 8 * int(bad.sum()) <= total and keep.numel() == case.n, f"{case.id}: the screen drops {int(bad.sum())} of {total} rows"
    x, W = cand[keep].contiguous(), Wc[:, keep].contiguous()
    r64 = {k: v[keep] for k, v in r64.items()}                      # (rows are independent)
    r32 = case_restate(case, x, W, torch.float32)
    _CACHE[case] = out = dict(x=x, W=W, r64=r64, r32=r32, screened=int(bad.sum()), total=total)
    return out


def compare(got, r64, r32):
    """util_lane.compare_forward (util_oracle's rule, factor 4 and floor 1e-6) over table, z, zFull, ctrlFull -> {name: (ok, err, tol, e32)}"""
    return ul.compare_forward({k: got[k] for k in ("table", "z", "zFull", "ctrlFull") if k in got}, r64, r32)


def chained(P, S, x, W, k, tspan, nt, stepper, alph):
    """one nonzero W[k] as two chained oracle.rollout calls (the shock construction on a uniform grid) -> zFull [n, d+4, nt+1] with the
    second segment's cost columns continued from the first's"""
    n, d = x.shape
    h = (tspan[1] - tspan[0]) / nt
    ts = tspan[0] + (k + 1) * h
    z1, _ = orc.rollout(x, P, S, [tspan[0], ts], k + 1, stepper, alph, intermediates=True)
    out = torch.zeros(n, d + 4, nt + 1, dtype=x.dtype)
    out[:, :, :k + 2] = z1
    out[:, :d, k + 1] += W[k].to(x.dtype)
    if k + 1 < nt:
        z2, _ = orc.rollout(out[:, :d, k + 1].clone(), P, S, [ts, tspan[1]], nt - k - 1, stepper, alph, intermediates=True)
        out[:, :, k + 2:] = z2[:, :, 1:]
        out[:, d:, k + 2:] += out[:, d:, k + 1:k + 2]
    return out


def state_close(a, b):
    return bool(((a.double() - b.double()).abs() <= STATE_ATOL + STATE_RTOL * b.double().abs()).all())
