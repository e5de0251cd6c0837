"""helpers of the double-precision sweep (CPU only: nothing here touches a GPU)

The fp64 kernels (csrc/nocf_f64.inc rollout_f64_kernel<T, WIDE>, phi_f64_kernel<T, WIDE>, prob_f64_kernel<4>; csrc/nocf_f64_bwd.inc
rollout_bwd_f64_kernel<T, true>, rollout_bwd_f64_narrow_kernel<T>) are the project's accuracy path, so a double-against-double comparison at
1e-9 cannot judge them.  This module holds

* a Python mirror of the three samples-per-workgroup choices and of the form f64_rows takes per product (f64_plan;
  tests/test_f64_sweep_cpu.py holds it against nocf_debug_f64_plan field by field);
* THE TRUTH: one numpy restatement of the rollout (written from oracle/ocflow_oracle.py, not from the kernels), generic in the dtype: in
  numpy.longdouble (x87 80-bit, eps 1.08e-19) for values, in numpy.clongdouble with a complex step of 1e-40 for directional derivatives --
  Im J(theta + i h v) / h is exact to the precision of the arithmetic, so values and gradients have one source and no autograd.  It is
  written analytically: |x| = x sign(Re x), masks and comparisons read real parts, constants are built in longdouble;
* the rule: util_oracle.tolerance with the precisions shifted -- a quantity passes if its max error against the truth is at most TOL_FACTOR
  x the error of the torch-fp64 oracle on the same quantity against the same truth, floor TOL_FLOOR * 2**-29 (1e-6 scaled by eps64 / eps32)
  of the quantity's scale (max |truth|; sum |g_i v_i| for a directional derivative);
* the rows the truth is computed on, the screen (util_oracle.near_edge on the truth's trajectory), the case lists, and the wrong
  restatements the rule must reject (the same numpy restatement in float64 with one defect switched on)."""
import contextlib
import dataclasses
import functools

import numpy as np
import torch

import util_oracle as uo
from oracle import ocflow_oracle as orc
from util_oracle import TOL_FACTOR, TOL_FLOOR

LD, CLD, F64 = np.longdouble, np.clongdouble, np.float64
TF64 = torch.float64
H_STEP = LD("1e-40")
FLOOR = TOL_FLOOR * 2.0 ** -29
ALPH = (100.0, 1.0e3, 50.0, 0.5, 0.25, 0.125)
E_SHAPE, E_LDS = -2, -6
LDS_BYTES = 160 * 1024


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------------------
# the plan, mirrored (csrc/nocf_kernels.hip f64_rollout_plan / f64_bwd_plan / f64_phi_plan, f64_rows_form; make_f64_plan, make_f64_bwd_plan)
# ---------------------------------------------------------------------------------------------------------------------------------
FIELDS = ("T", "wide", "lds", "f_open", "f_layer", "f_close", "rg_m", "pass_m", "rg_d1", "pass_d1", "trips_m", "trips_d1")   # out[12]
PLAIN, GEMM2, GEMM1, PIPE = 0, 1, 2, 3
ROLLOUT, ADJOINT, PHI = 0, 1, 2


def _carve(sizes):
    return sum((s + 1) & ~1 for s in sizes)


def fwd_lds(d, m, nTh, n_agents, T):
    D1, ZW, na = d + 1, d + 4, max(n_agents, 1)
    return _carve([T * D1, T * m, nTh * T * m, T * m, T * m, T * D1, T * 16, T * ZW, T * ZW, 3 * 256, T, T * na * 8, T * ZW])


def bwd_lds(d, m, nTh, n_agents, T):
    D1, ZW, na, L = d + 1, d + 4, max(n_agents, 1), nTh - 1
    return _carve([T * D1, T * D1, T * 16, 3 * 256, T, T * na * 8, T * ZW, (L + 1) * T * m, (L + 1) * T * m, L * T * m, (L + 1) * T * m,
                   T * m, T * m, T * m, T * m, T * D1, T * D1, T * 16, T * ZW, T * ZW, T * ZW, T * ZW, T * 4])


def img_rg(M):
    ng = cdiv(M, 16)
    return 8 if ng > 16 else 4 if ng > 8 else 2


def img_passes(M):
    return cdiv(cdiv(M, 16), 4 * img_rg(M))


def rows_form(T, wide, M, K):
    if wide and T == 4:
        return PIPE
    if wide and M > 256:
        return GEMM2
    if wide and K > 256:
        return GEMM1
    return PLAIN


def f64_plan(d, m, nTh, r, n_agents, n, which, bwd_t=0):
    """nocf_debug_f64_plan(d, m, nTh, r, n_agents, n, which) under NOCF_F64_BWD_T = bwd_t -> dict rc + FIELDS (all 0 on a refusal)"""
    out = dict.fromkeys(FIELDS, 0)
    out["rc"] = E_SHAPE
    if which not in (0, 1, 2) or n < 1 or d < 1 or m < 1 or nTh < 2 or r < 1 or r > 16:
        return out
    wide = m > 256
    T = lds = 0
    if which == ADJOINT:
        for cand in (4, 2, 1):
            if (wide and cand == 4) or (bwd_t and cand > bwd_t):
                continue
            lds = bwd_lds(d, m, nTh, n_agents, cand)
            if lds * 8 <= LDS_BYTES:
                T = cand
                break
    else:
        na = n_agents if which == ROLLOUT else 1
        first = 4 if n >= 1024 else 2 if n >= 512 else 1
        for q, cand in enumerate((first, 2, 1)):
            if q and cand >= first:
                continue
            lds = fwd_lds(d, m, nTh, na, cand)
            if lds * 8 <= LDS_BYTES:
                T = cand
                break
    if not T:
        out["rc"] = E_LDS
        return out
    D1 = d + 1
    f0, f1, f2 = rows_form(T, wide, m, D1), rows_form(T, wide, m, m), rows_form(T, wide, D1, m)
    pipe = f1 == PIPE
    out.update(rc=0, T=T, wide=int(wide), lds=lds, f_open=f0, f_layer=f1, f_close=f2, rg_m=img_rg(m) if pipe else 0,
               pass_m=img_passes(m) if pipe else 0, rg_d1=img_rg(D1) if pipe else 0, pass_d1=img_passes(D1) if pipe else 0,
               trips_m=cdiv(m, 512) if f1 == GEMM2 else 0, trips_d1=cdiv(D1, 512) if f2 == GEMM2 else 0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# cases: problems, weights, starts
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    prob: str
    n: int
    nTh: int = 2
    m: int = 24
    stepper: str = "rk4"
    nt: int = 2
    training: bool = False
    tspan: tuple = (0.0, 1.0)
    bwd_t: int = 0                    # NOCF_F64_BWD_T the adjoint runs under (0: unset)
    var0: float = 0.5

    @property
    def id(self):
        return (f"{self.prob}-n{self.n}-L{self.nTh}-m{self.m}-{self.stepper}-nt{self.nt}-{'train' if self.training else 'eval'}"
                + (f"-T{self.bwd_t}" if self.bwd_t else "") + ("" if self.tspan == (0.0, 1.0) else "-seg"))

    @property
    def d(self):
        return dim_of(self.prob)

    @property
    def r(self):
        return min(10, self.d + 1)

    @property
    def n_agents(self):
        return self.d // {"singlequad": 12, "swarm": 3, "swarm50": 3}.get(self.prob, 2)

    def plan(self, which, n=None):
        return f64_plan(self.d, self.m, self.nTh, self.r, self.n_agents, self.n if n is None else n, which, self.bwd_t)


@functools.lru_cache(None)
def _init(name):
    import neuraloc_amd as na
    with torch.random.fork_rng():                              # (initProb's draws are not used)
        prob, _, _, xInit = na.initProb(name, 2, 2, 0.5, list(ALPH), lambda t: t.to(TF64))
    return prob, xInit.reshape(-1)


def dim_of(name):
    return _init(name)[1].numel()


def make_prob(case, device="cpu"):
    """a fresh package problem object in double, in the case's mode"""
    import neuraloc_amd as na
    with torch.random.fork_rng():
        prob, _, _, _ = na.initProb(case.prob, 2, 2, 0.5, list(ALPH), lambda t: t.to(TF64).to(device))
    prob.train() if case.training else prob.eval()
    return prob


def spec_of(case):
    prob = make_prob(case)
    S = orc.ProbSpec.from_object(prob)
    S.xtarget = S.xtarget.cpu().to(TF64)
    return S


@functools.lru_cache(None)
def _state_dict(nTh, m, d):
    """closed-form double weights (no RNG, not representable in fp32): entries s sin(a i + b j + phase), s ~ 1 / sqrt(fan_in)"""
    def fill(rows, cols, a, b, ph, s):
        i = torch.arange(rows, dtype=TF64).unsqueeze(1)
        j = torch.arange(cols, dtype=TF64).unsqueeze(0)
        return s * torch.sin(a * i + b * j + ph)
    r, seed = min(10, d + 1), 0.01 * (nTh + m + d)
    sd = {"A": fill(r, d + 1, 0.37, 0.11, 0.1 + seed, 1.0 / (d + 1) ** 0.5),
          "c.weight": fill(1, d + 1, 0.0, 0.23, 0.4 + seed, 0.3), "c.bias": torch.tensor([0.05], dtype=TF64),
          "w.weight": 1.0 + fill(1, m, 0.0, 0.31, 0.7 + seed, 0.2),
          "N.layers.0.weight": fill(m, d + 1, 0.41, 0.13, 0.2 + seed, 1.0 / (d + 1) ** 0.5),
          "N.layers.0.bias": fill(1, m, 0.0, 0.19, 0.3 + seed, 0.1).reshape(m)}
    for l in range(1, nTh):
        sd[f"N.layers.{l}.weight"] = fill(m, m, 0.29 + 0.01 * l, 0.17, 0.5 + seed + l, 1.0 / m ** 0.5)
        sd[f"N.layers.{l}.bias"] = fill(1, m, 0.0, 0.27, 0.6 + seed + l, 0.1).reshape(m)
    return sd


def state_dict(case):
    return {k: v.clone() for k, v in _state_dict(case.nTh, case.m, case.d).items()}


def make_net(case, device, train=False):
    import neuraloc_amd as na
    net = na.Phi(nTh=case.nTh, m=case.m, d=case.d, alph=list(ALPH)).to(TF64)
    net.load_state_dict(state_dict(case))
    net = net.to(device)
    return net.train() if train else net.eval()


# swap2's straight paths pass between the hard corridor's two discs and never meet them: its middle starts are moved (agent 1 down by 3.2
# into the lower disc, agent 2 by 1.2 to pass close to agent 1) so that Q is nonzero in both modes
MID_SHIFT = {"swap2": (0.0, -3.2, 0.0, -1.2)}
# seeds whose starts keep the screen's cap in both modes (tests/test_f64_sweep_cpu.py asserts the cap); 0 where not listed
START_SEED = {('swap12_1pair', 513): 1, ('swap12_3pair', 513): 1}


@functools.lru_cache(None)
def _starts(name, n, var0):
    """n starts in double: two of three around xInit, every third around the middle of the path (where the agents meet each other and the
    obstacles), var0 randn around either (a CPU generator)"""
    prob, xInit = _init(name)
    xt = prob.xtarget.reshape(-1).to(TF64)
    g = torch.Generator().manual_seed(4242 + n + 100000 * START_SEED.get((name, n), 0))
    x = xInit + var0 * torch.randn(n, xInit.numel(), generator=g, dtype=TF64)
    mid = torch.arange(n) % 3 == 1
    x[mid] += 0.5 * (xt - xInit)
    if name in MID_SHIFT:                                           # (tests/util_oracle.py START_SHIFT: the same move, for the same reason)
        x[mid] += torch.tensor(MID_SHIFT[name], dtype=TF64)
    return x.contiguous()


def starts(case):
    return _starts(case.prob, case.n, case.var0).clone()


# ---------------------------------------------------------------------------------------------------------------------------------
# the rollout restated in numpy, generic in the dtype
# ---------------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ("two_pi_f32", "hN_f32", "stage_time_f32", "log1p_f32", "drop_last_k", "lost_second_pass", "row_alias_256", "reduce_64", "cov_1e-11")


class Restate:
    """src/OCflow.py, src/Phi.py, src/problem/*.py as oracle/ocflow_oracle.py restates them, in numpy.
    dtype: longdouble / clongdouble (the truth) or float64 (a stand-in for a kernel: then `mut`, one of MUTATIONS, switches a defect on, and
    kernel_forms forms sigma and tanh as f64_act_pair does, from one expm1).  T: samples per workgroup (the reduce_64 defect's group size)."""

    def __init__(self, sd, S, dtype, mut=None, kernel_forms=False, T=1):
        self.dt, self.mut, self.kf, self.T = dtype, mut, kernel_forms, T
        self.seq = kernel_forms                                   # the plain loop's grouping: one k after the other, starting from the bias
        self.rdt = LD if dtype in (LD, CLD) else F64
        c = self.c = lambda v: np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v).astype(dtype)
        self.nTh = sum(1 for k in sd if k.startswith("N.layers.") and k.endswith(".weight"))
        self.K = [c(sd[f"N.layers.{i}.weight"]) for i in range(self.nTh)]
        self.b = [c(sd[f"N.layers.{i}.bias"]) for i in range(self.nTh)]
        self.w, self.A, self.cw, self.cb = c(sd["w.weight"]).reshape(-1), c(sd["A"]), c(sd["c.weight"]).reshape(-1), c(sd["c.bias"]).reshape(())
        self.S = S
        self.xt = np.asarray(S.xtarget.numpy()).astype(self.rdt)
        R = self.rdt
        self.hN = R(1) / R(self.nTh - 1)
        if mut == "hN_f32":
            self.hN = R(np.float32(self.hN))
        self.two_pi = R(8) * np.arctan(R(1))
        if mut == "two_pi_f32":
            self.two_pi = R(np.float32(self.two_pi))

    # ---- helpers
    def abs(self, x):
        return x * np.sign(x.real)

    def mm(self, X, Wm, init=None):
        """init + X [n, K] times Wm [M, K] transposed -> [n, M] (a product of f64_rows: M rows, contraction K, the sums started at init)"""
        M, K = Wm.shape
        Kd = K - 1 if (self.mut == "drop_last_k" and K % 4 != 0) else K
        if self.seq:
            out = np.zeros((X.shape[0], M), self.dt) + (0 if init is None else init)
            if self.dt is F64:                                   # v_fma_f64: the product enters the sum unrounded (here: to 64 bits)
                Xl, Wl = X.astype(LD), Wm.astype(LD)
                for k in range(Kd):
                    out = (out.astype(LD) + Xl[:, k:k + 1] * Wl[:, k]).astype(F64)
            else:
                for k in range(Kd):
                    out = out + X[:, k:k + 1] * Wm[:, k]
        else:
            out = X[:, :Kd] @ Wm[:, :Kd].T
            if init is not None:
                out = out + init
        if self.mut == "lost_second_pass" and M > 512:
            out[:, 512:] = 0
        if self.mut == "row_alias_256" and M > 256:
            k = min(256, M - 256)
            out[:, 256:256 + k] = out[:, :k]
        return out

    def act(self, x):
        """sigma(x) (src/Phi.py:8-9) and tanh(x)"""
        ax = self.abs(x)
        if self.kf:
            em1 = np.expm1(-2 * ax)
            return ax + np.log1p(1 + em1), np.sign(x.real) * (-em1 / (2 + em1))
        e = np.exp(-2 * ax)
        lg = np.log1p(e.astype(np.float32)).astype(self.dt) if self.mut == "log1p_f32" else np.log(1 + e)
        return ax + lg, np.tanh(x)

    # ---- Phi (src/Phi.py:91-138)
    def phi(self, s, value=False):
        hN = self.hN
        sg, th0 = self.act(self.mm(s, self.K[0], self.b[0]))
        u, ths = sg, [th0]
        for i in range(1, self.nTh):
            sg, th = self.act(self.mm(u, self.K[i], self.b[i]))
            u = u + hN * sg
            ths.append(th)
        back = np.broadcast_to(self.w, u.shape)
        for i in range(self.nTh - 1, 0, -1):
            back = back + hN * self.mm(ths[i] * back, self.K[i].T)
        zA = s @ self.A.T
        g = self.mm(th0 * back, self.K[0].T) + zA @ self.A + self.cw
        if not value:
            return g
        return g, u @ self.w + 0.5 * np.sum(zA * zA, 1) + s @ self.cw + self.cb

    # ---- the problems (src/problem/*.py, src/utils.py:70-86)
    def gauss(self, xa, mu, cov):
        R = self.rdt
        cov = [R(c) for c in cov]
        if self.mut == "cov_1e-11":
            cov = [c * (1 + R(1e-11)) for c in cov]
        k = len(mu)
        denom = self.two_pi ** (R(k) / 2) * np.sqrt(np.prod(np.asarray(cov, dtype=R)))
        q = sum((xa[..., j] - R(mu[j])) ** 2 / cov[j] for j in range(k))
        return np.exp(-q / 2) / denom

    def Q(self, x):
        """sum over agents of the obstacle value [n]"""
        S, R = self.S, self.rdt
        n = x.shape[0]
        if S.obstacle is None or S.kind == orc.KIND_QUAD:
            return np.zeros(n, self.dt)
        xa = x.reshape(n, S.n_agents, S.agent_dim)
        r = R(S.r)
        if S.obstacle == "softcorridor":
            q = sum(self.gauss(xa, mu, (0.2, 0.2)) for mu in ((-2.5, 0.), (2.5, 0.), (-1.5, 0.), (1.5, 0.)))
        elif S.obstacle == "hardcorridor":
            nrm = [np.sqrt((xa[..., 0].real - mu[0]) ** 2 + (xa[..., 1].real - mu[1]) ** 2) for mu in ((0., 4.), (0., -3.5))]
            thr = R(2) + r if S.training else R(2)
            inside = (nrm[0] < thr) | (nrm[1] < thr)
            q = (self.gauss(xa, (0., 4.), (1., 1.)) + self.gauss(xa, (0., -3.5), (1., 1.))) if S.training else np.ones(inside.shape, self.dt)
            q = np.where(inside, q, 0)
        elif S.obstacle == "blocks":
            px, py, pz = xa[..., 0].real, xa[..., 1].real, xa[..., 2].real
            e = r if S.training else R(0)
            inside = ((px < 2 + e) & (px > -2 - e) & (py < R(0.5) + e) & (py > -R(0.5) - e) & (pz < 7 + e)) \
                | ((px < 4 + e) & (px > 2 - e) & (py < 1 + e) & (py > -1 - e) & (pz < 4 + e))
            q = (self.gauss(xa, (0., 0., 2.), (9., 3., 9.)) + self.gauss(xa, (2.5, 0., 2.), (9., 3., 3.)) + 999) if S.training \
                else np.ones(inside.shape, self.dt)
            q = np.where(inside, q, 0)
        else:
            raise ValueError(S.obstacle)
        return q.sum(1)

    def W(self, x):
        """pairwise interaction cost [n] (Cross2D.py:127-162, SwarmTraj.py:131-164, Quadcopter.py:133-158)"""
        S, R = self.S, self.rdt
        n, N = x.shape[0], S.n_agents
        if N < 2:
            return np.zeros(n, self.dt)
        quad = S.kind == orc.KIND_QUAD
        k = 3 if quad else S.agent_dim
        xa = x.reshape(n, N, S.agent_dim)[..., :k]
        fac = R(2) if (quad or not S.training) else (R(3.2) if (S.kind == orc.KIND_SWARM and N > 2) else R(2.2))
        thr, r = fac * R(S.r), R(S.r)
        iu = np.triu_indices(N, 1)
        e = xa[:, iu[0]] - xa[:, iu[1]]
        d2 = np.sum(e * e, -1)
        near = np.sqrt(d2.real) < thr
        return np.where(near, np.exp(-d2 / (2 * r * r)), 0).sum(1)

    def sum_p2(self, p):
        if self.mut == "reduce_64":                                 # threads j0 >= 64 of a (256 / T)-thread group lose their share
            keep = (np.arange(p.shape[1]) % (256 // self.T)) < 64
            return np.sum(p[:, keep] ** 2, 1)
        return np.sum(p * p, 1)

    def quad_u(self, xa, pa):
        sps, sth, sph = np.sin(xa[:, 3]), np.sin(xa[:, 4]), np.sin(xa[:, 5])
        cps, cth, cph = np.cos(xa[:, 3]), np.cos(xa[:, 4]), np.cos(xa[:, 5])
        f7, f8, f9 = sps * sph + cps * sth * cph, -cps * sph + sps * sth * cph, cth * cph
        return -1 / (2 * self.rdt(self.S.mass)) * (f7 * pa[:, 6] + f8 * pa[:, 7] + f9 * pa[:, 8]), f7, f8, f9

    def lhqw(self, x, p):
        S, R = self.S, self.rdt
        aQ, aW = R(S.alph_Q), R(S.alph_W)
        zero = np.zeros(x.shape[0], self.dt)
        if S.kind != orc.KIND_QUAD:
            sp2 = self.sum_p2(p)
            if S.kind == orc.KIND_CROSS2D:
                Q = aQ * self.Q(x)
                L = sp2 / 2 + Q
            else:
                Q = self.Q(x) if S.alph_Q > 0 else zero
                L = sp2 / 2 + aQ * Q
            W = self.W(x) if S.alph_W != 0.0 else zero
            L = L + aW * W
            return L, -L + sp2, Q, W
        mass, grav = R(S.mass), R(S.grav)
        Q, H = zero, zero
        W = self.W(x) if S.alph_W > 0.0 else zero
        L = aQ * Q + aW * W
        for i in range(S.n_agents):
            xa, pa = x[:, 12 * i:12 * i + 12], p[:, 12 * i:12 * i + 12]
            sq = pa[:, 9] ** 2 + pa[:, 10] ** 2 + pa[:, 11] ** 2
            u, f7, f8, f9 = self.quad_u(xa, pa)
            L = L + 2 + u * u + sq / 4
            H = H - L - np.sum(xa[:, 6:9] * pa[:, 0:3], 1) - np.sum(xa[:, 9:12] * pa[:, 3:6], 1) \
                - (u / mass) * (f7 * pa[:, 6] + f8 * pa[:, 7] + f9 * pa[:, 8]) + grav * pa[:, 8] + sq / 2
        return L, H, Q, W

    def gradpH(self, x, p):
        S = self.S
        if S.kind != orc.KIND_QUAD:
            return p
        mass, grav = self.rdt(S.mass), self.rdt(S.grav)
        cols = []
        for i in range(S.n_agents):
            xa, pa = x[:, 12 * i:12 * i + 12], p[:, 12 * i:12 * i + 12]
            u, f7, f8, f9 = self.quad_u(xa, pa)
            cols += [-xa[:, 6:12], np.stack([-(u / mass) * f7, -(u / mass) * f8, -(u / mass) * f9 + grav], 1), pa[:, 9:12] / 2]
        return np.concatenate(cols, 1)

    def ctrls(self, x, p):
        S = self.S
        if S.kind != orc.KIND_QUAD:
            return -p
        cols = []
        for i in range(S.n_agents):
            xa, pa = x[:, 12 * i:12 * i + 12], p[:, 12 * i:12 * i + 12]
            cols += [self.quad_u(xa, pa)[0][:, None], -pa[:, 9:12] / 2]
        return np.concatenate(cols, 1)

    # ---- the rollout (src/OCflow.py)
    def rhs(self, z, t, rec):
        n, d = z.shape[0], z.shape[1] - 4
        s = np.concatenate([z[:, :d], np.full((n, 1), t, self.dt)], 1)
        if rec is not None:
            rec.append(s)
        g = self.phi(s)
        L, H, Q, W = self.lhqw(s[:, :d], g[:, :d])
        return np.concatenate([-self.gradpH(s[:, :d], g[:, :d]), np.stack([L, self.abs(g[:, -1] - H), Q, W], 1)], 1)

    def rollout(self, x, tspan, nt, stepper, alph, intermediates=False):
        """-> dict: table [n, 7], z [n, d+4], s_all [E, n, d+1] (the stage inputs), means [7], Jc; intermediates: zFull, ctrlFull too"""
        R = self.rdt
        x = self.c(x)
        n, d = x.shape
        t0, t1 = R(tspan[0]), R(tspan[1])
        h = (t1 - t0) / nt
        z = np.concatenate([x, np.zeros((n, 4), self.dt)], 1)
        tk, rec = t0, []
        zF, cF = [z], [None]
        f32 = (lambda t: R(np.float32(t))) if self.mut == "stage_time_f32" else (lambda t: t)
        for _ in range(nt):
            hs = (tk + h) - tk
            if stepper == "rk4":
                z0 = z
                k = hs * self.rhs(z0, tk, rec)
                z = z0 + k / 6
                k = hs * self.rhs(z0 + k / 2, f32(tk + hs / 2), rec)
                z = z + k / 3
                k = hs * self.rhs(z0 + k / 2, f32(tk + hs / 2), rec)
                z = z + k / 3
                k = hs * self.rhs(z0 + k, tk + hs, rec)
                z = z + k / 6
            else:
                z = z + hs * self.rhs(z, tk, rec)
            tk = tk + h
            if intermediates:
                zF.append(z)
                s = np.concatenate([z[:, :d], np.full((n, 1), tk - h, self.dt)], 1)
                cF.append(self.ctrls(z[:, :d], self.phi(s)[:, :d]))
        a = [R(v) for v in alph]
        res = z[:, :d] - self.xt
        cG = np.sum(res * res, 1) / 2
        sT = np.concatenate([z[:, :d], np.full((n, 1), t1, self.dt)], 1)
        g1, phi1 = self.phi(sT, value=True)
        table = np.stack([z[:, d], cG, z[:, d + 1], self.abs(phi1 - a[0] * cG), np.sum(self.abs(g1[:, :d] - a[0] * res[:, :d]), 1), z[:, d + 2],
                          z[:, d + 3]], 1)
        means = table.sum(0) / n
        out = dict(table=table, z=z, s_all=np.stack(rec), means=means,
                   Jc=means[0] + a[0] * means[1] + a[3] * means[2] + a[4] * means[3] + a[5] * means[4], final=sT)
        if intermediates:
            cF[0] = np.zeros_like(cF[1])
            out.update(zFull=np.stack(zF, 2), ctrlFull=np.stack(cF, 2))
        return out


def restate(case, dtype, rows=None, mut=None, kernel_forms=False, sd=None, x=None, intermediates=False, T=None):
    x = starts(case) if x is None else x
    if rows is not None:
        x = x[rows]
    T = T or case.plan(ROLLOUT)["T"] or 1
    R = Restate(state_dict(case) if sd is None else sd, spec_of(case), dtype, mut, kernel_forms, T)
    return R.rollout(x, case.tspan, case.nt, case.stepper, ALPH, intermediates)


# ---------------------------------------------------------------------------------------------------------------------------------
# rows, screen, truth and oracle per case
# ---------------------------------------------------------------------------------------------------------------------------------
def truth_rows(case, T=None):
    """the rows the truth is computed on: the first and the last workgroup's (the ragged tail), one workgroup in the middle (every T-slot);
    at most 16 rows for wide cases and 32 otherwise -- a batch within that cap is taken whole"""
    n = case.n
    T = T or case.plan(ROLLOUT)["T"]
    cap = 16 if case.m > 256 else 32
    if n <= cap:
        return list(range(n))
    nwg = cdiv(n, T)
    rows = set(range(T)) | set(range((nwg - 1) * T, n)) | set(range((nwg // 2) * T, (nwg // 2) * T + T))
    assert len(rows) <= cap
    return sorted(rows)


def tail_rows(case, T=None):
    T = T or case.plan(ROLLOUT)["T"]
    return list(range((cdiv(case.n, T) - 1) * T, case.n))


@functools.lru_cache(None)
def truth(case):
    """the longdouble rollout on truth_rows -> dict of restate() + rows, keep (bool per truth row: passes the screen)"""
    rows = truth_rows(case)
    out = restate(case, LD, rows, intermediates=True)
    d = case.d
    traj = np.concatenate([out["s_all"][:, :, :d], out["z"][None, :, :d]], 0).astype(F64)          # [E + 1, rows, d]
    S = spec_of(case)
    keep = ~uo.near_edge(S, torch.from_numpy(traj).permute(1, 0, 2).contiguous()).numpy()
    out.update(rows=rows, keep=keep)
    return out


def screen_ok(case, T=None):
    """at most 10 % of the subset screened, and never the whole ragged tail"""
    t = truth(case)
    tail = set(tail_rows(case, T))
    tail_kept = any(k for r, k in zip(t["rows"], t["keep"]) if r in tail)
    return (~t["keep"]).sum() <= 0.1 * len(t["rows"]) and tail_kept


@contextlib.contextmanager
def _recording(stages):
    """the stage inputs of every oracle evaluation inside a rollout (orc.rhs)"""
    real = orc.rhs

    def rhs(P, S, z, t):
        d = z.shape[1] - 4
        stages.append(torch.nn.functional.pad(z[:, :d], (0, 1, 0, 0), value=t).detach().clone())
        return real(P, S, z, t)
    orc.rhs = rhs
    try:
        yield
    finally:
        orc.rhs = real


@functools.lru_cache(None)
def oracle(case):
    """the torch-fp64 oracle on ALL rows -> table, z, s_all, means, Jc, zFull / ctrlFull (truth rows only), as float64 numpy"""
    x = starts(case)
    P = orc.PhiParams.from_state_dict(state_dict(case), dtype=TF64)
    S = spec_of(case)
    ts = list(case.tspan)
    stages = []
    with torch.no_grad():
        with _recording(stages):
            Jn, cs = orc.rollout(x, P, S, ts, case.nt, case.stepper, list(ALPH), noMean=True)
        table = torch.cat([c.reshape(-1, 1) for c in cs], 1)
        means = [torch.mean(table[:, j]) for j in range(7)]                     # (src/OCflow.py:78-95: the means of the noMean columns)
        Jc = means[0] + ALPH[0] * means[1] + ALPH[3] * means[2] + ALPH[4] * means[3] + ALPH[5] * means[4]
        zF, cF = orc.rollout(x[truth_rows(case)], P, S, ts, case.nt, case.stepper, list(ALPH), intermediates=True)
    return dict(table=table.numpy(), s_all=torch.stack(stages).numpy(), means=torch.stack([c.reshape(()) for c in means]).numpy(),
                Jc=float(Jc), zFull=zF.numpy(), ctrlFull=cF.numpy(), z=zF[:, :, -1].numpy())


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------
def compare(got, want, ref, scale=None):
    """-> (ok, err, tol, oracle error): got / ref (the torch-fp64 oracle) against want (the truth), max norm over the whole array, in longdouble"""
    got, want, ref = (np.asarray(v, dtype=LD) for v in (got, want, ref))
    e_ref = float(np.abs(ref - want).max()) if want.size else 0.0
    scale = float(np.abs(want).max()) if scale is None and want.size else float(scale or 0.0)
    tol = max(TOL_FACTOR * e_ref, FLOOR * scale)
    err = float(np.abs(got - want).max()) if want.size else 0.0
    return bool(err <= tol), err, tol, e_ref


TABLE_COLS = ("L", "G", "HJt", "HJfin", "HJgrad", "Q", "W")


@functools.lru_cache(None)
def second_values(case):
    """the second fp64 restatement of the rollout on the truth rows: the numpy restatement in float64 with the kernels' formulas"""
    return restate(case, F64, truth_rows(case), kernel_forms=True, intermediates=True)


def compare_rollout(case, got, what=("table", "z", "s_all", "zFull", "ctrlFull"), second=True):
    """got: dict of arrays over ALL rows (table [n, 7], s_all [E, n, d+1]) or over the truth rows (z, zFull, ctrlFull)
    -> {name: (ok, err, tol, oracle error)} on the truth rows that pass the screen.  second: the entries of SECOND take the larger of the two
    restatements' errors"""
    t, o = truth(case), oracle(case)
    rows, keep = np.asarray(t["rows"]), t["keep"]
    out = {}

    def put(name, g, w, r):
        out[name] = compare(g, w, r)

    for k in what:
        if k not in got:
            continue
        if k == "table":
            for c, cn in enumerate(TABLE_COLS):
                put(f"table.{cn}", got[k][rows][keep][:, c], t[k][keep][:, c], o[k][rows][keep][:, c])
                if second and takes_second(case, f"table.{cn}"):
                    out[f"table.{cn}"] = _wider(out[f"table.{cn}"], second_values(case)["table"][keep][:, c], t[k][keep][:, c])
        elif k == "s_all":
            put(k, got[k][:, rows][:, keep], t[k][:, keep], o[k][:, rows][:, keep])
        else:
            put(k, got[k][keep], t[k][keep], o[k][keep])
    return out


def failures(res):
    return {k: v for k, v in res.items() if not v[0]}


def rows_off_1e9(tab, want, rtol=1e-9):
    """the existing double-against-double comparison (tests/test_f64_gpu.py _rows_off): rows of tab off want"""
    t, w = np.asarray(tab, dtype=F64), np.asarray(want, dtype=F64)
    tol = rtol * np.abs(w) + rtol * np.abs(w).max(-1, keepdims=True) + 1e-12
    return int((np.abs(t - w) > tol).any(-1).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# gradients: complex-step truth, fp64 autograd oracle, directions
# ---------------------------------------------------------------------------------------------------------------------------------
def param_names(case):
    return list(_state_dict(case.nTh, case.m, case.d))


@contextlib.contextmanager
def no_eval_soft_term():
    """the defect of the adjoint before its fix: in eval mode the soft corridor's value enters the objective, its x-gradient does not"""
    real = orc.prob_Q

    def prob_Q(S, x):
        return real(S, x.detach()) if (S.obstacle == "softcorridor" and not S.training) else real(S, x)
    orc.prob_Q = prob_Q
    try:
        yield
    finally:
        orc.prob_Q = real


def _sign(v):
    return np.sign(v)


def _xgrad_np(R, x, cf):
    """f64_xgrad: cf d(alphQ Q + alphW W)/dx of the point-agent problems, masks constant [n, d]; R: a float64 Restate"""
    S = R.S
    n, N, ad = x.shape[0], S.n_agents, S.agent_dim
    xa = x.reshape(n, N, ad)
    gq, gw = np.zeros_like(xa), np.zeros_like(xa)
    r = S.r
    if S.obstacle == "softcorridor":
        for mu in (-2.5, 2.5, -1.5, 1.5):
            pdf = R.gauss(xa, (mu, 0.0), (0.2, 0.2))
            gq[..., 0] -= pdf * (xa[..., 0] - mu) / 0.2
            gq[..., 1] -= pdf * xa[..., 1] / 0.2
    elif S.obstacle == "hardcorridor" and S.training:
        x0, x1 = xa[..., 0], xa[..., 1]
        n1, n2 = np.sqrt(x0 * x0 + (x1 - 4.0) * (x1 - 4.0)), np.sqrt(x0 * x0 + (x1 + 3.5) * (x1 + 3.5))
        inside = (n1 < 2.0 + r) | (n2 < 2.0 + r)
        p1, p2 = R.gauss(xa, (0.0, 4.0), (1.0, 1.0)), R.gauss(xa, (0.0, -3.5), (1.0, 1.0))
        gq[..., 0] = np.where(inside, -(p1 + p2) * x0, 0.0)
        gq[..., 1] = np.where(inside, -p1 * (x1 - 4.0) - p2 * (x1 + 3.5), 0.0)
    elif S.obstacle == "blocks" and S.training and S.alph_Q > 0.0:
        x0, x1, x2 = xa[..., 0], xa[..., 1], xa[..., 2]
        inside = ((x0 < 2.0 + r) & (x0 > -2.0 - r) & (x1 < 0.5 + r) & (x1 > -0.5 - r) & (x2 < 7.0 + r)) \
            | ((x0 < 4.0 + r) & (x0 > 2.0 - r) & (x1 < 1.0 + r) & (x1 > -1.0 - r) & (x2 < 4.0 + r))
        q1, q2 = R.gauss(xa, (0., 0., 2.), (9., 3., 9.)), R.gauss(xa, (2.5, 0., 2.), (9., 3., 3.))
        e2, f0 = x2 - 2.0, x0 - 2.5
        gq[..., 0] = np.where(inside, -q1 * x0 / 9.0 - q2 * f0 / 9.0, 0.0)
        gq[..., 1] = np.where(inside, -q1 * x1 / 3.0 - q2 * x1 / 3.0, 0.0)
        gq[..., 2] = np.where(inside, -q1 * e2 / 9.0 - q2 * e2 / 3.0, 0.0)
    if S.alph_W != 0.0 and N >= 2:
        fac = (2.2 if N == 2 else (3.2 if S.kind == orc.KIND_SWARM else 2.2)) if S.training else 2.0
        thr, den, inv_r2 = fac * r, 2.0 * r * r, 1.0 / (r * r)
        for a in range(N):
            for b in range(N):
                if a == b:
                    continue
                e = xa[:, a] - xa[:, b]
                dist = np.sqrt(np.sum(e * e, 1))
                w = np.exp(-(dist * dist) / den)
                on = (dist < thr) & ((N == 2) | (w != 1.0))
                gw[:, a] -= np.where(on, w, 0.0)[:, None] * e * inv_r2
    return (cf[:, None, None] * (S.alph_Q * gq + S.alph_W * gw)).reshape(n, -1)


def _quad_adjoint_np(S, x, p, lam, xp, hs, wst, cpl, kL, ekh):
    """f64_quad_adjoint for every craft -> gb [n, d], xd [n, d]"""
    N, M, grav = S.n_agents, S.mass, S.grav
    mh = -1.0 / (2.0 * M)
    gb, xd = np.zeros_like(x), np.zeros_like(x)
    for a in range(N):
        xa, pa = x[:, 12 * a:12 * a + 12], p[:, 12 * a:12 * a + 12]
        cl, ch = kL + ekh * float(N - a), -ekh
        fb = hs * (wst * lam[:, 12 * a:12 * a + 12] + cpl * xp[:, 12 * a:12 * a + 12])
        sps, sth, sph, cps, cth, cph = np.sin(xa[:, 3]), np.sin(xa[:, 4]), np.sin(xa[:, 5]), np.cos(xa[:, 3]), np.cos(xa[:, 4]), np.cos(xa[:, 5])
        f7, f8, f9 = sps * sph + cps * sth * cph, -cps * sph + sps * sth * cph, cth * cph
        u = mh * (f7 * pa[:, 6] + f8 * pa[:, 7] + f9 * pa[:, 8])
        fu = (fb[:, 6] * f7 + fb[:, 7] * f8 + fb[:, 8] * f9) / M
        ku = fu + (2.0 * cl + 4.0 * ch) * u
        g, xq = gb[:, 12 * a:12 * a + 12], xd[:, 12 * a:12 * a + 12]
        g[:, 0:6] = -ch[:, None] * xa[:, 6:12]
        xq[:, 6:12] = fb[:, 0:6] - ch[:, None] * pa[:, 0:6]
        g[:, 6], g[:, 7], g[:, 8] = ku * mh * f7, ku * mh * f8, ku * mh * f9 + ch * grav
        g[:, 9:12] = -0.5 * fb[:, 9:12] + (0.5 * cl + ch)[:, None] * pa[:, 9:12]
        a7, a8, a9 = ku * mh * pa[:, 6] + u * fb[:, 6] / M, ku * mh * pa[:, 7] + u * fb[:, 7] / M, ku * mh * pa[:, 8] + u * fb[:, 8] / M
        xq[:, 3] = -a7 * f8 + a8 * f7
        xq[:, 4] = a7 * cps * cth * cph + a8 * sps * cth * cph - a9 * sth * cph
        xq[:, 5] = a7 * (sps * cph - cps * sth * sph) + a8 * (-cps * cph - sps * sth * sph) - a9 * cth * sph
    return gb, xd


@functools.lru_cache(None)
def second_grads(case):
    """THE SECOND fp64 RESTATEMENT OF THE GRADIENT: the adjoint as csrc/nocf_f64_bwd.inc and neuraloc_amd/train.py form it, in float64 numpy --
    evaluations latest first at the recorded stage inputs, sigma and tanh from one expm1, products summed one k after the other by fused
    multiply-adds (Restate.mm), the
    cotangent of the right-hand side from the RK adjoint recurrences, the VJP of grad Phi by its recurrences, the streamed rows contracted
    over all evaluations at once, dA = A (dM + dM') -> {name: gradient} for every parameter tensor and "x0" """
    S = spec_of(case)
    assert S.kind != orc.KIND_QUAD or S.n_agents == 1 or S.alph_W <= 0.0
    R = Restate(state_dict(case), S, F64, kernel_forms=True)
    x0 = starts(case).numpy()
    fwd = R.rollout(x0, case.tspan, case.nt, case.stepper, ALPH)
    n, d = x0.shape
    D1, Lr, hN = d + 1, R.nTh - 1, R.hN
    nstage = 4 if case.stepper == "rk4" else 1
    a0, a3, a4, a5 = ALPH[0], ALPH[3], ALPH[4], ALPH[5]
    inv = 1.0 / n
    h = (case.tspan[1] - case.tspan[0]) / case.nt
    tk, hs_l = case.tspan[0], []
    for _ in range(case.nt):
        hs_l.append((tk + h) - tk)
        tk += h
    K, A, w, cw = R.K, R.A, R.w, R.cw
    total = case.nt * nstage
    st_rows = {k: [] for k in ("Y", "Gb", "Sx", "Ob", "Wb")}
    lay_rows = [{k: [] for k in ("V", "Ab", "Qb", "U0")} for _ in range(Lr)]
    LAM, XS, XP = np.zeros((n, d)), np.zeros((n, d)), np.zeros((n, d))
    val = None
    for ev in range(total, -1, -1):
        fin = ev == total
        k, st = (case.nt, 0) if fin else divmod(ev, nstage)
        hs = 0.0 if fin else hs_l[k]
        wst, cpl = 1.0, 0.0
        if nstage != 1:
            wst = (1.0 / 6.0) if st in (0, 3) else (2.0 / 6.0)
            cpl = 0.0 if st == 3 else (1.0 if st == 2 else 0.5)
        if fin:
            s = np.concatenate([fwd["z"][:, :d], np.full((n, 1), case.tspan[1])], 1)
        else:
            if st == nstage - 1:
                XS, XP = np.zeros((n, d)), np.zeros((n, d))
            s = fwd["s_all"][ev]
        # grad Phi keeping every layer
        sg, th = R.act(R.mm(s, K[0], R.b[0]))
        U, TH = [sg], [th]
        for l in range(1, Lr + 1):
            sg, th = R.act(R.mm(U[l - 1], K[l], R.b[l]))
            U.append(U[l - 1] + hN * sg)
            TH.append(th)
        ZA = s @ A.T
        AA = [None] * (Lr + 1)
        AA[Lr] = np.broadcast_to(w, U[0].shape)
        for l in range(Lr, 0, -1):
            AA[l - 1] = AA[l] + hN * R.mm(TH[l] * AA[l], K[l].T)
        y = TH[0] * AA[0]
        G = R.mm(y, K[0].T) + ZA @ A + cw
        GB, XD = np.zeros((n, D1)), np.zeros((n, d))
        if fin:
            PHI = U[Lr] @ w + 0.5 * np.sum(ZA * ZA, 1) + s @ cw + R.cb
            res = s[:, :d] - R.xt
            cG = 0.5 * np.sum(res * res, 1)
            ef = _sign(PHI - a0 * cG)
            dg = G[:, :d] - a0 * res
            eg = _sign(dg)
            LAM = inv * (a0 * res + a4 * ef[:, None] * dg - a5 * a0 * eg)
            GB[:, :d] = inv * a5 * eg
            phib = inv * a4 * ef
            val = dict(Qb=[phib[:, None] * hN * TH[i] * AA[i] for i in range(1, Lr + 1)], U0=[U[i - 1] for i in range(1, Lr + 1)],
                       Ob=phib[:, None] * y, Wb=phib[:, None] * U[Lr], Sx=s, PHIb=phib)
        else:
            x, p = s[:, :d], G[:, :d]
            _, H, _, _ = R.lhqw(x, p)
            eh = _sign(G[:, d] - H)
            kL = np.full(n, hs * wst * inv)
            ekh = eh * hs * wst * a3 * inv
            if S.kind == orc.KIND_QUAD:
                GB[:, :d], XD = _quad_adjoint_np(S, x, p, LAM, XP, hs, wst, cpl, kL, ekh)
            else:
                fbar = hs * (wst * LAM + cpl * XP)
                GB[:, :d] = -fbar + (kL - ekh)[:, None] * p
                XD = _xgrad_np(R, x, kL + ekh)
            GB[:, d] = ekh
        # the vector-Jacobian product of grad Phi
        ZB = GB @ A.T
        yb = R.mm(GB, K[0])
        AB = TH[0] * yb
        TB = [AA[0] * yb]
        for i in range(1, Lr + 1):
            lay_rows[i - 1]["V"].append(hN * TH[i] * AA[i])
            lay_rows[i - 1]["Ab"].append(AB.copy())
            lay_rows[i - 1]["U0"].append(U[i - 1])
            vb = hN * R.mm(AB, K[i])
            TB.append(AA[i] * vb)
            AB = AB + TH[i] * vb
        st_rows["Wb"].append(AB)
        UB = np.zeros_like(AB)
        for i in range(Lr, 0, -1):
            QB = (1.0 - TH[i] * TH[i]) * TB[i] + (0.0 if i == Lr else hN * TH[i] * UB)
            lay_rows[i - 1]["Qb"].append(QB)
            UB = UB + R.mm(QB, K[i].T)
        QB = (1.0 - TH[0] * TH[0]) * TB[0] + TH[0] * UB
        st_rows["Ob"].append(QB)
        SBAR = R.mm(QB, K[0].T) + ZB @ A
        st_rows["Y"].append(y)
        st_rows["Gb"].append(GB)
        st_rows["Sx"].append(s)
        xb = SBAR[:, :d] + XD
        if fin:
            LAM = LAM + xb
        else:
            XP = xb
            XS = XS + xb
            if st == 0:
                LAM = LAM + XS
    cat = lambda rows: np.concatenate(rows[::-1], 0)                         # (the streams' row order: evaluation 0 first)
    Y, Gb, Sx, Ob, Wb = (cat(st_rows[k]) for k in ("Y", "Gb", "Sx", "Ob", "Wb"))
    sT, PHIb = val["Sx"], val["PHIb"]
    z = np.zeros_like
    Obv, Sxv = np.concatenate([Ob, val["Ob"]], 0), np.concatenate([Sx, sT], 0)
    out = {"N.layers.0.weight": Obv.T @ Sxv + Y.T @ Gb, "N.layers.0.bias": Obv.sum(0)}
    for i in range(1, Lr + 1):
        r_ = lay_rows[i - 1]
        Qb = np.concatenate([cat(r_["Qb"]), val["Qb"][i - 1]], 0)
        U0 = np.concatenate([cat(r_["U0"]), val["U0"][i - 1]], 0)
        out[f"N.layers.{i}.weight"] = Qb.T @ U0 + cat(r_["V"]).T @ cat(r_["Ab"])
        out[f"N.layers.{i}.bias"] = Qb.sum(0)
    out["w.weight"] = np.concatenate([Wb, val["Wb"]], 0).sum(0).reshape(1, -1)
    out["c.weight"] = (Gb.sum(0) + PHIb @ sT).reshape(1, -1)
    out["c.bias"] = PHIb.sum().reshape(1)
    dM = Gb.T @ Sx + 0.5 * (sT * PHIb[:, None]).T @ sT
    out["A"] = A @ (dM + dM.T)
    out["x0"] = LAM
    return out


def _autograd(case):
    sd = {k: v.clone().requires_grad_(True) for k, v in state_dict(case).items()}
    x = starts(case).requires_grad_(True)
    P = orc.PhiParams.from_state_dict(sd)
    Jc, _ = orc.rollout(x, P, spec_of(case), list(case.tspan), case.nt, case.stepper, list(ALPH))
    names = list(sd)
    gs = torch.autograd.grad(Jc, [sd[k] for k in names] + [x], allow_unused=True)
    out = {k: (torch.zeros_like(sd[k]) if g is None else g).numpy() for k, g in zip(names, gs[:-1])}
    out["x0"] = gs[-1].numpy()
    return float(Jc.detach()), out


@functools.lru_cache(None)
def oracle_grads(case):
    """fp64 autograd of the oracle -> (Jc, {name: gradient}) for every parameter tensor and "x0" """
    return _autograd(case)


def mutated_grads(case):
    with no_eval_soft_term():
        return _autograd(case)


def directions(case):
    """[(name, label, v)]: per parameter tensor one seeded random direction and unit directions at its first entry, its last entry and the
    entry where the fp64 autograd gradient is largest; for x0 one random direction and two unit directions (first entry, largest gradient)"""
    _, og = oracle_grads(case)
    out = []
    for j, name in enumerate(param_names(case) + ["x0"]):
        g = og[name]
        rng = np.random.default_rng(977 + j)
        out.append((name, "random", rng.standard_normal(g.shape)))
        picks = [("first", 0), ("argmax", int(np.abs(g).argmax()))] if name == "x0" else [("first", 0), ("last", g.size - 1),
                                                                                           ("argmax", int(np.abs(g).argmax()))]
        for label, idx in picks:
            v = np.zeros(g.size)
            v[idx] = 1.0
            out.append((name, label, v.reshape(g.shape)))
    return out


@functools.lru_cache(None)
def grad_truth(case):
    """-> (Jc in longdouble, [(name, label, v, Im J(theta + i h v) / h, sum |g_i v_i| of the oracle's gradient)])"""
    S = spec_of(case)
    sd0, x0 = state_dict(case), starts(case)
    J = Restate(sd0, S, LD).rollout(x0, case.tspan, case.nt, case.stepper, ALPH)["Jc"]
    _, og = oracle_grads(case)
    out = []
    for name, label, v in directions(case):
        sd = {k: t.numpy().astype(CLD) for k, t in sd0.items()}
        x = x0.numpy().astype(CLD)
        if name == "x0":
            x = x + 1j * H_STEP * v.astype(LD)
        else:
            sd[name] = sd[name] + 1j * H_STEP * v.astype(LD)
        Jv = Restate(sd, S, CLD).rollout(x, case.tspan, case.nt, case.stepper, ALPH)["Jc"]
        out.append((name, label, v, LD(Jv.imag) / H_STEP, float(np.abs(og[name].astype(LD) * v).sum())))
    return J, out


def dot(g, v):
    """g . v in longdouble from a double gradient"""
    return (np.asarray(g, dtype=LD).reshape(-1) * np.asarray(v, dtype=LD).reshape(-1)).sum()


# Quantities whose yardstick is doubled: (case id, quantity) -> the kernels' error as measured on the MI355X, beyond 4 x the torch-fp64
# oracle's error there.  Each takes the larger of the two fp64 restatements' errors, the oracle's and the second restatement's (values:
# second_values, the numpy restatement in float64 with sigma and tanh from one expm1 as f64_act_pair forms them and products summed one k
# after the other from the bias by fused multiply-adds; gradients: second_grads, the adjoint as nocf_f64_bwd.inc and train.py form it);
# factor and floor unchanged.  tests/test_f64_sweep_cpu.py asserts for every entry that 4 x the second restatement's error reaches the
# measured figure; an entry for which it does not is not listed here and fails.  Every other quantity keeps the oracle alone.
# All gradient entries are unit directions (one of them over x0): one entry of a gradient is a sum of cancelling terms whose rounding is a single draw.
SECOND = {
    ("swap12_1pair-n513-L2-m24-rk4-nt2-train", "table.W"): 1.554e-15, ("swap12_1pair-n513-L2-m24-rk4-nt2-eval", "table.W"): 1.554e-15,
    ("softcorridor-n5-L2-m24-rk4-nt2-train", "N.layers.1.bias/first"): 2.151e-14,
    ("softcorridor-n5-L2-m24-rk4-nt2-train", "N.layers.1.bias/last"): 2.062e-14,
    ("softcorridor-n5-L2-m24-rk4-nt2-eval", "N.layers.1.bias/first"): 2.055e-14,
    ("softcorridor-n5-L2-m24-rk4-nt2-eval", "N.layers.1.bias/last"): 2.074e-14,
    ("swarm-n5-L2-m24-rk4-nt1-train", "N.layers.0.weight/first"): 4.785e-13, ("swarm-n5-L2-m24-rk4-nt1-train", "N.layers.0.bias/first"): 3.098e-13,
    ("singlequad-n7-L3-m24-rk4-nt2-train", "A/first"): 6.951e-14, ("singlequad-n7-L3-m24-rk4-nt2-train", "A/last"): 3.198e-14,
    ("singlequad-n7-L3-m24-rk4-nt2-train", "N.layers.2.bias/first"): 3.121e-15,
    ("softcorridor-n1-L2-m24-rk1-nt3-eval", "N.layers.0.weight/first"): 2.68e-13,
    ("midcross4-n3-L6-m200-rk1-nt1-train", "N.layers.5.bias/last"): 5.02e-13,
    ("midcross4-n1-L9-m256-rk1-nt1-train", "N.layers.7.weight/first"): 3.11e-13,
    ("midcross4-n1-L9-m256-rk1-nt1-train", "N.layers.7.bias/first"): 2.55e-13,
    ("midcross4-n1-L9-m256-rk1-nt1-train", "N.layers.7.bias/argmax"): 8.27e-13,
    ("midcross4-n3-L2-m260-rk4-nt1-train", "c.weight/argmax"): 2.14e-11,
    ("midcross4-n1-L4-m512-rk1-nt1-train", "N.layers.1.weight/last"): 5.734e-11,
    ("midcross4-n1-L4-m512-rk1-nt1-train", "N.layers.2.weight/last"): 2.2e-11,
    ("midcross4-n1-L4-m512-rk1-nt1-train", "N.layers.2.bias/last"): 6.7e-12,
    ("midcross4-n1-L4-m512-rk1-nt1-train", "N.layers.3.bias/last"): 3.72e-12,
    ("midcross4-n3-L4-m24-rk4-nt1-train-T2", "N.layers.0.weight/first"): 4.91e-12,
    ("midcross4-n3-L4-m24-rk4-nt1-train-T2", "N.layers.2.bias/last"): 1.5e-12,
    ("midcross4-n3-L4-m24-rk4-nt1-train-T2", "N.layers.3.bias/last"): 8.3e-13,
    ("midcross4-n3-L2-m24-rk1-nt2-train-T4", "N.layers.0.weight/last"): 8.38e-14,
    ("midcross4-n3-L2-m257-rk1-nt1-train-T1", "N.layers.0.bias/last"): 8.64e-12,
    ("midcross4-n3-L2-m257-rk1-nt1-train-T2", "N.layers.0.bias/last"): 8.64e-12,
    ("softcorridor-n5-L2-m24-rk4-nt3-eval-seg", "table.W"): 4.170e-16,
    ("swap2-n6-L2-m24-rk1-nt3-train", "N.layers.1.bias/first"): 2.034e-14, ("swap2-n6-L2-m24-rk1-nt3-train", "N.layers.1.bias/last"): 3.705e-14,
    ("softcorridor-n1-L2-m24-rk1-nt3-eval", "N.layers.0.bias/first"): 3.912e-14,
    ("swap2-n5-L2-m24-rk4-nt1-eval", "N.layers.0.weight/last"): 1.244e-13, ("swap2-n5-L2-m24-rk4-nt1-eval", "N.layers.1.bias/last"): 3.282e-13,
    ("midcross4-n5-L2-m24-rk4-nt2-train-seg", "N.layers.0.weight/last"): 1.472e-14,
    ("midcross4-n5-L2-m24-rk4-nt2-train-seg", "N.layers.0.bias/last"): 2.499e-14,
    ("midcross4-n5-L2-m24-rk4-nt2-train-seg", "N.layers.1.bias/last"): 1.357e-14,
    ("midcross4-n5-L2-m24-rk4-nt2-train-seg", "x0/first"): 5.472e-14,
    ("midcross4-n3-L4-m24-rk4-nt1-train-T2", "N.layers.2.bias/first"): 1.627e-12,
    ("midcross4-n3-L2-m24-rk1-nt2-train-T4", "N.layers.1.bias/last"): 3.362e-13,
}


def takes_second(case, key):
    return (case.id, key) in SECOND


def _wider(first, ref2, want):
    """first = compare(got, want, oracle) re-judged with the larger of the oracle's and ref2's error"""
    ok, err, tol, e_ref = first
    e2 = float(np.abs(np.asarray(ref2, dtype=LD) - np.asarray(want, dtype=LD)).max())
    tol = max(tol, TOL_FACTOR * e2)
    return bool(err <= tol), err, tol, max(e_ref, e2)


def compare_grads(case, grads, second=True):
    """grads {name: array}: the code under test -> {name/label: (ok, err, tol, oracle error)}; second: the entries of SECOND take the larger of the two
    restatements' errors"""
    _, og = oracle_grads(case)
    out = {}
    for name, label, v, want, scale in grad_truth(case)[1]:
        key = f"{name}/{label}"
        out[key] = compare(dot(grads[name], v), want, dot(og[name], v), scale=scale)
        if second and takes_second(case, key):
            out[key] = _wider(out[key], dot(second_grads(case)[name], v), want)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# Phi and the problem calls
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def phi_points(case):
    g = torch.Generator().manual_seed(55 + case.n)
    return torch.randn(case.n, case.d + 1, generator=g, dtype=TF64)


@functools.lru_cache(None)
def phi_truth(case):
    """-> rows, truth (grad, value) in longdouble on them, oracle (grad, value) on ALL rows"""
    rows = truth_rows(case, case.plan(PHI)["T"])
    s = phi_points(case)
    g, v = Restate(state_dict(case), spec_of(case), LD).phi(s[rows].numpy().astype(LD), value=True)
    P = orc.PhiParams.from_state_dict(state_dict(case), dtype=TF64)
    with torch.no_grad():
        og, ov = orc.phi_grad(P, s).numpy(), orc.phi_value(P, s).numpy().reshape(-1)
    return rows, (g, v), (og, ov)


@functools.lru_cache(None)
def prob_truth(case):
    """calcLHQW / calcGradpH / calcCtrls at the case's starts and seeded momenta -> p, truth dict, oracle dict, keep (screen)"""
    x = starts(case)
    g = torch.Generator().manual_seed(9)
    p = 0.7 * torch.randn(x.shape, generator=g, dtype=TF64)
    S = spec_of(case)
    R = Restate(state_dict(case), S, LD)
    xl, pl = x.numpy().astype(LD), p.numpy().astype(LD)
    L, H, Q, W = R.lhqw(xl, pl)
    t = dict(L=L, H=H, Q=Q, W=W, gradpH=R.gradpH(xl, pl), ctrls=R.ctrls(xl, pl))
    oL, oH, oQ, oW = orc.prob_LHQW(S, x, p)
    f = lambda v: torch.as_tensor(v, dtype=TF64).reshape(x.shape[0], -1).numpy()
    o = dict(L=f(oL)[:, 0], H=f(oH)[:, 0], Q=f(oQ)[:, 0], W=f(oW)[:, 0], gradpH=f(orc.prob_gradpH(S, x, p)), ctrls=f(orc.prob_ctrls(S, x, p)))
    keep = ~uo.near_edge(S, x.reshape(x.shape[0], 1, -1)).numpy()
    return p, t, o, keep


# ---------------------------------------------------------------------------------------------------------------------------------
# the case lists of tests/test_f64_sweep_gpu.py (tests/test_f64_sweep_cpu.py asserts from the mirror what they reach)
# ---------------------------------------------------------------------------------------------------------------------------------
def problem_names():
    import importlib
    return sorted(importlib.import_module("neuraloc_amd.initProb").PROBLEM_NAMES)


C = Case
# rollout: plain / recording / intermediates; rk1 and rk4
ROLLOUT_CASES = [
    C("midcross4", 1), C("midcross4", 3, stepper="rk1", nt=3), C("midcross4", 513, nt=3), C("midcross4", 1026, stepper="rk1", nt=2),
    C("midcross4", 1025, m=130, nt=1),
    # a time segment: t0 != 0 and h = (t1 - t0) / nt in the stage times, the time column of the stage inputs and the final time of Phi
    C("softcorridor", 5, nt=3, tspan=(0.25, 0.9)), C("swap12", 513, stepper="rk1", nt=3, tspan=(0.25, 0.9)),
    C("midcross4", 3, m=260, nt=1), C("midcross4", 3, m=520, nt=1, stepper="rk1"), C("midcross4", 513, m=260, nt=1, stepper="rk1"),
    C("midcross4", 513, m=520, nt=1),
    C("midcross4", 1025, m=260, nt=1), C("midcross4", 1025, m=520, nt=1, stepper="rk1"), C("softcorridor", 1025, m=260, nt=1, stepper="rk1"),
    C("swarm50", 1025, m=260, nt=1, stepper="rk1", training=True), C("midcross4", 1025, m=258, nt=1, stepper="rk1"),
    # LDS fallbacks at n >= 1024: 4 -> 2 and 2 -> 1 (m = 512; nocf_debug_f64_plan / f64_plan give the depths)
    C("midcross4", 1025, nTh=7, m=512, nt=1, stepper="rk1"), C("midcross4", 1025, nTh=17, m=512, nt=1, stepper="rk1"),
]
LDS_REFUSED = C("midcross4", 1025, nTh=36, m=512, nt=1, stepper="rk1")
# physics: every initProb problem in both modes at T = 2 and T = 4, a small narrow network
ALL_PROBLEMS = ("midcross2", "midcross20", "midcross30", "midcross4", "singlequad", "softcorridor", "swap12", "swap12_1pair", "swap12_2pair",
                "swap12_3pair", "swap12_4pair", "swap12_5pair", "swap2", "swarm", "swarm50")          # initProb's PROBLEM_NAMES
PHYSICS_CASES = [C(name, n, nTh=2, m=24, nt=2, training=tr) for name in ALL_PROBLEMS for n in (513, 1026) for tr in (True, False)]
COST_SUM_N = (1, 255, 513)
# adjoint: natural shapes of the five instantiations (the LDS decides), each again forced by NOCF_F64_BWD_T on a small network; all three
# problem classes in train mode; eval mode on the soft corridor (the fixed term), the hard corridor (a mask) and singlequad
ADJOINT_CASES = [
    C("softcorridor", 5, m=24, training=True), C("swap2", 6, m=24, training=True, stepper="rk1", nt=3),
    C("swarm", 5, m=24, training=True, nt=1), C("singlequad", 7, nTh=3, m=24, training=True),
    C("softcorridor", 5, m=24), C("softcorridor", 1, m=24, stepper="rk1", nt=3), C("swap2", 5, m=24, nt=1), C("singlequad", 3, m=24, stepper="rk1"),
    C("midcross4", 5, m=24, training=True, nt=2, tspan=(0.25, 0.9)),              # a time segment
    C("midcross4", 3, nTh=6, m=200, training=True, nt=1, stepper="rk1"),          # narrow, 4 -> 2
    C("midcross4", 1, nTh=9, m=256, training=True, nt=1, stepper="rk1"),          # narrow, 2 -> 1
    C("midcross4", 3, nTh=2, m=260, training=True, nt=1),                         # wide, 2
    C("midcross4", 1, nTh=4, m=512, training=True, nt=1, stepper="rk1"),          # wide, 2 -> 1
    C("midcross4", 3, nTh=4, m=24, training=True, nt=1, bwd_t=2), C("softcorridor", 3, m=24, nt=1, bwd_t=1),
    C("midcross4", 3, m=24, training=True, stepper="rk1", bwd_t=4),
    C("midcross4", 3, m=257, training=True, nt=1, stepper="rk1", bwd_t=1), C("midcross4", 3, m=257, training=True, nt=1, stepper="rk1", bwd_t=2),
]
EVAL_SOFT_ADJOINT = C("softcorridor", 5, m=24)
PHI_CASES = [C("midcross4", n, nTh=2, m=m) for n in (3, 513, 1025) for m in (24, 520)]
PROB_CASES = [C(name, n, training=tr) for name in ALL_PROBLEMS for n in (1, 19) for tr in (True, False)]
