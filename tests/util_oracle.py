"""oracle-side helpers shared by the tests (CPU only: nothing here touches a GPU)

The direct-transcription baseline (baseline2D.py, compareCorridor.py) restated on oracle.ocflow_oracle: the objective, its gradient and
the report, in fp32 and fp64, for a batch of starts at once; the fp32 Euler trajectory the kernels reproduce bit for bit; the screen
that keeps starts away from the problems' decision edges; the self-calibrating comparator; and the case list of the baseline sweep
(tests/test_baseline_sweep_gpu.py runs it on the GPU, tests/test_baseline_cpu.py checks that the comparator has teeth on it)."""
import dataclasses

import torch

from oracle import ocflow_oracle as orc


def spec_of(g, training):
    m = g.meta
    kind = {"Cross2D": orc.KIND_CROSS2D, "SwarmTraj": orc.KIND_SWARM, "Quadcopter": orc.KIND_QUAD}[m["prob_class"]]
    return orc.ProbSpec(kind=kind, xtarget=g.t("xtarget"), obstacle=m["obstacle"], alph_Q=m["alph_Q"],
                        alph_W=m["alph_W"], r=m["r"], training=training)


def oracle_objective(S, U, z0, nt, alphG):
    """baseline2D.py:42-63 restated on the oracle's calcLHQW (oracle.prob_LHQW)"""
    h = 1. / nt
    Z, loss = z0, 0
    for i in range(nt):
        Z = Z + h * U[i]
        L, _, _, _ = orc.prob_LHQW(S, Z.view(1, -1), U[i].view(1, -1))
        loss = loss + h * L
    return (loss + alphG * 0.5 * torch.sum((Z - S.xtarget) ** 2)).reshape(())


# ---------------------------------------------------------------------------------------------------------------------------------
# the baseline restated for a batch of starts
# ---------------------------------------------------------------------------------------------------------------------------------
def euler_traj_f32(z0, U):
    """z_{i+1} = z_i + (1/nt) u_i in fp32, one torch op at a time on the CPU (the reference's recursion, baseline2D.py:50-51).
    z0 [..., d], U [..., nt, d] -> [..., nt+1, d]"""
    nt = U.shape[-2]
    h = 1. / nt
    Z = [z0.detach().float().cpu()]
    Uf = U.detach().float().cpu()
    for i in range(nt):
        Z.append(Z[-1] + h * Uf[..., i, :])
    return torch.stack(Z, -2)


def _lhqw(S, X, P, B, nt, w_spec=None):
    """calcLHQW on B*nt rows -> L, Q, W each [B, nt].  w_spec: take W (and its term in L) from this spec instead of S."""
    d = X.shape[-1]
    L, _, Q, W = orc.prob_LHQW(S, X.reshape(-1, d), P.reshape(-1, d))
    if w_spec is not None and S.alph_W != 0.0:
        W2 = orc.prob_W(w_spec, X.reshape(-1, d)).reshape(L.shape)
        L = L + S.alph_W * (W2 - W.reshape(L.shape))
        W = W2
    return (torch.as_tensor(L).reshape(B, nt), torch.as_tensor(Q).reshape(B, nt).to(L.dtype),
            torch.as_tensor(W).reshape(B, nt).to(L.dtype))


MUTATIONS = ("pre_state", "h_nt_plus_1", "train_threshold_in_eval", "last_step_detached")


def restate(S, z0, U, alphG, dtype, traj=None, mutation=None):
    """The baseline objective (baseline2D.py:42-63), dJ/dU by autograd, and the report (compareCorridor.py:100-113) for B starts.
    S: ProbSpec (train / eval from its .training); z0 [B, d]; U [B, nt, d]; dtype: float32 or float64.
    Everything is evaluated at `traj` ([B, nt+1, d], default: the fp32 trajectory), the trajectory the kernels compute bit for bit;
    autograd still sees z_{i+1} = z_i + h u_i.  mutation: one of MUTATIONS, a deliberately wrong restatement (for the comparator's
    teeth).  -> dict J [B], grad [B, nt, d], report [B, 5] (L+G, L, G, Q, W) in `dtype`"""
    B, nt, d = U.shape
    if traj is None:
        traj = euler_traj_f32(z0, U)
    Sd = S.to(dtype)
    h = 1. / (nt + 1) if mutation == "h_nt_plus_1" else 1. / nt
    u = U.detach().cpu().to(dtype).clone().requires_grad_(True)
    lin = torch.cat([torch.zeros(B, 1, d, dtype=dtype), torch.cumsum(h * u, 1)], 1)
    Z = traj.to(dtype) + (lin - lin.detach())                          # the fp32 trajectory's values, the recursion's derivative
    w_spec = dataclasses.replace(Sd, training=True) if (mutation == "train_threshold_in_eval" and not Sd.training) else None
    X = Z[:, :-1] if mutation == "pre_state" else Z[:, 1:]
    if mutation == "last_step_detached":
        X = torch.cat([X[:, :-1], X[:, -1:].detach()], 1)
    L, _, _ = _lhqw(Sd, X, u, B, nt, w_spec)
    loss = 0
    for i in range(nt):                                                  # the reference's running sum
        loss = loss + h * L[:, i]
    J = loss + alphG * 0.5 * torch.sum((Z[:, -1] - Sd.xtarget) ** 2, -1)
    (grad,) = torch.autograd.grad(J.sum(), u)
    with torch.no_grad():
        L, Q, W = _lhqw(Sd, Z[:, :-1], u, B, nt, w_spec)
        aL = aQ = aW = 0
        for j in range(nt):
            aL = aL + h * L[:, j]
            aQ = aQ + h * Q[:, j]
            aW = aW + h * W[:, j]
        G = alphG * 0.5 * torch.sum((Z[:, -1] - Sd.xtarget) ** 2, -1)
        rep = torch.stack([G + aL, aL, G, aQ, aW], 1)
    return dict(J=J.detach(), grad=grad, report=rep)


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------------------------------------------
TOL_FACTOR = 4.0
TOL_FLOOR = 1e-6


def tolerance(want64, ref32):
    """the error allowed for one quantity: TOL_FACTOR x the fp32 restatement's own max error against fp64, at least
    TOL_FLOOR x max|want|"""
    want64 = want64.double()
    e32 = float((ref32.double() - want64).abs().max())
    return max(TOL_FACTOR * e32, TOL_FLOOR * float(want64.abs().max())), e32


def compare(got, want64, ref32):
    """-> (ok, err, tol, err32) for one quantity: got / ref32 against want64 over the whole tensor"""
    tol, e32 = tolerance(want64, ref32)
    err = float((got.detach().double().cpu() - want64.double()).abs().max())
    return err <= tol, err, tol, e32


def compare_all(got, want64, ref32):
    """got / want64 / ref32: dicts of restate().  J, dJ/dU, and each report column on its own -> {name: (ok, err, tol, err32)}"""
    out = {"J": compare(got["J"], want64["J"], ref32["J"]), "grad": compare(got["grad"], want64["grad"], ref32["grad"])}
    if got.get("report") is not None:
        for c, name in enumerate(("L+G", "L", "G", "Q", "W")):
            out[f"report.{name}"] = compare(got["report"][:, c], want64["report"][:, c], ref32["report"][:, c])
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# starts, screen
# ---------------------------------------------------------------------------------------------------------------------------------
W_REL = 1e-4          # pair distances: relative to the W threshold
HARD_ABS = 1e-4       # hard-corridor norms
BOX_ABS = 1e-5        # SwarmTraj block coordinates
PERTURB, USPREAD = 0.3, 0.5


def near_edge(S, Z):
    """Z [B, nt+1, d] (the fp32 trajectory) -> bool [B]: some state lies within the margins of a decision edge of S's problem, in
    train or eval mode (tests/golden/make_golden_baseline.py documents the same screen)"""
    B = Z.shape[0]
    ad, N = S.agent_dim, S.n_agents
    X = Z.double().reshape(B, Z.shape[1], N, ad)
    bad = torch.zeros(B, dtype=torch.bool)
    if N >= 2 and S.alph_W != 0.0:
        iu = torch.triu_indices(N, N, 1)
        dd = (X[:, :, iu[0]] - X[:, :, iu[1]]).norm(dim=-1)
        ftrain = 3.2 if (S.kind == orc.KIND_SWARM and N > 2) else 2.2
        for thr in (ftrain * S.r, 2.0 * S.r):
            bad |= ((dd - thr).abs() <= W_REL * thr).flatten(1).any(1)
    if S.obstacle == "hardcorridor":
        for mu in ((0., 4.), (0., -3.5)):
            n = torch.sqrt((X[..., 0] - mu[0]) ** 2 + (X[..., 1] - mu[1]) ** 2)
            for thr in (2.0 + S.r, 2.0):
                bad |= ((n - thr).abs() <= HARD_ABS).flatten(1).any(1)
    if S.obstacle == "blocks":
        r = S.r
        bounds = [(0, [2.0 + r, -2.0 - r, 4.0 + r, 2.0 - r, 2.0, -2.0, 4.0]),
                  (1, [0.5 + r, -0.5 - r, 1.0 + r, -1.0 - r, 0.5, -0.5, 1.0, -1.0]), (2, [7.0 + r, 4.0 + r, 7.0, 4.0])]
        for k, bs in bounds:
            for bnd in bs:
                bad |= ((X[..., k] - bnd).abs() <= BOX_ABS).flatten(1).any(1)
    return bad


SEEDS = tuple(range(1000, 2024))


def _draw(S, centre, nt, count, seeds):
    d = centre.numel()
    xt = S.xtarget.detach().float().cpu().reshape(-1)
    z0s, Us, trajs, used = [], [], [], []
    for c0 in range(0, len(seeds), 32):
        chunk = seeds[c0:c0 + 32]
        zc, Uc = [], []
        for seed in chunk:
            g = torch.Generator().manual_seed(seed * 1000 + nt)
            z0 = centre + PERTURB * torch.randn(d, generator=g)
            zc.append(z0)
            Uc.append((xt - z0) * torch.ones(nt, d) + USPREAD * torch.randn(nt, d, generator=g))
        zc, Uc = torch.stack(zc), torch.stack(Uc)
        tc = euler_traj_f32(zc, Uc)
        for i in (~near_edge(S, tc)).nonzero().flatten().tolist()[:count - len(used)]:
            z0s.append(zc[i]); Us.append(Uc[i]); trajs.append(tc[i]); used.append(chunk[i])
        if len(used) == count:
            return torch.stack(z0s), torch.stack(Us), torch.stack(trajs), used
    raise AssertionError(f"only {len(used)} of {len(seeds)} seeds pass the screen (nt = {nt}), {count} wanted")


def draw_starts(S, xInit, nt, count, mid=0, seeds=SEEDS):
    """the first seeds whose start passes the screen: z0 = xInit + 0.3 randn, U = (xtarget - z0) + 0.5 randn (a CPU generator per seed);
    the last `mid` of the `count` starts are drawn around the middle of the path, (xInit + xtarget) / 2, instead.
    -> (z0 [count, d], U [count, nt, d], fp32 trajectory [count, nt+1, d], seeds used)"""
    xi = xInit.detach().float().cpu().reshape(-1)
    xt = S.xtarget.detach().float().cpu().reshape(-1)
    parts = [_draw(S, xi, nt, count - mid, seeds)] + ([_draw(S, 0.5 * (xi + xt), nt, mid, seeds)] if mid else [])
    return tuple(torch.cat([p[k] for p in parts]) for k in range(3)) + (sum((p[3] for p in parts), []),)


# ---------------------------------------------------------------------------------------------------------------------------------
# the case list of the baseline sweep
# ---------------------------------------------------------------------------------------------------------------------------------
# alph (G, Q, W) per problem: the deployment lines of the four point-agent problems the reference logs, the baseline driver's default
# (100, 1e4, 300) for the other Cross2D problems, swap12's for its sub-problems
BASE_ALPH = {"softcorridor": (100.0, 1e4, 300.0), "midcross2": (100.0, 1e4, 300.0), "swap2": (300.0, 1e6, 1e5),
             "swap12": (300.0, 0.0, 1e5), "swap12_1pair": (300.0, 0.0, 1e5), "swap12_2pair": (300.0, 0.0, 1e5),
             "swap12_3pair": (300.0, 0.0, 1e5), "swap12_4pair": (300.0, 0.0, 1e5), "swap12_5pair": (300.0, 0.0, 1e5),
             "midcross4": (100.0, 1e4, 300.0), "midcross20": (100.0, 1e4, 300.0), "midcross30": (100.0, 1e4, 300.0),
             "swarm": (900.0, 1e7, 25000.0), "swarm50": (900.0, 1e7, 25000.0)}
N_AGENTS = {"softcorridor": 2, "midcross2": 2, "swap2": 2, "swap12": 12, "swap12_1pair": 2, "swap12_2pair": 4, "swap12_3pair": 6,
            "swap12_4pair": 8, "swap12_5pair": 10, "midcross4": 4, "midcross20": 20, "midcross30": 30, "swarm": 32, "swarm50": 50}
# the largest nt each entry point accepts (nocf_baseline.inc bl_layout within 160 KiB of LDS, NOCF_BL_MAX_NT = 256): (eval, adam)
NT_LIMIT = {"midcross20": (256, 186), "midcross30": (206, 124), "swarm": (129, 78), "swarm50": (83, 50)}
NT_MAX = 256
# alph variants: Q or W switched off (the reference's placeholder columns, Cross2D.py:79-83, SwarmTraj.py:73-83)
VARIANTS = {"softcorridor": (100.0, 0.0, 300.0), "swarm": (900.0, 0.0, 25000.0), "midcross4": (100.0, 1e4, 0.0)}
# swap2's straight paths pass between the hard corridor's two discs and never meet them: its starts are moved first (agent 1 down by
# 3.2 toward the lower disc, agent 2 by 1.2 to pass close to agent 1) so that Q and W are nonzero on the way, in both modes
START_SHIFT = {"swap2": (0.0, -3.2, 0.0, -1.2)}
# below this nt a straight path from xInit steps over the obstacles and the other agents (at nt = 1 its states are the two ends):
# two of the three starts of such a case begin half-way along the path, where the agents meet each other and the obstacles
MIDPATH_NT = 16


def nt_limits(name):
    return NT_LIMIT.get(name, (NT_MAX, NT_MAX))


def launch_shape(N, nt):
    """baseline_setup's choice (nocf_kernels.hip): threads per workgroup and lanes per time step"""
    nth = 1024 if nt * N >= 512 else 256
    G = 64
    while G > 1 and G * nt > nth:
        G //= 2
    return nth, G


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    nt: int
    mode: str                 # "train" / "eval"
    alph: tuple               # (G, Q, W)
    starts: int = 3

    @property
    def id(self):
        v = "" if self.alph == BASE_ALPH[self.name] else "-Q0" if self.alph[1] == 0.0 else "-W0"
        return f"{self.name}{v}-nt{self.nt}-{self.mode}"


def case_nts(name):
    """nt = 1, 7, 9 (G = 64 / 32 / 16 at 256 threads; bl_forward's tail alone, or after one 8-step block), the largest nt below the
    1024-thread switch and the next, and the largest nt of each entry point"""
    N = N_AGENTS[name]
    lo = (512 + N - 1) // N - 1
    return sorted({1, 7, 9, lo, lo + 1, *nt_limits(name)})


def sweep_cases():
    cases = []
    for p, name in enumerate(sorted(BASE_ALPH)):
        for q, nt in enumerate(case_nts(name)):
            # from nt = 128 on one mode per (problem, nt), alternating, so that each (nth, G) pair still meets both modes
            modes = ("train", "eval") if nt < 128 else (("train",) if (p + q) % 2 == 0 else ("eval",))
            cases += [Case(name, nt, m, BASE_ALPH[name], 2 if nt >= 128 else 3) for m in modes]
    for name, alph in VARIANTS.items():
        N = N_AGENTS[name]
        for nt in (7, (512 + N - 1) // N):
            cases += [Case(name, nt, m, alph) for m in ("train", "eval")]
    return cases


SWEEP = sweep_cases()


def make_prob(name, alph, mode, device="cpu"):
    """the package's problem object (initProb's draws are not used) in `mode` -> (prob, xInit [d])"""
    import neuraloc_amd as na
    prob, _, _, xInit = na.initProb(name, 2, 2, var0=1.0, cvt=lambda t: t.float().to(device),
                                    alph=[alph[0], alph[1], alph[2], 0.0, 0.0, 0.0])
    prob.train() if mode == "train" else prob.eval()
    return prob, xInit.reshape(-1)


_STARTS = {}


def case_data(case):
    """-> (ProbSpec of the case's mode, z0 [S, d], U [S, nt, d], fp32 trajectory [S, nt+1, d]); the starts depend on the problem, alph
    and nt only (both modes share them), and are cached"""
    prob, xInit = make_prob(case.name, case.alph, case.mode)
    if case.name in START_SHIFT:
        xInit = xInit + torch.tensor(START_SHIFT[case.name])
    S = orc.ProbSpec.from_object(prob)
    key = (case.name, case.alph, case.nt, case.starts)
    if key not in _STARTS:
        z0, U, traj, _ = draw_starts(S, xInit, case.nt, case.starts, mid=2 if case.nt < MIDPATH_NT else 0)
        _STARTS[key] = (z0, U, traj)
    return (S,) + _STARTS[key]


def physics_gaps(case, S, r64):
    """-> the reasons the case does not exercise the physics it should (empty: it does).  With an obstacle and
    alph_Q != 0 the fp64 Q sum is > 0 for some start, and with alph_W != 0 and N >= 2 so is the W sum; Q / W switched off: exactly 0."""
    out = []
    q, w = r64["report"][:, 3], r64["report"][:, 4]
    if S.obstacle is not None and S.alph_Q != 0.0 and not bool((q > 0).any()):
        out.append("Q sum is 0 for every start")
    if S.alph_W != 0.0 and S.n_agents >= 2 and not bool((w > 0).any()):
        out.append("W sum is 0 for every start")
    if S.alph_Q == 0.0 and bool((q != 0).any()):
        out.append("alph_Q = 0 but Q != 0")
    if S.alph_W == 0.0 and bool((w != 0).any()):
        out.append("alph_W = 0 but W != 0")
    return out
