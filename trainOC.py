#!/usr/bin/env python3
"""trainOC-style driver on the MI355X path.

Same flags, log columns and checkpoint layout as the reference driver (trainOC.py:22-63 flags, :155-160 header,
:176-196 iteration line, :199-207 checkpoint, :249-265 lr decay / resampling / alph switch, including the reference's behaviour at an lr
decay: its "reload of the best parameters" is a no-op because bestParams aliases the live tensors, and so it is here by default
(--lr_reload clone really rolls back, and then also resets Adam's moments)); every OCflow call --
forward, Jc.backward(), validation -- runs in the HIP kernels.  No plotting (viz_freq is accepted and ignored).

One GPU:   python trainOC.py --data softcorridor --niters 200
N GPUs:    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 trainOC.py ...
           (one rank per GPU; each rank draws n_train/N samples; the 8 cost sums and one flat gradient buffer are
           all-reduced over RCCL per iteration, so every rank takes the same Adam step).

--noise_rng counter (addition, with --noise): the disturbances come from the counter-based generator inside the kernels
(seed = noise_seed << 32 | iteration, row = the sample's global row), so the run does not depend on the number of ranks.
--noise SIGMA [--noise_seed S] (addition): the training rollouts run under per-step Brownian state disturbances sigma dB
(neuraloc_amd.disturbed_ocflow_train), a fresh W every iteration; validation and its logged costs stay undisturbed.
SIGMA = 0 (default) is the run without the flag.
--adv EPS [--adv_mode free|pgd] [--adv_steps K] [--adv_objective Jc|control] (addition): min-max training against the worst per-step state
disturbance in the ball ||W_i||_2 <= EPS over every start's [nt, d] path.  free (default): one W per rank persists
across the iterations on a batch -- zero at the start and whenever the batch is resampled -- and takes one projected ascent step of length
2.5 EPS / K per Adam step, from the same backward that gives the parameter gradients (neuraloc_amd.adversarial_step).  pgd: every iteration
runs a K-step search from zero first (neuraloc_amd.pgd_ocflow_train), on the training loss (Jc) or on L + alph0 G (control).  Validation stays
undisturbed.  EPS = 0 (default) is the run without the flag.
--members E [--members_alph FILE] (addition): E networks of the run's shape trained in ONE process, one launch per rollout and per adjoint
for all of them (neuraloc_amd.ensemble).  Member e is the network the run with --seed SEED+e builds; all members see
member 0's batches.  FILE: E lines of six comma-separated multipliers, one member each (default: every member uses --alph).  One log line per
member and iteration, the usual line prefixed by "m<e>"; one checkpoint per member in the reference's layout, ..._m<e>_checkpt.pth, each
keeping that member's own best.  The small-network shapes only; not with --prec double, --noise, --adv, --resume or more than one rank.
--members_family mid (addition, with --members): the ensemble runs on the one-CU kernels instead: 32 < m <= 128,
d + 1 <= 32, every problem class -- --data singlequad, and --m 64 / 128 on the point-agent problems.  The default, lane, is the above.
--members_sigma S0,S1,... [--noise_seed S] (addition, with --members): E noise levels >= 0, one per member -- a sweep over the noise level in
one process.  Member e trains under per-step Brownian state disturbances sigma_e dB drawn inside the kernels
(neuraloc_amd.ensemble_noisy_ocflow_train), one launch per rollout and per adjoint for all members, on either family.
The seed is noise_seed << 32 | iteration for ALL members (the --noise_rng counter convention, 0 <= noise_seed < 2**32): every member meets
the same noise realisations scaled by its own level, so the members' costs are a paired comparison across sigma.  A level of 0 is the
undisturbed member; validation stays undisturbed.  --members with --noise stays refused: this flag is the way in.
--noise_rho RHO (addition, with --noise SIGMA): the disturbances are correlated in time -- an AR(1) / Ornstein-Uhlenbeck path per sample and
component with lag-one correlation 0 < RHO < 1 and the white noise's variance at every step.  --noise_rng counter:
drawn inside the kernels (neuraloc_amd.noisy_ocflow_train(..., rho=RHO)); --noise_rng torch: neuraloc_amd.brownian_disturbances(..., rho=RHO).
The default 0 is the white noise of --noise.  --risk takes it; not with --members, --adv or --prec double.
--risk cvar|entropic --risk_level A [--risk_paths R] [--risk_mix M] (addition, with --noise SIGMA --noise_rng counter): risk-sensitive
training (neuraloc_amd.risk_ocflow_train).  Every training batch is repeated R times (repeat_interleave: R noise paths
per start) and the objective is the risk of each start's R costs -- CVaR at level A, or the entropic risk with theta = A -- blended with their
mean by M; its exact gradient comes from one weighted adjoint launch.  The loss column carries the risk's value; validation stays undisturbed
and averaged.  Single precision, one rank; not with --members or --adv.
--members_risk cvar|entropic|mean --members_risk_level A | A0,A1,... [--members_risk_paths R] [--members_risk_mix M] (addition, with --members E
--members_sigma ...): a sweep over the risk level in one process (neuraloc_amd.ensemble_risk_ocflow_train).  Every
training batch is repeated R times (default 8) for every member, member e's objective is the risk of each start's R costs at ITS level -- one
level per member, or one for all -- and all members' exact gradients come from ONE weighted ensemble adjoint launch.  The seed is
noise_seed << 32 | iteration for all members; the loss column carries each member's risk value; validation stays undisturbed and averaged;
one checkpoint per member as with --members.  --risk with --members stays refused: this flag is the way in.
--members_adv EPS0,EPS1,... [--adv_steps K] (addition, with --members): E adversary budgets >= 0, one per member -- a sweep over the budget in
one process (neuraloc_amd.ensemble_adversarial_step).  Free-mode min-max training: one W [E, nt, n, d] persists across
the iterations on a batch -- zero at the start and whenever the batch is resampled -- and per Adam step member e's slice takes one projected
ascent step of length 2.5 EPS_e / K inside its ball ||W_i||_2 <= EPS_e, from the same joint ensemble adjoint launch that gives all members'
parameter gradients: three launches per iteration for all members, on either family.  A budget of 0 is the undisturbed member; validation stays
undisturbed; one log line and one checkpoint per member as with --members.  Not with --members_sigma, --members_risk, --noise or --adv:
--members with --adv stays refused, this flag is the way in."""
import argparse
import datetime
import os
import time

import torch

import neuraloc_amd as na
from neuraloc_amd.checkpoint import save_checkpoint
from neuraloc_amd.initProb import PROBLEM_NAMES, initProb, resample


# (flag, type, default, note) -- names and defaults are the reference driver's (trainOC.py:22-63); notes are ours
_FLAGS = [
    ("data", str, "softcorridor", "problem name"),
    ("nt", int, 20, "RK4 steps while training"),
    ("nt_val", int, 32, "RK4 steps in validation plots (kept for compatibility)"),
    ("alph", str, "100.0, 10000.0, 300.0, 0.2, 0.2, 0.2", "weights of G, Q, W, HJt, HJfin, HJgrad"),
    ("m", int, 32, "width of Phi"),
    ("nTh", int, 2, "depth of Phi"),
    ("niters", int, 1800, "Adam iterations"),
    ("lr", float, 0.01, "learning rate"),
    ("optim", str, "adam", "only adam"),
    ("weight_decay", float, 0.0, ""),
    ("resume", str, None, "checkpoint to continue from"),
    ("save", str, "experiments/oc/run", "output directory"),
    ("gpu", int, 0, "device index of a single-process run"),
    ("prec", str, "single", "single or double (trainOC.py:44,76-79): double runs the whole training -- rollout, adjoint, Adam -- in float64"),
    ("approach", str, "ocflow", ""),
    ("lr_reload", str, "alias", "(addition) alias: the reference's behaviour (its reload at lr_freq is a no-op); clone: really roll back to the best validated parameters and reset Adam's moments"),
    ("viz_freq", int, 100, "ignored: nothing is plotted"),
    ("val_freq", int, 25, "validate every this many iterations"),
    ("log_freq", int, 1, "print every this many iterations"),
    ("lr_freq", int, 600, "decay the learning rate every this many iterations"),
    ("lr_decay", float, 0.1, "decay factor"),
    ("n_train", int, 1024, "GLOBAL batch size"),
    ("var0", float, 1.0, "scale of rho_0"),
    ("sample_freq", int, 100, "draw a new batch every this many iterations"),
    ("new_alph", str, None, "'iter, a0, ..., a5': switch the weights at that iteration"),
    ("seed", int, None, "torch seed (rank is added); the reference is unseeded"),
    ("noise", float, 0.0, "(addition) SIGMA > 0: train on rollouts under Brownian state disturbances sigma dB at every step "
                          "(neuraloc_amd.disturbed_ocflow_train); validation stays undisturbed; single precision only"),
    ("noise_seed", int, 0, "(addition) seed of the disturbances for --noise (rank is added)"),
    ("noise_rng", str, "torch", "(addition) torch: every rank draws its shard's disturbances with torch.randn; counter: they are drawn inside "
                                "the kernels from (noise_seed, iteration, global row) (neuraloc_amd.noisy_ocflow_train), the same on any number of ranks"),
    ("noise_rho", float, 0.0, "(addition, with --noise) 0 <= RHO < 1: time-correlated (Ornstein-Uhlenbeck) disturbances of lag-one correlation RHO "
                              "(neuraloc_amd.noisy_ocflow_train / brownian_disturbances with rho=RHO); 0: the white noise of --noise"),
    ("adv", float, 0.0, "(addition) EPS > 0: min-max training against the worst disturbance path of norm <= EPS per start "
                        "(neuraloc_amd.adversarial_step / pgd_ocflow_train); validation stays undisturbed; single precision only; not with --noise"),
    ("adv_mode", str, "free", "(addition) free: one persistent W per rank, one ascent step per Adam step from the joint adjoint; "
                              "pgd: a K-step search from zero in front of every iteration"),
    ("adv_steps", int, 4, "(addition) K: free mode takes ascent steps of length 2.5 EPS / K; pgd mode runs K inner steps"),
    ("adv_objective", str, "Jc", "(addition, pgd only) what the adversary climbs: Jc (the training loss) or control (L + alph0 G)"),
    ("members", int, None, "(addition) E >= 1: train E networks of this shape in one process, one launch per rollout for all of them "
                        "(neuraloc_amd.ensemble); member e is seeded --seed + e; single precision, one rank, the small-network shapes only"),
    ("members_alph", str, None, "(addition, with --members) file of E lines of six comma-separated multipliers, one member each (default: --alph)"),
    ("members_family", str, "lane", "(addition, with --members) lane: the small-network lane kernels; mid: the one-CU kernels "
                                    "(32 < m <= 128, d + 1 <= 32, every problem class, singlequad among them)"),
    ("members_sigma", str, None, "(addition, with --members) S0,S1,...: E noise levels >= 0, member e trains under Brownian state disturbances "
                                 "sigma_e dB drawn inside the kernels (neuraloc_amd.ensemble_noisy_ocflow_train), all members under the seed "
                                 "noise_seed << 32 | iteration; validation stays undisturbed"),
    ("members_risk", str, None, "(addition, with --members E --members_sigma ...) cvar, entropic or mean: every member trains on that risk measure "
                                "of each start's costs over --members_risk_paths noise paths (neuraloc_amd.ensemble_risk_ocflow_train)"),
    ("members_risk_level", str, None, "(addition, with --members_risk) A or A0,A1,...: one level for all members or one per member (cvar: "
                                      "0 <= A < 1; entropic: theta > 0)"),
    ("members_risk_paths", int, 8, "(addition, with --members_risk) R >= 1 noise paths per start: every batch is repeated R times per member"),
    ("members_risk_mix", float, 1.0, "(addition, with --members_risk) 0 <= M <= 1: every member's objective is (1 - M) mean + M risk"),
    ("members_adv", str, None, "(addition, with --members) EPS0,EPS1,...: E adversary budgets >= 0, member e trains against the worst "
                               "disturbance path of norm <= EPS_e per start (neuraloc_amd.ensemble_adversarial_step, free mode; --adv_steps K)"),
    ("risk", str, None, "(addition, with --noise SIGMA --noise_rng counter) cvar or entropic: train on a risk measure of each start's costs over "
                        "--risk_paths noise paths (neuraloc_amd.risk_ocflow_train) instead of their mean"),
    ("risk_level", float, None, "(addition, with --risk) cvar: the level 0 <= A < 1 (the mean of the worst (1 - A) share); entropic: theta > 0"),
    ("risk_paths", int, 8, "(addition, with --risk) R >= 1 noise paths per start: every batch is repeated R times"),
    ("risk_mix", float, 1.0, "(addition, with --risk) 0 <= M <= 1: the objective is (1 - M) mean + M risk"),
]
_CHOICES = {"data": PROBLEM_NAMES, "optim": ["adam"], "prec": ["single", "double"], "approach": ["ocflow"], "noise_rng": ["torch", "counter"],
            "adv_mode": ["free", "pgd"], "risk": ["cvar", "entropic"], "members_risk": list(na.risk.RISKS), "adv_objective": ["Jc", "control"], "members_family": list(na.ensemble.FAMILIES)}


def parse_args(argv=None):
    p = argparse.ArgumentParser("Optimal Control (MI355X)")
    for name, typ, dflt, note in _FLAGS:
        p.add_argument("--" + name, type=typ, default=dflt, help=note or None, choices=_CHOICES.get(name))
    a = p.parse_args(argv)
    a.alph = [float(v) for v in a.alph.split(",")]
    if a.new_alph is not None:
        a.new_alph = [float(v) for v in a.new_alph.split(",")]
    noise_rho_refusals(a)
    return a


def noise_rho_refusals(args):
    """--noise_rho: everything the time-correlated noise does not take, refused by the parser itself"""
    if args.noise_rho == 0:
        return
    if not 0.0 <= args.noise_rho < 1.0:                    # (a NaN fails both comparisons)
        raise SystemExit("--noise_rho RHO must be a number with 0 <= RHO < 1")
    if not args.noise > 0:
        raise SystemExit("--noise_rho needs --noise SIGMA > 0: it shapes that noise in time")
    if args.members is not None or args.members_alph is not None or args.members_family != "lane" or args.members_sigma is not None \
            or args.members_risk is not None or args.members_risk_level is not None or args.members_adv is not None:
        raise SystemExit("--noise_rho excludes --members: the time-correlated noise takes one network")
    if args.adv > 0:
        raise SystemExit("--noise_rho excludes --adv: one disturbance per rollout")
    if args.prec == "double":
        raise SystemExit("--noise_rho runs in single precision only (the double-precision rollout takes no disturbance)")


def _level_in_range(risk, level):
    """the range of a risk's level: cvar 0 <= A < 1, entropic a finite theta > 0 (the mean reads none)"""
    if risk == "cvar":
        return 0.0 <= level < 1.0
    if risk == "entropic":
        return 0.0 < level < float("inf")
    return True


def risk_refusals(args, world):
    """--risk: everything the risk-sensitive run does not take, refused before anything runs or is written"""
    if args.risk is None:
        if args.risk_level is not None:
            raise SystemExit("--risk_level needs --risk cvar|entropic")
        return
    if args.prec == "double":
        raise SystemExit("--risk runs in single precision only (the weighted adjoint takes no float64)")
    if not args.noise > 0:
        raise SystemExit("--risk needs --noise SIGMA > 0 (with --noise_rng counter): the risk is taken over each start's noise paths")
    if args.noise_rng != "counter":
        raise SystemExit("--risk needs --noise_rng counter, not --noise_rng torch: the paths' disturbances are drawn inside the kernels")
    if args.members is not None or args.members_alph is not None or args.members_family != "lane" or args.members_sigma is not None:
        raise SystemExit("--risk excludes --members: the weighted adjoint takes one network")
    if args.adv > 0:
        raise SystemExit("--risk excludes --adv: dJ/dW together with weights is not supported")
    if world > 1:
        raise SystemExit("--risk runs on one rank (one GPU): sharded batches are not supported")
    if args.risk_level is None:
        raise SystemExit("--risk needs --risk_level A")
    if args.risk == "cvar" and not _level_in_range("cvar", args.risk_level):
        raise SystemExit("--risk cvar needs 0 <= --risk_level < 1")
    if args.risk == "entropic" and not _level_in_range("entropic", args.risk_level):
        raise SystemExit("--risk entropic needs a finite --risk_level (theta) > 0")
    if args.risk_paths < 1:
        raise SystemExit("--risk_paths R must be >= 1")
    if not 0.0 <= args.risk_mix <= 1.0:
        raise SystemExit("--risk_mix M must lie in [0, 1]")


def members_refusals(args, world):
    """--members: everything the ensemble run does not take, refused before anything runs or is written.  -> the members' multipliers"""
    if args.members is None or args.members < 1:
        raise SystemExit("--members E must be >= 1 (--members_alph needs --members)")
    if args.prec == "double":
        raise SystemExit("--members runs in single precision only (the double-precision kernels take one network)")
    if args.noise > 0 or args.adv > 0:
        raise SystemExit("--members excludes --noise and --adv: the disturbed rollouts take one network")
    if world > 1:
        raise SystemExit("--members runs on one rank (one GPU)")
    if args.resume is not None:
        raise SystemExit("--members does not take --resume: a checkpoint holds one network")
    if args.lr_reload == "clone":
        raise SystemExit("--members keeps the reference's --lr_reload alias only")
    mid = args.members_family == "mid"
    if args.data not in PROBLEM_NAMES or (args.data == "singlequad" and not mid):
        raise SystemExit("--members takes the point-agent problems only")
    if len(args.alph) < 6:
        raise SystemExit("--alph needs 6 entries")
    rows = [list(args.alph[:6])] * args.members
    if args.members_alph is not None:
        with open(args.members_alph) as f:
            rows = [[float(v) for v in ln.split(",")] for ln in f if ln.strip()]
        if len(rows) != args.members or any(len(r_) != 6 for r_ in rows):
            raise SystemExit("--members_alph: the file must hold --members lines of six comma-separated multipliers")
    # the shape, known without a device: the ensemble runs on the small-network kernels, whose adjoint takes Cross2D agents (ensemble.LANE_LIMITS)
    prob, x0, _x0v, _xInit = initProb(args.data, 1, 1, var0=args.var0, alph=args.alph, cvt=lambda t: t.float())
    d = x0.size(1)
    if mid:
        # (the one-CU kernels and their adjoint: ensemble.MID_LIMITS; Phi's default rank of A is min(10, d + 1))
        if not na.ensemble._mid_eligible(args.nTh, args.m, d, min(10, d + 1), int(prob.nAgents), train=True):
            raise SystemExit("--members --members_family mid: {:} with m={:}, nTh={:} (d={:}) is outside the one-CU kernels this ensemble runs "
                             "on: {:}".format(args.data, args.m, args.nTh, d, na.ensemble.MID_LIMITS))
        return rows
    if not (args.nTh == 2 and 1 <= args.m <= 32 and d + 1 <= 32 and isinstance(prob, na.Cross2D) and prob.nAgents <= 16):
        raise SystemExit("--members: {:} with m={:}, nTh={:} (d={:}) is outside the small-network kernels an ensemble runs on: {:}, Cross2D "
                         "agents for training".format(args.data, args.m, args.nTh, d, na.ensemble.LANE_LIMITS))
    return rows


def members_sigma_levels(args):
    """--members_sigma: the members' noise levels, refused before anything runs or is written.  -> E floats, or None without the flag"""
    if args.members_sigma is None:
        return None
    if args.members is None or args.members < 1:
        raise SystemExit("--members_sigma needs --members E: one noise level per member")
    try:
        levels = [float(v) for v in args.members_sigma.split(",")]
    except ValueError:
        raise SystemExit("--members_sigma S0,S1,...: a comma-separated list of numbers, got {!r}".format(args.members_sigma))
    if len(levels) != args.members:
        raise SystemExit("--members_sigma needs one level per member: --members {:} but {:} values".format(args.members, len(levels)))
    if any(not 0 <= v < float("inf") for v in levels):
        raise SystemExit("--members_sigma: every level must be a finite number >= 0")
    if not 0 <= args.noise_seed < 2 ** 32:
        raise SystemExit("--members_sigma needs 0 <= --noise_seed < 2**32 (the iteration takes the seed's low word)")
    return levels


def members_risk_spec(args, sigmas):
    """--members_risk: the members' risk measure and levels, refused before anything runs or is written.
    -> (risk, E levels, paths, mix), or None without the flag"""
    if args.members_risk is None:
        if args.members_risk_level is not None:
            raise SystemExit("--members_risk_level needs --members_risk cvar|entropic|mean")
        return None
    if args.members is None or args.members < 1 or sigmas is None:
        raise SystemExit("--members_risk needs --members E --members_sigma S0,S1,...: the risk is taken over each start's noise paths")
    if args.members_risk_level is None:
        if args.members_risk != "mean":
            raise SystemExit("--members_risk needs --members_risk_level A or A0,A1,...")
        levels = [0.0]
    else:
        try:
            levels = [float(v) for v in args.members_risk_level.split(",")]
        except ValueError:
            raise SystemExit("--members_risk_level A or A0,A1,...: a number or a comma-separated list of numbers, got {!r}".format(
                args.members_risk_level))
    if len(levels) == 1:
        levels = levels * args.members
    if len(levels) != args.members:
        raise SystemExit("--members_risk_level needs one level for all members or one per member: --members {:} but {:} values".format(
            args.members, len(levels)))
    if args.members_risk == "cvar" and not all(_level_in_range("cvar", v) for v in levels):
        raise SystemExit("--members_risk cvar needs 0 <= --members_risk_level < 1 for every member")
    if args.members_risk == "entropic" and not all(_level_in_range("entropic", v) for v in levels):
        raise SystemExit("--members_risk entropic needs a finite --members_risk_level (theta) > 0 for every member")
    if args.members_risk_paths < 1:
        raise SystemExit("--members_risk_paths R must be >= 1")
    if not 0.0 <= args.members_risk_mix <= 1.0:
        raise SystemExit("--members_risk_mix M must lie in [0, 1]")
    return args.members_risk, levels, args.members_risk_paths, args.members_risk_mix


def members_adv_budgets(args, sigmas, mrisk):
    """--members_adv: the members' adversary budgets, refused before anything runs or is written.  -> E floats, or None without the flag"""
    if args.members_adv is None:
        return None
    if args.members is None or args.members < 1:
        raise SystemExit("--members_adv needs --members E: one adversary budget per member")
    try:
        budgets = [float(v) for v in args.members_adv.split(",")]
    except ValueError:
        raise SystemExit("--members_adv EPS0,EPS1,...: a comma-separated list of numbers, got {!r}".format(args.members_adv))
    if len(budgets) != args.members:
        raise SystemExit("--members_adv needs one budget per member: --members {:} but {:} values".format(args.members, len(budgets)))
    if not all(v >= 0.0 and v != float("inf") for v in budgets):
        raise SystemExit("--members_adv: every budget must be a finite number >= 0")
    if sigmas is not None or mrisk is not None:
        raise SystemExit("--members_adv excludes --members_sigma and --members_risk: one disturbance per rollout, and dJ/dW together with "
                         "weights is not supported")
    if args.noise > 0 or args.adv > 0:
        raise SystemExit("--members_adv excludes --noise and --adv: the members' budgets are the disturbance of the run")
    if args.adv_steps < 1:
        raise SystemExit("--adv_steps K must be >= 1")
    return budgets


def train_members(args, rows, sigmas=None, mrisk=None, budgets=None):
    """the training loop of main() for E networks at once (neuraloc_amd.ensemble): same schedule, one log line and one checkpoint per member.
    sigmas (--members_sigma): member e's training rollouts run under Brownian disturbances of level sigmas[e].  mrisk (--members_risk, with
    sigmas): (risk, E levels, paths, mix) -- member e trains on that risk of each start's `paths` costs at its level.  budgets (--members_adv):
    member e trains against the worst disturbance of norm <= budgets[e] per start, free mode"""
    E = args.members
    dev = torch.device("cuda", args.gpu)
    assert torch.cuda.is_available(), "trainOC.py needs an MI355X: there is no CPU path"
    cvt = lambda t: t.float().to(dev)                                  # noqa: E731
    tspan = [0.0, 1.0]
    # member e: the network the single-network run with --seed SEED+e builds (its generator has drawn that run's batches first); the batches
    # and every later draw are member 0's, so member 0 of an ensemble run IS the single-network run with --seed SEED
    nets, state0 = [], None
    for e in range(E):
        if args.seed is not None:
            torch.manual_seed(args.seed + e)
        p_e, x0_e, x0v_e, xInit_e = initProb(args.data, args.n_train, args.n_train, var0=args.var0, alph=rows[e], cvt=cvt)
        nets.append(na.Phi(nTh=args.nTh, m=args.m, d=x0_e.size(1), alph=rows[e]))
        if e == 0:
            prob, x0, x0v, xInit = p_e, x0_e, x0v_e, xInit_e
            state0 = torch.get_rng_state()
    torch.set_rng_state(state0)
    d, m, nTh = x0.size(1), args.m, args.nTh
    ens = na.PhiEnsemble.from_members(nets, alph=rows).to(dev)
    optim = torch.optim.Adam(ens.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    stamp = datetime.datetime.now().strftime("%Y_%m_%d_%H_%M_%S")
    title = args.data + "_" + stamp + "_alph{:}_{:}_{:}_{:}_{:}_{:}_m{:}".format(*[int(v) for v in args.alph], m)
    print("DIMENSION={:}  m={:}  nTh={:}   members={:}".format(d, m, nTh, E))
    for e in range(E):
        print("m{:}  alpha={:}".format(e, rows[e]))
    print("nt={:}   nt_val={:}".format(args.nt, args.nt_val))
    print("Number of trainable parameters: {} per member".format(sum(p.numel() for p in ens.parameters() if p.requires_grad) // E))
    print("data={:} device={:} ranks=1".format(args.data, dev))
    print("n_train={:}".format(args.n_train))
    print("{:4s} {:5s} {:7s} {:6s}   {:9s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}     {:9s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}".format(
        "mem", "iter", "lr", "  time", "loss", "L", "G", "HJt", "HJfin", "HJgrad", "Q", "W",
        "valLoss", "valL", "valG", "valHJt", "valHJf", "valHJg", "valQ", "valW"))
    n_change = int(args.new_alph[0]) if args.new_alph is not None else -1
    best_loss, total = [float("inf")] * E, 0.0
    # --members_adv: one W for all members, kept across the iterations on a batch (zeroed with every new batch)
    adv_W = torch.zeros(E, args.nt, x0.shape[0], d, device=dev, requires_grad=True) if budgets is not None else None
    prob.train()
    end = time.time()
    for itr in range(1, args.niters + 1):
        optim.zero_grad()
        if mrisk is not None:                             # R noise paths per start and member, rows [i R, (i + 1) R) of every member's batch
            Jc, cs, _ = na.ensemble_risk_ocflow_train(x0.repeat_interleave(mrisk[2], 0), ens, prob, tspan, args.nt, mrisk[0], mrisk[1],
                                                      paths=mrisk[2], mix=mrisk[3], sigma=[[s_] for s_ in sigmas],
                                                      seed=(args.noise_seed << 32) | itr, stepper="rk4", family=args.members_family)
        elif adv_W is not None:                           # forward, joint adjoint (both gradients) and the members' ascent steps: three launches
            Jc, cs = na.ensemble_adversarial_step(x0, ens, prob, tspan, args.nt, adv_W, budgets, [2.5 * b_ / args.adv_steps for b_ in budgets],
                                                  stepper="rk4", family=args.members_family)
        elif sigmas is not None:                          # one seed for all members: the same noise realisations at E levels
            Jc, cs = na.ensemble_noisy_ocflow_train(x0, ens, prob, tspan, args.nt, [[s_] for s_ in sigmas], (args.noise_seed << 32) | itr,
                                                    "rk4", family=args.members_family)
        else:
            Jc, cs = na.ensemble_ocflow_train(x0, ens, prob, tspan, args.nt, "rk4", family=args.members_family)
        if adv_W is None:                                 # (upstream gradient 1 for every member: E independent gradients)
            Jc.sum().backward()
        torch.cuda.synchronize()
        optim.step()
        dt = time.time() - end
        total += dt
        Jh, ch = Jc.tolist(), cs.tolist()
        lines = ["m{:<3d} {:05d} {:7.1e} {:6.2f}   {:9.3e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}".format(
            e, itr, optim.param_groups[0]["lr"], dt, Jh[e], *ch[e]) for e in range(E)]
        if itr % args.val_freq == 0 or itr == args.niters:
            with torch.no_grad():
                prob.eval()
                vl, vcs = na.ensemble_rollout(x0v, ens, prob, tspan, args.nt, "rk4", family=args.members_family)
                vh, vch = vl.tolist(), vcs.tolist()
                for e in range(E):
                    lines[e] += "    {:9.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e} ".format(vh[e], *vch[e])
                    if vh[e] < best_loss[e]:
                        best_loss[e] = vh[e]
                        os.makedirs(args.save, exist_ok=True)
                        a_e = argparse.Namespace(**vars(args))
                        a_e.alph, a_e.member = list(rows[e]), e
                        torch.save({"args": a_e, "state_dict": {k: v.cpu() for k, v in ens.member_state_dict(e).items()}},
                                   os.path.join(args.save, title + "_m{:}_checkpt.pth".format(e)))
                prob.train()
        if itr % args.log_freq == 0:
            for ln in lines:
                print(ln)
        if itr % args.lr_freq == 0 and min(best_loss) < float("inf"):
            for g in optim.param_groups:                  # (--lr_reload alias, the reference's behaviour: no roll-back)
                g["lr"] *= args.lr_decay
        if itr % args.sample_freq == 0:
            x0 = resample(x0, xInit, args.var0, cvt)
            if adv_W is not None:
                with torch.no_grad():
                    adv_W.zero_()
        if itr == n_change:
            rows = [[r_[0]] + list(args.new_alph[2:4]) + list(r_[3:]) for r_ in rows]       # like main(): the Q / W weights change, the others stay
            ens.alph = [list(r_) for r_ in rows]
            print("alph values changed")
        end = time.time()
    print("Training Time: {:} seconds".format(total))
    print("Training has finished.  " + os.path.join(args.save, title))
    return best_loss


def main(argv=None):
    args = parse_args(argv)
    if args.noise < 0:
        raise SystemExit("--noise SIGMA must be >= 0")
    if args.noise > 0 and args.prec == "double":                       # refused before anything runs or is written
        raise SystemExit("--noise runs in single precision only (the double-precision rollout takes no disturbance)")
    if args.noise_rng == "counter" and args.prec == "double":
        raise SystemExit("--noise_rng counter runs in single precision only (the double-precision rollout takes no disturbance)")
    if args.noise_rng == "counter" and not 0 <= args.noise_seed < 2 ** 32:
        raise SystemExit("--noise_rng counter needs 0 <= --noise_seed < 2**32 (the iteration takes the seed's low word)")
    if not args.adv >= 0 or args.adv == float("inf"):
        raise SystemExit("--adv EPS must be a finite number >= 0")
    if args.adv > 0 and args.prec == "double":
        raise SystemExit("--adv runs in single precision only (the double-precision rollout takes no disturbance)")
    if args.adv > 0 and args.noise > 0:
        raise SystemExit("--adv and --noise exclude each other: one disturbance per rollout")
    if args.adv > 0 and args.adv_steps < 1:
        raise SystemExit("--adv_steps K must be >= 1")
    if args.adv > 0 and args.adv_mode == "free" and args.adv_objective == "control":
        raise SystemExit("--adv_objective control needs --adv_mode pgd: the free adversary climbs the training loss itself")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    risk_refusals(args, world)
    if args.members is not None or args.members_alph is not None or args.members_family != "lane" or args.members_sigma is not None \
            or args.members_risk is not None or args.members_risk_level is not None or args.members_adv is not None:
        sigmas = members_sigma_levels(args)
        mrisk = members_risk_spec(args, sigmas)
        budgets = members_adv_budgets(args, sigmas, mrisk)
        return train_members(args, members_refusals(args, world), sigmas, mrisk, budgets)
    if world > 1:
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
        dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("NOCF_TRAIN_BACKEND", "nccl")
        dist.init_process_group(backend, **({"device_id": dev} if backend == "nccl" else {}))
    else:
        dist = None
        dev = torch.device("cuda", args.gpu)
    assert torch.cuda.is_available(), "trainOC.py needs an MI355X: there is no CPU path"
    if args.seed is not None:
        torch.manual_seed(args.seed + rank)
    say = print if rank == 0 else (lambda *a, **k: None)
    n_change = int(args.new_alph[0]) if args.new_alph is not None else -1
    prec = torch.float64 if args.prec == "double" else torch.float32
    cvt = lambda t: t.to(prec).to(dev)                                 # noqa: E731
    lo, hi = na.shard_rows(args.n_train, rank, world)
    n_local = hi - lo
    alph = args.alph
    prob, x0, x0v, xInit = initProb(args.data, n_local, n_local, var0=args.var0, alph=alph, cvt=cvt)
    d, m, nTh, tspan = x0.size(1), args.m, args.nTh, [0.0, 1.0]
    net = na.Phi(nTh=nTh, m=m, d=d, alph=alph)
    if args.resume is not None:
        from neuraloc_amd.checkpoint import load_file
        ck = load_file(args.resume)
        m, nTh = ck["args"].m, ck["args"].nTh
        net = na.Phi(nTh=nTh, m=m, d=d, alph=alph)                      # alph from the command line wins (trainOC.py:129)
        net.load_state_dict(ck["state_dict"])
    net = net.to(prec).to(dev)
    if dist:                                                           # identical initial parameters on every rank
        for prm in net.parameters():
            dist.broadcast(prm.data, src=0)
    optim = torch.optim.Adam(net.parameters(), lr=args.lr, weight_decay=args.weight_decay)
    stamp = datetime.datetime.now().strftime("%Y_%m_%d_%H_%M_%S")
    title = args.data + "_" + stamp + "_alph{:}_{:}_{:}_{:}_{:}_{:}_m{:}".format(*[int(v) for v in alph], m)
    say("DIMENSION={:}  m={:}  nTh={:}   alpha={:}".format(d, m, nTh, alph))
    say("nt={:}   nt_val={:}".format(args.nt, args.nt_val))
    say("Number of trainable parameters: {}".format(sum(p.numel() for p in net.parameters() if p.requires_grad)))
    say("data={:} device={:} ranks={:}".format(args.data, dev, world))
    say("n_train={:}".format(args.n_train))
    say("{:5s} {:7s} {:6s}   {:9s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}     {:9s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}  {:8s}".format(
        "iter", "lr", "  time", "loss", "L", "G", "HJt", "HJfin", "HJgrad", "Q", "W",
        "valLoss", "valL", "valG", "valHJt", "valHJf", "valHJg", "valQ", "valW"))

    rollout = na.OCflow_sharded if dist else na.OCflow
    # --noise: every iteration draws its own W on the device; each rank its own shard's, from its own generator
    # --noise_rng counter: nothing is drawn -- the kernels form the disturbance of (iteration, global row, step, component) themselves
    noise_counter = args.noise > 0 and args.noise_rng == "counter"
    noise_gen = torch.Generator(device=dev).manual_seed(args.noise_seed + rank) if args.noise > 0 and not noise_counter else None
    # --adv, free mode: one W per rank, kept across the iterations on a batch (zeroed with every new batch)
    adv_W = torch.zeros(args.nt, x0.shape[0], d, device=dev, requires_grad=True) if args.adv > 0 and args.adv_mode == "free" else None
    rho_kw = {"rho": args.noise_rho} if args.noise_rho != 0 else {}     # --noise_rho 0: the white path and its entry points
    best_loss, best_params, total = float("inf"), None, 0.0
    net.train()
    prob.train()
    end = time.time()
    for itr in range(1, args.niters + 1):
        optim.zero_grad()
        if args.risk is not None:                         # R noise paths per start, rows [i R, (i + 1) R): the risk of each start's costs
            Jc, cs, _ = na.risk_ocflow_train(x0.repeat_interleave(args.risk_paths, 0), net, prob, tspan, args.nt, args.risk, args.risk_level,
                                             paths=args.risk_paths, mix=args.risk_mix, sigma=args.noise,
                                             seed=(args.noise_seed << 32) | itr, stepper="rk4", alph=net.alph, **rho_kw)
        elif noise_counter:
            Jc, cs = na.noisy_ocflow_train(x0, net, prob, tspan, args.nt, args.noise, (args.noise_seed << 32) | itr, "rk4", net.alph,
                                           row_offset=lo, group=True if dist else None, **rho_kw)
        elif noise_gen is not None:
            W = na.brownian_disturbances(args.nt, x0.shape[0], d, args.noise, tspan=tspan, generator=noise_gen, device=dev, **rho_kw)
            Jc, cs = na.disturbed_ocflow_train(x0, net, prob, tspan, args.nt, W, "rk4", net.alph, group=True if dist else None)
        elif adv_W is not None:
            Jc, cs = na.adversarial_step(x0, net, prob, tspan, args.nt, adv_W, args.adv, 2.5 * args.adv / args.adv_steps, stepper="rk4",
                                         alph=net.alph, group=True if dist else None)
        elif args.adv > 0:
            Jc, cs, _ = na.pgd_ocflow_train(x0, net, prob, tspan, args.nt, args.adv, args.adv_steps, objective=args.adv_objective,
                                            stepper="rk4", alph=net.alph, group=True if dist else None)
        else:
            Jc, cs = rollout(x0, net, prob, tspan, args.nt, "rk4", net.alph)
        if adv_W is None:                                 # (adversarial_step has run the backward: both gradients come from one adjoint)
            Jc.backward()
        torch.cuda.synchronize()
        na.check_errors()                                 # (after the synchronisation and BEFORE the step: a timed-out rollout raises, its NaN gradients are not applied)
        optim.step()
        dt = time.time() - end
        total += dt
        line = "{:05d} {:7.1e} {:6.2f}   {:9.3e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}".format(
            itr, optim.param_groups[0]["lr"], dt, Jc.item(), *[c.item() for c in cs])
        if itr % args.val_freq == 0 or itr == args.niters:
            with torch.no_grad():
                net.eval()
                prob.eval()
                vl, vcs = rollout(x0v, net, prob, tspan, args.nt, "rk4", net.alph)   # nt, not nt_val: trainOC.py:191
                line += "    {:9.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e}  {:8.2e} ".format(
                    vl.item(), *[c.item() for c in vcs])
                if vl.item() < best_loss:
                    best_loss = vl.item()
                    best_params = {k: v.detach().clone() for k, v in net.state_dict().items()}
                    if rank == 0:
                        os.makedirs(args.save, exist_ok=True)
                        save_checkpoint(os.path.join(args.save, title + "_checkpt.pth"), net, args)
                net.train()
                prob.train()
        if itr % args.log_freq == 0:
            say(line)
        if itr % args.lr_freq == 0 and best_params is not None:
            # In the reference, bestParams = net.state_dict() ALIASES the live tensors (trainOC.py:199), so its
            # load_state_dict(bestParams) at lr_freq (:250-253) is a no-op: the default here too (--lr_reload alias).  --lr_reload clone
            # rolls back to the best validated parameters for real; Adam's moments belong to the abandoned iterates and are reset.
            if args.lr_reload == "clone":
                net.load_state_dict(best_params)
                optim.state.clear()
            for g in optim.param_groups:
                g["lr"] *= args.lr_decay
        if itr % args.sample_freq == 0:
            x0 = resample(x0, xInit, args.var0, cvt)
            if adv_W is not None:
                with torch.no_grad():
                    adv_W.zero_()
        if itr == n_change:
            # like trainOC.py:258-263: the problem is rebuilt with the new Q/W weights; net.alph (what OCflow gets) stays
            alph = args.new_alph[1:]
            prob, _, _, _ = initProb(args.data, n_local, n_local, var0=args.var0, alph=alph, cvt=cvt)
            prob.train()
            say("alph values changed")
        end = time.time()
    say("Training Time: {:} seconds".format(total))
    say("Training has finished.  " + os.path.join(args.save, title))
    if dist:
        dist.barrier()
        dist.destroy_process_group()
    return best_loss


if __name__ == "__main__":
    main()
