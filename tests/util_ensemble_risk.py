"""helpers of the risk-sensitive ensembles' tests (CPU only: nothing here touches a GPU)

The weighted ensemble adjoints (neuraloc_amd/ensemble_risk.py; csrc/nocf_lane_bwd.inc and csrc/nocf_mono_bwd.inc with ENS and RW) read one
weight per row of every member.  Their yardstick is the single-network weighted call (weighted_ocflow_train / risk_ocflow_train, held to the
fp64 oracle by tests/test_risk_gpu.py) on each member alone, bit for bit, so no oracle and no tolerance appears here: this module takes the
cases of tests/util_ensemble_noise.py -- one per adjoint instantiation of both families, each with its sigma rows, seeds, row offset and mask
-- and adds the weights, the risk shapes and the members' risk measures.

given weights   the lists' own shapes, E = 3, nt = 2: lane n = 5 (15 rows in 4 workgroups of four waves: workgroups 1 and 2 hold rows of two
                members, the last one a tail wave); one-CU n = 17 (two tiles per member, the second with one valid row)
risk            E = 3, paths = 3: lane n = 6 (18 rows in 5 workgroups: workgroup 1 holds rows of members 0 and 1, the last one two tail waves);
                one-CU n = 18 (the group of rows 15 .. 17 lies across the tile boundary, the tail tile has 2 valid rows)"""
import dataclasses

import torch

import util_ensemble_noise as uen
import util_ensemble_mid as uem

E = uen.E
GIVEN = list(uen.TRAIN)                                             # 6 lane + 6 one-CU: every adjoint instantiation once

PATHS = 3
RISK_N = {"lane": 6, "mid": 18}
# the members' noise levels in the risk cases.  Member 0 runs undisturbed: the three paths of each of its starts are the same row three
# times, so every group of member 0 is a three-way TIE at the CVaR boundary.  Both legs -- the ensemble call and the single-network call --
# order the group with the same stable sort (risk._group_risk), so the tie falls the same way and the bits still agree
RISK_SIGMA = [[0.0], [0.1], [0.3]]
# (risk, level, mix) per member; the entropic theta (None here) is set from the member's own costs: theta_of
RISK_SPECS = [("cvar", 0.5, 1.0),          # k = (1 - 0.5) * 3 = 1.5: one whole row and a fractional boundary row
              ("entropic", None, 1.0),
              ("cvar", 0.0, 0.5)]           # level 0 is the mean; blended with the mean
# the smallest and the largest instantiation of each family: lane (MP, DP) = (16, 8) and (32, 32); one-CU (KBM, KBD) = (4, 1) and (8, 2)
RISK_SHAPES = {"lane": [(16, 8), (32, 32)], "mid": [(4, 1), (8, 2)]}
RISK = [c for c in GIVEN if c.base.shape in RISK_SHAPES[c.family]]
CAPPED = uen.NoiseCase("mid", uem.CAPPED, 0, 0, False)             # n = 16385, nt = 1, rk1: a workgroup walks tiles j, j + 1024
CAPPED_E = 2


def member_weights(seed, n):
    """[n] float32 weights in the manner of util_risk.case_weights: both signs, one exact zero, magnitudes over a range of about 100, of
    the order of 1 / n"""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (2.0 * torch.rand(n, generator=g, dtype=torch.float64) - 2.0)          # 0.01 ... 1
    sgn = torch.where(torch.rand(n, generator=g, dtype=torch.float64) < 0.3, -1.0, 1.0)
    w = mag * sgn
    if n > 1:
        w[0], w[n - 1] = 1.0, -0.01                                                      # (the range's ends and both signs, whatever the draw)
    w[n // 2] = 0.0
    return (w / n).to(torch.float32)


def weights(nc, members=E, n=None):
    """[members, n] float32: member e's row drawn from its own seed, so the rows differ"""
    n = nc.base.n if n is None else n
    return torch.stack([member_weights(104729 * nc.base.seed + 17 * n + 5 + 7919 * (e + 1), n) for e in range(members)]).contiguous()


def risk_starts(nc, members=E):
    """[members, n, d] with n = RISK_N[family]: n / PATHS starts per member, each repeated PATHS times (repeat_interleave's layout)"""
    n = RISK_N[nc.family]
    return nc.util.starts(nc.case, members, n=n // PATHS).repeat_interleave(PATHS, dim=1).contiguous()


def theta_of(persample, alph_row, paths=PATHS):
    """the entropic level of a member as util_risk sets it: 2 / (the mean over the groups of max - min of the member's costs), from the
    member's [n, 7] table of an evaluation rollout -> a Python float"""
    a = [float(v) for v in alph_row]
    J = (persample[:, 0] + a[0] * persample[:, 1] + a[3] * persample[:, 2] + a[4] * persample[:, 3] + a[5] * persample[:, 4]).double()
    Jg = J.reshape(-1, paths)
    return 2.0 / float((Jg.max(1).values - Jg.min(1).values).mean())


def lane_workgroups(members, n):
    """the members each workgroup of the lane launch holds rows of, and the number of tail waves of the last one"""
    rows = members * n
    groups = [sorted({g // n for g in range(4 * j, min(4 * j + 4, rows))}) for j in range((rows + 3) // 4)]
    return groups, 4 * len(groups) - rows


def mid_tiles(n):
    """(tiles per member, valid rows of the last tile)"""
    return (n + 15) // 16, n - 16 * ((n + 15) // 16 - 1)


def with_sigma(nc, isigma):
    return dataclasses.replace(nc, isigma=isigma)
