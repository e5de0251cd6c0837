"""helpers of the ensemble tests (CPU only: nothing here touches a GPU)

An ensemble launch (neuraloc_amd/ensemble.py; csrc/nocf_lane.inc, csrc/nocf_lane_bwd.inc with ENS) is one batch of E * n rows on the lane
kernels, row g = sample g % n of member g // n.  Its yardstick is the single-network call on each member alone, bit for bit, so no oracle
and no tolerance appears here: this module holds the cases -- one per (MP, DP) instantiation for the forward and for the adjoint, at the
smallest shapes that can still go wrong -- and builds the members, the per-member problems and the starts of a case.

E = 3, n = 5: 15 rows in 4 workgroups of four waves, so workgroups 1 and 2 hold rows of two members and the last one a tail wave; nt = 2."""
import dataclasses

import torch

import util_lane as ul
from util_hip import closed_form_normal

E, N, NT = 3, 5, 2
# rows of six multipliers [G, Q, W, HJt, HJfin, HJgrad], one per member: all different, member 1 without interaction cost (alph_W = 0: the
# want_W branch differs between the members of one launch, and inside one workgroup).  Every value is a float32: the single-network call
# rounds its double alph_Q / alph_W to float32, the table holds float32
ALPH_ROWS = [[100.0, 50.0, 30.0, 0.5, 0.25, 0.125],
             [80.0, 20.0, 0.0, 1.0, 0.5, 0.25],
             [64.0, 12.5, 7.5, 0.25, 0.125, 0.5]]


@dataclasses.dataclass(frozen=True)
class EnsCase:
    base: ul.LaneCase
    own_x: bool                # every member its own starts ([E, n, d]) or one shared batch ([n, d])

    @property
    def id(self):
        b = self.base
        return f"{b.kind}{b.d}-m{b.m}-r{b.r}-{b.obstacle or 'free'}-{b.mode}-{b.stepper}-{'own' if self.own_x else 'shared'}"


def _C(own_x, kind, d, m, r, obstacle, mode, stepper):
    return EnsCase(ul._F(kind, d, m, r, obstacle, mode, N, stepper, NT), own_x)


# forward: one case per instantiation; rk4 on all but one, both modes, both problem classes, shared and own starts; d = 30 is 15 agents, whose
# pairs need the kernel's second trip
FORWARD = [
    _C(False, "cross2d", 4, 9, 5, "softcorridor", "train", "rk4"),       # (16, 8)
    _C(True, "swarm", 15, 16, 16, "blocks", "eval", "rk4"),             # (16, 16)
    _C(False, "cross2d", 16, 16, 16, None, "train", "rk1"),             # (16, 32)
    _C(True, "cross2d", 6, 31, 1, "softcorridor", "eval", "rk4"),       # (32, 8)
    _C(False, "cross2d", 14, 32, 15, "hardcorridor", "train", "rk4"),   # (32, 16)
    _C(True, "cross2d", 30, 32, 16, "softcorridor", "eval", "rk4"),     # (32, 32)
]

# training (the lane adjoint: Cross2D, train mode): one case per instantiation, every member its own starts so that x.grad is compared
TRAIN = [
    _C(True, "cross2d", 4, 9, 5, "softcorridor", "train", "rk4"),
    _C(True, "cross2d", 8, 16, 9, "hardcorridor", "train", "rk4"),
    _C(True, "cross2d", 16, 16, 16, None, "train", "rk1"),
    _C(True, "cross2d", 6, 31, 1, "softcorridor", "train", "rk4"),
    _C(True, "cross2d", 14, 32, 15, "hardcorridor", "train", "rk4"),
    _C(True, "cross2d", 30, 32, 16, "softcorridor", "train", "rk4"),
]


def member_case(case, e, rows=ALPH_ROWS):
    """the LaneCase of member e: its own seed (weights) and its own alph_Q / alph_W"""
    b = case.base
    return dataclasses.replace(b, seed=b.seed + 101 * (e + 1), alph_Q=rows[e % len(rows)][1], alph_W=rows[e % len(rows)][2])


def member_nets(case, device, members=E, first=0):
    """the members' networks as Phi: member e is the lane sweep's synthetic network of seed index first + e"""
    nets = [ul.make_net(member_case(case, first + e), device) for e in range(members)]
    for e, q in enumerate(nets):                     # (the synthetic c.bias is one constant: every member gets its own)
        q.c.bias.data.add_(0.03125 * (first + e))
    return nets


def member_rows(members=E, first=0):
    return [list(ALPH_ROWS[(first + e) % len(ALPH_ROWS)]) for e in range(members)]


def member_problem(case, e, device, first=0):
    """the problem the single-network leg of member e runs on: the case's, with that member's alph_Q / alph_W"""
    return ul.make_problem(member_case(case, first + e), device)


def starts(case, members=E, n=N, first=0):
    """[members, n, d] starts around the case's layout (CPU); a shared-x case uses block `first`"""
    xi, _ = ul.layout(case.base)
    d = case.base.d
    return torch.stack([(xi + ul.VAR0 * closed_form_normal(n, d, case.base.seed + 7 * (first + e))).contiguous() for e in range(members)])
