"""helpers of the one-CU ensemble tests (CPU only: nothing here touches a GPU)

An ensemble launch of the one-CU family (neuraloc_amd/ensemble.py with family="mid"; csrc/nocf_mono.inc, csrc/nocf_mono_bwd.inc with ENS) gives
member e the workgroups [e * tiles, (e + 1) * tiles) of one launch; every buffer is member-major.  Its yardstick is the single-network call on
each member alone, bit for bit, so no oracle and no tolerance appears here: this module holds the cases -- one per forward and per adjoint
instantiation, networks, problems and starts from tests/util_mono.py -- and a mirror of the family's eligibility.

E = 3, n = 17: two tiles per member, the second with one valid row and fifteen replicas of it, so every member boundary is a tile boundary
behind a tail; nt = 2."""
import dataclasses

import torch

import util_mono as um
from util_ensemble import ALPH_ROWS

E, N, NT = 3, 17, 2


def mid_eligible(nTh, m, d, r, n_agents, train=False):
    """family="mid" takes the shape: a one-CU plan exists (make_mono_plan); train: and an adjoint instantiation (nocf_mid_grad_rows != 0)"""
    kbd = um.cdiv(d + 1, 16)
    ok = nTh == 2 and 1 <= m <= 128 and d + 1 <= 32 and 1 <= r <= min(16, d + 1) and 1 <= n_agents <= (8 if kbd == 1 else 16)
    return ok and (m > 32 or not train)


@dataclasses.dataclass(frozen=True)
class MidCase:
    base: um.MonoCase
    own_x: bool                # every member its own starts ([E, n, d]) or one shared batch ([n, d])

    @property
    def id(self):
        b = self.base
        return f"{b.kind}{b.d}-m{b.m}-r{b.r}-{b.obstacle or 'free'}-{b.mode}-{b.stepper}-{'own' if self.own_x else 'shared'}"


def _C(own_x, kind, d, m, r, obstacle, mode, stepper, n=N, nt=NT, **kw):
    return MidCase(um.MonoCase(kind, d, m, r, obstacle, mode, n, stepper, nt, seed=d + 3 * m + r, **kw), own_x)


# forward: one case per (KBM, KBD) shape in util_mono.FORWARD_SHAPES' order, each run as evaluation and as recording forward; rk4 on all but one,
# both modes, all three problem classes, shared and own starts; (8, 1) is singlequad's shape, (8, 2) two quadcopters; widths in whole 16-blocks
# (an activation record is written) and not
FORWARD = [
    _C(False, "quad", 12, 128, 10, None, "eval", "rk4"),                # (8, 1)
    _C(True, "swarm", 15, 96, 16, "blocks", "train", "rk4"),            # (6, 1)
    _C(False, "cross2d", 14, 64, 10, "hardcorridor", "train", "rk1"),   # (4, 1)
    _C(True, "quad", 12, 32, 10, None, "eval", "rk4"),                  # (2, 1): the quadcopter's alone (point agents of m <= 32: lane kernel)
    _C(False, "quad", 24, 128, 10, None, "train", "rk4"),               # (8, 2)
    _C(True, "cross2d", 30, 65, 1, "hardcorridor", "eval", "rk4"),      # (6, 2)
    _C(False, "swarm", 30, 48, 16, "blocks", "train", "rk4"),           # (4, 2)
]

# training (train mode): one case per adjoint instantiation in util_mono.ADJOINT_SHAPES' order, every member its own starts so that x.grad is
# compared; widths with m % 16 == 0 (the adjoint reads the record) and without (it recomputes)
TRAIN = [
    _C(True, "quad", 12, 128, 10, None, "train", "rk4"),                # (8, 1), record
    _C(True, "cross2d", 14, 81, 15, "softcorridor", "train", "rk4"),    # (6, 1), recompute
    _C(True, "swarm", 15, 64, 16, "blocks", "train", "rk1"),            # (4, 1), record
    _C(True, "quad", 24, 127, 10, None, "train", "rk4"),                # (8, 2), recompute
    _C(True, "cross2d", 24, 96, 10, "softcorridor", "train", "rk4"),    # (6, 2), record
    _C(True, "cross2d", 16, 33, 1, "hardcorridor", "train", "rk4"),     # (4, 2), recompute
]

# the capped adjoint grid: more than 1024 tiles per member, so a workgroup walks tiles j, j + 1024, ... under a member offset; the cheapest
# adjoint shape
CAPPED = _C(False, "cross2d", 14, 48, 10, "hardcorridor", "train", "rk1", n=um.BIG, nt=1)


def member_case(case, e, rows=ALPH_ROWS):
    """the MonoCase of member e: its own seed (weights) and its own alph_Q / alph_W"""
    b = case.base
    return dataclasses.replace(b, seed=b.seed + 101 * (e + 1), alph_Q=rows[e % len(rows)][1], alph_W=rows[e % len(rows)][2])


def member_nets(case, device, members=E, first=0):
    """the members' networks as Phi: member e is the one-CU sweep's synthetic network of seed index first + e"""
    nets = [um.make_net(member_case(case, first + e), device) for e in range(members)]
    for e, q in enumerate(nets):                     # (the synthetic c.bias is one constant: every member gets its own)
        q.c.bias.data.add_(0.03125 * (first + e))
    return nets


def member_rows(members=E, first=0):
    return [list(ALPH_ROWS[(first + e) % len(ALPH_ROWS)]) for e in range(members)]


def member_problem(case, e, device, first=0):
    """the problem the single-network leg of member e runs on: the case's, with that member's alph_Q / alph_W"""
    return um.make_problem(member_case(case, first + e), device)


def starts(case, members=E, n=None, first=0):
    """[members, n, d] starts around the case's layout (CPU), util_mono.candidates with one draw per member; a shared-x case uses block `first`"""
    n = case.base.n if n is None else n
    return torch.stack([um.candidates(dataclasses.replace(case.base, draw=7 * (first + e)), n) for e in range(members)])
