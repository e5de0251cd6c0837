"""helpers of the adversarial-ensemble tests (CPU only: nothing here touches a GPU)

A disturbed ensemble launch (neuraloc_amd/ensemble_minmax.py; csrc/nocf_lane.inc and csrc/nocf_mono.inc with ENS and DIST == 1, the adjoints
with ENS and STATES == 1 / 2) is the ensemble launch under a tensor disturbance W [E, nt, n, d], member e's slice being the W of its
single-network call.  The yardstick is disturbed_rollout / minmax_ocflow_train / disturbance_gradient / ascend_disturbances /
worst_case_disturbances on each member alone with its slice, on the same kernel family, bit for bit: no oracle and no tolerance appears here.
This module holds the case lists -- the undisturbed ensembles' unchanged (tests/util_ensemble.py: E = 3, n = 5, nt = 2, a workgroup holds rows
of two members and there is a tail wave; tests/util_ensemble_mid.py: E = 3, n = 17, the last tile of a member has one valid row), every second
case with every third coordinate masked out -- and draws the disturbances."""
import dataclasses

import torch

import util_ensemble as ue
import util_ensemble_mid as uem

E = 3
assert ue.E == E and uem.E == E
SCALE = 0.05                   # the magnitude of W: comparable to the states' step at nt = 2
GJ = [1.0, 0.5, -2.0]          # the upstream gradient of the members' Jc
EPS = [0.0, 0.1, 0.3]          # the search's radii: member 0 may not move


def mask_of(d):
    """every third coordinate is not disturbed"""
    return [0.0 if i % 3 == 1 else 1.0 for i in range(d)]


@dataclasses.dataclass(frozen=True)
class AdvCase:
    family: str                # "lane" / "mid"
    case: object               # util_ensemble.EnsCase / util_ensemble_mid.MidCase
    index: int                 # position in its list: the seed of its disturbances
    masked: bool

    @property
    def base(self):
        return self.case.base

    @property
    def own_x(self):
        return self.case.own_x

    @property
    def util(self):
        return ue if self.family == "lane" else uem

    @property
    def mask(self):
        return mask_of(self.base.d) if self.masked else None

    @property
    def id(self):
        return f"{self.family}-{self.case.id}{'-mask' if self.masked else ''}"


def _cases(family, cases, shift):
    return [AdvCase(family, c, i, (i + shift) % 2 == 1) for i, c in enumerate(cases)]


# evaluation / recording forward (FORWARD) and the adjoints (TRAIN): every case of the undisturbed ensembles' lists, both families
FORWARD = _cases("lane", ue.FORWARD, 0) + _cases("mid", uem.FORWARD, 1)
TRAIN = _cases("lane", ue.TRAIN, 1) + _cases("mid", uem.TRAIN, 0)


def disturbance(ac, members=E, salt=0):
    """W [members, nt, n, d] (CPU, float32): member e's slice from its own generator seed, SCALE * randn, masked coordinates exactly 0"""
    b = ac.base
    out = []
    for e in range(members):
        g = torch.Generator().manual_seed(7919 * (ac.index + 1) + 104729 * (e + 1) + 31 * salt + (0 if ac.family == "lane" else 1))
        out.append(SCALE * torch.randn(b.nt, b.n, b.d, generator=g, dtype=torch.float32))
    W = torch.stack(out)
    if ac.masked:
        W = W * torch.tensor(ac.mask)
    return W.contiguous()


def first(cases, family, **want):
    """the first case of a family with the given properties (own_x, masked)"""
    return next(c for c in cases if c.family == family and all(getattr(c, k) == v for k, v in want.items()))
