"""helpers of the noisy-ensemble tests (CPU only: nothing here touches a GPU)

A noisy ensemble launch (neuraloc_amd/ensemble_noise.py; csrc/nocf_lane.inc and csrc/nocf_mono.inc with ENS and DIST == 2) is the ensemble
launch with the Brownian disturbance drawn inside the kernel, member e at its own level and seed, the key of a row its index inside the
member.  Its yardstick is noisy_rollout / noisy_ocflow_train on each member alone, bit for bit, so no oracle and no tolerance appears here:
this module holds the sigma rows, the seeds, the row offsets and the case lists -- the undisturbed ensembles' (tests/util_ensemble.py: E = 3,
n = 5, nt = 2, a workgroup holds rows of two members and there is a tail wave; tests/util_ensemble_mid.py: E = 3, n = 17, the last tile of a
member has one valid row), each with one sigma row, one row offset and, every second case, a mask."""
import dataclasses

import util_ensemble as ue
import util_ensemble_mid as uem

E = 3
assert ue.E == E and uem.E == E

# one seed for all members (shared-x cases); one per member (own-x cases): a small one, one with the top bit set, the largest
SEED_SHARED = 0x243F6A8885A308D3
SEEDS_OWN = [3, 2 ** 63 + 5, 2 ** 64 - 1]
# the key of a member's row 0; the last one uses the counter's high word
ROW_OFFSETS = [0, 7, 2 ** 32 + 3]


def sigma_rows(d):
    """the three sigma arguments, each a level per member: [E, 1] with three different levels; [E, 1] with member 1 at 0; [E, d] with unequal
    components"""
    table = [[0.02 * (e + 1) * (1 + (i % 3)) for i in range(d)] for e in range(E)]
    return [[[0.05], [0.1], [0.2]], [[0.1], [0.0], [0.3]], table]


def member_sigma(sigma, e):
    """what the single-network call on member e takes: a float ([E, 1]) or its row of d levels"""
    row = sigma[e]
    return float(row[0]) if len(row) == 1 else [float(v) for v in row]


def mask_of(d):
    """every third coordinate is not disturbed"""
    return [0.0 if i % 3 == 1 else 1.0 for i in range(d)]


@dataclasses.dataclass(frozen=True)
class NoiseCase:
    family: str                # "lane" / "mid"
    case: object               # util_ensemble.EnsCase / util_ensemble_mid.MidCase
    isigma: int                # index into sigma_rows(d)
    row_offset: int
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
    def sigma(self):
        return sigma_rows(self.base.d)[self.isigma]

    @property
    def mask(self):
        return mask_of(self.base.d) if self.masked else None

    @property
    def seed(self):
        """own starts: a seed per member; shared starts: one seed (the members meet the same noise)"""
        return list(SEEDS_OWN) if self.own_x else SEED_SHARED

    def member_seed(self, e):
        return SEEDS_OWN[e] if self.own_x else SEED_SHARED

    @property
    def id(self):
        return f"{self.family}-{self.case.id}-s{self.isigma}-r{self.row_offset}{'-mask' if self.masked else ''}"


def _cases(family, cases, shift):
    return [NoiseCase(family, c, (i + shift) % 3, ROW_OFFSETS[(i + shift) % 3], (i + shift) % 2 == 1) for i, c in enumerate(cases)]


# evaluation and recording forward + gradients: every case of the undisturbed ensembles' lists, both families
FORWARD = _cases("lane", ue.FORWARD, 0) + _cases("mid", uem.FORWARD, 1)
TRAIN = _cases("lane", ue.TRAIN, 1) + _cases("mid", uem.TRAIN, 2)


def first(cases, family, **want):
    """the first case of a family with the given properties (own_x, isigma, masked)"""
    return next(c for c in cases if c.family == family and all(getattr(c, k) == v for k, v in want.items()))
