"""The time-correlated (AR(1) / Ornstein-Uhlenbeck) disturbance of DESIGN.md section 3.18 restated on the host: the Philox words come from
the library's host copy of the generator (nocf_debug_noise_words: no device is touched), the Gaussian from util_noise's float64 Box-Muller
transform, and the path from the float32 recursion

    w_0 = v_0(s0),   w_k = fl32(fl32(rho_i w_{k-1}) + v_k(s1))       v_k(s) = fp32(s_i g(seed, row, k, i))

in numpy, whose float32 arithmetic rounds every product and every sum on its own -- the two roundings of the kernels.  Also: the three host
tables in float64 (what noise_corr_scales is held to), the recursion over two given white tensors (what the fill kernel is held to, bit
for bit), and the shapes the GPU file runs (the smallest batch of every kernel family that has a ragged tail)."""
import ctypes as C
import dataclasses

import numpy as np

import util_disturb as ud
import util_mono as um
import util_tile as ut


def tables64(sigma, rho, nt, d, tspan=(0., 1.), mask=None):
    """(s0, s1, rho) [d] of the specification, formed in float64 and rounded to float32 once; the scales are 0 where mask == 0"""
    h = (float(tspan[1]) - float(tspan[0])) / int(nt)
    sg = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (d,))
    r = np.broadcast_to(np.asarray(rho, dtype=np.float64), (d,))
    s0 = (sg * np.sqrt(h)).astype(np.float32)
    s1 = (sg * np.sqrt(h) * np.sqrt(1.0 - r * r)).astype(np.float32)
    if mask is not None:
        keep = np.asarray(mask).reshape(-1) != 0
        s0, s1 = np.where(keep, s0, np.float32(0)), np.where(keep, s1, np.float32(0))
    return s0, s1, r.astype(np.float32)


def recursion(A, B, rho):
    """the path over two white tensors [nt, n, d] float32: step 0 of A (scale s0), steps k >= 1 of B (scale s1); rho [d] float32.
    Every operation is a float32 numpy operation: one rounding for the product, one for the sum"""
    A, B, rho = np.asarray(A, dtype=np.float32), np.asarray(B, dtype=np.float32), np.asarray(rho, dtype=np.float32)
    W = np.empty_like(A)
    W[0] = A[0]
    for k in range(1, A.shape[0]):
        p = rho[None, :] * W[k - 1]
        assert p.dtype == np.float32
        W[k] = p + B[k]
    return W


def words_grid(L, seed, nt, n, d, row0=0):
    """Philox words 0 and 1 of every (row0 + row, k, i) through nocf_debug_noise_words -> two uint64 arrays [nt, n, d]"""
    f = L.nocf_debug_noise_words
    f.restype = C.c_int
    f.argtypes = [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_uint32)]
    out = (C.c_uint32 * 4)()
    w0 = np.empty((nt, n, d), dtype=np.uint64)
    w1 = np.empty((nt, n, d), dtype=np.uint64)
    for k in range(nt):
        for row in range(n):
            for i in range(d):
                if f(seed, row0 + row, k, i, out) != 0:
                    raise RuntimeError("nocf_debug_noise_words refused a valid key")
                w0[k, row, i], w1[k, row, i] = out[0], out[1]
    return w0, w1


def gauss_of_words(w0, w1):
    """util_noise.gauss from the words: the float64 Box-Muller transform of the specification"""
    u1 = ((w0 >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = ((w1 >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def paths(g, s0, s1, rho):
    """the restated paths [nt, n, d] float32 from the Gaussians g [nt, n, d] float64 and the three float32 tables"""
    A = (s0.astype(np.float64)[None, None, :] * g).astype(np.float32)
    B = (s1.astype(np.float64)[None, None, :] * g).astype(np.float32)
    return recursion(A, B, rho)


def pearson(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


# The GPU file's shapes, from the existing case lists: per family the smallest batch that has one full tile and a ragged one (lane: a
# workgroup is 4 rows; one-CU: 16; per-tile: T = 4), nt = 3.  The one-CU family has three write-back paths (singlequad's register path, the
# generic sweep with one and with two trips per thread) and the per-tile family three (point agents, quadcopters, swarm50's deferred one).
def _small(case, n, **kw):
    return dataclasses.replace(case, n=n, nt=3, stepper="rk4", **kw)


CASES = [
    ("lane", _small(ud.CASES[1][1], 5)),                            # softcorridor, (MP, DP) = (32, 8)
    ("mono", _small(ud.CASES[3][1], 17)),                           # singlequad: z in registers
    ("mono", _small(ud.CASES[4][1], 17)),                           # cross2d d = 14, m = 64: the sweep, one trip
    ("mono", _small(um.ADJOINT[6], 17, mode="eval")),               # cross2d d = 24, m = 64: KBD = 2, two trips for some threads
    ("tile", _small(ud.CASES[5][1], 5)),                            # cross2d d = 4, m = 129: point agents
    ("tile", _small(ut.FORWARD_DEFAULT[5].case, 5, tspan=ud.T1)),   # one quadcopter, m = 129: the sweep over d + 4 components
    ("tile-fixed", _small(ud.CASES[7][1], 5)),                      # swarm50's shape: the deferred write-back, two items for some threads
]
FAMILY_FIRST = [CASES[0], CASES[1], CASES[4], CASES[6]]            # one case per family
KERNEL = {"lane": "rollout_lane_kernel<noise-corr>", "mono": "rollout_mono_kernel<noise-corr>",
          "tile": "rollout_kernel<generic, noise-corr>", "tile-fixed": "rollout_kernel<shape-specialised, noise-corr>"}
TILE = {"lane": 4, "mono": 16, "tile": 4, "tile-fixed": 4}


def case_id(fc):
    return ud.case_id(fc)


def rho_of(case):
    """per component, so that a swapped table index shows; 0 on component 1 (the white value through the new path)"""
    r = 0.3 + 0.6 * np.arange(case.d, dtype=np.float64) / case.d
    r[1] = 0.0
    return r
