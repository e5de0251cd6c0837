"""The counter-based disturbance generator restated in numpy: Philox4x32-10 in uint64 arithmetic, the
Box-Muller transform in float64.  The tests hold the kernels (nocf_noise.inc) to this file; nothing here touches the library."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

# (counter, key, words)
PHILOX_VECTORS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
# (seed, row, k, i, words, g)
NOISE_VECTORS = [
    (1, 0, 0, 0, (0xe3e80670, 0xe50a0ebc, 0x95f222c0, 0xb615aa27), 0.3804007020347322),
    (0xDEADBEEFCAFEF00D, 2 ** 32 + 7, 2, 149, (0x8a688488, 0x3996be31, 0x1771bb3d, 0x4d3f8def), 0.17378962738023698),
    (12345, 5, 1, 3, (0xed9c5c04, 0xe1f3f66b, 0x95dd2bf9, 0xd3fc326b), 0.2857949376537547),
]


def philox4x32_10(counter, key):
    """counter: 4 arrays (broadcastable), key: 2 -> 4 uint64 arrays holding 32-bit words"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & MASK for v in key)
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return c


def noise_words(seed, row, k, i):
    """the layout of the specification: counter (row lo, row hi, k, i), key (seed lo, seed hi); row may be an array"""
    seed = int(seed)
    row = np.asarray(row, dtype=np.uint64)
    return philox4x32_10((row & MASK, row >> S32, np.asarray(k, dtype=np.uint64), np.asarray(i, dtype=np.uint64)),
                         (seed & 0xFFFFFFFF, seed >> 32))


def gauss(seed, row, k, i):
    """g of the specification in float64"""
    w = noise_words(seed, row, k, i)
    u1 = ((w[0] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = ((w[1] >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def gauss_grid(seed, nt, n, d, row0=0):
    """g over the grid [nt, n, d] (time-major like W), float64"""
    k = np.arange(nt, dtype=np.uint64)[:, None, None]
    row = (np.arange(n, dtype=np.uint64) + np.uint64(row0))[None, :, None]
    i = np.arange(d, dtype=np.uint64)[None, None, :]
    return gauss(seed, row, k, i)


def scale_of(sigma, d, nt, tspan=(0., 1.), mask=None):
    """scale[i] = fp32(sigma_i sqrt(h)), formed in double; 0 where mask == 0"""
    h = (float(tspan[1]) - float(tspan[0])) / int(nt)
    s = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (d,)) * np.sqrt(h)
    s = s.astype(np.float32)
    if mask is not None:
        s = np.where(np.asarray(mask).reshape(-1) != 0, s, np.float32(0))
    return s


def disturbances(seed, nt, n, d, sigma, tspan=(0., 1.), mask=None, row0=0):
    """-> (W reference in float64: scale_i * g, scale [d] float32, g [nt, n, d] float64)"""
    sc = scale_of(sigma, d, nt, tspan, mask)
    g = gauss_grid(seed, nt, n, d, row0)
    return sc.astype(np.float64)[None, None, :] * g, sc, g


def zscores(g, g2):
    """the statistics of the specification on a grid g [nt, n, d] (and a second seed's grid g2), each as a z-score under N(0, 1) iid"""
    N = g.size
    out = {"mean": g.mean() * np.sqrt(N),
           "var": (np.mean(g * g) - 1.0) * np.sqrt(N / 2.0),
           "m4": (np.mean(g ** 4) - 3.0) * np.sqrt(N / 96.0)}
    for name, a, b in (("lag_step", g[:-1], g[1:]), ("lag_row", g[:, :-1], g[:, 1:]), ("lag_comp", g[:, :, :-1], g[:, :, 1:]),
                       ("seed", g, g2)):
        out[name] = np.mean(a * b) * np.sqrt(a.size)
    return out
