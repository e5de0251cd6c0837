"""CPU: the counter-based disturbance generator.  The numpy restatement (tests/util_noise.py) against the known
answers of Philox4x32-10 and of the (seed, row, k, i) layout; the library's host copy of the integer part (nocf_debug_noise_words) against
the restatement; the restatement's statistics on a 64 x 1024 x 64 grid; the refusals of the three C entries, of the Python calls and of the
drivers -- all before a device is touched."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import neuraloc_amd as na
from neuraloc_amd import _lib, noise
import util_noise as un

E_NULL, E_SHAPE = -1, -2


@pytest.fixture(scope="module")
def L():
    entry.build()
    return _lib.lib()


def test_restatement_reproduces_the_philox_vectors():
    for counter, key, words in un.PHILOX_VECTORS:
        assert tuple(int(w) for w in un.philox4x32_10(counter, key)) == words


def test_restatement_reproduces_the_layout_vectors():
    for seed, row, k, i, words, g in un.NOISE_VECTORS:
        assert tuple(int(w) for w in un.noise_words(seed, row, k, i)) == words
        assert abs(float(un.gauss(seed, row, k, i)) - g) <= 4e-16 * abs(g)


def _lib_words(L, seed, row, k, i):
    f = L.nocf_debug_noise_words
    f.restype = C.c_int
    f.argtypes = [C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_uint32)]
    out = (C.c_uint32 * 4)()
    assert f(seed, row, k, i, out) == 0
    return tuple(out)


def test_library_words_are_the_restatement(L):
    assert _lib.lib().nocf_version() == 113
    for counter, key, words in un.PHILOX_VECTORS:                   # the raw vectors through the layout: row = c0 | c1 << 32, seed = k0 | k1 << 32
        row = counter[0] | (counter[1] << 32)
        if row < 2 ** 63 and counter[2] < 2 ** 31 and counter[3] < 2 ** 31:
            assert _lib_words(L, key[0] | (key[1] << 32), row, counter[2], counter[3]) == words
    for seed, row, k, i, words, _ in un.NOISE_VECTORS:
        assert _lib_words(L, seed, row, k, i) == words
    rnd = random.Random(20240607)
    for q in range(300):
        seed = rnd.getrandbits(64) if q % 3 else rnd.getrandbits(31)        # high word set / clear
        row = rnd.getrandbits(44) if q % 2 else rnd.getrandbits(20)         # rows >= 2^32 and small ones
        k, i = rnd.getrandbits(12), rnd.getrandbits(9)
        assert _lib_words(L, seed, row, k, i) == tuple(int(w) for w in un.noise_words(seed, row, k, i)), (seed, row, k, i)
    out = (C.c_uint32 * 4)()
    assert L.nocf_debug_noise_words(1, -1, 0, 0, out) == E_SHAPE
    assert L.nocf_debug_noise_words(1, 0, 0, 0, None) == E_NULL


def test_statistics_of_the_grid():
    """mean, variance, fourth moment, lag-1 correlations along steps / rows / components and the correlation between two seeds on
    nt, n, d = 64, 1024, 64 at seed 12345, each as a z-score: within 5 (the restatement itself stays under 2: DESIGN.md section 3.10)"""
    g = un.gauss_grid(12345, 64, 1024, 64)
    g2 = un.gauss_grid(12346, 64, 1024, 64)
    z = un.zscores(g, g2)
    print({k: round(float(v), 3) for k, v in z.items()})
    assert float(np.abs(g).max()) <= 5.77
    for k, v in z.items():
        assert abs(v) <= 5.0, (k, v)
    want = {"mean": -1.09, "var": 0.93, "m4": 1.98, "lag_step": -0.85, "lag_row": -0.26, "lag_comp": -0.49, "seed": 1.43}
    for k, v in want.items():                                        # (the specification's table)
        assert abs(z[k] - v) <= 0.006, (k, z[k], v)


def _fill(L):
    f = L.nocf_noise_fill_f32
    f.restype = C.c_int
    f.argtypes = _lib.PROTOTYPES["nocf_noise_fill_f32"][1]
    return f


def test_fill_refusals(L):
    f = _fill(L)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    assert f(None, 2, 2, 2, p, 1, 0, None) == E_NULL
    assert f(p, 2, 2, 2, None, 1, 0, None) == E_NULL
    assert f(p, 0, 2, 2, p, 1, 0, None) == E_SHAPE
    assert f(p, 2, 0, 2, p, 1, 0, None) == E_SHAPE
    assert f(p, 2, 2, 0, p, 1, 0, None) == E_SHAPE
    assert f(p, 2, 2, 2, p, 1, -1, None) == E_SHAPE


def _phi_prob(d=4, m=16):
    return na.Phi(nTh=2, m=m, d=d, alph=[1.0] * 6), na.Cross2D(torch.zeros(d))


def test_rollout_entries_refuse_before_anything_is_enqueued(L):
    """null scale / outputs -> NOCF_E_NULL; n, nt < 1 or row0 < 0 -> NOCF_E_SHAPE; the pointers are never dereferenced"""
    fe, fr = noise._entry(L, "nocf_rollout_noisy_f32"), noise._entry(L, "nocf_rollout_record_noisy_f32")
    assert fe is not None and fr is not None
    phi = _lib.NocfPhi()
    phi.d, phi.m, phi.nTh, phi.r = 4, 16, 2, 5
    for k in ("K0", "b0", "K", "b", "w", "A", "cw", "cb_dev"):
        setattr(phi, k, 0x1000)                                      # (never dereferenced: every call below is refused)
    prob, keep = na.Cross2D(torch.zeros(4))._c_struct("cpu")
    p = C.c_void_p(0x1000)
    alph = (C.c_float * 6)(*[1.0] * 6)
    rec = C.c_int32(-1)

    def ev(scale=p, row0=0, n=3, nt=2, z=p, tab=p, sums=None, means=None):
        return fe(C.byref(phi), C.byref(prob), p, scale, 7, row0, n, 0.0, 1.0, nt, _lib_stepper(), alph,
                  z, tab, sums, means, None, None, p, 4096 * 4, None)

    def rc(scale=p, row0=0, n=3, nt=2, z=p, s_all=p):
        return fr(C.byref(phi), C.byref(prob), p, scale, 7, row0, n, 0.0, 1.0, nt, _lib_stepper(), alph,
                  z, p, None, s_all, None, C.byref(rec), p, 4096 * 4, None)

    assert ev(scale=None) == E_NULL and rc(scale=None) == E_NULL
    assert ev(row0=-1) == E_SHAPE and rc(row0=-1) == E_SHAPE
    assert ev(n=0) == E_SHAPE and rc(n=0) == E_SHAPE
    assert ev(nt=0) == E_SHAPE and rc(nt=0) == E_SHAPE
    assert ev(tab=None, sums=p) == E_NULL                            # sums without the table they are formed from
    assert ev(sums=None, means=p) == E_NULL
    assert rc(z=None) == E_NULL and rc(s_all=None) == E_NULL
    assert rec.value == 0                                            # (the flag is cleared even by a refused call)


def _lib_stepper():
    from neuraloc_amd.OCflow import _STEPPERS
    return _STEPPERS["rk4"]


def test_python_refusals_touch_no_device():
    net, prob = _phi_prob()
    x = torch.zeros(3, 4)
    ts = [0.0, 1.0]
    # float64
    with pytest.raises(RuntimeError, match="single precision only"):
        na.noisy_rollout(x.double(), net, prob, 2, 0.1, 1)
    with pytest.raises(RuntimeError, match="single precision only"):
        na.noisy_ocflow_train(x.double(), net, prob, ts, 2, 0.1, 1)
    # shapes
    with pytest.raises(ValueError, match="nex-by-d"):
        na.noisy_rollout(x[0], net, prob, 2, 0.1, 1)
    with pytest.raises(ValueError, match="Phi was built for"):
        na.noisy_rollout(torch.zeros(3, 5), net, prob, 2, 0.1, 1)
    with pytest.raises(ValueError, match="nt must be"):
        na.noisy_ocflow_train(x, net, prob, ts, 0, 0.1, 1)
    with pytest.raises(ValueError, match="stepper"):
        na.noisy_rollout(x, net, prob, 2, 0.1, 1, stepper="rk2")
    with pytest.raises(ValueError, match=">= 1"):
        na.counter_disturbances(0, 3, 4, 0.1, 1, device="cuda:0")
    # sigma / mask of the wrong length
    for bad in (torch.ones(3), torch.ones(2, 4)):
        with pytest.raises(ValueError, match="sigma"):
            na.noisy_rollout(x, net, prob, 2, bad, 1)
        with pytest.raises(ValueError, match="sigma"):
            na.noisy_ocflow_train(x, net, prob, ts, 2, bad, 1)
        with pytest.raises(ValueError, match="sigma"):
            na.counter_disturbances(2, 3, 4, bad, 1, device="cuda:0")
    with pytest.raises(ValueError, match="mask"):
        na.counter_disturbances(2, 3, 4, 0.1, 1, mask=torch.ones(3), device="cuda:0")
    # seeds: Python ints in [0, 2^64)
    for bad in (-1, 2 ** 64, 1.0, True, None, torch.tensor(3)):
        with pytest.raises(ValueError, match="seed"):
            na.noisy_rollout(x, net, prob, 2, 0.1, bad)
        with pytest.raises(ValueError, match="seed"):
            na.noisy_ocflow_train(x, net, prob, ts, 2, 0.1, bad)
        with pytest.raises(ValueError, match="seed"):
            na.counter_disturbances(2, 3, 4, 0.1, bad, device="cuda:0")
    with pytest.raises(ValueError, match="row_offset"):
        na.noisy_rollout(x, net, prob, 2, 0.1, 1, row_offset=-1)
    # noise_study: the generator belongs to rng="torch", the seed to rng="counter"
    with pytest.raises(ValueError, match="generator"):
        na.noise_study(x, net, prob, 2, 0.1, 4, rng="counter", seed=1, generator=torch.Generator())
    with pytest.raises(ValueError, match="seed"):
        na.noise_study(x, net, prob, 2, 0.1, 4, rng="counter")
    with pytest.raises(ValueError, match="seed"):
        na.noise_study(x, net, prob, 2, 0.1, 4, rng="counter", seed=2 ** 64)
    with pytest.raises(ValueError, match="rng"):
        na.noise_study(x, net, prob, 2, 0.1, 4, rng="philox", seed=1)
    # no CPU fallback: a valid call on host tensors is refused too
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.noisy_rollout(x, net, prob, 2, 0.1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.counter_disturbances(2, 3, 4, 0.1, 1, device="cpu")
    # the scale is formed in double and rounded once
    sc = noise.noise_scale(torch.tensor([0.1, 0.2, 0.3, 0.7]), 3, 4, (0.25, 1.0), mask=[1, 0, 1, 1])
    assert np.array_equal(sc.numpy(), un.scale_of([0.1, 0.2, 0.3, 0.7], 4, 3, (0.25, 1.0), [1, 0, 1, 1]))
    for name in ("counter_disturbances", "noisy_rollout", "noisy_ocflow_train"):
        assert name in dir(na)


def test_drivers_refuse_counter_noise_in_double_precision(tmp_path, capsys):
    import evalOC
    import trainOC
    save = str(tmp_path / "t")
    with pytest.raises(SystemExit, match="single precision"):
        trainOC.main(["--data", "softcorridor", "--niters", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save,
                      "--prec", "double", "--noise_rng", "counter"])
    with pytest.raises(SystemExit, match="single precision"):
        trainOC.main(["--data", "softcorridor", "--niters", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", save,
                      "--prec", "double", "--noise", "0.1", "--noise_rng", "counter"])
    save2 = str(tmp_path / "e")
    with pytest.raises(SystemExit, match="single precision"):
        evalOC.main(["--resume", str(tmp_path / "none_checkpt.pth"), "--save", save2, "--prec", "double", "--noise_rng", "counter"])
    with pytest.raises(SystemExit, match="single precision"):
        evalOC.main(["--resume", str(tmp_path / "none_checkpt.pth"), "--save", save2, "--prec", "double", "--noise", "0.1",
                     "--noise_paths", "8", "--noise_rng", "counter"])
    assert not (tmp_path / "t").exists() and not (tmp_path / "e").exists()
    assert "loading model" not in capsys.readouterr().out
