"""CPU: time-correlated (Ornstein-Uhlenbeck) noise, DESIGN.md section 3.18.  The host tables against a float64 formula; the host
restatement (tests/util_noise_corr.py: Philox words through nocf_debug_noise_words, float64 Box-Muller, float32 recursion) and its
statistics; brownian_disturbances(..., rho=); every refusal of rho, of the three new C entries and of the drivers' --noise_rho -- all
before a device is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import __graft_entry__ as entry
import neuraloc_amd as na
from neuraloc_amd import _lib, noise
import util_noise as un
import util_noise_corr as uc

E_NULL, E_SHAPE = -1, -2
STAT_SEED = 20241                # pinned: the restatement alone satisfies the bounds of test_statistics_of_the_restated_paths


@pytest.fixture(scope="module")
def L():
    entry.build()
    return _lib.lib()


# ---------------------------------------------------------------- host tables
def test_host_tables_against_the_float64_formula():
    sigma = torch.tensor([0.1, 0.2, 0.3, 0.7, 0.05])
    rho = torch.tensor([0.0, 0.5, 0.9, 0.999, 0.25])
    mask = [1, 0, 1, 1, 1]
    for sg, rh, mk, ts, nt in ((sigma, rho, mask, (0.25, 1.0), 3), (0.4, 0.8, None, (0.0, 1.0), 7), (sigma, 0.6, None, (0.0, 2.0), 5),
                               (0.4, rho, mask, (0.0, 1.0), 2)):
        s0, s1, r = na.noise_corr_scales(sg, rh, nt, 5, ts, mk)
        sgn = sg.double().numpy() if isinstance(sg, torch.Tensor) else sg
        rhn = rh.double().numpy() if isinstance(rh, torch.Tensor) else rh
        e0, e1, er = uc.tables64(sgn, rhn, nt, 5, ts, mk)
        assert s0.dtype == s1.dtype == r.dtype == torch.float32 and s0.shape == s1.shape == r.shape == (5,)
        assert np.array_equal(s0.numpy(), e0) and np.array_equal(s1.numpy(), e1) and np.array_equal(r.numpy(), er)
        assert np.array_equal(s0.numpy(), noise.noise_scale(sg, nt, 5, ts, mk).numpy())          # s0 is the white scale
        if mk is not None:
            assert s0[1] == 0 and s1[1] == 0 and float(s0[0]) > 0 and float(s1[2]) > 0
    # rho = 0: s1 == s0, bit for bit
    s0, s1, r = na.noise_corr_scales(sigma, 0.0, 3, 5, (0.25, 1.0), mask)
    assert torch.equal(s0, s1) and float(r.abs().max()) == 0.0
    # the variance is stationary: s1^2 + rho^2 s0^2 = s0^2 up to the tables' rounding
    s0, s1, r = (t.double() for t in na.noise_corr_scales(sigma, rho, 3, 5))
    assert float(((s1 ** 2 + r ** 2 * s0 ** 2) / s0 ** 2 - 1).abs().max()) < 4 * 2.0 ** -23


# ---------------------------------------------------------------- the restatement
def test_restatement_words_and_recursion(L):
    """the words of the library's host generator are util_noise's, the Gaussian of the words is util_noise.gauss, and the recursion is the
    two-rounding one: an fma would differ on this example"""
    seed, row0 = 0xDEADBEEFCAFEF00D, 2 ** 32 + 7
    w0, w1 = uc.words_grid(L, seed, 3, 4, 5, row0)
    k, row, i = np.meshgrid(np.arange(3), np.arange(4) + row0, np.arange(5), indexing="ij")
    ref = un.noise_words(seed, row, k, i)
    assert np.array_equal(w0, ref[0]) and np.array_equal(w1, ref[1])
    assert np.array_equal(uc.gauss_of_words(w0, w1), un.gauss_grid(seed, 3, 4, 5, row0))
    # a hand-made path: rho = 1/3 and 0.1 are not float32 numbers, the products round
    rho = np.array([1.0 / 3.0, 0.1], dtype=np.float32)
    A = np.array([[[0.7, -1.3]], [[9.0, 9.0]], [[9.0, 9.0]]], dtype=np.float32)
    B = np.array([[[5.0, 5.0]], [[0.11, 0.23]], [[-0.5, 0.01]]], dtype=np.float32)
    W = uc.recursion(A, B, rho)
    f32 = np.float32
    for c in range(2):
        w1_ = f32(f32(rho[c] * A[0, 0, c]) + B[1, 0, c])
        w2_ = f32(f32(rho[c] * w1_) + B[2, 0, c])
        assert W[0, 0, c] == A[0, 0, c] and W[1, 0, c] == w1_ and W[2, 0, c] == w2_
    # (float64 product, one rounding of the sum: the fma's result -- differs somewhere on this example, so the test could tell)
    rs = np.random.RandomState(5)
    A2, B2 = rs.standard_normal((2, 1, 256)).astype(f32), rs.standard_normal((2, 1, 256)).astype(f32)
    rho2 = rs.uniform(0.0, 1.0, 256).astype(f32)
    fma = (rho2.astype(np.float64) * A2[0, 0].astype(np.float64) + B2[1, 0].astype(np.float64)).astype(f32)
    assert (fma != uc.recursion(A2, B2, rho2)[1, 0]).any()
    # rho = 0 gives the white values
    assert np.array_equal(uc.recursion(A, A, np.zeros(2, dtype=np.float32)), A)


def test_statistics_of_the_restated_paths(L):
    """n d = 4096 paths of nt = 64 steps at one seed.  Lag-j correlation: the Pearson coefficient over the pairs (w_k, w_{k+j}) at
    k = 0, 16, 32, 48 of every path -- N = 4 * 4096 pairs, independent across paths and 16 steps apart inside one (rho^16 = 0.03), so the
    coefficient's standard error is the independent-pairs one, (1 - rho^2) / sqrt(N); within 5 of them of rho and rho^2.  Variance: the
    sample variance of the 4096 independent values of every step k has the standard error s0^2 sqrt(2 / (N - 1)); within 5 of them of s0^2."""
    nt, n, d, rho, sigma = 64, 64, 64, 0.8, 0.35
    s0, s1, r = uc.tables64(sigma, rho, nt, d)
    g = uc.gauss_of_words(*uc.words_grid(L, STAT_SEED, nt, n, d))
    W = uc.paths(g, s0, s1, r).astype(np.float64)
    ks = np.arange(0, nt - 2, 16)
    N = ks.size * n * d
    assert n * d >= 4096 and N == 4 * 4096
    se = (1.0 - rho ** 2) / np.sqrt(N)
    for lag, want in ((1, rho), (2, rho ** 2)):
        got = uc.pearson(W[ks], W[ks + lag])
        print("lag", lag, "correlation", got, "expected", want, "z", (got - want) / se)
        assert abs(got - want) <= 5.0 * se, (lag, got, want, se)
    var0 = float(s0[0]) ** 2
    sev = var0 * np.sqrt(2.0 / (n * d - 1))
    v = W.reshape(nt, -1).var(axis=1, ddof=1)
    print("largest variance z", float(np.abs(v - var0).max() / sev))
    assert (np.abs(v - var0) <= 5.0 * sev).all()
    # rho = 0: the same Gaussians give the white tensor
    assert np.array_equal(uc.paths(g[:4], s0, s0, np.zeros(d, dtype=np.float32)), (s0.astype(np.float64) * g[:4]).astype(np.float32))


# ---------------------------------------------------------------- the torch helper
def test_brownian_disturbances_rho():
    gen = lambda: torch.Generator().manual_seed(11)                  # noqa: E731
    sig = torch.tensor([0.1, 0.2, 0.3, 0.4])
    white = na.brownian_disturbances(5, 7, 4, sig, (0.25, 1.0), generator=gen(), mask=[1, 1, 0, 1])
    zero = na.brownian_disturbances(5, 7, 4, sig, (0.25, 1.0), generator=gen(), mask=[1, 1, 0, 1], rho=0.0)
    assert torch.equal(white, zero)
    # the recursion by hand on a 3-step example: w_0 = v_0, w_k = rho w_{k-1} + sqrt(1 - rho^2) v_k
    rho = torch.tensor([0.5, 0.0, 0.9, 0.25])
    v = na.brownian_disturbances(3, 2, 4, sig, generator=gen())
    w = na.brownian_disturbances(3, 2, 4, sig, generator=gen(), rho=rho)
    q = torch.sqrt(1 - rho.double() ** 2).float()
    w1 = rho * v[0] + q * v[1]
    w2 = rho * w1 + q * v[2]
    assert w.dtype == torch.float32 and w.shape == (3, 2, 4) and w.is_contiguous()
    assert torch.equal(w[0], v[0]) and torch.allclose(w[1], w1, rtol=1e-6, atol=0) and torch.allclose(w[2], w2, rtol=1e-6, atol=0)
    assert torch.equal(w[:, :, 1], v[:, :, 1])                       # (the component with rho = 0)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="rho"):
            na.brownian_disturbances(3, 2, 4, sig, rho=bad)


# ---------------------------------------------------------------- refusals
def _phi_prob(d=4, m=16):
    return na.Phi(nTh=2, m=m, d=d, alph=[1.0] * 6), na.Cross2D(torch.zeros(d))


def _calls(x, net, prob, ts):
    """every Python call that takes rho, as name -> f(rho)"""
    w = torch.full((x.shape[0],), 1.0 / x.shape[0])
    return {
        "counter_disturbances": lambda rho: na.counter_disturbances(2, 3, 4, 0.1, 1, device="cuda:0", rho=rho),
        "noisy_rollout": lambda rho: na.noisy_rollout(x, net, prob, 2, 0.1, 1, rho=rho),
        "noisy_ocflow_train": lambda rho: na.noisy_ocflow_train(x, net, prob, ts, 2, 0.1, 1, rho=rho),
        "noise_study": lambda rho: na.noise_study(x, net, prob, 2, 0.1, 4, rng="counter", seed=1, rho=rho),
        "noise_study_torch": lambda rho: na.noise_study(x, net, prob, 2, 0.1, 4, generator=torch.Generator(), rho=rho),
        "risk_ocflow_train": lambda rho: na.risk_ocflow_train(x, net, prob, ts, 2, "cvar", 0.5, paths=3, sigma=0.1, seed=1, rho=rho),
        "weighted_ocflow_train": lambda rho: na.weighted_ocflow_train(x, net, prob, ts, 2, w, sigma=0.1, seed=1, rho=rho),
        "noise_corr_scales": lambda rho: na.noise_corr_scales(0.1, rho, 2, 4),
    }


def test_python_refusals_of_rho_touch_no_device():
    net, prob = _phi_prob()
    x = torch.zeros(3, 4)
    ts = [0.0, 1.0]
    calls = _calls(x, net, prob, ts)
    for name, f in calls.items():
        # outside [0, 1) or non-finite
        for bad in (1.0, -0.25, float("nan"), float("inf"), torch.tensor([0.1, 0.2, 1.5, 0.3]), 1.0 - 2.0 ** -30, True):
            with pytest.raises(ValueError, match="0 <= rho < 1"):
                f(bad)
        # a wrong shape
        for bad in (torch.full((3,), 0.5), torch.full((2, 4), 0.5), [0.5, 0.5]):
            with pytest.raises(ValueError, match="rho must be a float or a \\[d\\] tensor"):
                f(bad)
        # float64
        with pytest.raises((RuntimeError, NotImplementedError), match="rho is float64"):
            f(torch.full((4,), 0.5, dtype=torch.float64))
    # float64 states keep their refusal with rho
    with pytest.raises(RuntimeError, match="single precision only"):
        na.noisy_rollout(x.double(), net, prob, 2, 0.1, 1, rho=0.5)
    with pytest.raises(RuntimeError, match="single precision only"):
        na.noisy_ocflow_train(x.double(), net, prob, ts, 2, 0.1, 1, rho=0.5)
    with pytest.raises(NotImplementedError, match="float64"):
        na.risk_ocflow_train(x.double(), net, prob, ts, 2, "cvar", 0.5, paths=3, sigma=0.1, seed=1, rho=0.5)
    # a PhiEnsemble
    ens = na.PhiEnsemble(2, nTh=2, m=16, d=4, r=5, seeds=[1, 2])
    with pytest.raises(NotImplementedError, match="rho with a PhiEnsemble is not supported"):
        na.noisy_rollout(x, ens, prob, 2, 0.1, 1, rho=0.5)
    with pytest.raises(NotImplementedError, match="rho with a PhiEnsemble is not supported"):
        na.noisy_ocflow_train(x, ens, prob, ts, 2, 0.1, 1, rho=0.5)
    with pytest.raises(NotImplementedError, match="rho with a PhiEnsemble is not supported"):
        na.noise_study(x, ens, prob, 2, 0.1, 4, rng="counter", seed=1, rho=0.5)
    with pytest.raises(NotImplementedError, match="ensembles are not supported"):
        na.risk_ocflow_train(x, ens, prob, ts, 2, "cvar", 0.5, paths=3, sigma=0.1, seed=1, rho=0.5)
    for f in (lambda: na.ensemble_noisy_rollout(x, ens, prob, ts, 2, 0.1, 1, rho=0.5),
              lambda: na.ensemble_noisy_ocflow_train(x, ens, prob, ts, 2, 0.1, 1, rho=0.0),
              lambda: na.ensemble_noise_study(x, ens, prob, 2, 0.1, 4, 1, rho=0.5)):
        with pytest.raises(NotImplementedError, match="rho is not supported for ensembles"):
            f()
    # rho together with a tensor W
    W = torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match="rho belongs to sigma"):
        na.risk_ocflow_train(x, net, prob, ts, 2, "cvar", 0.5, paths=3, W=W, rho=0.5)
    with pytest.raises(ValueError, match="rho belongs to sigma"):
        na.weighted_ocflow_train(x, net, prob, ts, 2, torch.full((3,), 1.0 / 3), W=W, rho=0.5)
    # no CPU fallback: a valid call with rho on host tensors is refused too, behind every argument check
    for name in ("noisy_rollout", "noisy_ocflow_train", "noise_study", "risk_ocflow_train", "weighted_ocflow_train"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            calls[name](0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        na.counter_disturbances(2, 3, 4, 0.1, 1, device="cpu", rho=0.5)
    assert "noise_corr_scales" in dir(na)


def _stepper():
    from neuraloc_amd.OCflow import _STEPPERS
    return _STEPPERS["rk4"]


def test_c_entries_refuse_before_anything_is_enqueued(L):
    """a NULL table or output -> NOCF_E_NULL; n, nt, d < 1 or row0 < 0 -> NOCF_E_SHAPE; the pointers are never dereferenced"""
    ff, fe, fr = (noise._entry(L, name) for name in ("nocf_noise_fill_corr_f32", "nocf_rollout_noisy_corr_f32",
                                                      "nocf_rollout_record_noisy_corr_f32"))
    assert ff is not None and fe is not None and fr is not None
    p = C.c_void_p(0x1000)
    assert ff(None, 2, 2, 2, p, p, p, 1, 0, None) == E_NULL
    for tabs in ((None, p, p), (p, None, p), (p, p, None)):
        assert ff(p, 2, 2, 2, *tabs, 1, 0, None) == E_NULL
    assert ff(p, 0, 2, 2, p, p, p, 1, 0, None) == E_SHAPE
    assert ff(p, 2, 0, 2, p, p, p, 1, 0, None) == E_SHAPE
    assert ff(p, 2, 2, 0, p, p, p, 1, 0, None) == E_SHAPE
    assert ff(p, 2, 2, 2, p, p, p, 1, -1, None) == E_SHAPE
    phi = _lib.NocfPhi()
    phi.d, phi.m, phi.nTh, phi.r = 4, 16, 2, 5
    for k in ("K0", "b0", "K", "b", "w", "A", "cw", "cb_dev"):
        setattr(phi, k, 0x1000)                                      # (never dereferenced: every call below is refused)
    prob, keep = na.Cross2D(torch.zeros(4))._c_struct("cpu")
    alph = (C.c_float * 6)(*[1.0] * 6)
    rec = C.c_int32(-1)

    def ev(tabs=(p, p, p), row0=0, n=3, nt=2, z=p, tab=p, sums=None, means=None):
        return fe(C.byref(phi), C.byref(prob), p, *tabs, 7, row0, n, 0.0, 1.0, nt, _stepper(), alph,
                  z, tab, sums, means, None, None, p, 4096 * 4, None)

    def rc(tabs=(p, p, p), row0=0, n=3, nt=2, z=p, s_all=p):
        return fr(C.byref(phi), C.byref(prob), p, *tabs, 7, row0, n, 0.0, 1.0, nt, _stepper(), alph,
                  z, p, None, s_all, None, C.byref(rec), p, 4096 * 4, None)

    for tabs in ((None, p, p), (p, None, p), (p, p, None)):
        assert ev(tabs=tabs) == E_NULL and rc(tabs=tabs) == E_NULL
    assert ev(row0=-1) == E_SHAPE and rc(row0=-1) == E_SHAPE
    assert ev(n=0) == E_SHAPE and rc(n=0) == E_SHAPE
    assert ev(nt=0) == E_SHAPE and rc(nt=0) == E_SHAPE
    assert ev(tab=None, sums=p) == E_NULL and ev(sums=None, means=p) == E_NULL
    assert rc(z=None) == E_NULL and rc(s_all=None) == E_NULL
    assert rec.value == 0                                            # (the flag is cleared even by a refused call)


def test_drivers_refuse_noise_rho_in_their_parsers(tmp_path, capsys):
    import evalOC
    import trainOC
    base = ["--data", "softcorridor", "--niters", "2", "--n_train", "16", "--nt", "4", "--m", "16", "--save", str(tmp_path / "t")]
    ok = trainOC.parse_args(base + ["--noise", "0.1", "--noise_rho", "0.5"])
    assert ok.noise_rho == 0.5 and trainOC.parse_args(base).noise_rho == 0.0
    ok = trainOC.parse_args(base + ["--noise", "0.1", "--noise_rng", "counter", "--noise_rho", "0.5", "--risk", "cvar", "--risk_level", "0.5"])
    assert ok.risk == "cvar"                                         # --risk takes it
    for flags, msg in ((["--noise_rho", "0.5"], "needs --noise"),
                       (["--noise", "0.1", "--noise_rho", "1.0"], "0 <= RHO < 1"),
                       (["--noise", "0.1", "--noise_rho", "-0.5"], "0 <= RHO < 1"),
                       (["--noise", "0.1", "--noise_rho", "nan"], "0 <= RHO < 1"),
                       (["--noise", "0.1", "--noise_rho", "0.5", "--members", "2"], "excludes --members"),
                       (["--noise", "0.1", "--noise_rho", "0.5", "--members", "2", "--members_sigma", "0.1,0.2"], "excludes --members"),
                       (["--noise", "0.1", "--noise_rho", "0.5", "--adv", "0.3"], "excludes --adv"),
                       (["--noise", "0.1", "--noise_rho", "0.5", "--prec", "double"], "single precision")):
        with pytest.raises(SystemExit, match=msg):
            trainOC.parse_args(base + flags)
        with pytest.raises(SystemExit, match=msg):
            trainOC.main(base + flags)
    ebase = ["--resume", str(tmp_path / "none_checkpt.pth"), "--save", str(tmp_path / "e")]
    a = evalOC.p.parse_args(ebase + ["--noise", "0.1", "--noise_rho", "0.5"])
    evalOC.noise_rho_refusals(a)
    assert a.noise_rho == 0.5 and evalOC.p.parse_args(ebase).noise_rho == 0.0
    for flags, msg in ((["--noise_rho", "0.5"], "needs --noise"), (["--noise", "0.1", "--noise_rho", "1.5"], "0 <= RHO < 1"),
                       (["--noise", "0.1", "--noise_rho", "0.5", "--prec", "double"], "single precision")):
        with pytest.raises(SystemExit, match=msg):
            evalOC.noise_rho_refusals(evalOC.p.parse_args(ebase + flags))
        with pytest.raises(SystemExit, match=msg):
            evalOC.main(ebase + flags)
    assert not (tmp_path / "t").exists() and not (tmp_path / "e").exists()
    assert "loading model" not in capsys.readouterr().out
