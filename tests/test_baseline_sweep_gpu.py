"""GPU: the direct-transcription baseline kernels (nocf_baseline.inc) against an fp64 restatement at every launch shape baseline_setup
can choose, for every point-agent problem in train and eval mode, at the largest nt each entry point accepts; torch's CPU Adam step in
isolation (m and v bit for bit; U bit for bit up to torch's CPU float sqrt); the best-iterate bookkeeping; the batch forms and a
3000-start launch.

The tolerance calibrates itself (tests/util_oracle.py compare): the kernel may be off fp64 by 4x what the fp32 restatement is off, at
least 1e-6 of the quantity's size.  The trajectory must be the reference's fp32 recursion bit for bit."""
import pytest
import torch

import neuraloc_amd as na
import util_oracle as uo

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _dev(*ts):
    return [t.to(DEV) for t in ts]


@pytest.mark.parametrize("case", uo.SWEEP, ids=lambda c: c.id)
def test_sweep_against_fp64(case):
    S, z0, U, traj = uo.case_data(case)
    prob, _ = uo.make_prob(case.name, case.alph, case.mode, DEV)
    aG = case.alph[0]
    zd, Ud = _dev(z0, U)
    J, g = na.baseline_loss(zd, Ud, prob, aG, grad=True)
    rep, tr = na.baseline_report(zd, Ud, prob, aG)
    assert torch.equal(tr.cpu(), traj.transpose(1, 2)), "trajectory differs from the fp32 recursion"
    r64 = uo.restate(S, z0, U, aG, torch.float64, traj)
    r32 = uo.restate(S, z0, U, aG, torch.float32, traj)
    res = uo.compare_all(dict(J=J, grad=g, report=rep), r64, r32)
    nth, G = uo.launch_shape(uo.N_AGENTS[case.name], case.nt)
    print(f"[sweep] {case.id} nth={nth} G={G} " + " ".join(f"{k}:{e:.3g}/{e32:.3g}" for k, (_, e, _, e32) in res.items()))
    bad = {k: v for k, v in res.items() if not v[0]}
    assert not bad, f"{case.id} (nth {nth}, G {G}) off fp64 beyond tolerance: " + \
        ", ".join(f"{k} err {e:.3g} > tol {t:.3g} (fp32 restatement {e32:.3g})" for k, (_, e, t, e32) in bad.items())
    gaps = uo.physics_gaps(case, S, r64)
    assert not gaps, f"{case.id} does not test the physics: {gaps}"


# ---------------------------------------------------------------------------------------------------------------------------------
# one Adam step against torch.optim.Adam
# ---------------------------------------------------------------------------------------------------------------------------------
def _cpu_adam(U, m, v, g, step0, lr, betas, eps):
    """torch.optim.Adam's single-tensor step on the CPU in fp32 from the given state -> (U, m, v)"""
    p = torch.nn.Parameter(U.detach().cpu().clone())
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=False, fused=False)
    opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m.detach().cpu().clone(),
                    "exp_avg_sq": v.detach().cpu().clone()}
    p.grad = g.detach().cpu().clone()
    opt.step()
    return p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]


def _adam_ops(U, m, v, g, step0, lr, betas, eps, sqrt):
    """_single_tensor_adam's ops (torch/optim/adam.py) written out on CPU fp32 tensors, with `sqrt` for the square root"""
    U, m, v, g = (t.detach().cpu().clone() for t in (U, m, v, g))
    m.lerp_(g, 1 - betas[0])
    v.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
    step = float(step0 + 1)
    bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
    U.addcdiv_(m, (sqrt(v) / bc2 ** 0.5).add_(eps), value=-lr / bc1)
    return U, m, v


def _ieee_sqrt(x):
    """the correctly rounded fp32 square root (an fp64 square root rounded to fp32 is)"""
    return x.double().sqrt().float()


def _adam_one_step(prob, z0, U, m, v, aG, step0, lr, betas, eps):
    """one kernel Adam iteration against torch.optim.Adam on the CPU, fed with the kernel's gradient -> (elements of U not bitwise
    torch.optim.Adam's, elements where torch's CPU float sqrt of v is not the correctly rounded one)"""
    B = U.shape[0]
    J, g = na.baseline_loss(z0, U, prob, aG, grad=True)
    what = f"step0 {step0}, lr {lr}, betas {betas}, eps {eps}"
    # the Adam kernel's own gradient is baseline_loss's: with beta1 = 0 the new m is fmaf(0, g - m, g) = g
    m0, v0, U0 = m.clone(), v.clone(), U.clone()
    na.baseline_adam_steps(z0, U0, m0, v0, torch.full((B,), float("inf"), device=DEV), torch.zeros_like(U), prob, aG, 1,
                           step0=step0, lr=lr, betas=(0.0, betas[1]), eps=eps)
    assert torch.equal(m0, g), f"the Adam kernel's gradient is not baseline_loss's: {int((m0 != g).sum())} elements differ"
    Uk, mk, vk = U.clone(), m.clone(), v.clone()
    best = torch.full((B,), float("inf"), device=DEV)
    Ub = torch.zeros_like(U)
    hist = torch.empty(B, 1, device=DEV)
    na.baseline_adam_steps(z0, Uk, mk, vk, best, Ub, prob, aG, 1, step0=step0, lr=lr, betas=betas, eps=eps, hist=hist)
    assert torch.equal(hist[:, 0], J), "hist[0] != baseline_loss"
    assert torch.equal(best, J) and torch.equal(Ub, U)
    Uc, mc, vc = _cpu_adam(U, m, v, g, step0, lr, betas, eps)
    # the written-out ops are torch.optim.Adam's step, bit for bit
    assert all(torch.equal(a, b) for a, b in zip(_adam_ops(U, m, v, g, step0, lr, betas, eps, torch.sqrt), (Uc, mc, vc))), what
    # m and v (no square root in them): bitwise torch.optim.Adam's
    assert torch.equal(mk.cpu(), mc), f"m: {int((mk.cpu() != mc).sum())} elements not bitwise torch.optim.Adam's ({what})"
    assert torch.equal(vk.cpu(), vc), f"v: {int((vk.cpu() != vc).sum())} elements not bitwise torch.optim.Adam's ({what})"
    # U: bitwise torch's ops with a correctly rounded sqrt; it differs from torch.optim.Adam's only where torch's own float sqrt of v
    # is not correctly rounded (the CPU's vector sqrt; the kernel's sqrtf is correctly rounded)
    Ui = _adam_ops(U, m, v, g, step0, lr, betas, eps, _ieee_sqrt)[0]
    assert torch.equal(Uk.cpu(), Ui), f"U: {int((Uk.cpu() != Ui).sum())} elements not bitwise torch's Adam ops ({what})"
    off, root_off = Uk.cpu() != Uc, torch.sqrt(vc) != _ieee_sqrt(vc)
    assert not bool((off & ~root_off).any()), what
    return int(off.sum()), int(root_off.sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# the nt limits
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(uo.BASE_ALPH))
def test_nt_limits(name):
    """the largest nt of each entry point launches; one more is refused on the host (NOCF_E_SHAPE -> RuntimeError).  At the adam limit
    (its largest LDS footprint) one iteration is torch's CPU Adam step."""
    ev, ad = uo.nt_limits(name)
    alph = uo.BASE_ALPH[name]
    prob, xInit = uo.make_prob(name, alph, "train", DEV)
    d = xInit.numel()
    with pytest.raises(RuntimeError):
        na.baseline_loss(xInit, torch.zeros(ev + 1, d, device=DEV), prob, alph[0])
    with pytest.raises(RuntimeError):
        na.solve_baseline(xInit, prob, ad + 1, niters=1, U0=torch.zeros(ad + 1, d, device=DEV))
    assert bool(torch.isfinite(na.baseline_loss(xInit, torch.zeros(ev, d, device=DEV), prob, alph[0])))
    gen = torch.Generator().manual_seed(11)
    U = torch.randn(2, ad, d, generator=gen)
    m = 0.1 * torch.randn(2, ad, d, generator=gen)
    v = torch.rand(2, ad, d, generator=gen) * 0.01
    z0 = xInit.cpu() + 0.3 * torch.randn(2, d, generator=gen)
    n, r = _adam_one_step(prob, *_dev(z0, U, m, v), alph[0], 5, 0.1, (0.9, 0.999), 1e-8)
    print(f"[limits] {name} eval {ev} adam {ad}: {n} elements of U not bitwise torch.optim.Adam's, {r} of its sqrt(v) not correctly "
          f"rounded")


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam in isolation, the best iterate
# ---------------------------------------------------------------------------------------------------------------------------------
ADAM_SHAPES = [("softcorridor", 50), ("swarm", 20)]          # 256 threads (G 4), 1024 threads (G 32)


@pytest.mark.parametrize("name,nt", ADAM_SHAPES)
def test_adam_step_is_torch_cpu_adam(name, nt):
    alph = uo.BASE_ALPH[name]
    prob, xInit = uo.make_prob(name, alph, "train", DEV)
    assert uo.launch_shape(uo.N_AGENTS[name], nt)[0] == (256 if name == "softcorridor" else 1024)
    d = xInit.numel()
    gen = torch.Generator().manual_seed(5)
    z0 = xInit.cpu() + 0.3 * torch.randn(2, d, generator=gen)
    U = (uo.make_prob(name, alph, "train")[0].xtarget.reshape(-1) - z0).unsqueeze(1) + 0.5 * torch.randn(2, nt, d, generator=gen)
    m = 0.3 * torch.randn(2, nt, d, generator=gen)
    v = torch.rand(2, nt, d, generator=gen) ** 2
    off = roots = 0
    for step0 in (0, 1, 37, 10000):
        for lr in (0.1, 1e-3):
            for betas in ((0.9, 0.999), (0.5, 0.9)):
                for eps in (1e-8, 1e-3):
                    n, r = _adam_one_step(prob, *_dev(z0, U, m, v), alph[0], step0, lr, betas, eps)
                    off, roots = off + n, roots + r
    print(f"[adam] {name} nt={nt}, 32 settings: m, v bitwise torch.optim.Adam's; {off} elements of U not, {roots} of its sqrt(v) "
          f"not correctly rounded")


def _state(U0):
    B = U0.shape[0]
    return [U0.clone(), torch.zeros_like(U0), torch.zeros_like(U0), torch.full((B,), float("inf"), device=DEV),
            torch.zeros_like(U0)]


def test_best_iterate_bookkeeping():
    name, nt, K, lr = "softcorridor", 20, 12, 2.0
    alph = uo.BASE_ALPH[name]
    prob, xInit = uo.make_prob(name, alph, "train", DEV)
    gen = torch.Generator().manual_seed(9)
    z0 = (xInit.cpu() + 0.3 * torch.randn(3, xInit.numel(), generator=gen)).to(DEV)
    U0 = na.baseline.initial_guess(z0, prob, nt, torch.Generator(device=DEV).manual_seed(9))
    one = _state(U0)
    h1 = torch.empty(3, K, device=DEV)
    na.baseline_adam_steps(z0, *one, prob, alph[0], K, lr=lr, hist=h1)
    split = _state(U0)
    hs, Us = [], []
    for k in range(K):
        Us.append(split[0].clone())
        h = torch.empty(3, 1, device=DEV)
        na.baseline_adam_steps(z0, *split, prob, alph[0], 1, step0=k, lr=lr, hist=h)
        hs.append(h)
    hs = torch.cat(hs, 1)
    for a, b in zip(one, split):
        assert torch.equal(a, b)
    assert torch.equal(h1, hs)
    assert bool((hs[:, 1:] > hs[:, :-1]).any(1).all()), f"J is monotone for some start: {hs.tolist()}"
    U_k = torch.stack(Us, 1)                                                           # [B, K, nt, d]
    for k in range(K):
        assert torch.equal(hs[:, k], na.baseline_loss(z0, U_k[:, k], prob, alph[0])), k
    best, Ubest = one[3], one[4]
    for b in range(3):
        kmin = next(k for k in range(K) if hs[b, k] == hs[b].min())
        assert torch.equal(Ubest[b], U_k[b, kmin]), (b, kmin)
    assert torch.equal(best, hs.min(1).values)
    assert torch.equal(na.baseline_loss(z0, Ubest, prob, alph[0]), best)


def test_resume_keeps_or_replaces_best():
    name, nt = "swap12", 20
    alph = uo.BASE_ALPH[name]
    prob, xInit = uo.make_prob(name, alph, "train", DEV)
    z0 = xInit.reshape(1, -1).repeat(2, 1)
    U0 = na.baseline.initial_guess(z0, prob, nt, torch.Generator(device=DEV).manual_seed(4))
    J0 = na.baseline_loss(z0, U0, prob, alph[0])
    sentinel = torch.randn(U0.shape, generator=torch.Generator(device=DEV).manual_seed(8), device=DEV)
    # a finite best below every J of the run: Ubest stays
    st = _state(U0)
    hist = torch.empty(2, 5, device=DEV)
    low = torch.full((2,), 1.0, device=DEV)
    st[3], st[4] = low.clone(), sentinel.clone()
    na.baseline_adam_steps(z0, *st, prob, alph[0], 5, hist=hist)
    assert bool((hist > 1.0).all())
    assert torch.equal(st[3], low) and torch.equal(st[4], sentinel)
    # one above the first J: replaced by the first iterate
    st = _state(U0)
    st[3], st[4] = J0 * 2, sentinel.clone()
    na.baseline_adam_steps(z0, *st, prob, alph[0], 1)
    assert torch.equal(st[3], J0) and torch.equal(st[4], U0)
    # niters = 0: nothing moves
    st = _state(U0)
    st[3], st[4] = J0 * 2, sentinel.clone()
    before = [t.clone() for t in st]
    na.baseline_adam_steps(z0, *st, prob, alph[0], 0)
    for a, b in zip(st, before):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# batch forms, a large grid
# ---------------------------------------------------------------------------------------------------------------------------------
def test_broadcast_and_unbatched_forms():
    name, nt, B = "midcross4", 20, 4
    alph = uo.BASE_ALPH[name]
    prob, xInit = uo.make_prob(name, alph, "eval", DEV)
    d = xInit.numel()
    gen = torch.Generator().manual_seed(6)
    z0s, Us = _dev(xInit.cpu() + 0.3 * torch.randn(B, d, generator=gen), torch.randn(B, nt, d, generator=gen))

    def full(z, U):
        J, g = na.baseline_loss(z, U, prob, alph[0], grad=True)
        rep, tr = na.baseline_report(z, U, prob, alph[0])
        return J, g, rep, tr
    # z0 [d] against U [B, nt, d]
    got = full(xInit, Us)
    want = full(xInit.reshape(1, -1).expand(B, d).contiguous(), Us)
    assert got[0].shape == (B,) and got[1].shape == (B, nt, d) and got[2].shape == (B, 5) and got[3].shape == (B, d, nt + 1)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    # z0 [B, d] against U [nt, d]
    got = full(z0s, Us[0])
    want = full(z0s, Us[0:1].expand(B, nt, d).contiguous())
    assert got[0].shape == (B,) and all(torch.equal(a, b) for a, b in zip(got, want))
    # unbatched: 0-d objective, no batch dimension anywhere
    got = full(z0s[1], Us[1])
    assert got[0].dim() == 0 and got[1].shape == (nt, d) and got[2].shape == (5,) and got[3].shape == (d, nt + 1)
    want = full(z0s, Us)
    assert all(torch.equal(a, b[1]) for a, b in zip(got, want))


def test_3000_starts_at_the_largest_footprint():
    """swarm50 at its adam limit (1024 threads, the largest LDS use): one eval launch and a 2-iteration Adam launch over 3000 starts;
    rows equal their single-start launches bit for bit"""
    name = "swarm50"
    nt = uo.nt_limits(name)[1]
    alph = uo.BASE_ALPH[name]
    prob, xInit = uo.make_prob(name, alph, "train", DEV)
    d, B = xInit.numel(), 3000
    gen = torch.Generator().manual_seed(12)
    z0 = xInit.cpu() + 0.3 * torch.randn(B, d, generator=gen)
    U = (prob.xtarget.cpu().reshape(-1) - z0).unsqueeze(1) + 0.5 * torch.randn(B, nt, d, generator=gen)
    z0, U = _dev(z0, U)
    J, g = na.baseline_loss(z0, U, prob, alph[0], grad=True)
    rep, tr = na.baseline_report(z0, U, prob, alph[0])
    st = _state(U)
    hist = torch.empty(B, 2, device=DEV)
    na.baseline_adam_steps(z0, *st, prob, alph[0], 2, hist=hist)
    assert bool(torch.isfinite(J).all()) and bool(torch.isfinite(st[0]).all())
    for r in (0, 1, 255, 256, 1023, 1024, 2999):
        j1, g1 = na.baseline_loss(z0[r:r + 1], U[r:r + 1], prob, alph[0], grad=True)
        rep1, tr1 = na.baseline_report(z0[r:r + 1], U[r:r + 1], prob, alph[0])
        assert torch.equal(j1[0], J[r]) and torch.equal(g1[0], g[r]) and torch.equal(rep1[0], rep[r]) and torch.equal(tr1[0], tr[r]), r
        s1 = _state(U[r:r + 1])
        h1 = torch.empty(1, 2, device=DEV)
        na.baseline_adam_steps(z0[r:r + 1], *s1, prob, alph[0], 2, hist=h1)
        assert torch.equal(h1[0], hist[r]), r
        for a, b in zip(s1, st):
            assert torch.equal(a[0], b[r]), r
