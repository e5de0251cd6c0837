// nocf_bwd.inc -- the backward of the rollout: exact gradient of the DISCRETE scheme (discretise-then-optimise),
// what trainOC.py:172-173 obtains with Jc.backward() through the unrolled RK4 graph (SURVEY.md 8f row 1).
//
// For every RK evaluation, latest first, the kernel re-runs grad Phi at the recorded stage input s (forward
// kernel, RollArgs::sAll), forms the cotangent of the right-hand side from the RK4 adjoint recurrences and
// pushes it back through the physics and through grad Phi.  The vector-Jacobian product of grad Phi is four
// more GEMM phases on the SAME packed images as the forward sweep:
// (shown for nTh = 2; phi_vjp states the general recurrences)
//     ybar = K0 gbar        (opening image)       abar = tanh(o).ybar ,  tau0bar = a.ybar
//     vbar = K1 abar        (forward image)       qbar = (1-tanh(q)^2) . w . vbar
//     u0bar = K1' qbar      (backward image)      obar = tanh(o).u0bar + (1-tanh(o)^2).tau0bar
//     sbar = K0' obar + A'A gbar   (closing image)
// Parameter gradients are sums of outer products over all samples and evaluations,
//     dK0 = sum y gbar' + obar s' ,  dK1 = sum v abar' + qbar u0' ,  db0 = sum obar , db1 = sum qbar ,
//     dw = sum abar + tanh(q).vbar ,  dc = sum gbar ,  d(A'A) = sum gbar s'
// so the kernel only STREAMS the per-evaluation rows (y, obar, v, abar, qbar, u0, dw-row, gbar, s) to HBM --
// ~15 KB per sample and evaluation, 5 GB for swarm50, sized for a 288 GB device -- and the host contracts them
// with plain library GEMMs (torch.matmul -> hipBLASLt): [m x N][N x m] with N = n*(4 nt + 2) rows.
// any depth nTh >= 2 that fits the LDS; Cross2D, SwarmTraj, Quadcopter.

struct BwdArgs {
    const float* sAll;            // [nt*nstage][n][d+1] stage inputs recorded by the forward launch
    const float* zT;              // [n][d+4] final z of the forward launch
    const float* hs;              // [nt] fp32 step sizes exactly as the forward launch used them
    long n;
    int nt, nstage;
    float t1;
    float a0, a3, a4, a5, inv_n;  // alph[0,3,4,5] and 1/(global batch size)
    float *Y, *Ob, *Wb;                         // [Nrows][m] row streams
    float *V, *Ab, *Qb, *U0;                    // [nTh-1][Nrows][m]: per residual layer
    long lstride;                               // Nrows*m
    float *Gb, *Sx;                             // [Nrows][d+1]
    float* PHIb;                                // [n]   cotangent of Phi(x_T, t1)
    float* lam0;                                // [n][d] dJc/dx0 (nullable)
    // optional activation record of the forward launch (RollArgs::act): when given (two-layer networks, the split-role forward) the
    // kernel loads u0, tanh(o), tanh(q), a and grad Phi of every RK evaluation instead of re-running grad Phi's forward sweep -- four of
    // its eight GEMM phases per evaluation and the 2.6 MB of weights they stream
    const float* act; long actRows;
    float* gpart; long gstride;                 // nocf_mono_bwd.inc: one partial gradient vector per workgroup
    // value_only (nocf_phi_value_bwd_f32): no rollout -- nt = 0, sAll holds the n points s = [x, t], PHIb is an INPUT (the cotangent of Phi(s));
    // the kernel writes the value rows of the parameter gradients (src/Phi.py:91-96 under autograd) and nothing else that matters
    int value_only;
    // value_only == 2 (nocf_phi_grad_bwd_f32): the vector-Jacobian product of grad Phi alone -- nt = 0, sAll the n points, gbar_in [n][d+1] the
    // cotangent of grad Phi(s) (src/Phi.py:99-138 under autograd); sbar_out [n][d+1] = (d grad Phi / d s)' gbar, the rows of the first block
    // carry the parameter gradients
    const float* gbar_in; float* sbar_out;
    // state-only instantiations (STATES, nocf_rollout_bwd_states_f32): [nt][n][d] (nullable), the state cotangent LAM when the last stage of
    // step k begins = dJ/dW[k] of a disturbed rollout (z_{k+1} = step(z_k) + W[k]); lamW[nt-1] is the terminal cotangent dJ/dx(T).
    // STATES is a mode: 0 full, 1 state-only, 2 joint (nocf_rollout_bwd_*_w_f32: mode 0's statements plus this store)
    float* lamW;
    // weighted instantiations (RW, nocf_rollout_bwd_*_rw_f32): [n], one weight per sample, standing where inv_n stands for that sample's
    // cotangent seeds (LAM, gbar, phib, kL / kh); read by those instantiations only (the last field: no existing offset moves)
    const float* wrow;
};

// d(raw obstacle cost of agent a)/dx at the sample x, added into gq[3]: the per-agent math of physics_xgrad's obstacle part
// (Cross2D.py:89-125, SwarmTraj.py:89-125), shared with the baseline kernels (nocf_baseline.inc).  The caller decides when the
// train-mode masks apply (treated as constants, like autograd does): the baseline also calls it for eval-mode softcorridor, whose
// cost does not depend on the mode.  A macro, not an inline function: physics_xgrad then compiles token for token as before (an
// inlined call changed the register allocation of the adjoint kernels).
#define NOCF_OBSTACLE_XGRAD(pb, x, a, gq) \
{ \
    if (pb.kind == NOCF_PROB_CROSS2D) { \
        const float x0 = x[2 * a], x1 = x[2 * a + 1]; \
        if (pb.obstacle == NOCF_OBS_SOFTCORRIDOR) { \
            const float cov = 0.2f, denom = (float)TWO_PI_D * sqrtf(cov * cov); \
            const float mus[4] = {-2.5f, 2.5f, -1.5f, 1.5f}; \
            _Pragma("unroll") \
            for (int k = 0; k < 4; ++k) { \
                const float pdf = gauss2(x0, x1, mus[k], 0.f, cov, denom); \
                gq[0] -= pdf * (x0 - mus[k]) / cov; \
                gq[1] -= pdf * x1 / cov; \
            } \
        } else if (pb.obstacle == NOCF_OBS_HARDCORRIDOR) { \
            const float denom = (float)TWO_PI_D; \
            const float n1 = sqrtf(x0 * x0 + (x1 - 4.f) * (x1 - 4.f)), n2 = sqrtf(x0 * x0 + (x1 + 3.5f) * (x1 + 3.5f)); \
            const float th2 = (float)(2.0 + pb.r); \
            if (n1 < th2 || n2 < th2) { \
                const float p1 = gauss2(x0, x1, 0.f, 4.f, 1.f, denom), p2 = gauss2(x0, x1, 0.f, -3.5f, 1.f, denom); \
                gq[0] = -(p1 + p2) * x0; \
                gq[1] = -p1 * (x1 - 4.f) - p2 * (x1 + 3.5f); \
            } \
        } \
    } else if (pb.kind == NOCF_PROB_SWARMTRAJ && pb.obstacle == NOCF_OBS_BLOCKS && pb.alphQ > 0.0) { \
        const float x0 = x[3 * a], x1 = x[3 * a + 1], x2 = x[3 * a + 2]; \
        if (obstacle_swarm(pb, x0, x1, x2) != 0.f) {      /* inside an inflated block (the +999 offset has no gradient) */ \
            const float c15 = (float)15.749609945722419; \
            const float den1 = c15 * sqrtf(243.f), den2 = c15 * sqrtf(81.f); \
            const float e2 = x2 - 2.f, f0 = x0 - 2.5f; \
            const float q1 = expf(-0.5f * (((x0 * x0) / 9.f + (x1 * x1) / 3.f) + (e2 * e2) / 9.f)) / den1; \
            const float q2 = expf(-0.5f * (((f0 * f0) / 9.f + (x1 * x1) / 3.f) + (e2 * e2) / 3.f)) / den2; \
            gq[0] = -q1 * x0 / 9.f - q2 * f0 / 9.f; \
            gq[1] = -q1 * x1 / 3.f - q2 * x1 / 3.f; \
            gq[2] = -q1 * e2 / 9.f - q2 * e2 / 3.f; \
        } \
    } \
}

// d(alphQ*Q + alphW*W)/dx of the point-agent problems for the T samples in SB, scaled per sample by coef[t],
// into XD[t][0..d).  Train-mode masks are treated as constants, like autograd does with the reference.
// The interaction part walks all (a, b) pairs: PD (coordinates per agent) is a template parameter so the
// difference vector stays in registers, and the b-range of every agent is split over SPL adjacent lanes whose
// partial forces are added with a fixed-order lane exchange (deterministic).
template <int PD>
__device__ __forceinline__ void pair_force(const float* x, int a, int b0, int b1, float thr, float den, float inv_r2, bool excl1,
                                           float (&gw)[3]) {
    float xa[PD];
#pragma unroll
    for (int k = 0; k < PD; ++k) xa[k] = x[PD * a + k];
    const float thr2 = thr * thr * 1.000002f;           // cheap reject (most pairs are far apart); the exact test follows
    for (int bb = b0; bb < b1; bb += 5) {               // five partners per turn: their LDS reads are issued together
        float e[5][PD], s2[5];
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            const int b = (bb + u < b1) ? bb + u : a;   // out-of-range slots alias the agent itself (distance 0, skipped)
            float q = 0.f;
#pragma unroll
            for (int k = 0; k < PD; ++k) { e[u][k] = xa[k] - x[PD * b + k]; q += e[u][k] * e[u][k]; }
            s2[u] = (b == a) ? 3.0e38f : q;
        }
#pragma unroll
        for (int u = 0; u < 5; ++u) {
            if (s2[u] < thr2) {
                const float dist = sqrtf(s2[u]);
                if (dist < thr) {
                    const float w = expf(-(dist * dist) / den);
                    if (!excl1 || w != 1.f) {            // N > 2: entries equal to 1 are dropped by calcW (Cross2D.py:156-158)
#pragma unroll
                        for (int k = 0; k < PD; ++k) gw[k] -= w * e[u][k] * inv_r2;
                    }
                }
            }
        }
    }
}

__device__ void physics_xgrad(const Ctx& c, const DevPlan& pl, const DevProb& pb, const float* coef, int cstride) {
    const int T = pl.T, N = pb.nAgents, ad = pb.agentDim;
    const int Gsz = c.nthreads / T;
    const int t = c.tid / Gsz, j0 = c.tid - t * Gsz;
    const float* x = lds + pl.lSB + t * pl.LDs;
    float* xd = lds + pl.lXD + t * pl.ZLD;
    const float cf = coef[t * cstride];
    const bool wantW = want_W(pb) && N >= 2;
    const float den = (float)(2.0 * pb.r * pb.r);
    const float inv_r2 = 1.f / ((float)pb.r * (float)pb.r);
    const double fac = pb.training ? (N == 2 ? 2.2 : (pb.kind == NOCF_PROB_SWARMTRAJ ? 3.2 : 2.2)) : 2.0;
    const float thr = (float)(fac * pb.r);
    const float aQ = (float)pb.alphQ, aW = (float)pb.alphW;
    // how many adjacent lanes share one agent's b-loop (power of two, as many as the group can seat)
    int SPL = 1;
    while (wantW && SPL < 8 && 2 * SPL * N <= Gsz && SPL * 4 < N) SPL *= 2;
    // obstacle part (one thread per agent) seeds XD; the barrier orders it before the interaction part adds to it
    for (int a = j0; a < N; a += Gsz) {
        float gq[3] = {0.f, 0.f, 0.f};
        // (eval mode: the hard corridor and the blocks are masks without a gradient; the soft corridor's Gaussians are the train-mode ones)
        if ((pb.training && pb.obstacle != NOCF_OBS_NONE) || pb.obstacle == NOCF_OBS_SOFTCORRIDOR) NOCF_OBSTACLE_XGRAD(pb, x, a, gq)
        if (ad == 2) { xd[2 * a] = cf * aQ * gq[0]; xd[2 * a + 1] = cf * aQ * gq[1]; }
        else { xd[3 * a] = cf * aQ * gq[0]; xd[3 * a + 1] = cf * aQ * gq[1]; xd[3 * a + 2] = cf * aQ * gq[2]; }
    }
    if (!wantW) return;
    __syncthreads();
    for (int q0 = 0; q0 < N * SPL; q0 += Gsz) {
        const int q = q0 + j0;
        const bool live = q < N * SPL;
        const int a = live ? q / SPL : 0, part = q - a * SPL;
        const int b0 = live ? (N * part) / SPL : 0, b1 = live ? (N * (part + 1)) / SPL : 0;
        float gw[3] = {0.f, 0.f, 0.f};
        if (ad == 2) pair_force<2>(x, a, b0, b1, thr, den, inv_r2, N > 2, gw);
        else pair_force<3>(x, a, b0, b1, thr, den, inv_r2, N > 2, gw);
#pragma unroll
        for (int k = 0; k < 3; ++k) gw[k] = sum_seg(gw[k], SPL);
        if (live && part == 0) {
            const float sc = cf * aW;
            if (ad == 2) { xd[2 * a] += sc * gw[0]; xd[2 * a + 1] += sc * gw[1]; }
            else { xd[3 * a] += sc * gw[0]; xd[3 * a + 1] += sc * gw[1]; xd[3 * a + 2] += sc * gw[2]; }
        }
    }
}

// Quadcopter (Quadcopter.py:65-113): cotangents of one evaluation through the thrust/rotation physics.  With
//   F = -grad_p H (the state derivative), l_a = 2 + u_a^2 + |p_9:12|^2/4, h_a = -v.p_0:3 - w.p_3:6 + 2 u_a^2 + g p_8 + |p_9:12|^2/2
// the evaluation contributes  fbar.F + sum_a cl_a l_a + ch sum_a h_a  where the reference's running-L loop
// (Quadcopter.py:98-110: H -= L with L still accumulating) counts l_a (N - a) times in H:
//   cl_a = kL + e kh (N - a),  ch = -e kh.   Writes GB[0..d) (cotangent of p) and XD[0..d) (direct x term).
__device__ void quad_adjoint(const Ctx& c, const DevPlan& pl, const DevProb& pb, float hs, float wst, float cpl, const float* SCB) {
    const int T = pl.T, N = pb.nAgents;
    const float M = (float)pb.mass, grav = (float)pb.grav;
    const float mh = (float)(-1.0 / (2.0 * pb.mass));
    for (int idx = c.tid; idx < T * N; idx += c.nthreads) {
        const int t = idx / N, a = idx - t * N;
        const float* xa = lds + pl.lSB + t * pl.LDs + 12 * a;
        const float* pa = lds + pl.lG + t * pl.GLD + 12 * a;
        const float* lam = lds + pl.lLAM + t * pl.ZLD + 12 * a;
        const float* xp = lds + pl.lXP + t * pl.ZLD + 12 * a;
        float* gb = lds + pl.lGB + t * pl.LDs + 12 * a;
        float* xd = lds + pl.lXD + t * pl.ZLD + 12 * a;
        const float* tr = lds + pl.lTRIG + (t * N + a) * 6;
        const float kL = SCB[t * 4 + 0], ekh = SCB[t * 4 + 1];
        const float cl = kL + ekh * (float)(N - a), ch = -ekh;
        float fb[12];
        for (int k = 0; k < 12; ++k) fb[k] = hs * (wst * lam[k] + cpl * xp[k]);
        const float sps = tr[0], sth = tr[1], sph = tr[2], cps = tr[3], cth = tr[4], cph = tr[5];
        const float f7 = sps * sph + cps * sth * cph, f8 = -cps * sph + sps * sth * cph, f9 = cth * cph;
        const float u = mh * (f7 * pa[6] + f8 * pa[7] + f9 * pa[8]);
        const float fu = (fb[6] * f7 + fb[7] * f8 + fb[8] * f9) / M;
        const float ku = fu + (2.f * cl + 4.f * ch) * u;              // d/du of the contribution at fixed rotation
        for (int k = 0; k < 6; ++k) { gb[k] = -ch * xa[6 + k]; xd[6 + k] = fb[k] - ch * pa[k]; }
        gb[6] = ku * mh * f7; gb[7] = ku * mh * f8; gb[8] = ku * mh * f9 + ch * grav;
        for (int k = 9; k < 12; ++k) gb[k] = -0.5f * fb[k] + (0.5f * cl + ch) * pa[k];
        const float a7 = ku * mh * pa[6] + u * fb[6] / M, a8 = ku * mh * pa[7] + u * fb[7] / M, a9 = ku * mh * pa[8] + u * fb[8] / M;
        xd[0] = 0.f; xd[1] = 0.f; xd[2] = 0.f;
        xd[3] = -a7 * f8 + a8 * f7;                                                              // d/dpsi
        xd[4] = a7 * cps * cth * cph + a8 * sps * cth * cph - a9 * sth * cph;                    // d/dtheta
        xd[5] = a7 * (sps * cph - cps * sth * sph) + a8 * (-cps * cph - sps * sth * sph) - a9 * cth * sph;   // d/dphi
    }
    __syncthreads();
    if (N == 2 && want_W(pb) && c.tid < T) {             // Quadcopter.py:139-143, mask constant
        const int t = c.tid;
        const float* x = lds + pl.lSB + t * pl.LDs;
        float* xd = lds + pl.lXD + t * pl.ZLD;
        float e[3], s2 = 0.f;
        for (int k = 0; k < 3; ++k) { e[k] = x[k] - x[12 + k]; s2 += e[k] * e[k]; }
        const float dist = sqrtf(s2), r = (float)pb.r;
        if (dist < (float)(2.0 * pb.r)) {
            const float w = expf(-(dist * dist) / (float)(2.0 * pb.r * pb.r));
            const float cw = (SCB[t * 4 + 0] + SCB[t * 4 + 1] * 2.f) * (float)pb.alphW;   // base L sits in both running sums
            for (int k = 0; k < 3; ++k) { const float g = -cw * w * e[k] / (r * r); xd[k] += g; xd[12 + k] -= g; }
        }
    }
}

// vector-Jacobian product of grad Phi at the point whose forward activations sit in LDS (phi_eval just ran on an
// adjoint plan, which keeps u_i, a_i, v_i, tanh of every layer).  With L = nTh-1 residual layers:
//   ybar = K0 gbar ;  abar_0 = tau_0.ybar ,  taubar_0 = a_0.ybar
//   i = 1..L :  vbar_i = hN K_i abar_{i-1} ;  taubar_i = a_i.vbar_i ,  abar_i = abar_{i-1} + tau_i.vbar_i      (abar_L = dw row)
//   i = L..1 :  qbar_i = (1-tau_i^2).taubar_i + hN tau_i.ubar_i  (ubar_L = 0) ;  ubar_{i-1} = ubar_i + K_i' qbar_i
//   obar = (1-tau_0^2).taubar_0 + tau_0.ubar_0 ;  sbar = K0' obar + A'A gbar
// in: GB[t][0..d] ; out: SBAR[t][0..d], and the row streams of this evaluation at global row `grow0 + t`
// (per layer i: hN v_i with abar_{i-1}, and qbar_i with u_{i-1}, at layer offset (i-1)*lstride).
// STATES == 1: no row stream is stored and no stream pointer is dereferenced (the state-only adjoint: SBAR is all the caller needs);
// 0 and 2 (full and joint) store them alike -- the joint mode's lamW store sits in rollout_bwd_body, not here.
template <int S, int STATES = 0>
__device__ void phi_vjp(const Ctx& c, const DevPlan& pl, Ring& rg, const BwdArgs& ba, long grow0, long nvalid) {
    const int T = pl.T, LD = pl.LD, m = pl.m, D1 = pl.D1, r = pl.r, L = pl.nTh - 1, TLD = pl.T * pl.LD;
    const float hN = pl.hN;
    const float* vec = lds + pl.lVEC - pl.ob0;
    const float* wv = vec + pl.ow;
    const float* Araw = vec + pl.oA;
    auto oTH = [&](int i) { return pl.lTH + i * TLD; };                       // tanh of layer i (0 = opening)
    auto oA = [&](int i) { return pl.lAV + (L - 1 - i) * TLD; };              // a_i, i < L   (a_L = w)
    auto oV = [&](int i) { return pl.lV0 + (L - i) * TLD; };                  // v_i ; v_0 = y
    auto oU = [&](int i) { return pl.lU0 + i * TLD; };                        // u_i
    auto oTB = [&](int i) { return pl.lT0B + i * TLD; };                      // taubar_i, i < L
    auto oAB = [&](int k) { return pl.lAB + k * TLD; };                       // abar_k, k < L (all kept: streamed at the end)
    auto oQB = [&](int k) { return pl.lQB + k * TLD; };                       // qbar_{L-k}, k < L
    const PhaseDesc phOpen = {pl.oW0f, pl.MB, pl.KQ1, pl.SK1, m};
    const PhaseDesc phClose = {pl.oW0b, pl.DB, pl.KQm, pl.SK6, D1};
    const PhaseDesc phNone = {0, 0, 0, 0, 0};
    auto phFwd = [&](int i) { return PhaseDesc{pl.oWf + (long)(i - 1) * pl.strideW, pl.MB, pl.KQm, pl.SKm, m}; };
    auto phBwd = [&](int i) { return PhaseDesc{pl.oWb + (long)(i - 1) * pl.strideW, pl.MB, pl.KQm, pl.SKm, m}; };
    // zb = A gbar (8 lanes per row), for the A'A gbar term
    {
        const int items = T * r * 8;
        for (int base = 0; base < items; base += c.nthreads) {
            const int id = base + c.tid;
            const int part = id & 7, tr = id >> 3;
            float acc = 0.f;
            if (id < items) {
                const int t = tr / r, rr = tr - t * r;
                for (int i = part; i < D1; i += 8) acc += Araw[rr * D1 + i] * lds[pl.lGB + t * pl.LDs + i];
            }
            acc = sum8(acc);
            if (id < items && part == 0) { const int t = tr / r; lds[pl.lZQB + t * ZQLD + (tr - t * r)] = acc; }
        }
    }
    TL(c, 54);
    // ybar = K0 gbar
    {
        const int oT0 = oTH(0), oA0 = oA(0), oab = oAB(0), otb = oTB(0);
        gemm_phase<S>(c, pl, rg, false, phOpen, phFwd(1), pl.lGB, pl.LDs, [&](int t, int col, float yb) {
            if (col < m) {
                lds[oab + t * LD + col] = lds[oT0 + t * LD + col] * yb;          // abar_0
                lds[otb + t * LD + col] = lds[oA0 + t * LD + col] * yb;          // taubar_0 = a_0 . ybar
            }
        });
        __syncthreads();
    }
    TL(c, 55);
    // vbar_i = hN K_i abar_{i-1}
    for (int i = 1; i <= L; ++i) {
        const int oin = oAB(i - 1), oout = oAB(i), oTi = oTH(i), oAi = (i < L) ? oA(i) : 0, otb = (i < L) ? oTB(i) : 0, oq = oQB(0);
        const bool last = (i == L);
        gemm_phase<S>(c, pl, rg, true, phFwd(i), last ? phBwd(L) : phFwd(i + 1), oin, LD, [&](int t, int col, float x) {
            if (col < m) {
                const float vb = hN * x, ti = lds[oTi + t * LD + col];
                const float ab = lds[oin + t * LD + col] + ti * vb;             // abar_i
                if (!last) {
                    lds[oout + t * LD + col] = ab;
                    lds[otb + t * LD + col] = lds[oAi + t * LD + col] * vb;     // taubar_i
                } else {
                    lds[oq + t * LD + col] = (1.f - ti * ti) * wv[col] * vb;    // qbar_L  (a_L = w, ubar_L = 0)
                    if constexpr (STATES != 1) { if (t < nvalid) ba.Wb[(grow0 + t) * m + col] = ab; }          // dw row
                }
            }
        });
        __syncthreads();
    }
    TL(c, 56);
    // ubar_{i-1} = ubar_i + K_i' qbar_i
    for (int i = L; i >= 1; --i) {
        const int oq = oQB(L - i), oqn = oQB(L - i + 1), oTp = oTH(i - 1), otb = oTB(i - 1), oub = pl.lUB, oob = pl.lOB;
        const bool top = (i == L), first = (i == 1);
        gemm_phase<S>(c, pl, rg, true, phBwd(i), first ? phClose : phBwd(i - 1), oq, LD, [&](int t, int col, float x) {
            if (col < m) {
                const float ub = top ? x : x + lds[oub + t * LD + col];
                const float tp = lds[oTp + t * LD + col], tb = lds[otb + t * LD + col];
                if (!first) {
                    lds[oub + t * LD + col] = ub;
                    lds[oqn + t * LD + col] = (1.f - tp * tp) * tb + hN * tp * ub;      // qbar_{i-1}
                } else {
                    lds[oob + t * LD + col] = (1.f - tp * tp) * tb + tp * ub;           // obar
                }
            }
        });
        __syncthreads();
    }
    TL(c, 57);
    // sbar = K0' obar + A'(A gbar)
    gemm_phase<S>(c, pl, rg, true, phClose, phNone, pl.lOB, LD, [&](int t, int i, float sb) {
        if (i < D1) {
            for (int q = 0; q < r; ++q) sb += Araw[q * D1 + i] * lds[pl.lZQB + t * ZQLD + q];
            lds[pl.lSBAR + t * pl.GLD + i] = sb;
        }
    });
    __syncthreads();
    TL(c, 58);
    if constexpr (STATES != 1) {
    // row streams of this evaluation (coalesced rows), after the last phase: nothing here competes with a weight prefetch
    const int oy = oV(0);
    // the m-wide streams go out as 16-B pieces (one float4 per lane and stream: a quarter of the store instructions of a
    // float-per-lane sweep, 1 KiB per wave and instruction); rows of d+1 floats are not 16-B aligned and stay scalar
    int lay = m | LD | oy | pl.lOB;
    for (int i = 1; i <= L; ++i) lay |= oV(i) | oAB(i - 1) | oQB(L - i) | oU(i - 1);
    const bool vec4 = (lay & 3) == 0 && ((reinterpret_cast<size_t>(ba.Y) | reinterpret_cast<size_t>(ba.Ob) | reinterpret_cast<size_t>(ba.V) |
                                          reinterpret_cast<size_t>(ba.Ab) | reinterpret_cast<size_t>(ba.Qb) | reinterpret_cast<size_t>(ba.U0)) & 15) == 0;
    if (vec4) {
        const int m4 = m >> 2;
        const float4* L4 = reinterpret_cast<const float4*>(lds);
        const int tv = (int)(nvalid < T ? nvalid : T);
        for (int idx = c.tid; idx < tv * m4; idx += c.nthreads) {
            const int t = idx / m4, c4 = idx - t * m4;
            const long ro = (grow0 + t) * m4 + c4;                       // float4 index in a [rows][m] stream
            const int lo4 = (t * LD) / 4 + c4;
            reinterpret_cast<float4*>(ba.Y)[ro] = L4[oy / 4 + lo4];
            reinterpret_cast<float4*>(ba.Ob)[ro] = L4[pl.lOB / 4 + lo4];
            for (int i = 1; i <= L; ++i) {
                const long lo = ((long)(i - 1) * ba.lstride) / 4 + ro;
                float4 v = L4[oV(i) / 4 + lo4];
                v.x *= hN; v.y *= hN; v.z *= hN; v.w *= hN;
                reinterpret_cast<float4*>(ba.V)[lo] = v;
                reinterpret_cast<float4*>(ba.Ab)[lo] = L4[oAB(i - 1) / 4 + lo4];
                reinterpret_cast<float4*>(ba.Qb)[lo] = L4[oQB(L - i) / 4 + lo4];
                reinterpret_cast<float4*>(ba.U0)[lo] = L4[oU(i - 1) / 4 + lo4];
            }
        }
    }
    for (int t = 0; t < T && t < nvalid; ++t) {
        const long row = grow0 + t;
        if (!vec4)
            for (int col = c.tid; col < m; col += c.nthreads) {
                ba.Y[row * m + col] = lds[oy + t * LD + col];
                ba.Ob[row * m + col] = lds[pl.lOB + t * LD + col];
                for (int i = 1; i <= L; ++i) {
                    const long lo = (long)(i - 1) * ba.lstride + row * m + col;
                    ba.V[lo] = hN * lds[oV(i) + t * LD + col];
                    ba.Ab[lo] = lds[oAB(i - 1) + t * LD + col];
                    ba.Qb[lo] = lds[oQB(L - i) + t * LD + col];
                    ba.U0[lo] = lds[oU(i - 1) + t * LD + col];
                }
            }
        for (int i = c.tid; i < D1; i += c.nthreads) {
            ba.Gb[row * D1 + i] = lds[pl.lGB + t * pl.LDs + i];
            ba.Sx[row * D1 + i] = lds[pl.lSB + t * pl.LDs + i];
        }
    }
    }
}

// RW (STATES = 0; nocf_rollout_bwd_act_rw_f32): the per-sample weight ba.wrow[row] stands where ba.inv_n stands at the four cotangent seeds
// below (LAM, GB, phib, kL / kh); a tail row, which replicates a valid sample, takes weight 0.  The three seeds of the terminal evaluation load
// it per row from global memory, once.  The kL seed recurs in every RK evaluation, where a global load put one memory latency into each of them
// (1.3 % of swarm50's adjoint, profiles/risk), and four registers held across the loop cost spills: the per-sample LDS slot SC[t][3], which
// carries e_f through the terminal evaluation and is idle afterwards, keeps the weight instead -- written at the end of the terminal
// evaluation by the thread that reads it at every kL site.  Every RW test is a compile-time choice at its place of use: the other
// instantiations keep their statements.
template <int S, int STATES = 0, bool RW = false>
__device__ __forceinline__ void rollout_bwd_body(const DevPlan& pl, const DevPlan* __restrict__ plp, const DevProb& pb,
                                                 const float* __restrict__ ws, const BwdArgs& ba) {
    Ctx c;
    ctx_init(c, ws, (unsigned)(pl.oPlan * 4));
    c.cb = plp->cb;
    const int T = pl.T, d = pl.d, D1 = pl.D1, ZLD = pl.ZLD, m = pl.m, LD = pl.LD;
    const long row0 = (long)blockIdx.x * T;
    const long nvalid = (ba.n - row0 < T) ? (ba.n - row0) : T;
    float* SB = lds + pl.lSB;
    float* GB = lds + pl.lGB;
    float* LAM = lds + pl.lLAM;          // dJ/dx of the current step boundary
    float* XS = lds + pl.lXS;            // sum of the stage contributions of this step
    float* XP = lds + pl.lXP;            // xbar of the stage evaluated just before (i.e. the later stage)
    float* XD = lds + pl.lXD;            // direct physics term
    const float* G = lds + pl.lG;
    const float* SBAR = lds + pl.lSBAR;
    float* SC = lds + pl.lSCB;           // per-sample scalars: [t*4+0]=coef, +1 = e*kh, +2 = kL - e*kh, +3 = e_f
    const bool quad = (pb.kind == NOCF_PROB_QUADCOPTER);
    Ring rg;
    bool ring_ready = false;

    for (int i = c.tid; i < pl.ldsFloats; i += c.nthreads) lds[i] = 0.f;
    __syncthreads();
    load_vectors(c, pl);
    // One loop over the evaluations, latest first, so that phi_eval and phi_vjp have ONE call site each (two would
    // double the code and, once the compiler stops inlining them, put the weight ring in scratch memory):
    // ev == total is the terminal evaluation (costs G, HJfin, HJgrad, src/OCflow.py:58-90), ev < total the RK stages.
    const float c16 = (float)(1.0 / 6.0), c26 = (float)(2.0 / 6.0);
    const long total = (long)ba.nt * ba.nstage;
    for (long ev = total; ev >= 0; --ev) {
        const bool gmode = ba.value_only == 2;
        const bool fin = (ev == total) && !gmode;
        const int k = fin ? ba.nt : (int)(ev / ba.nstage), st = fin ? 0 : (int)(ev - (long)k * ba.nstage);
        const float hs = (fin || gmode) ? 0.f : ba.hs[k];
        // weight of this stage in z_{k+1}, and how the LATER stage's input depended on this stage's K
        float wst = 1.f, cpl = 0.f;
        if (ba.nstage != 1) { wst = (st == 0 || st == 3) ? c16 : c26; cpl = (st == 3) ? 0.f : (st == 2 ? 1.f : 0.5f); }
        if (fin && ba.value_only) {
            for (int j = c.tid; j < T * D1; j += c.nthreads) {
                const int t = j / D1, i = j - t * D1;
                long row = row0 + t; if (row >= ba.n) row = ba.n - 1;
                SB[t * pl.LDs + i] = ba.sAll[row * D1 + i];
            }
        } else if (fin) {
            for (int j = c.tid; j < T * d; j += c.nthreads) {
                const int t = j / d, i = j - t * d;
                long row = row0 + t; if (row >= ba.n) row = ba.n - 1;
                SB[t * pl.LDs + i] = ba.zT[row * (d + 4) + i];
            }
            if (c.tid < T) SB[c.tid * pl.LDs + d] = ba.t1;
        } else {
            if constexpr (STATES != 0) {
                if (st == ba.nstage - 1 && ba.lamW)
                    for (int j = c.tid; j < T * d; j += c.nthreads) {
                        const int t = j / d, i = j - t * d;
                        if (t < nvalid) ba.lamW[((long)k * ba.n + row0 + t) * d + i] = LAM[t * ZLD + i];
                    }
            }
            if (st == ba.nstage - 1)
                for (int j = c.tid; j < T * d; j += c.nthreads) { const int t = j / d, i = j - t * d; XS[t * ZLD + i] = 0.f; XP[t * ZLD + i] = 0.f; }
            const float* src = ba.sAll + (ev * ba.n) * D1;
            for (int j = c.tid; j < T * D1; j += c.nthreads) {
                const int t = j / D1, i = j - t * D1;
                long row = row0 + t; if (row >= ba.n) row = ba.n - 1;
                SB[t * pl.LDs + i] = src[row * D1 + i];
            }
        }
        __syncthreads();
#ifdef NOCF_STAMPS
        c.tl = (ba.lam0 == nullptr && ba.PHIb && blockIdx.x == 7 && ev == total - 160 && g_tl_dev) ? g_tl_dev : nullptr;
#endif
        TL(c, 38);
        if (!fin && ba.act && pl.nTh == 2) {
            // forward activations of this evaluation from the record (what phi_eval leaves in LDS on an adjoint plan): u0, tanh(o),
            // tanh(q), a_0 (= w + hN K1' v), v_1 = tanh(q).w, v_0 = y = tanh(o).a_0, grad Phi; z = A s is recomputed (r dot products)
            const float* wv = lds + pl.lVEC - pl.ob0 + pl.ow;
            const long M4 = pl.m >> 2, sec = ba.actRows * pl.m;
            const int TLDa = T * LD;
            for (int jx = c.tid; jx < T * (int)M4; jx += c.nthreads) {
                const int t = jx / (int)M4, c4 = jx - t * (int)M4;
                long row = row0 + t; if (row >= ba.n) row = ba.n - 1;
                const float4* src = reinterpret_cast<const float4*>(ba.act + (ev * ba.n + row) * pl.m) + c4;
                const float4 u = src[0], t0 = src[sec >> 2], t1 = src[2 * (sec >> 2)], a = src[3 * (sec >> 2)];
                const int o = t * LD + 4 * c4;
                const float uu[4] = {u.x, u.y, u.z, u.w}, t0v[4] = {t0.x, t0.y, t0.z, t0.w}, t1v[4] = {t1.x, t1.y, t1.z, t1.w}, av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    lds[pl.lU0 + o + q] = uu[q];
                    lds[pl.lTH + o + q] = t0v[q];
                    lds[pl.lTH + TLDa + o + q] = t1v[q];
                    lds[pl.lAV + o + q] = av[q];
                    lds[pl.lV0 + o + q] = t1v[q] * wv[4 * c4 + q];
                    lds[pl.lV0 + TLDa + o + q] = t0v[q] * av[q];
                }
            }
            const float* gsrc = ba.act + 4 * sec;
            for (int jx = c.tid; jx < T * D1; jx += c.nthreads) {
                const int t = jx / D1, i = jx - t * D1;
                long row = row0 + t; if (row >= ba.n) row = ba.n - 1;
                lds[pl.lG + t * pl.GLD + i] = gsrc[(ev * ba.n + row) * D1 + i];
            }
            z_from_s(pl, c.tid, c.nthreads);
            ring_ready = false;
            __syncthreads();
        } else {
            phi_eval<S>(c, pl, fin, rg, ring_ready, false);
        }
        TL(c, 39);
        if (fin && ba.value_only) {
            for (int j = c.tid; j < T * d; j += c.nthreads) {
                const int t = j / d, i = j - t * d;
                LAM[t * ZLD + i] = 0.f; GB[t * pl.LDs + i] = 0.f; XD[t * ZLD + i] = 0.f;
            }
            if (c.tid < T) { GB[c.tid * pl.LDs + d] = 0.f; SC[c.tid * 4 + 3] = 0.f; }
            __syncthreads();
        } else if (fin) {
            const int Gsz = c.nthreads / T;
            const int t = c.tid / Gsz, j0 = c.tid - t * Gsz;
            float v[1] = {0.f};
            for (int i = j0; i < d; i += Gsz) { const float res = SB[t * pl.LDs + i] - pb.xtarget[i]; v[0] += res * res; }
            group_reduce<1>(c, pl, v);
            if (c.tid < T) {
                const float cG = 0.5f * group_total<1>(c, pl, c.tid, 0);
                const float dd = lds[pl.lPHI + c.tid] - ba.a0 * cG;
                SC[c.tid * 4 + 3] = (dd > 0.f) ? 1.f : (dd < 0.f ? -1.f : 0.f);          // e_f = sign(Phi1 - a0 cG)
            }
            __syncthreads();
            for (int j = c.tid; j < T * d; j += c.nthreads) {
                const int t = j / d, i = j - t * d;
                const float res = SB[t * pl.LDs + i] - pb.xtarget[i];
                const float gi = G[t * pl.GLD + i];
                const float dg = gi - ba.a0 * res;
                const float eg = (dg > 0.f) ? 1.f : (dg < 0.f ? -1.f : 0.f);
                const float ef = SC[t * 4 + 3];
                float wI = 0.f;
                if constexpr (RW) { if (t < nvalid) wI = ba.wrow[row0 + t]; }
                LAM[t * ZLD + i] = (RW ? wI : ba.inv_n) * (ba.a0 * res + ba.a4 * ef * dg - ba.a5 * ba.a0 * eg);
                GB[t * pl.LDs + i] = (RW ? wI : ba.inv_n) * ba.a5 * eg;
                XD[t * ZLD + i] = 0.f;
            }
            if (c.tid < T) GB[c.tid * pl.LDs + d] = 0.f;
            __syncthreads();
        }
        if (fin) {
            if constexpr (STATES != 1) {
            // value rows: the cotangent of Phi1 reuses the forward quantities: ubar_i = phib a_i, so
            // qbar_i = phib hN v_i, obar = phib y, dw row = phib u_L  (no extra GEMM)
            const long vrow0 = (total + 1) * ba.n + row0;
            const int Lr = pl.nTh - 1, TLD = T * LD;
            for (int t = 0; t < T; ++t) {
                if (t >= nvalid) break;
                const float phib = ba.value_only ? ba.PHIb[row0 + t] : (RW ? ba.wrow[row0 + t] : ba.inv_n) * ba.a4 * SC[t * 4 + 3];
                const long row = vrow0 + t;
                for (int col = c.tid; col < m; col += c.nthreads) {
                    for (int i = 1; i <= Lr; ++i) {
                        const long lo = (long)(i - 1) * ba.lstride;
                        ba.Qb[lo + row * m + col] = phib * pl.hN * lds[pl.lV0 + (Lr - i) * TLD + t * LD + col];
                        ba.U0[lo + row * m + col] = lds[pl.lU0 + (i - 1) * TLD + t * LD + col];
                    }
                    ba.Ob[row * m + col] = phib * lds[pl.lV0 + Lr * TLD + t * LD + col];
                    ba.Wb[row * m + col] = phib * lds[pl.lU0 + Lr * TLD + t * LD + col];
                }
                for (int i = c.tid; i < D1; i += c.nthreads) ba.Sx[row * D1 + i] = SB[t * pl.LDs + i];
                if (c.tid == 0 && !ba.value_only) ba.PHIb[row0 + t] = phib;
            }
            }
        } else if (gmode) {
            for (int j = c.tid; j < T * D1; j += c.nthreads) {
                const int t = j / D1, i = j - t * D1;
                GB[t * pl.LDs + i] = (t < nvalid) ? ba.gbar_in[(row0 + t) * D1 + i] : 0.f;
                if (i < d) XD[t * ZLD + i] = 0.f;
            }
            __syncthreads();
        } else {
            physics_sums(c, pl, pb);
            TL(c, 45);
            if (c.tid < T) {
                const int s = c.tid;
                const Costs cs = physics_finish(c, pl, pb, s);
                const float dh = G[s * pl.GLD + d] - cs.H;
                const float eh = (dh > 0.f) ? 1.f : (dh < 0.f ? -1.f : 0.f);
                const float wI = RW ? SC[s * 4 + 3] : 0.f;      // (RW: the row's weight, kept in e_f's slot since the terminal evaluation)
                const float kL = hs * wst * (RW ? wI : ba.inv_n), kh = hs * wst * ba.a3 * (RW ? wI : ba.inv_n);
                SC[s * 4 + 0] = quad ? kL : kL + eh * kh;   // point agents: multiplies d(alphQ Q + alphW W)/dx
                SC[s * 4 + 1] = eh * kh;                 // cotangent of dPhi/dt
                SC[s * 4 + 2] = kL - eh * kh;            // multiplies p in the cotangent of grad_x Phi
            }
            __syncthreads();
            if (quad) {
                quad_adjoint(c, pl, pb, hs, wst, cpl, SC);
            } else {
                for (int j = c.tid; j < T * d; j += c.nthreads) {
                    const int t = j / d, i = j - t * d;
                    const float fbar = hs * (wst * LAM[t * ZLD + i] + cpl * XP[t * ZLD + i]);     // cotangent of f_x = -p
                    GB[t * pl.LDs + i] = -fbar + SC[t * 4 + 2] * G[t * pl.GLD + i];
                    XD[t * ZLD + i] = 0.f;
                }
            }
            if (c.tid < T) GB[c.tid * pl.LDs + d] = SC[c.tid * 4 + 1];
            __syncthreads();
            TL(c, 46);
            if (!quad) physics_xgrad(c, pl, pb, SC, 4);
            TL(c, 47);
        }
        phi_vjp<S, STATES>(c, pl, rg, ba, ev * ba.n + row0, nvalid);
        TL(c, 59);
        if (gmode)
            for (int j = c.tid; j < T * D1; j += c.nthreads) {
                const int t = j / D1, i = j - t * D1;
                if (t < nvalid) ba.sbar_out[(row0 + t) * D1 + i] = SBAR[t * pl.GLD + i];
            }
        for (int j = c.tid; j < T * d; j += c.nthreads) {
            const int t = j / d, i = j - t * d;
            const float xb = SBAR[t * pl.GLD + i] + XD[t * ZLD + i];
            if (fin) {
                LAM[t * ZLD + i] += xb;                                  // dJ/dx_T
            } else {
                XP[t * ZLD + i] = xb;
                const float xs = XS[t * ZLD + i] + xb;
                XS[t * ZLD + i] = xs;
                if (st == 0) LAM[t * ZLD + i] += xs;                     // all stages of step k are in
            }
        }
        if constexpr (RW) {                  // e_f's last readers are behind phi_vjp's barriers: its slot takes the row's weight for the kL seeds
            if (fin && c.tid < T) SC[c.tid * 4 + 3] = (c.tid < nvalid) ? ba.wrow[row0 + c.tid] : 0.f;
        }
        __syncthreads();
    }
    if (ba.lam0)
        for (int j = c.tid; j < T * d; j += c.nthreads) {
            const int t = j / d, i = j - t * d;
            if (t < nvalid) ba.lam0[(row0 + t) * d + i] = LAM[t * ZLD + i];
        }
}

template <int S, class SP, int STATES = 0, bool RW = false>
__global__ void __launch_bounds__(NOCF_MAXTHREADS) rollout_bwd_kernel(const DevPlan* __restrict__ plp, DevProb pb,
                                                                      const float* __restrict__ ws, BwdArgs ba) {
    static_assert(!RW || STATES == 0, "the weighted variant is the parameter-and-lam0 adjoint");
    if constexpr (SP::fixed) {
        constexpr DevPlan plc = SP::make();
        rollout_bwd_body<S, STATES, RW>(plc, plp, pb, ws, ba);
    } else {
        rollout_bwd_body<S, STATES, RW>(*plp, plp, pb, ws, ba);
    }
}
