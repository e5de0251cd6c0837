// nocf_f64_bwd.inc -- the adjoint of the rollout in DOUBLE precision: `trainOC.py --prec double` (trainOC.py:44,76-79: the whole
// training run in float64), i.e. Jc.backward() through the unrolled RK graph (trainOC.py:172-174) with every tensor a double.
//
// Same mathematics as nocf_bwd.inc (its header states the recurrences), written in the style of nocf_f64.inc: T samples per workgroup,
// one thread group per sample, products through f64_rows, everything else plain loops.  Correctness first -- this is the seldom-used
// precision of the reference; the products are the register-tiled / plain forms of the evaluation kernel (no packed MFMA images here).
// Per evaluation, latest first: grad Phi re-run at the recorded stage input keeping every layer's u, tanh and a; the cotangent of the
// right-hand side from the RK adjoint recurrences, the HJ sign masks and the physics (all three problem classes); the VJP of grad Phi
// (2 L + 2 products); the rows whose outer products are the weight gradients STREAMED in double (layout of nocf_rollout_bwd_f32), the
// caller contracts them with double GEMMs.  Any depth that fits the LDS (T = 4, 2 or 1 samples per workgroup by size).

struct F64BwdPlan {
    F64Plan b;                                    // shapes, workspace offsets, and the LDS offsets f64_physics uses (lS, lG, lRED, lSC, lDX, lZA, lPHI)
    int lU, lTH, lA, lTB, lAB, lQB, lUB, lVV;     // [L+1][T][m], [L+1][T][m], [L][T][m], [L+1][T][m], [T][m] x 4
    int lGB, lSBAR, lZB, lLAM, lXS, lXP, lXD, lSCB;
    int ldsDoubles, pad_;
};

struct F64BwdArgs {
    const double* sAll; const double* zT; const double* hs;
    long n; int nt, nstage;
    double t1, a0, a3, a4, a5, inv_n;
    double *Y, *Ob, *Wb, *V, *Ab, *Qb, *U0; long lstride;
    double *Gb, *Sx, *PHIb, *lam0;
};

static int make_f64_bwd_plan(int d, int m, int nTh, int r, int nAgents, int T, F64BwdPlan* out) {
    F64BwdPlan p{};
    F64Plan& b = p.b;
    b.d = d; b.D1 = d + 1; b.m = m; b.r = r; b.nTh = nTh; b.T = T; b.ZW = d + 4;
    b.hN = 1.0 / (nTh - 1);
    b.oK0T = 0; b.oKT = (long)b.D1 * m;
    const int L = nTh - 1;
    int l = 0;
    auto take = [&](long n) { int o = l; l += (int)((n + 1) & ~1L); return o; };
    b.lS = take((long)T * b.D1); b.lG = take((long)T * b.D1); b.lZA = take((long)T * 16); b.lRED = take(3 * 256); b.lPHI = take(T);
    b.lSC = take((long)T * (nAgents > 0 ? nAgents : 1) * 8); b.lDX = take((long)T * b.ZW);
    p.lU = take((long)(L + 1) * T * m); p.lTH = take((long)(L + 1) * T * m); p.lA = take((long)L * T * m); p.lTB = take((long)(L + 1) * T * m);
    p.lAB = take((long)T * m); p.lQB = take((long)T * m); p.lUB = take((long)T * m); p.lVV = take((long)T * m);
    p.lGB = take((long)T * b.D1); p.lSBAR = take((long)T * b.D1); p.lZB = take((long)T * 16);
    p.lLAM = take((long)T * b.ZW); p.lXS = take((long)T * b.ZW); p.lXP = take((long)T * b.ZW); p.lXD = take((long)T * b.ZW); p.lSCB = take((long)T * 4);
    p.ldsDoubles = l; b.ldsDoubles = l;
    *out = p;
    return ((size_t)l * 8 <= 160u * 1024u) ? 0 : NOCF_E_LDS;
}

// d(alphQ Q + alphW W)/dx of the point-agent problems for the thread group's sample, times cf, into XD[0..d); train-mode masks are constants;
// eval mode: the hard corridor and the blocks are masks without a gradient, the soft corridor's Gaussians are the train-mode ones
// (nocf_bwd.inc physics_xgrad restated in double: Cross2D.py:89-160, SwarmTraj.py:89-162)
__device__ __forceinline__ void f64_xgrad(const F64Prob& pb, const double* x, double* xd, double cf, int j0, int Gsz) {
    const int N = pb.nAgents, ad = pb.agentDim;
    const bool wantW = (pb.alphW != 0.0) && N >= 2;
    const double den = 2.0 * pb.r * pb.r, inv_r2 = 1.0 / (pb.r * pb.r);
    const double thr = (pb.training ? (N == 2 ? 2.2 : (pb.kind == NOCF_PROB_SWARMTRAJ ? 3.2 : 2.2)) : 2.0) * pb.r;
    const double two_pi = 6.283185307179586;
    for (int a = j0; a < N; a += Gsz) {
        double gq[3] = {0.0, 0.0, 0.0}, gw[3] = {0.0, 0.0, 0.0};
        if ((pb.training && pb.obstacle != NOCF_OBS_NONE) || pb.obstacle == NOCF_OBS_SOFTCORRIDOR) {
            if (pb.kind == NOCF_PROB_CROSS2D) {
                const double x0 = x[2 * a], x1 = x[2 * a + 1];
                if (pb.obstacle == NOCF_OBS_SOFTCORRIDOR) {
                    const double cov = 0.2, denom = two_pi * sqrt(cov * cov);
                    const double mus[4] = {-2.5, 2.5, -1.5, 1.5};
                    for (int k = 0; k < 4; ++k) {
                        const double pdf = f64_gauss2(x0, x1, mus[k], 0.0, cov, denom);
                        gq[0] -= pdf * (x0 - mus[k]) / cov;
                        gq[1] -= pdf * x1 / cov;
                    }
                } else if (pb.obstacle == NOCF_OBS_HARDCORRIDOR) {
                    const double n1 = sqrt(x0 * x0 + (x1 - 4.0) * (x1 - 4.0)), n2 = sqrt(x0 * x0 + (x1 + 3.5) * (x1 + 3.5));
                    const double th2 = 2.0 + pb.r;
                    if (n1 < th2 || n2 < th2) {
                        const double p1 = f64_gauss2(x0, x1, 0.0, 4.0, 1.0, two_pi), p2 = f64_gauss2(x0, x1, 0.0, -3.5, 1.0, two_pi);
                        gq[0] = -(p1 + p2) * x0;
                        gq[1] = -p1 * (x1 - 4.0) - p2 * (x1 + 3.5);
                    }
                }
            } else if (pb.kind == NOCF_PROB_SWARMTRAJ && pb.obstacle == NOCF_OBS_BLOCKS && pb.alphQ > 0.0) {
                const double x0 = x[3 * a], x1 = x[3 * a + 1], x2 = x[3 * a + 2], r = pb.r;
                const bool in1 = (x0 < 2.0 + r) && (x0 > -2.0 - r) && (x1 < 0.5 + r) && (x1 > -0.5 - r) && (x2 < 7.0 + r);
                const bool in2 = (x0 < 4.0 + r) && (x0 > 2.0 - r) && (x1 < 1.0 + r) && (x1 > -1.0 - r) && (x2 < 4.0 + r);
                if (in1 || in2) {                            // inside an inflated block (the + 999 offset has no gradient)
                    const double c15 = 15.749609945722419;
                    const double den1 = c15 * sqrt(243.0), den2 = c15 * sqrt(81.0);
                    const double e2 = x2 - 2.0, f0 = x0 - 2.5;
                    const double q1 = exp(-0.5 * (((x0 * x0) / 9.0 + (x1 * x1) / 3.0) + (e2 * e2) / 9.0)) / den1;
                    const double q2 = exp(-0.5 * (((f0 * f0) / 9.0 + (x1 * x1) / 3.0) + (e2 * e2) / 3.0)) / den2;
                    gq[0] = -q1 * x0 / 9.0 - q2 * f0 / 9.0;
                    gq[1] = -q1 * x1 / 3.0 - q2 * x1 / 3.0;
                    gq[2] = -q1 * e2 / 9.0 - q2 * e2 / 3.0;
                }
            }
        }
        if (wantW) {
            for (int bb = 0; bb < N; ++bb) {
                if (bb == a) continue;
                double e[3] = {0.0, 0.0, 0.0}, s2 = 0.0;
                for (int k = 0; k < ad; ++k) { e[k] = x[ad * a + k] - x[ad * bb + k]; s2 += e[k] * e[k]; }
                const double dist = sqrt(s2);
                if (dist < thr) {
                    const double w = exp(-(dist * dist) / den);
                    if (N == 2 || w != 1.0)                  // N > 2: entries equal to 1 are dropped by calcW (Cross2D.py:156-158)
                        for (int k = 0; k < ad; ++k) gw[k] -= w * e[k] * inv_r2;
                }
            }
        }
        for (int k = 0; k < ad; ++k) xd[ad * a + k] = cf * (pb.alphQ * gq[k] + pb.alphW * gw[k]);
    }
}

// Quadcopter cotangents of one evaluation for the thread group's sample (nocf_bwd.inc quad_adjoint restated in double; Quadcopter.py:65-113)
__device__ __forceinline__ void f64_quad_adjoint(const F64Prob& pb, const double* x, const double* p, const double* lam, const double* xp,
                                                 double* gb, double* xd, double hs, double wst, double cpl, double kL, double ekh, int j0, int Gsz) {
    const int N = pb.nAgents;
    const double M = pb.mass, grav = pb.grav, mh = -1.0 / (2.0 * pb.mass);
    for (int a = j0; a < N; a += Gsz) {
        const double* xa = x + 12 * a; const double* pa = p + 12 * a;
        const double cl = kL + ekh * (double)(N - a), ch = -ekh;
        double fb[12];
        for (int k = 0; k < 12; ++k) fb[k] = hs * (wst * lam[12 * a + k] + cpl * xp[12 * a + k]);
        const double sps = sin(xa[3]), sth = sin(xa[4]), sph = sin(xa[5]), cps = cos(xa[3]), cth = cos(xa[4]), cph = cos(xa[5]);
        const double f7 = sps * sph + cps * sth * cph, f8 = -cps * sph + sps * sth * cph, f9 = cth * cph;
        const double u = mh * (f7 * pa[6] + f8 * pa[7] + f9 * pa[8]);
        const double fu = (fb[6] * f7 + fb[7] * f8 + fb[8] * f9) / M;
        const double ku = fu + (2.0 * cl + 4.0 * ch) * u;
        double* g = gb + 12 * a; double* xq = xd + 12 * a;
        for (int k = 0; k < 6; ++k) { g[k] = -ch * xa[6 + k]; xq[6 + k] = fb[k] - ch * pa[k]; }
        g[6] = ku * mh * f7; g[7] = ku * mh * f8; g[8] = ku * mh * f9 + ch * grav;
        for (int k = 9; k < 12; ++k) g[k] = -0.5 * fb[k] + (0.5 * cl + ch) * pa[k];
        const double a7 = ku * mh * pa[6] + u * fb[6] / M, a8 = ku * mh * pa[7] + u * fb[7] / M, a9 = ku * mh * pa[8] + u * fb[8] / M;
        xq[0] = 0.0; xq[1] = 0.0; xq[2] = 0.0;
        xq[3] = -a7 * f8 + a8 * f7;
        xq[4] = a7 * cps * cth * cph + a8 * sps * cth * cph - a9 * sth * cph;
        xq[5] = a7 * (sps * cph - cps * sth * sph) + a8 * (-cps * cph - sps * sth * sph) - a9 * cth * sph;
    }
}

template <int T, bool WIDE>
__device__ __forceinline__ void rollout_bwd_f64_body(const F64BwdPlan& bp, const F64Phi& P, const F64Prob& pb, const double* __restrict__ ws, const F64BwdArgs& ba, double* ldsd) {
    const F64Plan& pl = bp.b;
    const int tid = threadIdx.x;
    constexpr int Gsz = 256 / T;
    const int tg = tid / Gsz, j0 = tid - tg * Gsz;
    const int d = pl.d, D1 = pl.D1, m = pl.m, r = pl.r, nTh = pl.nTh, ZW = pl.ZW, N = pb.nAgents, L = nTh - 1;
    const long row0 = (long)blockIdx.x * T;
    const bool valid = row0 + tg < ba.n;
    const long myrow = valid ? row0 + tg : ba.n - 1;
    double* S = ldsd + pl.lS; double* G = ldsd + pl.lG; double* ZAq = ldsd + pl.lZA; double* RED = ldsd + pl.lRED; double* PHI = ldsd + pl.lPHI;
    double* U = ldsd + bp.lU; double* TH = ldsd + bp.lTH; double* AA = ldsd + bp.lA; double* TB = ldsd + bp.lTB;
    double* AB = ldsd + bp.lAB; double* QB = ldsd + bp.lQB; double* UB = ldsd + bp.lUB; double* VV = ldsd + bp.lVV;
    double* GB = ldsd + bp.lGB; double* SBAR = ldsd + bp.lSBAR; double* ZB = ldsd + bp.lZB;
    double* LAM = ldsd + bp.lLAM; double* XS = ldsd + bp.lXS; double* XP = ldsd + bp.lXP; double* XD = ldsd + bp.lXD; double* SCB = ldsd + bp.lSCB;
    const long TM = (long)T * m;
    const double* K0T = ws + pl.oK0T;
    const double hN = pl.hN;
    const double cb = P.cbp ? P.cbp[0] : 0.0;
    const bool quad = pb.kind == NOCF_PROB_QUADCOPTER;
    const double inv = valid ? ba.inv_n : 0.0;                  // tail rows replicate a valid sample with 1/N = 0: all their cotangents are 0

    for (int i = tid; i < bp.ldsDoubles; i += 256) ldsd[i] = 0.0;
    __syncthreads();

    const long total = (long)ba.nt * ba.nstage;
    for (long ev = total; ev >= 0; --ev) {
        const bool fin = (ev == total);
        const int k = fin ? ba.nt : (int)(ev / ba.nstage), st = fin ? 0 : (int)(ev - (long)k * ba.nstage);
        const double hs = fin ? 0.0 : ba.hs[k];
        double wst = 1.0, cpl = 0.0;
        if (ba.nstage != 1) { wst = (st == 0 || st == 3) ? (1.0 / 6.0) : (2.0 / 6.0); cpl = (st == 3) ? 0.0 : (st == 2 ? 1.0 : 0.5); }
        // ---- the stage input
        if (fin) {
            for (int i = j0; i < d; i += Gsz) S[tg * D1 + i] = ba.zT[myrow * ZW + i];
            if (j0 == 0) S[tg * D1 + d] = ba.t1;
        } else {
            if (st == ba.nstage - 1) for (int i = j0; i < d; i += Gsz) { XS[tg * ZW + i] = 0.0; XP[tg * ZW + i] = 0.0; }
            for (int i = j0; i < D1; i += Gsz) S[tg * D1 + i] = ba.sAll[(ev * ba.n + myrow) * D1 + i];
        }
        __syncthreads();
        // ---- grad Phi at s keeping u_l, tanh_l (l = 0 .. L) and a_l (l = 0 .. L-1; a_L = w)   (src/Phi.py:99-138)
        f64_rows<T, WIDE>(K0T, m, nullptr, m, D1, S, D1, tid, [&](int i) { return P.b0[i]; },
                    [&](int i, int t, double a) { double sg, th; f64_act_pair(a, sg, th); U[t * m + i] = sg; TH[t * m + i] = th; });
        for (int q = tid; q < T * r; q += 256) {
            const int t = q / r, rr = q - t * r;
            double acc = 0.0;
            for (int kk = 0; kk < D1; ++kk) acc += P.A[rr * D1 + kk] * S[t * D1 + kk];
            ZAq[t * 16 + rr] = acc;
        }
        __syncthreads();
        for (int l = 1; l <= L; ++l) {
            const double* KT = ws + pl.oKT + (long)(l - 1) * m * m;
            const double* bl = P.b + (long)(l - 1) * m;
            f64_rows<T, WIDE>(KT, m, nullptr, m, m, U + (l - 1) * TM, m, tid, [&](int i) { return bl[i]; },
                        [&](int i, int t, double a) { VV[t * m + i] = a; });
            __syncthreads();
            for (int q = tid; q < T * m; q += 256) { double sg, th; f64_act_pair(VV[q], sg, th); U[l * TM + q] = U[(l - 1) * TM + q] + hN * sg; TH[l * TM + q] = th; }
            __syncthreads();
        }
        if (fin) {
            double v[1] = {0.0};
            for (int i = j0; i < m; i += Gsz) v[0] += P.w[i] * U[L * TM + tg * m + i];
            for (int q = j0; q < r; q += Gsz) v[0] += 0.5 * ZAq[tg * 16 + q] * ZAq[tg * 16 + q];
            for (int kk = j0; kk < D1; kk += Gsz) v[0] += P.cw[kk] * S[tg * D1 + kk];
            f64_group_sum<1>(RED, tid, tg, j0, Gsz, v);
            if (j0 == 0) PHI[tg] = v[0] + cb;
        }
        for (int l = L; l >= 1; --l) {                           // a_{l-1} = a_l + hN K_l' (tanh_l . a_l)
            const double* Kl = P.K + (long)(l - 1) * m * m;
            for (int q = tid; q < T * m; q += 256) VV[q] = TH[l * TM + q] * ((l == L) ? P.w[q % m] : AA[l * TM + q]);
            __syncthreads();
            f64_rows<T, WIDE>(Kl, m, nullptr, m, m, VV, m, tid, [&](int) { return 0.0; },
                        [&](int j, int t, double a) { AA[(l - 1) * TM + t * m + j] = ((l == L) ? P.w[j] : AA[l * TM + t * m + j]) + hN * a; });
            __syncthreads();
        }
        for (int q = tid; q < T * m; q += 256) VV[q] = TH[q] * AA[q];              // y = tanh_0 . a_0
        __syncthreads();
        f64_rows<T, WIDE>(P.K0, D1, nullptr, D1, m, VV, m, tid, [&](int) { return 0.0; },
                    [&](int j, int t, double a) {
                        double sa = 0.0;
                        for (int q = 0; q < r; ++q) sa += P.A[q * D1 + j] * ZAq[t * 16 + q];
                        G[t * D1 + j] = a + sa + P.cw[j];
                    });
        __syncthreads();
        // streams of this evaluation that are forward quantities: y, s
        {
            const long row = ev * ba.n + row0 + tg;
            if (valid) {
                for (int i = j0; i < m; i += Gsz) ba.Y[row * m + i] = VV[tg * m + i];
                for (int i = j0; i < D1; i += Gsz) ba.Sx[row * D1 + i] = S[tg * D1 + i];
            }
        }
        // ---- the cotangent of the right-hand side
        if (fin) {
            double v[1] = {0.0};
            for (int i = j0; i < d; i += Gsz) { const double res = S[tg * D1 + i] - pb.xtarget[i]; v[0] += res * res; }
            f64_group_sum<1>(RED, tid, tg, j0, Gsz, v);
            const double cG = 0.5 * v[0];
            const double dd = PHI[tg] - ba.a0 * cG;
            const double ef = (dd > 0.0) ? 1.0 : (dd < 0.0 ? -1.0 : 0.0);
            for (int i = j0; i < d; i += Gsz) {
                const double res = S[tg * D1 + i] - pb.xtarget[i];
                const double dg = G[tg * D1 + i] - ba.a0 * res;
                const double eg = (dg > 0.0) ? 1.0 : (dg < 0.0 ? -1.0 : 0.0);
                LAM[tg * ZW + i] = inv * (ba.a0 * res + ba.a4 * ef * dg - ba.a5 * ba.a0 * eg);
                GB[tg * D1 + i] = inv * ba.a5 * eg;
                XD[tg * ZW + i] = 0.0;
            }
            if (j0 == 0) GB[tg * D1 + d] = 0.0;
            // value rows: ubar_i = phib a_i, so qbar_i = phib hN v_i, obar = phib y, dw row = phib u_L
            const double phib = inv * ba.a4 * ef;
            if (valid) {
                const long row = (total + 1) * ba.n + row0 + tg;
                for (int col = j0; col < m; col += Gsz) {
                    for (int i = 1; i <= L; ++i) {
                        const long lo = (long)(i - 1) * ba.lstride;
                        const double ai = (i == L) ? P.w[col] : AA[i * TM + tg * m + col];
                        ba.Qb[lo + row * m + col] = phib * hN * TH[i * TM + tg * m + col] * ai;
                        ba.U0[lo + row * m + col] = U[(i - 1) * TM + tg * m + col];
                    }
                    ba.Ob[row * m + col] = phib * VV[tg * m + col];
                    ba.Wb[row * m + col] = phib * U[L * TM + tg * m + col];
                }
                for (int i = j0; i < D1; i += Gsz) ba.Sx[row * D1 + i] = S[tg * D1 + i];
                if (j0 == 0) ba.PHIb[row0 + tg] = phib;
            }
            __syncthreads();
        } else {
            double Lc, H, Q, W;
            f64_physics<T>(pl, pb, ldsd, Lc, H, Q, W);           // (sums + barriers; H of the thread group's sample)
            const double dh = G[tg * D1 + d] - H;
            const double eh = (dh > 0.0) ? 1.0 : (dh < 0.0 ? -1.0 : 0.0);
            const double kL = hs * wst * inv, ekh = eh * hs * wst * ba.a3 * inv;
            if (quad) {
                f64_quad_adjoint(pb, S + tg * D1, G + tg * D1, LAM + tg * ZW, XP + tg * ZW, GB + tg * D1, XD + tg * ZW, hs, wst, cpl, kL, ekh, j0, Gsz);
                __syncthreads();
                if (N == 2 && pb.alphW > 0.0 && j0 == 0) {      // Quadcopter.py:139-143, mask constant
                    const double* x = S + tg * D1; double* xd = XD + tg * ZW;
                    double e[3], s2 = 0.0;
                    for (int q = 0; q < 3; ++q) { e[q] = x[q] - x[12 + q]; s2 += e[q] * e[q]; }
                    const double dist = sqrt(s2);
                    if (dist < 2.0 * pb.r) {
                        const double w = exp(-(dist * dist) / (2.0 * pb.r * pb.r));
                        const double cw = (kL + ekh * 2.0) * pb.alphW;
                        for (int q = 0; q < 3; ++q) { const double g = -cw * w * e[q] / (pb.r * pb.r); xd[q] += g; xd[12 + q] -= g; }
                    }
                }
            } else {
                for (int i = j0; i < d; i += Gsz) {
                    const double fbar = hs * (wst * LAM[tg * ZW + i] + cpl * XP[tg * ZW + i]);
                    GB[tg * D1 + i] = -fbar + (kL - ekh) * G[tg * D1 + i];
                    XD[tg * ZW + i] = 0.0;
                }
                __syncthreads();
                f64_xgrad(pb, S + tg * D1, XD + tg * ZW, kL + ekh, j0, Gsz);
            }
            if (j0 == 0) GB[tg * D1 + d] = ekh;
            __syncthreads();
        }
        // ---- the vector-Jacobian product of grad Phi (recurrences: nocf_bwd.inc phi_vjp)
        const long row = ev * ba.n + row0 + tg;
        for (int q = tid; q < T * r; q += 256) {                 // A gbar
            const int t = q / r, rr = q - t * r;
            double acc = 0.0;
            for (int kk = 0; kk < D1; ++kk) acc += P.A[rr * D1 + kk] * GB[t * D1 + kk];
            ZB[t * 16 + rr] = acc;
        }
        if (valid) for (int i = j0; i < D1; i += Gsz) ba.Gb[row * D1 + i] = GB[tg * D1 + i];
        f64_rows<T, WIDE>(K0T, m, nullptr, m, D1, GB, D1, tid, [&](int) { return 0.0; },                       // ybar = K0 gbar
                    [&](int i, int t, double yb) { AB[t * m + i] = TH[t * m + i] * yb; TB[t * m + i] = AA[t * m + i] * yb; });
        __syncthreads();
        for (int i = 1; i <= L; ++i) {                           // vbar_i = hN K_i abar_{i-1}
            const double* KT = ws + pl.oKT + (long)(i - 1) * m * m;
            const long lo = (long)(i - 1) * ba.lstride;
            if (valid)
                for (int col = j0; col < m; col += Gsz) {
                    const double ai = (i == L) ? P.w[col] : AA[i * TM + tg * m + col];
                    ba.V[lo + row * m + col] = hN * TH[i * TM + tg * m + col] * ai;
                    ba.Ab[lo + row * m + col] = AB[tg * m + col];
                    ba.U0[lo + row * m + col] = U[(i - 1) * TM + tg * m + col];
                }
            f64_rows<T, WIDE>(KT, m, nullptr, m, m, AB, m, tid, [&](int) { return 0.0; },
                        [&](int col, int t, double x) { VV[t * m + col] = hN * x; });
            __syncthreads();
            for (int q = tid; q < T * m; q += 256) {
                const double vb = VV[q], ai = (i == L) ? P.w[q % m] : AA[i * TM + q];
                TB[i * TM + q] = ai * vb;                        // taubar_i (i = L: w . vbar_L)
                AB[q] += TH[i * TM + q] * vb;                    // abar_i
            }
            __syncthreads();
        }
        if (valid) for (int col = j0; col < m; col += Gsz) ba.Wb[row * m + col] = AB[tg * m + col];          // dw row = abar_L
        for (int q = tid; q < T * m; q += 256) UB[q] = 0.0;
        __syncthreads();
        for (int i = L; i >= 1; --i) {                           // qbar_i ; ubar_{i-1} = ubar_i + K_i' qbar_i
            const double* Kl = P.K + (long)(i - 1) * m * m;
            const long lo = (long)(i - 1) * ba.lstride;
            for (int q = tid; q < T * m; q += 256) {
                const double ti = TH[i * TM + q];
                QB[q] = (1.0 - ti * ti) * TB[i * TM + q] + ((i == L) ? 0.0 : hN * ti * UB[q]);
            }
            __syncthreads();
            if (valid) for (int col = j0; col < m; col += Gsz) ba.Qb[lo + row * m + col] = QB[tg * m + col];
            f64_rows<T, WIDE>(Kl, m, nullptr, m, m, QB, m, tid, [&](int) { return 0.0; },
                        [&](int col, int t, double x) { UB[t * m + col] += x; });
            __syncthreads();
        }
        for (int q = tid; q < T * m; q += 256) { const double t0 = TH[q]; QB[q] = (1.0 - t0 * t0) * TB[q] + t0 * UB[q]; }     // obar
        __syncthreads();
        if (valid) for (int col = j0; col < m; col += Gsz) ba.Ob[row * m + col] = QB[tg * m + col];
        f64_rows<T, WIDE>(P.K0, D1, nullptr, D1, m, QB, m, tid, [&](int) { return 0.0; },                      // sbar = K0' obar + A'(A gbar)
                    [&](int j, int t, double a) {
                        double sa = 0.0;
                        for (int q = 0; q < r; ++q) sa += P.A[q * D1 + j] * ZB[t * 16 + q];
                        SBAR[t * D1 + j] = a + sa;
                    });
        __syncthreads();
        // ---- RK adjoint recurrences
        for (int i = j0; i < d; i += Gsz) {
            const double xb = SBAR[tg * D1 + i] + XD[tg * ZW + i];
            if (fin) {
                LAM[tg * ZW + i] += xb;
            } else {
                XP[tg * ZW + i] = xb;
                const double xs = XS[tg * ZW + i] + xb;
                XS[tg * ZW + i] = xs;
                if (st == 0) LAM[tg * ZW + i] += xs;
            }
        }
        __syncthreads();
    }
    if (ba.lam0 && valid) for (int i = j0; i < d; i += Gsz) ba.lam0[(row0 + tg) * d + i] = LAM[tg * ZW + i];
}

// Wide networks (register-tiled products) take the whole register file; narrow ones are latency-bound plain loops and run at two
// workgroups' worth of waves per SIMD (256 registers per lane) so that a second workgroup hides the first one's L2 round trips
template <int T, bool WIDE>
__global__ void __launch_bounds__(256) rollout_bwd_f64_kernel(F64BwdPlan bp, F64Phi P, F64Prob pb, const double* __restrict__ ws, F64BwdArgs ba) {
    extern __shared__ double ldsd[];
    rollout_bwd_f64_body<T, WIDE>(bp, P, pb, ws, ba, ldsd);
}
template <int T>
__global__ void __launch_bounds__(256, 2) rollout_bwd_f64_narrow_kernel(F64BwdPlan bp, F64Phi P, F64Prob pb, const double* __restrict__ ws, F64BwdArgs ba) {
    extern __shared__ double ldsd[];
    rollout_bwd_f64_body<T, false>(bp, P, pb, ws, ba, ldsd);
}
