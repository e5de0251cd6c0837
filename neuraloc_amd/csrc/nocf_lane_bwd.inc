// nocf_lane_bwd.inc -- the adjoint of the rollout for SMALL value networks, one wavefront per sample (the training
// counterpart of nocf_lane.inc; same eligibility: nTh = 2, m <= 32, d+1 <= 32, Cross2D agents).
//
// Same mathematics as nocf_bwd.inc (discretise-then-optimise RK adjoint, VJP of grad Phi), but nothing is streamed:
// every lane keeps its row/column of the weights AND its row of every weight gradient in registers, a matvec or an
// outer-product update is a chain of v_readlane + v_fma, and at the end each wave writes ONE gradient vector
//     gpart[sample] = [dK0 (m x D1) | db0 (m) | dK1 (m x m) | db1 (m) | dw (m) | dc.weight (D1) | dc.bias (1) | dM (D1 x D1)]
// (dM = d/d(A'A), the host forms dA = A (dM + dM')).  The host sums gpart over the samples (fixed order).
// 4x the parallelism of the 4-samples-per-wave tile adjoint, no LDS, no barrier, no row streams, no contraction GEMMs.
//
// STATES (nocf_rollout_bwd_states_f32): the state-only instantiation.  The lambda recursion (fbar, gbar, XD, XS, XP, LAM) is the same
// statements; the gradient rows, their FMAs and the gpart store are compiled out, and LAM is written to lamW[k] when the last stage of step
// k begins -- z_{k+1} = step(z_k) + W[k], so that cotangent is dJ/dW[k] (lamW[nt-1]: the terminal cotangent dJ/dx(T)).
// STATES is a mode: 0 the full adjoint, 1 the state-only one (`false` / `true` select these two as before), 2 the JOINT one
// (nocf_rollout_bwd_small_w_f32): every statement of mode 0 plus the lamW[k] store of mode 1 at the same place -- one launch gives the
// parameter gradients and dJ/dW of a disturbed rollout (min-max training).  Both tests are `if constexpr`: mode 0 carries no trace of the store.

struct LaneBwdArgs {
    DevPhi P;
    int d, m, r, nAg;
    float cb;
    const float* sAll; const float* zT; const float* hs;
    long n; int nt, nstage;
    float t1, a0, a3, a4, a5, inv_n;
    float* gpart; long P_total;
    float* lam0;
    float* lamW;              // [nt][n][d] (nullable): the state cotangent behind every step, dJ/dW of a disturbed rollout (STATES modes 1 and 2)
    const float* wrow;        // [n] (RW instantiations only): one weight per sample, standing where inv_n stands (nocf_rollout_bwd_small_rw_f32)
};

__device__ __forceinline__ float sgnf(float v) { return (v > 0.f) ? 1.f : (v < 0.f ? -1.f : 0.f); }

// ENS (STATES = 0; nocf_rollout_bwd_small_ensemble_f32): the adjoint of an ensemble rollout (nocf_lane.inc), one launch for E networks: la.n =
// E * ea.n rows, row g belongs to member g / ea.n; la.P holds the stacked tensors; row e of the table ea.alph stands for a0, a3, a4, a5
// (entries 0, 3, 4, 5) and for the problem's alph_Q / alph_W (1, 2); la.inv_n is 1 / ea.n, the mean over ONE member's samples.  As there: the member of a wave is uniform,
// its pointers and multipliers sit in scalar registers, every statement behind those reads is the single-network one, and every ENS test is
// `if constexpr`.  Row g's gradient vector goes to gpart[g]: member e's partials are the contiguous rows [e ea.n, (e + 1) ea.n)
//
// RW (STATES = 0, no ensemble; nocf_rollout_bwd_small_rw_f32): the per-sample weight la.wrow[sample] stands where la.inv_n stands at the four
// cotangent seeds (LAM, gbar, phib, kL): gpart[sample] = wrow[sample] grad J_sample, lam0[sample] = wrow[sample] dJ_sample/dx.  The sample of
// a wave is uniform, so the weight is read once into a scalar register; every RW test is a compile-time choice at its place of use.
//
// ENS && RW (STATES = 0; nocf_rollout_bwd_small_ensemble_rw_f32): both of the above and nothing more.  la.wrow is [E, ea.n] contiguous, which is
// the row order of the E * ea.n batch, so row g reads la.wrow[g] through the same scalar read; la.inv_n is not read.
//
// ENS && STATES == 2 (nocf_rollout_bwd_small_ensemble_w_f32) and ENS && STATES == 1 (nocf_rollout_bwd_small_ensemble_states_f32), DESIGN.md
// section 3.17: the ensemble adjoint with the lamW[k] store of the joint / state-only modes.  la.lamW is [E, nt, ea.n, d] MEMBER-major -- member
// e's slice is the [nt, n, d] the single-network call writes, so W.grad of a disturbed ensemble needs no transposition.  A wave offsets the
// pointer once to its member's slice and its row of step 0 (wave-uniform); the store stands where the single-network store stands.  Tail waves
// write nothing.  RW with STATES != 0 stays refused (the static_assert below): a weighted adversarial ensemble is not built.
template <int MP, int DP, int STATES = 0, bool ENS = false, bool RW = false>
__global__ void __launch_bounds__(256) rollout_lane_bwd_kernel(LaneBwdArgs la, DevProb pb, EnsArgs ea) {
    static_assert(!RW || STATES == 0, "the weighted variants are parameter-and-lam0 adjoints");
    const int lane = threadIdx.x & 63;
    const long sample = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = sample < la.n;
    const long row = live ? sample : la.n - 1;
    const int d = la.d, D1 = d + 1, m = la.m, N = la.nAg;
    DevPhi P = la.P;
    float eA0 = 0.f, eAQ = 0.f, eAW = 0.f, eA3 = 0.f, eA4 = 0.f, eA5 = 0.f;      // ENS: the member's row of the multiplier table
    float* lamWe = la.lamW;                                         // ENS && STATES != 0: this wave's row of step 0 in the member's slice of lamW
    if constexpr (ENS) {
        const unsigned e = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)row / ea.n));
        P.K0 += (long)e * m * D1; P.b0 += (long)e * m; P.K += (long)e * m * m; P.b += (long)e * m; P.w += (long)e * m;
        P.A += (long)e * la.r * D1; P.cw += (long)e * D1; P.cbp += e;
        const float* at = ea.alph + (long)e * 6;
        eA0 = at[0]; eAQ = at[1]; eAW = at[2]; eA3 = at[3]; eA4 = at[4]; eA5 = at[5];
        if constexpr (STATES != 0) { if (lamWe) lamWe += (((long)e * la.nt) * ea.n + (row - (long)e * ea.n)) * d; }
    }
    // (below, `ENS ? member's : the call's` is a compile-time choice at the place of use: the other instantiations keep their statements)
    float wI = 0.f;                                                 // RW: this wave's sample weight (a tail wave reads the last row's and writes nothing)
    if constexpr (RW) wI = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, la.wrow[row])));

    // ---- weights: my row and my column of every matrix (as in the forward lane kernel)
    float k0row[DP], symA[DP], k1row[MP], k1col[MP], k0col[MP];
#pragma unroll
    for (int i = 0; i < DP; ++i) k0row[i] = (lane < m && i < D1) ? P.K0[lane * D1 + i] : 0.f;
#pragma unroll
    for (int k = 0; k < MP; ++k) {
        k1row[k] = (lane < m && k < m) ? P.K[lane * m + k] : 0.f;
        k1col[k] = (lane < m && k < m) ? P.K[k * m + lane] : 0.f;
        k0col[k] = (lane < D1 && k < m) ? P.K0[k * D1 + lane] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < DP; ++j) {
        float a = 0.f;
        if (lane < D1 && j < D1)
            for (int q = 0; q < la.r; ++q) a += P.A[q * D1 + lane] * P.A[q * D1 + j];
        symA[j] = a;
    }
    const float b0 = lane < m ? P.b0[lane] : 0.f;
    const float b1 = lane < m ? P.b[lane] : 0.f;
    const float wv = lane < m ? P.w[lane] : 0.f;
    const float cw = lane < D1 ? P.cw[lane] : 0.f;
    const float cbv = P.cbp ? *P.cbp : la.cb;
    const float xt = lane < d ? pb.xtarget[lane] : 0.f;

    // ---- gradient rows of this lane
    float gK0[DP], gK1[MP], gM[DP];
#pragma unroll
    for (int i = 0; i < DP; ++i) { gK0[i] = 0.f; gM[i] = 0.f; }
#pragma unroll
    for (int k = 0; k < MP; ++k) gK1[k] = 0.f;
    float gb0 = 0.f, gb1 = 0.f, gw = 0.f, gcw = 0.f, gcb = 0.f;

    const bool wantW = (ENS ? eAW != 0.f : want_W(pb)) && N >= 2;
    const float den = (float)(2.0 * pb.r * pb.r);
    const float inv_r2 = 1.f / ((float)pb.r * (float)pb.r);
    const double facN = pb.training ? 2.2 : 2.0;                     // Cross2D.py:130-160 (N == 2 and N > 2 alike)
    const float thr = (float)(facN * pb.r);
    const float aQ = ENS ? eAQ : (float)pb.alphQ, aW = ENS ? eAW : (float)pb.alphW;
    const int comp = lane & 1;                                      // Cross2D: lane = 2*agent + comp

    float LAM = 0.f, XS = 0.f, XP = 0.f;
    const float c16 = (float)(1.0 / 6.0), c26 = (float)(2.0 / 6.0);
    const long total = (long)la.nt * la.nstage;
    for (long ev = total; ev >= 0; --ev) {
        const bool fin = (ev == total);
        const int k = fin ? la.nt : (int)(ev / la.nstage), st = fin ? 0 : (int)(ev - (long)k * la.nstage);
        const float hs = fin ? 0.f : la.hs[k];
        float wst = 1.f, cpl = 0.f;
        if (la.nstage != 1) { wst = (st == 0 || st == 3) ? c16 : c26; cpl = (st == 3) ? 0.f : (st == 2 ? 1.f : 0.5f); }
        if (!fin && st == la.nstage - 1) {
            if constexpr (STATES != 0 && ENS) { if (lamWe && live && lane < d) lamWe[(long)k * ea.n * d + lane] = LAM; }
            else if constexpr (STATES != 0) { if (la.lamW && live && lane < d) la.lamW[((long)k * la.n + sample) * d + lane] = LAM; }
            XS = 0.f; XP = 0.f;
        }
        float s;
        if (fin) s = lane < d ? la.zT[row * (d + 4) + lane] : (lane == d ? la.t1 : 0.f);
        else s = lane < D1 ? la.sAll[(ev * la.n + row) * D1 + lane] : 0.f;

        // ---- grad Phi at s with every intermediate kept (src/Phi.py:99-138)
        float o = b0;
#pragma unroll
        for (int i = 0; i < DP; ++i) o = fmaf(k0row[i], lane_bcast(s, i), o);
        float u0, th0;
        act_pair(o, u0, th0);
        float q = b1;
#pragma unroll
        for (int kk = 0; kk < MP; ++kk) q = fmaf(k1row[kk], lane_bcast(u0, kk), q);
        const float th1 = tanh_fast(q);
        const float v = th1 * wv;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < MP; ++j) acc = fmaf(k1col[j], lane_bcast(v, j), acc);
        const float a = wv + acc;
        const float y = th0 * a;
        float g = cw, sy = 0.f;
#pragma unroll
        for (int kk = 0; kk < MP; ++kk) g = fmaf(k0col[kk], lane_bcast(y, kk), g);
#pragma unroll
        for (int j = 0; j < DP; ++j) sy = fmaf(symA[j], lane_bcast(s, j), sy);
        g += sy;

        // ---- cotangent of grad Phi (gbar, one component per lane <= d) and the direct x term XD
        float gbar = 0.f, XD = 0.f;
        if (fin) {
            const float u1 = u0 + sigma_act(q);
            const float phi = wave_sum(lane < m ? wv * u1 : 0.f) + 0.5f * wave_sum(lane < D1 ? s * sy : 0.f)
                              + wave_sum(lane < D1 ? cw * s : 0.f) + cbv;
            const float res = lane < d ? s - xt : 0.f;
            const float cG = 0.5f * wave_sum(res * res);
            const float ef = sgnf(phi - (ENS ? eA0 : la.a0) * cG);
            const float dg = g - (ENS ? eA0 : la.a0) * res;
            const float eg = sgnf(dg);
            if (lane < d) {
                LAM = (RW ? wI : la.inv_n) * ((ENS ? eA0 : la.a0) * res + (ENS ? eA4 : la.a4) * ef * dg - (ENS ? eA5 : la.a5) * (ENS ? eA0 : la.a0) * eg);
                gbar = (RW ? wI : la.inv_n) * (ENS ? eA5 : la.a5) * eg;
            }
            // the value cotangent reuses the forward quantities: ubar = phib a, qbar = phib v, obar = phib y
            if constexpr (STATES != 1) {
            const float phib = (RW ? wI : la.inv_n) * (ENS ? eA4 : la.a4) * ef;
#pragma unroll
            for (int kk = 0; kk < MP; ++kk) gK1[kk] = fmaf(phib * v, lane_bcast(u0, kk), gK1[kk]);
#pragma unroll
            for (int i = 0; i < DP; ++i) {
                const float si = lane_bcast(s, i);
                gK0[i] = fmaf(phib * y, si, gK0[i]);
                gM[i] = fmaf(0.5f * phib * s, si, gM[i]);
            }
            gb1 += phib * v; gb0 += phib * y; gw += phib * u1;
            if (lane < D1) gcw += phib * s;
            gcb += phib;
            }
        } else {
            // problem physics (Cross2D.py:73-160): sum p^2, obstacle sum, interaction sum and their x-gradients
            const float sp2 = wave_sum(lane < d ? g * g : 0.f);
            const float xo = dpp_peer<0xB1>(s);                       // the other coordinate of my agent
            const float x0 = comp ? xo : s, x1 = comp ? s : xo;
            float qa = 0.f, gq = 0.f;                                 // obstacle value (comp 0 lanes) and my component of its gradient
            if (pb.obstacle != NOCF_OBS_NONE && lane < d) {
                const float val = obstacle_cross2d(pb, x0, x1);
                if (comp == 0) qa = val;
                // (the soft corridor's Gaussians do not depend on the mode: their gradient is due in eval mode too -- a disturbed or an eval-mode
                // training call differentiates them; the eval-mode hard corridor is a mask, whose gradient is 0)
                if (pb.training || pb.obstacle == NOCF_OBS_SOFTCORRIDOR) {
                    if (pb.obstacle == NOCF_OBS_SOFTCORRIDOR) {
                        const float cov = 0.2f, denom = (float)TWO_PI_D * sqrtf(cov * cov);
                        const float mus[4] = {-2.5f, 2.5f, -1.5f, 1.5f};
#pragma unroll
                        for (int kk = 0; kk < 4; ++kk) {
                            const float pdf = gauss2(x0, x1, mus[kk], 0.f, cov, denom);
                            gq -= comp ? pdf * x1 / cov : pdf * (x0 - mus[kk]) / cov;
                        }
                    } else if (pb.obstacle == NOCF_OBS_HARDCORRIDOR) {
                        const float denom = (float)TWO_PI_D;
                        const float n1 = sqrtf(x0 * x0 + (x1 - 4.f) * (x1 - 4.f)), n2 = sqrtf(x0 * x0 + (x1 + 3.5f) * (x1 + 3.5f));
                        const float th2 = (float)(2.0 + pb.r);
                        if (n1 < th2 || n2 < th2) {
                            const float p1 = gauss2(x0, x1, 0.f, 4.f, 1.f, denom), p2 = gauss2(x0, x1, 0.f, -3.5f, 1.f, denom);
                            gq = comp ? (-p1 * (x1 - 4.f) - p2 * (x1 + 3.5f)) : (-(p1 + p2) * x0);
                        }
                    }
                }
            }
            const float Qraw = wave_sum(qa);
            float wsum = 0.f, gwf = 0.f;                              // sum over my partners of the pair weight; my force component
            if (wantW) {
                for (int j = 1; j < N; ++j) {
                    int src = lane + 2 * j; if (src >= d) src -= d;
                    const float xb = __shfl(s, lane < d ? src : lane);
                    const float e = s - xb;
                    const float e2 = e * e;
                    const float s2 = e2 + dpp_peer<0xB1>(e2);
                    const float dist = sqrtf(s2);
                    if (lane < d && dist < thr) {
                        const float w = expf(-(dist * dist) / den);
                        if (N == 2 || w != 1.f) { wsum += w; gwf -= w * e * inv_r2; }
                    }
                }
            }
            const float Wv = wantW ? 0.5f * wave_sum((lane < d && comp == 0) ? wsum : 0.f) : 0.f;   // every unordered pair twice
            const float Qs = aQ * Qraw;
            float Lg = 0.5f * sp2 + Qs;
            if ((ENS ? eAW != 0.f : want_W(pb))) Lg = Lg + aW * Wv;
            const float H = -Lg + sp2;
            const float gt = lane_bcast_u(g, d);
            const float eh = sgnf(gt - H);
            const float kL = hs * wst * (RW ? wI : la.inv_n), kh = kL * (ENS ? eA3 : la.a3);
            if (lane < d) {
                const float fbar = hs * (wst * LAM + cpl * XP);
                gbar = -fbar + (kL - eh * kh) * g;
                XD = (kL + eh * kh) * (aQ * gq + (wantW ? aW * gwf : 0.f));
            } else if (lane == d) gbar = eh * kh;
        }

        // ---- VJP of grad Phi and the gradient rows
        float ybar = 0.f, sA = 0.f;
#pragma unroll
        for (int i = 0; i < DP; ++i) {
            const float gi = lane_bcast(gbar, i), si = lane_bcast(s, i);
            ybar = fmaf(k0row[i], gi, ybar);
            sA = fmaf(symA[i], gi, sA);
            if constexpr (STATES != 1) { gK0[i] = fmaf(y, gi, gK0[i]); gM[i] = fmaf(gbar, si, gM[i]); } else (void)si;
        }
        const float abar = th0 * ybar, tau0bar = a * ybar;
        float vbar = 0.f;
#pragma unroll
        for (int kk = 0; kk < MP; ++kk) {
            const float ak = lane_bcast(abar, kk);
            vbar = fmaf(k1row[kk], ak, vbar);
            if constexpr (STATES != 1) gK1[kk] = fmaf(v, ak, gK1[kk]);
        }
        const float qbar = (1.f - th1 * th1) * wv * vbar;
        if constexpr (STATES != 1) gw += abar + th1 * vbar;
        float u0bar = 0.f;
#pragma unroll
        for (int j = 0; j < MP; ++j) u0bar = fmaf(k1col[j], lane_bcast(qbar, j), u0bar);
        if constexpr (STATES != 1) {
#pragma unroll
            for (int kk = 0; kk < MP; ++kk) gK1[kk] = fmaf(qbar, lane_bcast(u0, kk), gK1[kk]);
        }
        const float obar = th0 * u0bar + (1.f - th0 * th0) * tau0bar;
        float sbar = sA;
#pragma unroll
        for (int kk = 0; kk < MP; ++kk) sbar = fmaf(k0col[kk], lane_bcast(obar, kk), sbar);
        if constexpr (STATES != 1) {
#pragma unroll
            for (int i = 0; i < DP; ++i) gK0[i] = fmaf(obar, lane_bcast(s, i), gK0[i]);
            gb0 += obar; gb1 += qbar;
            if (lane < D1) gcw += gbar;
        }

        const float xb = (lane < d) ? sbar + XD : 0.f;
        if (fin) LAM += xb;
        else {
            XP = xb; XS += xb;
            if (st == 0) LAM += XS;
        }
    }

    if (!live) return;
    if constexpr (STATES != 1) {
    float* gp = la.gpart + sample * la.P_total;
    long o = 0;
#pragma unroll
    for (int i = 0; i < DP; ++i) if (lane < m && i < D1) gp[o + (long)lane * D1 + i] = gK0[i];
    o += (long)m * D1;
    if (lane < m) gp[o + lane] = gb0;
    o += m;
#pragma unroll
    for (int kk = 0; kk < MP; ++kk) if (lane < m && kk < m) gp[o + (long)lane * m + kk] = gK1[kk];
    o += (long)m * m;
    if (lane < m) gp[o + lane] = gb1;
    o += m;
    if (lane < m) gp[o + lane] = gw;
    o += m;
    if (lane < D1) gp[o + lane] = gcw;
    o += D1;
    if (lane == 0) gp[o] = gcb;
    o += 1;
#pragma unroll
    for (int j = 0; j < DP; ++j) if (lane < D1 && j < D1) gp[o + (long)lane * D1 + j] = gM[j];
    }
    if (la.lam0 && lane < d) la.lam0[sample * d + lane] = LAM;
}

// One projected-ascent step of the worst-case search (nocf_disturbance_ascent_f32), one wavefront per row i over its [nt, d] path of
// W / g [nt][n][d]:  W_i += step (mask o g_i) / ||mask o g_i||  (row untouched when that norm is 0 or not finite: no step, no projection),
// then W_i *= eps / ||W_i|| when ||W_i|| > eps.  Masked components take no step (left bit for bit); the projection scales the whole row.
// Both norms: every lane sums its elements e = lane, lane + 64, ... in that order, sum64 adds the lanes in a fixed order -- no atomics,
// identical inputs give identical bits.  A lane re-reads only elements it wrote itself.
__global__ void __launch_bounds__(256) disturbance_ascent_kernel(float* __restrict__ W, const float* __restrict__ g, const float* __restrict__ mask,
                                                                 long n, int nt, int d, float step, float eps) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;                                            // (wave-uniform: sum64 needs every lane of the wave)
    const int L = nt * d;
    float s = 0.f;
    for (int e = lane; e < L; e += 64) {
        const int k = e / d, i = e - k * d;
        float v = g[((long)k * n + row) * d + i];
        if (mask) v *= mask[i];
        s = fmaf(v, v, s);
    }
    const float gn = sqrtf(sum64(s));
    if (!(gn > 0.f) || !(gn <= 3.0e38f)) return;
    const float sc = step / gn;
    float q = 0.f;
    for (int e = lane; e < L; e += 64) {
        const int k = e / d, i = e - k * d;
        const long o = ((long)k * n + row) * d + i;
        float w = W[o];
        const float mk = mask ? mask[i] : 1.f;
        if (mk != 0.f) { w = fmaf(sc, mk * g[o], w); W[o] = w; }
        q = fmaf(w, w, q);
    }
    const float wn = sqrtf(sum64(q));
    if (!(wn > eps)) return;
    const float f = eps / wn;
    for (int e = lane; e < L; e += 64) {
        const int k = e / d, i = e - k * d;
        const long o = ((long)k * n + row) * d + i;
        W[o] *= f;
    }
}

// The same step for an ensemble (nocf_disturbance_ascent_ensemble_f32, DESIGN.md section 3.17): W / g are [E, nt, n, d] member-major, one
// wavefront per row of the E * n batch.  The member of a row (wave-uniform) picks its step length and radius from the device tables steps [E]
// and epss [E] and its slice of W / g; behind that the statements are disturbance_ascent_kernel's on the member's [nt, n, d] slice, so member
// e's slice carries the bits of the single-network step on a copy of it with (steps[e], epss[e]).
__global__ void __launch_bounds__(256) disturbance_ascent_ens_kernel(float* __restrict__ W, const float* __restrict__ g, const float* __restrict__ mask,
                                                                     long n, int members, int nt, int d, const float* __restrict__ steps,
                                                                     const float* __restrict__ epss) {
    const int lane = threadIdx.x & 63;
    const long grow = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (grow >= n * members) return;                                 // (wave-uniform: sum64 needs every lane of the wave)
    const long e_ = grow / n, row = grow - e_ * n;
    W += e_ * nt * n * d; g += e_ * nt * n * d;
    const float step = steps[e_], eps = epss[e_];
    const int L = nt * d;
    float s = 0.f;
    for (int e = lane; e < L; e += 64) {
        const int k = e / d, i = e - k * d;
        float v = g[((long)k * n + row) * d + i];
        if (mask) v *= mask[i];
        s = fmaf(v, v, s);
    }
    const float gn = sqrtf(sum64(s));
    if (!(gn > 0.f) || !(gn <= 3.0e38f)) return;
    const float sc = step / gn;
    float q = 0.f;
    for (int e = lane; e < L; e += 64) {
        const int k = e / d, i = e - k * d;
        const long o = ((long)k * n + row) * d + i;
        float w = W[o];
        const float mk = mask ? mask[i] : 1.f;
        if (mk != 0.f) { w = fmaf(sc, mk * g[o], w); W[o] = w; }
        q = fmaf(w, w, q);
    }
    const float wn = sqrtf(sum64(q));
    if (!(wn > eps)) return;
    const float f = eps / wn;
    for (int e = lane; e < L; e += 64) {
        const int k = e / d, i = e - k * d;
        const long o = ((long)k * n + row) * d + i;
        W[o] *= f;
    }
}
