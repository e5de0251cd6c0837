// nocf_lane.inc -- register-resident rollout for SMALL value networks (nTh = 2, m <= 32, d+1 <= 32, point-agent
// problems): one wavefront integrates one sample, a lane is a hidden unit / a state component / an agent pair.
//
// Why a second kernel: for m <= 32 the whole network is < 2.5 k parameters.  The MFMA tile kernel spends such a
// rollout in LDS round trips and barriers (~30 k cycles per evaluation for 4 samples on an otherwise idle CU).
// Here every lane keeps its row AND its column of K0, K1 and A'A in registers for the whole rollout; a matvec is
// a chain of v_readlane (broadcast of one input component into an SGPR) + v_fma, cross-lane sums are DPP
// reductions, the RK state z lives one component per lane.  No LDS, no barrier, no memory traffic between the
// load of x and the final cost row, and four samples per 256-thread workgroup run as four independent waves.
// src/Phi.py:99-138, src/OCflow.py:104-184, src/problem/{Cross2D,SwarmTraj}.py restated per lane.

__device__ __forceinline__ float lane_bcast(float v, int k) {          // k must be a compile-time constant
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k));
}
__device__ __forceinline__ float lane_bcast_u(float v, int k_uniform) { // wave-uniform runtime lane
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k_uniform));
}
__device__ __forceinline__ float wave_sum(float v) { return sum64(v); }

struct LaneArgs {
    DevPhi P;                 // the reference tensors as given (no packing needed here)
    int d, m, r, nAg;
    float cb;
    // one launch per call (round 6): sums != null -> the last workgroup to finish reduces the per-sample table into sums [8] (and means [8])
    float* sums; float* means; unsigned* ticket;
    float a0, a3, a4, a5;
};

// ENS instantiations only (include/nocf.h, nocf_rollout_ensemble_f32; the adjoint: nocf_lane_bwd.inc): the batch is E * n rows, row g is sample
// g % n of member g / n; DevPhi then holds the STACKED tensors ([E, ...], contiguous: member e's tensor begins e tensor sizes behind the base),
// xs is the member stride of x in floats (0: every member integrates the same starts) and alph the device table [E, 6] of the multipliers.
// The LAST kernel argument, behind the existing ones: their offsets, and with them every existing instantiation's instructions, stay as they are
struct EnsArgs { unsigned n; long xs; const float* alph; };

// REC: the training variant also stores every stage input (RollArgs::sAll); the evaluation variant carries no trace of it
// ONE: the instantiation WITH the last-workgroup reduction (NOCF_LANE_ONE=1, evaluation only).  Its own instantiation because the reduction's code
// at the kernel's end costs the register-resident rollout in front of it 5-7 % (swap2 0.084 -> 0.090 ms) even when it is never taken
// DIST: the disturbed rollout (RollArgs::dist, W [nt][n][d]): lane j < d adds W[k][sample][j] to its component behind step k.  The load is
// issued at the top of the step -- its address does not depend on the step -- and consumed behind the last stage.  REC and DIST together (the
// recording forward of disturbed training): the next step's first stage input is formed from the displaced z, so it is recorded displaced
// DIST == 2: the same with the entry drawn here (nocf_noise.inc: RollArgs::nzScale / nzSeed / nzRow0) where DIST == 1 loads it -- into the same
// register, at the top of the step, so every instruction behind it is shared.  Tail waves draw the noise of the row they replicate
// DIST == 3: time-correlated noise (nocf_noise.inc, DESIGN.md section 3.18): DIST == 2 with the entry formed from the lane's carried w_{k-1},
// one more register per lane for the whole rollout; single networks only (no ENS instantiation exists)
// ENS: an ensemble of E networks of one shape in one launch (DIST 0 / 1 / 2, ONE = false).  A wave is a whole sample and nothing in a workgroup is
// shared, so the only change is WHICH network, multipliers and start a wave reads: the member e = row / ensN is wave-uniform and is kept, with
// the member's eight tensor pointers and its row of the multiplier table, in scalar registers; every statement of the rollout behind these
// reads is the single-network one, so member e's rows carry the bits of the single-network call on that member.  Every ENS test is
// `if constexpr`: the other instantiations carry no trace of it
// ENS with DIST == 2: every member under its own noise level and seed (EnsNoiseArgs, nocf_noise.inc).  Both are wave-uniform like the member's
// pointers: lane j < d reads scale[e * d + j], the seed is seeds[e], and the key of a row is RollArgs::nzRow0 + the row INSIDE the member --
// members given one seed meet the same noise.  Behind these reads the DIST == 2 statements, so member e carries the bits of the single-network
// noisy call
// ENS with DIST == 1 (nocf_rollout_disturbed_ensemble_f32, DESIGN.md section 3.17; REC or not): every member under its own tensor disturbance,
// RollArgs::dist = W [E, nt, n, d] member-major -- member e's slice is the [nt, n, d] of the single-network disturbed call -- or, with
// EnsNoiseArgs::ws == 0, one [nt, n, d] for all members.  The member's slice begins e * ws floats behind the base (wave-uniform, like the
// member's other pointers) and is indexed by the step and the row INSIDE the member; the load stands where the DIST == 1 load stands, at the
// top of the step, and every statement behind it is the DIST == 1 one
// HOLD (DIST 0 / 1; no REC, ONE, ENS): the zero-order-hold rollout.  The lane keeps the sampled grad Phi in ONE register (gh) across the steps
// and calls grad_phi only when k % K == 0 -- at the step's first stage input, which carries W[k-1] already; every stage of every step is
// rhs(s, gh), the physics and the cost quadrature at the current state with p = -c held (lane d + 1, the HJB residual, gives 0), and
// ctrlFull[k+1] is the held -gh: no control evaluation behind the step.  Every HOLD test is `if constexpr`
template <int MP, int DP, bool REC, bool ONE = false, int DIST = 0, bool ENS = false, bool HOLD = false>
__global__ void __launch_bounds__(256) rollout_lane_kernel(LaneArgs la, DevProb pb, RollArgs ra, EnsArgs ea, EnsNoiseArgs nz, HoldArgs hd) {
    static_assert(!HOLD || (!REC && !ONE && !ENS && DIST <= 1), "the held rollout: evaluation of one network, W from memory or none");
    const int lane = threadIdx.x & 63;
    const long sample = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const bool live = sample < ra.n;
    const long row = live ? sample : ra.n - 1;
    const int d = la.d, D1 = d + 1, m = la.m, N = la.nAg, ad = pb.agentDim;
    DevPhi P = la.P;
    const float* xrow = ra.x;                           // (ENS: the member's block of starts, indexed by the row inside the member)
    long xr = row;
    float eA0 = 0.f, eAQ = 0.f, eAW = 0.f;              // ENS: the member's alph[0], alph_Q, alph_W
    const float* nzScale = ra.nzScale;                  // DIST == 2: the noise scale [d] and seed of this wave's rows (ENS: the member's)
    unsigned long long nzSeed = ra.nzSeed;
    const float* wmem = ra.dist;                        // ENS with DIST == 1: the member's slice [nt, ea.n, d] of the disturbance
    if constexpr (ENS) {
        const unsigned e = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)row / ea.n));
        P.K0 += (long)e * m * D1; P.b0 += (long)e * m; P.K += (long)e * m * m; P.b += (long)e * m; P.w += (long)e * m;
        P.A += (long)e * la.r * D1; P.cw += (long)e * D1; P.cbp += e;
        xrow += (long)e * ea.xs; xr = row - (long)e * ea.n;
        const float* at = ea.alph + (long)e * 6;
        eA0 = at[0]; eAQ = at[1]; eAW = at[2];
        if constexpr (DIST == 2) { nzScale = nz.scale + (long)e * d; nzSeed = nz.seeds[e]; }
        if constexpr (DIST == 1) wmem += (long)e * nz.ws;
    }
    // the multipliers and the decisions they take: the problem's (one network), the member's (ENS) -- wave-uniform either way
    auto wantWp = [&]() -> bool { if constexpr (ENS) return eAW != 0.f; else return want_W(pb); };
    auto posQ = [&]() -> bool { if constexpr (ENS) return eAQ > 0.f; else return pb.alphQ > 0.0; };
    auto alph0 = [&]() -> float { if constexpr (ENS) return eA0; else return ra.a0; };

    // ---- weights: my row and my column of every matrix, for the whole rollout
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
    for (int j = 0; j < DP; ++j) {                      // symA = A'A like the reference forms it (src/Phi.py:110)
        float a = 0.f;
        if (lane < D1 && j < D1)
            for (int q = 0; q < la.r; ++q) a += P.A[q * D1 + lane] * P.A[q * D1 + j];
        symA[j] = a;
    }
    const float b0 = lane < m ? P.b0[lane] : 0.f;
    const float b1 = lane < m ? P.b[lane] : 0.f;
    const float wv = lane < m ? P.w[lane] : 0.f;
    const float cw = lane < D1 ? P.cw[lane] : 0.f;
    const float xt = lane < d ? pb.xtarget[lane] : 0.f;
    float nzs = 0.f;                                    // this lane's component of sigma sqrt(h)
    if constexpr (DIST == 2 || DIST == 3) nzs = lane < d ? nzScale[lane] : 0.f;
    float nzs1 = 0.f, nzr = 0.f, wc = 0.f;              // DIST == 3: this lane's s1 and rho, and the carried w_{k-1} (one register per lane)
    if constexpr (DIST == 3) { nzs1 = lane < d ? ra.nzScale1[lane] : 0.f; nzr = lane < d ? ra.nzRho[lane] : 0.f; }

    // ---- agent pairs handled by this lane (two trips cover up to 128 pairs; eligibility keeps N <= 15)
    const int npairs = (N * (N - 1)) / 2;
    int pi_[2], pj_[2];
#pragma unroll
    for (int tr = 0; tr < 2; ++tr) {
        const int q = lane + 64 * tr;
        int i = 0, rem = q;
        while (i < N - 1 && rem >= N - 1 - i) { rem -= N - 1 - i; ++i; }
        pi_[tr] = (q < npairs) ? i * ad : 0;
        pj_[tr] = (q < npairs) ? (i + 1 + rem) * ad : 0;
    }
    const bool wantW = wantWp() && N >= 2;
    const float den = (float)(2.0 * pb.r * pb.r);
    const double facN = pb.training ? (N == 2 ? 2.2 : (pb.kind == NOCF_PROB_SWARMTRAJ ? 3.2 : 2.2)) : 2.0;
    const float thr = (float)(facN * pb.r);
    const float thr2 = thr * thr * 1.000002f;
    const float aQ = ENS ? eAQ : (float)pb.alphQ, aW = ENS ? eAW : (float)pb.alphW;

    // grad Phi at s (one component per lane); optionally Phi itself
    auto grad_phi = [&](float s, bool need_value, float& phival) -> float {
        float o = b0;
#pragma unroll
        for (int i = 0; i < DP; ++i) o = fmaf(k0row[i], lane_bcast(s, i), o);
        float u0, th0;
        act_pair(o, u0, th0);
        float q = b1;
#pragma unroll
        for (int k = 0; k < MP; ++k) q = fmaf(k1row[k], lane_bcast(u0, k), q);
        const float v = tanh_fast(q) * wv;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < MP; ++j) acc = fmaf(k1col[j], lane_bcast(v, j), acc);
        const float y = th0 * (wv + acc);                          // hN = 1 for nTh = 2
        float g = cw, sy = 0.f;
#pragma unroll
        for (int k = 0; k < MP; ++k) g = fmaf(k0col[k], lane_bcast(y, k), g);
#pragma unroll
        for (int j = 0; j < DP; ++j) sy = fmaf(symA[j], lane_bcast(s, j), sy);
        g += sy;
        if (need_value) {
            const float u1 = u0 + sigma_act(q);
            phival = wave_sum(lane < m ? wv * u1 : 0.f) + 0.5f * wave_sum(lane < D1 ? s * sy : 0.f)
                     + wave_sum(lane < D1 ? cw * s : 0.f) + (P.cbp ? *P.cbp : la.cb);
        }
        return g;
    };

    // right-hand side per lane: lanes < d: -p ; d: L ; d+1: |dPhi/dt - H| ; d+2: Q ; d+3: W
    auto rhs = [&](float s, float g) -> float {
        const float sp2 = wave_sum(lane < d ? g * g : 0.f);
        float qa = 0.f;
        if (pb.obstacle != NOCF_OBS_NONE && (pb.kind == NOCF_PROB_CROSS2D || posQ())) {
            const int a0 = (lane < N ? lane : 0) * ad;
            const float x0 = __shfl(s, a0), x1 = __shfl(s, a0 + 1);
            const float x2 = (ad == 3) ? __shfl(s, a0 + 2) : 0.f;
            if (lane < N) qa = (pb.kind == NOCF_PROB_CROSS2D) ? obstacle_cross2d(pb, x0, x1) : obstacle_swarm(pb, x0, x1, x2);
        }
        const float Qraw = wave_sum(qa);
        float Wv = 0.f;
        if (wantW) {
            if (N == 2) {
                float s2 = 0.f;
                for (int k = 0; k < ad; ++k) { const float e = lane_bcast_u(s, k) - lane_bcast_u(s, ad + k); s2 += e * e; }
                const float dist = sqrtf(s2);
                if (dist < thr) Wv = expf(-(dist * dist) / den);
            } else {
                float wacc = 0.f;
#pragma unroll
                for (int tr = 0; tr < 2; ++tr) {
                    float s2 = 0.f;
                    for (int k = 0; k < ad; ++k) { const float e = __shfl(s, pi_[tr] + k) - __shfl(s, pj_[tr] + k); s2 += e * e; }
                    if (lane + 64 * tr < npairs && s2 < thr2) {
                        const float dist = sqrtf(s2);
                        if (dist < thr) { const float e = expf(-(dist * dist) / den); if (e != 1.f) wacc += e; }
                    }
                }
                Wv = wave_sum(wacc);
            }
        }
        float Lg, Qret;
        if (pb.kind == NOCF_PROB_CROSS2D) { Qret = aQ * Qraw; Lg = 0.5f * sp2 + Qret; }
        else { Qret = Qraw; Lg = 0.5f * sp2 + aQ * Qraw; }
        if (wantWp()) Lg = Lg + aW * Wv;
        const float H = -Lg + sp2;
        const float gt = lane_bcast_u(g, d);
        float dz = -g;
        if (lane == d) dz = Lg;
        else if (lane == d + 1) { if constexpr (HOLD) dz = 0.f; else dz = fabsf(gt - H); }
        else if (lane == d + 2) dz = Qret;
        else if (lane == d + 3) dz = Wv;
        return (lane < d + 4) ? dz : 0.f;
    };

    // ---- state: z one component per lane (x | L | HJt | Q | W), s = stage input [x, t]
    float z = lane < d ? xrow[xr * d + lane] : 0.f;
    if (ra.zFull && live) {
        if (lane < d + 4) ra.zFull[sample * (d + 4) + lane] = z;
        if (lane < d) ra.ctrlFull[sample * ra.cdim + lane] = 0.f;
    }
    const float c16 = (float)(1.0 / 6.0), c26 = (float)(2.0 / 6.0);
    double tk = ra.t0;
    float dummy;
    float gh = 0.f;                                     // HOLD: the sampled grad Phi, this lane's component
    int kh = 0;                                         // HOLD: steps left until the next sample
    for (int k = 0; k < ra.nt; ++k) {
        const double t1k = tk + ra.h;
        const double hsd = t1k - tk;                      // stepRK4 re-derives h = t1 - t0 (src/OCflow.py:170)
        const float hs = (float)hsd;
        float wk = 0.f;
        if constexpr (DIST == 3) { wc = lane < d ? noise_corr_value(nzs, nzs1, nzr, wc, nzSeed, ra.nzRow0 + row, k, lane) : 0.f; wk = wc; }
        else if constexpr (DIST == 2) wk = lane < d ? noise_value(nzs, nzSeed, ra.nzRow0 + (ENS ? xr : row), k, lane) : 0.f;
        else if constexpr (DIST == 1 && ENS) wk = lane < d ? wmem[((long)k * ea.n + xr) * d + lane] : 0.f;
        else if constexpr (DIST == 1) wk = lane < d ? ra.dist[((long)k * ra.n + row) * d + lane] : 0.f;
        // training: the stage input s = [x, t] of every evaluation goes to sAll[(k*nstage + st)][sample][0..d] (one row per lane group)
        auto stage_g = [&](float s) -> float { if constexpr (HOLD) return gh; else return grad_phi(s, false, dummy); };
        auto record = [&](int st, int nstage, float s) {
            if (REC && ra.sAll && live && lane <= d) ra.sAll[(((long)k * nstage + st) * ra.n + sample) * (d + 1) + lane] = s;
        };
        if (ra.stepper == NOCF_RK4) {
            const float z0 = z;
            float s = lane < d ? z0 : (lane == d ? (float)tk : 0.f);
            record(0, 4, s);
            if constexpr (HOLD) { if (kh == 0) { gh = grad_phi(s, false, dummy); kh = hd.K; } --kh; }
            float K = hs * rhs(s, stage_g(s));
            float za = z0 + c16 * K;
            float xs = z0 + 0.5f * K;
            s = lane < d ? xs : (lane == d ? (float)(tk + hsd / 2) : 0.f);
            record(1, 4, s);
            K = hs * rhs(s, stage_g(s));
            za += c26 * K;
            xs = z0 + 0.5f * K;
            s = lane < d ? xs : (lane == d ? (float)(tk + hsd / 2) : 0.f);
            record(2, 4, s);
            K = hs * rhs(s, stage_g(s));
            za += c26 * K;
            xs = z0 + K;
            s = lane < d ? xs : (lane == d ? (float)(tk + hsd) : 0.f);
            record(3, 4, s);
            K = hs * rhs(s, stage_g(s));
            z = za + c16 * K;
        } else {
            const float s = lane < d ? z : (lane == d ? (float)tk : 0.f);
            record(0, 1, s);
            if constexpr (HOLD) { if (kh == 0) { gh = grad_phi(s, false, dummy); kh = hd.K; } --kh; }
            z = z + hs * rhs(s, stage_g(s));
        }
        if constexpr (DIST) z += wk;                       // (lanes >= d hold 0: the four cost components are not displaced)
        tk += ra.h;
        if (ra.zFull) {
            // src/OCflow.py:51-55: z_{k+1}, and the control from grad Phi at (x_{k+1}, tk - h)
            const float s = lane < d ? z : (lane == d ? (float)(tk - ra.h) : 0.f);
            const float g = stage_g(s);                     // (HOLD: the control applied over step k)
            if (live) {
                if (lane < d + 4) ra.zFull[((long)(k + 1) * ra.n + sample) * (d + 4) + lane] = z;
                if (lane < d) ra.ctrlFull[((long)(k + 1) * ra.n + sample) * ra.cdim + lane] = -g;
            }
        }
    }
    // ---- terminal costs (src/OCflow.py:58-76)
    {
        const float s = lane < d ? z : (lane == d ? (float)ra.t1 : 0.f);
        float phi1 = 0.f;
        const float g = grad_phi(s, true, phi1);
        const float res = lane < d ? z - xt : 0.f;
        const float cG = 0.5f * wave_sum(res * res);
        const float hjg = wave_sum(lane < d ? fabsf(g - alph0() * res) : 0.f);
        const float cL = lane_bcast_u(z, d), cHJt = lane_bcast_u(z, d + 1), cQ = lane_bcast_u(z, d + 2), cW = lane_bcast_u(z, d + 3);
        if (live) {
            if (ra.persample && lane == 0) {
                float* o = ra.persample + sample * 7;
                o[0] = cL; o[1] = cG; o[2] = cHJt; o[3] = fabsf(phi1 - alph0() * cG); o[4] = hjg; o[5] = cQ; o[6] = cW;
            }
            if (ra.z_out && lane < d + 4) ra.z_out[sample * (d + 4) + lane] = z;
        }
    }
    // ---- one launch per call: the LAST workgroup to get here forms the 7 column sums, the count, the means and Jc -- cost_sum_kernel's body, so the
    // result does not depend on which workgroup that is.  The classic last-block pattern of the HIP memory model: rows stored, agent-scope fence
    // (on gfx950: L2 write-back, the rows leave this XCD), ticket; the last one fences again (non-local lines invalidated) and reads every row.
    // (DYNAMIC LDS, passed only by a launch that has a ticket: as a static array the 14 KB were allocated for every launch of this kernel -- which
    // otherwise uses no LDS at all -- and the two-launch default came out 5 us slower per call)
    if (ONE && la.sums) {
        double* lane_sh = reinterpret_cast<double*>(lds);       // [256 * 7]
        unsigned* lane_last = reinterpret_cast<unsigned*>(lds) + 2 * 256 * 7;
        __syncthreads();                                        // (the four waves' rows are ordered in front of ...)
        if (threadIdx.x == 0) {
            __threadfence();                                    // (... ONE agent-scope release per workgroup: an L2 write-back each, they add up)
            *lane_last = (atomicInc(la.ticket, gridDim.x - 1) == gridDim.x - 1) ? 1u : 0u;      // (wraps to 0: ready for the next launch)
        }
        __syncthreads();
        if (*lane_last) {
            __threadfence();
            __syncthreads();                                    // (the flag has been read by every thread before the sums overwrite the LDS around it)
            cost_sum_body(lane_sh, ra.persample, (long)ra.n, la.sums, nullptr, MeanArgs{la.means, la.a0, la.a3, la.a4, la.a5});
        }
    }
}
