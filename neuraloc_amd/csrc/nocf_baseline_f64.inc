// nocf_baseline_f64.inc -- the direct-transcription baseline (nocf_baseline.inc; baseline2D.py --prec double) in double precision:
//     J(U) = sum_i h L(z_{i+1}, U_i) + alphG/2 |z_nt - xtarget|^2 ,   z_{i+1} = z_i + h U_i ,   Adam on U
// One workgroup per initial point, a whole solve in one launch, the structure of the fp32 kernels phase for phase: forward as a
// per-coordinate running sum in the reference's order (contraction off), a group of G lanes per time step for the costs and the
// x-gradients, a suffix sum per coordinate for the adjoint, torch's _single_tensor_adam step with the bias corrections in double.
// The physics is the double-precision device code of the rollout kernels, called as it stands: f64_obstacle / f64_gauss2
// (nocf_f64.inc) for the obstacle values, f64_xgrad (nocf_f64_bwd.inc) for d(alphQ Q + alphW W)/dz; the pair sum and calcLHQW's
// scalars are f64_physics' statements (they are not a function there).  f64_xgrad covers both modes: the soft corridor's Gaussians
// have the same gradient in train and eval mode, the hard corridor and the blocks are masks without a gradient in eval mode.
//
// LDS (doubles): U, Z [nt+1][d], XD [nt][d], three partial sums per thread, three cost rows [nt], 8 scalars.  The Adam moments are NOT
// in LDS: an element is always touched by the same thread, once per iteration, so they live in that thread's registers (256-thread
// launches) or stay in the global M / V arrays (1024-thread launches; see baseline_adam_f64_kernel).  bl64_layout().total doubles <= 160 KiB is the limit
// for both kernels (nocf_baseline_max_nt): swarm (d = 96) nt <= 59, swarm50 (d = 150) nt <= 38.
// No atomics, no waiting on other workgroups: a point's bits do not depend on B, and a solve split by step0 is bitwise one launch.

#define NOCF_BL64_KR 6               // Adam moments per thread of a 256-thread launch, in registers (2 x 6 doubles = 24 VGPRs)

struct Base64Lay {
    int oU, oZ, oXD, oP, oR, oS, total;
};

__host__ __device__ __forceinline__ Base64Lay bl64_layout(int nt, int d, int nthreads) {
    Base64Lay l;
    const int nd = nt * d;
    l.oU = 0;
    l.oZ = nd;
    l.oXD = l.oZ + nd + d;
    l.oP = l.oXD + nd;
    l.oR = l.oP + 3 * nthreads;
    l.oS = l.oR + 3 * nt;
    l.total = l.oS + 8;
    return l;
}

struct Base64Args {
    const double* z0;                    // [B][d]
    double* U;                           // [B][nt][d]: eval: the controls; adam: the iterate (in / out)
    double *M, *V;                       // adam: the moments (in / out)
    double* best;                        // adam: [B] best objective so far (in / out)
    double* Ubest;                       // adam: [B][nt][d] the iterate of the best objective (in / out)
    double* hist;                        // adam: [B][niters] objective of every iteration, or null
    double* loss;                        // eval: [B] objective
    double* grad;                        // eval: [B][nt][d] dJ/dU, or null
    double* report;                      // eval: [B][5] L+G, L, G, Q, W, or null
    double* traj;                        // eval: [B][d][nt+1] the trajectory, or null
    int d, nt, G;                        // G: lanes per time step (power of two, G * nt <= blockDim.x)
    double h, aG;
    double lr, b1, b2, eps;
    int step0, niters;
};

// Z[i+1] = Z[i] + h U[i], one thread per coordinate: the reference's own order and rounding (no contraction)
__device__ __forceinline__ void bl64_forward(double* L, const Base64Lay& ly, int d, int nt, double h) {
#pragma clang fp contract(off)
    for (int k = threadIdx.x; k < d; k += blockDim.x) {
        double z = L[ly.oZ + k];
        for (int i = 0; i < nt; ++i) { z = z + h * L[ly.oU + i * d + k]; L[ly.oZ + (i + 1) * d + k] = z; }
    }
}

// Partial sums of L(z_{i + shift}, U_i) for all steps: lanes [i G, (i+1) G) take step i and leave sum U_i^2, the raw obstacle sum and the
// raw interaction sum of their share in P[0 / 1 / 2][tid].  grad: also XD[i] = h d(alphQ Q + alphW W)/dz at z_{i+shift}.
__device__ void bl64_costs(double* L, const F64Prob& pb, const Base64Lay& ly, int d, int nt, int G, int shift, bool grad, double h) {
    const int tid = threadIdx.x, nth = blockDim.x;
    const int i = tid / G, j0 = tid - i * G;
    double sp = 0.0, vq = 0.0, vw = 0.0;
    if (i < nt) {
        const int N = pb.nAgents, ad = pb.agentDim;
        const double* x = L + ly.oZ + (i + shift) * d;
        const double* u = L + ly.oU + i * d;
        for (int k = j0; k < d; k += G) sp += u[k] * u[k];
        // f64_physics' sums (nocf_f64.inc), the group's lanes over the agents
        const bool wantQ = pb.obstacle != NOCF_OBS_NONE && (pb.kind == NOCF_PROB_CROSS2D || pb.alphQ > 0.0);
        if (wantQ) for (int a = j0; a < N; a += G) vq += f64_obstacle(pb, x + ad * a);
        if (pb.alphW != 0.0 && N >= 2) {
            const double den = 2.0 * pb.r * pb.r;
            if (N == 2) {
                if (j0 == 0) {
                    double s2 = 0.0;
                    for (int k = 0; k < ad; ++k) { const double e = x[k] - x[ad + k]; s2 += e * e; }
                    const double dist = sqrt(s2);
                    if (dist < (pb.training ? 2.2 : 2.0) * pb.r) vw = exp(-(dist * dist) / den);
                }
            } else {
                const double thr = (pb.training ? (pb.kind == NOCF_PROB_SWARMTRAJ ? 3.2 : 2.2) : 2.0) * pb.r;
                for (int a = j0; a < N; a += G)
                    for (int b = a + 1; b < N; ++b) {
                        double s2 = 0.0;
                        for (int k = 0; k < ad; ++k) { const double e = x[ad * a + k] - x[ad * b + k]; s2 += e * e; }
                        const double dist = sqrt(s2);
                        if (dist < thr) { const double e = exp(-(dist * dist) / den); if (e != 1.0) vw += e; }
                    }
            }
        }
        if (grad) {
            double* xd = L + ly.oXD + i * d;
            f64_xgrad(pb, x, xd, h, j0, G);
        }
    }
    L[ly.oP + tid] = sp;
    L[ly.oP + nth + tid] = vq;
    L[ly.oP + 2 * nth + tid] = vw;
}

// After bl64_costs and a barrier: R[0 / 1 / 2][i] = L, Q, W of step i (calcLHQW's values as f64_physics forms them), and
// S[1] = |z_nt - xtarget|^2 / 2 (the last wave, fixed-order lane sums).  Ends with a barrier.
__device__ void bl64_rows(double* L, const F64Prob& pb, const Base64Lay& ly, int d, int nt, int G) {
    const int tid = threadIdx.x, nth = blockDim.x;
    if (tid < nt) {
        double sp = 0.0, vq = 0.0, vw = 0.0;
        for (int j = 0; j < G; ++j) {
            sp += L[ly.oP + tid * G + j];
            vq += L[ly.oP + nth + tid * G + j];
            vw += L[ly.oP + 2 * nth + tid * G + j];
        }
        const bool wantW = pb.alphW != 0.0;
        double Q, Lg;
        if (pb.kind == NOCF_PROB_CROSS2D) { Q = pb.alphQ * vq; Lg = 0.5 * sp + Q; }
        else { Q = vq; Lg = 0.5 * sp + pb.alphQ * vq; }
        if (wantW) Lg = Lg + pb.alphW * vw;
        L[ly.oR + tid] = Lg;
        L[ly.oR + nt + tid] = Q;
        L[ly.oR + 2 * nt + tid] = wantW ? vw : 0.0;
    }
    if ((tid >> 6) == (nth >> 6) - 1) {
        const int lane = tid & 63;
        double s = 0.0;
        for (int k = lane; k < d; k += 64) { const double e = L[ly.oZ + nt * d + k] - pb.xtarget[k]; s += e * e; }
        s = sum64(s);
        if (lane == 0) L[ly.oS + 1] = 0.5 * s;
    }
    __syncthreads();
}

// J = sum_i h L_i (the reference's running sum) + alphG cG
__device__ __forceinline__ double bl64_objective(const double* L, const Base64Lay& ly, int nt, double h, double aG) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int i = 0; i < nt; ++i) acc = acc + h * L[ly.oR + i];
    return acc + aG * L[ly.oS + 1];
}

// dJ/dU_i = h U_i + h lam_{i+1}, lam_{i+1} = alphG (z_nt - xtarget) + sum_{j >= i} XD_j: a suffix sum per coordinate.  Into XD (in place)
// and, when out != null, to out [nt][d].
__device__ __forceinline__ void bl64_adjoint(double* L, const F64Prob& pb, const Base64Lay& ly, int d, int nt, double h, double aG, double* out) {
#pragma clang fp contract(off)
    for (int k = threadIdx.x; k < d; k += blockDim.x) {
        double lam = aG * (L[ly.oZ + nt * d + k] - pb.xtarget[k]);
        for (int i = nt - 1; i >= 0; --i) {
            lam += L[ly.oXD + i * d + k];
            const double g = fma(h, L[ly.oU + i * d + k], h * lam);     // one fixed rounding: the eval and the Adam kernel agree
            L[ly.oXD + i * d + k] = g;
            if (out) out[i * d + k] = g;
        }
    }
}

__global__ void __launch_bounds__(1024) baseline_eval_f64_kernel(F64Prob pb, Base64Args ba) {
    extern __shared__ double ldsd[];
    double* L = ldsd;
    const Base64Lay ly = bl64_layout(ba.nt, ba.d, blockDim.x);
    const long b = blockIdx.x;
    const int d = ba.d, nt = ba.nt, nd = nt * d, tid = threadIdx.x, nth = blockDim.x;
    const double* U = ba.U + b * nd;
    for (int e = tid; e < nd; e += nth) L[ly.oU + e] = U[e];
    for (int k = tid; k < d; k += nth) L[ly.oZ + k] = ba.z0[b * d + k];
    __syncthreads();
    bl64_forward(L, ly, d, nt, ba.h);
    __syncthreads();
    bl64_costs(L, pb, ly, d, nt, ba.G, 1, ba.grad != nullptr, ba.h);
    __syncthreads();
    bl64_rows(L, pb, ly, d, nt, ba.G);
    if (tid == 0) ba.loss[b] = bl64_objective(L, ly, nt, ba.h, ba.aG);
    if (ba.grad) bl64_adjoint(L, pb, ly, d, nt, ba.h, ba.aG, ba.grad + b * nd);
    if (ba.traj)
        for (int e = tid; e < d * (nt + 1); e += nth) {
            const int k = e / (nt + 1), j = e - k * (nt + 1);
            ba.traj[b * d * (nt + 1) + e] = L[ly.oZ + j * d + k];
        }
    if (!ba.report) return;
    // the report (compareCorridor.py:100-113): L(z_j, U_j) at the state BEFORE the step, sums of h L, h Q, h W; the same G
    __syncthreads();
    bl64_costs(L, pb, ly, d, nt, ba.G, 0, false, ba.h);
    __syncthreads();
    bl64_rows(L, pb, ly, d, nt, ba.G);
    if (tid == 0) {
#pragma clang fp contract(off)
        double aL = 0.0, aQ = 0.0, aW = 0.0;
        // The hard obstacles' eval-mode Q is a count: the reference returns the boolean mask, its sum is an integer tensor, and h * Q of
        // an integer tensor and a Python float is a float32 tensor whatever --prec says.  The reference's Q column is then an fp32
        // running sum of fp32 products (h rounded to fp32 too), also in a double-precision run; so is this one.
        const bool q32 = !pb.training && (pb.obstacle == NOCF_OBS_HARDCORRIDOR || pb.obstacle == NOCF_OBS_BLOCKS);
        float aQf = 0.f;
        for (int j = 0; j < nt; ++j) {
            aL = aL + ba.h * L[ly.oR + j];
            aQ = aQ + ba.h * L[ly.oR + nt + j];
            aQf = aQf + (float)L[ly.oR + nt + j] * (float)ba.h;
            aW = aW + ba.h * L[ly.oR + 2 * nt + j];
        }
        if (q32) aQ = (double)aQf;
        const double G = ba.aG * L[ly.oS + 1];
        double* r = ba.report + b * 5;
        r[0] = G + aL; r[1] = aL; r[2] = G; r[3] = aQ; r[4] = aW;
    }
}

// niters Adam iterations of baseline2D.py:88-105 in one launch: evaluate J(U); if J < best keep U as Ubest; dJ/dU; Adam step.
// Steps are numbered from step0 + 1 (torch's state['step']), so a solve split over launches is bitwise one launch.
// REG (launches of 256 threads: nt x agents < 512, so nt d < 1536 = NOCF_BL64_KR x 256): the moments of this thread's elements
// (e = tid + k blockDim.x) stay in registers for the whole launch.  Launches of 1024 threads have 128 VGPRs per thread, which the
// double-precision physics needs for itself: there the moments stay in the global M / V arrays, read and written once per iteration,
// consecutive threads on consecutive addresses.  Same arithmetic, same bits either way.
template <bool REG>
__global__ void __launch_bounds__(REG ? 256 : 1024) baseline_adam_f64_kernel(F64Prob pb, Base64Args ba) {
    extern __shared__ double ldsd[];
    double* L = ldsd;
    const Base64Lay ly = bl64_layout(ba.nt, ba.d, blockDim.x);
    const long b = blockIdx.x;
    const int d = ba.d, nt = ba.nt, nd = nt * d, tid = threadIdx.x, nth = blockDim.x;
    double* U = ba.U + b * nd;
    double* M = ba.M + b * nd;
    double* V = ba.V + b * nd;
    double* Ub = ba.Ubest + b * nd;
    constexpr int KR = REG ? NOCF_BL64_KR : 1;
    double mr[KR], vr[KR];
    for (int e = tid; e < nd; e += nth) L[ly.oU + e] = U[e];
    if constexpr (REG) {
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            const int e = tid + k * nth;
            mr[k] = e < nd ? M[e] : 0.0;
            vr[k] = e < nd ? V[e] : 0.0;
        }
    }
    for (int k = tid; k < d; k += nth) L[ly.oZ + k] = ba.z0[b * d + k];
    double best = ba.best[b];
    const double w1 = 1.0 - ba.b1, b2 = ba.b2, c2 = 1.0 - ba.b2, eps = ba.eps;
    __syncthreads();
    for (int it = 0; it < ba.niters; ++it) {
        bl64_forward(L, ly, d, nt, ba.h);
        __syncthreads();
        bl64_costs(L, pb, ly, d, nt, ba.G, 1, true, ba.h);
        __syncthreads();
        bl64_rows(L, pb, ly, d, nt, ba.G);
        if (tid == 0) {
            L[ly.oS] = bl64_objective(L, ly, nt, ba.h, ba.aG);
            // torch's bias corrections, formed once per iteration: S[2] = -lr / (1 - b1^step), S[3] = sqrt(1 - b2^step)
            const double step = (double)(ba.step0 + it + 1);
            L[ly.oS + 2] = -(ba.lr / (1.0 - pow(ba.b1, step)));
            L[ly.oS + 3] = sqrt(1.0 - pow(ba.b2, step));
        }
        bl64_adjoint(L, pb, ly, d, nt, ba.h, ba.aG, nullptr);
        __syncthreads();
        const double J = L[ly.oS];
        if (ba.hist && tid == 0) ba.hist[b * (long)ba.niters + it] = J;
        if (J < best) {                                   // uniform over the workgroup: every thread read the same J
            best = J;
            for (int e = tid; e < nd; e += nth) Ub[e] = L[ly.oU + e];
        }
        // torch single-tensor Adam on float64 tensors: m.lerp_(g, 1-b1); v.mul_(b2).addcmul_(g, g, 1-b2); denom = sqrt(v) / sqrt(bc2) + eps;
        // U.addcdiv_(m, denom, -lr / bc1), in that op order
        const double nss = L[ly.oS + 2], bc2s = L[ly.oS + 3];
        auto update = [&](int e, double& m, double& v) {
#pragma clang fp contract(off)
            const double g = L[ly.oXD + e];
            m = fabs(w1) < 0.5 ? fma(w1, g - m, m) : fma(w1 - 1.0, g - m, g);      // ATen's lerp
            v = v * b2;
            v = fma(c2 * g, g, v);                                                // ATen's addcmul
            const double den = sqrt(v) / bc2s + eps;
            L[ly.oU + e] = L[ly.oU + e] + nss * m / den;
        };
        if constexpr (REG) {
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                const int e = tid + k * nth;
                if (e < nd) update(e, mr[k], vr[k]);
            }
        } else {
            for (int e = tid; e < nd; e += nth) {
                double m = M[e], v = V[e];
                update(e, m, v);
                M[e] = m;
                V[e] = v;
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < nd; e += nth) U[e] = L[ly.oU + e];
    if constexpr (REG) {
#pragma unroll
        for (int k = 0; k < KR; ++k) {
            const int e = tid + k * nth;
            if (e < nd) { M[e] = mr[k]; V[e] = vr[k]; }
        }
    }
    if (tid == 0) ba.best[b] = best;
}
