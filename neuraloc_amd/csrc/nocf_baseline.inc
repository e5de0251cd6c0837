// nocf_baseline.inc -- the direct-transcription baseline of the reference (baseline2D.py, compareCorridor.py:95-113): one initial
// state z0, the nt x d control sequence U as the unknowns, forward Euler with h = 1/nt, Adam on
//     J(U) = sum_i h L(z_{i+1}, U_i) + alphG/2 |z_nt - xtarget|^2 ,   z_{i+1} = z_i + h U_i           (baseline2D.py:42-63)
// for the point-agent problems (Cross2D, SwarmTraj: z' = u).  One workgroup per initial point; B points per launch, independent.
//
// With z' = u one iteration is parallel over (time step x agent) where the cost is:
//   forward   z_{i+1} = z_i + h U_i                         per coordinate, in the reference's order (bitwise its trajectory)
//   costs     L_i, d(h (alphQ Q + alphW W))/dz at z_{i+1}   a group of G lanes per time step: all nt steps at once
//   adjoint   lam_i = alphG (z_nt - xtarget) + sum_{j >= i} XD_j ,  dJ/dU_i = h U_i + h lam_i     (a suffix sum per coordinate)
//   Adam      elementwise on the nt x d iterate, torch's single-tensor update (torch/optim/adam.py, _single_tensor_adam)
// The physics is the fp32 device code of the rollout kernels: obstacle_cross2d / obstacle_swarm / pair_sum_cyclic / costs_point for
// the costs, NOCF_OBSTACLE_XGRAD / pair_force for the x-gradients, with their train / eval thresholds and SwarmTraj's eval-mode count.
//
// LDS (floats): U, [M, V,] Z [nt+1][d], XD [nt][d], three partial sums per thread, three cost rows [nt], 8 scalars.  Everything of a
// solve lives there: the limit is bl_layout().total floats <= 160 KiB (swarm50: nt <= 50); past it the entry points return NOCF_E_SHAPE.
// No atomics, no waiting on other workgroups: a point's result does not depend on B or on what else runs on the device.

#define NOCF_BL_MAX_NT 256

struct BaseLay {
    int oU, oM, oV, oZ, oXD, oP, oR, oS, total;
};

__host__ __device__ __forceinline__ BaseLay bl_layout(int nt, int d, int nthreads, bool adam) {
    BaseLay l;
    const int nd = nt * d;
    l.oU = 0;
    l.oM = nd;
    l.oV = adam ? 2 * nd : nd;
    l.oZ = adam ? 3 * nd : nd;
    l.oXD = l.oZ + nd + d;
    l.oP = l.oXD + nd;
    l.oR = l.oP + 3 * nthreads;
    l.oS = l.oR + 3 * nt;
    l.total = l.oS + 8;
    return l;
}

struct BaseArgs {
    const float* z0;                     // [B][d]
    float* U;                            // [B][nt][d]: eval: the controls; adam: the iterate (in / out)
    float *M, *V;                        // adam: the moments (in / out)
    float* best;                         // adam: [B] best objective so far (in / out)
    float* Ubest;                        // adam: [B][nt][d] the iterate of the best objective (in / out)
    float* hist;                         // adam: [B][niters] objective of every iteration, or null
    float* loss;                         // eval: [B] objective
    float* grad;                         // eval: [B][nt][d] dJ/dU, or null
    float* report;                       // eval: [B][5] L+G, L, G, Q, W of compareCorridor.py:100-113, or null
    float* traj;                         // eval: [B][d][nt+1] the trajectory, or null
    int d, nt, G;                        // G: lanes per time step (power of two, G * nt <= blockDim.x)
    float h, aG;
    double lr, b1, b2, eps;
    int step0, niters;
};

// Z[i+1] = Z[i] + h U[i], i = 0..nt-1, one thread per coordinate: the reference's own order and rounding (no contraction)
__device__ __forceinline__ void bl_forward(const BaseLay& ly, int d, int nt, float h) {
#pragma clang fp contract(off)
    for (int k = threadIdx.x; k < d; k += blockDim.x) {
        float z = lds[ly.oZ + k];
        int i = 0;
        for (; i + 8 <= nt; i += 8) {
            float u[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) u[q] = lds[ly.oU + (i + q) * d + k];
#pragma unroll
            for (int q = 0; q < 8; ++q) { z = z + h * u[q]; lds[ly.oZ + (i + q + 1) * d + k] = z; }
        }
        for (; i < nt; ++i) { z = z + h * lds[ly.oU + i * d + k]; lds[ly.oZ + (i + 1) * d + k] = z; }
    }
}

// Partial sums of L(z_{i + shift}, U_i) for all steps: lanes [i G, (i+1) G) take step i and leave sum U_i^2, the raw obstacle sum and the
// raw interaction sum of their share in P[0 / 1 / 2][tid].  grad: also XD[i] = h d(alphQ Q + alphW W)/dz at z_{i+shift}.
__device__ void bl_costs(const DevProb& pb, const BaseLay& ly, int d, int nt, int G, int shift, bool grad, float h) {
    const int tid = threadIdx.x, nth = blockDim.x;
    const int i = tid / G, j0 = tid - i * G;
    float sp = 0.f, vq = 0.f, vw = 0.f;
    if (i < nt) {
        const int N = pb.nAgents, ad = pb.agentDim;
        const float* x = lds + ly.oZ + (i + shift) * d;
        const float* u = lds + ly.oU + i * d;
        for (int k = j0; k < d; k += G) sp += u[k] * u[k];
        if (pb.kind == NOCF_PROB_CROSS2D) {
            if (pb.obstacle != NOCF_OBS_NONE)
                for (int a = j0; a < N; a += G) vq += obstacle_cross2d(pb, x[2 * a], x[2 * a + 1]);
        } else if (pb.obstacle != NOCF_OBS_NONE && pb.alphQ > 0.0) {
            for (int a = j0; a < N; a += G) vq += obstacle_swarm(pb, x[3 * a], x[3 * a + 1], x[3 * a + 2]);
        }
        const bool wantW = want_W(pb) && N >= 2;
        const float den = (float)(2.0 * pb.r * pb.r);
        const double fac = pb.training ? (N == 2 ? 2.2 : (pb.kind == NOCF_PROB_SWARMTRAJ ? 3.2 : 2.2)) : 2.0;
        const float thr = (float)(fac * pb.r);
        if (wantW) {
            if (N == 2) {                                      // Cross2D.py:137-148 / SwarmTraj.py:139-147: no exclusion of 1's
                if (j0 == 0) {
                    float s2 = 0.f;
                    for (int k = 0; k < ad; ++k) { const float e = x[k] - x[ad + k]; s2 += e * e; }
                    const float dist = sqrtf(s2);
                    if (dist < thr) vw = expf(-(dist * dist) / den);
                }
            } else {
                const float thr2 = thr * thr * 1.000002f;
                vw = (ad == 3) ? pair_sum_cyclic<3>(x, N, j0, G, thr, thr2, den) : pair_sum_cyclic<2>(x, N, j0, G, thr, thr2, den);
            }
        }
        if (grad) {
            // eval mode: the hard obstacles are counts (no gradient); softcorridor's cost is the same in both modes
            const bool obsGrad = pb.obstacle != NOCF_OBS_NONE && (pb.training || pb.obstacle == NOCF_OBS_SOFTCORRIDOR);
            const float inv_r2 = 1.f / ((float)pb.r * (float)pb.r);
            const float cq = h * (float)pb.alphQ, cw = h * (float)pb.alphW;
            float* xd = lds + ly.oXD + i * d;
            for (int a = j0; a < N; a += G) {
                float gq[3] = {0.f, 0.f, 0.f}, gw[3] = {0.f, 0.f, 0.f};
                if (obsGrad) NOCF_OBSTACLE_XGRAD(pb, x, a, gq)
                if (wantW) {
                    if (ad == 2) pair_force<2>(x, a, 0, N, thr, den, inv_r2, N > 2, gw);
                    else pair_force<3>(x, a, 0, N, thr, den, inv_r2, N > 2, gw);
                }
                // written out: a contractible a * b + c * d may fuse either product, differently in the two kernels that inline this
                for (int k = 0; k < ad; ++k) xd[ad * a + k] = fmaf(cq, gq[k], cw * gw[k]);
            }
        }
    }
    lds[ly.oP + tid] = sp;
    lds[ly.oP + nth + tid] = vq;
    lds[ly.oP + 2 * nth + tid] = vw;
}

// After bl_costs and a barrier: R[0 / 1 / 2][i] = L, Q, W of step i (calcLHQW's values, costs_point), and S[1] = |z_nt - xtarget|^2 / 2
// (the last wave, fixed-order lane sums).  Ends with a barrier.
__device__ void bl_rows(const DevProb& pb, const BaseLay& ly, int d, int nt, int G) {
    const int tid = threadIdx.x, nth = blockDim.x;
    if (tid < nt) {
        float sp = 0.f, vq = 0.f, vw = 0.f;
        for (int j = 0; j < G; ++j) {
            sp += lds[ly.oP + tid * G + j];
            vq += lds[ly.oP + nth + tid * G + j];
            vw += lds[ly.oP + 2 * nth + tid * G + j];
        }
        const Costs c = costs_point(pb, sp, vq, vw);
        lds[ly.oR + tid] = c.L;
        lds[ly.oR + nt + tid] = c.Q;
        lds[ly.oR + 2 * nt + tid] = c.W;
    }
    if ((tid >> 6) == (nth >> 6) - 1) {
        const int lane = tid & 63;
        float s = 0.f;
        for (int k = lane; k < d; k += 64) { const float e = lds[ly.oZ + nt * d + k] - pb.xtarget[k]; s += e * e; }
        s = sum64(s);
        if (lane == 0) lds[ly.oS + 1] = 0.5f * s;
    }
    __syncthreads();
}

// thread 0: J = sum_i h L_i (the reference's running sum) + alphG cG  ->  S[0]
__device__ __forceinline__ float bl_objective(const BaseLay& ly, int nt, float h, float aG) {
#pragma clang fp contract(off)
    float acc = 0.f;
    for (int i = 0; i < nt; ++i) acc = acc + h * lds[ly.oR + i];
    return acc + aG * lds[ly.oS + 1];
}

// dJ/dU_i = h U_i + h lam_{i+1}, lam_{i+1} = alphG (z_nt - xtarget) + sum_{j >= i} XD_j: a suffix sum per coordinate.  Into XD (in place)
// and, when out != null, to out [nt][d].
__device__ __forceinline__ void bl_adjoint(const DevProb& pb, const BaseLay& ly, int d, int nt, float h, float aG, float* out) {
#pragma clang fp contract(off)
    for (int k = threadIdx.x; k < d; k += blockDim.x) {
        float lam = aG * (lds[ly.oZ + nt * d + k] - pb.xtarget[k]);
        for (int i = nt - 1; i >= 0; --i) {
            lam += lds[ly.oXD + i * d + k];
            const float g = fmaf(h, lds[ly.oU + i * d + k], h * lam);   // one fixed rounding: the eval and the Adam kernel agree
            lds[ly.oXD + i * d + k] = g;
            if (out) out[i * d + k] = g;
        }
    }
}

__global__ void __launch_bounds__(1024) baseline_eval_kernel(DevProb pb, BaseArgs ba) {
    const BaseLay ly = bl_layout(ba.nt, ba.d, blockDim.x, false);
    const long b = blockIdx.x;
    const int d = ba.d, nt = ba.nt, nd = nt * d, tid = threadIdx.x, nth = blockDim.x;
    const float* U = ba.U + b * nd;
    for (int e = tid; e < nd; e += nth) lds[ly.oU + e] = U[e];
    for (int k = tid; k < d; k += nth) lds[ly.oZ + k] = ba.z0[b * d + k];
    __syncthreads();
    bl_forward(ly, d, nt, ba.h);
    __syncthreads();
    bl_costs(pb, ly, d, nt, ba.G, 1, ba.grad != nullptr, ba.h);
    __syncthreads();
    bl_rows(pb, ly, d, nt, ba.G);
    if (tid == 0) ba.loss[b] = bl_objective(ly, nt, ba.h, ba.aG);
    if (ba.grad) bl_adjoint(pb, ly, d, nt, ba.h, ba.aG, ba.grad + b * nd);
    if (ba.traj)
        for (int e = tid; e < d * (nt + 1); e += nth) {
            const int k = e / (nt + 1), j = e - k * (nt + 1);
            ba.traj[b * d * (nt + 1) + e] = lds[ly.oZ + j * d + k];
        }
    if (!ba.report) return;
    // the report (compareCorridor.py:100-113): L(z_j, U_j) at the state BEFORE the step, sums of h L, h Q, h W; the same G
    __syncthreads();
    bl_costs(pb, ly, d, nt, ba.G, 0, false, ba.h);
    __syncthreads();
    bl_rows(pb, ly, d, nt, ba.G);
    if (tid == 0) {
#pragma clang fp contract(off)
        float aL = 0.f, aQ = 0.f, aW = 0.f;
        for (int j = 0; j < nt; ++j) {
            aL = aL + ba.h * lds[ly.oR + j];
            aQ = aQ + ba.h * lds[ly.oR + nt + j];
            aW = aW + ba.h * lds[ly.oR + 2 * nt + j];
        }
        const float G = ba.aG * lds[ly.oS + 1];
        float* r = ba.report + b * 5;
        r[0] = G + aL; r[1] = aL; r[2] = G; r[3] = aQ; r[4] = aW;
    }
}

// niters Adam iterations of baseline2D.py:88-105 in one launch: evaluate J(U); if J < best keep U as Ubest; dJ/dU; Adam step.
// Steps are numbered from step0 + 1 (torch's state['step']), so a solve split over launches is bitwise one launch.
__global__ void __launch_bounds__(1024) baseline_adam_kernel(DevProb pb, BaseArgs ba) {
    const BaseLay ly = bl_layout(ba.nt, ba.d, blockDim.x, true);
    const long b = blockIdx.x;
    const int d = ba.d, nt = ba.nt, nd = nt * d, tid = threadIdx.x, nth = blockDim.x;
    float* U = ba.U + b * nd;
    float* M = ba.M + b * nd;
    float* V = ba.V + b * nd;
    float* Ub = ba.Ubest + b * nd;
    for (int e = tid; e < nd; e += nth) { lds[ly.oU + e] = U[e]; lds[ly.oM + e] = M[e]; lds[ly.oV + e] = V[e]; }
    for (int k = tid; k < d; k += nth) lds[ly.oZ + k] = ba.z0[b * d + k];
    float best = ba.best[b];
    const float w1 = (float)(1.0 - ba.b1), b2 = (float)ba.b2, c2 = (float)(1.0 - ba.b2), eps = (float)ba.eps;
    __syncthreads();
    for (int it = 0; it < ba.niters; ++it) {
        bl_forward(ly, d, nt, ba.h);
        __syncthreads();
        bl_costs(pb, ly, d, nt, ba.G, 1, true, ba.h);
        __syncthreads();
        bl_rows(pb, ly, d, nt, ba.G);
        if (tid == 0) lds[ly.oS] = bl_objective(ly, nt, ba.h, ba.aG);
        bl_adjoint(pb, ly, d, nt, ba.h, ba.aG, nullptr);
        __syncthreads();
        const float J = lds[ly.oS];
        if (ba.hist && tid == 0) ba.hist[b * (long)ba.niters + it] = J;
        if (J < best) {                                   // uniform over the workgroup: every thread read the same J
            best = J;
            for (int e = tid; e < nd; e += nth) Ub[e] = lds[ly.oU + e];
        }
        // torch single-tensor Adam (CPU): m.lerp_(g, 1-b1); v.mul_(b2).addcmul_(g, g, 1-b2); bias corrections in double;
        // denom = sqrt(v) / sqrt(bc2) + eps; U.addcdiv_(m, denom, -lr / bc1), in that op order with a correctly rounded sqrt
        const double step = (double)(ba.step0 + it + 1);
        const float nss = (float)(-(ba.lr / (1.0 - pow(ba.b1, step))));
        const float bc2s = (float)sqrt(1.0 - pow(ba.b2, step));
        for (int e = tid; e < nd; e += nth) {
#pragma clang fp contract(off)
            const float g = lds[ly.oXD + e];
            float m = lds[ly.oM + e], v = lds[ly.oV + e];
            // ATen's vectorised lerp: fmadd(w, end - start, start) for |w| < 0.5, else fmadd(w - 1, end - start, end)
            m = fabsf(w1) < 0.5f ? fmaf(w1, g - m, m) : fmaf(w1 - 1.f, g - m, g);
            v = v * b2;
            v = fmaf(c2 * g, g, v);                       // ATen's vectorised addcmul: fmadd(value * t1, t2, self)
            const float den = sqrtf(v) / bc2s + eps;
            lds[ly.oM + e] = m;
            lds[ly.oV + e] = v;
            lds[ly.oU + e] = lds[ly.oU + e] + nss * m / den;
        }
        __syncthreads();
    }
    for (int e = tid; e < nd; e += nth) { U[e] = lds[ly.oU + e]; M[e] = lds[ly.oM + e]; V[e] = lds[ly.oV + e]; }
    if (tid == 0) ba.best[b] = best;
}
