// nocf_baseline_quad.inc -- the quadcopter baseline of the reference (baselineQuad.py): one initial state x0 of a single quadcopter
// (d = 12), the nt x 4 controls U as the unknowns, forward Euler with h = 1/nt, torch.optim.LBFGS (strong Wolfe) on
//     J(U) = sum_i h (2 + |U_i|^2) + alphG/2 |x_nt - xtarget|^2 ,   x_{i+1} = x_i + h dyn(U_i, x_i)        (baselineQuad.py:44-70)
//     dyn = [v, w, (u0/mass) f7(a), (u0/mass) f8(a), (u0/mass) f9(a) - grav, u1:4]      x = [p, a, v, w] (3 each), f = Quadcopter.f
// One 64-lane workgroup (one wavefront) per start; B starts per launch, independent (no atomics, no waiting on other workgroups).
//
// The forward is four layers of per-coordinate running sums: w from U[:, 1:4]; a from w; v from increments that depend only on
// that step's a and u0; p from v.  The trig, the velocity increments and the running-cost terms are parallel over time (a lane per
// step); what remains are the sequential sums, three lanes (one per coordinate) each, in the reference's order and rounding
// (x + h dx, no contraction).  The adjoint of the Euler scheme has the same shape in reverse:
//   lam_p = alphG (p_nt - p*)             constant
//   lam_v_i = lam_v_{i+1} + h lam_p       a suffix sum
//   lam_a_i = lam_a_{i+1} + h (u0_i/m) (df/da (a_i))^T lam_v_{i+1}     (the Jacobian terms: parallel over i)
//   lam_w_i = lam_w_{i+1} + h lam_a_{i+1}
//   dJ/du0_i = 2 h u0_i + (h/m) f(a_i) . lam_v_{i+1} ,   dJ/du_{1:4, i} = 2 h u_{1:4, i} + h lam_w_{i+1}
//
// The L-BFGS kernel runs a whole torch.optim.LBFGS.step (torch/optim/lbfgs.py: two-loop recursion, _strong_wolfe, _cubic_interpolate,
// every exit test in torch's order) in one launch.  Its vectors (iterate, gradient, direction, previous gradient, trial gradient, the
// two bracket gradients) live in registers, E = ceil(4 nt / 64) elements per lane, element e = lane + 64 k; the history pairs
// (s, y) live in a global workspace, [2][history][4 nt] floats per start, read back with the next pair's loads issued ahead.  The
// scalars follow torch's types: a loss is a Python float (double, widened from the fp32 objective); a dot product is an fp32 0-dim
// tensor (a fixed-order fp32 sum here); t, the bracket and the interpolation are Python floats until an fp32 tensor enters them, and
// fp32 from then on (PyNum below), with torch's rule for mixing the two.
//
// LDS (floats): U, G [4 nt], X [nt+1][12], TRIG [nt][6], DV [nt][3], TA [nt][3], LV [nt+1][3], C [nt], 8 scalars, ro / al [history].

#define NOCF_BLQ_WAVE 64

struct QuadLay {
    int oU, oG, oX, oTR, oDV, oTA, oLV, oC, oS, oRo, oAl, total;
};

__host__ __device__ __forceinline__ QuadLay blq_layout(int nt, int hist) {
    QuadLay l;
    int o = 0;
    l.oU = o; o += 4 * nt;
    l.oG = o; o += 4 * nt;
    l.oX = o; o += 12 * (nt + 1);
    l.oTR = o; o += 6 * nt;
    l.oDV = o; o += 3 * nt;
    l.oTA = o; o += 3 * nt;
    l.oLV = o; o += 3 * (nt + 1);
    l.oC = o; o += nt;
    l.oS = o; o += 8;
    l.oRo = o; o += hist;
    l.oAl = o; o += hist;
    l.total = o;
    return l;
}

struct QuadArgs {
    const float* z0;                     // [B][12]
    const float* xt;                     // [12] the target
    float* U;                            // [B][nt][4]: eval: the controls; lbfgs: the iterate (in: U0, out: the final iterate)
    float* loss;                         // [B] J (lbfgs: of the final iterate)
    float* grad;                         // eval: [B][nt][4] dJ/dU, or null
    float* report;                       // eval: [B][3] L+G, L, G, or null
    float* traj;                         // eval: [B][12][nt+1], or null
    int *n_iter, *n_evals, *reason;      // lbfgs: [B]
    float* ws;                           // lbfgs: [B][2][hist][4 nt]
    int nt, hist, max_iter, max_eval;
    float h, aG, aGh, mass, grav;        // aGh = (float)(alphG * 0.5), as baselineQuad.py:68 forms it
    double lr, tol_grad, tol_change;
};

// J at the controls in U (LDS), with X[0] = x0 already in LDS; grad: dJ/dU into G.  Every lane of the wave calls it.
// Leaves S[0 / 1 / 2] = L + G, L, G and returns J = L + G (the same value on every lane).
__device__ float blq_eval(const QuadLay& ly, const QuadArgs& qa, bool grad) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, nt = qa.nt;
    const float h = qa.h;
    const float* U = lds + ly.oU;
    float* X = lds + ly.oX;
    float* TR = lds + ly.oTR;
    float* DV = lds + ly.oDV;
    float* C = lds + ly.oC;
    // angles and angular velocities: a_{i+1} = a_i + h w_i, w_{i+1} = w_i + h u_{1+q, i}
    if (lane < 3) {
        float a = X[3 + lane], w = X[9 + lane];
        for (int i = 0; i < nt; ++i) {
            const float an = a + h * w;
            w = w + h * U[4 * i + 1 + lane];
            a = an;
            X[12 * (i + 1) + 3 + lane] = a;
            X[12 * (i + 1) + 9 + lane] = w;
        }
    }
    __syncthreads();
    // per step: sin / cos of (psi, theta, phi), the velocity increments h dv_i and the running-cost terms h (2 + |u_i|^2)
    for (int i = lane; i < nt; i += NOCF_BLQ_WAVE) {
        const float* x = X + 12 * i;
        const float* u = U + 4 * i;
        float sp, cp, st, ct, sf, cf;
        sincosf(x[3], &sp, &cp);
        sincosf(x[4], &st, &ct);
        sincosf(x[5], &sf, &cf);
        float* tr = TR + 6 * i;
        tr[0] = sp; tr[1] = st; tr[2] = sf; tr[3] = cp; tr[4] = ct; tr[5] = cf;
        const float f7 = sp * sf + (cp * st) * cf;             // Quadcopter.f, torch's op order
        const float f8 = (-cp) * sf + (sp * st) * cf;
        const float f9 = ct * cf;
        const float tmp = u[0] / qa.mass;
        DV[3 * i] = h * (tmp * f7);
        DV[3 * i + 1] = h * (tmp * f8);
        DV[3 * i + 2] = h * (tmp * f9 - qa.grav);
        const float s2 = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3];
        const float nrm = sqrtf(s2);                           // torch.norm(ctrls[i], p=2) ** 2
        C[i] = h * (2.f + nrm * nrm);
    }
    __syncthreads();
    // velocities and positions: v_{i+1} = v_i + h dv_i, p_{i+1} = p_i + h v_i
    if (lane < 3) {
        float v = X[6 + lane], p = X[lane];
        for (int i = 0; i < nt; ++i) {
            const float pn = p + h * v;
            v = v + DV[3 * i + lane];
            p = pn;
            X[12 * (i + 1) + lane] = p;
            X[12 * (i + 1) + 6 + lane] = v;
        }
    }
    __syncthreads();
    if (lane == 0) {
        float L = 0.f;
        for (int i = 0; i < nt; ++i) L = L + C[i];
        float s = 0.f;
        for (int k = 0; k < 12; ++k) { const float e = X[12 * nt + k] - qa.xt[k]; s = s + e * e; }
        const float ng = sqrtf(s);
        const float G = qa.aGh * (ng * ng);
        lds[ly.oS] = L + G;
        lds[ly.oS + 1] = L;
        lds[ly.oS + 2] = G;
    }
    __syncthreads();
    const float J = lds[ly.oS];
    if (!grad) return J;

    float* G = lds + ly.oG;
    float* TA = lds + ly.oTA;
    float* LV = lds + ly.oLV;
    const float aG = qa.aG, h2 = 2.f * h, hm = h / qa.mass;
    if (lane < 3) {                                            // lam_v_{i}, i = nt .. 1
        const float hlp = h * (aG * (X[12 * nt + lane] - qa.xt[lane]));
        float lv = aG * (X[12 * nt + 6 + lane] - qa.xt[6 + lane]);
        LV[3 * nt + lane] = lv;
        for (int i = nt - 1; i >= 1; --i) { lv = lv + hlp; LV[3 * i + lane] = lv; }
    }
    __syncthreads();
    for (int i = lane; i < nt; i += NOCF_BLQ_WAVE) {          // the Jacobian terms of lam_a, and dJ/du0
        const float* tr = TR + 6 * i;
        const float sp = tr[0], st = tr[1], sf = tr[2], cp = tr[3], ct = tr[4], cf = tr[5];
        const float l7 = LV[3 * (i + 1)], l8 = LV[3 * (i + 1) + 1], l9 = LV[3 * (i + 1) + 2];
        const float f7 = sp * sf + (cp * st) * cf;
        const float f8 = (-cp) * sf + (sp * st) * cf;
        const float f9 = ct * cf;
        const float u0 = U[4 * i];
        const float hk = h * (u0 / qa.mass);
        // d f / d psi = (-f8, f7, 0);  d f / d theta = (cp ct cf, sp ct cf, -st cf);  d f / d phi = (sp cf - cp st sf, -cp cf - sp st sf, -ct sf)
        const float gpsi = fmaf(f7, l8, -f8 * l7);
        const float gth = fmaf(-st * cf, l9, fmaf(sp * ct * cf, l8, (cp * ct * cf) * l7));
        const float gph = fmaf(-ct * sf, l9, fmaf(-cp * cf - sp * st * sf, l8, (sp * cf - cp * st * sf) * l7));
        TA[3 * i] = hk * gpsi;
        TA[3 * i + 1] = hk * gth;
        TA[3 * i + 2] = hk * gph;
        G[4 * i] = fmaf(h2, u0, hm * fmaf(f9, l9, fmaf(f8, l8, f7 * l7)));
    }
    __syncthreads();
    if (lane < 3) {                                            // lam_a, lam_w and dJ/du_{1:4}
        float la = aG * (X[12 * nt + 3 + lane] - qa.xt[3 + lane]);
        float lw = aG * (X[12 * nt + 9 + lane] - qa.xt[9 + lane]);
        for (int i = nt - 1; i >= 0; --i) {
            G[4 * i + 1 + lane] = fmaf(h2, U[4 * i + 1 + lane], h * lw);
            const float lwn = lw + h * la;
            la = la + TA[3 * i + lane];
            lw = lwn;
        }
    }
    __syncthreads();
    return J;
}

// U[b] and x0[b] into LDS
__device__ __forceinline__ void blq_load(const QuadLay& ly, const QuadArgs& qa, long b) {
    const int n = 4 * qa.nt;
    for (int e = threadIdx.x; e < n; e += NOCF_BLQ_WAVE) lds[ly.oU + e] = qa.U[b * n + e];
    if (threadIdx.x < 12) lds[ly.oX + threadIdx.x] = qa.z0[b * 12 + threadIdx.x];
    __syncthreads();
}

__global__ void __launch_bounds__(NOCF_BLQ_WAVE) baseline_quad_eval_kernel(QuadArgs qa) {
    const QuadLay ly = blq_layout(qa.nt, 0);
    const long b = blockIdx.x;
    const int nt = qa.nt, n = 4 * nt, lane = threadIdx.x;
    blq_load(ly, qa, b);
    const float J = blq_eval(ly, qa, qa.grad != nullptr);
    if (lane == 0) {
        qa.loss[b] = J;
        if (qa.report) {
            float* r = qa.report + b * 3;
            r[0] = lds[ly.oS]; r[1] = lds[ly.oS + 1]; r[2] = lds[ly.oS + 2];
        }
    }
    if (qa.grad)
        for (int e = lane; e < n; e += NOCF_BLQ_WAVE) qa.grad[b * n + e] = lds[ly.oG + e];
    if (qa.traj)
        for (int e = lane; e < 12 * (nt + 1); e += NOCF_BLQ_WAVE) {
            const int k = e / (nt + 1), j = e - k * (nt + 1);
            qa.traj[b * 12 * (nt + 1) + e] = lds[ly.oX + 12 * j + k];
        }
}

// ---- L-BFGS ------------------------------------------------------------------------------------------------------------------

// A scalar of torch's LBFGS as Python sees it: a Python float (f = false, held in double) or a 0-dim fp32 tensor (f = true).  An
// operation with a tensor operand is an fp32 operation with the Python float cast to fp32 (torch's wrapped-number promotion);
// float / tensor is tensor.__rtruediv__: reciprocal, then a multiply.
struct PyNum {
    double v;
    bool f;
};
__device__ __forceinline__ PyNum pd(double v) { return {v, false}; }
__device__ __forceinline__ PyNum pf(float v) { return {(double)v, true}; }
__device__ __forceinline__ PyNum p_add(PyNum a, PyNum b) { return (a.f || b.f) ? pf((float)a.v + (float)b.v) : pd(a.v + b.v); }
__device__ __forceinline__ PyNum p_sub(PyNum a, PyNum b) { return (a.f || b.f) ? pf((float)a.v - (float)b.v) : pd(a.v - b.v); }
__device__ __forceinline__ PyNum p_mul(PyNum a, PyNum b) { return (a.f || b.f) ? pf((float)a.v * (float)b.v) : pd(a.v * b.v); }
__device__ __forceinline__ PyNum p_div(PyNum a, PyNum b) {
    if (a.f) return pf((float)a.v / (float)b.v);
    if (b.f) return pf((1.f / (float)b.v) * (float)a.v);
    return pd(a.v / b.v);
}
__device__ __forceinline__ PyNum p_abs(PyNum a) { return {fabs(a.v), a.f}; }
__device__ __forceinline__ bool p_lt(PyNum a, PyNum b) { return (a.f || b.f) ? (float)a.v < (float)b.v : a.v < b.v; }
__device__ __forceinline__ bool p_le(PyNum a, PyNum b) { return (a.f || b.f) ? (float)a.v <= (float)b.v : a.v <= b.v; }
// Python's min(a, b) / max(a, b): the first argument unless the second compares strictly smaller / larger
__device__ __forceinline__ PyNum p_min(PyNum a, PyNum b) { return p_lt(b, a) ? b : a; }
__device__ __forceinline__ PyNum p_max(PyNum a, PyNum b) { return p_lt(a, b) ? b : a; }

// _cubic_interpolate(x1, f1, g1, x2, f2, g2, bounds): f1, f2 losses (Python floats), g1, g2 directional derivatives (fp32 tensors)
__device__ PyNum blq_cubic(PyNum x1, double f1, float g1, PyNum x2, double f2, float g2, bool bounded, PyNum lo, PyNum hi) {
    PyNum xmin = lo, xmax = hi;
    if (!bounded) {
        if (p_le(x1, x2)) { xmin = x1; xmax = x2; } else { xmin = x2; xmax = x1; }
    }
    const PyNum d1 = p_sub(pf(g1 + g2), p_div(pd(3.0 * (f1 - f2)), p_sub(x1, x2)));
    const float d1f = (float)d1.v;
    const float d2sq = d1f * d1f - g1 * g2;
    if (d2sq >= 0.f) {
        const float d2 = sqrtf(d2sq);
        PyNum mp;
        if (p_le(x1, x2)) mp = p_sub(x2, p_mul(p_sub(x2, x1), pf(((g2 + d2) - d1f) / ((g2 - g1) + 2.f * d2))));
        else mp = p_sub(x1, p_mul(p_sub(x1, x2), pf(((g1 + d2) - d1f) / ((g1 - g2) + 2.f * d2))));
        return p_min(p_max(mp, xmin), xmax);
    }
    return p_div(p_add(xmin, xmax), pd(2.0));
}

template <int E>
__device__ __forceinline__ float blq_dot(const float* a, const float* b) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < E; ++k) s = fmaf(a[k], b[k], s);
    return sum64(s);
}

template <int E>
__device__ __forceinline__ float blq_absmax(const float* a) {
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < E; ++k) m = fmaxf(m, fabsf(a[k]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}

template <int E>
__device__ __forceinline__ void blq_copy(float* dst, const float* src) {
#pragma unroll
    for (int k = 0; k < E; ++k) dst[k] = src[k];
}

// the closure at x + t d (torch's _add_grad: p.add_(d, alpha=t), a fused multiply-add with alpha in fp32), or at x itself when
// at_x: J, and dJ/dU into g
template <int E>
__device__ __forceinline__ double blq_feval(const QuadLay& ly, const QuadArgs& qa, const float* x, const float* d, PyNum t, float* g,
                                            bool at_x = false) {
    const int n = 4 * qa.nt, lane = threadIdx.x;
    const float tf = (float)t.v;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = lane + NOCF_BLQ_WAVE * k;
        if (e < n) lds[ly.oU + e] = at_x ? x[k] : fmaf(tf, d[k], x[k]);
    }
    __syncthreads();
    const float J = blq_eval(ly, qa, true);
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = lane + NOCF_BLQ_WAVE * k;
        g[k] = e < n ? lds[ly.oG + e] : 0.f;
    }
    __syncthreads();
    return (double)J;
}

template <int E>
__device__ __forceinline__ void blq_load_pair(const float* S, const float* Y, int n, float* s, float* y) {
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = threadIdx.x + NOCF_BLQ_WAVE * k;
        s[k] = e < n ? S[e] : 0.f;
        y[k] = e < n ? Y[e] : 0.f;
    }
}

// One torch.optim.LBFGS.step(closure) per start (line_search_fn = "strong_wolfe"), from U[b]; writes the final iterate back.
template <int E>
__global__ void __launch_bounds__(NOCF_BLQ_WAVE) baseline_quad_lbfgs_kernel(QuadArgs qa) {
    const int nt = qa.nt, n = 4 * nt, H = qa.hist, lane = threadIdx.x;
    const QuadLay ly = blq_layout(nt, H);
    const long b = blockIdx.x;
    float* Sb = qa.ws + (size_t)b * 2 * H * n;                // s pairs [H][n], then y pairs [H][n]
    float* Yb = Sb + (size_t)H * n;
    float* Ro = lds + ly.oRo;
    float* Al = lds + ly.oAl;
    const float tolg = (float)qa.tol_grad;
    const PyNum tolc = pd(qa.tol_change);

    float x[E], g[E], pg[E], d[E], gn[E], bg0[E], bg1[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = lane + NOCF_BLQ_WAVE * k;
        x[k] = e < n ? qa.U[b * n + e] : 0.f;
        d[k] = 0.f;
    }
    if (lane < 12) lds[ly.oX + lane] = qa.z0[b * 12 + lane];
    __syncthreads();
    double loss = blq_feval<E>(ly, qa, x, d, pd(0.0), g, true);
    int evals = 1, n_iter = 0, reason = 0;
    if (blq_absmax<E>(g) <= tolg) {
        reason = NOCF_LB_GRAD_AT_START;
    } else {
        int count = 0, head = 0;                               // history: count pairs, the oldest in slot head
        float Hdiag = 1.f;
        PyNum t = pd(0.0);
        for (;;) {
            ++n_iter;
            // ---- direction
            if (n_iter == 1) {
#pragma unroll
                for (int k = 0; k < E; ++k) d[k] = -g[k];
            } else {
                float y[E], s[E];
                const float tf = (float)t.v;
#pragma unroll
                for (int k = 0; k < E; ++k) { y[k] = g[k] - pg[k]; s[k] = d[k] * tf; }
                const float ys = blq_dot<E>(y, s);
                if (ys > (float)1e-10) {
                    int slot;
                    if (count == H) { slot = head; head = head + 1 == H ? 0 : head + 1; }
                    else { slot = head + count >= H ? head + count - H : head + count; ++count; }
#pragma unroll
                    for (int k = 0; k < E; ++k) {
                        const int e = lane + NOCF_BLQ_WAVE * k;
                        if (e < n) { Sb[(size_t)slot * n + e] = s[k]; Yb[(size_t)slot * n + e] = y[k]; }
                    }
                    Ro[slot] = 1.f / ys;
                    Hdiag = ys / blq_dot<E>(y, y);
                }
                // two-loop recursion, q (then r) in d
#pragma unroll
                for (int k = 0; k < E; ++k) d[k] = -g[k];
                // the next pair's loads are issued before this pair's reduction, up to E = 8 (at E = 16 the extra 32 registers
                // would spill)
                constexpr bool PF = E <= 8;
                constexpr int EP = PF ? E : 1;
                float sc[E], yc[E];
                if (PF && count > 0) {
                    const int sl = head + count - 1 >= H ? head + count - 1 - H : head + count - 1;
                    blq_load_pair<E>(Sb + (size_t)sl * n, Yb + (size_t)sl * n, n, sc, yc);
                }
                for (int i = count - 1; i >= 0; --i) {
                    const int sl = head + i >= H ? head + i - H : head + i;
                    float sn[EP], yn[EP];
                    if constexpr (PF) {
                        if (i > 0) {
                            const int sl2 = sl == 0 ? H - 1 : sl - 1;
                            blq_load_pair<E>(Sb + (size_t)sl2 * n, Yb + (size_t)sl2 * n, n, sn, yn);
                        }
                    } else {
                        blq_load_pair<E>(Sb + (size_t)sl * n, Yb + (size_t)sl * n, n, sc, yc);
                    }
                    const float al = blq_dot<E>(sc, d) * Ro[sl];
                    Al[i] = al;
#pragma unroll
                    for (int k = 0; k < E; ++k) d[k] = fmaf(-al, yc[k], d[k]);
                    if constexpr (PF) {
                        if (i > 0) { blq_copy<E>(sc, sn); blq_copy<E>(yc, yn); }
                    }
                }
#pragma unroll
                for (int k = 0; k < E; ++k) d[k] = d[k] * Hdiag;
                if (PF && count > 0) blq_load_pair<E>(Sb + (size_t)head * n, Yb + (size_t)head * n, n, sc, yc);
                for (int i = 0; i < count; ++i) {
                    const int sl = head + i >= H ? head + i - H : head + i;
                    float sn[EP], yn[EP];
                    if constexpr (PF) {
                        if (i + 1 < count) {
                            const int sl2 = sl + 1 == H ? 0 : sl + 1;
                            blq_load_pair<E>(Sb + (size_t)sl2 * n, Yb + (size_t)sl2 * n, n, sn, yn);
                        }
                    } else {
                        blq_load_pair<E>(Sb + (size_t)sl * n, Yb + (size_t)sl * n, n, sc, yc);
                    }
                    const float be = blq_dot<E>(yc, d) * Ro[sl];
                    const float c = Al[i] - be;
#pragma unroll
                    for (int k = 0; k < E; ++k) d[k] = fmaf(c, sc[k], d[k]);
                    if constexpr (PF) {
                        if (i + 1 < count) { blq_copy<E>(sc, sn); blq_copy<E>(yc, yn); }
                    }
                }
            }
            blq_copy<E>(pg, g);
            const double prev_loss = loss;
            // ---- initial step: min(1, 1 / |g|_1) * lr, then lr
            if (n_iter == 1) {
                float s1 = 0.f;
#pragma unroll
                for (int k = 0; k < E; ++k) s1 += fabsf(g[k]);
                s1 = sum64(s1);
                t = p_mul(p_min(pd(1.0), pf(1.f / s1)), pd(qa.lr));
            } else {
                t = pd(qa.lr);
            }
            const float gtd = blq_dot<E>(g, d);
            if (gtd > -(float)qa.tol_change) { reason = NOCF_LB_GTD; break; }

            // ---- _strong_wolfe(obj_func, x, t, d, loss, g, gtd, c1 = 1e-4, c2 = 0.9, tolerance_change = 1e-9, max_ls)
            const int max_ls = qa.max_eval - evals;
            const double f = loss;
            const PyNum c1tg = pd(1e-4);
            const float c2gtd = gtd * (float)-0.9;              // -c2 * gtd
            const float d_norm = blq_absmax<E>(d);
            double f_new = blq_feval<E>(ly, qa, x, d, t, gn);
            int ls_evals = 1;
            float gtd_new = blq_dot<E>(gn, d);
            PyNum t_prev = pd(0.0);
            double f_prev = f;
            float gtd_prev = gtd;
            blq_copy<E>(bg0, g);                               // g_prev lives in bracket slot 0 until a bracket forms
            PyNum br0 = pd(0.0), br1 = pd(0.0);
            double bf0 = 0.0, bf1 = 0.0;
            float bt0 = 0.f, bt1 = 0.f;
            int blen = 2;
            bool done = false;
            int ls_iter = 0;
            // Armijo fails: f_new > f + c1 t gtd (an fp32 comparison: gtd is a tensor)
            auto armijo_fails = [&](double fn, PyNum tt) { return p_lt(p_add(pd(f), p_mul(p_mul(c1tg, tt), pf(gtd))), pd(fn)); };
            while (ls_iter < max_ls) {
                if (armijo_fails(f_new, t) || (ls_iter > 1 && f_new >= f_prev)) {
                    br0 = t_prev; br1 = t; bf0 = f_prev; bf1 = f_new; bt0 = gtd_prev; bt1 = gtd_new;
                    blq_copy<E>(bg1, gn);
                    break;
                }
                if (fabsf(gtd_new) <= c2gtd) {
                    br0 = t; bf0 = f_new; blen = 1; done = true;
                    blq_copy<E>(bg0, gn);
                    break;
                }
                if (gtd_new >= 0.f) {
                    br0 = t_prev; br1 = t; bf0 = f_prev; bf1 = f_new; bt0 = gtd_prev; bt1 = gtd_new;
                    blq_copy<E>(bg1, gn);
                    break;
                }
                const PyNum min_step = p_add(t, p_mul(pd(0.01), p_sub(t, t_prev)));
                const PyNum max_step = p_mul(t, pd(10.0));
                const PyNum tmp = t;
                t = blq_cubic(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, true, min_step, max_step);
                t_prev = tmp;
                f_prev = f_new;
                blq_copy<E>(bg0, gn);
                gtd_prev = gtd_new;
                f_new = blq_feval<E>(ly, qa, x, d, t, gn);
                ++ls_evals;
                gtd_new = blq_dot<E>(gn, d);
                ++ls_iter;
            }
            if (ls_iter == max_ls) {
                br0 = pd(0.0); br1 = t; bf0 = f; bf1 = f_new; blen = 2;
                blq_copy<E>(bg0, pg);
                blq_copy<E>(bg1, gn);
            }
            bool insuf = false;
            int low = bf0 <= (blen == 1 ? bf0 : bf1) ? 0 : 1;
            while (!done && ls_iter < max_ls) {
                if (p_lt(p_mul(p_abs(p_sub(br1, br0)), pf(d_norm)), pd(1e-9))) break;
                t = blq_cubic(br0, bf0, bt0, br1, bf1, bt1, false, pd(0.0), pd(0.0));
                const PyNum bmax = p_max(br0, br1), bmin = p_min(br0, br1);
                const PyNum eps = p_mul(pd(0.1), p_sub(bmax, bmin));
                if (p_lt(p_min(p_sub(bmax, t), p_sub(t, bmin)), eps)) {
                    if (insuf || p_le(bmax, t) || p_le(t, bmin)) {
                        if (p_lt(p_abs(p_sub(t, bmax)), p_abs(p_sub(t, bmin)))) t = p_sub(bmax, eps);
                        else t = p_add(bmin, eps);
                        insuf = false;
                    } else {
                        insuf = true;
                    }
                } else {
                    insuf = false;
                }
                f_new = blq_feval<E>(ly, qa, x, d, t, gn);
                ++ls_evals;
                gtd_new = blq_dot<E>(gn, d);
                ++ls_iter;
                const double flow = low == 0 ? bf0 : bf1;
                if (armijo_fails(f_new, t) || f_new >= flow) {
                    if (low == 0) { br1 = t; bf1 = f_new; bt1 = gtd_new; blq_copy<E>(bg1, gn); }
                    else { br0 = t; bf0 = f_new; bt0 = gtd_new; blq_copy<E>(bg0, gn); }
                    low = bf0 <= bf1 ? 0 : 1;
                } else {
                    if (fabsf(gtd_new) <= c2gtd) {
                        done = true;
                    } else {
                        const PyNum bh = low == 0 ? br1 : br0, bl = low == 0 ? br0 : br1;
                        if ((float)p_mul(pf(gtd_new), p_sub(bh, bl)).v >= 0.f) {   // old high becomes new low
                            if (low == 0) { br1 = br0; bf1 = bf0; bt1 = bt0; blq_copy<E>(bg1, bg0); }
                            else { br0 = br1; bf0 = bf1; bt0 = bt1; blq_copy<E>(bg0, bg1); }
                        }
                    }
                    if (low == 0) { br0 = t; bf0 = f_new; bt0 = gtd_new; blq_copy<E>(bg0, gn); }
                    else { br1 = t; bf1 = f_new; bt1 = gtd_new; blq_copy<E>(bg1, gn); }
                }
            }
            if (low == 0) { t = br0; loss = bf0; blq_copy<E>(g, bg0); }
            else { t = br1; loss = bf1; blq_copy<E>(g, bg1); }
            // ---- accept: x += t d
            {
                const float tf = (float)t.v;
#pragma unroll
                for (int k = 0; k < E; ++k) x[k] = fmaf(tf, d[k], x[k]);
            }
            const bool opt_cond = blq_absmax<E>(g) <= tolg;
            evals += ls_evals;
            if (n_iter == qa.max_iter) { reason = NOCF_LB_MAX_ITER; break; }
            if (evals >= qa.max_eval) { reason = NOCF_LB_MAX_EVAL; break; }
            if (opt_cond) { reason = NOCF_LB_GRAD; break; }
            {
                float dt[E];
                const float tf = (float)t.v;
#pragma unroll
                for (int k = 0; k < E; ++k) dt[k] = d[k] * tf;
                if (p_le(pf(blq_absmax<E>(dt)), tolc)) { reason = NOCF_LB_STEP; break; }
            }
            if (fabs(loss - prev_loss) < qa.tol_change) { reason = NOCF_LB_LOSS; break; }
        }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = lane + NOCF_BLQ_WAVE * k;
        if (e < n) qa.U[b * n + e] = x[k];
    }
    if (lane == 0) {
        qa.loss[b] = (float)loss;
        qa.n_iter[b] = n_iter;
        qa.n_evals[b] = evals;
        qa.reason[b] = reason;
    }
}
