// nocf_baseline_quad.inc -- the quadcopter baseline of the reference (baselineQuad.py): one initial state x0 of a single quadcopter
// (d = 12), the nt x 4 controls U as the unknowns, forward Euler with h = 1/nt, torch.optim.LBFGS (strong Wolfe) on
//     J(U) = sum_i h (2 + |U_i|^2) + alphG/2 |x_nt - xtarget|^2 ,   x_{i+1} = x_i + h dyn(U_i, x_i)        (baselineQuad.py:44-70)
//     dyn = [v, w, (u0/mass) f7(a), (u0/mass) f8(a), (u0/mass) f9(a) - grav, u1:4]      x = [p, a, v, w] (3 each), f = Quadcopter.f
// One 64-lane workgroup (one wavefront) per start; B starts per launch, independent (no atomics, no waiting on other workgroups).
// Every kernel here is a template on the scalar type T: float (--prec single) or double (--prec double; sincos in double, precise).
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
// two bracket gradients) live in registers, E = ceil(4 nt / 64) elements per lane (a double takes two VGPRs), element e = lane + 64 k;
// wave reductions run in one fixed order per precision (sum64); the history pairs (s, y) live in a global workspace,
// [2][history][4 nt] elements per start, read back with the next pair's loads issued ahead (NOCF_BLQ_PF_E).
//
// The scalars follow torch's types (PyNum below).  A loss is a Python float (a double; in fp32 widened from the objective); a dot
// product is a 0-dim tensor of dtype T (a fixed-order sum here); t, the bracket and the interpolation are Python floats until a tensor
// enters them, and tensors from then on.  In fp32 that decides the precision of every operation on them (torch's rule for mixing the
// two).  In fp64 every quantity is a double either way and one thing is left of the tracking, at a bit per scalar: Python float /
// tensor is tensor.__rtruediv__, reciprocal() * float, and not a division; _cubic_interpolate's 3 (f1 - f2) / (x1 - x2) takes that
// path exactly when one of the two step lengths is a tensor.
//
// LDS (elements of T: blq_layout's offsets count elements): U, G [4 nt], X [nt+1][12], TRIG [nt][6], DV [nt][3], TA [nt][3],
// LV [nt+1][3], C [nt], 8 scalars, ro / al [history]  (fp64: 90 KiB at nt = 256 with 1024 pairs).

#define NOCF_BLQ_WAVE 64
// The two-loop recursion loads the next history pair ahead of the current pair's reduction up to this many elements per lane; at
// E = 16 the two extra vectors (32 registers in fp32, 64 in fp64) would spill.
#define NOCF_BLQ_PF_E 8

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

template <typename T>
struct QuadArgs {
    const T* z0;                     // [B][12]
    const T* xt;                     // [12] the target
    T* U;                            // [B][nt][4]: eval: the controls; lbfgs: the iterate (in: U0, out: the final iterate)
    T* loss;                         // [B] J (lbfgs: of the final iterate)
    T* grad;                         // eval: [B][nt][4] dJ/dU, or null
    T* report;                       // eval: [B][3] L+G, L, G, or null
    T* traj;                         // eval: [B][12][nt+1], or null
    int *n_iter, *n_evals, *reason;  // lbfgs: [B]
    T* ws;                           // lbfgs: [B][2][hist][4 nt]
    int nt, hist, max_iter, max_eval;
    T h, aG, aGh, mass, grav;        // aGh = (T)(alphG * 0.5), as baselineQuad.py:68 forms it
    double lr, tol_grad, tol_change;
};

// What differs between the two precisions beyond the type: the LDS array (fp32: the one of nocf_dev.h; fp64: an array of doubles
// over the same dynamic LDS; either way the name is known after inlining and every access is a ds_* instruction), the wave sum
// (nocf_dev.h, sum64(float): DPP rows and readlane; sum64(double): a butterfly -- each order is part of its precision's bits) and
// sincos.  sqrt / fma / fabs / fmax are overloaded already.
template <typename T> __device__ __forceinline__ T* blq_lds();
template <> __device__ __forceinline__ float* blq_lds<float>() { return lds; }
template <> __device__ __forceinline__ double* blq_lds<double>() {
    extern __shared__ double ldsd[];
    return ldsd;
}
__device__ __forceinline__ void blq_sincos(float x, float* s, float* c) { sincosf(x, s, c); }
__device__ __forceinline__ void blq_sincos(double x, double* s, double* c) { sincos(x, s, c); }

// J at the controls in U (LDS), with X[0] = x0 already in LDS; grad: dJ/dU into G.  Every lane of the wave calls it.
// Leaves S[0 / 1 / 2] = L + G, L, G and returns J = L + G (the same value on every lane).
template <typename T>
__device__ T blq_eval(const QuadLay& ly, const QuadArgs<T>& qa, bool grad) {
#pragma clang fp contract(off)
    T* const Ld = blq_lds<T>();
    const int lane = threadIdx.x, nt = qa.nt;
    const T h = qa.h;
    const T* U = Ld + ly.oU;
    T* X = Ld + ly.oX;
    T* TR = Ld + ly.oTR;
    T* DV = Ld + ly.oDV;
    T* C = Ld + ly.oC;
    // angles and angular velocities: a_{i+1} = a_i + h w_i, w_{i+1} = w_i + h u_{1+q, i}
    if (lane < 3) {
        T a = X[3 + lane], w = X[9 + lane];
        for (int i = 0; i < nt; ++i) {
            const T an = a + h * w;
            w = w + h * U[4 * i + 1 + lane];
            a = an;
            X[12 * (i + 1) + 3 + lane] = a;
            X[12 * (i + 1) + 9 + lane] = w;
        }
    }
    __syncthreads();
    // per step: sin / cos of (psi, theta, phi), the velocity increments h dv_i and the running-cost terms h (2 + |u_i|^2)
    for (int i = lane; i < nt; i += NOCF_BLQ_WAVE) {
        const T* x = X + 12 * i;
        const T* u = U + 4 * i;
        T sp, cp, st, ct, sf, cf;
        blq_sincos(x[3], &sp, &cp);
        blq_sincos(x[4], &st, &ct);
        blq_sincos(x[5], &sf, &cf);
        T* tr = TR + 6 * i;
        tr[0] = sp; tr[1] = st; tr[2] = sf; tr[3] = cp; tr[4] = ct; tr[5] = cf;
        const T f7 = sp * sf + (cp * st) * cf;             // Quadcopter.f, torch's op order
        const T f8 = (-cp) * sf + (sp * st) * cf;
        const T f9 = ct * cf;
        const T tmp = u[0] / qa.mass;
        DV[3 * i] = h * (tmp * f7);
        DV[3 * i + 1] = h * (tmp * f8);
        DV[3 * i + 2] = h * (tmp * f9 - qa.grav);
        const T s2 = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3];
        const T nrm = sqrt(s2);                           // torch.norm(ctrls[i], p=2) ** 2
        C[i] = h * (T(2) + nrm * nrm);
    }
    __syncthreads();
    // velocities and positions: v_{i+1} = v_i + h dv_i, p_{i+1} = p_i + h v_i
    if (lane < 3) {
        T v = X[6 + lane], p = X[lane];
        for (int i = 0; i < nt; ++i) {
            const T pn = p + h * v;
            v = v + DV[3 * i + lane];
            p = pn;
            X[12 * (i + 1) + lane] = p;
            X[12 * (i + 1) + 6 + lane] = v;
        }
    }
    __syncthreads();
    if (lane == 0) {
        T L = T(0);
        for (int i = 0; i < nt; ++i) L = L + C[i];
        T s = T(0);
        for (int k = 0; k < 12; ++k) { const T e = X[12 * nt + k] - qa.xt[k]; s = s + e * e; }
        const T ng = sqrt(s);
        const T G = qa.aGh * (ng * ng);
        Ld[ly.oS] = L + G;
        Ld[ly.oS + 1] = L;
        Ld[ly.oS + 2] = G;
    }
    __syncthreads();
    const T J = Ld[ly.oS];
    if (!grad) return J;

    T* G = Ld + ly.oG;
    T* TA = Ld + ly.oTA;
    T* LV = Ld + ly.oLV;
    const T aG = qa.aG, h2 = T(2) * h, hm = h / qa.mass;
    if (lane < 3) {                                            // lam_v_{i}, i = nt .. 1
        const T hlp = h * (aG * (X[12 * nt + lane] - qa.xt[lane]));
        T lv = aG * (X[12 * nt + 6 + lane] - qa.xt[6 + lane]);
        LV[3 * nt + lane] = lv;
        for (int i = nt - 1; i >= 1; --i) { lv = lv + hlp; LV[3 * i + lane] = lv; }
    }
    __syncthreads();
    for (int i = lane; i < nt; i += NOCF_BLQ_WAVE) {          // the Jacobian terms of lam_a, and dJ/du0
        const T* tr = TR + 6 * i;
        const T sp = tr[0], st = tr[1], sf = tr[2], cp = tr[3], ct = tr[4], cf = tr[5];
        const T l7 = LV[3 * (i + 1)], l8 = LV[3 * (i + 1) + 1], l9 = LV[3 * (i + 1) + 2];
        const T f7 = sp * sf + (cp * st) * cf;
        const T f8 = (-cp) * sf + (sp * st) * cf;
        const T f9 = ct * cf;
        const T u0 = U[4 * i];
        const T hk = h * (u0 / qa.mass);
        // d f / d psi = (-f8, f7, 0);  d f / d theta = (cp ct cf, sp ct cf, -st cf);  d f / d phi = (sp cf - cp st sf, -cp cf - sp st sf, -ct sf)
        const T gpsi = fma(f7, l8, -f8 * l7);
        const T gth = fma(-st * cf, l9, fma(sp * ct * cf, l8, (cp * ct * cf) * l7));
        const T gph = fma(-ct * sf, l9, fma(-cp * cf - sp * st * sf, l8, (sp * cf - cp * st * sf) * l7));
        TA[3 * i] = hk * gpsi;
        TA[3 * i + 1] = hk * gth;
        TA[3 * i + 2] = hk * gph;
        G[4 * i] = fma(h2, u0, hm * fma(f9, l9, fma(f8, l8, f7 * l7)));
    }
    __syncthreads();
    if (lane < 3) {                                            // lam_a, lam_w and dJ/du_{1:4}
        T la = aG * (X[12 * nt + 3 + lane] - qa.xt[3 + lane]);
        T lw = aG * (X[12 * nt + 9 + lane] - qa.xt[9 + lane]);
        for (int i = nt - 1; i >= 0; --i) {
            G[4 * i + 1 + lane] = fma(h2, U[4 * i + 1 + lane], h * lw);
            const T lwn = lw + h * la;
            la = la + TA[3 * i + lane];
            lw = lwn;
        }
    }
    __syncthreads();
    return J;
}

// U[b] and x0[b] into LDS
template <typename T>
__device__ __forceinline__ void blq_load(const QuadLay& ly, const QuadArgs<T>& qa, long b) {
    T* const Ld = blq_lds<T>();
    const int n = 4 * qa.nt;
    for (int e = threadIdx.x; e < n; e += NOCF_BLQ_WAVE) Ld[ly.oU + e] = qa.U[b * n + e];
    if (threadIdx.x < 12) Ld[ly.oX + threadIdx.x] = qa.z0[b * 12 + threadIdx.x];
    __syncthreads();
}

template <typename T>
__global__ void __launch_bounds__(NOCF_BLQ_WAVE) baseline_quad_eval_kernel(QuadArgs<T> qa) {
    T* const Ld = blq_lds<T>();
    const QuadLay ly = blq_layout(qa.nt, 0);
    const long b = blockIdx.x;
    const int nt = qa.nt, n = 4 * nt, lane = threadIdx.x;
    blq_load(ly, qa, b);
    const T J = blq_eval(ly, qa, qa.grad != nullptr);
    if (lane == 0) {
        qa.loss[b] = J;
        if (qa.report) {
            T* r = qa.report + b * 3;
            r[0] = Ld[ly.oS]; r[1] = Ld[ly.oS + 1]; r[2] = Ld[ly.oS + 2];
        }
    }
    if (qa.grad)
        for (int e = lane; e < n; e += NOCF_BLQ_WAVE) qa.grad[b * n + e] = Ld[ly.oG + e];
    if (qa.traj)
        for (int e = lane; e < 12 * (nt + 1); e += NOCF_BLQ_WAVE) {
            const int k = e / (nt + 1), j = e - k * (nt + 1);
            qa.traj[b * 12 * (nt + 1) + e] = Ld[ly.oX + 12 * j + k];
        }
}

// ---- L-BFGS ------------------------------------------------------------------------------------------------------------------

// A scalar of torch's LBFGS as Python sees it: a Python float (ten = false) or a 0-dim tensor of dtype T (ten = true), held in a
// double either way.  An operation with a tensor operand is an operation in T with the Python float cast to T (torch's
// wrapped-number promotion); float / tensor is tensor.__rtruediv__: reciprocal, then a multiply.  For T = double the casts do
// nothing, both branches of every operation are the same doubles, and only p_div still reads the flag.
template <typename T>
struct PyNum {
    double v;
    bool ten;
    static __device__ __forceinline__ PyNum py(double v) { return {v, false}; }
    static __device__ __forceinline__ PyNum tensor(T v) { return {(double)v, true}; }
    friend __device__ __forceinline__ PyNum p_add(PyNum a, PyNum b) { return (a.ten || b.ten) ? tensor((T)a.v + (T)b.v) : py(a.v + b.v); }
    friend __device__ __forceinline__ PyNum p_sub(PyNum a, PyNum b) { return (a.ten || b.ten) ? tensor((T)a.v - (T)b.v) : py(a.v - b.v); }
    friend __device__ __forceinline__ PyNum p_mul(PyNum a, PyNum b) { return (a.ten || b.ten) ? tensor((T)a.v * (T)b.v) : py(a.v * b.v); }
    friend __device__ __forceinline__ PyNum p_div(PyNum a, PyNum b) {
        if (a.ten) return tensor((T)a.v / (T)b.v);
        if (b.ten) return tensor((T(1) / (T)b.v) * (T)a.v);
        return py(a.v / b.v);
    }
    // a * b at the two places where the precisions round differently: the Armijo test and the minimiser in blq_cubic, each a product
    // that goes straight into a sum.  torch rounds the product on its own, and so does the fp64 kernel (no contraction).  The fp32
    // kernel has left the two contractable since it was written, the compiler makes one fma of them, and the recorded fp32 results
    // hold those bits: kept.
    friend __device__ __forceinline__ PyNum p_mul_then_sum(PyNum a, PyNum b) {
#pragma clang fp contract(off)
        if constexpr (sizeof(T) == 4) return p_mul(a, b);      // (p_mul's own multiply: contractable)
        else return (a.ten || b.ten) ? tensor((T)a.v * (T)b.v) : py(a.v * b.v);
    }
    friend __device__ __forceinline__ PyNum p_abs(PyNum a) { return {fabs(a.v), a.ten}; }
    friend __device__ __forceinline__ bool p_lt(PyNum a, PyNum b) { return (a.ten || b.ten) ? (T)a.v < (T)b.v : a.v < b.v; }
    friend __device__ __forceinline__ bool p_le(PyNum a, PyNum b) { return (a.ten || b.ten) ? (T)a.v <= (T)b.v : a.v <= b.v; }
    // Python's min(a, b) / max(a, b): the first argument unless the second compares strictly smaller / larger
    friend __device__ __forceinline__ PyNum p_min(PyNum a, PyNum b) { return p_lt(b, a) ? b : a; }
    friend __device__ __forceinline__ PyNum p_max(PyNum a, PyNum b) { return p_lt(a, b) ? b : a; }
};

// _cubic_interpolate(x1, f1, g1, x2, f2, g2, bounds): f1, f2 losses (Python floats), g1, g2 directional derivatives (tensors)
template <typename T>
__device__ PyNum<T> blq_cubic(PyNum<T> x1, double f1, T g1, PyNum<T> x2, double f2, T g2, bool bounded, PyNum<T> lo, PyNum<T> hi) {
    // No contraction of what is written out in here: torch rounds every operation.  fp64 depends on it; the fp32 instantiation comes out
    // of the compiler the same with and without (the one product it does contract is p_mul_then_sum's, outside this pragma's reach).
#pragma clang fp contract(off)
    using P = PyNum<T>;
    P xmin = lo, xmax = hi;
    if (!bounded) {
        if (p_le(x1, x2)) { xmin = x1; xmax = x2; } else { xmin = x2; xmax = x1; }
    }
    const P d1 = p_sub(P::tensor(g1 + g2), p_div(P::py(3.0 * (f1 - f2)), p_sub(x1, x2)));
    const T d1f = (T)d1.v;
    const T d2sq = d1f * d1f - g1 * g2;
    if (d2sq >= T(0)) {
        const T d2 = sqrt(d2sq);
        P mp;
        if (p_le(x1, x2)) mp = p_sub(x2, p_mul_then_sum(p_sub(x2, x1), P::tensor(((g2 + d2) - d1f) / ((g2 - g1) + T(2) * d2))));
        else mp = p_sub(x1, p_mul_then_sum(p_sub(x1, x2), P::tensor(((g1 + d2) - d1f) / ((g1 - g2) + T(2) * d2))));
        return p_min(p_max(mp, xmin), xmax);
    }
    return p_div(p_add(xmin, xmax), P::py(2.0));
}

template <int E, typename T>
__device__ __forceinline__ T blq_dot(const T* a, const T* b) {
    T s = T(0);
#pragma unroll
    for (int k = 0; k < E; ++k) s = fma(a[k], b[k], s);
    return sum64(s);
}

template <int E, typename T>
__device__ __forceinline__ T blq_absmax(const T* a) {
    T m = T(0);
#pragma unroll
    for (int k = 0; k < E; ++k) m = fmax(m, fabs(a[k]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    return m;
}

template <int E, typename T>
__device__ __forceinline__ void blq_copy(T* dst, const T* src) {
#pragma unroll
    for (int k = 0; k < E; ++k) dst[k] = src[k];
}

// the closure at x + t d (torch's _add_grad: p.add_(d, alpha=t), a fused multiply-add with alpha in T), or at x itself when
// at_x: J, and dJ/dU into g
template <int E, typename T>
__device__ __forceinline__ double blq_feval(const QuadLay& ly, const QuadArgs<T>& qa, const T* x, const T* d, PyNum<T> t, T* g,
                                            bool at_x = false) {
    T* const Ld = blq_lds<T>();
    const int n = 4 * qa.nt, lane = threadIdx.x;
    const T tf = (T)t.v;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = lane + NOCF_BLQ_WAVE * k;
        if (e < n) Ld[ly.oU + e] = at_x ? x[k] : fma(tf, d[k], x[k]);
    }
    __syncthreads();
    const T J = blq_eval(ly, qa, true);
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = lane + NOCF_BLQ_WAVE * k;
        g[k] = e < n ? Ld[ly.oG + e] : T(0);
    }
    __syncthreads();
    return (double)J;
}

template <int E, typename T>
__device__ __forceinline__ void blq_load_pair(const T* S, const T* Y, int n, T* s, T* y) {
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = threadIdx.x + NOCF_BLQ_WAVE * k;
        s[k] = e < n ? S[e] : T(0);
        y[k] = e < n ? Y[e] : T(0);
    }
}

// One torch.optim.LBFGS.step(closure) per start (line_search_fn = "strong_wolfe"), from U[b]; writes the final iterate back.
template <typename T, int E>
__global__ void __launch_bounds__(NOCF_BLQ_WAVE) baseline_quad_lbfgs_kernel(QuadArgs<T> qa) {
    using P = PyNum<T>;
    T* const Ld = blq_lds<T>();
    const int nt = qa.nt, n = 4 * nt, H = qa.hist, lane = threadIdx.x;
    const QuadLay ly = blq_layout(nt, H);
    const long b = blockIdx.x;
    T* Sb = qa.ws + (size_t)b * 2 * H * n;                // s pairs [H][n], then y pairs [H][n]
    T* Yb = Sb + (size_t)H * n;
    T* Ro = Ld + ly.oRo;
    T* Al = Ld + ly.oAl;
    const T tolg = (T)qa.tol_grad;
    const P tolc = P::py(qa.tol_change);

    T x[E], g[E], pg[E], d[E], gn[E], bg0[E], bg1[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = lane + NOCF_BLQ_WAVE * k;
        x[k] = e < n ? qa.U[b * n + e] : T(0);
        d[k] = T(0);
    }
    if (lane < 12) Ld[ly.oX + lane] = qa.z0[b * 12 + lane];
    __syncthreads();
    double loss = blq_feval<E>(ly, qa, x, d, P::py(0.0), g, true);
    int evals = 1, n_iter = 0, reason = 0;
    if (blq_absmax<E>(g) <= tolg) {
        reason = NOCF_LB_GRAD_AT_START;
    } else {
        int count = 0, head = 0;                               // history: count pairs, the oldest in slot head
        T Hdiag = T(1);
        P t = P::py(0.0);
        for (;;) {
            ++n_iter;
            // ---- direction
            if (n_iter == 1) {
#pragma unroll
                for (int k = 0; k < E; ++k) d[k] = -g[k];
            } else {
                T y[E], s[E];
                const T tf = (T)t.v;
#pragma unroll
                for (int k = 0; k < E; ++k) { y[k] = g[k] - pg[k]; s[k] = d[k] * tf; }
                const T ys = blq_dot<E>(y, s);
                if (ys > (T)1e-10) {
                    int slot;
                    if (count == H) { slot = head; head = head + 1 == H ? 0 : head + 1; }
                    else { slot = head + count >= H ? head + count - H : head + count; ++count; }
#pragma unroll
                    for (int k = 0; k < E; ++k) {
                        const int e = lane + NOCF_BLQ_WAVE * k;
                        if (e < n) { Sb[(size_t)slot * n + e] = s[k]; Yb[(size_t)slot * n + e] = y[k]; }
                    }
                    Ro[slot] = T(1) / ys;
                    Hdiag = ys / blq_dot<E>(y, y);
                }
                // two-loop recursion, q (then r) in d
#pragma unroll
                for (int k = 0; k < E; ++k) d[k] = -g[k];
                // the next pair's loads are issued before this pair's reduction, up to E = NOCF_BLQ_PF_E
                constexpr bool PF = E <= NOCF_BLQ_PF_E;
                constexpr int EP = PF ? E : 1;
                T sc[E], yc[E];
                if (PF && count > 0) {
                    const int sl = head + count - 1 >= H ? head + count - 1 - H : head + count - 1;
                    blq_load_pair<E>(Sb + (size_t)sl * n, Yb + (size_t)sl * n, n, sc, yc);
                }
                for (int i = count - 1; i >= 0; --i) {
                    const int sl = head + i >= H ? head + i - H : head + i;
                    T sn[EP], yn[EP];
                    if constexpr (PF) {
                        if (i > 0) {
                            const int sl2 = sl == 0 ? H - 1 : sl - 1;
                            blq_load_pair<E>(Sb + (size_t)sl2 * n, Yb + (size_t)sl2 * n, n, sn, yn);
                        }
                    } else {
                        blq_load_pair<E>(Sb + (size_t)sl * n, Yb + (size_t)sl * n, n, sc, yc);
                    }
                    const T al = blq_dot<E>(sc, d) * Ro[sl];
                    Al[i] = al;
#pragma unroll
                    for (int k = 0; k < E; ++k) d[k] = fma(-al, yc[k], d[k]);
                    if constexpr (PF) {
                        if (i > 0) { blq_copy<E>(sc, sn); blq_copy<E>(yc, yn); }
                    }
                }
#pragma unroll
                for (int k = 0; k < E; ++k) d[k] = d[k] * Hdiag;
                if (PF && count > 0) blq_load_pair<E>(Sb + (size_t)head * n, Yb + (size_t)head * n, n, sc, yc);
                for (int i = 0; i < count; ++i) {
                    const int sl = head + i >= H ? head + i - H : head + i;
                    T sn[EP], yn[EP];
                    if constexpr (PF) {
                        if (i + 1 < count) {
                            const int sl2 = sl + 1 == H ? 0 : sl + 1;
                            blq_load_pair<E>(Sb + (size_t)sl2 * n, Yb + (size_t)sl2 * n, n, sn, yn);
                        }
                    } else {
                        blq_load_pair<E>(Sb + (size_t)sl * n, Yb + (size_t)sl * n, n, sc, yc);
                    }
                    const T be = blq_dot<E>(yc, d) * Ro[sl];
                    const T c = Al[i] - be;
#pragma unroll
                    for (int k = 0; k < E; ++k) d[k] = fma(c, sc[k], d[k]);
                    if constexpr (PF) {
                        if (i + 1 < count) { blq_copy<E>(sc, sn); blq_copy<E>(yc, yn); }
                    }
                }
            }
            blq_copy<E>(pg, g);
            const double prev_loss = loss;
            // ---- initial step: min(1, 1 / |g|_1) * lr, then lr
            if (n_iter == 1) {
                T s1 = T(0);
#pragma unroll
                for (int k = 0; k < E; ++k) s1 += fabs(g[k]);
                s1 = sum64(s1);
                t = p_mul(p_min(P::py(1.0), P::tensor(T(1) / s1)), P::py(qa.lr));
            } else {
                t = P::py(qa.lr);
            }
            const T gtd = blq_dot<E>(g, d);
            if (gtd > -(T)qa.tol_change) { reason = NOCF_LB_GTD; break; }

            // ---- _strong_wolfe(obj_func, x, t, d, loss, g, gtd, c1 = 1e-4, c2 = 0.9, tolerance_change = 1e-9, max_ls)
            const int max_ls = qa.max_eval - evals;
            const double f = loss;
            const P c1tg = P::py(1e-4);
            const T c2gtd = gtd * (T)-0.9;              // -c2 * gtd
            const T d_norm = blq_absmax<E>(d);
            double f_new = blq_feval<E>(ly, qa, x, d, t, gn);
            int ls_evals = 1;
            T gtd_new = blq_dot<E>(gn, d);
            P t_prev = P::py(0.0);
            double f_prev = f;
            T gtd_prev = gtd;
            blq_copy<E>(bg0, g);                               // g_prev lives in bracket slot 0 until a bracket forms
            P br0 = P::py(0.0), br1 = P::py(0.0);
            double bf0 = 0.0, bf1 = 0.0;
            T bt0 = T(0), bt1 = T(0);
            int blen = 2;
            bool done = false;
            int ls_iter = 0;
            // Armijo fails: f_new > f + c1 t gtd (a comparison in T: gtd is a tensor)
            auto armijo_fails = [&](double fn, P tt) { return p_lt(p_add(P::py(f), p_mul_then_sum(p_mul(c1tg, tt), P::tensor(gtd))), P::py(fn)); };
            while (ls_iter < max_ls) {
                if (armijo_fails(f_new, t) || (ls_iter > 1 && f_new >= f_prev)) {
                    br0 = t_prev; br1 = t; bf0 = f_prev; bf1 = f_new; bt0 = gtd_prev; bt1 = gtd_new;
                    blq_copy<E>(bg1, gn);
                    break;
                }
                if (fabs(gtd_new) <= c2gtd) {
                    br0 = t; bf0 = f_new; blen = 1; done = true;
                    blq_copy<E>(bg0, gn);
                    break;
                }
                if (gtd_new >= T(0)) {
                    br0 = t_prev; br1 = t; bf0 = f_prev; bf1 = f_new; bt0 = gtd_prev; bt1 = gtd_new;
                    blq_copy<E>(bg1, gn);
                    break;
                }
                const P min_step = p_add(t, p_mul(P::py(0.01), p_sub(t, t_prev)));
                const P max_step = p_mul(t, P::py(10.0));
                const P tmp = t;
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
                br0 = P::py(0.0); br1 = t; bf0 = f; bf1 = f_new; blen = 2;
                blq_copy<E>(bg0, pg);
                blq_copy<E>(bg1, gn);
            }
            bool insuf = false;
            int low = bf0 <= (blen == 1 ? bf0 : bf1) ? 0 : 1;
            while (!done && ls_iter < max_ls) {
                if (p_lt(p_mul(p_abs(p_sub(br1, br0)), P::tensor(d_norm)), P::py(1e-9))) break;
                t = blq_cubic(br0, bf0, bt0, br1, bf1, bt1, false, P::py(0.0), P::py(0.0));
                const P bmax = p_max(br0, br1), bmin = p_min(br0, br1);
                const P eps = p_mul(P::py(0.1), p_sub(bmax, bmin));
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
                    if (fabs(gtd_new) <= c2gtd) {
                        done = true;
                    } else {
                        // gtd_new * (bracket[high] - bracket[low]).  fp64 reads the two values alone (its product is the same double
                        // either way): handing the picked PyNums on whole makes the compiler carry their padding bytes along, 36
                        // bytes of scratch per lane, which the fp32 kernel has had from the start and the fp64 kernel never.
                        const P bh = low == 0 ? br1 : br0, bl = low == 0 ? br0 : br1;
                        T slope;
                        if constexpr (sizeof(T) == 4) slope = (T)p_mul(P::tensor(gtd_new), p_sub(bh, bl)).v;
                        else slope = gtd_new * (bh.v - bl.v);
                        if (slope >= T(0)) {                   // old high becomes new low
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
                const T tf = (T)t.v;
#pragma unroll
                for (int k = 0; k < E; ++k) x[k] = fma(tf, d[k], x[k]);
            }
            const bool opt_cond = blq_absmax<E>(g) <= tolg;
            evals += ls_evals;
            if (n_iter == qa.max_iter) { reason = NOCF_LB_MAX_ITER; break; }
            if (evals >= qa.max_eval) { reason = NOCF_LB_MAX_EVAL; break; }
            if (opt_cond) { reason = NOCF_LB_GRAD; break; }
            {
                T dt[E];
                const T tf = (T)t.v;
#pragma unroll
                for (int k = 0; k < E; ++k) dt[k] = d[k] * tf;
                if (p_le(P::tensor(blq_absmax<E>(dt)), tolc)) { reason = NOCF_LB_STEP; break; }
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
        qa.loss[b] = (T)loss;
        qa.n_iter[b] = n_iter;
        qa.n_evals[b] = evals;
        qa.reason[b] = reason;
    }
}
