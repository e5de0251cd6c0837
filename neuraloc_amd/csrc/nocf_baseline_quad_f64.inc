// nocf_baseline_quad_f64.inc -- the quadcopter baseline (nocf_baseline_quad.inc; baselineQuad.py --prec double) in double precision:
//     J(U) = sum_i h (2 + |U_i|^2) + alphG/2 |x_nt - xtarget|^2 ,   x_{i+1} = x_i + h dyn(U_i, x_i) ,   torch.optim.LBFGS (strong Wolfe)
// One 64-lane workgroup (one wavefront) per start, the fp32 kernels' structure phase for phase: four layers of per-coordinate running
// sums for the forward (three lanes each, the reference's order and rounding, no contraction), the trig / velocity increments / cost
// terms parallel over time, the adjoint of the Euler scheme in reverse; sincos in double, precise.
//
// The L-BFGS kernel mirrors torch/optim/lbfgs.py with float64 tensors.  Every quantity there is then a double -- the loss a Python float,
// a dot product a 0-dim float64 tensor -- so nothing of the fp32 kernel's promotion tracking remains, with one exception that costs a bit
// per scalar: Python float / tensor is tensor.__rtruediv__, reciprocal() * float, and not a division; _cubic_interpolate's
// 3 (f1 - f2) / (x1 - x2) takes that path exactly when one of the two step lengths is a tensor (TNum::ten below).  Vectors in registers,
// E = ceil(4 nt / 64) doubles per lane (two VGPRs each), element e = lane + 64 k; wave reductions in one fixed order; history pairs in
// the global workspace, [2][history][4 nt] doubles per start, the next pair's loads issued ahead up to E = 8 (NOCF_BLQ64_PF_E).
//
// LDS (doubles): U, G [4 nt], X [nt+1][12], TRIG [nt][6], DV [nt][3], TA [nt][3], LV [nt+1][3], C [nt], 8 scalars, ro / al [history]
// (blq_layout's offsets, counted in doubles: 90 KiB at nt = 256 with 1024 pairs).

#define NOCF_BLQ64_PF_E 8

struct Quad64Args {
    const double* z0;                    // [B][12]
    const double* xt;                    // [12] the target
    double* U;                           // [B][nt][4]: eval: the controls; lbfgs: the iterate (in: U0, out: the final iterate)
    double* loss;                        // [B] J (lbfgs: of the final iterate)
    double* grad;                        // eval: [B][nt][4] dJ/dU, or null
    double* report;                      // eval: [B][3] L+G, L, G, or null
    double* traj;                        // eval: [B][12][nt+1], or null
    int *n_iter, *n_evals, *reason;      // lbfgs: [B]
    double* ws;                          // lbfgs: [B][2][hist][4 nt]
    int nt, hist, max_iter, max_eval;
    double h, aG, aGh, mass, grav;       // aGh = alphG * 0.5, as baselineQuad.py:68 forms it
    double lr, tol_grad, tol_change;
};

__device__ __forceinline__ double blq64_sum64(double v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}

// J at the controls in U (LDS), with X[0] = x0 already in LDS; grad: dJ/dU into G.  Every lane of the wave calls it.
// Leaves S[0 / 1 / 2] = L + G, L, G and returns J = L + G (the same value on every lane).
__device__ double blq64_eval(double* Ld, const QuadLay& ly, const Quad64Args& qa, bool grad) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, nt = qa.nt;
    const double h = qa.h;
    const double* U = Ld + ly.oU;
    double* X = Ld + ly.oX;
    double* TR = Ld + ly.oTR;
    double* DV = Ld + ly.oDV;
    double* C = Ld + ly.oC;
    if (lane < 3) {                                            // a_{i+1} = a_i + h w_i, w_{i+1} = w_i + h u_{1+q, i}
        double a = X[3 + lane], w = X[9 + lane];
        for (int i = 0; i < nt; ++i) {
            const double an = a + h * w;
            w = w + h * U[4 * i + 1 + lane];
            a = an;
            X[12 * (i + 1) + 3 + lane] = a;
            X[12 * (i + 1) + 9 + lane] = w;
        }
    }
    __syncthreads();
    for (int i = lane; i < nt; i += NOCF_BLQ_WAVE) {
        const double* x = X + 12 * i;
        const double* u = U + 4 * i;
        double sp, cp, st, ct, sf, cf;
        sincos(x[3], &sp, &cp);
        sincos(x[4], &st, &ct);
        sincos(x[5], &sf, &cf);
        double* tr = TR + 6 * i;
        tr[0] = sp; tr[1] = st; tr[2] = sf; tr[3] = cp; tr[4] = ct; tr[5] = cf;
        const double f7 = sp * sf + (cp * st) * cf;            // Quadcopter.f, torch's op order
        const double f8 = (-cp) * sf + (sp * st) * cf;
        const double f9 = ct * cf;
        const double tmp = u[0] / qa.mass;
        DV[3 * i] = h * (tmp * f7);
        DV[3 * i + 1] = h * (tmp * f8);
        DV[3 * i + 2] = h * (tmp * f9 - qa.grav);
        const double s2 = ((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]) + u[3] * u[3];
        const double nrm = sqrt(s2);                           // torch.norm(ctrls[i], p=2) ** 2
        C[i] = h * (2.0 + nrm * nrm);
    }
    __syncthreads();
    if (lane < 3) {                                            // v_{i+1} = v_i + h dv_i, p_{i+1} = p_i + h v_i
        double v = X[6 + lane], p = X[lane];
        for (int i = 0; i < nt; ++i) {
            const double pn = p + h * v;
            v = v + DV[3 * i + lane];
            p = pn;
            X[12 * (i + 1) + lane] = p;
            X[12 * (i + 1) + 6 + lane] = v;
        }
    }
    __syncthreads();
    if (lane == 0) {
        double L = 0.0;
        for (int i = 0; i < nt; ++i) L = L + C[i];
        double s = 0.0;
        for (int k = 0; k < 12; ++k) { const double e = X[12 * nt + k] - qa.xt[k]; s = s + e * e; }
        const double ng = sqrt(s);
        const double G = qa.aGh * (ng * ng);
        Ld[ly.oS] = L + G;
        Ld[ly.oS + 1] = L;
        Ld[ly.oS + 2] = G;
    }
    __syncthreads();
    const double J = Ld[ly.oS];
    if (!grad) return J;

    double* G = Ld + ly.oG;
    double* TA = Ld + ly.oTA;
    double* LV = Ld + ly.oLV;
    const double aG = qa.aG, h2 = 2.0 * h, hm = h / qa.mass;
    if (lane < 3) {                                            // lam_v_{i}, i = nt .. 1
        const double hlp = h * (aG * (X[12 * nt + lane] - qa.xt[lane]));
        double lv = aG * (X[12 * nt + 6 + lane] - qa.xt[6 + lane]);
        LV[3 * nt + lane] = lv;
        for (int i = nt - 1; i >= 1; --i) { lv = lv + hlp; LV[3 * i + lane] = lv; }
    }
    __syncthreads();
    for (int i = lane; i < nt; i += NOCF_BLQ_WAVE) {          // the Jacobian terms of lam_a, and dJ/du0
        const double* tr = TR + 6 * i;
        const double sp = tr[0], st = tr[1], sf = tr[2], cp = tr[3], ct = tr[4], cf = tr[5];
        const double l7 = LV[3 * (i + 1)], l8 = LV[3 * (i + 1) + 1], l9 = LV[3 * (i + 1) + 2];
        const double f7 = sp * sf + (cp * st) * cf;
        const double f8 = (-cp) * sf + (sp * st) * cf;
        const double f9 = ct * cf;
        const double u0 = U[4 * i];
        const double hk = h * (u0 / qa.mass);
        // d f / d psi = (-f8, f7, 0);  d f / d theta = (cp ct cf, sp ct cf, -st cf);  d f / d phi = (sp cf - cp st sf, -cp cf - sp st sf, -ct sf)
        const double gpsi = fma(f7, l8, -f8 * l7);
        const double gth = fma(-st * cf, l9, fma(sp * ct * cf, l8, (cp * ct * cf) * l7));
        const double gph = fma(-ct * sf, l9, fma(-cp * cf - sp * st * sf, l8, (sp * cf - cp * st * sf) * l7));
        TA[3 * i] = hk * gpsi;
        TA[3 * i + 1] = hk * gth;
        TA[3 * i + 2] = hk * gph;
        G[4 * i] = fma(h2, u0, hm * fma(f9, l9, fma(f8, l8, f7 * l7)));
    }
    __syncthreads();
    if (lane < 3) {                                            // lam_a, lam_w and dJ/du_{1:4}
        double la = aG * (X[12 * nt + 3 + lane] - qa.xt[3 + lane]);
        double lw = aG * (X[12 * nt + 9 + lane] - qa.xt[9 + lane]);
        for (int i = nt - 1; i >= 0; --i) {
            G[4 * i + 1 + lane] = fma(h2, U[4 * i + 1 + lane], h * lw);
            const double lwn = lw + h * la;
            la = la + TA[3 * i + lane];
            lw = lwn;
        }
    }
    __syncthreads();
    return J;
}

__global__ void __launch_bounds__(NOCF_BLQ_WAVE) baseline_quad_eval_f64_kernel(Quad64Args qa) {
    extern __shared__ double ldsd[];
    double* Ld = ldsd;
    const QuadLay ly = blq_layout(qa.nt, 0);
    const long b = blockIdx.x;
    const int nt = qa.nt, n = 4 * nt, lane = threadIdx.x;
    for (int e = lane; e < n; e += NOCF_BLQ_WAVE) Ld[ly.oU + e] = qa.U[b * n + e];
    if (lane < 12) Ld[ly.oX + lane] = qa.z0[b * 12 + lane];
    __syncthreads();
    const double J = blq64_eval(Ld, ly, qa, qa.grad != nullptr);
    if (lane == 0) {
        qa.loss[b] = J;
        if (qa.report) {
            double* r = qa.report + b * 3;
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

// a step length of torch's line search: its value, and whether Python holds it as a 0-dim tensor (ten) or as a float.  Sums, differences
// and products are the same doubles either way; only float / tensor differs (t_rdiv).
struct TNum {
    double v;
    bool ten;
};
__device__ __forceinline__ TNum tfl(double v) { return {v, false}; }
__device__ __forceinline__ TNum tten(double v) { return {v, true}; }
__device__ __forceinline__ TNum t_add(TNum a, TNum b) { return {a.v + b.v, a.ten || b.ten}; }
__device__ __forceinline__ TNum t_sub(TNum a, TNum b) { return {a.v - b.v, a.ten || b.ten}; }
__device__ __forceinline__ TNum t_mul(TNum a, TNum b) { return {a.v * b.v, a.ten || b.ten}; }
// Python float a over b: a true division when b is a float, tensor.__rtruediv__ (reciprocal, then a multiply) when b is a tensor
__device__ __forceinline__ double t_rdiv(double a, TNum b) { return b.ten ? (1.0 / b.v) * a : a / b.v; }
// Python's min(a, b) / max(a, b): the first argument unless the second compares strictly smaller / larger
__device__ __forceinline__ TNum t_min(TNum a, TNum b) { return b.v < a.v ? b : a; }
__device__ __forceinline__ TNum t_max(TNum a, TNum b) { return a.v < b.v ? b : a; }

// _cubic_interpolate(x1, f1, g1, x2, f2, g2, bounds): f1, f2 losses (Python floats), g1, g2 directional derivatives (tensors)
__device__ TNum blq64_cubic(TNum x1, double f1, double g1, TNum x2, double f2, double g2, bool bounded, TNum lo, TNum hi) {
#pragma clang fp contract(off)
    TNum xmin = lo, xmax = hi;
    if (!bounded) {
        if (x1.v <= x2.v) { xmin = x1; xmax = x2; } else { xmin = x2; xmax = x1; }
    }
    const double d1 = (g1 + g2) - t_rdiv(3.0 * (f1 - f2), t_sub(x1, x2));
    const double d2sq = d1 * d1 - g1 * g2;
    if (d2sq >= 0.0) {
        const double d2 = sqrt(d2sq);
        TNum mp;
        if (x1.v <= x2.v) mp = tten(x2.v - (x2.v - x1.v) * (((g2 + d2) - d1) / ((g2 - g1) + 2.0 * d2)));
        else mp = tten(x1.v - (x1.v - x2.v) * (((g1 + d2) - d1) / ((g1 - g2) + 2.0 * d2)));
        return t_min(t_max(mp, xmin), xmax);
    }
    return {(xmin.v + xmax.v) / 2.0, xmin.ten || xmax.ten};
}

template <int E>
__device__ __forceinline__ double blq64_dot(const double* a, const double* b) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) s = fma(a[k], b[k], s);
    return blq64_sum64(s);
}

template <int E>
__device__ __forceinline__ double blq64_absmax(const double* a) {
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) m = fmax(m, fabs(a[k]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    return m;
}

template <int E>
__device__ __forceinline__ void blq64_copy(double* dst, const double* src) {
#pragma unroll
    for (int k = 0; k < E; ++k) dst[k] = src[k];
}

// the closure at x + t d (torch's _add_grad: p.add_(d, alpha=t), a fused multiply-add), or at x itself when at_x: J, and dJ/dU into g
template <int E>
__device__ __forceinline__ double blq64_feval(double* Ld, const QuadLay& ly, const Quad64Args& qa, const double* x, const double* d, double t,
                                              double* g, bool at_x = false) {
    const int n = 4 * qa.nt, lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = lane + NOCF_BLQ_WAVE * k;
        if (e < n) Ld[ly.oU + e] = at_x ? x[k] : fma(t, d[k], x[k]);
    }
    __syncthreads();
    const double J = blq64_eval(Ld, ly, qa, true);
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = lane + NOCF_BLQ_WAVE * k;
        g[k] = e < n ? Ld[ly.oG + e] : 0.0;
    }
    __syncthreads();
    return J;
}

template <int E>
__device__ __forceinline__ void blq64_load_pair(const double* S, const double* Y, int n, double* s, double* y) {
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = threadIdx.x + NOCF_BLQ_WAVE * k;
        s[k] = e < n ? S[e] : 0.0;
        y[k] = e < n ? Y[e] : 0.0;
    }
}

// One torch.optim.LBFGS.step(closure) per start (line_search_fn = "strong_wolfe"), from U[b]; writes the final iterate back.
template <int E>
__global__ void __launch_bounds__(NOCF_BLQ_WAVE) baseline_quad_lbfgs_f64_kernel(Quad64Args qa) {
    extern __shared__ double ldsd[];
    double* Ld = ldsd;
    const int nt = qa.nt, n = 4 * nt, H = qa.hist, lane = threadIdx.x;
    const QuadLay ly = blq_layout(nt, H);
    const long b = blockIdx.x;
    double* Sb = qa.ws + (size_t)b * 2 * H * n;               // s pairs [H][n], then y pairs [H][n]
    double* Yb = Sb + (size_t)H * n;
    double* Ro = Ld + ly.oRo;
    double* Al = Ld + ly.oAl;
    const double tolg = qa.tol_grad, tolc = qa.tol_change;

    double x[E], g[E], pg[E], d[E], gn[E], bg0[E], bg1[E];
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = lane + NOCF_BLQ_WAVE * k;
        x[k] = e < n ? qa.U[b * n + e] : 0.0;
        d[k] = 0.0;
    }
    if (lane < 12) Ld[ly.oX + lane] = qa.z0[b * 12 + lane];
    __syncthreads();
    double loss = blq64_feval<E>(Ld, ly, qa, x, d, 0.0, g, true);
    int evals = 1, n_iter = 0, reason = 0;
    if (blq64_absmax<E>(g) <= tolg) {
        reason = NOCF_LB_GRAD_AT_START;
    } else {
        int count = 0, head = 0;                               // history: count pairs, the oldest in slot head
        double Hdiag = 1.0;
        TNum t = tfl(0.0);
        for (;;) {
            ++n_iter;
            // ---- direction
            if (n_iter == 1) {
#pragma unroll
                for (int k = 0; k < E; ++k) d[k] = -g[k];
            } else {
                double y[E], s[E];
#pragma unroll
                for (int k = 0; k < E; ++k) { y[k] = g[k] - pg[k]; s[k] = d[k] * t.v; }
                const double ys = blq64_dot<E>(y, s);
                if (ys > 1e-10) {
                    int slot;
                    if (count == H) { slot = head; head = head + 1 == H ? 0 : head + 1; }
                    else { slot = head + count >= H ? head + count - H : head + count; ++count; }
#pragma unroll
                    for (int k = 0; k < E; ++k) {
                        const int e = lane + NOCF_BLQ_WAVE * k;
                        if (e < n) { Sb[(size_t)slot * n + e] = s[k]; Yb[(size_t)slot * n + e] = y[k]; }
                    }
                    Ro[slot] = 1.0 / ys;
                    Hdiag = ys / blq64_dot<E>(y, y);
                }
                // two-loop recursion, q (then r) in d; the next pair's loads are issued before this pair's reduction up to E = 8
                // (at E = 16 the extra 64 registers would spill)
#pragma unroll
                for (int k = 0; k < E; ++k) d[k] = -g[k];
                constexpr bool PF = E <= NOCF_BLQ64_PF_E;
                constexpr int EP = PF ? E : 1;
                double sc[E], yc[E];
                if (PF && count > 0) {
                    const int sl = head + count - 1 >= H ? head + count - 1 - H : head + count - 1;
                    blq64_load_pair<E>(Sb + (size_t)sl * n, Yb + (size_t)sl * n, n, sc, yc);
                }
                for (int i = count - 1; i >= 0; --i) {
                    const int sl = head + i >= H ? head + i - H : head + i;
                    double sn[EP], yn[EP];
                    if constexpr (PF) {
                        if (i > 0) {
                            const int sl2 = sl == 0 ? H - 1 : sl - 1;
                            blq64_load_pair<E>(Sb + (size_t)sl2 * n, Yb + (size_t)sl2 * n, n, sn, yn);
                        }
                    } else {
                        blq64_load_pair<E>(Sb + (size_t)sl * n, Yb + (size_t)sl * n, n, sc, yc);
                    }
                    const double al = blq64_dot<E>(sc, d) * Ro[sl];
                    Al[i] = al;
#pragma unroll
                    for (int k = 0; k < E; ++k) d[k] = fma(-al, yc[k], d[k]);
                    if constexpr (PF) {
                        if (i > 0) { blq64_copy<E>(sc, sn); blq64_copy<E>(yc, yn); }
                    }
                }
#pragma unroll
                for (int k = 0; k < E; ++k) d[k] = d[k] * Hdiag;
                if (PF && count > 0) blq64_load_pair<E>(Sb + (size_t)head * n, Yb + (size_t)head * n, n, sc, yc);
                for (int i = 0; i < count; ++i) {
                    const int sl = head + i >= H ? head + i - H : head + i;
                    double sn[EP], yn[EP];
                    if constexpr (PF) {
                        if (i + 1 < count) {
                            const int sl2 = sl + 1 == H ? 0 : sl + 1;
                            blq64_load_pair<E>(Sb + (size_t)sl2 * n, Yb + (size_t)sl2 * n, n, sn, yn);
                        }
                    } else {
                        blq64_load_pair<E>(Sb + (size_t)sl * n, Yb + (size_t)sl * n, n, sc, yc);
                    }
                    const double be = blq64_dot<E>(yc, d) * Ro[sl];
                    const double c = Al[i] - be;
#pragma unroll
                    for (int k = 0; k < E; ++k) d[k] = fma(c, sc[k], d[k]);
                    if constexpr (PF) {
                        if (i + 1 < count) { blq64_copy<E>(sc, sn); blq64_copy<E>(yc, yn); }
                    }
                }
            }
            blq64_copy<E>(pg, g);
            const double prev_loss = loss;
            // ---- initial step: min(1, 1 / |g|_1) * lr, then lr
            if (n_iter == 1) {
                double s1 = 0.0;
#pragma unroll
                for (int k = 0; k < E; ++k) s1 += fabs(g[k]);
                s1 = blq64_sum64(s1);
                t = t_mul(t_min(tfl(1.0), tten(1.0 / s1)), tfl(qa.lr));
            } else {
                t = tfl(qa.lr);
            }
            const double gtd = blq64_dot<E>(g, d);
            if (gtd > -tolc) { reason = NOCF_LB_GTD; break; }

            // ---- _strong_wolfe(obj_func, x, t, d, loss, g, gtd, c1 = 1e-4, c2 = 0.9, tolerance_change = 1e-9, max_ls)
            const int max_ls = qa.max_eval - evals;
            const double f = loss;
            const double c2gtd = -0.9 * gtd;                   // -c2 * gtd
            const double d_norm = blq64_absmax<E>(d);
            double f_new = blq64_feval<E>(Ld, ly, qa, x, d, t.v, gn);
            int ls_evals = 1;
            double gtd_new = blq64_dot<E>(gn, d);
            TNum t_prev = tfl(0.0);
            double f_prev = f;
            double gtd_prev = gtd;
            blq64_copy<E>(bg0, g);                             // g_prev lives in bracket slot 0 until a bracket forms
            TNum br0 = tfl(0.0), br1 = tfl(0.0);
            double bf0 = 0.0, bf1 = 0.0;
            double bt0 = 0.0, bt1 = 0.0;
            int blen = 2;
            bool done = false;
            int ls_iter = 0;
            // Armijo fails: f_new > f + c1 t gtd
            auto armijo_fails = [&](double fn, TNum tt) {
#pragma clang fp contract(off)
                return f + (1e-4 * tt.v) * gtd < fn;
            };
            while (ls_iter < max_ls) {
                if (armijo_fails(f_new, t) || (ls_iter > 1 && f_new >= f_prev)) {
                    br0 = t_prev; br1 = t; bf0 = f_prev; bf1 = f_new; bt0 = gtd_prev; bt1 = gtd_new;
                    blq64_copy<E>(bg1, gn);
                    break;
                }
                if (fabs(gtd_new) <= c2gtd) {
                    br0 = t; bf0 = f_new; blen = 1; done = true;
                    blq64_copy<E>(bg0, gn);
                    break;
                }
                if (gtd_new >= 0.0) {
                    br0 = t_prev; br1 = t; bf0 = f_prev; bf1 = f_new; bt0 = gtd_prev; bt1 = gtd_new;
                    blq64_copy<E>(bg1, gn);
                    break;
                }
                const TNum min_step = t_add(t, t_mul(tfl(0.01), t_sub(t, t_prev)));
                const TNum max_step = t_mul(t, tfl(10.0));
                const TNum tmp = t;
                t = blq64_cubic(t_prev, f_prev, gtd_prev, t, f_new, gtd_new, true, min_step, max_step);
                t_prev = tmp;
                f_prev = f_new;
                blq64_copy<E>(bg0, gn);
                gtd_prev = gtd_new;
                f_new = blq64_feval<E>(Ld, ly, qa, x, d, t.v, gn);
                ++ls_evals;
                gtd_new = blq64_dot<E>(gn, d);
                ++ls_iter;
            }
            if (ls_iter == max_ls) {
                br0 = tfl(0.0); br1 = t; bf0 = f; bf1 = f_new; blen = 2;
                blq64_copy<E>(bg0, pg);
                blq64_copy<E>(bg1, gn);
            }
            bool insuf = false;
            int low = bf0 <= (blen == 1 ? bf0 : bf1) ? 0 : 1;
            while (!done && ls_iter < max_ls) {
                if (fabs(br1.v - br0.v) * d_norm < 1e-9) break;
                t = blq64_cubic(br0, bf0, bt0, br1, bf1, bt1, false, tfl(0.0), tfl(0.0));
                const TNum bmax = t_max(br0, br1), bmin = t_min(br0, br1);
                const TNum eps = t_mul(tfl(0.1), t_sub(bmax, bmin));
                if (fmin(bmax.v - t.v, t.v - bmin.v) < eps.v) {
                    if (insuf || t.v >= bmax.v || t.v <= bmin.v) {
                        if (fabs(t.v - bmax.v) < fabs(t.v - bmin.v)) t = t_sub(bmax, eps);
                        else t = t_add(bmin, eps);
                        insuf = false;
                    } else {
                        insuf = true;
                    }
                } else {
                    insuf = false;
                }
                f_new = blq64_feval<E>(Ld, ly, qa, x, d, t.v, gn);
                ++ls_evals;
                gtd_new = blq64_dot<E>(gn, d);
                ++ls_iter;
                const double flow = low == 0 ? bf0 : bf1;
                if (armijo_fails(f_new, t) || f_new >= flow) {
                    if (low == 0) { br1 = t; bf1 = f_new; bt1 = gtd_new; blq64_copy<E>(bg1, gn); }
                    else { br0 = t; bf0 = f_new; bt0 = gtd_new; blq64_copy<E>(bg0, gn); }
                    low = bf0 <= bf1 ? 0 : 1;
                } else {
                    if (fabs(gtd_new) <= c2gtd) {
                        done = true;
                    } else {
                        const TNum bh = low == 0 ? br1 : br0, bl = low == 0 ? br0 : br1;
                        if (gtd_new * (bh.v - bl.v) >= 0.0) {   // old high becomes new low
                            if (low == 0) { br1 = br0; bf1 = bf0; bt1 = bt0; blq64_copy<E>(bg1, bg0); }
                            else { br0 = br1; bf0 = bf1; bt0 = bt1; blq64_copy<E>(bg0, bg1); }
                        }
                    }
                    if (low == 0) { br0 = t; bf0 = f_new; bt0 = gtd_new; blq64_copy<E>(bg0, gn); }
                    else { br1 = t; bf1 = f_new; bt1 = gtd_new; blq64_copy<E>(bg1, gn); }
                }
            }
            if (low == 0) { t = br0; loss = bf0; blq64_copy<E>(g, bg0); }
            else { t = br1; loss = bf1; blq64_copy<E>(g, bg1); }
            // ---- accept: x += t d
#pragma unroll
            for (int k = 0; k < E; ++k) x[k] = fma(t.v, d[k], x[k]);
            const bool opt_cond = blq64_absmax<E>(g) <= tolg;
            evals += ls_evals;
            if (n_iter == qa.max_iter) { reason = NOCF_LB_MAX_ITER; break; }
            if (evals >= qa.max_eval) { reason = NOCF_LB_MAX_EVAL; break; }
            if (opt_cond) { reason = NOCF_LB_GRAD; break; }
            {
                double dt[E];
#pragma unroll
                for (int k = 0; k < E; ++k) dt[k] = d[k] * t.v;
                if (blq64_absmax<E>(dt) <= tolc) { reason = NOCF_LB_STEP; break; }
            }
            if (fabs(loss - prev_loss) < tolc) { reason = NOCF_LB_LOSS; break; }
        }
    }
#pragma unroll
    for (int k = 0; k < E; ++k) {
        const int e = lane + NOCF_BLQ_WAVE * k;
        if (e < n) qa.U[b * n + e] = x[k];
    }
    if (lane == 0) {
        qa.loss[b] = loss;
        qa.n_iter[b] = n_iter;
        qa.n_evals[b] = evals;
        qa.reason[b] = reason;
    }
}
