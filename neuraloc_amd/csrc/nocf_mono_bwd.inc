// nocf_mono_bwd.inc -- the adjoint of the rollout for MEDIUM two-layer networks (nTh = 2, m <= 128, d + 1 <= 16: singlequad) on the
// one-CU weight-stationary layout of nocf_mono.inc: what trainOC.py:172-174 obtains with Jc.backward() through the unrolled graph.
//
// One workgroup (4 waves, 16 samples) keeps the whole network in its registers and LDS, like the forward kernel, and walks the RK
// evaluations of its samples latest first.  Per evaluation:
//   forward sweep   P1..P4 of nocf_mono.inc at the recorded stage input (RollArgs::sAll of the forward launch): u0, tanh(o), tanh(q), a,
//                   grad Phi -- 136 MFMAs per wave instead of a 2 KB-per-sample activation record;
//   physics / RK    the cotangent of the right-hand side from the RK adjoint recurrences, the HJ sign masks and the physics
//                   (the device functions of nocf_bwd.inc on the 16-sample view: quad_adjoint / physics_xgrad);
//   VJP of grad Phi four products on the SAME resident images (nocf_bwd.inc's header states the recurrences):
//                   ybar = K0 gbar, vbar = K1 abar0, ubar0 = K1' qbar, sbar = K0' obar + A'(A gbar);
//   weight gradients ACCUMULATED IN THE KERNEL: every operand of an outer product is written once more in row layout
//                   [sample][feature] (stride 132: the float4 writes of a fragment and the transposed b32 reads are both conflict-free
//                   with sample 4 (lane/16) + e on the MFMA's k axis), and v_mfma_f32_16x16x4_f32 adds
//                       dK1 += (hN v) abar0' + qbar u0'        (wave w: row tiles w, w+4 x all column tiles = 64 accumulator registers)
//                       dK0 += y gbar' + obar s' ,   dM += gbar s'   (d(A'A), one tile)
//                   with the samples on k; db0 / db1 / dw ride in the epilogues' registers, dc in 16 threads.
// At the end every workgroup writes ONE partial gradient vector (layout of nocf_small_grad_floats: K0, b0, K1, b1, w, c.weight, c.bias,
// dM); the caller adds the partials in a fixed order.  No row stream, no library GEMM.
// Tail rows (row >= n) replicate a valid sample with inv_n = 0: every cotangent of such a sample is exactly 0.
//
// STATES (nocf_rollout_bwd_states_f32): the state-only instantiation.  The lambda recursion is the same statements; the row-layout copies of
// the outer products' operands, the outer-product MFMAs, every gradient accumulator and the partial-vector write are compiled out, and LAM
// goes to BwdArgs::lamW[k] when the last stage of step k begins (dJ/dW[k] of a disturbed rollout; lamW[nt-1] is the terminal cotangent).
// STATES is a mode: 0 the full adjoint, 1 the state-only one (`false` / `true` select these two as before), 2 the JOINT one
// (nocf_rollout_bwd_mid_w_f32): every statement of mode 0 plus the lamW[k] store of mode 1 at the same place, both under `if constexpr`.

// accumulator in AccVGPRs (the 64 registers of a wave's dK1 tiles sit beside the resident K1 images in the upper half of the register file)
__device__ __forceinline__ void mfma16_aa(f32x4& acc, float a, float b) {
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+a"(acc) : "v"(a), "v"(b));
}
#define SL_FENCE1A(a) asm volatile("s_nop 7\n\ts_nop 4" : "+a"(a))

// The LDS layout is a compile-time constant (row strides of the 16-sample view at their d + 1 <= 16 values, room for 8 agents): every
// address is one lane-dependent register plus an immediate.  With the offsets in scalar registers (as the forward kernel has them) the
// compiler hoisted ~140 base + lane sums out of the evaluation loop and spilled them (584 B of scratch, a reload in front of every use).
struct MonoBwdLds {
    int lSF, lUF, lVF, lK4, lAT, lVO, lCW, lZP, lGP, lPHIP, lGF, lRV, lRAB, lRQB, lRU0, lRY, lROB;
    int lSB, lG, lZQ, lDZ, lRED, lSC, lPHI, lTRIG, lPT, lPW, lGB, lSBAR, lZQB, lLAM, lXS, lXP, lXD, lSCB, lINV, lPHIB, lACC, total;
};
#define MONO_BWD_LDS_S 68
#define MONO_BWD_GLD 64
#define MONO_BWD_ZLD(KBD) ((KBD) == 1 ? 20 : 36)          // row stride of the (d + 4)-wide state rows: d + 1 <= 16 / <= 32
#define MONO_BWD_NAG(KBD) ((KBD) == 1 ? 8 : 16)           // agents (point agents: d / 2 or d / 3; quadcopters: d / 12)
constexpr MonoBwdLds mono_bwd_lds(int KBM, int KBD) {
    MonoBwdLds L{};
    int l = 0;
    const int T = 16;
    const int ZLDc = MONO_BWD_ZLD(KBD), NAGc = MONO_BWD_NAG(KBD);
    L.lSF = l; l += KBD * 256; L.lUF = l; l += KBM * 256; L.lVF = l; l += KBM * 256; L.lK4 = l; l += KBD * KBM * 256; L.lAT = l; l += KBD * 256;
    L.lVO = l; l += 3 * KBM * 16; L.lCW = l; l += KBD * 16; L.lZP = l; l += 1024; L.lGP = l; l += KBD * 1024; L.lPHIP = l; l += 64; L.lGF = l; l += KBD * 256;
    L.lRV = l; l += T * 132; L.lRAB = l; l += T * 132; L.lRQB = l; l += T * 132; L.lRU0 = l; l += T * 132; L.lRY = l; l += T * 132; L.lROB = l; l += T * 132;
    L.lSB = l; l += T * MONO_BWD_LDS_S; L.lG = l; l += T * MONO_BWD_GLD; L.lZQ = l; l += T * ZQLD; L.lDZ = l; l += T * ZLDc;
    L.lRED = l; l += 64; L.lSC = l; l += T * NAGc + 8; L.lPHI = l; l += T; L.lTRIG = l; l += T * KBD * 6 /* quadcopters: d / 12 crafts */; L.lPT = l; l += 4; L.lPW = l; l += 4;
    L.lGB = l; l += T * MONO_BWD_LDS_S; L.lSBAR = l; l += T * MONO_BWD_GLD; L.lZQB = l; l += T * ZQLD;
    L.lLAM = l; l += T * ZLDc; L.lXS = l; l += T * ZLDc; L.lXP = l; l += T * ZLDc; L.lXD = l; l += T * ZLDc;
    L.lSCB = l; l += T * 4 + 8;
    L.lINV = l; l += T; L.lPHIB = l; l += T;
    L.lACC = l; l += 3 * KBM * 256;               // db0 / db1 / dw: every lane's own sums (4 features of one sample), in LDS instead of 24 registers
    L.total = l;
    return L;
}

template <int KBD>
__device__ __forceinline__ void mono_rows_to_frag(int lF, int lRows, int ld, int D1, int tid) {
    float4* L4 = reinterpret_cast<float4*>(lds);
    for (int f = tid; f < KBD * 64; f += 256) {
        const int l = f & 63, kb = f >> 6;
        const float* srow = lds + lRows + (l & 15) * ld + 16 * kb + 4 * (l >> 4);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (16 * kb + 4 * (l >> 4) + e < D1) ? srow[e] : 0.f;
        L4[(lF >> 2) + f] = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// partial K0' x + A' z of this wave (hidden k-blocks wave, wave+4, ...; wave 0 adds the low-rank term) -> GP[(dt*4 + wave)*64 + lane]
template <int MT, int KBM, int KBD>
__device__ __forceinline__ void mono_close(const MonoPlan& mp, int lFrag, int wave, int lane) {
    float4* L4 = reinterpret_cast<float4*>(lds);
    float4 zf = make_float4(0.f, 0.f, 0.f, 0.f);
    if (wave == 0) {
        const float4 z0 = L4[(mp.lZP >> 2) + lane], z1 = L4[(mp.lZP >> 2) + 64 + lane];
        const float4 z2 = L4[(mp.lZP >> 2) + 128 + lane], z3 = L4[(mp.lZP >> 2) + 192 + lane];
        zf.x = ((z0.x + z1.x) + z2.x) + z3.x; zf.y = ((z0.y + z1.y) + z2.y) + z3.y;
        zf.z = ((z0.z + z1.z) + z2.z) + z3.z; zf.w = ((z0.w + z1.w) + z2.w) + z3.w;
    }
#pragma unroll
    for (int dt = 0; dt < KBD; ++dt) {
        f32x4 a0, a1;
        float4 wf[MT], bf[MT];
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {
            const int kb = wave + 4 * mi;
            wf[mi] = L4[(mp.lK4 >> 2) + (dt * KBM + (kb < KBM ? kb : 0)) * 64 + lane];
            bf[mi] = L4[(lFrag >> 2) + (kb < KBM ? kb : 0) * 64 + lane];
            if (kb >= KBM) wf[mi] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float4 af = L4[(mp.lAT >> 2) + dt * 64 + lane];
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {                          // two chains, started from the inline constant 0
            if (mi == 0) { mfma16_vv0(a0, wf[mi].x, bf[mi].x); mfma16_vv0(a1, wf[mi].y, bf[mi].y); }
            else { mfma16_vv(a0, wf[mi].x, bf[mi].x); mfma16_vv(a1, wf[mi].y, bf[mi].y); }
            mfma16_vv(a0, wf[mi].z, bf[mi].z); mfma16_vv(a1, wf[mi].w, bf[mi].w);
        }
        if (wave == 0) { mfma16_vv(a0, af.x, zf.x); mfma16_vv(a1, af.y, zf.y); mfma16_vv(a0, af.z, zf.z); mfma16_vv(a1, af.w, zf.w); }
        asm volatile("s_nop 7\n\ts_nop 4" : "+v"(a0), "+v"(a1));
        const f32x4 ps = a0 + a1;
        L4[(mp.lGP >> 2) + (dt * 4 + wave) * 64 + lane] = make_float4(ps[0], ps[1], ps[2], ps[3]);
    }
}

// rows[t][0 .. 16 KBD) = the fixed-order sum of the four waves' partials (+ c when addc)
template <int KBD>
__device__ __forceinline__ void mono_close_rows(const MonoPlan& mp, int lRows, int ld, bool addc, int tid) {
    const float4* L4 = reinterpret_cast<const float4*>(lds);
    for (int f = tid; f < KBD * 64; f += 256) {
        const int l = f & 63, dt = f >> 6;
        const float4 p0 = L4[(mp.lGP >> 2) + (dt * 4 + 0) * 64 + l], p1 = L4[(mp.lGP >> 2) + (dt * 4 + 1) * 64 + l];
        const float4 p2 = L4[(mp.lGP >> 2) + (dt * 4 + 2) * 64 + l], p3 = L4[(mp.lGP >> 2) + (dt * 4 + 3) * 64 + l];
        float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if (addc) c4 = L4[(mp.lCW >> 2) + dt * 4 + (l >> 4)];
        float4 gsum;
        gsum.x = (((p0.x + p1.x) + p2.x) + p3.x) + c4.x; gsum.y = (((p0.y + p1.y) + p2.y) + p3.y) + c4.y;
        gsum.z = (((p0.z + p1.z) + p2.z) + p3.z) + c4.z; gsum.w = (((p0.w + p1.w) + p2.w) + p3.w) + c4.w;
        *reinterpret_cast<float4*>(lds + lRows + (l & 15) * ld + 16 * dt + 4 * (l >> 4)) = gsum;
    }
}

// z-type partial A x of the fragment at lFrag (waves < KBD contract one input k-block each) -> ZP[wave*64 + lane]
template <int KBD>
__device__ __forceinline__ void mono_lowrank(const MonoPlan& mp, const f32x4& AZ, int lFrag, int wave, int lane) {
    float4* L4 = reinterpret_cast<float4*>(lds);
    f32x4 zacc = {0.f, 0.f, 0.f, 0.f};
    if (wave < KBD) {
        const float4 bz = L4[(lFrag >> 2) + wave * 64 + lane];
        f32x4 z0, z1;
        mfma16_vv0(z0, AZ[0], bz.x); mfma16_vv0(z1, AZ[1], bz.y); mfma16_vv(z0, AZ[2], bz.z); mfma16_vv(z1, AZ[3], bz.w);
        asm volatile("s_nop 7\n\ts_nop 4" : "+v"(z0), "+v"(z1));
        zacc = z0 + z1;
    }
    L4[(mp.lZP >> 2) + wave * 64 + lane] = make_float4(zacc[0], zacc[1], zacc[2], zacc[3]);
}

// ENS (STATES = 0; nocf_rollout_bwd_mid_ensemble_f32): the adjoint of an ensemble rollout (nocf_mono.inc, MonoEnsArgs).  en.tiles =
// nocf_mid_grad_rows workgroups per member; workgroup j of member e walks the member's tiles j, j + en.tiles, ... (the single-network tile
// order) and writes partial vector gpart[e][j] = row blockIdx.x.  Every ENS test is a compile-time choice at its place of use.
//
// RW (STATES = 0, no ensemble; nocf_rollout_bwd_mid_rw_f32): the per-sample table lINV, which every cotangent seed already reads, is filled
// with BwdArgs::wrow[row] instead of the one value inv_n (0 for the tail rows, as before): one load per sample and tile, nothing else differs.
//
// ENS && RW (STATES = 0; nocf_rollout_bwd_mid_ensemble_rw_f32): BwdArgs::wrow is [E, en.n]; member e's workgroups move it to their member's
// row where they move zT and lam0, and fill lINV from it as the RW instantiation does.  ba.inv_n is not read.
//
// ENS && STATES == 2 (nocf_rollout_bwd_mid_ensemble_w_f32) and ENS && STATES == 1 (nocf_rollout_bwd_mid_ensemble_states_f32), DESIGN 3.17: the
// ensemble adjoint with the lamW[k] store of the joint / state-only modes.  BwdArgs::lamW is [E, nt, en.n, d] member-major; member e's
// workgroups move it to their member's slice where they move zT and lam0 (workgroup-uniform), and ba.n / row0 are the member's, so the store is
// the single-network statement on that slice: tail rows of a member's last tile write nothing.  STATES == 1 writes no partial vector (gpart is
// not read).  RW with STATES != 0 stays refused.
template <int KBM, int KBD, int STATES = 0, bool ENS = false, bool RW = false>
__global__ void __launch_bounds__(256) rollout_mono_bwd_kernel(const MonoPlan* __restrict__ mpp, DevProb pb, const float* __restrict__ ws, BwdArgs ba,
                                                               MonoEnsArgs en) {
    static_assert(KBD == 1 || KBD == 2, "d + 1 <= 32: the (sample, entry) threads take KBD entries each; dM is KBD x KBD tiles on the four waves");
    static_assert(!RW || STATES == 0, "the weighted variants are parameter-and-lam0 adjoints");
    constexpr int MT = (KBM + 3) / 4;
    constexpr int T = 16;
    constexpr MonoBwdLds LL = mono_bwd_lds(KBM, KBD);
    unsigned etile = 0;                  // ENS: this workgroup's index inside its member
    if constexpr (ENS) {
        const unsigned e = blockIdx.x / en.tiles;
        etile = blockIdx.x - e * en.tiles;
        ws += e * en.wss;
        mpp = reinterpret_cast<const MonoPlan*>(reinterpret_cast<const float*>(mpp) + e * en.wss);
        const float* at = en.alph + e * 6;
        ba.a0 = at[0]; pb.alphQ = (double)at[1]; pb.alphW = (double)at[2]; ba.a3 = at[3]; ba.a4 = at[4]; ba.a5 = at[5];
        ba.sAll += e * en.sas;
        if (ba.act) ba.act += e * en.acts;
    }
    MonoPlan mp = *mpp;
    mp.lSF = LL.lSF; mp.lUF = LL.lUF; mp.lVF = LL.lVF; mp.lK4 = LL.lK4; mp.lAT = LL.lAT; mp.lVO = LL.lVO; mp.lCW = LL.lCW; mp.lZP = LL.lZP;
    mp.lGP = LL.lGP; mp.lPHIP = LL.lPHIP; mp.lGF = LL.lGF; mp.lRV = LL.lRV; mp.lRAB = LL.lRAB; mp.lRQB = LL.lRQB; mp.lRU0 = LL.lRU0;
    mp.lRY = LL.lRY; mp.lROB = LL.lROB;
    {
        DevPlan& q = mp.pp;
        q.T = 16; q.nwaves = 4; q.LDs = MONO_BWD_LDS_S; q.GLD = MONO_BWD_GLD; q.ZLD = MONO_BWD_ZLD(KBD);
        q.lSB = LL.lSB; q.lG = LL.lG; q.lZQ = LL.lZQ; q.lDZ = LL.lDZ; q.lRED = LL.lRED; q.lSC = LL.lSC; q.lPHI = LL.lPHI; q.lTRIG = LL.lTRIG;
        q.lPT = LL.lPT; q.lPW = LL.lPW; q.lGB = LL.lGB; q.lSBAR = LL.lSBAR; q.lZQB = LL.lZQB; q.lLAM = LL.lLAM; q.lXS = LL.lXS; q.lXP = LL.lXP;
        q.lXD = LL.lXD; q.lSCB = LL.lSCB; q.ldsFloats = LL.total;
        NOCF_PIN(q.d); NOCF_PIN(q.D1); NOCF_PIN(q.m); NOCF_PIN(q.r); NOCF_PIN(q.hN); NOCF_PIN(q.cb); NOCF_PIN(q.nAg);
    }
    const DevPlan& pl = mp.pp;
    Ctx c;
    ctx_init(c, ws, (unsigned)(pl.oPlan * 4));
    c.cb = pl.cb;
    const int d = pl.d, D1 = pl.D1, r = pl.r, ZLD = pl.ZLD, GLD = pl.GLD, LDs = pl.LDs, m = pl.m;
    const int wave = c.wave, lane = c.lane, tid = c.tid;
    const int slot = lane >> 4, l16 = lane & 15;
    constexpr int LDR = 132;
    const float hN = pl.hN;
    const float4* ws4 = reinterpret_cast<const float4*>(ws);
    float4* L4 = reinterpret_cast<float4*>(lds);
    if constexpr (ENS) {                 // the member's blocks of z_final [E, n, d+4] and lam0 [E, n, d]
        const long eo = (long)(blockIdx.x / en.tiles) * en.n;
        ba.zT += eo * (d + 4);
        if (ba.lam0) ba.lam0 += eo * d;
        if constexpr (RW) ba.wrow += eo;
        if constexpr (STATES != 0) { if (ba.lamW) ba.lamW += eo * ba.nt * d; }      // lamW [E, nt, n, d]: the member's slice
    }

    // ---- resident weights (as the forward kernel's)
    f32x4 W2[MT][KBM], W3[MT][KBM], K1[MT][KBD], AZ;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
        const int mt = wave + 4 * mi;
        const bool on = mt < KBM;
#pragma unroll
        for (int kb = 0; kb < KBM; ++kb) {
            const float4 a = on ? ws4[mp.oW2 + (long)(mt * KBM + kb) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 b = on ? ws4[mp.oW3 + (long)(mt * KBM + kb) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
            W2[mi][kb] = (f32x4){a.x, a.y, a.z, a.w};
            W3[mi][kb] = (f32x4){b.x, b.y, b.z, b.w};
        }
#pragma unroll
        for (int kb = 0; kb < KBD; ++kb) {
            const float4 a = on ? ws4[mp.oK1 + (long)(mt * KBD + kb) * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
            K1[mi][kb] = (f32x4){a.x, a.y, a.z, a.w};
        }
    }
    {
        const float4 a = (wave < KBD) ? ws4[mp.oAZ + (long)wave * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
        AZ = (f32x4){a.x, a.y, a.z, a.w};
    }
    // the answers are taken here: a first use inside the evaluation loop would wait for ALL outstanding requests (vmcnt(0)) every time round
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
        for (int kb = 0; kb < KBD; ++kb) asm volatile("" : "+v"(K1[mi][kb]));
    asm volatile("" : "+v"(AZ));
    for (int i = tid; i < pl.ldsFloats; i += 256) lds[i] = 0.f;
    __syncthreads();
    for (int i = tid; i < KBD * KBM * 64; i += 256) L4[(mp.lK4 >> 2) + i] = ws4[mp.oK4 + i];
    for (int i = tid; i < KBD * 64; i += 256) L4[(mp.lAT >> 2) + i] = ws4[mp.oAT + i];
    for (int i = tid; i < KBM * 16; i += 256) {
        lds[mp.lVO + i] = (i < m) ? c.ws[pl.ob0 + i] : 0.f;
        lds[mp.lVO + KBM * 16 + i] = (i < m) ? c.ws[pl.ob + i] : 0.f;
        lds[mp.lVO + 2 * KBM * 16 + i] = (i < m) ? c.ws[pl.ow + i] : 0.f;
    }
    for (int i = tid; i < KBD * 16; i += 256) lds[mp.lCW + i] = (i < D1) ? c.ws[pl.ocw + i] : 0.f;
    __syncthreads();
    float wv[MT][4];                     // (b0 / b1 are read from LDS where the forward sweep needs them: terminal evaluation, no record)
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
        const int mt = wave + 4 * mi;
        const int o = (mt < KBM ? mt : 0) * 4 + slot;
        const float4 x2 = L4[((mp.lVO + 2 * KBM * 16) >> 2) + o];
        wv[mi][0] = x2.x; wv[mi][1] = x2.y; wv[mi][2] = x2.z; wv[mi][3] = x2.w;
        if (mt >= KBM) {
#pragma unroll
            for (int e = 0; e < 4; ++e) wv[mi][e] = 0.f;
        }
    }

    float* SB = lds + pl.lSB;
    float* GB = lds + pl.lGB;
    float* LAM = lds + pl.lLAM;
    float* XS = lds + pl.lXS;
    float* XP = lds + pl.lXP;
    float* XD = lds + pl.lXD;
    const float* G = lds + pl.lG;
    const float* SBAR = lds + pl.lSBAR;
    float* SC = lds + pl.lSCB;           // per sample: [t*4+0] = coef, +1 = e kh, +2 = kL - e kh, +3 = e_f
    const bool quad = (pb.kind == NOCF_PROB_QUADCOPTER);
    const bool quad1 = KBD == 1 && quad && pb.nAgents == 1 && d == 12;     // singlequad: wave-local physics below

    // ---- gradient accumulators
    f32x4 dK1a[MT][KBM], dK0a[MT][KBD], dMa = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
#pragma unroll
        for (int ct = 0; ct < KBD; ++ct) dK0a[mi][ct] = dMa;
#pragma unroll
        for (int jt = 0; jt < KBM; ++jt) dK1a[mi][jt] = dMa;
    }
    float dca[KBD], dcba = 0.f;          // dc: entries tid % 16 (+ 16) of sample tid / 16's share; c.bias (tid < 16: sample tid's share)
#pragma unroll
    for (int q = 0; q < KBD; ++q) dca[q] = 0.f;

    // ---- the 16-sample tiles of this workgroup (tile, tile + gridDim.x, ...: the launch caps the grid, so the partial gradient vectors stay
    // a bounded buffer for any batch size), every tile's evaluations latest first; the gradient sums run on across the tiles
    const long ntiles = (ba.n + T - 1) / T;
    for (long tile = ENS ? etile : blockIdx.x; tile < ntiles; tile += ENS ? en.tiles : gridDim.x) {
        const long row0 = tile * T;
        const long nvalid = (ba.n - row0 < T) ? (ba.n - row0) : T;
        __syncthreads();                                   // (the previous tile's last reads of the tables and rows)
        // per-sample tables: 1/N (0 for the tail rows that replicate a valid sample) and the cotangent of Phi(z(T), T) (terminal evaluation only)
        if constexpr (RW) { if (tid < T) { lds[LL.lINV + tid] = (tid < nvalid) ? ba.wrow[row0 + tid] : 0.f; lds[LL.lPHIB + tid] = 0.f; } }
        else
        if (tid < T) { lds[LL.lINV + tid] = (tid < nvalid) ? ba.inv_n : 0.f; lds[LL.lPHIB + tid] = 0.f; }
        __syncthreads();
        const float c16 = (float)(1.0 / 6.0), c26 = (float)(2.0 / 6.0);
        const long total = (long)ba.nt * ba.nstage;
        float g_next[KBD];                   // ... and of grad Phi from the activation record
        float4 r_u0[MT], r_t0[MT], r_t1[MT], r_a[MT];       // the record's fragments of the next evaluation (lane: sample lane % 16, 4 features)
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) { r_u0[mi] = make_float4(0.f, 0.f, 0.f, 0.f); r_t0[mi] = r_u0[mi]; r_t1[mi] = r_u0[mi]; r_a[mi] = r_u0[mi]; }
        float hs_next = 0.f;                 // step size of the next evaluation (0 at the terminal one)
        float s_next[KBD];                   // entries tid % 16 (+ 16) of sample tid / 16 of the next evaluation's stage input; first: [z(T), t1]
#pragma unroll
        for (int q = 0; q < KBD; ++q) {
            const int t = tid >> 4, i = (tid & 15) + 16 * q;
            long row = row0 + t; if (row >= ba.n) row = ba.n - 1;
            s_next[q] = (i < d) ? ba.zT[row * (d + 4) + i] : ba.t1;
            g_next[q] = 0.f;
        }
        int kk = ba.nt, stt = 0;
        for (long ev = total; ev >= 0; --ev) {
            const bool fin = (ev == total);
            // the lane / thread numbers behind an empty asm: everything derived from them is formed where it is used instead of being hoisted
            // out of this loop into registers the allocator does not have (the first build spilled ~140 hoisted address and mask values)
            int lane_o = c.lane, tid_o = c.tid;
            asm volatile("" : "+v"(lane_o), "+v"(tid_o));
            Ctx cc = c;
            cc.lane = lane_o; cc.tid = tid_o;
            const int lane = lane_o, tid = tid_o, slot = lane_o >> 4, l16 = lane_o & 15;
#ifdef NOCF_STAMPS
            cc.tl = (blockIdx.x == 7 && ev == total - 10 && g_tl_dev) ? g_tl_dev : nullptr;      // tools/timeline_bwd.py singlequad
#endif
            TL(cc, 0);
            const int k = kk, st = stt;                          // (counted down below: a 64-bit division here cost ~1 k cycles per evaluation)
            float hs = hs_next;                                   // (requested one evaluation ahead with the stage input: a load whose answer is consumed
                                                                  // further down would make every later use wait for ALL outstanding requests)
            asm volatile("" : "+v"(hs));                           // the answer is taken HERE, in front of the next requests
            float wst = 1.f, cpl = 0.f;
            if (ba.nstage != 1) { wst = (st == 0 || st == 3) ? c16 : c26; cpl = (st == 3) ? 0.f : (st == 2 ? 1.f : 0.5f); }
            // ---- the stage input of this evaluation: requested one evaluation ahead (thread (t, i) = (tid / 16, tid % 16) holds entry i of sample
            // t), written here to the state rows AND to the fragment of P1; with an activation record also u0, tanh(o), tanh(q), a and grad Phi
            const bool rec = !fin && ba.act != nullptr;
            f32x4 acc[MT], th0[MT], th1[MT], av[MT], u1k[MT];
            {
                const int t = tid >> 4;
#pragma unroll
                for (int q = 0; q < KBD; ++q) {
                    const int i = (tid & 15) + 16 * q;
                    if (i < D1) SB[t * LDs + i] = s_next[q];
                    lds[mp.lSF + q * 256 + (((tid & 15) >> 2) * 16 + t) * 4 + (tid & 3)] = (i < D1) ? s_next[q] : 0.f;
                    if constexpr (STATES != 0) {
                        if (!fin && st == ba.nstage - 1 && i < d && ba.lamW && t < nvalid) ba.lamW[((long)k * ba.n + row0 + t) * d + i] = LAM[t * ZLD + i];
                    }
                    if (!fin && st == ba.nstage - 1 && i < d) { XS[t * ZLD + i] = 0.f; XP[t * ZLD + i] = 0.f; }
                    if (rec && i < D1) lds[pl.lG + t * GLD + i] = g_next[q];
                }
                if (rec) {
#pragma unroll
                    for (int mi = 0; mi < MT; ++mi) {
                        const int mt = wave + 4 * mi;
                        th0[mi] = (f32x4){r_t0[mi].x, r_t0[mi].y, r_t0[mi].z, r_t0[mi].w};
                        th1[mi] = (f32x4){r_t1[mi].x, r_t1[mi].y, r_t1[mi].z, r_t1[mi].w};
                        av[mi] = (f32x4){r_a[mi].x, r_a[mi].y, r_a[mi].z, r_a[mi].w};
                        u1k[mi] = (f32x4){0.f, 0.f, 0.f, 0.f};
                        if (STATES != 1 && mt < KBM) {
                            const int ro = l16 * LDR + 16 * mt + 4 * slot;
                            *reinterpret_cast<float4*>(lds + mp.lRU0 + ro) = r_u0[mi];
                            *reinterpret_cast<float4*>(lds + mp.lRV + ro) = make_float4(hN * th1[mi][0] * wv[mi][0], hN * th1[mi][1] * wv[mi][1],
                                                                                        hN * th1[mi][2] * wv[mi][2], hN * th1[mi][3] * wv[mi][3]);
                            *reinterpret_cast<float4*>(lds + mp.lRY + ro) = make_float4(th0[mi][0] * av[mi][0], th0[mi][1] * av[mi][1],
                                                                                        th0[mi][2] * av[mi][2], th0[mi][3] * av[mi][3]);
                        }
                    }
                }
                if (ev > 0) {
                    // wave-uniform 64-bit bases + 32-bit lane offsets (per-lane 64-bit address arithmetic for ten loads cost ~1.5 k cycles here)
                    const unsigned tc = (unsigned)((t < nvalid) ? t : nvalid - 1), lc = (unsigned)((l16 < nvalid) ? l16 : nvalid - 1);
                    const float* sb_ = ba.sAll + ((ev - 1) * ba.n + row0) * D1;
#pragma unroll
                    for (int q = 0; q < KBD; ++q) { const int i = (tid & 15) + 16 * q; if (i < D1) s_next[q] = sb_[tc * (unsigned)D1 + (unsigned)i]; }
                    hs_next = ba.hs[stt == 0 ? kk - 1 : kk];
                    if (ba.act) {
                        const long sec = ba.actRows * m;
                        const float* gb_ = ba.act + 4 * sec + ((ev - 1) * ba.n + row0) * D1;
#pragma unroll
                        for (int q = 0; q < KBD; ++q) { const int i = (tid & 15) + 16 * q; if (i < D1) g_next[q] = gb_[tc * (unsigned)D1 + (unsigned)i]; }
                        const float* ab_ = ba.act + ((ev - 1) * ba.n + row0) * m;
                        const float* a1_ = ab_ + sec; const float* a2_ = a1_ + sec; const float* a3_ = a2_ + sec;
#pragma unroll
                        for (int mi = 0; mi < MT; ++mi) {
                            const int mt = wave + 4 * mi;
                            if (mt < KBM) {
                                const unsigned off = lc * (unsigned)m + (unsigned)(16 * mt + 4 * slot);
                                r_u0[mi] = *reinterpret_cast<const float4*>(ab_ + off); r_t0[mi] = *reinterpret_cast<const float4*>(a1_ + off);
                                r_t1[mi] = *reinterpret_cast<const float4*>(a2_ + off); r_a[mi] = *reinterpret_cast<const float4*>(a3_ + off);
                            }
                        }
                    }
                }
            }
            __syncthreads();
            TL(cc, 1);

            // ================= forward sweep (nocf_mono.inc P1 .. P4): the terminal evaluation, and every one without a record =================
            if (!rec) {
                mono_gemm<MT, KBD, false>(K1, (mp.lSF >> 2) + lane, acc);
                mono_lowrank<KBD>(mp, AZ, mp.lSF, wave, lane);
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    const int mt = wave + 4 * mi;
                    f32x4 sg, th;
                    const float4 b04 = (mt < KBM) ? L4[(mp.lVO >> 2) + mt * 4 + slot] : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float b0v_[4] = {b04.x, b04.y, b04.z, b04.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) { float s_, t_; act_pair(acc[mi][e] + b0v_[e], s_, t_); sg[e] = s_; th[e] = t_; }
                    th0[mi] = th; u1k[mi] = sg;
                    if (mt < KBM) {
                        const float4 u4 = make_float4(sg[0], sg[1], sg[2], sg[3]);
                        L4[(mp.lUF >> 2) + mt * 64 + lane] = u4;
                        if constexpr (STATES != 1) *reinterpret_cast<float4*>(lds + mp.lRU0 + l16 * LDR + 16 * mt + 4 * slot) = u4;
                    }
                }
                TL(cc, 2);
                __syncthreads();
                TL(cc, 3);
                mono_gemm<MT, KBM, true>(W2, (mp.lUF >> 2) + lane, acc);
                TL(cc, 4);
                float pr = 0.f;
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    const int mt = wave + 4 * mi;
                    float vv[4];
                    const float4 b14 = (mt < KBM) ? L4[((mp.lVO + KBM * 16) >> 2) + mt * 4 + slot] : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float b1v_[4] = {b14.x, b14.y, b14.z, b14.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float q = acc[mi][e] + b1v_[e];
                        th1[mi][e] = tanh_fast(q);
                        vv[e] = th1[mi][e] * wv[mi][e];
                        if (fin) { u1k[mi][e] = u1k[mi][e] + hN * sigma_act(q); pr += wv[mi][e] * u1k[mi][e]; }       // src/Phi.py:91-96
                    }
                    if (mt < KBM) {
                        L4[(mp.lVF >> 2) + mt * 64 + lane] = make_float4(vv[0], vv[1], vv[2], vv[3]);
                        if constexpr (STATES != 1) *reinterpret_cast<float4*>(lds + mp.lRV + l16 * LDR + 16 * mt + 4 * slot) = make_float4(hN * vv[0], hN * vv[1], hN * vv[2], hN * vv[3]);
                    }
                }
                if (fin) {
                    pr += __shfl_xor(pr, 16); pr += __shfl_xor(pr, 32);
                    if (lane < 16) lds[mp.lPHIP + wave * 16 + lane] = pr;
                }
                TL(cc, 5);
                __syncthreads();
                TL(cc, 6);
                {
                    const int s_ = tid >> 4, row = tid & 15;
                    const float* zp = lds + mp.lZP + ((row >> 2) * 16 + s_) * 4 + (row & 3);
                    lds[pl.lZQ + s_ * ZQLD + row] = ((zp[0] + zp[256]) + zp[512]) + zp[768];
                }
                mono_gemm<MT, KBM, true>(W3, (mp.lVF >> 2) + lane, acc);
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    const int mt = wave + 4 * mi;
                    float4 y;
#pragma unroll
                    for (int e = 0; e < 4; ++e) av[mi][e] = wv[mi][e] + hN * acc[mi][e];
                    y.x = th0[mi][0] * av[mi][0]; y.y = th0[mi][1] * av[mi][1]; y.z = th0[mi][2] * av[mi][2]; y.w = th0[mi][3] * av[mi][3];
                    if (mt < KBM) {
                        L4[(mp.lUF >> 2) + mt * 64 + lane] = y;
                        if constexpr (STATES != 1) *reinterpret_cast<float4*>(lds + mp.lRY + l16 * LDR + 16 * mt + 4 * slot) = y;
                    }
                }
                TL(cc, 7);
                __syncthreads();
                TL(cc, 8);
                mono_close<MT, KBM, KBD>(mp, mp.lUF, wave, lane);
                TL(cc, 9);
                __syncthreads();
                mono_close_rows<KBD>(mp, pl.lG, GLD, true, tid);
                if (fin && tid < T) {
                    const int s_ = tid;
                    float ph = ((lds[mp.lPHIP + s_] + lds[mp.lPHIP + 16 + s_]) + lds[mp.lPHIP + 32 + s_]) + lds[mp.lPHIP + 48 + s_];
                    float qd = 0.f;
                    for (int q = 0; q < r; ++q) { const float z = lds[pl.lZQ + s_ * ZQLD + q]; qd += 0.5f * z * z; }
                    float lin = 0.f;
                    for (int i = 0; i < D1; ++i) lin += lds[mp.lCW + i] * SB[s_ * LDs + i];
                    lds[pl.lPHI + s_] = ph + qd + lin + pl.cb;
                }
                __syncthreads();
            }
            TL(cc, 10);

            // ================= cotangent of the right-hand side (nocf_bwd.inc rollout_bwd_body, 16 samples) =================
            if (fin) {
                const int Gsz = 256 / T;
                const int t = tid / Gsz, j0 = tid - t * Gsz;
                float v[1] = {0.f};
                for (int i = j0; i < d; i += Gsz) { const float res = SB[t * LDs + i] - pb.xtarget[i]; v[0] += res * res; }
                group_reduce<1>(cc, pl, v);
                if (tid < T) {
                    const float cG = 0.5f * group_total<1>(cc, pl, tid, 0);
                    const float dd = lds[pl.lPHI + tid] - ba.a0 * cG;
                    const float ef_ = (dd > 0.f) ? 1.f : (dd < 0.f ? -1.f : 0.f);            // e_f = sign(Phi1 - a0 cG)
                    SC[tid * 4 + 3] = ef_;
                    lds[LL.lPHIB + tid] = lds[LL.lINV + tid] * ba.a4 * ef_;                  // cotangent of Phi(z(T), T)
                }
                __syncthreads();
                for (int j = tid; j < T * d; j += 256) {
                    const int t2 = j / d, i = j - t2 * d;
                    const float inv = lds[LL.lINV + t2];
                    const float res = SB[t2 * LDs + i] - pb.xtarget[i];
                    const float gi = G[t2 * GLD + i];
                    const float dg = gi - ba.a0 * res;
                    const float eg = (dg > 0.f) ? 1.f : (dg < 0.f ? -1.f : 0.f);
                    const float ef = SC[t2 * 4 + 3];
                    LAM[t2 * ZLD + i] = inv * (ba.a0 * res + ba.a4 * ef * dg - ba.a5 * ba.a0 * eg);
                    GB[t2 * LDs + i] = inv * ba.a5 * eg;
                    XD[t2 * ZLD + i] = 0.f;
                }
                if (tid < T) GB[tid * LDs + d] = 0.f;
                __syncthreads();
            } else if (quad1) {
                // ---- one quadcopter per sample: cost scalars, HJ sign and the physics cotangents wave-locally, 16 lanes per sample, no barrier
                // (physics_finish + quad_adjoint of nocf_bwd.inc for N = 1, restated like the forward kernel's wave-local physics: every lane
                // forms the scalars, lane j keeps component j of gbar = [d/dp (12) | d/d(dPhi/dt)] and of the direct x term)
                const int s_ = tid >> 4, j = tid & 15;
                float xv[12], pv[13], fb[12];
                {
                    const float4* x4 = reinterpret_cast<const float4*>(SB + s_ * LDs);
                    const float4* p4 = reinterpret_cast<const float4*>(G + s_ * GLD);
                    const float4* l4 = reinterpret_cast<const float4*>(LAM + s_ * ZLD);
                    const float4* q4 = reinterpret_cast<const float4*>(XP + s_ * ZLD);
#pragma unroll
                    for (int q = 0; q < 3; ++q) {
                        const float4 a = x4[q], b = p4[q], l_ = l4[q], xq = q4[q];
                        xv[4 * q] = a.x; xv[4 * q + 1] = a.y; xv[4 * q + 2] = a.z; xv[4 * q + 3] = a.w;
                        pv[4 * q] = b.x; pv[4 * q + 1] = b.y; pv[4 * q + 2] = b.z; pv[4 * q + 3] = b.w;
                        fb[4 * q] = hs * (wst * l_.x + cpl * xq.x); fb[4 * q + 1] = hs * (wst * l_.y + cpl * xq.y);
                        fb[4 * q + 2] = hs * (wst * l_.z + cpl * xq.z); fb[4 * q + 3] = hs * (wst * l_.w + cpl * xq.w);
                    }
                    pv[12] = G[s_ * GLD + 12];
                }
                TL(cc, 27);
                float* TR = lds + pl.lTRIG + s_ * 6;
                if (j < 3) { float sn, cs; mono_sincos(j == 0 ? xv[3] : (j == 1 ? xv[4] : xv[5]), sn, cs); TR[j] = sn; TR[3 + j] = cs; }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
                const float sps = TR[0], sth = TR[1], sph = TR[2], cps = TR[3], cth = TR[4], cph = TR[5];
                TL(cc, 28);
                const float Mq = (float)pb.mass, grav = (float)pb.grav, mh = (float)(-1.0 / (2.0 * pb.mass));
                const float f7 = sps * sph + cps * sth * cph, f8 = -cps * sph + sps * sth * cph, f9 = cth * cph;
                const float fsum = f7 * pv[6] + f8 * pv[7] + f9 * pv[8];
                const float u = mh * fsum;
                const float sq = pv[9] * pv[9] + pv[10] * pv[10] + pv[11] * pv[11];
                float Lg = (float)pb.alphQ * 0.f;                                  // Quadcopter.py:116-122 (one craft: W = 0)
                Lg = Lg + 2.f + u * u + 0.25f * sq;
                const float s1 = xv[6] * pv[0] + xv[7] * pv[1] + xv[8] * pv[2];
                const float s2 = xv[9] * pv[3] + xv[10] * pv[4] + xv[11] * pv[5];
                const float H = 0.f - Lg - s1 - s2 - (u / Mq) * fsum + grav * pv[8] + 0.5f * sq;
                const float dh = pv[12] - H;
                const float eh = (dh > 0.f) ? 1.f : (dh < 0.f ? -1.f : 0.f);
                const float inv = lds[LL.lINV + s_];
                const float kL = hs * wst * inv, ekh = eh * (hs * wst * ba.a3 * inv);
                const float cl = kL + ekh, ch = -ekh;                              // quad_adjoint with N = 1, a = 0
                const float fu = (fb[6] * f7 + fb[7] * f8 + fb[8] * f9) / Mq;
                const float ku = fu + (2.f * cl + 4.f * ch) * u;
                const float kum = ku * mh;
                const float a7 = kum * pv[6] + u * fb[6] / Mq, a8 = kum * pv[7] + u * fb[7] / Mq, a9 = kum * pv[8] + u * fb[8] / Mq;
                // component j of gbar and of the direct x term (every candidate is formed, the choice compiles to v_cndmask)
                const float xsel = j == 0 ? xv[6] : j == 1 ? xv[7] : j == 2 ? xv[8] : j == 3 ? xv[9] : j == 4 ? xv[10] : xv[11];
                const float g678 = j == 6 ? kum * f7 : (j == 7 ? kum * f8 : kum * f9 + ch * grav);
                const float fbh = j == 9 ? fb[9] : (j == 10 ? fb[10] : fb[11]);
                const float phh = j == 9 ? pv[9] : (j == 10 ? pv[10] : pv[11]);
                float gbj = 0.f;
                gbj = (j == 12) ? ekh : gbj;
                gbj = (j >= 9 && j < 12) ? (-0.5f * fbh + (0.5f * cl + ch) * phh) : gbj;
                gbj = (j >= 6 && j < 9) ? g678 : gbj;
                gbj = (j < 6) ? -ch * xsel : gbj;
                const float fbl = j == 6 ? fb[0] : j == 7 ? fb[1] : j == 8 ? fb[2] : j == 9 ? fb[3] : j == 10 ? fb[4] : fb[5];
                const float pl_ = j == 6 ? pv[0] : j == 7 ? pv[1] : j == 8 ? pv[2] : j == 9 ? pv[3] : j == 10 ? pv[4] : pv[5];
                const float xd3 = -a7 * f8 + a8 * f7;
                const float xd4 = a7 * cps * cth * cph + a8 * sps * cth * cph - a9 * sth * cph;
                const float xd5 = a7 * (sps * cph - cps * sth * sph) + a8 * (-cps * cph - sps * sth * sph) - a9 * cth * sph;
                float xdj = 0.f;
                xdj = (j >= 6 && j < 12) ? (fbl - ch * pl_) : xdj;
                xdj = (j == 3) ? xd3 : (j == 4 ? xd4 : (j == 5 ? xd5 : xdj));
                TL(cc, 29);
                if (j <= 12) GB[s_ * LDs + j] = gbj;
                if (j < 12) XD[s_ * ZLD + j] = xdj;
                lds[mp.lGF + ((j >> 2) * 16 + s_) * 4 + (j & 3)] = (j <= 12) ? gbj : 0.f;      // ... and the gbar fragment of P1'
            } else {
                physics_sums(cc, pl, pb);
                TL(cc, 11);
                if (tid < T) {
                    const int s = tid;
                    const float inv = lds[LL.lINV + s];
                    const Costs cs = physics_finish(cc, pl, pb, s);
                    const float dh = G[s * GLD + d] - cs.H;
                    const float eh = (dh > 0.f) ? 1.f : (dh < 0.f ? -1.f : 0.f);
                    const float kL = hs * wst * inv, kh = hs * wst * ba.a3 * inv;
                    SC[s * 4 + 0] = quad ? kL : kL + eh * kh;
                    SC[s * 4 + 1] = eh * kh;
                    SC[s * 4 + 2] = kL - eh * kh;
                }
                __syncthreads();
                if (quad) {
                    quad_adjoint(cc, pl, pb, hs, wst, cpl, SC);
                } else {
                    for (int j = tid; j < T * d; j += 256) {
                        const int t = j / d, i = j - t * d;
                        const float fbar = hs * (wst * LAM[t * ZLD + i] + cpl * XP[t * ZLD + i]);
                        GB[t * LDs + i] = -fbar + SC[t * 4 + 2] * G[t * GLD + i];
                        XD[t * ZLD + i] = 0.f;
                    }
                }
                if (tid < T) GB[tid * LDs + d] = SC[tid * 4 + 1];
                __syncthreads();
                if (!quad) { physics_xgrad(cc, pl, pb, SC, 4); __syncthreads(); }
            }

            // ================= vector-Jacobian product of grad Phi =================
            TL(cc, 12);
            if (fin || !quad1) mono_rows_to_frag<KBD>(mp.lGF, pl.lGB, LDs, D1, tid);
            // the value's cotangent (terminal evaluation only; weight gradients only: the state's share is already in lambda)
            const float phib = lds[LL.lPHIB + l16];
            __syncthreads();
            TL(cc, 13);
            mono_gemm<MT, KBD, false>(K1, (mp.lGF >> 2) + lane, acc);                  // ybar = K0 gbar
            mono_lowrank<KBD>(mp, AZ, mp.lGF, wave, lane);                             // A gbar (z is consumed: P4 and Phi are behind barriers)
            f32x4 ab0[MT], tb0[MT];
#pragma unroll
            for (int mi = 0; mi < MT; ++mi) {
                const int mt = wave + 4 * mi;
#pragma unroll
                for (int e = 0; e < 4; ++e) { ab0[mi][e] = th0[mi][e] * acc[mi][e]; tb0[mi][e] = av[mi][e] * acc[mi][e]; }
                if (mt < KBM) {
                    const float4 a4 = make_float4(ab0[mi][0], ab0[mi][1], ab0[mi][2], ab0[mi][3]);
                    L4[(mp.lVF >> 2) + mt * 64 + lane] = a4;                           // (v fragments are consumed: behind P3's barrier)
                    if constexpr (STATES != 1) *reinterpret_cast<float4*>(lds + mp.lRAB + l16 * LDR + 16 * mt + 4 * slot) = a4;
                }
            }
            TL(cc, 14);
            __syncthreads();
            TL(cc, 15);
            mono_gemm<MT, KBM, true>(W2, (mp.lVF >> 2) + lane, acc);                   // vbar = hN K1 abar0
            TL(cc, 16);
#pragma unroll
            for (int mi = 0; mi < MT; ++mi) {
                const int mt = wave + 4 * mi;
                float qb[4], qt[4], dwv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float vb = hN * acc[mi][e], t1 = th1[mi][e];
                    const float dwr = ab0[mi][e] + t1 * vb + phib * u1k[mi][e];        // dw row (+ the value's: phib u_1)
                    qb[e] = (1.f - t1 * t1) * wv[mi][e] * vb;
                    qt[e] = qb[e] + phib * hN * (t1 * wv[mi][e]);                      // + the value's: phib hN v
                    dwv[e] = dwr;
                }
                if (mt < KBM) {
                    if constexpr (STATES != 1) {
                        float4 s1_ = L4[(LL.lACC >> 2) + (KBM + mt) * 64 + lane], s2_ = L4[(LL.lACC >> 2) + (2 * KBM + mt) * 64 + lane];
                        s1_.x += qt[0]; s1_.y += qt[1]; s1_.z += qt[2]; s1_.w += qt[3];
                        s2_.x += dwv[0]; s2_.y += dwv[1]; s2_.z += dwv[2]; s2_.w += dwv[3];
                        L4[(LL.lACC >> 2) + (KBM + mt) * 64 + lane] = s1_; L4[(LL.lACC >> 2) + (2 * KBM + mt) * 64 + lane] = s2_;
                    }
                    L4[(mp.lUF >> 2) + mt * 64 + lane] = make_float4(qb[0], qb[1], qb[2], qb[3]);      // (y fragments are consumed: behind P4's barrier)
                    if constexpr (STATES != 1) *reinterpret_cast<float4*>(lds + mp.lRQB + l16 * LDR + 16 * mt + 4 * slot) = make_float4(qt[0], qt[1], qt[2], qt[3]);
                }
            }
            TL(cc, 17);
            __syncthreads();
            TL(cc, 18);
            mono_gemm<MT, KBM, true>(W3, (mp.lUF >> 2) + lane, acc);                   // ubar0 = K1' qbar
            TL(cc, 19);
#pragma unroll
            for (int mi = 0; mi < MT; ++mi) {
                const int mt = wave + 4 * mi;
                float ob[4], ot[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t0 = th0[mi][e];
                    ob[e] = (1.f - t0 * t0) * tb0[mi][e] + t0 * acc[mi][e];
                    ot[e] = ob[e] + phib * (t0 * av[mi][e]);                           // + the value's: phib y
                }
                if (mt < KBM) {
                    if constexpr (STATES != 1) {
                        float4 s0_ = L4[(LL.lACC >> 2) + mt * 64 + lane];
                        s0_.x += ot[0]; s0_.y += ot[1]; s0_.z += ot[2]; s0_.w += ot[3];
                        L4[(LL.lACC >> 2) + mt * 64 + lane] = s0_;
                    }
                    L4[(mp.lVF >> 2) + mt * 64 + lane] = make_float4(ob[0], ob[1], ob[2], ob[3]);      // (abar0 fragments are consumed: behind the barrier above)
                    if constexpr (STATES != 1) *reinterpret_cast<float4*>(lds + mp.lROB + l16 * LDR + 16 * mt + 4 * slot) = make_float4(ot[0], ot[1], ot[2], ot[3]);
                }
            }
            TL(cc, 20);
            __syncthreads();
            TL(cc, 21);
            mono_close<MT, KBM, KBD>(mp, mp.lVF, wave, lane);                          // sbar = K0' obar + A'(A gbar)
            TL(cc, 22);
            __syncthreads();
            mono_close_rows<KBD>(mp, pl.lSBAR, GLD, false, tid);
            TL(cc, 23);

            // ================= weight gradients: outer products with the 16 samples on the k axis =================
            if constexpr (STATES != 1) {
                float aV[MT][4], aQ[MT][4], aY[MT][4], aO[MT][4];
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    const int mt = wave + 4 * mi, mo = 16 * (mt < KBM ? mt : 0) + l16;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int so = (4 * slot + e) * LDR + mo;
                        aV[mi][e] = lds[mp.lRV + so]; aQ[mi][e] = lds[mp.lRQB + so];
                        aY[mi][e] = lds[mp.lRY + so]; aO[mi][e] = lds[mp.lROB + so];
                        if (mt >= KBM) { aV[mi][e] = 0.f; aQ[mi][e] = 0.f; aY[mi][e] = 0.f; aO[mi][e] = 0.f; }
                    }
                }
                float bG[KBD][4], bS[KBD][4];
#pragma unroll
                for (int ct = 0; ct < KBD; ++ct)
#pragma unroll
                    for (int e = 0; e < 4; ++e) { bG[ct][e] = GB[(4 * slot + e) * LDs + 16 * ct + l16]; bS[ct][e] = SB[(4 * slot + e) * LDs + 16 * ct + l16]; }
#pragma unroll
                for (int ct = 0; ct < KBD; ++ct)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
#pragma unroll
                        for (int mi = 0; mi < MT; ++mi) mfma16_vv(dK0a[mi][ct], aY[mi][e], bG[ct][e]);
#pragma unroll
                        for (int mi = 0; mi < MT; ++mi) mfma16_vv(dK0a[mi][ct], aO[mi][e], bS[ct][e]);
                    }
                // dM = sum gbar s' (+ the value's 1/2 phib s s'): one tile (wave 3), or the 2 x 2 tiles (row block wave / 2, column block wave % 2)
                if (KBD == 2 || wave == 3) {
                    const int ri = KBD == 2 ? (wave >> 1) : 0, ci = KBD == 2 ? (wave & 1) : 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float gr = KBD == 2 ? (ri ? bG[KBD - 1][e] : bG[0][e]) : bG[0][e], sr = KBD == 2 ? (ri ? bS[KBD - 1][e] : bS[0][e]) : bS[0][e];
                        const float sc_ = KBD == 2 ? (ci ? bS[KBD - 1][e] : bS[0][e]) : bS[0][e];
                        const float ag = gr + 0.5f * lds[LL.lPHIB + 4 * slot + e] * sr;
                        mfma16_vv(dMa, ag, sc_);
                    }
                }
                float bA[2][4], bU[2][4];                                              // column operands one tile ahead of the MFMAs that use them
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int so = (4 * slot + e) * LDR + l16;
                    bA[0][e] = lds[mp.lRAB + so]; bU[0][e] = lds[mp.lRU0 + so];
                }
#pragma unroll
                for (int jt = 0; jt < KBM; ++jt) {
                    if (jt + 1 < KBM) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int so = (4 * slot + e) * LDR + 16 * (jt + 1) + l16;
                            bA[(jt + 1) & 1][e] = lds[mp.lRAB + so]; bU[(jt + 1) & 1][e] = lds[mp.lRU0 + so];
                        }
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
#pragma unroll
                        for (int mi = 0; mi < MT; ++mi) mfma16_aa(dK1a[mi][jt], aV[mi][e], bA[jt & 1][e]);
#pragma unroll
                        for (int mi = 0; mi < MT; ++mi) mfma16_aa(dK1a[mi][jt], aQ[mi][e], bU[jt & 1][e]);
                    }
                }
                if (tid < 16) dcba += lds[LL.lPHIB + tid];                             // c.bias = sum phib
            }
            TL(cc, 24);
            __syncthreads();
            TL(cc, 25);
            // ================= RK adjoint recurrences =================
            {
                const int t = tid >> 4;
#pragma unroll
                for (int q = 0; q < KBD; ++q) {
                    const int i = (tid & 15) + 16 * q;
                    if constexpr (STATES != 1) dca[q] += GB[t * LDs + i] + lds[LL.lPHIB + t] * SB[t * LDs + i];  // dc = sum gbar (+ phib s); entries >= d + 1 of the rows are 0
                    if (i < d) {
                        const float xb = SBAR[t * GLD + i] + XD[t * ZLD + i];
                        if (fin) {
                            LAM[t * ZLD + i] += xb;
                        } else {
                            XP[t * ZLD + i] = xb;
                            const float xs = XS[t * ZLD + i] + xb;
                            XS[t * ZLD + i] = xs;
                            if (st == 0) LAM[t * ZLD + i] += xs;
                        }
                    }
                }
            }
            if (fin && tid < T) lds[LL.lPHIB + tid] = 0.f;
            if (stt == 0) { --kk; stt = ba.nstage - 1; } else { --stt; }
            __syncthreads();
            TL(cc, 26);
        }
        if (ba.lam0)
            for (int j = tid; j < T * d; j += 256) {
                const int t = j / d, i = j - t * d;
                if (t < nvalid) ba.lam0[(row0 + t) * d + i] = LAM[t * ZLD + i];
            }
    }

    if constexpr (STATES != 1) {
    // ---- this workgroup's partial gradient vector: K0 [m][D1], b0, K1 [m][m], b1, w, c.weight [D1], c.bias, dM [D1][D1]
    float* gp = ba.gpart + (long)blockIdx.x * ba.gstride;
    const long oK0 = 0, ob0 = (long)m * D1, oK1 = ob0 + m, ob1 = oK1 + (long)m * m, ow = ob1 + m, ocw = ow + m, ocb = ocw + D1, oM = ocb + 1;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
        const int mt = wave + 4 * mi;
#pragma unroll
        for (int ct = 0; ct < KBD; ++ct) SL_FENCE4(dK0a[mi][ct], dK0a[mi][ct], dK0a[mi][ct], dK0a[mi][ct]);
#pragma unroll
        for (int jt = 0; jt < KBM; ++jt) SL_FENCE1A(dK1a[mi][jt]);
        if (mt >= KBM) continue;
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int i = 16 * mt + 4 * slot + rr;
            if (i >= m) continue;
#pragma unroll
            for (int ct = 0; ct < KBD; ++ct) if (16 * ct + l16 < D1) gp[oK0 + (long)i * D1 + 16 * ct + l16] = dK0a[mi][ct][rr];
#pragma unroll
            for (int jt = 0; jt < KBM; ++jt) {
                const int j = 16 * jt + l16;
                if (j < m) gp[oK1 + (long)i * m + j] = dK1a[mi][jt][rr];
            }
        }
        // the vectors: every lane holds 4 features of ONE sample; the 16 samples of a feature sit in one 16-lane row
        {
            const float4 v0 = L4[(LL.lACC >> 2) + mt * 64 + lane], v1 = L4[(LL.lACC >> 2) + (KBM + mt) * 64 + lane], v2 = L4[(LL.lACC >> 2) + (2 * KBM + mt) * 64 + lane];
            const float a0_[4] = {v0.x, v0.y, v0.z, v0.w}, a1_[4] = {v1.x, v1.y, v1.z, v1.w}, a2_[4] = {v2.x, v2.y, v2.z, v2.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float s0 = sum16(a0_[e]), s1 = sum16(a1_[e]), s2 = sum16(a2_[e]);
                const int i = 16 * mt + 4 * slot + e;
                if (l16 == 0 && i < m) { gp[ob0 + i] = s0; gp[ob1 + i] = s1; gp[ow + i] = s2; }
            }
        }
    }
    if (KBD == 2 || wave == 3) {
        const int ri = KBD == 2 ? (wave >> 1) : 0, ci = KBD == 2 ? (wave & 1) : 0;
        SL_FENCE4(dMa, dMa, dMa, dMa);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int i = 16 * ri + 4 * slot + rr, j = 16 * ci + l16;
            if (i < D1 && j < D1) gp[oM + (long)i * D1 + j] = dMa[rr];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < KBD; ++q) lds[LL.lRV + q * 256 + tid] = dca[q];      // (the row operands are consumed)
    __syncthreads();
    if (tid < 16) {
#pragma unroll
        for (int q = 0; q < KBD; ++q) {
            float sdc = 0.f;
            for (int t = 0; t < T; ++t) sdc += lds[LL.lRV + q * 256 + t * 16 + tid];
            if (16 * q + tid < D1) gp[ocw + 16 * q + tid] = sdc;
        }
        const float cb = sum16(dcba);
        if (tid == 0) gp[ocb] = cb;
    }
    }
}
