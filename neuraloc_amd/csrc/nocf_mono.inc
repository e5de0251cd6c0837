// nocf_mono.inc -- weight-STATIONARY rollout for MEDIUM networks (nTh = 2, m <= 128: singlequad, m = 128, d = 12): the whole
// network fits ONE CU's AccVGPRs, so a workgroup (4 waves, 16 samples) never fetches a weight after its prologue and never
// talks to another workgroup: the GEMM chain of an evaluation runs out of registers and LDS alone.
//
// Same arithmetic shape as the slab kernel (nocf_slab.inc): v_mfma_f32_16x16x4_f32 with the WEIGHTS as the A operand (16 output
// features) and the 16 samples as N, activations in 1 KiB fragments [64 lanes][4 floats] (a lane's four result registers are
// four consecutive features of one sample = the B fragment of the next GEMM), hand-written MFMAs with AccVGPR SrcA operands.
// Wave w owns the hidden M-tiles w and w+4 (m = 128: 2 x 8 k-blocks of K1 per orientation = 128 AccVGPRs per lane).
//     P1  o = K0 s + b0, u0 = sigma(o), tanh(o)         (B = s fragments built from the state rows)
//     P2  q = K1 u0 + b1, v = tanh(q) . w               (B = u0 fragments: LDS, one barrier)
//     P3  a = w + hN K1^T v, y = tanh(o) . a            (B = v fragments)
//     P4  g = K0^T y + A^T (A s) + c                    (contraction split over the waves, fixed-order sum through LDS)
// then the problem physics (all three classes, the same device functions as the tile kernel, T = 16 samples) and the RK update.
// intermediates=True (zFull / ctrlFull, the extra control evaluation per step of src/OCflow.py:51-55) is supported: the shock
// sweep of BASELINE config 5 runs here.  Compile-time shapes: KBM = ceil(m/16) k-blocks of the hidden width (hidden units are
// zero-padded to it), KBD = ceil((d+1)/16) k-blocks of the input.

// ---- written-out v_mfma_f32_16x16x4_f32 with the wait states the compiler does not add around inline asm (round 3: the fences NAME
// the accumulators; round 2's operand-less fence let the scheduler hoist the first VALU read of an accumulator above its wait
// states -- the register-allocation-dependent wrong results recorded in DESIGN 3.1d, found by tools/mfma_hazard_check.py)
__device__ __forceinline__ f32x4 mfma16(float a, float b, f32x4 c) {
    // D[m][n] += sum_k A[m][k] B[k][n];  A: lane -> (m = lane%16, k = lane/16);  B: lane -> (k = lane/16, n = lane%16);
    // D: lane -> n = lane%16, register r -> m = 4 (lane/16) + r
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// The resident weight slices live in AccVGPRs (the upper half of the unified 512-entry register file).  Left to itself the
// compiler copies every A operand down with v_accvgpr_read_b32 first, and each such copy stalls the matrix pipe (measured:
// 46..53 cycles per MFMA instead of 32); the instruction itself may name an AccVGPR as SrcA, so the MFMAs of the slab kernel
// are written out.  The accumulators are ordinary VGPRs; four independent chains per GEMM keep dependent instructions
// 128 cycles apart (no software wait states needed between them); SL_FENCE4 / SL_LEAD4 below carry the wait states the ISA
// demands around a chain (the hazard recogniser cannot see through inline assembly).
// ("s_nop 1" inside the string: a VGPR operand a VALU instruction wrote just before needs 2 states, and nothing outside the string
// is padded for it; beside a 32-cycle MFMA the 2 issue cycles are free)
__device__ __forceinline__ void mfma16_acc(f32x4& acc, float w_acc, float b) {
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "a"(w_acc), "v"(b));
}
__device__ __forceinline__ void mfma16_vv(f32x4& acc, float w, float b) {
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x4_f32 %0, %1, %2, %0" : "+v"(acc) : "v"(w), "v"(b));
}
// the FIRST product of a chain: C = 0 as an inline constant, so the accumulators are never zeroed by VALU moves (32 v_mov per product and
// wave: 128 of the ~530 vector instructions of a forward evaluation, counters in profiles/r4/16_*)
__device__ __forceinline__ void mfma16_acc0(f32x4& acc, float w_acc, float b) {
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x4_f32 %0, %1, %2, 0" : "=v"(acc) : "a"(w_acc), "v"(b));
}
__device__ __forceinline__ void mfma16_vv0(f32x4& acc, float w, float b) {
    asm volatile("s_nop 1\n\tv_mfma_f32_16x16x4_f32 %0, %1, %2, 0" : "=v"(acc) : "v"(w), "v"(b));
}
// The wait states between the last MFMA of a chain and the first VALU access of its accumulators (8 passes: 12 states) and
// between a VALU write of an operand and the MFMA that reads it (2 states).  Both statements NAME the accumulators as "+v"
// operands: an asm statement is ordered against register-only instructions only through its operands ("memory" orders loads
// and stores, nothing else).  Round 2's fence had no operands, and in a build with a different register allocation (lYF in a
// pinned SGPR) the scheduler hoisted the v_pk_add_f32 that sums the four chains ABOVE the nops, 3..6 states behind the last
// MFMA: it read accumulators the matrix pipe was still writing -- the "wrong costs" of DESIGN 3.1d (round 2), found by
// tools/mfma_hazard_check.py (profiles/r3/00_lyf_rootcause_*).
#define SL_FENCE4(a, b, c, d) asm volatile("s_nop 7\n\ts_nop 4" : "+v"(a), "+v"(b), "+v"(c), "+v"(d))
#define SL_LEAD4(a, b, c, d) asm volatile("s_nop 1" : "+v"(a), "+v"(b), "+v"(c), "+v"(d))

#define NOCF_PIN(v) asm volatile("" : "+s"(v))
__device__ __forceinline__ void pin_plan(DevPlan& p) {
    NOCF_PIN(p.d); NOCF_PIN(p.D1); NOCF_PIN(p.m); NOCF_PIN(p.r); NOCF_PIN(p.LD); NOCF_PIN(p.LDs); NOCF_PIN(p.GLD); NOCF_PIN(p.ZLD); NOCF_PIN(p.T);
    NOCF_PIN(p.hN); NOCF_PIN(p.cb);
    NOCF_PIN(p.lSB); NOCF_PIN(p.lG); NOCF_PIN(p.lZQ); NOCF_PIN(p.lZ0); NOCF_PIN(p.lZA); NOCF_PIN(p.lDZ); NOCF_PIN(p.lRED); NOCF_PIN(p.lSC);
    NOCF_PIN(p.lPHI); NOCF_PIN(p.lTRIG); NOCF_PIN(p.lPT); NOCF_PIN(p.lPW); NOCF_PIN(p.nAg);
}


struct MonoPlan {
    DevPlan pp;                    // shapes, vector offsets, the physics view (T = 16 samples per workgroup)
    int KBM, KBD;
    long oW2, oW3, oK1, oK4, oAZ, oAT;       // float4 offsets of the images in the workspace
    int lSF, lUF, lVF, lK4, lAT, lVO, lCW, lZP, lGP, lPHIP;    // LDS float offsets
    int lGF, lRV, lRAB, lRQB, lRU0, lRY, lROB, pad_;            // adjoint (nocf_mono_bwd.inc): gbar fragments, the row-layout operands of the outer products
};
static_assert(sizeof(MonoPlan) % 4 == 0 && sizeof(MonoPlan) / 4 <= 256, "plan copy is done by one 256-thread block");

// The LDS layout of the forward kernel as a compile-time constant (round 4, like the adjoint's: nocf_mono_bwd.inc): row strides at their
// d + 1 <= 64 values, room for MONO_NAG agents.  With the offsets in scalar registers the kernel ran out of them (62 v_readlane reloads of
// spilled scalars per evaluation); as constants every LDS address is one lane-dependent register plus an immediate.
struct MonoFwdLds { int lSF, lUF, lVF, lK4, lAT, lVO, lCW, lZP, lGP, lPHIP, lSB, lG, lZQ, lZ0, lZA, lDZ, lRED, lSC, lPHI, lTRIG, lPT, lPW, total; };
#define MONO_LDS_S 68
#define MONO_GLD 64
#define MONO_ZLD(KBD) ((KBD) == 1 ? 20 : 36)
#define MONO_NAG(KBD) ((KBD) == 1 ? 8 : 16)
constexpr MonoFwdLds mono_fwd_lds(int KBM, int KBD) {
    MonoFwdLds L{};
    int l = 0;
    const int T = 16, Z = MONO_ZLD(KBD), NA = MONO_NAG(KBD);
    L.lSF = l; l += KBD * 256; L.lUF = l; l += KBM * 256; L.lVF = l; l += KBM * 256; L.lK4 = l; l += KBD * KBM * 256; L.lAT = l; l += KBD * 256;
    L.lVO = l; l += 3 * KBM * 16; L.lCW = l; l += KBD * 16; L.lZP = l; l += 4 * 256; L.lGP = l; l += KBD * 4 * 256; L.lPHIP = l; l += 64;
    L.lSB = l; l += T * MONO_LDS_S; L.lG = l; l += T * MONO_GLD; L.lZQ = l; l += T * ZQLD; L.lZ0 = l; l += T * Z; L.lZA = l; l += T * Z; L.lDZ = l; l += T * Z;
    L.lRED = l; l += 64; L.lSC = l; l += T * NA + 8; L.lPHI = l; l += T; L.lTRIG = l; l += T * KBD * 6 /* quadcopters: d / 12 crafts */; L.lPT = l; l += 4; L.lPW = l; l += 4;
    L.total = l;
    return L;
}

// images (mt = hidden M-tile, kb = k-block, dt = tile of the d+1 outputs), all zero-padded:
//   W2[mt][kb][lane] = K1[16mt + lane%16][16kb + 4(lane/16) + q]      W3[mt][kb][lane] = K1[16kb + 4(lane/16) + q][16mt + lane%16]
//   K1[mt][kb][lane] = K0[16mt + lane%16][16kb + 4(lane/16) + q]      K4[dt][kb][lane] = K0[16kb + 4(lane/16) + q][16dt + lane%16]
//   AZ[kb][lane]     = A[lane%16][16kb + 4(lane/16) + q]              AT[dt][lane]     = A[4(lane/16) + q][16dt + lane%16]
__global__ void mono_pack_kernel(MonoPlan mp, DevPhi P, float* __restrict__ ws) {
#define PACK_BID blockIdx.x
#define PACK_NBLK gridDim.x
#include "nocf_mono_pack_body.inc"
#undef PACK_BID
#undef PACK_NBLK
}

// Ensembles on this family (include/nocf.h, nocf_rollout_mid_ensemble_f32; DESIGN 3.13): E networks of one shape, member e on workgroups
// [e * tiles, (e + 1) * tiles) of ONE launch.  A tile never leaves its CU and a network never leaves its workgroup, so an ENS kernel offsets
// its pointers to member e's blocks at its top and runs the single-network statements on them.  The member information is a LAST kernel
// argument (no new field in RollArgs / BwdArgs / MonoPlan: the offsets of the existing arguments stay where they are).  All strides in floats.
struct MonoEnsArgs {
    unsigned n;                      // rows of ONE member
    unsigned tiles;                  // workgroups per member: ceil(n / 16) (forward), nocf_mid_grad_rows (adjoint)
    long xs;                         // member stride of x: 0 (shared starts) or n d
    long wss;                        // member stride of the workspace (images, padded vectors, the plan record with the member's c.bias)
    const float* alph;               // device [E, 6]: [0] -> a0, [1] -> alph_Q, [2] -> alph_W, [3..5] -> a3..a5
    long zfs, cfs, sas, acts;        // member strides of zFull [nt+1, n, d+4], ctrlFull [nt+1, n, cdim], s_all [nt*nstage, n, d+1], the activation record
};

// packs all members in one launch: member blockIdx.y, the two single-network pack bodies on that member's tensors and workspace block
// (pack_kernel's padded vectors and copy of A, then the images and the plan record of mono_pack_kernel; both write the plan words, the same
// thread the same word, the one-CU record last)
__global__ void mono_ens_pack_kernel(DevPlan pl, MonoPlan mp, DevPhi Pst, float* __restrict__ ws0, long wss) {
    const long e = blockIdx.y;
    const long m = pl.m, D1 = pl.D1;
    const DevPhi P{Pst.K0 + e * m * D1, Pst.b0 + e * m, Pst.K + e * (pl.nTh - 1) * m * m, Pst.b + e * (pl.nTh - 1) * m, Pst.w + e * m,
                   Pst.A + e * pl.r * D1, Pst.cw + e * D1, Pst.cbp + e};
    float* __restrict__ ws = ws0 + e * wss;
#define PACK_BID blockIdx.x
#define PACK_NBLK gridDim.x
    {
#include "nocf_pack_body.inc"
    }
    {
#include "nocf_mono_pack_body.inc"
    }
#undef PACK_BID
#undef PACK_NBLK
}

// acc[mi] = sum over NKB k-blocks of W[mi][kb] (A operand, registers) x the fragments at LDS float4 index bq + kb*64 (B operand),
// for the wave's MT M-tiles at once (a B fragment is read once and feeds all of them); two chains per tile and k-parity.
template <int MT, int NKB, bool ACC>
__device__ __forceinline__ void mono_gemm(const f32x4 (&W)[MT][NKB], int bq, f32x4 (&out)[MT]) {
    // two chains per tile (components x, z / y, w of a k-block), as in the split-role kernel: a dependent MFMA follows two issue slots
    // behind its predecessor, and the epilogue adds two accumulators instead of four (4 instead of 12 v_add per tile and product)
    f32x4 a[MT][2];
    const float4* L4 = reinterpret_cast<const float4*>(lds);
    float4 ring[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) ring[i] = L4[bq + (i < NKB ? i : 0) * 64];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        if (kb + 3 < NKB) ring[(kb + 3) & 3] = L4[bq + (kb + 3) * 64];
        const float4 bf = ring[kb & 3];
#pragma unroll
        for (int mi = 0; mi < MT; ++mi) {
            if (ACC) {
                if (kb == 0) { mfma16_acc0(a[mi][0], W[mi][kb][0], bf.x); mfma16_acc0(a[mi][1], W[mi][kb][1], bf.y); }      // (the chains start from the inline constant 0)
                else { mfma16_acc(a[mi][0], W[mi][kb][0], bf.x); mfma16_acc(a[mi][1], W[mi][kb][1], bf.y); }
                mfma16_acc(a[mi][0], W[mi][kb][2], bf.z); mfma16_acc(a[mi][1], W[mi][kb][3], bf.w);
            } else {
                if (kb == 0) { mfma16_vv0(a[mi][0], W[mi][kb][0], bf.x); mfma16_vv0(a[mi][1], W[mi][kb][1], bf.y); }
                else { mfma16_vv(a[mi][0], W[mi][kb][0], bf.x); mfma16_vv(a[mi][1], W[mi][kb][1], bf.y); }
                mfma16_vv(a[mi][0], W[mi][kb][2], bf.z); mfma16_vv(a[mi][1], W[mi][kb][3], bf.w);
            }
        }
    }
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) asm volatile("s_nop 7\n\ts_nop 4" : "+v"(a[mi][0]), "+v"(a[mi][1]));
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) out[mi] = a[mi][0] + a[mi][1];
}

// sin and cos of one angle, <= 1.6 ulp for |x| <= 1e3 (3-term Cody-Waite reduction by pi/2 with FMAs, the classic degree-7 / degree-8
// minimax polynomials on [-pi/4, pi/4]); larger arguments take the library's.  ~30 instructions instead of the library's ~300-cycle path:
// the quadcopter's angles sit on the critical path of every evaluation.
__device__ __forceinline__ void mono_sincos(float x, float& sn, float& cs) {
    if (!(fabsf(x) <= 1000.f)) { sincosf(x, &sn, &cs); return; }
    const float q = rintf(x * 0.63661977236758134f);
    float r = fmaf(q, -1.5707963705062866f, x);
    r = fmaf(q, 4.371138828673793e-08f, r);
    r = fmaf(q, 1.7763568394002505e-15f, r);
    const float z = r * r;
    const float s = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), z * r, r);
    const float c = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), z * z, fmaf(-0.5f, z, 1.f));
    const int n = (int)q & 3;
    sn = (n & 1) ? c : s; cs = (n & 1) ? s : c;
    if (n & 2) sn = -sn;
    if ((n + 1) & 2) cs = -cs;
}

// REC: the training variant (stage inputs RollArgs::sAll, activation record RollArgs::act); the evaluation variant carries no trace of it
// DIST: the disturbed rollout (RollArgs::dist, W [nt][n][d]): behind step k the state rows take z[:, :d] += W[k] where the step's z is written
// back (in front of the zFull store and of the control evaluation).  Each thread loads the entries of its own components at the top of the step
// (KBD + 1 registers at most; one for singlequad) and adds them behind the last stage.  REC and DIST together (the recording forward of
// disturbed training): the state rows SB hold the displaced state when the next step's first stage input and activations are recorded
// DIST == 2: the entries are drawn (nocf_noise.inc: RollArgs::nzScale / nzSeed / nzRow0) where DIST == 1 ADDS them, behind the last stage, into the
// same variable: nothing is held across the step's evaluations (drawn at the top of the step like the loads, the (4, 2) instantiation lost a wave)
// DIST == 3: time-correlated noise (nocf_noise.inc, DESIGN 3.18): the entry is formed where DIST == 2 draws it, from the w_{k-1} this thread carries
// for each of its components of the sweep (wcar: KBD + 1 registers at most, one for singlequad; RollArgs::nzScale1 / nzRho); rows past n and the
// four cost components carry 0 and draw nothing, so a tail tile's replicated rows leave the real rows' paths alone.  Single networks only
// ENS (DIST 0 / 1 / 2): an ensemble, see MonoEnsArgs.  ra.n is a member's row count; member e = blockIdx.x / en.tiles is workgroup-uniform, the
// member's last tile replicates the member's row n - 1.  Every ENS test is a compile-time choice at its place of use.
// ENS with DIST == 2 (nocf_rollout_noisy_mid_ensemble_f32, DESIGN 3.14): member e under its own noise level and seed, EnsNoiseArgs (nocf_noise.inc)
// as a further last argument that no other instantiation reads.  row0 is the tile's first row INSIDE the member, so ra.nzRow0 + row0 + s_ is
// already the key of a row; the kernel's copy of `ra` takes the member's scale row and seed, and both places that draw read them from there
// ENS with DIST == 1 (nocf_rollout_disturbed_mid_ensemble_f32, DESIGN 3.17; REC or not): member e under its own tensor disturbance, ra.dist = W
// [E, nt, n, d] member-major (EnsNoiseArgs::ws = nt n d) or one [nt, n, d] for all members (ws = 0).  The kernel's copy of ra.dist moves to the
// member's slice once, with the member's other pointers (workgroup-uniform); ra.n and row0 are the member's, so the DIST == 1 load and add
// below are the single-network statements on that slice
// HOLD (DIST 0 / 1; no REC, ENS; HoldArgs, nocf_dev.h): the zero-order-hold rollout (include/nocf.h, nocf_rollout_held_f32; DESIGN 3.19).  The
// network runs at the first stage of every K-th step -- on the state rows as the previous step left them, W[k-1] included -- and at the final
// time; every other evaluation is `held`: it skips the fragments, P1..P4, the gather and the gradient rows and goes straight to the physics.
// k, st and K are kernel-uniform, so every barrier of the skipped section is skipped by all 256 threads.  What stays where it is: the gradient
// rows Gl (point agents: physics_sums / physics_finish read p = -c from them) and the P4 partials GP (singlequad: the 16 lanes of a sample
// re-form the same pv from them), and singlequad's thrust in one register per thread (uh) -- f7..f9 come from the current angles, u does not.
// The HJB column's right-hand side is 0, the control evaluation behind a step with intermediates is gone (nsub = nstage) and ctrl_write
// writes the held control behind the last stage.  One craft only: the dispatcher refuses the general quadcopter branch of physics_finish
template <int KBM, int KBD, bool REC, int DIST = 0, bool ENS = false, bool HOLD = false>
__global__ void __launch_bounds__(256) rollout_mono_kernel(const MonoPlan* __restrict__ mpp, DevProb pb, float* ws, RollArgs ra, MonoEnsArgs en,
                                                           EnsNoiseArgs nz, HoldArgs hd) {
    static_assert(!HOLD || (!REC && !ENS && DIST <= 1), "the held rollout: evaluation of one network, W from memory or none");
    constexpr int MT = (KBM + 3) / 4;              // hidden M-tiles per wave: tiles w, w+4, ...
    constexpr int T = 16;
    constexpr MonoFwdLds LL = mono_fwd_lds(KBM, KBD);
    unsigned etile = 0;                            // ENS: this workgroup's tile inside its member
    if constexpr (ENS) {
        const unsigned e = blockIdx.x / en.tiles;
        etile = blockIdx.x - e * en.tiles;
        ws += e * en.wss;
        mpp = reinterpret_cast<const MonoPlan*>(reinterpret_cast<const float*>(mpp) + e * en.wss);
        const float* at = en.alph + e * 6;
        ra.a0 = at[0]; pb.alphQ = (double)at[1]; pb.alphW = (double)at[2];
        ra.x += e * en.xs;
        if (ra.zFull) { ra.zFull += e * en.zfs; ra.ctrlFull += e * en.cfs; }
        if (REC) { if (ra.sAll) ra.sAll += e * en.sas; if (ra.act) ra.act += e * en.acts; }
        if constexpr (DIST == 1) ra.dist += e * nz.ws;
    }
    MonoPlan mp = *mpp;                    // local copy; the LDS layout is a compile-time constant, the shape words sit in scalar registers
    mp.lSF = LL.lSF; mp.lUF = LL.lUF; mp.lVF = LL.lVF; mp.lK4 = LL.lK4; mp.lAT = LL.lAT; mp.lVO = LL.lVO; mp.lCW = LL.lCW; mp.lZP = LL.lZP;
    mp.lGP = LL.lGP; mp.lPHIP = LL.lPHIP;
    {
        DevPlan& q = mp.pp;
        q.T = 16; q.nwaves = 4; q.LDs = MONO_LDS_S; q.GLD = MONO_GLD; q.ZLD = MONO_ZLD(KBD);
        q.lSB = LL.lSB; q.lG = LL.lG; q.lZQ = LL.lZQ; q.lZ0 = LL.lZ0; q.lZA = LL.lZA; q.lDZ = LL.lDZ; q.lRED = LL.lRED; q.lSC = LL.lSC; q.lPHI = LL.lPHI;
        q.lTRIG = LL.lTRIG; q.lPT = LL.lPT; q.lPW = LL.lPW; q.ldsFloats = LL.total;
        NOCF_PIN(q.d); NOCF_PIN(q.D1); NOCF_PIN(q.m); NOCF_PIN(q.r); NOCF_PIN(q.hN); NOCF_PIN(q.cb); NOCF_PIN(q.nAg);
    }
    const DevPlan& pl = mp.pp;
    Ctx c;
    ctx_init(c, ws, (unsigned)(pl.oPlan * 4));
    c.cb = pl.cb;
    const int d = pl.d, D1 = pl.D1, r = pl.r, ZLD = pl.ZLD, GLD = pl.GLD, LDs = pl.LDs;
    const int wave = c.wave, lane = c.lane, tid = c.tid;
    const int slot = lane >> 4;
    const long row0 = (long)(ENS ? etile : blockIdx.x) * T;
    if constexpr (ENS) {                           // the member's blocks of persample [E, n, 7] and z_out [E, n, d+4]
        const long eo = (long)(blockIdx.x / en.tiles) * en.n;
        if (ra.persample) ra.persample += eo * 7;
        if (ra.z_out) ra.z_out += eo * (d + 4);
        if constexpr (DIST == 2) {                 // the member's row of the scale table [E, d] and its seed (workgroup-uniform)
            const unsigned e = blockIdx.x / en.tiles;
            ra.nzScale = nz.scale + (long)e * d; ra.nzSeed = nz.seeds[e];
        }
    }
    // time parameters of this tile's rows: the launch's, or its segment's (SegTab: segments are whole tiles)
    double sg_t0 = ra.t0, sg_h = ra.h;
    int sg_nt = ra.nt;
    long sg_slot = 0;                                                  // first time slot of these rows in zFull / ctrlFull
    if (!ENS && ra.seg.n > 0) {                    // (ENS: no segments; and the table is not indexed in a kernel that writes to its copy of `ra`)
        int k = (int)(row0 / ra.seg.rows); if (k >= ra.seg.n) k = ra.seg.n - 1;
        sg_t0 = ra.seg.t0[k]; sg_nt = ra.seg.nt[k]; sg_h = (ra.t1 - sg_t0) / sg_nt; sg_slot = ra.seg.slot0[k];
    }
    const float hN = pl.hN;
    const float4* ws4 = reinterpret_cast<const float4*>(ws);
    float4* L4 = reinterpret_cast<float4*>(lds);

    // ---- resident weights
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
    {   // z = A s: wave w contracts the input k-block w (KBD <= 4 here; more blocks would take further turns)
        const float4 a = (wave < KBD) ? ws4[mp.oAZ + (long)wave * 64 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
        AZ = (f32x4){a.x, a.y, a.z, a.w};
    }

    for (int i = tid; i < pl.ldsFloats; i += 256) lds[i] = 0.f;
    __syncthreads();
    // LDS-resident: K0^T tiles of P4, A^T tiles, the padded vectors b0 / b1 / w / c
    for (int i = tid; i < KBD * KBM * 64; i += 256) L4[(mp.lK4 >> 2) + i] = ws4[mp.oK4 + i];
    for (int i = tid; i < KBD * 64; i += 256) L4[(mp.lAT >> 2) + i] = ws4[mp.oAT + i];
    for (int i = tid; i < KBM * 16; i += 256) {
        lds[mp.lVO + i] = (i < pl.m) ? c.ws[pl.ob0 + i] : 0.f;
        lds[mp.lVO + KBM * 16 + i] = (i < pl.m) ? c.ws[pl.ob + i] : 0.f;
        lds[mp.lVO + 2 * KBM * 16 + i] = (i < pl.m) ? c.ws[pl.ow + i] : 0.f;
    }
    for (int i = tid; i < KBD * 16; i += 256) lds[mp.lCW + i] = (i < D1) ? c.ws[pl.ocw + i] : 0.f;

    float* SB = lds + pl.lSB;
    float* Z0 = lds + pl.lZ0;
    float* ZA = lds + pl.lZA;
    float* DZ = lds + pl.lDZ;
    const float* Gl = lds + pl.lG;
    for (int t = 0; t < T; ++t) {
        long row = row0 + t; if (row >= ra.n) row = ra.n - 1;          // tail rows replicate a valid sample
        for (int i = tid; i < d; i += 256) { const float v = ra.x[row * d + i]; Z0[t * ZLD + i] = v; SB[t * LDs + i] = v; }
        if (tid == 0) SB[t * LDs + d] = (float)sg_t0;
        if (ra.zFull && row0 + t < ra.n) {
            for (int i = tid; i < d + 4; i += 256) ra.zFull[(sg_slot * ra.n + row0 + t) * (d + 4) + i] = (i < d) ? ra.x[(row0 + t) * d + i] : 0.f;
            for (int i = tid; i < ra.cdim; i += 256) ra.ctrlFull[(sg_slot * ra.n + row0 + t) * ra.cdim + i] = 0.f;
        }
    }
    __syncthreads();

    // bias / w of this lane's features (16 mt + 4 slot + e) for the wave's M-tiles
    float b0v[MT][4], b1v[MT][4], wv[MT][4];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) {
        const int mt = wave + 4 * mi;
        const int o = (mt < KBM ? mt : 0) * 4 + slot;
        const float4 x0 = L4[(mp.lVO >> 2) + o], x1 = L4[((mp.lVO + KBM * 16) >> 2) + o], x2 = L4[((mp.lVO + 2 * KBM * 16) >> 2) + o];
        b0v[mi][0] = x0.x; b0v[mi][1] = x0.y; b0v[mi][2] = x0.z; b0v[mi][3] = x0.w;
        b1v[mi][0] = x1.x; b1v[mi][1] = x1.y; b1v[mi][2] = x1.z; b1v[mi][3] = x1.w;
        wv[mi][0] = x2.x; wv[mi][1] = x2.y; wv[mi][2] = x2.z; wv[mi][3] = x2.w;
        if (mt >= KBM) {                                       // a wave without an M-tile in this turn (m <= 32): its features are padding
#pragma unroll
            for (int e = 0; e < 4; ++e) { b0v[mi][e] = 0.f; b1v[mi][e] = 0.f; wv[mi][e] = 0.f; }
        }
    }

    const float c16 = (float)(1.0 / 6.0), c26 = (float)(2.0 / 6.0);
    const int nstage = (ra.stepper == NOCF_RK4) ? 4 : 1;
    const int nsub = nstage + ((ra.zFull && !HOLD) ? 1 : 0);
    const bool quad = (pb.kind == NOCF_PROB_QUADCOPTER);
    double tk = sg_t0;
    const bool quad1 = quad && pb.nAgents == 1 && d == 12 && KBD == 1;     // singlequad: wave-local physics below
    float qz0 = quad1 ? Z0[(tid >> 4) * ZLD + (tid & 15)] : 0.f, qzA = 0.f; // ... with component tid%16 of sample tid/16 of z in registers
    bool sf_ready = false;                                             // the RK update has already written the next stage state's fragments
    float uh = 0.f;                                                    // HOLD, singlequad: the held thrust of this thread's sample
    int kh = 0;                                                        // HOLD: steps left until the next sample
    float wcar[KBD + 1];                                               // DIST == 3: w_{k-1} of this thread's components of the write-back sweep
    if constexpr (DIST == 3) {
#pragma unroll
        for (int q = 0; q < KBD + 1; ++q) wcar[q] = 0.f;
    }

    for (int k = 0; k <= sg_nt; ++k) {
        const bool fin = (k == sg_nt);
        const double t1k = tk + sg_h;
        const double hsd = t1k - tk;                           // stepRK4 re-derives h = t1 - t0 (src/OCflow.py:170)
        const float hs = (float)hsd;
        if (fin) {
            if (tid < T) SB[tid * LDs + d] = (float)ra.t1;     // src/OCflow.py:62
            sf_ready = false;                                  // (the fragments carry the last step's own end time)
            __syncthreads();
        }
        constexpr int NDW = KBD + 1;                           // T (d + 4) <= 256 KBD + 48 components over 256 threads
        float wpre[NDW];
        if constexpr (DIST == 1) {
#pragma unroll
            for (int q = 0; q < NDW; ++q) wpre[q] = 0.f;
            if (!fin) {
                const float* wk = ra.dist + ((long)k * ra.n + row0) * d;
                if (quad1) {
                    const int s_ = tid >> 4, j = tid & 15;
                    if (j < d && row0 + s_ < ra.n) wpre[0] = wk[s_ * d + j];
                } else {
#pragma unroll
                    for (int q = 0; q < NDW; ++q) {
                        const int j = tid + 256 * q;
                        const int t = j / (d + 4), i = j - t * (d + 4);
                        if (j < T * (d + 4) && i < d && row0 + t < ra.n) wpre[q] = wk[t * d + i];
                    }
                }
            }
        }
        for (int st = 0; st < (fin ? 1 : nsub); ++st) {
            bool held = false;                                         // HOLD: this evaluation takes the sampled control (kernel-uniform)
            if constexpr (HOLD) {
                if (!fin && st == 0) { if (kh == 0) kh = hd.K; else held = true; --kh; }
                else held = !fin;
            }
#ifdef NOCF_STAMPS
            c.tl = (ra.stamps && blockIdx.x == 9 && k == 40 && st == 1) ? ra.stamps + 264 * 12 : nullptr;     // tools/slab_timeline.py mono
#endif
            TL(c, 0);
            // ---- stage-state fragments from the state rows: (kb, lane) = sample lane%16, entries 16 kb + 4 (lane/16) + e of [x, t]
            if (!sf_ready && !held) {
                for (int f = tid; f < KBD * 64; f += 256) {
                    const int l = f & 63, kb = f >> 6;
                    const float* srow = SB + (l & 15) * LDs + 16 * kb + 4 * (l >> 4);
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (16 * kb + 4 * (l >> 4) + e < D1) ? srow[e] : 0.f;
                    L4[(mp.lSF >> 2) + f] = make_float4(v[0], v[1], v[2], v[3]);
                }
                __syncthreads();
            }
            sf_ready = false;
            // training: the stage input s = [x, t] of this evaluation (RollArgs::sAll, [nt*nstage][n][d+1]); the state rows are complete
            // (the end barrier of the previous evaluation / the prologue) and nothing rewrites them before the RK update
            // (wave-uniform 64-bit bases + 32-bit lane offsets: per-lane 64-bit address arithmetic and a division by d + 1 for every stored piece
            // were ~2.9 k cycles per evaluation of the recording variant)
            if (REC && ra.sAll && !fin && st < nstage) {
                float* dst = ra.sAll + ((long)(k * nstage + st) * ra.n + row0) * D1;
                if (KBD == 1) {
                    const unsigned t = (unsigned)tid >> 4, i = (unsigned)tid & 15;
                    if ((int)i < D1 && row0 + t < ra.n) dst[t * (unsigned)D1 + i] = SB[t * LDs + i];
                } else {
                    for (int j = tid; j < T * D1; j += 256) {
                        const int t = j / D1, i = j - t * D1;
                        if (row0 + t < ra.n) dst[t * D1 + i] = SB[t * LDs + i];
                    }
                }
            }
            // ... and with an activation record (RollArgs::act) the activations of grad Phi of this evaluation: index of its rows, or -1
            const long recEv = (REC && ra.act && ra.sAll && !fin && st < nstage) ? (long)(k * nstage + st) : -1;
            float* recB = (REC && recEv >= 0) ? ra.act + (recEv * ra.n + row0) * pl.m : nullptr;          // rows of this tile in the first section
            const long recSec = ra.actRows * pl.m;
            const unsigned recL = (unsigned)(lane & 15) * (unsigned)pl.m + 4u * (unsigned)slot;              // + 16 mt: this lane's 4 features of its sample
            if (!held) {                                               // (HOLD: a held evaluation goes straight to the physics)
                TL(c, 1);
                // ================= P1: o = K0 s + b0, u0 = sigma(o), tanh(o);  z = A s rides along =================
                f32x4 acc[MT], th0[MT], u0k[MT];
                mono_gemm<MT, KBD, false>(K1, (mp.lSF >> 2) + lane, acc);
                {
                    f32x4 zacc = {0.f, 0.f, 0.f, 0.f};
                    if (wave < KBD) {
                        const float4 bz = L4[(mp.lSF >> 2) + wave * 64 + lane];
                        f32x4 z0, z1;
                        mfma16_vv0(z0, AZ[0], bz.x); mfma16_vv0(z1, AZ[1], bz.y); mfma16_vv(z0, AZ[2], bz.z); mfma16_vv(z1, AZ[3], bz.w);
                        asm volatile("s_nop 7\n\ts_nop 4" : "+v"(z0), "+v"(z1));
                        zacc = z0 + z1;
                    }
                    L4[(mp.lZP >> 2) + wave * 64 + lane] = make_float4(zacc[0], zacc[1], zacc[2], zacc[3]);     // lane: sample lane%16, rows 4 (lane/16) + e of A
                }
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    const int mt = wave + 4 * mi;
                    f32x4 sg, th;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { float s_, t_; act_pair(acc[mi][e] + b0v[mi][e], s_, t_); sg[e] = s_; th[e] = t_; }
                    th0[mi] = th; u0k[mi] = sg;
                    if (mt < KBM) L4[(mp.lUF >> 2) + mt * 64 + lane] = make_float4(sg[0], sg[1], sg[2], sg[3]);
                    if (recEv >= 0 && mt < KBM && 16 * mt + 4 * slot + 3 < pl.m && row0 + (lane & 15) < ra.n) {      // activation record: u0, tanh(o)
                        *reinterpret_cast<float4*>(recB + (recL + 16u * mt)) = make_float4(sg[0], sg[1], sg[2], sg[3]);
                        *reinterpret_cast<float4*>(recB + recSec + (recL + 16u * mt)) = make_float4(th[0], th[1], th[2], th[3]);
                    }
                }
                __syncthreads();
                TL(c, 2);
                // ================= P2: q = K1 u0 + b1 ; v = tanh(q) . w   (final time: also w . u_1 for Phi) =================
                mono_gemm<MT, KBM, true>(W2, (mp.lUF >> 2) + lane, acc);
                TL(c, 3);
                float pr = 0.f;
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    const int mt = wave + 4 * mi;
                    float4 v;
                    float vv[4], tq[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float q = acc[mi][e] + b1v[mi][e];
                        tq[e] = tanh_fast(q);
                        vv[e] = tq[e] * wv[mi][e];
                        if (fin) pr += wv[mi][e] * (u0k[mi][e] + hN * sigma_act(q));          // src/Phi.py:91-96
                    }
                    v = make_float4(vv[0], vv[1], vv[2], vv[3]);
                    if (mt < KBM) L4[(mp.lVF >> 2) + mt * 64 + lane] = v;
                    if (recEv >= 0 && mt < KBM && 16 * mt + 4 * slot + 3 < pl.m && row0 + (lane & 15) < ra.n)            // activation record: tanh(q)
                        *reinterpret_cast<float4*>(recB + 2 * recSec + (recL + 16u * mt)) = make_float4(tq[0], tq[1], tq[2], tq[3]);
                }
                if (fin) {
                    pr += __shfl_xor(pr, 16); pr += __shfl_xor(pr, 32);
                    if (lane < 16) lds[mp.lPHIP + wave * 16 + lane] = pr;
                }
                __syncthreads();
                TL(c, 4);
                // z = A s per sample (rows of the physics view): the fixed-order sum of the waves' partials
                {
                    const int s_ = tid >> 4, row = tid & 15;
                    const float* zp = lds + mp.lZP + ((row >> 2) * 16 + s_) * 4 + (row & 3);
                    lds[pl.lZQ + s_ * ZQLD + row] = ((zp[0] + zp[256]) + zp[512]) + zp[768];
                }
                // ================= P3: a = w + hN K1^T v ; y = tanh(o) . a =================
                mono_gemm<MT, KBM, true>(W3, (mp.lVF >> 2) + lane, acc);
                TL(c, 5);
#pragma unroll
                for (int mi = 0; mi < MT; ++mi) {
                    const int mt = wave + 4 * mi;
                    const float4 a4 = make_float4(wv[mi][0] + hN * acc[mi][0], wv[mi][1] + hN * acc[mi][1], wv[mi][2] + hN * acc[mi][2], wv[mi][3] + hN * acc[mi][3]);
                    float4 y;
                    y.x = th0[mi][0] * a4.x; y.y = th0[mi][1] * a4.y;
                    y.z = th0[mi][2] * a4.z; y.w = th0[mi][3] * a4.w;
                    if (mt < KBM) L4[(mp.lUF >> 2) + mt * 64 + lane] = y;              // u0 is dead: every wave is past the barrier behind P2
                    if (recEv >= 0 && mt < KBM && 16 * mt + 4 * slot + 3 < pl.m && row0 + (lane & 15) < ra.n)            // activation record: a = w + hN K1' v
                        *reinterpret_cast<float4*>(recB + 3 * recSec + (recL + 16u * mt)) = a4;
                }
                __syncthreads();
                TL(c, 6);
                // ================= P4: g = K0^T y + A^T z + c, the contraction over the hidden units split over the waves =================
                {
                    // this wave's share: hidden k-blocks wave, wave+4, ... ; wave 0 adds the low-rank term (k = rows of A, one block)
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
                            bf[mi] = L4[(mp.lUF >> 2) + (kb < KBM ? kb : 0) * 64 + lane];
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
                __syncthreads();
                TL(c, 7);
                // (singlequad's stage evaluations read the partials themselves; HOLD with intermediates: ctrl_write reads the held p[9..11] from the rows)
                const bool g_rows = !quad1 || fin || st >= nstage || (HOLD && ra.zFull);
                if (g_rows)
                for (int f = tid; f < KBD * 64; f += 256) {        // fixed-order sum of the four waves' partials, + c, into the gradient rows
                    const int l = f & 63, dt = f >> 6;
                    const float4 p0 = L4[(mp.lGP >> 2) + (dt * 4 + 0) * 64 + l], p1 = L4[(mp.lGP >> 2) + (dt * 4 + 1) * 64 + l];
                    const float4 p2 = L4[(mp.lGP >> 2) + (dt * 4 + 2) * 64 + l], p3 = L4[(mp.lGP >> 2) + (dt * 4 + 3) * 64 + l];
                    const float4 c4 = L4[(mp.lCW >> 2) + dt * 4 + (l >> 4)];
                    float4 gsum;
                    gsum.x = (((p0.x + p1.x) + p2.x) + p3.x) + c4.x; gsum.y = (((p0.y + p1.y) + p2.y) + p3.y) + c4.y;
                    gsum.z = (((p0.z + p1.z) + p2.z) + p3.z) + c4.z; gsum.w = (((p0.w + p1.w) + p2.w) + p3.w) + c4.w;
                    *reinterpret_cast<float4*>(lds + pl.lG + (l & 15) * GLD + 16 * dt + 4 * (l >> 4)) = gsum;
                }
                if (fin && tid < T) {
                    // Phi at the final time: w.u_1 (wave partials, fixed order) + 1/2 |A s|^2 + c.s + cb
                    const int s_ = tid;
                    float ph = ((lds[mp.lPHIP + s_] + lds[mp.lPHIP + 16 + s_]) + lds[mp.lPHIP + 32 + s_]) + lds[mp.lPHIP + 48 + s_];
                    float qd = 0.f;
                    for (int q = 0; q < r; ++q) { const float z = lds[pl.lZQ + s_ * ZQLD + q]; qd += 0.5f * z * z; }
                    float lin = 0.f;
                    for (int i = 0; i < D1; ++i) lin += lds[mp.lCW + i] * SB[s_ * LDs + i];
                    lds[pl.lPHI + s_] = ph + qd + lin + pl.cb;
                }
                if (g_rows) __syncthreads();
                if (recEv >= 0 && g_rows) {                                        // activation record: grad Phi from the gradient rows
                    float* gdst = ra.act + 4 * ra.actRows * pl.m + (recEv * ra.n + row0) * D1;
                    for (int jx = tid; jx < T * D1; jx += 256) {
                        const int t = jx / D1, i = jx - t * D1;
                        if (row0 + t < ra.n) gdst[t * D1 + i] = lds[pl.lG + t * GLD + i];
                    }
                }
                if (fin) break;
            }

            TL(c, 8);
            // ================= one quadcopter per sample (singlequad): physics + RK wave-locally, 16 lanes per sample =================
            // Quadcopter.py:65-113 for N = 1 restated so that no workgroup barrier and no serial per-sample loop is left: the 16
            // lanes of a sample read x and p (broadcast LDS reads, all issued before the first use), lanes 0..2 take the three
            // sin/cos pairs, every lane forms the scalars (same operation order as physics_finish) and lane j advances component
            // j of z = [x (12) | L | |dPhi/dt - H| | Q | W] (d + 4 = 16).
            if (quad1) {
                const int s_ = tid >> 4, j = tid & 15;
                float xv[12], pv[16];
#pragma unroll
                for (int q = 0; q < 3; ++q) {                                  // x from the stage-state fragments
                    const float4 x4 = L4[(mp.lSF >> 2) + q * 16 + s_];
                    xv[4 * q] = x4.x; xv[4 * q + 1] = x4.y; xv[4 * q + 2] = x4.z; xv[4 * q + 3] = x4.w;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {                                  // p = the four waves' P4 partials (fixed order) + c
                    const float4 p0 = L4[(mp.lGP >> 2) + q * 16 + s_], p1 = L4[(mp.lGP >> 2) + 64 + q * 16 + s_];
                    const float4 p2 = L4[(mp.lGP >> 2) + 128 + q * 16 + s_], p3 = L4[(mp.lGP >> 2) + 192 + q * 16 + s_];
                    const float4 c4 = L4[(mp.lCW >> 2) + q];
                    pv[4 * q] = (((p0.x + p1.x) + p2.x) + p3.x) + c4.x; pv[4 * q + 1] = (((p0.y + p1.y) + p2.y) + p3.y) + c4.y;
                    pv[4 * q + 2] = (((p0.z + p1.z) + p2.z) + p3.z) + c4.z; pv[4 * q + 3] = (((p0.w + p1.w) + p2.w) + p3.w) + c4.w;
                    if (recEv >= 0 && j == q && row0 + s_ < ra.n) {            // activation record: grad Phi (lane q of the sample: entries 4 q .. 4 q + 3)
                        float* gb = ra.act + 4 * recSec + (recEv * ra.n + row0) * D1;
                        const unsigned go = (unsigned)s_ * (unsigned)D1 + 4u * q;
#pragma unroll
                        for (int e = 0; e < 4; ++e) if (4 * q + e < D1) gb[go + e] = pv[4 * q + e];
                    }
                }
                TL(c, 9);
                float* TR = lds + pl.lTRIG + s_ * 6;
                if (j < 3) { float sn, cs; mono_sincos(j == 0 ? xv[3] : (j == 1 ? xv[4] : xv[5]), sn, cs); TR[j] = sn; TR[3 + j] = cs; }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");           // same wave, in-order LDS: the six values are there for its reads
                __builtin_amdgcn_wave_barrier();
                const float sps = TR[0], sth = TR[1], sph = TR[2], cps = TR[3], cth = TR[4], cph = TR[5];
                TL(c, 10);
                const float mass = (float)pb.mass, grav = (float)pb.grav;
                const float f7 = sps * sph + cps * sth * cph;
                const float f8 = -cps * sph + sps * sth * cph;
                const float f9 = cth * cph;
                const float fsum = f7 * pv[6] + f8 * pv[7] + f9 * pv[8];
                float u = (float)(-1.0 / (2.0 * pb.mass)) * fsum;
                if constexpr (HOLD) { if (held) u = uh; else uh = u; }        // (the thrust of the sampling instant; f7..f9 above are the current angles')
                const float sq = pv[9] * pv[9] + pv[10] * pv[10] + pv[11] * pv[11];
                float Lg = (float)pb.alphQ * 0.f;                              // Quadcopter.py:116-122: no obstacle implemented; one craft: W = 0
                Lg = Lg + 2.f + u * u + 0.25f * sq;
                const float s1 = xv[6] * pv[0] + xv[7] * pv[1] + xv[8] * pv[2];
                const float s2 = xv[9] * pv[3] + xv[10] * pv[4] + xv[11] * pv[5];
                const float um = u / mass;
                const float H = 0.f - Lg - s1 - s2 - um * fsum + grav * pv[8] + 0.5f * sq;
                if (j == 0) lds[pl.lSC + s_] = u;                              // thrust, for calcCtrls
                if (st < nstage) {
                    double tnext;
                    if (nstage == 1) tnext = t1k;
                    else tnext = (st < 2) ? (tk + hsd / 2) : (st == 2 ? (tk + hsd) : t1k);
                    const bool last = (st == nstage - 1);
                    if (last && ra.zFull && !HOLD) tnext = t1k - sg_h;
                    // (selects over named registers: a lane-indexed xv[6 + j] would become a loop over the lanes' distinct indices;
                    // every candidate is formed first so that the choice compiles to v_cndmask, not to a ladder of branches)
                    const float xsel = j == 0 ? xv[6] : j == 1 ? xv[7] : j == 2 ? xv[8] : j == 3 ? xv[9] : j == 4 ? xv[10] : xv[11];
                    const float psel = -0.5f * (j == 9 ? pv[9] : (j == 10 ? pv[10] : pv[11]));
                    const float f7u = um * f7, f8u = um * f8, f9u = um * f9 - grav;
                    const float fsel = j == 6 ? f7u : (j == 7 ? f8u : f9u);
                    const float hj = HOLD ? 0.f : fabsf(pv[12] - H);          // (a held control has no HJB residual)
                    float dzi = 0.f;                                           // Q, W
                    dzi = (j == 13) ? hj : dzi;
                    dzi = (j == 12) ? Lg : dzi;
                    dzi = (j >= 9 && j < 12) ? psel : dzi;
                    dzi = (j >= 6 && j < 9) ? fsel : dzi;
                    dzi = (j < 6) ? xsel : dzi;
                    // stepRK4 / stepRK1 (src/OCflow.py:143-184) as weights; this lane's component of z stays in two registers
                    const float K = hs * dzi;
                    const float rk_wa = (nstage == 1) ? 1.f : ((st == 0 || st == 3) ? c16 : c26);
                    const float rk_wx = (st < 2) ? 0.5f : 1.f;
                    float xs_;
                    if (last) {
                        xs_ = (nstage == 1 ? qz0 : qzA) + rk_wa * K;
                        if constexpr (DIST == 3) {
                            if (j < d && row0 + s_ < ra.n)
                                wcar[0] = noise_corr_value(ra.nzScale[j], ra.nzScale1[j], ra.nzRho[j], wcar[0], ra.nzSeed, ra.nzRow0 + row0 + s_, k, j);
                            xs_ += wcar[0];                                    // (j >= 12 and rows past n: 0 for the whole rollout)
                        }
                        else if constexpr (DIST == 2) xs_ += (j < d && row0 + s_ < ra.n) ? noise_value(ra.nzScale[j], ra.nzSeed, ra.nzRow0 + row0 + s_, k, j) : 0.f;
                        else if constexpr (DIST == 1) xs_ += wpre[0];          // (j >= 12: 0)
                        qz0 = xs_;
                    }
                    else { qzA = (st == 0 ? qz0 : qzA) + rk_wa * K; xs_ = qz0 + rk_wx * K; }
                    const float tn = (float)tnext;
                    __builtin_amdgcn_wave_barrier();                           // every lane of the sample has read x before it is overwritten
                    if (j <= 12) SB[s_ * LDs + j] = (j < 12) ? xs_ : tn;       // (d = 12: the time entry is component 12 of the row)
                    // ... and the next evaluation's stage-state fragment: entry j of sample s_ ([x | t | 0 0 0])
                    lds[mp.lSF + ((j >> 2) * 16 + s_) * 4 + (j & 3)] = (j < 12) ? xs_ : (j == 12 ? tn : 0.f);
                    sf_ready = true;
                    if (last && ra.zFull && row0 + s_ < ra.n) ra.zFull[((sg_slot + k + 1) * ra.n + row0 + s_) * (d + 4) + j] = xs_;
                    if constexpr (HOLD) {
                        if (last && ra.zFull) {                                // the control applied over step k: the held thrust (SC) and -p[9..11] / 2 (Gl)
                            __syncthreads();
                            ctrl_write(c, pl, pb, ra.ctrlFull + (sg_slot + k + 1) * ra.n * ra.cdim, row0, ra.n, ra.cdim);
                        }
                    }
                } else {
                    __syncthreads();
                    ctrl_write(c, pl, pb, ra.ctrlFull + (sg_slot + k + 1) * ra.n * ra.cdim, row0, ra.n, ra.cdim);
                    if (tid < T) SB[tid * LDs + d] = (float)t1k;
                }
                TL(c, 11);
                __syncthreads();
                TL(c, 12);
                continue;
            }
            // ================= physics + RK for the 16 samples (src/OCflow.py:104-184; same device functions as the tile kernel) =================
            physics_sums(c, pl, pb);                           // ends with a barrier
            TL(c, 9);
            if (st < nstage) {
                double tnext;
                if (nstage == 1) tnext = t1k;
                else tnext = (st < 2) ? (tk + hsd / 2) : (st == 2 ? (tk + hsd) : t1k);
                const bool last = (st == nstage - 1);
                if (last && ra.zFull && !HOLD) tnext = t1k - sg_h;      // with intermediates the next evaluation is the control at (z_{k+1}, (tk+h)-h)
                if (tid < T) {
                    const int s_ = tid;
                    const Costs cs = physics_finish(c, pl, pb, s_);          // quadcopter: also -grad_p H -> DZ rows, thrusts -> SC
                    DZ[s_ * ZLD + d] = cs.L;
                    DZ[s_ * ZLD + d + 1] = HOLD ? 0.f : fabsf(Gl[s_ * GLD + d] - cs.H);
                    DZ[s_ * ZLD + d + 2] = cs.Q;
                    DZ[s_ * ZLD + d + 3] = cs.W;
                }
                __syncthreads();
                TL(c, 10);
                int it = 0;
                for (int j = tid; j < T * (d + 4); j += 256) {
                    const int t = j / (d + 4), i = j - t * (d + 4);
                    const float dzi = (i < d && !quad) ? -Gl[t * GLD + i] : DZ[t * ZLD + i];      // point agents: dx = -p
                    const float K = hs * dzi;
                    const float z0 = Z0[t * ZLD + i];
                    float xs;
                    if (nstage == 1) { xs = z0 + K; Z0[t * ZLD + i] = xs; }
                    else if (st == 0) { ZA[t * ZLD + i] = z0 + c16 * K; xs = z0 + 0.5f * K; }
                    else if (st == 1) { ZA[t * ZLD + i] += c26 * K; xs = z0 + 0.5f * K; }
                    else if (st == 2) { ZA[t * ZLD + i] += c26 * K; xs = z0 + K; }
                    else { xs = ZA[t * ZLD + i] + c16 * K; Z0[t * ZLD + i] = xs; }
                    if constexpr (DIST) {
                        if (last) {
                            float w = 0.f;
                            if constexpr (DIST == 3) {
                                // (trip `it` of the sweep is the same (t, i) in every step: its w_{k-1} is wcar[it], selected like wpre)
                                if (i < d && row0 + t < ra.n) {
                                    float wp = 0.f;
#pragma unroll
                                    for (int q = 0; q < NDW; ++q) wp = (it == q) ? wcar[q] : wp;
                                    w = noise_corr_value(ra.nzScale[i], ra.nzScale1[i], ra.nzRho[i], wp, ra.nzSeed, ra.nzRow0 + row0 + t, k, i);
#pragma unroll
                                    for (int q = 0; q < NDW; ++q) wcar[q] = (it == q) ? w : wcar[q];
                                }
                            } else if constexpr (DIST == 2) {
                                if (i < d && row0 + t < ra.n) w = noise_value(ra.nzScale[i], ra.nzSeed, ra.nzRow0 + row0 + t, k, i);
                            } else {
#pragma unroll
                                for (int q = 0; q < NDW; ++q) w = (it == q) ? wpre[q] : w;
                            }
                            xs += w;
                            Z0[t * ZLD + i] = xs;
                        }
                        ++it;
                    }
                    if (i < d) SB[t * LDs + i] = xs;
                    if (last && ra.zFull && row0 + t < ra.n) ra.zFull[((sg_slot + k + 1) * ra.n + row0 + t) * (d + 4) + i] = xs;
                }
                if (tid < T) SB[tid * LDs + d] = (float)tnext;
                if constexpr (HOLD) {                          // the control applied over step k: the held -p of the gradient rows
                    if (last && ra.zFull) ctrl_write(c, pl, pb, ra.ctrlFull + (sg_slot + k + 1) * ra.n * ra.cdim, row0, ra.n, ra.cdim);
                }
            } else {
                if (quad && tid < T) (void)physics_finish(c, pl, pb, tid);         // thrusts for calcCtrls
                if (quad) __syncthreads();
                ctrl_write(c, pl, pb, ra.ctrlFull + (sg_slot + k + 1) * ra.n * ra.cdim, row0, ra.n, ra.cdim);
                if (tid < T) SB[tid * LDs + d] = (float)t1k;
            }
            TL(c, 11);
            __syncthreads();
            TL(c, 12);
        }
        tk += sg_h;
    }
    if (quad1) { Z0[(tid >> 4) * ZLD + (tid & 15)] = qz0; __syncthreads(); }      // the RK state returns from its registers

    // ---- terminal costs (src/OCflow.py:58-76)
    {
        const int Gsz = 256 / T;
        const int t = tid / Gsz, j0 = tid - t * Gsz;
        const float* gg = Gl + t * GLD;
        float v[2] = {0.f, 0.f};
        for (int i = j0; i < d; i += Gsz) {
            const float res = Z0[t * ZLD + i] - pb.xtarget[i];
            v[0] += res * res;
            v[1] += fabsf(gg[i] - ra.a0 * res);
        }
        group_reduce<2>(c, pl, v);
        if (tid < T && row0 + tid < ra.n) {
            const int s_ = tid;
            const long row = row0 + s_;
            const float cG = 0.5f * group_total<2>(c, pl, s_, 0);
            const float* z = Z0 + s_ * ZLD;
            if (ra.persample) {
                float* op = ra.persample + row * 7;
                op[0] = z[d]; op[1] = cG; op[2] = z[d + 1];
                op[3] = fabsf(lds[pl.lPHI + s_] - ra.a0 * cG);
                op[4] = group_total<2>(c, pl, s_, 1);
                op[5] = z[d + 2]; op[6] = z[d + 3];
            }
        }
        if (ra.z_out)
            for (int tt = 0; tt < T; ++tt)
                if (row0 + tt < ra.n)
                    for (int i = tid; i < d + 4; i += 256) ra.z_out[(row0 + tt) * (d + 4) + i] = Z0[tt * ZLD + i];
    }
}
