// nocf_noise.inc -- the counter-based Brownian disturbance (DESIGN.md section 3.10): entry (row, k, i) of the disturbance is a pure function
// of (seed, GLOBAL row, step, component), so a row meets the same noise alone, in any batch, on any rank and in any chunk, and no tensor
// W [nt][n][d] has to exist.  Included by nocf_kernels.hip in front of the three rollout kernels (the DIST == 2 instantiations read
// RollArgs::nzScale / nzSeed / nzRow0, nocf_dev.h); noise_words is host code too (nocf_debug_noise_words).  DIST == 3 chains these entries
// into a time-correlated path per (row, component): noise_corr_next / noise_corr_value below (section 3.18).
//
//   words   Philox4x32-10, counter (row lo, row hi, k, i), key (seed lo, seed hi)
//   u1, u2  ((w >> 9) + 0.5) 2^-23 of words 0 and 1: exact in fp32, inside [2^-24, 1 - 2^-24]
//   g       sqrtf(-2 logf(u1)) cospif(2 u2)            (Box-Muller, the accurate library functions; |g| <= 5.77)
//   value   fl(scale[i] * g), rounded on its own and THEN added to the state by the caller's +=

__host__ __device__ __forceinline__ void noise_words(unsigned long long seed, long long row, int k, int i, unsigned int out[4]) {
    const unsigned int M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    unsigned int c0 = (unsigned int)((unsigned long long)row & 0xffffffffull), c1 = (unsigned int)((unsigned long long)row >> 32);
    unsigned int c2 = (unsigned int)k, c3 = (unsigned int)i;
    unsigned int k0 = (unsigned int)(seed & 0xffffffffull), k1 = (unsigned int)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)M0 * c0, p1 = (unsigned long long)M1 * c2;
        const unsigned int n0 = (unsigned int)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned int)p1;
        const unsigned int n2 = (unsigned int)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned int)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The value is the same bits wherever it is formed (the fill kernel, the three rollout kernels): the uniforms enter and the product leaves
// through an empty asm, so nothing of the caller's arithmetic can be merged into the transform -- in particular the product cannot contract
// into an fma with the state it is added to (__fmul_rn is a plain multiplication to this compiler).
__device__ __forceinline__ float noise_value(float scale, unsigned long long seed, long long row, int k, int i) {
    unsigned int w[4];
    noise_words(seed, row, k, i, w);
    float u1 = ((float)(w[0] >> 9) + 0.5f) * 1.1920928955078125e-07f;       // 2^-23
    float u2 = ((float)(w[1] >> 9) + 0.5f) * 1.1920928955078125e-07f;
    asm volatile("" : "+v"(u1), "+v"(u2));
    float g = sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
    asm volatile("" : "+v"(g));
    float v = __fmul_rn(scale, g);
    asm volatile("" : "+v"(v));
    return v;
}

// Time-correlated (AR(1) / Ornstein-Uhlenbeck) noise, DIST == 3 (DESIGN.md section 3.18): per component i, rho_i in [0, 1),
//   w_0 = noise_value(s0_i, seed, row, 0, i)                                        s0_i = fp32(sigma_i sqrt(h))
//   w_k = fl(fl(rho_i w_{k-1}) + noise_value(s1_i, seed, row, k, i))    k >= 1      s1_i = fp32(sigma_i sqrt(h) sqrt(1 - rho_i^2))
// so every w_k has the white entry's variance and corr(w_k, w_{k+j}) = rho_i^j.  Two roundings, never an fma: the product and the sum each
// leave through an empty asm (noise_value's fence), so neither can merge with the other or with the caller's +=, and numpy float32
// arithmetic restates the path bit for bit.  The carried w_{k-1} stays with the thread that forms the component's entry (a register on the
// lane and one-CU kernels, an LDS slot of its own on the per-tile kernel); s0 is RollArgs::nzScale, s1 and rho are RollArgs::nzScale1 / nzRho.
__device__ __forceinline__ float noise_corr_next(float rho, float wprev, float v) {
    float p = __fmul_rn(rho, wprev);
    asm volatile("" : "+v"(p));
    float w = __fadd_rn(p, v);
    asm volatile("" : "+v"(w));
    return w;
}

// entry k of the path of (row, i), given entry k - 1 (ignored at k == 0)
__device__ __forceinline__ float noise_corr_value(float s0, float s1, float rho, float wprev, unsigned long long seed, long long row, int k, int i) {
    const float v = noise_value(k == 0 ? s0 : s1, seed, row, k, i);
    const float w = noise_corr_next(rho, wprev, v);
    return k == 0 ? v : w;
}

// Noisy ENSEMBLES (nocf_rollout_noisy_ensemble_f32 / nocf_rollout_noisy_mid_ensemble_f32, DESIGN.md section 3.14): every member under its own
// level and seed -- scale [E, d] (member e's fp32 sigma_i sqrt(h)) and seeds [E], device tables.  The LAST argument of the lane and the one-CU
// rollout kernels, behind EnsArgs / MonoEnsArgs and for their reason (the offsets of the arguments in front of it stay where they are), and
// read by the ENS instantiations with DIST == 2 alone.  The key of a row is RollArgs::nzRow0 + the row INSIDE its member
// ws (the struct's last word, so nothing in front of it moves): read by the ENS instantiations with DIST == 1 alone
// (nocf_rollout_disturbed_ensemble_f32 / nocf_rollout_disturbed_mid_ensemble_f32, DESIGN.md section 3.17) -- the member stride of the tensor
// disturbance RollArgs::dist in floats, nt n d for W [E, nt, n, d] or 0 for one [nt, n, d] that every member meets
struct EnsNoiseArgs { const float* scale; const unsigned long long* seeds; long ws; };

// W[k][row][i] = noise_value(scale[i], seed, row0 + row, k, i): one thread per element, rows < n and d floats per row only
__global__ void __launch_bounds__(256) noise_fill_kernel(float* __restrict__ W, long n, int nt, int d, const float* __restrict__ scale,
                                                         unsigned long long seed, long row0) {
    const long per = n * d, total = per * nt;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        const long k = e / per, rem = e - k * per;
        const long row = rem / d;
        const int i = (int)(rem - row * d);
        W[e] = noise_value(scale[i], seed, row0 + row, (int)k, i);
    }
}

// W[k][row][i] = entry k of the correlated path of (row0 + row, i): one thread per (row, i) walks k, so for every k the stores of
// neighbouring threads are neighbours in W
__global__ void __launch_bounds__(256) noise_fill_corr_kernel(float* __restrict__ W, long n, int nt, int d, const float* __restrict__ scale0,
                                                              const float* __restrict__ scale1, const float* __restrict__ rho,
                                                              unsigned long long seed, long row0) {
    const long per = n * d;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < per; e += (long)gridDim.x * 256) {
        const long row = e / d;
        const int i = (int)(e - row * d);
        const float s0 = scale0[i], s1 = scale1[i], r = rho[i];
        float w = 0.f;
        for (int k = 0; k < nt; ++k) {
            w = noise_corr_value(s0, s1, r, w, seed, row0 + row, k, i);
            W[(long)k * per + e] = w;
        }
    }
}
