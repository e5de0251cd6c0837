/*
 * nocf.h -- C ABI of libnocf.so: the MI355X (gfx950) OCflow rollout hot path.
 *
 * The reference (donken/NeuralOC) is pure Python and has no FFI; this header is the
 * boundary a maintainer binds with ctypes (stub in INTEGRATION.md).  Each entry point
 * names the reference interface it replaces (file:line into donken/NeuralOC).
 *
 * Conventions
 *   - every pointer marked "device" is a HIP device pointer on the current device;
 *     all tensors are dense row-major fp32 unless stated otherwise
 *   - functions enqueue work on `stream` (a hipStream_t passed as void*, 0 = default
 *     stream) and return without synchronising; nothing is allocated or freed -- with ONE opt-in exception since version 113: with
 *     NOCF_LANE_ONE=1 in the environment the first rollout of a small network (m <= 32: one wavefront per sample) on a device allocates
 *     256 bytes of device memory for the life of the process: the self-resetting ticket words (one per stream, at most 64) with which that
 *     kernel's last workgroup forms the cost sums itself instead of a second launch (measured slower on the MI355X: off by default)
 *   - return value: 0 ok; <0 argument error (NOCF_E_*); >0 a hipError_t
 *   - no exceptions, no aborts.  Process-global state: the diagnostic environment knobs (NOCF_LANE, NOCF_FIXED, NOCF_DUO,
 *     NOCF_MONO, NOCF_DEBUG ...) are read from the environment once, at first use, and cached (nocf_debug_reload_env drops the
 *     cache); the measurement hooks nocf_profile_begin/_end, nocf_last_rollout_kernel, nocf_last_rollout_status_async and
 *     nocf_debug_set_* keep a list of HIP events / the last launch's name and error-word address / a diagnostic buffer pointer
 *     and are NOT thread-safe.  The compute entry points themselves keep no state between calls (the caller owns the workspace)
 */
#ifndef NOCF_H
#define NOCF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NOCF_VERSION 113            /* major*100 + minor */

#define NOCF_E_NULL      (-1)       /* required pointer is NULL                     */
#define NOCF_E_SHAPE     (-2)       /* d/m/nTh/n/nt out of the supported range      */
#define NOCF_E_PROB      (-3)       /* unknown problem kind / obstacle combination  */
#define NOCF_E_WORKSPACE (-4)       /* workspace too small (see nocf_workspace_bytes) */
#define NOCF_E_STEPPER   (-5)       /* stepper is neither NOCF_RK4 nor NOCF_RK1     */
#define NOCF_E_LDS       (-6)       /* network too deep/wide for the 160 KiB LDS plan */

/* stepper, src/OCflow.py:46-49 ("rk4" / "rk1") */
#define NOCF_RK4 4
#define NOCF_RK1 1

/* problem classes, src/problem/{Cross2D,SwarmTraj,Quadcopter}.py */
#define NOCF_PROB_CROSS2D    0
#define NOCF_PROB_SWARMTRAJ  1
#define NOCF_PROB_QUADCOPTER 2

/* obstacle strings of the problem constructors */
#define NOCF_OBS_NONE         0
#define NOCF_OBS_SOFTCORRIDOR 1    /* Cross2D.py:43-48   */
#define NOCF_OBS_HARDCORRIDOR 2    /* Cross2D.py:49-52   */
#define NOCF_OBS_BLOCKS       3    /* SwarmTraj.py:46-50 */

/* The value network Phi (src/Phi.py:57-87).  Pointers are the tensors of the reference
 * state_dict, unmodified: N.layers.0.weight, N.layers.0.bias, N.layers.{1..nTh-1}.weight
 * stacked, ...bias stacked, w.weight, A, c.weight; cb = c.bias[0]. */
typedef struct NocfPhi {
    int32_t d;          /* space dimension; inputs are (x,t) in R^{d+1}              */
    int32_t m;          /* hidden width                                               */
    int32_t nTh;        /* number of ResNet layers, >= 2 (src/Phi.py:25-27)           */
    int32_t r;          /* rows of A = min(10, d+1) (src/Phi.py:75)                   */
    const float* K0;    /* device [m, d+1]                                            */
    const float* b0;    /* device [m]                                                 */
    const float* K;     /* device [nTh-1, m, m]                                       */
    const float* b;     /* device [nTh-1, m]                                          */
    const float* w;     /* device [m]                                                 */
    const float* A;     /* device [r, d+1]                                            */
    const float* cw;    /* device [d+1]                                               */
    float cb;           /* c.bias as a host value (used when cb_dev is NULL)          */
    const float* cb_dev;/* optional: device address of c.bias; when set the kernels   */
                        /* read the bias there and the caller needs no device-to-host */
                        /* copy (a synchronisation per call) to fill `cb`             */
} NocfPhi;

/* One problem object (the attributes the reference's calcLHQW/calcGradpH/calcCtrls read). */
typedef struct NocfProb {
    int32_t kind;       /* NOCF_PROB_*                                                */
    int32_t obstacle;   /* NOCF_OBS_*                                                 */
    int32_t n_agents;   /* d / agentDim                                               */
    int32_t training;   /* prob.training: masks and thresholds differ */
    /* Python-side floats are doubles; the kernels derive their fp32 constants from these the
     * way torch does when a Python scalar meets an fp32 tensor (thresholds such as 3.2*r or
     * 2.0+r are formed in double, then rounded once). */
    double r;           /* agent radius                                               */
    double alph_Q;
    double alph_W;
    double mass;        /* Quadcopter only                                            */
    double grav;        /* Quadcopter only                                            */
    const float* xtarget; /* device [d]                                               */
} NocfProb;

int nocf_version(void);

/* measurement hook: name of the rollout kernel the last nocf_rollout_f32 / nocf_rollout_record_f32 call of this process
 * launched ("rollout_duo_kernel", "rollout_mono_kernel", "rollout_kernel<shape-specialised>", "rollout_kernel<generic>",
 * "rollout_lane_kernel", or "none"); a static string, not thread-safe (bench.py labels its roofline with it) */
const char* nocf_last_rollout_kernel(void);

/* Asynchronous status of the last rollout / adjoint call on the calling thread's CURRENT DEVICE (per-call state is kept per device:
 * threads driving different GPUs do not see each other's; a backward that a framework runs on a worker thread shares the forward's).
 * The split-role kernels' workgroups wait for each other with bounded polls; when one times out
 * (the GPU was shared with another kernel, so that not all workgroups were resident) the kernel sets an error word, finishes, and
 * every output of the call -- persample rows, the cost sums, z_out, zFull, ctrlFull -- is turned into NaN on the stream (the training
 * tape and s_all are not: call nocf_poison_if_failed_f32 on what is derived from them).  This call enqueues a
 * 4-byte device-to-host copy of that word into `host_word` (pinned host memory) on `stream`; once the stream has reached it,
 * *host_word != 0 means the rollout failed (0x3000 + the exchange kind that timed out).  Returns 1 when a copy was enqueued, 0 when
 * the last rollout kernel has no such word (*host_word is set to 0), or an error code.  The Python layer raises RuntimeError from it. */
int nocf_last_rollout_status_async(uint32_t* host_word, void* stream);

/* The library reads its NOCF_* environment knobs once (first use) and caches them; this drops the cache so that the next call reads
 * the environment again (tests that switch kernels between calls; the Python layer calls it when NOCF_ENV_WATCH=1). */
void nocf_debug_reload_env(void);
/* Override one NOCF_* knob for THIS process's library instance (clear != 0: drop the override again).  Unlike the environment it is not
 * inherited by child processes (compiler children, self-launched ranks) and survives nocf_debug_reload_env: the in-process fallback of a
 * process that shares its GPU (neuraloc_amd/_lib.py: duo_guard) uses it to switch the weight-stationary kernels off. */
int nocf_set_knob(const char* name, int32_t value, int32_t clear);
/* The geometry the per-tile kernels (rollout_kernel / rollout_bwd_kernel) would run a shape with, under the NOCF_NWAVES / NOCF_SUBTILES knobs
 * in force: out = { T (samples per tile), waves per workgroup, MB, DB (64-column blocks of m and of d+1), KQ1, KQm (k-quads of the two
 * contraction lengths, padded to 8), SK1, SK6, SKm (split-K factors of the opening, closing and residual products), the split-K cap the LDS
 * carve ended on (8 or 4 unless LDS was short; 0: no cap fits), LDS floats per workgroup, and 1 / 2 when the plan is that of a
 * shape-specialised instantiation (2: one taken by the recording forward and the adjoint only), else 0 }.  bwd != 0: the adjoint's plan.
 * Returns 0 or the code the rollout would return (NOCF_E_SHAPE, NOCF_E_LDS: out[9] is still set, the rest 0).  Makes no GPU call. */
int nocf_debug_tile_plan(int32_t d, int32_t m, int32_t nTh, int32_t r, int32_t n_agents, int32_t bwd, int32_t out[12]);
/* The instantiation the double-precision kernels would run a shape with.  which: 0 nocf_rollout_f64 / nocf_rollout_record_f64, 1
 * nocf_rollout_bwd_f64 (under the NOCF_F64_BWD_T knob in force), 2 nocf_phi_f64 (n_agents is not used).  out = { T (samples per workgroup),
 * wide (m > 256), LDS doubles per workgroup, the form of the m x (d+1), m x m and (d+1) x m products (0 plain loop, 1 register-tiled two
 * rows per thread, 2 register-tiled one row per thread, 3 matrix pipe), matrix pipe: row groups per wave and passes at M = m, the same at
 * M = d+1 (0 otherwise), register-tiled two-row form: 512-row trips at M = m and at M = d+1 (0 otherwise) }.  Returns 0 or the code the
 * entry would return for these shapes (NOCF_E_SHAPE, NOCF_E_LDS: out is all 0).  Makes no GPU call.  Libraries older than this entry
 * lack the symbol: probe for it. */
int nocf_debug_f64_plan(int32_t d, int32_t m, int32_t nTh, int32_t r, int32_t n_agents, int64_t n, int32_t which, int32_t out[12]);

/* bytes of scratch `workspace` a call with these shapes needs (packed weight images) */
size_t nocf_workspace_bytes(int32_t d, int32_t m, int32_t nTh);

/* bytes a nocf_rollout_f32 call over n samples can use: >= nocf_workspace_bytes; the extra room holds the
 * activation-exchange buffers of the weight-sliced group kernel (without it the per-tile kernel runs) */
size_t nocf_rollout_workspace_bytes(int32_t d, int32_t m, int32_t nTh, int64_t n);

/* number of control components per sample: d (Cross2D, SwarmTraj) or 4*n_agents (Quadcopter) */
int nocf_ctrl_dim(const NocfProb* prob, int32_t d);

/*
 * OCflow -- replaces src/OCflow.py:7-95 (driver), :104-140 (ocOdefun), :143-184 (steppers)
 * together with Phi.getGrad (src/Phi.py:99-138), Phi.forward (:91-96) and the problem's
 * calcLHQW / calcGradpH / calcCtrls for every stage, fused into one launch.
 *
 *   x          device [n, d]          initial states (not modified)
 *   t0,t1,nt   tspan and number of steps; h=(t1-t0)/nt, times advance in double like the reference
 *   alph       host  [6]              only [0],[3],[4],[5] are used (SURVEY 8a note 7)
 *   z_out      device [n, d+4]        final z = [x(T) | L | HJt | Q | W]           (nullable)
 *   persample  device [n, 7]          per-sample [L, G, HJt, HJfin, HJgrad, Q, W] = the
 *                                     reference's noMean=True list, src/OCflow.py:66-76 (nullable)
 *   cost_sums  device [8]             sums over the n samples of the 7 columns above, then n.
 *                                     Deterministic (fixed-order, fp64-accumulated) reduction.
 *                                     The caller forms means / Jc (and all-reduces first when
 *                                     the batch is sharded over GPUs).                (nullable)
 *   zFull      device [nt+1, n, d+4]  intermediates=True: z after every step, slot 0 = z0.
 *                                     TIME-MAJOR; the reference's [n, d+4, nt+1] is the
 *                                     permute(1,2,0) view of it.                       (nullable)
 *   ctrlFull   device [nt+1, n, a]    controls, a = nocf_ctrl_dim(); slot 0 stays zero and slot
 *                                     k+1 uses (z_{k+1}, t_k) exactly like src/OCflow.py:51-55.
 *                                     Required iff zFull is given.
 */
int nocf_rollout_f32(const NocfPhi* phi, const NocfProb* prob,
                     const float* x, int64_t n,
                     double t0, double t1, int32_t nt, int32_t stepper,
                     const float* alph,
                     float* z_out, float* persample, float* cost_sums,
                     float* zFull, float* ctrlFull,
                     void* workspace, size_t workspace_bytes, void* stream);

/*
 * nocf_rollout_f32 that also forms the means: cost_means device [8] = the 7 batch means [L, G, HJt, HJfin, HJgrad, Q, W] and Jc
 * (src/OCflow.py:80-90; what nocf_cost_means_f32 computes from cost_sums, same arithmetic), written by the launch that reduces the
 * per-sample table -- for callers with no all-reduce between the sums and the means (one device, the whole batch): one launch less per call.
 * cost_means nullable; it needs cost_sums.
 */
int nocf_rollout_means_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n,
                           double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                           float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull,
                           void* workspace, size_t workspace_bytes, void* stream);

/*
 * nocf_rollout_means_f32 under per-step state disturbances: W device [nt, n, d], float32, time-major like zFull, contiguous, not modified.
 * With h, tk and the steppers of nocf_rollout_f32:
 *     z = [x, 0, 0, 0, 0]; for k in 0 .. nt-1: z = step(z, tk, tk + h); z[:, :d] += W[k]; (zFull[k+1] = z, ctrlFull[k+1] from grad Phi at
 *     the displaced state and the step's start time); tk += h
 * and the terminal terms at the displaced z(T): additive noise in the Euler-Maruyama position.  The four cost columns are not displaced;
 * W[nt-1] lands on the terminal state and nothing reacts to it.  W == 0 gives the undisturbed call's outputs on the same kernel.
 * Dispatch: the register-resident small-network kernel, then the one-CU kernel, then the per-tile kernel -- never the split-role kernel
 * (m = 512 networks run on the per-tile kernel here).  float32 only; an evaluation (nothing is recorded for an adjoint); no segments.
 * W == NULL: NOCF_E_NULL.  Every refusal returns before anything is enqueued.
 */
int nocf_rollout_disturbed_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, const float* W, int64_t n,
                               double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                               float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull,
                               void* workspace, size_t workspace_bytes, void* stream);

/*
 * The recording forward of training under per-step state disturbances: nocf_rollout_record_act_f32 (below) under the contract of
 * nocf_rollout_disturbed_f32 -- W device [nt, n, d], float32, time-major, contiguous, not modified; z = step(z, tk, tk + h);
 * z[:, :d] += W[k]; the terminal terms at the displaced z(T).  s_all [nt*nstage, n, d+1] receives the stage inputs of every RK evaluation:
 * the first stage of step k+1 is recorded at the DISPLACED state, and W[nt-1] lands on z_out, where the terminal block is evaluated.
 * W does not depend on the parameters, so the adjoint of the disturbed scheme is the adjoint of the undisturbed one at these recorded
 * inputs: s_all and z_out go to nocf_rollout_bwd_small_f32 / nocf_rollout_bwd_mid_f32 / nocf_rollout_bwd_act_f32 unchanged (they read
 * every stage input from s_all and the final state from z_out; none re-derives a state from the previous step).  These three do not form dJ/dW;
 * nocf_rollout_bwd_states_f32 (below) does, from the same s_all and z_out.
 * W == 0 gives nocf_rollout_record_act_f32's outputs on the same kernel.
 *   act_rec, recorded   as for nocf_rollout_record_act_f32: the one-CU kernel writes the activation record (recorded = 1), the lane and
 *                       per-tile kernels do not (recorded = 0; pass NULL for shapes the one-CU kernel does not take)
 * Dispatch: the register-resident small-network kernel, then the one-CU kernel, then the per-tile kernel -- never the split-role kernel
 * (m = 512 networks record on the per-tile kernel here, and their adjoint is nocf_rollout_bwd_act_f32 with a null record).  No tape.
 * float32 only; no segments.  W == NULL, s_all == NULL or z_out == NULL: NOCF_E_NULL.  Every refusal returns before anything is enqueued.
 */
int nocf_rollout_record_disturbed_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, const float* W, int64_t n,
                                      double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                      float* z_out, float* persample, float* cost_sums, float* s_all, float* act_rec, int32_t* recorded,
                                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * Brownian disturbances from a counter-based generator: the disturbance of (row, step k, component i) is a pure function
 *     w(seed, row, k, i) = fl32(scale[i] * g),   g = sqrtf(-2 logf(u1)) cospif(2 u2),   u = ((word >> 9) + 0.5) 2^-23 of words 0 and 1 of
 *     Philox4x32-10 with counter (row & 0xffffffff, row >> 32, k, i) and key (seed & 0xffffffff, seed >> 32)
 * (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85; words 2 and 3 are not used; |g| <= 5.77).  `row` is the
 * GLOBAL row: row0 + the row of this call.  A row meets the same disturbances alone, in any batch, on any device and in any chunk, and a
 * prefix in nt stays a prefix.  scale device [d], float32: sigma_i sqrt(h) with h = (t1 - t0) / nt, 0 for components that are not
 * disturbed.  The product is rounded to float32 on its own and then added to the state.
 *
 * nocf_noise_fill_f32 writes W[k][row][i] = w(seed, row0 + row, k, i), W device [nt, n, d], time-major, contiguous: the tensor that
 * nocf_rollout_disturbed_f32 takes.  Only rows < n and d floats per row are written.
 * W == NULL or scale == NULL: NOCF_E_NULL; n, nt or d < 1, or row0 < 0: NOCF_E_SHAPE.  Every refusal returns before anything is enqueued.
 */
int nocf_noise_fill_f32(float* W, int64_t n, int32_t nt, int32_t d, const float* scale, uint64_t seed, int64_t row0, void* stream);

/*
 * nocf_rollout_disturbed_f32 with the disturbances drawn inside the kernels: no W exists.  Same contract, dispatch, outputs and refusals;
 * the outputs equal, bit for bit, those of nocf_rollout_disturbed_f32 on the W that nocf_noise_fill_f32 writes for (scale, seed, row0).
 * nocf_last_rollout_kernel() reports "rollout_lane_kernel<noise>", "rollout_mono_kernel<noise>", "rollout_kernel<generic, noise>" or
 * "rollout_kernel<shape-specialised, noise>".  scale == NULL: NOCF_E_NULL; row0 < 0: NOCF_E_SHAPE.
 */
int nocf_rollout_noisy_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, const float* scale, uint64_t seed, int64_t row0,
                           int64_t n, double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                           float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull,
                           void* workspace, size_t workspace_bytes, void* stream);

/*
 * nocf_rollout_record_disturbed_f32 with the disturbances drawn inside the kernels: the recording forward of training under counter-based
 * noise.  s_all, z_out, persample and the activation record equal those of nocf_rollout_record_disturbed_f32 on the filled W bit for bit,
 * and go to the same adjoints.  scale == NULL, s_all == NULL or z_out == NULL: NOCF_E_NULL; row0 < 0: NOCF_E_SHAPE.
 */
int nocf_rollout_record_noisy_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, const float* scale, uint64_t seed, int64_t row0,
                                  int64_t n, double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                  float* z_out, float* persample, float* cost_sums, float* s_all, float* act_rec, int32_t* recorded,
                                  void* workspace, size_t workspace_bytes, void* stream);

/*
 * Time-correlated (AR(1) / Ornstein-Uhlenbeck) disturbances from the same generator.  With w(scale, seed, row, k, i) the white entry above,
 * component i of GLOBAL row `row` meets the path
 *     w_0 = w(scale0[i], seed, row, 0, i)
 *     w_k = fl32( fl32(rho[i] * w_{k-1}) + w(scale1[i], seed, row, k, i) )        k >= 1
 * -- two roundings, never an fma, fenced like the white product, so float32 arithmetic on the host restates it bit for bit.  Three device
 * tables [d], float32: rho[i] in [0, 1); scale0[i] = sigma_i sqrt(h); scale1[i] = sigma_i sqrt(h) sqrt(1 - rho_i^2) (formed in double, then
 * rounded; both 0 for a component that is not disturbed).  Then every w_k has the white entry's variance (a stationary start) and
 * corr(w_k, w_{k+j}) = rho_i^j; rho == 0 gives the white values (0 * w + v = v).  Row keys, row0 and the prefix property are the white
 * generator's: a row meets the same path alone, in any batch, on any device and in any chunk.  The carried w_{k-1} never leaves the kernel.
 * The values of rho are not checked here (the Python layer refuses rho outside [0, 1)); any finite table gives a defined path.
 *
 * nocf_noise_fill_corr_f32: nocf_noise_fill_f32 for the path, W[k][row][i] = w_k of (row0 + row, i).
 * nocf_rollout_noisy_corr_f32 / nocf_rollout_record_noisy_corr_f32: nocf_rollout_noisy_f32 / nocf_rollout_record_noisy_f32 with
 * (scale0, scale1, rho) where `scale` stands; every output equals, bit for bit, that of nocf_rollout_disturbed_f32 /
 * nocf_rollout_record_disturbed_f32 on the W that nocf_noise_fill_corr_f32 writes, and the recording forward goes to the same adjoints (W does
 * not depend on the parameters).  Same contract, dispatch (lane, one-CU, per-tile; never the split-role kernel) and refusals as the white
 * entries; a NULL table: NOCF_E_NULL.  On the per-tile kernel the carried values take T (d + 4) floats of LDS behind the plan's; a shape whose
 * plan leaves no room for them: NOCF_E_LDS.  Every refusal returns before anything is enqueued.  nocf_last_rollout_kernel() reports
 * "rollout_lane_kernel<noise-corr>", "rollout_mono_kernel<noise-corr>", "rollout_kernel<generic, noise-corr>" or
 * "rollout_kernel<shape-specialised, noise-corr>".  Single networks only; nocf_version() is unchanged: callers probe for the symbols.
 */
int nocf_noise_fill_corr_f32(float* W, int64_t n, int32_t nt, int32_t d, const float* scale0, const float* scale1, const float* rho,
                             uint64_t seed, int64_t row0, void* stream);
int nocf_rollout_noisy_corr_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, const float* scale0, const float* scale1,
                                const float* rho, uint64_t seed, int64_t row0,
                                int64_t n, double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull,
                                void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_record_noisy_corr_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, const float* scale0, const float* scale1,
                                       const float* rho, uint64_t seed, int64_t row0,
                                       int64_t n, double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                       float* z_out, float* persample, float* cost_sums, float* s_all, float* act_rec, int32_t* recorded,
                                       void* workspace, size_t workspace_bytes, void* stream);

/*
 * The zero-order-hold rollout: the control is sampled every hold-th step and applied, unchanged, until the next sample -- a deployed
 * controller's rate, where every other rollout re-evaluates the feedback law at every Runge-Kutta stage.  hold = K >= 1; W nullable, device
 * [nt, n, d], float32, time-major: exactly nocf_rollout_disturbed_f32's tensor; h, tk and the steppers are nocf_rollout_f32's.
 *     z = [x, 0, 0, 0, 0]
 *     for k in 0 .. nt-1:
 *         if k % K == 0:  c = calcCtrls(x_k, grad_x Phi(x_k, t_k))      the state the controller really meets: W[k-1] is already on it
 *         z = step(z) with the right-hand side  [ f(x, c) | L(x, c) | 0 | Q(x) | W(x) ]     RK4: four physics evaluations, c fixed; RK1: one
 *         if W: z[:, :d] += W[k]
 *         zFull[k+1] = z;  ctrlFull[k+1] = c                            the control APPLIED over step k (slot 0 stays zero)
 *     terminal block: unchanged, at z(T) (G, HJfin, HJgrad: one network evaluation)
 * Point agents (Cross2D, SwarmTraj): c = -p (d components), f = c, and L, Q, W are the reference's calcLHQW(x, p) at p = -c (the Cross2D /
 * SwarmTraj difference in where alph_Q sits included).  Quadcopter, one craft: c = (u, tau) = calcCtrls, 4 components, tau = -p[9:12] / 2;
 * f = [x[6:12], (u/m) f7(ang), (u/m) f8(ang), (u/m) f9(ang) - g, tau] with f7..f9 from the CURRENT angles; L = alph_Q Q + 2 + u^2 + |tau|^2
 * (the reference's 2 + u^2 + sq / 4); W = 0.  Every problem: the HJt column (persample[:, 2], z[:, d+1]) is identically 0 -- a held control
 * has no HJB residual.  persample [n, 7], cost_sums, cost_means and z_out keep their layouts.  K >= nt is the open-loop rollout of the
 * initial control; a K that does not divide nt leaves a short last interval.  The call makes ceil(nt / K) + 1 network evaluations where
 * nocf_rollout_f32 makes 4 nt + 1 (5 nt + 1 with zFull), and the same 4 nt physics evaluations.
 * Dispatch: the register-resident small-network kernel, then the one-CU kernel, with their existing eligibility tests; every other shape
 * (the per-tile and split-role families, nTh > 2, m > 128) and a quadcopter problem of more than one craft: NOCF_E_SHAPE.  hold < 1:
 * NOCF_E_SHAPE.  The null rules are nocf_rollout_disturbed_f32's, except that W may be NULL.  float32 only; an evaluation (nothing is
 * recorded for an adjoint); one network; no segments.  Every refusal returns before anything is enqueued.  nocf_last_rollout_kernel()
 * reports "rollout_lane_kernel<hold>" / "rollout_lane_kernel<hold,dist>" (with W) and "rollout_mono_kernel<hold>" /
 * "rollout_mono_kernel<hold,dist>".  nocf_version() is unchanged: callers probe for the symbol.
 */
int nocf_rollout_held_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, const float* W, int32_t hold, int64_t n,
                          double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                          float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull,
                          void* workspace, size_t workspace_bytes, void* stream);

/* host only: the four Philox words of (seed, row, k, i) as the kernels form them (no device is touched).  out == NULL: NOCF_E_NULL;
 * row, k or i < 0: NOCF_E_SHAPE. */
int nocf_debug_noise_words(uint64_t seed, int64_t row, int32_t k, int32_t i, uint32_t out[4]);

/*
 * Several rollouts that differ only in their start time and step count, in ONE launch (round 5): the second segments of a shock sweep.
 * The reference's shocked rollout (src/plotter.py:815-824, driven by evalOC.py:113-122) is OCflow on [0, t_s] with int(t_s nt) steps, the
 * shock added to the end state, and OCflow on [t_s, 1] with 1 + nt - int(t_s nt) steps; a sweep over shock times (BASELINE config 5) repeats
 * that per t_s.  Here rows [k * rows_per_seg, (k + 1) * rows_per_seg) of x are segment k: integrated over [t0s[k], t1] with nts[k] steps of
 * h_k = (t1 - t0s[k]) / nts[k], exactly what nocf_rollout_f32(x_k, ..., t0s[k], t1, nts[k], ...) computes for those rows (bit for bit: same
 * kernel, same per-tile arithmetic), but the launch covers all segments' tiles at once -- 9 x 512 rows fill the chip where 512 rows occupy an
 * eighth of it.
 *   nseg <= 16 segments; rows_per_seg a multiple of 16; (nseg - 1) * rows_per_seg < n <= nseg * rows_per_seg (a ragged last segment).
 *   t0s, nts       HOST arrays of nseg entries (copied into the kernel arguments)
 *   slot0s         HOST array (nullable = zeros): the first time slot of segment k in zFull / ctrlFull.  With slot0s[k] = int(t_s nt) + 1 the
 *                  caller's buffer holds, per row, the reference's concatenation cat(traj1, traj2) (src/plotter.py:822): it fills the slots
 *                  in front of slot0s[k] with the unshocked segment
 *   zFull          device [max(slot0s + nts) + 1, n, d+4], time-major as in nocf_rollout_f32; segment k writes slots slot0s[k] .. + nts[k] only
 *   ctrlFull       likewise                      cost_sums   device [nseg, 8]: one row of sums per segment
 * Returns NOCF_E_SHAPE when the network / problem has no one-CU weight-stationary kernel (singlequad has; nothing is launched then, and
 * the caller runs the segments one by one).
 */
int nocf_rollout_segments_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n,
                              int32_t nseg, int64_t rows_per_seg, const double* t0s, double t1, const int32_t* nts, const int32_t* slot0s,
                              int32_t stepper, const float* alph, float* z_out, float* persample, float* cost_sums, float* zFull, float* ctrlFull,
                              void* workspace, size_t workspace_bytes, void* stream);

/* 1 when nocf_rollout_segments_f32 has a kernel for this network / problem (host-side, nothing is launched), 0 otherwise: lets a caller
 * decide before it allocates and fills the segments' buffers (neuraloc_amd/shock.py). */
int nocf_segments_supported(const NocfPhi* phi, const NocfProb* prob);

/*
 * The last lines of OCflow (src/OCflow.py:80-90): out[0..6] = cost_sums[0..6] / cost_sums[7] (the batch means
 * [L, G, HJt, HJfin, HJgrad, Q, W]) and out[7] = Jc = L + alph[0] G + alph[3] HJt + alph[4] HJfin + alph[5] HJgrad.
 * cost_sums is what nocf_rollout_f32 wrote (after the all-reduce when the batch is sharded).  alph: host [6].
 */
int nocf_cost_means_f32(const float* cost_sums, const float* alph, float* out, void* stream);

/*
 * Training: the pair below replaces `Jc = OCflow(...); Jc.backward()` of trainOC.py:172-173
 * for every problem class and any depth nTh >= 2 whose activations fit the LDS (NOCF_E_LDS otherwise).
 *
 * nocf_rollout_record_f32 = nocf_rollout_f32 that also records the stage input s=[x,t] of every RK evaluation:
 *   s_all  device [nt*nstage, n, d+1]   (nstage = 4 for rk4, 1 for rk1);  z_out is required.
 *
 * nocf_rollout_bwd_f32 runs the exact adjoint of the discrete scheme.  It does not reduce the parameter
 * gradients itself: it streams, for every sample and evaluation, the vectors whose outer products they are,
 *   rows = (nt*nstage + 2) * n        (the two extra blocks are the terminal grad-Phi and Phi terms)
 *   Y, Ob, Wb                  device [rows, m]
 *   V, Ab, Qb, U0              device [nTh-1, rows, m]   one slab per residual layer i = 1..nTh-1
 *   Gb, Sx                     device [rows, d+1]
 *   (the kernel does not write the last n rows of Y, V, Ab, Gb: the caller zeroes those)
 *   PHIb                       device [n]         cotangent of Phi(x_T, t1);  lam0 device [n, d] = dJc/dx0 (nullable)
 * and the caller contracts them with library GEMMs:
 *   dK0 = Y'Gb + Ob'Sx   db0 = sum Ob   dK_i = V_i'Ab_i + Qb_i'U0_i   db_i = sum Qb_i   dw = sum Wb
 *   dc.weight = sum Gb + sum PHIb s_T
 *   dc.bias = sum PHIb   dM = Gb'Sx + 1/2 sum PHIb s_T s_T'   dA = A (dM + dM')
 *   hs      device [nt] fp32 step sizes as the forward used them: (float)((tk+h)-tk), tk += h in double
 *   inv_n   1 / (global batch size) -- the means of src/OCflow.py:80-86 run over all shards
 */
int nocf_rollout_record_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n,
                            double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                            float* z_out, float* persample, float* cost_sums, float* s_all,
                            void* workspace, size_t workspace_bytes, void* stream);

int nocf_rollout_bwd_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                         const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                         float* Y, float* Ob, float* V, float* Ab, float* Qb, float* U0, float* Wb, float* Gb, float* Sx,
                         float* PHIb, float* lam0, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Activation record (optional, training of two-layer networks that the split-role kernel takes: m = 512, point-agent problems; and that the
 * one-CU kernel takes: 32 < m <= 128 in whole 16-blocks, d+1 <= 32, every problem class).
 * nocf_rollout_record_act_f32 = nocf_rollout_record_f32 that also stores, for every RK evaluation and sample, the activations of
 * grad Phi -- u0 = sigma(o), tanh(o), tanh(q), a = w + hN K1' v ([nt*nstage, n, m] each) and grad Phi ([nt*nstage, n, d+1]) -- into
 *   act_rec  device [nocf_activation_record_floats(...)] floats (four sections of nt*nstage*n*m, one of nt*nstage*n*(d+1)); NULL: no record
 *   recorded host int32: 1 when the kernel this call launched wrote the record (the split-role and the one-CU kernel do), else 0
 * nocf_rollout_bwd_act_f32 = nocf_rollout_bwd_f32 that, given a record the forward launch WROTE (recorded == 1), loads these
 * activations instead of re-running grad Phi's forward sweep at every evaluation (four of its eight GEMM phases and the weights they
 * stream; the terminal evaluation is still recomputed).  act_rec NULL: exactly nocf_rollout_bwd_f32.
 * nocf_activation_record_floats returns 0 for shapes without a recording kernel (pass NULL then).
 * (src/OCflow.py:7-95 forward, trainOC.py:172-173 backward: what autograd keeps as saved tensors of the unrolled graph)
 */
size_t nocf_activation_record_floats(int32_t d, int32_t m, int32_t nTh, int64_t n, int32_t nt, int32_t stepper);
int nocf_rollout_record_act_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n,
                                double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                float* z_out, float* persample, float* cost_sums, float* s_all, float* act_rec, int32_t* recorded,
                                void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_bwd_act_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                             const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                             float* Y, float* Ob, float* V, float* Ab, float* Qb, float* U0, float* Wb, float* Gb, float* Sx,
                             float* PHIb, float* lam0, const float* act_rec, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Training tape + split-role adjoint (round 4; the path trainOC.py:172-174 takes for the networks the split-role kernel runs: m = 512,
 * nTh = 2, point-agent problems).  The tape is the activation record above with the TERMINAL evaluation as one more block and three
 * scalars per evaluation -- everything autograd would keep of the unrolled graph of src/OCflow.py:7-95 -- laid out as
 *     R = (nt*nstage + 1) * n rows, block e < nt*nstage = RK evaluation e, block nt*nstage = the terminal evaluation (src/OCflow.py:58-64)
 *     [0, 4 R m)                  u0 | tanh(o) | tanh(q) | a          four sections [R, m]
 *     [4 R m, + R (d+1))          grad Phi                            [R, d+1]   (padded to a multiple of 4 floats)
 *     then n m                    u_1 of the terminal evaluation      [n, m]
 *     then 4 R                    (dPhi/dt - H, q, w, 0) per row; terminal block: (Phi - alph0 G, 0, 0, 0)
 * nocf_tape_floats: size of that buffer in floats, 0 when the shape has no tape-writing kernel (use the record calls above then).
 * nocf_rollout_tape_f32 = nocf_rollout_record_f32 with s_all of nt*nstage + 1 blocks (the last: [z(T), t1]) and the tape;
 *   *recorded = 1 when the launched kernel wrote the tape (else only the first nt*nstage blocks of s_all are written: fall back to
 *   nocf_rollout_bwd_f32).
 * nocf_rollout_bwd_tape_f32: the adjoint of the discrete scheme on the split-role layout.  Writes the row vectors whose outer products
 *   are the weight gradients, one row per (block, sample) as on the tape:
 *     Y = tanh(o).a, Ab = abar0, Wb = dw row, Qb = qbar, Ob = obar   device [R, m];   Gb = gbar   device [R, d+1]
 *   The value's rows of nocf_rollout_bwd_f32 (cotangent phib of Phi(z(T), T)) are NOT in them: the caller adds phib.tanh(q).w to Qb,
 *   phib.Y to Ob and phib.u_1 (tape) to Wb on the n rows of the terminal block.  Then, with the tape's U0 = u0, TH1 = tanh(q), Sx = s_all,
 *     dK0 = Y'Gb + Ob'Sx,  db0 = colsum Ob,  dK1 = diag(w) TH1'Ab + Qb'U0,  db1 = colsum Qb,  dw = colsum Wb,
 *     dc.weight = colsum Gb + phib'sT,  d(A'A) = Gb'Sx + (sT.phib)'sT / 2,  phib = alph4 sign(tape scalar of the terminal block) / n_total.
 *   lam0 device [n, d] = dJc/dx0 (nullable).  Returns NOCF_E_SHAPE when the shape / problem / residency does not qualify (nothing launched).
 *   A timed-out exchange is reported like the forward's (nocf_last_rollout_status_async); nocf_poison_if_failed_f32 turns a buffer
 *   into NaN on the stream if the last launch on this device failed (call it on the gradients before they are used).
 *   Weight-gradient roles (optional): with dK1 device [m, m], dK0 device [m, d+1] and dw_scratch device [nocf_dw_scratch_floats()]
 *   the two large weight gradients are accumulated IN THE KERNEL by two more role workgroups per member that consume the row streams
 *   behind progress counters (csrc/nocf_duo_bwd.inc): on return (*dw_done = 1) dK1 and dK0 hold the complete sums INCLUDING the value's
 *   rows (the caller must then not add phib.v / phib.y to Qb / Ob before using them for anything else; Wb's value rows and the column sums
 *   stay the caller's).  *dw_done = 0: the kernel without those roles ran (NOCF_DUO_DW=0, or NULL pointers) and dK1 / dK0 are untouched.
 */
size_t nocf_tape_floats(int32_t d, int32_t m, int32_t nTh, int64_t n, int32_t nt, int32_t stepper);
int nocf_rollout_tape_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n,
                          double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                          float* z_out, float* persample, float* cost_sums, float* s_all, float* tape, int32_t* recorded,
                          void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_bwd_tape_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper,
                              const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                              const float* tape, float* Y, float* Ab, float* Wb, float* Qb, float* Ob, float* Gb, float* lam0,
                              float* dK1, float* dK0, float* dw_scratch, size_t dw_scratch_floats, int32_t* dw_done,
                              void* workspace, size_t workspace_bytes, void* stream);
size_t nocf_dw_scratch_floats(void);
/*
 * nocf_rollout_bwd_tape_sums_f32 = nocf_rollout_bwd_tape_f32 with the COLUMN SUMS formed in the kernel (round 5): the epilogues that hold the dw rows,
 * qbar and obar add them up (16 rows across a DPP row, then per wave in LDS; rows beyond the batch add nothing) and every group writes one partial:
 *     colsum   device [G, 3, m], G = colsum_floats / (3 m) >= nocf_bwd_colsum_floats(n) / (3 m):  (colsum Wb | colsum Qb | colsum Ob) per group of
 *              every launch, zero for the rest; the caller sums over G in index order (fixed order: deterministic).
 * The dw rows are then not streamed at all (no Wb: [R, m] floats less to allocate and to write) and db1 / db0 / dw need no pass over Qb / Ob / Wb.
 * As in nocf_rollout_bwd_tape_f32 the value's rows are not in them: the caller adds phib'(tanh(q).w), phib'Y and phib'u_1 of the terminal block's n rows.
 */
size_t nocf_bwd_colsum_floats(int64_t n);
int nocf_rollout_bwd_tape_sums_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper,
                                   const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                                   const float* tape, float* Y, float* Ab, float* Qb, float* Ob, float* Gb, float* lam0,
                                   float* dK1, float* dK0, float* dw_scratch, size_t dw_scratch_floats, int32_t* dw_done,
                                   float* colsum, size_t colsum_floats, void* workspace, size_t workspace_bytes, void* stream);
int nocf_poison_if_failed_f32(float* buf, int64_t count, void* stream);

/*
 * Parameter gradients of the stand-alone value call Phi(s) (src/Phi.py:91-96 under torch autograd: `net(x).backward(gout)`), any depth:
 * the rows whose outer products are the gradients, in the layout of nocf_rollout_bwd_f32 with nt = 0 (two blocks of n rows; the SECOND
 * block carries the value's rows, the first one is zero cotangents):  dK0 = Ob' Sx, db0 = colsum(Ob), dK_i = Qb_i' U0_i, db_i = colsum(Qb_i),
 * dw = colsum(Wb), dc.weight = gout' s, dc.bias = sum(gout), d(A'A) = 1/2 (s . gout)' s.  dPhi/ds is nocf_phi_grad_f32 times gout.
 *   s     device [n, d+1];   gout  device [n]: the cotangent of Phi(s), an INPUT
 *   Y, Ob, Wb  device [2 n, m];  V, Ab, Qb, U0  device [nTh-1, 2 n, m];  Gb, Sx  device [2 n, d+1]  (Y, V, Ab, Gb: second block zeroed by the caller)
 */
int nocf_phi_value_bwd_f32(const NocfPhi* phi, const float* s, int64_t n, float* gout,
                           float* Y, float* Ob, float* V, float* Ab, float* Qb, float* U0, float* Wb, float* Gb, float* Sx,
                           void* workspace, size_t workspace_bytes, void* stream);

/*
 * The vector-Jacobian product of the stand-alone gradient call (src/Phi.py:99-138 under torch autograd: `net.getGrad(x).backward(gbar)`), any depth:
 * sbar = (d grad Phi / d s)' gbar and, in the FIRST block of n rows of the streams (layout of nocf_rollout_bwd_f32 with nt = 0), the rows of the
 * parameter gradients:  dK0 = Y' Gb + Ob' Sx, db0 = colsum(Ob), dK_i = V_i' Ab_i + Qb_i' U0_i, db_i = colsum(Qb_i), dw = colsum(Wb),
 * dc.weight = colsum(Gb), d(A'A) = Gb' Sx  (Gb = gbar, Sx = s).
 *   s, gbar, sbar  device [n, d+1];   streams as in nocf_phi_value_bwd_f32 (2 n rows each; only the first n are written)
 */
int nocf_phi_grad_bwd_f32(const NocfPhi* phi, const float* s, int64_t n, const float* gbar, float* sbar,
                          float* Y, float* Ob, float* V, float* Ab, float* Qb, float* U0, float* Wb, float* Gb, float* Sx,
                          void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same adjoint for SMALL networks (nTh = 2, m <= 32, d+1 <= 32, Cross2D agents: the shapes the lane kernel of
 * nocf_rollout_f32 takes), one wavefront per sample with every weight-gradient row in registers: nothing is streamed and
 * nothing is left to contract.  Returns NOCF_E_SHAPE for any other shape (use nocf_rollout_bwd_f32 then).
 *   gpart  device [n, nocf_small_grad_floats(d, m)]: per-sample gradient vectors
 *          [dK0 (m x (d+1)) | db0 (m) | dK1 (m x m) | db1 (m) | dw (m) | dc.weight (d+1) | dc.bias (1) | dM ((d+1) x (d+1))],
 *          dM = d/d(A'A) (dA = A (dM + dM')); the caller sums them over the samples
 *   lam0   device [n, d] = dJc/dx0 (nullable)
 */
int64_t nocf_small_grad_floats(int32_t d, int32_t m);
int nocf_rollout_bwd_small_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                               const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                               float* gpart, float* lam0, void* stream);

/*
 * Ensembles: E = `members` small networks of ONE shape rolled out (and differentiated) in one launch each, on the lane kernels of
 * nocf_rollout_f32 / nocf_rollout_bwd_small_f32 (nTh = 2, m <= 32, d+1 <= 32, point agents, at most 16 of them; the adjoint: Cross2D
 * agents).  One wavefront integrates one sample, so the launch is one batch of E * n rows: row g is sample g % n of member g / n, a
 * workgroup may hold rows of two members, and member e's rows carry the bits of the single-network call on that member alone.
 *   phi        the STACKED network: K0 [E, m, d+1], b0 [E, m], K [E, m, m], b [E, m], w [E, m], A [E, r, d+1], cw [E, d+1], cb_dev [E]
 *              (contiguous: member e's tensor begins e tensor sizes behind the base; cb_dev is required, cb is not read)
 *   n          rows of ONE member;  members >= 1;  members * n < 2^31
 *   x          device [n, d] with x_member_stride = 0 (every member integrates the same starts) or [E, n, d] with x_member_stride = n * d
 *   alph       DEVICE [E, 6], float32: row e stands for the `alph` of the single-network calls ([0], [3], [4], [5]) AND for the problem's
 *              alph_Q ([1]) and alph_W ([2]) of member e; prob->alph_Q / alph_W are not read.  Everything else of `prob` (target, obstacle,
 *              r, mode) and t0, t1, nt, stepper are common to the members
 *   z_out [E*n, d+4], persample [E*n, 7], s_all [nt*nstage, E*n, d+1], zFull [nt+1, E*n, d+4], ctrlFull [nt+1, E*n, a]: the single-network
 *              layouts over E*n rows (time-major where they are);  gpart [E*n, nocf_small_grad_floats], lam0 [E*n, d]: member e's
 *              per-sample partials are rows [e n, (e + 1) n), the caller sums each member's rows;  inv_n: 1 / n of a member
 *   cost_sums  device [E, 8], cost_means device [E, 8] (nullable; needs cost_sums): per member what nocf_rollout_means_f32 returns, reduced
 *              in its order by one launch with the member on the grid
 *   workspace  not used (the lane kernels need none): may be NULL / 0
 * Any other shape, a quadcopter, members < 1 or NOCF_LANE=0 return NOCF_E_SHAPE / NOCF_E_PROB before anything is enqueued: no other
 * kernel family takes an ensemble.  nocf_last_rollout_kernel(): "rollout_lane_kernel<ens>" / "rollout_lane_bwd_kernel<ens>".
 */
int nocf_rollout_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members, int64_t x_member_stride,
                              double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                              float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull,
                              void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_record_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members, int64_t x_member_stride,
                                     double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                     float* z_out, float* persample, float* cost_sums, float* s_all,
                                     void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_bwd_small_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t members, int32_t nt, int32_t stepper, double t1,
                                        const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                                        float* gpart, float* lam0, void* stream);

/*
 * The same adjoint for MEDIUM two-layer networks (nTh = 2, 32 < m <= 128, d+1 <= 32, every problem class: the shapes the one-CU
 * weight-stationary kernel of nocf_rollout_f32 takes, e.g. singlequad; reference: trainOC.py:172-174 on src/OCflow.py:7-140).  One
 * workgroup per 16 samples keeps the network in its registers, takes grad Phi's activations from the forward's activation record
 * (act_rec of nocf_rollout_record_act_f32, requested one evaluation ahead; null or `recorded` = 0: it re-runs grad Phi at the recorded
 * stage inputs) and ACCUMULATES the weight gradients in the kernel (MFMA outer products with the samples on the k axis): no row
 * stream, no library GEMM.  Every workgroup writes one partial gradient vector; the caller adds the partial vectors (fixed order).
 *   nocf_mid_grad_rows   number of partial vectors for a batch of n rows (min(ceil(n / 16), 1024)), or 0 when the shape has no such kernel
 *                        (NOCF_E_SHAPE from the launch then: use nocf_rollout_bwd_act_f32)
 *   act_rec nullable: the activation record of the forward launch (only when that launch reported recorded = 1)
 *   gpart  device [gpart_rows, nocf_small_grad_floats(d, m)], the layout of nocf_rollout_bwd_small_f32
 *   lam0   device [n, d] = dJc/dx0 (nullable);   workspace: nocf_workspace_bytes (same as the forward's)
 */
int64_t nocf_mid_grad_rows(int32_t d, int32_t m, int32_t nTh, int32_t r, int32_t n_agents, int64_t n);
int nocf_rollout_bwd_mid_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                             const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                             const float* act_rec, float* gpart, int64_t gpart_rows, float* lam0, void* workspace, size_t workspace_bytes,
                             void* stream);

/*
 * Ensembles on the one-CU kernels: E = `members` networks of ONE shape with a one-CU plan (nTh = 2, m <= 128, d+1 <= 32, rank of A <= 16,
 * every problem class; the adjoint: 32 < m) rolled out, and differentiated, in one launch each.  A 16-sample tile stays on its CU and a
 * network in its workgroup, so member e simply takes workgroups [e * tiles, (e + 1) * tiles) of the launch; its last tile replicates ITS row
 * n - 1, and its results carry the bits of nocf_rollout_f32 / nocf_rollout_record_act_f32 / nocf_rollout_bwd_mid_f32 on that member alone.
 *   phi, n, x, x_member_stride, alph, cost_sums, cost_means    as for nocf_rollout_ensemble_f32 (stacked tensors, cb_dev required, alph the
 *              DEVICE table [E, 6] standing for alph[0, 3, 4, 5] and the problem's alph_Q / alph_W)
 *   every buffer is MEMBER-MAJOR -- member e's block has the single-network layout (this differs from the lane ensemble, which is time-major
 *   over E*n rows):  z_out [E, n, d+4], persample [E, n, 7], zFull [E, nt+1, n, d+4], ctrlFull [E, nt+1, n, a], s_all [E, nt*nstage, n, d+1],
 *              lam0 [E, n, d];  act_rec [E, S] with S = nocf_activation_record_floats(d, m, nTh, n, nt, stepper) rounded UP to a multiple
 *              of 4 floats (the record is read in 16-byte pieces), nullable, written under the single-network rule (m % 16 == 0, m > 32:
 *              *recorded = 1)
 *   gpart      device [E, gpart_rows, nocf_small_grad_floats(d, m)] with gpart_rows == nocf_mid_grad_rows(d, m, nTh, r, agents, n) exactly:
 *              workgroup j of member e walks the member's tiles j, j + gpart_rows, ... and writes gpart[e][j]; the caller adds each
 *              member's partial vectors in order.  inv_n: 1 / n of a member
 *   workspace  nocf_mid_ensemble_workspace_bytes(d, m, nTh, r, members) bytes, 0 when the shape has no one-CU plan; member e's block (images,
 *              padded vectors, the plan record with its c.bias) begins e * (bytes / members) behind the base.  All members are packed by
 *              ONE launch
 * Refused before anything is enqueued: a shape without a one-CU plan (the adjoint: without an adjoint instantiation), NOCF_MONO=0, members
 * < 1, a stride that is neither 0 nor n d, members * n >= 2^31 (NOCF_E_SHAPE); a workspace that is too small, gpart_rows != the query's
 * (NOCF_E_WORKSPACE); cb_dev == NULL (NOCF_E_NULL).  nocf_last_rollout_kernel(): "rollout_mono_kernel<ens>" / "rollout_mono_bwd_kernel<ens>".
 */
size_t nocf_mid_ensemble_workspace_bytes(int32_t d, int32_t m, int32_t nTh, int32_t r, int32_t members);
int nocf_rollout_mid_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members, int64_t x_member_stride,
                                  double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                  float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull,
                                  void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_record_mid_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members, int64_t x_member_stride,
                                         double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                         float* z_out, float* persample, float* cost_sums, float* s_all, float* act_rec, int32_t* recorded,
                                         void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_bwd_mid_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t members, int32_t nt, int32_t stepper, double t1,
                                      const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                                      const float* act_rec, float* gpart, int64_t gpart_rows, float* lam0,
                                      void* workspace, size_t workspace_bytes, void* stream);

/*
 * Ensembles under in-kernel Brownian noise: the four forward launches above (nocf_rollout_ensemble_f32 / nocf_rollout_record_ensemble_f32 on
 * the lane kernels, nocf_rollout_mid_ensemble_f32 / nocf_rollout_record_mid_ensemble_f32 on the one-CU kernels) with the per-step disturbance
 * of nocf_rollout_noisy_f32 drawn inside the kernel, every member at ITS OWN noise level and seed.  Behind x_member_stride they take
 *   scale      device [E, d], float32: row e = fp32(sigma_i sqrt(h)) of member e, the `scale` of nocf_rollout_noisy_f32 (a row of zeros: that
 *              member's rollout is the undisturbed one)
 *   seeds      device [E], uint64: member e's seed
 *   row0       >= 0: the key of row 0 of EVERY member.  Row j of member e meets the disturbance of (seeds[e], row0 + j, k, i) -- the row INSIDE
 *              the member, so members given one seed meet identical noise (common random numbers across the levels), and a member's rows may
 *              be cut into chunks as the rows of nocf_rollout_noisy_f32 may
 * and every other argument, buffer layout (lane: time-major over E*n rows; one-CU: member-major) and refusal is the undisturbed sibling's.
 * Member e's results carry the bits of nocf_rollout_noisy_f32 / nocf_rollout_record_noisy_f32 with (scale + e d, seeds[e], row0) on that
 * member alone, on the same kernel family.  The adjoints are the undisturbed ensembles' (nocf_rollout_bwd_small_ensemble_f32 /
 * nocf_rollout_bwd_mid_ensemble_f32) on the recorded displaced states: the disturbance does not depend on the parameters.
 * scale == NULL or seeds == NULL: NOCF_E_NULL; row0 < 0: NOCF_E_SHAPE.  nocf_last_rollout_kernel(): "rollout_lane_kernel<ens,noisy>" /
 * "rollout_mono_kernel<ens,noisy>".  Probe for the symbols: nocf_version() did not change with them.
 */
int nocf_rollout_noisy_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members, int64_t x_member_stride,
                                    const float* scale, const uint64_t* seeds, int64_t row0,
                                    double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                    float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull,
                                    void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_record_noisy_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members,
                                           int64_t x_member_stride, const float* scale, const uint64_t* seeds, int64_t row0,
                                           double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                           float* z_out, float* persample, float* cost_sums, float* s_all,
                                           void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_noisy_mid_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members, int64_t x_member_stride,
                                        const float* scale, const uint64_t* seeds, int64_t row0,
                                        double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                        float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull,
                                        void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_record_noisy_mid_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members,
                                               int64_t x_member_stride, const float* scale, const uint64_t* seeds, int64_t row0,
                                               double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                               float* z_out, float* persample, float* cost_sums, float* s_all, float* act_rec, int32_t* recorded,
                                               void* workspace, size_t workspace_bytes, void* stream);

/*
 * The STATE-ONLY adjoint: the lambda recursion of the three adjoints above (nocf_rollout_bwd_small_f32 / _mid_f32 / _act_f32) with every
 * parameter-gradient operation compiled out -- no gradient rows or accumulators, no outer products, no partial vectors, no row streams --
 * and the per-step state cotangents written out.  The inner loop of a worst-case disturbance search (nocf_disturbance_ascent_f32) and
 * the sensitivity of a disturbed rollout: with z_{k+1} = step(z_k) + W[k] (nocf_rollout_record_disturbed_f32), dJ/dW[k] is the cotangent
 * of z_{k+1}, which every adjoint kernel holds when it begins the last stage of step k.
 *   inputs   those of the three adjoints; s_all / z_final from ANY recording forward, disturbed or not; hs the forward's fp32 step sizes;
 *            inv_n = 1 / (global batch size) (1: every row's own objective); alph[3..5] = 0 is supported: the control objective L + alph0 G
 *   act_rec  nullable; the forward's activation record, used by the one-CU kernel only (when the forward reported recorded = 1)
 *   lam0     device [n, d] = dJ/dx0 (nullable)
 *   lamW     device [nt, n, d] (nullable), time-major like W, contiguous: lamW[k] = the state cotangent behind step k = dJ/dW[k];
 *            lamW[nt-1] is the terminal cotangent dJ/dx(T).  Only rows < n and d floats per row are written
 *   workspace: nocf_workspace_bytes (same as the forward's)
 * Dispatch: the register-resident small-network kernel, then the one-CU kernel, then the per-tile kernel -- the order of
 * nocf_rollout_record_disturbed_f32, so the adjoint runs on the forward's family.  nocf_last_rollout_kernel() reports
 * "rollout_lane_bwd_kernel<states>", "rollout_mono_bwd_kernel<states>" or "rollout_bwd_kernel<states>".
 * lam0 == NULL and lamW == NULL: NOCF_E_NULL.  Shape, stepper, workspace and LDS refusals are the three adjoints' own.  Every refusal
 * returns before anything is enqueued.  float32 only.
 */
int nocf_rollout_bwd_states_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                                const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                                const float* act_rec, float* lam0, float* lamW,
                                void* workspace, size_t workspace_bytes, void* stream);

/*
 * The JOINT adjoints: nocf_rollout_bwd_small_f32 / _mid_f32 / _act_f32 with one more output, lamW (after lam0), the per-step state
 * cotangents of nocf_rollout_bwd_states_f32.  One launch gives the parameter gradients (and lam0) exactly as the existing entry forms
 * them AND dJ/dW of a disturbed rollout: an iteration of min-max ("free" adversarial) training is one recording forward, one joint
 * adjoint and one nocf_disturbance_ascent_f32, where the existing entries need two forwards and two adjoints.  The kernels are the
 * existing ones' third instantiation: every statement of the full adjoint plus the lamW[k] store of the state-only one, at the same
 * place (the state cotangent when the last stage of step k begins; rk1 alike).
 *   lamW   device [nt, n, d] (nullable), time-major like W, contiguous: lamW[k] = dJ/dW[k]; lamW[nt-1] is the terminal cotangent dJ/dx(T).
 *          Only rows < n and d floats per row are written.  lamW == NULL: the call IS the existing entry (same kernel, same bits)
 *   every other argument, the workspace and every refusal: the existing entry's (each goes through that entry's own code path)
 * nocf_last_rollout_kernel() reports "rollout_lane_bwd_kernel<joint>", "rollout_mono_bwd_kernel<joint>" or "rollout_bwd_kernel<joint>"
 * (the existing names when lamW == NULL).  The per-tile joint kernel is instantiated for the generic plan and for the shapes whose
 * disturbed forward is specialised, like the state-only one.  nocf_version() is unchanged: callers probe for the symbols.  float32 only.
 */
int nocf_rollout_bwd_small_w_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                                 const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                                 float* gpart, float* lam0, float* lamW, void* stream);
int nocf_rollout_bwd_mid_w_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                               const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                               const float* act_rec, float* gpart, int64_t gpart_rows, float* lam0, float* lamW,
                               void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_bwd_act_w_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                               const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                               float* Y, float* Ob, float* V, float* Ab, float* Qb, float* U0, float* Wb, float* Gb, float* Sx,
                               float* PHIb, float* lam0, float* lamW, const float* act_rec,
                               void* workspace, size_t workspace_bytes, void* stream);

/*
 * The WEIGHTED adjoints: nocf_rollout_bwd_small_f32 / _mid_f32 / _act_f32 with one weight per sample in place of the scalar inv_n.
 * The gradient of a risk measure of the per-sample costs (CVaR, entropic risk), of an importance-weighted batch or of any other weighted
 * sum is sum_i w_i grad J_i; the existing entries seed every sample's cotangents with the one value inv_n and cannot form it.  The
 * kernels are the existing ones' further instantiation: wrow[row] stands where inv_n stands at that row's cotangent seeds (the terminal
 * state cotangent, the cotangent of grad Phi(z(T)), the cotangent of Phi(z(T), T), and the running-cost factor of every RK evaluation).
 *   wrow   device [n] float32, contiguous, not modified.  Any finite values, negative and zero included; nothing checks them on the
 *          device.  Tail rows of the last tile, which replicate a valid sample, keep weight 0
 *   every output is the existing entry's with wrow[row] for inv_n: the parameter gradient (gpart / the partial rows / the row streams
 *          Y ... PHIb) is sum_i wrow[i] grad J_i, and lam0[i] = wrow[i] dJ_i/dx_i.  wrow filled with (float)inv_n gives the existing
 *          entry's bits
 *   every other argument, the workspace, the dispatch (NOCF_E_SHAPE hands a shape on to the next family) and every refusal: the
 *          existing entry's;  wrow == NULL: NOCF_E_NULL.  Every refusal returns before anything is enqueued
 * nocf_last_rollout_kernel() reports "rollout_lane_bwd_kernel<weighted>", "rollout_mono_bwd_kernel<weighted>" or
 * "rollout_bwd_kernel<weighted>".  The per-tile weighted kernel is instantiated for the generic plan and for the shapes whose disturbed
 * forward is specialised, like the joint one.  The split-role kernel and the tape adjoint take no weights: a weighted call follows a
 * disturbed or noisy recording forward, which never runs them.  nocf_version() is unchanged: callers probe for the symbols.  float32 only.
 */
int nocf_rollout_bwd_small_rw_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                                  const float* alph, const float* wrow, const float* s_all, const float* z_final, const float* hs,
                                  float* gpart, float* lam0, void* stream);
int nocf_rollout_bwd_mid_rw_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                                const float* alph, const float* wrow, const float* s_all, const float* z_final, const float* hs,
                                const float* act_rec, float* gpart, int64_t gpart_rows, float* lam0,
                                void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_bwd_act_rw_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                                const float* alph, const float* wrow, const float* s_all, const float* z_final, const float* hs,
                                float* Y, float* Ob, float* V, float* Ab, float* Qb, float* U0, float* Wb, float* Gb, float* Sx,
                                float* PHIb, float* lam0, const float* act_rec,
                                void* workspace, size_t workspace_bytes, void* stream);

/*
 * The WEIGHTED ENSEMBLE adjoints: nocf_rollout_bwd_small_ensemble_f32 / nocf_rollout_bwd_mid_ensemble_f32 with one weight per row of every
 * member in place of the scalar inv_n -- a risk measure per member (a sweep over the CVaR level or over theta) differentiated in the one
 * launch the members' means cost.  The kernels are the ensemble adjoints' further instantiation (ensemble AND weighted, both compile-time
 * choices): the member's pointers and multipliers as in the ensemble adjoint, wrow[e][row] where inv_n stands at that row's cotangent seeds
 * as in the weighted adjoint.
 *   wrow   device [E, n] float32, contiguous, not modified: member e's weights are the n floats at wrow + e n -- the lane ensemble's row
 *          order (row g of the E n batch reads wrow[g]) and the one-CU ensemble's member-major order alike.  Any finite values, negative and
 *          zero included; nothing checks them on the device.  Tail rows of a member's last tile (one-CU) keep weight 0; a tail wave (lane)
 *          replicates the last row and writes nothing
 *   every output is the ensemble entry's with wrow[e][i] for inv_n: member e's partial vectors sum to sum_i wrow[e][i] grad J_{e,i} and
 *          lam0[e][i] = wrow[e][i] dJ_{e,i}/dx.  Member e's results carry the bits of nocf_rollout_bwd_small_rw_f32 /
 *          nocf_rollout_bwd_mid_rw_f32 with wrow + e n on that member alone; wrow filled with (float)inv_n gives the ensemble entry's bits
 *   every other argument, buffer layout (lane: rows [e n, (e + 1) n) of gpart / lam0; one-CU: member-major, gpart_rows == the query's), the
 *          workspace and every refusal: the ensemble entry's;  wrow == NULL: NOCF_E_NULL.  Every refusal returns before anything is enqueued
 * nocf_last_rollout_kernel() reports "rollout_lane_bwd_kernel<ens,weighted>" / "rollout_mono_bwd_kernel<ens,weighted>".  nocf_version()
 * is unchanged: callers probe for the symbols.  float32 only.
 */
int nocf_rollout_bwd_small_ensemble_rw_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t members, int32_t nt, int32_t stepper,
                                           double t1, const float* alph, const float* wrow, const float* s_all, const float* z_final,
                                           const float* hs, float* gpart, float* lam0, void* stream);
int nocf_rollout_bwd_mid_ensemble_rw_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t members, int32_t nt, int32_t stepper,
                                         double t1, const float* alph, const float* wrow, const float* s_all, const float* z_final,
                                         const float* hs, const float* act_rec, float* gpart, int64_t gpart_rows, float* lam0,
                                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * One step of projected gradient ascent on per-row disturbance paths, in place: for every row i, over its [nt, d] path of W,
 *     W_i += step (mask o g_i) / ||mask o g_i||_2          (the row is left untouched when that norm is 0 or not finite)
 *     W_i *= eps / ||W_i||_2   when ||W_i||_2 > eps         (projection onto the ball over the whole path)
 *   W     device [nt, n, d] float32, time-major, contiguous: updated
 *   g     device [nt, n, d]: the ascent direction (lamW of nocf_rollout_bwd_states_f32); not modified
 *   mask  device [d] floats of 0 / 1 (nullable), the meaning of brownian_disturbances(mask=): masked components take no step and keep
 *         their bits; the projection scales the whole row
 * One wavefront per row; both norms are reductions in a fixed order, no atomics: identical inputs give identical bits.  With the
 * recording forward and the state-only adjoint an iteration of the search is three launches and no host round trip.
 * n, nt, d < 1 or a negative / non-finite step or eps: NOCF_E_SHAPE.
 */
int nocf_disturbance_ascent_f32(float* W, const float* g, const float* mask, int64_t n, int32_t nt, int32_t d,
                                double step, double eps, void* stream);

/*
 * ADVERSARIAL ENSEMBLES: the ensemble launches above under a TENSOR disturbance per member, the ensemble adjoints with
 * dJ/dW written out, and the ascent step over all members -- an iteration of min-max training, or of a worst-case search, for E networks in
 * the three launches it costs one.  Every member e meets z_{k+1} = step(z_k) + W[e][k].
 *
 * Forwards: nocf_rollout_ensemble_f32 / nocf_rollout_record_ensemble_f32 (lane kernels) and nocf_rollout_mid_ensemble_f32 /
 * nocf_rollout_record_mid_ensemble_f32 (one-CU kernels) with, behind x_member_stride,
 *   W                device [E, nt, n, d] float32, MEMBER-major (both families): member e's slice is exactly the [nt, n, d] tensor of
 *                    nocf_rollout_disturbed_f32; not modified
 *   w_member_stride  nt * n * d, or 0: ONE [nt, n, d] tensor that every member meets (as x_member_stride = 0 shares the starts)
 * and every other argument, buffer layout (lane: time-major over E*n rows; one-CU: member-major) and refusal is the undisturbed sibling's.
 * Member e's results carry the bits of nocf_rollout_disturbed_f32 / nocf_rollout_record_disturbed_f32 with W + e w_member_stride on that
 * member alone, on the same kernel family.  W == NULL: NOCF_E_NULL; a stride that is neither 0 nor nt n d: NOCF_E_SHAPE.
 * nocf_last_rollout_kernel(): "rollout_lane_kernel<ens,disturbed>" / "rollout_mono_kernel<ens,disturbed>".
 *
 * Adjoints: nocf_rollout_bwd_small_ensemble_f32 / nocf_rollout_bwd_mid_ensemble_f32 with one more output behind lam0,
 *   lamW   device [E, nt, n, d] float32, MEMBER-major (both families), contiguous: lamW[e][k] = the state cotangent of member e behind step k
 *          = dJ_e/dW[e][k]; lamW[e][nt-1] is the terminal cotangent.  Only rows < n of each member and d floats per row are written
 * _w (JOINT): every output of the ensemble adjoint exactly as it forms them AND lamW; lamW == NULL: the call IS the ensemble adjoint (same
 *          kernel, same bits).  Member e's results carry the bits of nocf_rollout_bwd_small_w_f32 / nocf_rollout_bwd_mid_w_f32 on that member
 * _states (STATE-ONLY): no gpart / gpart_rows argument; lam0 [E*n, d] (lane) / [E, n, d] (one-CU) and lamW, at least one of them (both NULL:
 *          NOCF_E_NULL); alph rows with [3..5] = 0 give the control objective.  Member e's results carry the bits of
 *          nocf_rollout_bwd_states_f32 on that member, on the same family
 * Every other argument, the workspace and every refusal: the ensemble adjoint's.  A weighted (wrow) adversarial ensemble does not exist.
 * nocf_last_rollout_kernel(): "rollout_lane_bwd_kernel<ens,joint>" / "<ens,states>", "rollout_mono_bwd_kernel<ens,joint>" / "<ens,states>".
 *
 * nocf_disturbance_ascent_ensemble_f32: nocf_disturbance_ascent_f32 over the E * n rows of W / g [E, nt, n, d] in one launch; the member of a
 * row picks its step length and radius from the DEVICE tables steps [E] and epss [E] (float32, values >= 0 and finite: nothing checks them on
 * the device).  Member e's slice carries the bits of nocf_disturbance_ascent_f32 on it with ((double)steps[e], (double)epss[e]).
 * NULL W / g / steps / epss: NOCF_E_NULL; n, members, nt, d < 1 or members * n >= 2^31: NOCF_E_SHAPE.
 *
 * Every refusal returns before anything is enqueued.  nocf_version() is unchanged: callers probe for the symbols.  float32 only.
 */
int nocf_rollout_disturbed_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members, int64_t x_member_stride,
                                        const float* W, int64_t w_member_stride,
                                        double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                        float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull,
                                        void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_record_disturbed_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members,
                                               int64_t x_member_stride, const float* W, int64_t w_member_stride,
                                               double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                               float* z_out, float* persample, float* cost_sums, float* s_all,
                                               void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_disturbed_mid_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members,
                                            int64_t x_member_stride, const float* W, int64_t w_member_stride,
                                            double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                            float* z_out, float* persample, float* cost_sums, float* cost_means, float* zFull, float* ctrlFull,
                                            void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_record_disturbed_mid_ensemble_f32(const NocfPhi* phi, const NocfProb* prob, const float* x, int64_t n, int32_t members,
                                                   int64_t x_member_stride, const float* W, int64_t w_member_stride,
                                                   double t0, double t1, int32_t nt, int32_t stepper, const float* alph,
                                                   float* z_out, float* persample, float* cost_sums, float* s_all, float* act_rec, int32_t* recorded,
                                                   void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_bwd_small_ensemble_w_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t members, int32_t nt, int32_t stepper,
                                          double t1, const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                                          float* gpart, float* lam0, float* lamW, void* stream);
int nocf_rollout_bwd_mid_ensemble_w_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t members, int32_t nt, int32_t stepper,
                                        double t1, const float* alph, double inv_n, const float* s_all, const float* z_final, const float* hs,
                                        const float* act_rec, float* gpart, int64_t gpart_rows, float* lam0, float* lamW,
                                        void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_bwd_small_ensemble_states_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t members, int32_t nt, int32_t stepper,
                                               double t1, const float* alph, double inv_n, const float* s_all, const float* z_final,
                                               const float* hs, float* lam0, float* lamW, void* stream);
int nocf_rollout_bwd_mid_ensemble_states_f32(const NocfPhi* phi, const NocfProb* prob, int64_t n, int32_t members, int32_t nt, int32_t stepper,
                                             double t1, const float* alph, double inv_n, const float* s_all, const float* z_final,
                                             const float* hs, const float* act_rec, float* lam0, float* lamW,
                                             void* workspace, size_t workspace_bytes, void* stream);
int nocf_disturbance_ascent_ensemble_f32(float* W, const float* g, const float* mask, int64_t n, int32_t members, int32_t nt, int32_t d,
                                         const float* steps, const float* epss, void* stream);

/*
 * C[m, n] (+)= sum_k A[k, 0..m) (x) B[k, 0..n) for small outputs (m, n <= 512, at most 64 tiles of 64 x 64) and very many rows: the contraction of the rows that
 * nocf_rollout_bwd_f32 streams into the weight gradients of a SMALL network (what torch autograd does with one mm per
 * parameter in the backward of trainOC.py:173).  Two launches, deterministic.  Wider networks contract with library GEMMs.
 *   A device [K, m], B device [K, n] row-major;  C device [m, n];  accumulate != 0 adds to C
 *   scratch device [scratch_floats]: 4096 floats per workgroup and 64x64 output tile (up to 1024 of them, one workgroup per
 *           >= 256 rows and tile)
 */
int nocf_contract_f32(const float* A, const float* B, int64_t K, int32_t m, int32_t n, float* C, int32_t accumulate,
                      float* scratch, size_t scratch_floats, void* stream);

/*
 * out[n] (+)= column sums of X [K, n]: the bias, w and c.weight gradients are the sums of the adjoint's rows over every sample and
 * evaluation (torch autograd's sum-to-size in the backward of trainOC.py:173).  Two launches, fixed order (deterministic), reads
 * X once at HBM speed.  scratch device [scratch_floats]: n floats per row slice (up to 2048 slices of >= 128 rows).
 */
int nocf_colsum_f32(const float* X, int64_t K, int32_t n, float* out, int32_t accumulate,
                    float* scratch, size_t scratch_floats, void* stream);

/* Phi.getGrad -- replaces src/Phi.py:99-138.  s: device [n, d+1] -> grad: device [n, d+1] */
int nocf_phi_grad_f32(const NocfPhi* phi, const float* s, int64_t n, float* grad,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Phi.forward -- replaces src/Phi.py:91-96.  s: device [n, d+1] -> value: device [n] */
int nocf_phi_forward_f32(const NocfPhi* phi, const float* s, int64_t n, float* value,
                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * Problem physics on given (x, p) -- replaces calcLHQW / calcGradpH / calcCtrls of
 * src/problem/Cross2D.py:69-165, SwarmTraj.py:68-167, Quadcopter.py:65-174.
 *   x, p     device [n, d]
 *   lhqw     device [n, 4]   columns L, H, Q, W   (Q as the reference returns it: scaled by
 *                            alph_Q for Cross2D, un-scaled for SwarmTraj/Quadcopter)  (nullable)
 *   gradpH   device [n, d]                                                          (nullable)
 *   ctrls    device [n, a]                                                          (nullable)
 */
int nocf_prob_eval_f32(const NocfProb* prob, int32_t d, const float* x, const float* p, int64_t n,
                       float* lhqw, float* gradpH, float* ctrls, void* stream);

/*
 * Double precision -- the reference's `--prec double` (trainOC.py:76-79,96; evalOC.py:19,28-31): net, problem and states go
 * through .to(torch.float64) and the same OCflow (src/OCflow.py:7-95) runs.  Same arguments and layouts as nocf_rollout_f32 with
 * every buffer in double (alph: host [6] doubles; cost_sums: 7 column sums then n, as doubles).  Evaluation only (the adjoint is
 * fp32).  c.bias is read on the device (cb_dev is required).  workspace: nocf_workspace_bytes_f64(d, m, nTh) bytes.
 */
typedef struct NocfPhi64 {
    int32_t d, m, nTh, r;
    const double* K0;    /* device [m, d+1]      */
    const double* b0;    /* device [m]           */
    const double* K;     /* device [nTh-1, m, m] */
    const double* b;     /* device [nTh-1, m]    */
    const double* w;     /* device [m]           */
    const double* A;     /* device [r, d+1]      */
    const double* cw;    /* device [d+1]         */
    const double* cb_dev;/* device [1]           */
} NocfPhi64;

typedef struct NocfProb64 {
    int32_t kind, obstacle, n_agents, training;
    double r, alph_Q, alph_W, mass, grav;
    const double* xtarget; /* device [d] */
} NocfProb64;

size_t nocf_workspace_bytes_f64(int32_t d, int32_t m, int32_t nTh);

int nocf_rollout_f64(const NocfPhi64* phi, const NocfProb64* prob,
                     const double* x, int64_t n,
                     double t0, double t1, int32_t nt, int32_t stepper,
                     const double* alph,
                     double* z_out, double* persample, double* cost_sums,
                     double* zFull, double* ctrlFull,
                     void* workspace, size_t workspace_bytes, void* stream);

/*
 * Training in double precision (`trainOC.py --prec double`, trainOC.py:44,76-79,172-174): the recording forward and the adjoint of the
 * discrete RK scheme, every tensor a double.  Same semantics, row streams and contractions as nocf_rollout_record_f32 /
 * nocf_rollout_bwd_f32 (rows = (nt * nstage + 2) * n; the caller zeroes the last n rows of Y, V, Ab, Gb and contracts in double);
 * any depth that fits the LDS, all problem classes, rk4 / rk1.
 *   s_all  device [nt * nstage, n, d+1];   hs  device [nt] step sizes (tk + h) - tk as the forward formed them
 */
int nocf_rollout_record_f64(const NocfPhi64* phi, const NocfProb64* prob, const double* x, int64_t n,
                            double t0, double t1, int32_t nt, int32_t stepper, const double* alph,
                            double* z_out, double* persample, double* cost_sums, double* s_all,
                            void* workspace, size_t workspace_bytes, void* stream);
int nocf_rollout_bwd_f64(const NocfPhi64* phi, const NocfProb64* prob, int64_t n, int32_t nt, int32_t stepper, double t1,
                         const double* alph, double inv_n, const double* s_all, const double* z_final, const double* hs,
                         double* Y, double* Ob, double* V, double* Ab, double* Qb, double* U0, double* Wb, double* Gb, double* Sx,
                         double* PHIb, double* lam0, void* workspace, size_t workspace_bytes, void* stream);

/* Phi.forward (src/Phi.py:91-96) and Phi.getGrad (:99-138) in double: s device [n, d+1] -> value device [n] (nullable),
 * grad device [n, d+1] (nullable; at least one of the two) */
int nocf_phi_f64(const NocfPhi64* phi, const double* s, int64_t n, double* value, double* grad,
                 void* workspace, size_t workspace_bytes, void* stream);

/* calcLHQW / calcGradpH / calcCtrls in double: the arguments of nocf_prob_eval_f32 with double buffers */
int nocf_prob_eval_f64(const NocfProb64* prob, int32_t d, const double* x, const double* p, int64_t n,
                       double* lhqw, double* gradpH, double* ctrls, void* stream);

/*
 * Direct-transcription baseline -- replaces baseline2D.py:42-107 (loss_fun, trainBaseline) and the report loop of
 * baseline2D.py:136-150 / compareCorridor.py:95-113, for B independent initial points at once (one workgroup each).
 * Point-agent problems only (Cross2D, SwarmTraj: z' = u); a Quadcopter returns NOCF_E_PROB.  h = 1/nt; prob->training selects
 * the train / eval thresholds like every other entry point.  For one point z0 and controls U [nt, d]:
 *     z_{i+1} = z_i + h U_i ,   J = sum_i h L(z_{i+1}, U_i) + alphG |z_nt - xtarget|^2 / 2        (L = calcLHQW(z, p = U_i))
 * Limits: 1 <= nt <= 256 and U, z, dJ/dU of one point (and the Adam moments) in the 160 KiB of LDS:
 *     (5 nt d + d + 3 nt) floats (eval: 3 nt d + ...) plus 3 KiB / 12 KiB of partial sums (256 / 1024 lanes, the latter when
 *     nt * n_agents >= 512) -- swarm50 (d = 150) up to nt = 50.  Past the limits: NOCF_E_SHAPE.
 * Deterministic: no atomics, no dependence between workgroups; a point's result does not depend on B.
 *
 * nocf_baseline_eval_f32: the objective of every point, optionally its gradient, the report and the trajectory.
 *   z0       device [B, d]          initial states
 *   U        device [B, nt, d]      controls
 *   loss     device [B]             J
 *   grad     device [B, nt, d]      dJ/dU                                                               (nullable)
 *   report   device [B, 5]          L+G, L, G, Q, W of the report loop: L(z_j, U_j) at the state BEFORE
 *                                   the step, sums of h L, h Q, h W, G = alphG |z_nt - xtarget|^2 / 2;
 *                                   Q as calcLHQW returns it (scaled by alph_Q for Cross2D only)       (nullable)
 *   traj     device [B, d, nt+1]    z_0 .. z_nt                                                         (nullable)
 *
 * nocf_baseline_adam_f32: niters iterations of trainBaseline in ONE launch: evaluate J(U); if J < best_loss keep U in Ubest;
 * take torch's single-tensor Adam step (weight decay 0, constant lr; bias corrections formed in double from step0 + 1 on).
 *   U, m, v      device [B, nt, d]  iterate and Adam moments, read and written back (fresh solve: m = v = 0, step0 = 0)
 *   best_loss    device [B]         best J so far, read and written (fresh solve: +inf)
 *   Ubest        device [B, nt, d]  the iterate that reached best_loss (written when J improves)
 *   loss_hist    device [B, niters] J of every iteration                                                (nullable)
 *   step0        Adam steps already taken: a solve split into launches of k and niters - k iterations
 *                (the second with step0 = k) gives the bits of one launch
 */
int nocf_baseline_eval_f32(const NocfProb* prob, int32_t d, int64_t B, int32_t nt, double alphG,
                           const float* z0, const float* U, float* loss, float* grad, float* report, float* traj,
                           void* stream);
int nocf_baseline_adam_f32(const NocfProb* prob, int32_t d, int64_t B, int32_t nt, double alphG,
                           double lr, double beta1, double beta2, double eps, int32_t step0, int32_t niters,
                           const float* z0, float* U, float* m, float* v, float* best_loss, float* Ubest,
                           float* loss_hist, void* stream);

/*
 * Quadcopter baseline -- replaces baselineQuad.py (compute_loss, trainBaseline: torch.optim.LBFGS with the strong-Wolfe line
 * search, and the report loop that follows it) for B independent starts of ONE quadcopter (d = 12) at once, one 64-lane workgroup
 * each.  prob must be a Quadcopter (else NOCF_E_PROB) with d = 12 (else NOCF_E_SHAPE); mass, grav and xtarget come from it, alph_Q
 * and alph_W are ignored as the reference ignores them.  h = 1/nt.  For one start x0 and controls U [nt, 4]:
 *     x_{i+1} = x_i + h [v, w, (u0/mass) f7(a), (u0/mass) f8(a), (u0/mass) f9(a) - grav, u1:4]   (x = [p, a, v, w], Quadcopter.f)
 *     J = sum_i h (2 + |U_i|^2) + alphG |x_nt - xtarget|^2 / 2
 * Limits: 1 <= nt <= NOCF_BLQ_MAX_NT and 1 <= history_size <= NOCF_BLQ_MAX_HISTORY (the L-BFGS vectors are held in registers,
 * ceil(4 nt / 64) floats per lane each; LDS (4 nt + 4 nt + 12 (nt+1) + 6 nt + 3 nt + 3 nt + 3 (nt+1) + nt + 8 + 2 history) floats,
 * at most 45 KiB); past them, or B < 1: NOCF_E_SHAPE before any launch.  Deterministic: no atomics, no dependence between
 * workgroups; a start's result does not depend on B.
 *
 * nocf_baseline_quad_eval_f32: the objective of every start, optionally its gradient, the report and the trajectory.
 *   z0       device [B, 12]          initial states
 *   U        device [B, nt, 4]       controls
 *   loss     device [B]              J
 *   grad     device [B, nt, 4]       dJ/dU (the adjoint of the Euler scheme)                               (nullable)
 *   report   device [B, 3]           L+G, L, G as the reference's final loop prints them                  (nullable)
 *   traj     device [B, 12, nt+1]    x_0 .. x_nt                                                          (nullable)
 *
 * nocf_baseline_quad_lbfgs_f32: one whole torch.optim.LBFGS.step(closure) per start in ONE launch (line_search_fn
 * "strong_wolfe", lbfgs.py of torch 2.x mirrored step for step), from U.  max_iter = 0: a no-op returning 0.  max_eval >= 1.
 *   U           device [B, nt, 4]    in: the initial controls; out: the final iterate (torch leaves the last accepted point)
 *   loss        device [B]           J of the final iterate
 *   n_iter      device int32 [B]     iterations taken (torch's state["n_iter"] after one step)
 *   n_evals     device int32 [B]     objective evaluations (torch's state["func_evals"])
 *   reason      device int32 [B]     the exit that fired: NOCF_LB_*
 *   workspace   device, >= nocf_baseline_quad_workspace_bytes(B, nt, history_size) bytes (the history pairs), given in
 *               workspace_bytes (too small: NOCF_E_WORKSPACE)
 */
#define NOCF_BLQ_MAX_NT 256
#define NOCF_BLQ_MAX_HISTORY 1024
#define NOCF_LB_GRAD_AT_START 1     /* max |g| <= tolerance_grad at the initial point (n_iter = 0) */
#define NOCF_LB_GTD           2     /* directional derivative > -tolerance_change                   */
#define NOCF_LB_MAX_ITER      3     /* n_iter == max_iter                                           */
#define NOCF_LB_MAX_EVAL      4     /* func_evals >= max_eval                                       */
#define NOCF_LB_GRAD          5     /* max |g| <= tolerance_grad                                    */
#define NOCF_LB_STEP          6     /* max |t d| <= tolerance_change                                */
#define NOCF_LB_LOSS          7     /* |loss - prev_loss| < tolerance_change                        */
/* bytes of the L-BFGS workspace: 2 history_size 4 nt floats per start; 0 when an argument is out of range */
size_t nocf_baseline_quad_workspace_bytes(int64_t B, int32_t nt, int32_t history_size);
int nocf_baseline_quad_eval_f32(const NocfProb* prob, int32_t d, int64_t B, int32_t nt, double alphG,
                                const float* z0, const float* U, float* loss, float* grad, float* report, float* traj,
                                void* stream);
int nocf_baseline_quad_lbfgs_f32(const NocfProb* prob, int32_t d, int64_t B, int32_t nt, double alphG, double lr,
                                 int32_t max_iter, int32_t max_eval, double tolerance_grad, double tolerance_change,
                                 int32_t history_size, const float* z0, float* U, float* loss, int32_t* n_iter,
                                 int32_t* n_evals, int32_t* reason, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The two baselines in double precision (the reference's --prec double): the argument lists of the _f32 functions with double
 * buffers and a NocfProb64 (xtarget as doubles), the same semantics, error codes, NOCF_LB_* reasons and determinism.  What differs:
 *   - direct transcription: U, z and dJ/dU of one point live in LDS as doubles, (3 nt d + d + 3 nt + 8) doubles plus 6 KiB / 24 KiB of
 *     partial sums; the Adam moments do not (registers, or the m / v arrays themselves), so both entry points share one limit:
 *     nocf_baseline_max_nt(prob, d, adam, 8) -- swarm (d = 96) up to nt = 59, swarm50 (d = 150) up to nt = 38.
 *   - quadcopter: the fp32 kernels' source instantiated for double (csrc/nocf_baseline_quad.inc); every scalar of torch.optim.LBFGS
 *     is a double; the workspace holds doubles (twice the bytes).
 *
 * nocf_baseline_max_nt: the largest nt nocf_baseline_eval_* (adam = 0) / nocf_baseline_adam_* (adam != 0) accept for this problem,
 * for elem_bytes = 4 (the _f32 entry points) or 8 (_f64); every nt from 1 to it is accepted, every larger one returns NOCF_E_SHAPE
 * before any launch.  Only kind and n_agents of prob are read.  < 0: NOCF_E_* (a quadcopter: NOCF_E_PROB; elem_bytes: NOCF_E_SHAPE).
 */
int nocf_baseline_max_nt(const NocfProb* prob, int32_t d, int32_t adam, int32_t elem_bytes);
int nocf_baseline_eval_f64(const NocfProb64* prob, int32_t d, int64_t B, int32_t nt, double alphG,
                           const double* z0, const double* U, double* loss, double* grad, double* report, double* traj,
                           void* stream);
int nocf_baseline_adam_f64(const NocfProb64* prob, int32_t d, int64_t B, int32_t nt, double alphG,
                           double lr, double beta1, double beta2, double eps, int32_t step0, int32_t niters,
                           const double* z0, double* U, double* m, double* v, double* best_loss, double* Ubest,
                           double* loss_hist, void* stream);
/* bytes of the double-precision L-BFGS workspace: 2 history_size 4 nt doubles per start; 0 when an argument is out of range */
size_t nocf_baseline_quad_workspace_bytes_f64(int64_t B, int32_t nt, int32_t history_size);
int nocf_baseline_quad_eval_f64(const NocfProb64* prob, int32_t d, int64_t B, int32_t nt, double alphG,
                                const double* z0, const double* U, double* loss, double* grad, double* report, double* traj,
                                void* stream);
int nocf_baseline_quad_lbfgs_f64(const NocfProb64* prob, int32_t d, int64_t B, int32_t nt, double alphG, double lr,
                                 int32_t max_iter, int32_t max_eval, double tolerance_grad, double tolerance_change,
                                 int32_t history_size, const double* z0, double* U, double* loss, int32_t* n_iter,
                                 int32_t* n_evals, int32_t* reason, void* workspace, size_t workspace_bytes, void* stream);

/* Measurement hooks (bench.py): between begin and end every nocf_rollout_f32 call records a pair
 * of HIP events on its launch stream immediately around the rollout kernel; end synchronises on
 * them and returns the summed kernel time and the number of launches.  Not thread-safe. */
int nocf_profile_begin(void);
int nocf_profile_end(double* total_ms, int32_t* launches);

/* Diagnostic builds (-DNOCF_STAMPS, libnocf_stamps.so) only: device buffer of 12 uint64 per
 * workgroup receiving per-phase shader-cycle totals.  The production library returns an error. */
int nocf_debug_set_stamp_buffer(void* device_buf);
/* diagnostic builds only: [8 waves][64 points] shader-clock timeline of one evaluation of the adjoint kernel */
int nocf_debug_set_timeline_buffer(void* device_buf);

/* layout probe used by the tests: D = sum_k A_k B_k through the same 4x4x1 MFMA tile code
 * the rollout uses.  a: device [4, K], b: device [K, 64] -> out: device [4, 64] */
int nocf_selftest_mfma(const float* a, const float* b, int32_t K, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NOCF_H */
