/*
 * mmf.h -- C ABI of libmmf_hip.so, the MI355X (gfx950) filter hot path.
 *
 * Drop-in boundary for brentyi/multimodalfilter's batched filter recursions.  The
 * reference is pure Python; the interface each entry point replaces is the sequence of
 * stock torch ops at the cited lines (reference paths are relative to
 * /root/reference/).  The reference-side binding is a ctypes
 * stub; multimodalfilter_amd/_abi.py is that stub in this repo.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer valid on the current HIP device unless marked
 *     "host"; arrays are contiguous fp32 unless stated; N = trajectories, M = particles
 *     per trajectory, d = state_dim (1..4), rows R = N*M
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work
 *   - return value: 0 on success, a hipError_t (>0) from the runtime, or a negative
 *     MMF_E* code for argument errors; no allocation, no global state, re-entrant per
 *     stream; the caller owns every buffer
 *   - nothing here has a CPU fallback: without a GPU the launch fails with a hipError_t
 */
#ifndef MMF_H
#define MMF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMF_ABI_VERSION 42

#define MMF_EINVAL (-1)      /* bad argument (null pointer, d out of range, ...) */
#define MMF_ETOOLARGE (-2)   /* size beyond what the kernel supports (see each call) */

#define MMF_UNITS 64         /* hidden width of every per-particle layer (layers.py: units=64) */
#define MMF_MAX_RES 3        /* residual blocks after the join layer (LDS: 3 -> 149.5 KiB) */
#define MMF_MAX_STATE_DIM 4

/* The device status word: ONE int32 per device that the host hands to every call as `range_flag` (or null). Kernels only
 * ever OR into it; the host reads it (one 4-byte copy) where a result is about to be used, and clears what it consumed.
 *   MMF_FLAG_RANGE    OR-ed by an MMF_PREC_F16X3 kernel whose operand left the range in which the two-half f16
 *                     split is exact (|x| >= 65504: the result is finite but wrong -- re-run with MMF_PREC_F32); never
 *                     written by MMF_PREC_F32 launches.  Consumed by the host's check at the end of a forward_loop / step.
 *   MMF_FLAG_GAVE_UP  OR-ed by a persistent launch (mmf_pf_forward_loop, mmf_ekf_forward_loop, mmf_lstm_forward with
 *                     `persistent`) when a hand-off's bounded spin ran out because a workgroup of the launch was not
 *                     resident: every output of that call is to be discarded.  Consumed by the host right after the call,
 *                     which restores the call's in-place inputs and runs it again as launches.
 *   MMF_FLAG_NOT_PD   never OR-ed by a kernel of this library: the host ORs it in while it captures a training step (no
 *                     host read there) when initialize_beliefs met a covariance that is not positive definite; consumed
 *                     after the replay.
 * The value 2 is unused. */
#define MMF_FLAG_RANGE 1
#define MMF_FLAG_GAVE_UP 4
#define MMF_FLAG_NOT_PD 16

/* arithmetic of the 64x64 layers of the per-particle networks (K2) */
#define MMF_PREC_F32 0    /* v_mfma_f32_32x32x2_f32: exact fp32 products                        */
#define MMF_PREC_BF16 2   /* mmf_image_encoder only: operands rounded to ONE bf16, one v_mfma_*_bf16 per
                           * product, f32 accumulate (BASELINE config 5's "bf16 measurement CNN on MFMA")   */
#define MMF_PREC_F16X3 1  /* operands split x = hi + lo (2 x f16, exact to 2^-22), products
                             hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16, fp32 accumulate   */
#define MMF_PREC_F16X3_DUAL 3 /* mmf_pack_particle_net only (ABI 37): the f16x3 halves of every 64x64 layer as ONE
                             row-major, XOR-swizzled LDS image [out row][hi 64 | lo 64] that serves BOTH the forward
                             product (row reads, ds_read_b128) and the transposed product of the backward
                             (ds_read_b64_tr_b16): the fused training kernel keeps one copy of the weights in LDS.
                             Same blob size and section offsets as the other precisions */

int mmf_version(void);

/* ---------------------------------------------------------------- K1: reweight + resample
 * Replaces the post-measurement half of torchfilter.ParticleFilter.forward (external
 * dependency; call sites crossmodal/eval_helpers.py:139-142):
 *     logw += loglik; logw -= logsumexp(logw); estimate = sum exp(logw) x;
 *     indices ~ resample(logw); states = gather(states, indices); logw = -log(M_out)
 * as ONE kernel, one workgroup per trajectory: DPP wave reductions / scans, an integer
 * (fixed-point, 2^-24 of the row max) CDF, then systematic (mode 1: search-free -- every run of
 * particles announces the first output it owns, ancestors = prefix maximum of the announcements)
 * or multinomial (mode 2: binary search in LDS) selection.  The integer CDF makes the indices
 * independent of the scan order: bit-exact against oracle/resample.py.
 *
 *  loglik      (N, M)          measurement log-likelihoods
 *  logw_in     (N, M)          current log-weights; modes 1/2: null = uniform -log M (nothing is read)
 *  states_in   (N, M, d)
 *  u           mode 1: (N) uniforms in [0,1); mode 2: (N, M_out); mode 0: ignored (may be null)
 *  estimate    (N, d)          weighted-mean state estimate (always written)
 *  states_out  (N, M_out, d)   mode 1/2: resampled particles; must NOT alias states_in.
 *                              mode 0: may be null or alias states_in (no copy when it does)
 *  logw_out    (N, M_out)      mode 0: normalised log-weights (may alias logw_in);
 *                              mode 1/2: -log(M_out) (may alias logw_in when M_out == M); null = not
 *                              written (the survivors' weights are uniform by definition)
 *  indices_out (N, M_out) int32 ancestor indices, or null
 *  mode        0 none, 1 systematic, 2 multinomial
 * Limits: d <= 4; M, M_out <= 65536; mode 0 stages 4 B/particle in LDS (M <= 40,800),
 *         modes 1/2 keep the 8-byte CDF there (M <= 20,400: mmf_pf_reweight_resample_lds_bytes(M, mode)
 *         <= 160 KiB); larger -> MMF_ETOOLARGE.  Plain systematic resampling of M, M_out <= 20,000 takes
 *         the search-free kernel, everything else the CDF-search kernel.
 */
int mmf_pf_reweight_resample(const float* loglik, const float* logw_in, const float* states_in,
                             const float* u, float* estimate, float* states_out,
                             float* logw_out, int32_t* indices_out, int N, int M, int M_out,
                             int d, int mode, void* stream);

/* K1 with torchfilter's ``soft_resample_alpha`` option (upstream ParticleFilter._resample,
 * an option the reference leaves at its default 1.0): ancestors are drawn from the mixture
 * alpha * w + (1 - alpha) / M -- in fixed point, q'_i = ((A q_i << 8) + (2^24 - A) floor((Q << 8) / M)) >> 32
 * with A = floor(alpha 2^24) -- and the survivors carry the importance weights w / mixture, normalised,
 * instead of -log(M_out).  Same arguments as mmf_pf_reweight_resample; mode 1 or 2; 0 < alpha <= 1
 * (alpha == 1 is the plain resampler).
 */
int mmf_pf_reweight_resample_soft(const float* loglik, const float* logw_in, const float* states_in,
                                  const float* u, float* estimate, float* states_out,
                                  float* logw_out, int32_t* indices_out, int N, int M, int M_out,
                                  int d, int mode, float alpha, void* stream);

/* ABI 42.  K1 with the BELIEF RECORD of the step: the second moment, the effective sample size and the evidence increment of
 * the pre-resampling weighted set -- the set the weighted-mean estimate is taken from -- which upstream torchfilter leaves
 * to the caller (particle_states / particle_log_weights after every forward; the reference's vis_pf_likelihoods.ipynb).
 * With a_m = logw_in_m + loglik_m (logw_in null: uniform -log M), w_m = exp(a_m - logsumexp(a)), mu = sum_m w_m x_m:
 *   cov          (N, d, d)  sum_m w_m (x_m - mu)(x_m - mu)^T: full symmetric storage (symmetric bit for bit), no Bessel
 *                           factor -- the moment-matched Gaussian of the weighted set; about the weighted MEAN also where
 *                           estimation_method "argmax" reports another point
 *   ess          (N)        1 / sum_m w_m^2, in [1, M]
 *   log_evidence (N)        logsumexp_m(a_m): the step's increment of the log marginal likelihood estimate when logw_in is
 *                           normalised (every path of this library keeps it so)
 * each or null; all null = mmf_pf_reweight_resample (alpha == 1) / mmf_pf_reweight_resample_soft, same kernels: the
 * recording is a template flag of both K1 kernels, so the non-recording instantiations are the ones without it.
 * Arithmetic (fp32, one pass next to the estimate's sums): moments about a PIVOT, the first highest-weight particle p --
 *   e_m = exp(a_m - max), S = sum e, m1 = sum e (x - p), M2 = sum e (x - p)(x - p)^T, cov = M2 / S - (m1 / S)(m1 / S)^T,
 *   ess = S^2 / sum e^2, log_evidence = max + log S
 * -- chosen over a second pass about the fp32 mean because pass 1 already finds the maximum and the rows are in registers
 * when the estimate is accumulated (no second sweep, no re-read).  Raw moments E[x x^T] - mu mu^T lose a 1e-3-wide
 * cloud of O(1) states entirely in fp32; a fixed pivot fails once the weight sits far from it.  The sums follow the
 * estimate's partition rule (csrc/pf_resample_systematic.inc), so every form of K1 -- launch, persistent loop -- gives the
 * same bits.  A particle with a_m = -inf contributes exactly zero.  The opt-in cluster form does not record: a recording
 * call takes the one-workgroup kernels.
 * Limits: as mmf_pf_reweight_resample, less the record's reduction rows in LDS: M <= 20,200 (modes 1/2) / 40,500 (mode 0),
 *         larger -> MMF_ETOOLARGE.  mode 0 takes alpha == 1 only. */
int mmf_pf_reweight_resample_belief(const float* loglik, const float* logw_in, const float* states_in,
                                    const float* u, float* estimate, float* states_out,
                                    float* logw_out, int32_t* indices_out, int N, int M, int M_out,
                                    int d, int mode, float alpha, float* cov, float* ess,
                                    float* log_evidence, void* stream);

/* K1 with ESS-TRIGGERED (adaptive) resampling: a trajectory resamples only when its effective sample size has dropped below
 * a fraction of M, and otherwise carries its weights forward (the estimator between upstream's resample-always and
 * resample-never).  Purely additive to ABI 42: two new symbols (this one and mmf_pf_forward_loop_adaptive), no struct layout
 * changes, so MMF_ABI_VERSION stays 42.  The one definition every form of K1 follows:
 *   - mode 1 or 2, M_out == M, optional soft alpha, ess_threshold in (0, 1]
 *   - ess_n is the fp32 value the belief record reports (mmf_pf_reweight_resample_belief: S^2 / sum e^2 -- the same sums,
 *     the same partition rule, the same bits)
 *   - trajectory n RESAMPLES iff !(ess_n >= ess_threshold * (float)M), the product rounded once in fp32: a NaN ESS resamples
 *     (what a degenerate row does today), a tie keeps (uniform weights with ess_threshold == 1 keep)
 *   - a resampling trajectory produces bit for bit what mmf_pf_reweight_resample_belief produces with that mode / alpha:
 *     states_out, logw_out (-log M, or the soft importance weights), indices_out
 *   - a KEPT trajectory: states_out is a bit copy of states_in, logw_out is bit for bit what mode 0 writes for the same
 *     inputs, indices_out is 0 .. M-1
 *   - estimate and the record (cov, ess, log_evidence) are those of the pre-resampling set on both branches, unchanged
 *   - the uniforms `u` of a step are consumed whether or not a trajectory uses them ((N) / (N, M) as the mode says), so the
 *     noise stream of a run does not depend on its decisions and results stay shard-invariant
 *  logw_in     null = uniform (plain resampling only, as above)
 *  logw_out    required (a kept trajectory's weights are not uniform), must not alias logw_in
 *  resampled   (N) int32 1 / 0, or null
 * The decision is workgroup-uniform -- taken from the broadcast totals of S and sum e^2 after pass 2's reductions -- and a kept
 * trajectory leaves before the announcements / search and the gather.  A template flag of both K1 kernels, as the record is:
 * the instantiations without it are the ones that existed before.  Sum e^2 is reduced through the record's rows in LDS whether
 * or not a record is requested, so the size limits are those of a recording call.  The cluster form does not do adaptive.
 * MMF_EINVAL: mode 0, null logw_out / states_out / u, in-place gather, ess_threshold <= 0, > 1 or NaN, alpha outside (0, 1];
 * N == 0 is a successful no-op. */
int mmf_pf_reweight_resample_adaptive(const float* loglik, const float* logw_in, const float* states_in,
                                      const float* u, float* estimate, float* states_out,
                                      float* logw_out, int32_t* indices_out, int N, int M, int d, int mode,
                                      float alpha, float ess_threshold, int32_t* resampled, float* cov,
                                      float* ess, float* log_evidence, void* stream);

/* Belief initialisation (replaces torchfilter's ParticleFilter.initialize_beliefs; call site
 * eval_helpers.py:125-131): states[n][m] = mean[n] + chol(covariance[n]) eps[n][m], logw = -log M.
 *  mean (N, d), covariance (N, d, d), eps (N, M, d) standard normal -> states (N, M, d), logw (N, M)
 *  not_pd   device int32 or null: OR-ed with 1 when a covariance is not positive definite
 */
int mmf_pf_init_particles(const float* mean, const float* covariance, const float* eps, float* states,
                          float* logw, int32_t* not_pd, int N, int M, int d, void* stream);

/* K6: backward of the no-resample step (mode 0 of mmf_pf_reweight_resample):
 *   a = logw_in + loglik, logw_out = a - logsumexp_m(a), estimate = sum_m exp(logw_out) x_m.
 *  logw_out (N, M) as returned by the forward, states (N, M, d), g_estimate (N, d),
 *  g_logw_out (N, M) or null -> d_a (N, M) (= d loglik = d logw_in), d_states (N, M, d)
 */
int mmf_pf_reweight_backward(const float* logw_out, const float* states, const float* g_estimate,
                             const float* g_logw_out, float* d_a, float* d_states, int N, int M, int d,
                             void* stream);

/* Dynamic LDS bytes K1 will request for (M, mode) -- for occupancy planning / tests. */
size_t mmf_pf_reweight_resample_lds_bytes(int M, int mode);

/* ABI 39.  K1 for few trajectories ("for N < 256 split M across a WG-cluster"): with `enabled` != 0, plain
 * systematic resampling (mode 1) of N <= CUs / 2 trajectories of M = M_out <= 4096 particles (M a multiple of 512, d = 2 or 3)
 * gives every trajectory a CLUSTER of workgroups that meet twice through L2 (csrc/pf_resample_cluster.inc).  Same bits as
 * the one-workgroup kernel -- ancestors, gathered particles and estimates (tests/test_gpu_kernels.py).  OFF by default: measured
 * no faster (11.6 against 11.2 us per launch at 32 x 4096, profiles/r06/k1_cluster_ab.txt -- K1 at these sizes is one
 * thread's instruction chain plus memory round trips, which more workgroups do not shorten). */
void mmf_pf_set_resample_cluster(int enabled);
int mmf_pf_get_resample_cluster(void);

/* ---------------------------------------------------------------- K2: per-particle networks
 * The reference evaluates its dynamics and measurement MLPs as ~20 stock nn.Linear launches
 * over R = N*M rows, materialising (R, 64) activations after every layer and repeating the
 * control / observation features per particle (crossmodal/door_models/dynamics.py:102-134,
 * door_models/pf.py:63-107, push mirrors).  Both networks share one shape:
 *
 *   enc  : Linear(d -> 64), ReLU, ResLinear(64)                (layers.py:11-24)
 *   join : Linear(64*(1+k) -> 64) on cat(per-trajectory features, enc)  [+ ReLU for the
 *          measurement model]; the per-trajectory half is hoisted: the caller passes
 *          traj_bias (N, 64) = W[:, traj cols] @ traj_features + b
 *   res  : n_res x ResLinear(64)                               (3 dynamics, 2 measurement)
 *   head : Linear(64 -> n_out)                                 (d+1 dynamics, 1 measurement)
 *
 * The kernels keep every activation in registers: a wave owns 64 particles as the N
 * (lane) dimension of v_mfma_f32_32x32x2_f32 tiles, the accumulator tile of one layer is
 * the B operand of the next with no data movement, and a network's weights (<= 149 KiB,
 * fragment-ordered by mmf_pack_particle_net) live in LDS for the whole launch.
 */
typedef struct MmfParticleNetDesc {
  int32_t d_in;             /* state_dim: 1..4                                            */
  int32_t n_res;            /* residual blocks after the join layer: 0..MMF_MAX_RES       */
  int32_t relu_after_join;  /* 0 dynamics (dynamics.py:29-35), 1 measurement (pf.py:54-55) */
  int32_t n_out;            /* head width: 1..MMF_MAX_STATE_DIM+1                         */
  int32_t join_in;          /* row length of w_join (128, 192 or 256)                     */
  int32_t join_state_off;   /* first column of the state-feature block inside w_join      */
  const float* w_in;        /* (64, d_in)   enc Linear                                    */
  const float* b_in;        /* (64)                                                       */
  const float* w_enc[2];    /* (64, 64) x2  enc ResLinear block1, block2                  */
  const float* b_enc[2];    /* (64) x2                                                    */
  const float* w_join;      /* (64, join_in); only columns [off, off+64) are packed       */
  const float* w_res[2 * MMF_MAX_RES]; /* (64,64): block1, block2 of each residual block  */
  const float* b_res[2 * MMF_MAX_RES];
  const float* w_head;      /* (n_out, 64)                                                */
  const float* b_head;      /* (n_out)                                                    */
} MmfParticleNetDesc;       /* host struct holding device pointers (torch Linear layout)  */

/* Number of floats of a packed network blob with `n_res` residual blocks. */
size_t mmf_particle_net_floats(int n_res);

/* Re-order a network's weights into MFMA-fragment order (device -> device) for `precision`
 * (MMF_PREC_*); the blob size does not depend on it, the blob must be used with the same value. */
int mmf_pack_particle_net(const MmfParticleNetDesc* desc /* host */, float* packed, int precision,
                          void* stream);

/* x' = x + dir(x) * sigmoid(gate(x)) + L eps      (dynamics.py:102-134 + the reparameterised
 * MultivariateNormal(loc, scale_tril).rsample() of torchfilter's PF step)
 *  packed      blob from mmf_pack_particle_net (n_out must be d+1)
 *  states_in   (N*M, d)
 *  traj_bias   (N, 64)      hoisted control half of shared_layers[0] (+ its bias)
 *  noise       (N*M, d) standard normal, or null (EKF predict / open-loop rollouts)
 *  scale_tril  (d, d) row-major lower-triangular, shared by all rows (ignored if noise null)
 *  states_out  (N*M, d)     may alias states_in
 *  range_flag  int32 on the device or null; MMF_PREC_F16X3 ORs MMF_FLAG_RANGE into it when an activation
 *              exceeded the f16-split range (|x| >= 65504: the result is finite but wrong --
 *              re-run with MMF_PREC_F32); never written otherwise
 */
int mmf_pf_dynamics(const float* packed, int n_res, int precision, const float* states_in,
                    const float* traj_bias, const float* noise, const float* scale_tril,
                    float* states_out, int32_t* range_flag, int N, int M, int d, void* stream);

/* One modality's log-likelihood and its crossmodal combination
 * (pf.py:63-107 + base_models/crossmodal_pf.py:106-139):
 *      ll = net(x) + (modality_logw ? modality_logw[n * logw_stride] : 0)
 *      combine 0: loglik = ll          combine 1: loglik = log(exp(loglik) + exp(ll))
 * Calling it once per enabled modality with combine = 0, 1, 1, ... gives
 * logsumexp_k(log beta_k + ll_k).
 *  states (N*M, d); traj_bias (N, 64); loglik (N*M) in/out
 */
int mmf_pf_measure(const float* packed, int n_res, int precision, const float* states, const float* traj_bias,
                   const float* modality_logw, int logw_stride, float* loglik, int combine,
                   int32_t* range_flag, int N, int M, int d, void* stream);

/* `count` modalities' own log-likelihoods (combine 0 each) of the SAME particles in one launch (blockIdx.y = modality):
 * the training forward keeps every modality's log-likelihood for the backward's softmax over modalities
 * (base_models/crossmodal_pf.py:106-139), and at the reference's training size a launch is one tile per wave.
 *  packed, traj_bias, modality_logw (entries may be null), loglik: HOST arrays of `count` device pointers */
int mmf_pf_measure_multi(const float* const* packed, int count, int n_res, int precision, const float* states,
                         const float* const* traj_bias, const float* const* modality_logw, int logw_stride,
                         float* const* loglik, int32_t* range_flag, int N, int M, int d, void* stream);

/* Forward-mode Jacobian of the dynamics network (replaces torchfilter's default autograd
 * DynamicsModel.jacobian: batch replicated d times + one autograd.grad):
 *  states_in (N, d), traj_bias (N, 64) -> states_out (N, d), jac (N, d, d), jac[n][i][j] = d x'_i / d x_j
 *  precision: of `packed` (mmf_pack_particle_net); f16x3: the tangent columns are operands like any
 *  other (signed: their splits mask the sign for the range tracking), range_flag as in mmf_pf_dynamics
 */
int mmf_dynamics_jacobian(const float* packed, int n_res, int precision, const float* states_in,
                          const float* traj_bias, float* states_out, float* jac, int32_t* range_flag,
                          int N, int d, void* stream);

/* K independent Jacobian problems of one shape in ONE launch (the sub-filters of a fused EKF):
 * states_in / states_out (K, N, d), jac (K, N, d, d); packed[k], traj_bias[k] per problem.
 */
int mmf_dynamics_jacobian_multi(const float* const* packed, int n_res, int precision,
                                const float* states_in, const float* const* traj_bias,
                                float* states_out, float* jac, int32_t* range_flag, int K, int N,
                                int d, void* stream);

/* ---------------------------------------------------------------- K6: training through the per-particle networks
 * Replaces autograd through DoorDynamicsModel*.forward / DoorMeasurementModel.forward over N*M
 * rows (door_models/dynamics.py:102-134, door_models/pf.py:63-107; callers train_helpers.py via
 * torchfilter.train.*).  Exact fp32 (MMF_PREC_F32 blobs).
 *
 * forward:  out (R, NOUT) = head(network(states, traj_bias)) including the head bias, BEFORE the
 *           gate / noise / log-weight epilogue of mmf_pf_dynamics / mmf_pf_measure (NOUT = d + 1
 *           for kind 0 = dynamics, 1 for kind 1 = measurement), and
 *           stash (NL + 1, R, 64), NL = 3 + 2 n_res: [l] = input of 64x64 layer l, [NL] = head input.
 * backward: packed_t is a blob packed from the TRANSPOSED 64x64 layer weights (the state part of
 *           the join layer as a (64, 64) matrix; biases / first layer / head are ignored);
 *           head_w (NOUT, 64).  Writes dz (NL + 1, R, 64): [l] = gradient w.r.t. layer l's
 *           pre-activation output, [NL] = w.r.t. the first (d -> 64) layer's pre-activation,
 *           and d_states (R, d) = dz[NL] W_in (W_in is read from packed_t's first-layer section,
 *           which must hold the untransposed (64, d) weight).
 * Every reduction over particles is then a GEMM / column sum over the two stashes:
 *   dW_l = dz[l]^T stash[l], db_l = sum_rows dz[l], d traj_bias[n] = sum_m dz[2][n, m],
 *   dW_in = dz[NL]^T [states, 1], dW_head = d_out^T stash[NL].
 */
/* `mask` (NL + 1, R, 2) uint32: the sign bits of the stashed activations (bit 16 t + r of word h = feature
 * 32 t + (r & 3) + 8 (r >> 2) + 4 h), written by the forward, read by the backward's ReLU masks -- 8 B per
 * particle and layer where round 2 re-read the 256-B activation. */
int mmf_particle_net_train_forward(const float* packed, int n_res, int kind, const float* states,
                                   const float* traj_bias, float* stash, uint32_t* mask, float* out, int N, int M,
                                   int d, void* stream);
int mmf_particle_net_train_backward(const float* packed_t, const float* head_w, int n_res, int kind,
                                    const uint32_t* mask, const float* d_out, float* dz, float* d_states,
                                    int R, int d, void* stream);

/* dW_l = dz[l]^T stash[l] and db_l = column sums of dz[l] for l < n_layers, as per-slice partial
 * sums: partial_w (n_layers, n_splits, 64, 64), partial_b (n_layers, n_splits, 64); the caller
 * adds the n_splits slices (no float atomics).  dz, stash: (>= n_layers, R, 64).
 */
int mmf_particle_net_weight_grads(const float* dz, const float* stash, float* partial_w,
                                  float* partial_b, int n_layers, int R, int n_splits, void* stream);

/* The same, ADDING into the caller's partial sums when accumulate != 0 (each (layer, split) block of the
 * partials belongs to one workgroup: no atomics) -- the native training loop sums over time steps in place. */
int mmf_particle_net_weight_grads_acc(const float* dz, const float* stash, float* partial_w, float* partial_b,
                                      int n_layers, int R, int n_splits, int accumulate, void* stream);

/* The narrow reductions of the same backward in one pass over the rows (as GEMMs they are the
 * library's worst shapes, as torch reductions five passes over (R, 64) tensors):
 *   first layer   dW0[c][i]  = sum_r dz_first[r][c] states[r][i]          (64, d)
 *   head          dWh[o][c]  = sum_r d_out[r][o] h_last[r][c]             (n_out, 64),  dbh[o] = sum_r d_out[r][o]
 *   join layer    d traj_bias[n][c] = sum_m dz_join[n M + m][c]           (N, 64)
 * as per-slice partials over `n_slices` slices of every trajectory's M rows: p_first (N n_slices, 64, 4),
 * p_head (N n_slices, 4, 64), p_dout (N n_slices, 4), p_traj (N n_slices, 64); the caller adds the
 * slices.  dz_first, dz_join, h_last: (N M, 64); states (N M, d); d_out (N M, n_out); d, n_out <= 4.
 */
int mmf_particle_net_small_grads(const float* dz_first, const float* dz_join, const float* h_last,
                                 const float* states, const float* d_out, float* p_first, float* p_head,
                                 float* p_dout, float* p_traj, int N, int M, int d, int n_out,
                                 int n_slices, void* stream);

/* ---------------------------------------------------------------- K4: image encoder
 * Replaces observation_image_layers (crossmodal/door_models/layers.py:43-63;
 * push_models/layers.py:91-104, default variant): Conv 1->32 k5, ReLU, ResConv 32 k3,
 * Conv 32->16 k3, ReLU, Conv 16->8 k3, Flatten, Linear 8192->64, ReLU, ResLinear 64 --
 * as implicit-GEMM convolutions on v_mfma_f32_16x16x4_f32 with bias / skip / ReLU fused,
 * one launch per layer for ALL encoders of a step (they share the image, not the weights).
 */
typedef struct MmfImageEncoderDesc {
  const float* conv_w[5];   /* torch layouts: (32,1,5,5) (32,32,3,3) (32,32,3,3) (16,32,3,3) (8,16,3,3) */
  const float* conv_b[5];
  const float* fc_w;        /* (64, 8192) */
  const float* fc_b;        /* (64) */
  const float* res_w[2];    /* ResLinear(64): block1, block2 (64,64) */
  const float* res_b[2];
  int32_t variant;          /* MMF_ENCODER_DEFAULT, or MMF_ENCODER_SPANNING_POOL (the push virtual   */
                            /* sensor's stack, push_models/layers.py:43-65,77-90): conv_w[4] is     */
                            /* (2,16,3,3), then a full-height and a full-width average pool (2-wide) */
                            /* give 64 values and fc_w is (64, 64)                                   */
} MmfImageEncoderDesc;      /* host struct holding device pointers */
#define MMF_ENCODER_DEFAULT 0
#define MMF_ENCODER_SPANNING_POOL 1

size_t mmf_image_encoder_floats(void);                 /* floats of one packed encoder blob */
size_t mmf_image_encoder_workspace_bytes(int n_images, int n_nets);
int mmf_pack_image_encoder(const MmfImageEncoderDesc* desc /* host */, float* packed, void* stream);

/*  packed     host array of n_nets (1..4) device pointers to packed encoder blobs
 *  images     (N, 32, 32)        shared by every encoder
 *  feat       (n_nets, N, 64)    out
 *  workspace  >= mmf_image_encoder_workspace_bytes(N, n_nets) bytes of device memory
 *  range_flag int32 on the device or null: MMF_PREC_F16X3 ORs MMF_FLAG_RANGE into it when an activation
 *             left the f16-split range (see mmf_pf_dynamics)
 *  variant    MMF_ENCODER_*: the architecture every blob of this call was packed for
 *  precision  MMF_PREC_F32: every layer on the f32 MFMA, one launch per layer.  MMF_PREC_F16X3: split-f16
 *             products; stem + conv 32->32 and conv 32->32 + skip + conv 32->16 run as two fused,
 *             persistent kernels with the activations in LDS (csrc/image_encoder_fused.inc).
 *             MMF_PREC_BF16: the same two fused kernels with single bf16 products (94 % of the
 *             MACs); conv 16->8 and the linear tail stay f16x3.
  * f16x3 products (the default mode, and conv 16->8 + the linear layer of the bf16 mode): weights are
 * held as f16 fragments of 256 w (the split's "lo" half stays out of the f16 subnormals); |w| < 255.
 */
int mmf_image_encoder(const float* const* packed, int n_nets, const float* images, float* feat,
                      void* workspace, int32_t* range_flag, int precision, int variant, int N,
                      void* stream);

/* K6 for the image encoder's convolution stack (door_models/layers.py:43-58) -- what torch
 * autograd / MIOpen do under torchfilter.train.* (crossmodal/train_helpers.py:76-162).  One
 * encoder per call, exact fp32, MMF_ENCODER_DEFAULT only.
 *  mmf_image_convs_train_forward   images (N,32,32) -> a1 (N,32,32,32) stem, h (N,32,..) ResConv hidden,
 *                                  a2 (N,32,..) ResConv out, a3 (N,16,..), a4 (N,8,32,32) = input of the
 *                                  flatten + linear; `packed` = mmf_pack_image_encoder's blob.  precision
 *                                  MMF_PREC_F32: exact fp32 products; MMF_PREC_BF16 (BASELINE config 5's
 *                                  "bf16 measurement CNN"): the two 32->32 convolutions with bf16 products,
 *                                  conv 32->16 / 16->8 f16x3, stem fp32; MMF_PREC_F16X3: f16x3 throughout.
 *                                  The backward differentiates the exact network through the saved
 *                                  (rounded-forward) activations
 *  mmf_image_convs_train_backward  g_a4 -> pre-activation gradients g3 (N,16,..), g2, gh, g1 (N,32,..):
 *                                  the forward conv kernel on transposed + flipped weights
 *                                  (`packed_bwd` = mmf_pack_image_convs_backward), ReLU masks fused
 *  mmf_conv_weight_grads           dW[tap][co][ci] partials of one 3x3 layer from its output gradient g
 *                                  (N,co,32,32) and input act (N,ci,32,32): (co,ci) in {(32,32),(16,32),(8,16)};
 *                                  partial (n_blocks, 9, 32, 32) and the bias gradient's partial_b
 *                                  (n_blocks, 32) = sums of g per channel, both summed over dim 0 by the
 *                                  caller (one slot per workgroup; a workgroup walks half-images, so
 *                                  n_blocks <= 2N, 256 fills the chip).
 *                                  (co,ci) = (32,1): the 5x5 stem, act = images (N,32,32); the head of each
 *                                  partial slot holds dW1 as [co 32][tap 32] (25 taps live).
 *                                  dw (co, ci, k, k) / db (co), when given: the slots summed in ascending order into
 *                                  nn.Conv2d's own layout by a second launch (round 5; null: the caller sums)
 */
size_t mmf_image_convs_backward_floats(void);
int mmf_pack_image_convs_backward(const MmfImageEncoderDesc* desc, float* packed_bwd, void* stream);
int mmf_image_convs_train_forward(const float* packed, const float* images, float* a1, float* h,
                                  float* a2, float* a3, float* a4, int32_t* range_flag, int precision,
                                  int N, void* stream);
int mmf_image_convs_train_backward(const float* packed_bwd, const float* a1, const float* h,
                                   const float* a2, const float* a3, const float* g_a4, float* g1,
                                   float* gh, float* g2, float* g3, int N, void* stream);
int mmf_conv_weight_grads(const float* g, const float* act, float* partial, float* partial_b, int N, int co,
                          int ci, int n_blocks, float* dw, float* db, void* stream);

/* ABI 39.  mmf_image_convs_train_backward with the three layers that have 32 output channels (97 % of the MACs) on
 * v_mfma_f32_32x32x16_f16, three products per product: every gradient tensor is scaled by the power of two that brings its
 * largest magnitude to [2^14, 2^15) before its operand split and the result scaled back; masks, skip path and outputs as the
 * exact-fp32 form.  conv 16->8's gradient stays exact.  scratch (4 floats, device): max |g3|, max |g2|, max |gh|, max |g_a4| on
 * return -- reduced on the device (each launch leaves the next one's) -- the `g_absmax` words of mmf_conv_weight_grads_h. */
int mmf_image_convs_train_backward_h(const float* packed_bwd, const float* a1, const float* h,
                                     const float* a2, const float* a3, const float* g_a4, float* g1,
                                     float* gh, float* g2, float* g3, float* scratch, int N, void* stream);

/* ABI 39.  The same gradients of a 3x3 layer (co, ci) = (32, 32) | (16, 32) | (8, 16) on v_mfma_f32_32x32x16_f16 with the
 * three-product f16 split of both operands (csrc/image_encoder_train_h.inc): 54 MFMAs of 32 cycles per image row instead of
 * 144 of 64.  g_absmax: DEVICE scalar, the largest |g| (the caller reduces it first: no host read) -- g is multiplied by the
 * power of two that brings it to [2^14, 2^15) and the sums are multiplied back, so gradients of any magnitude keep their
 * leading bits; db is the exact fp32 sum.  range_flag (or null): OR-ed with MMF_FLAG_RANGE if an activation left the f16 range. */
int mmf_conv_weight_grads_h(const float* g, const float* act, const float* g_absmax, float* partial, float* partial_b,
                            int32_t* range_flag, int N, int co, int ci, int n_blocks, float* dw, float* db, void* stream);

/* ---------------------------------------------------------------- particle-filter step loop
 * Replaces the Python loop of torchfilter's Filter.forward_loop (call site
 * crossmodal/eval_helpers.py:139-142) for the fused models: one call enqueues the kernels of
 * all T steps (mmf_pf_dynamics, mmf_pf_measure per modality, mmf_pf_reweight_resample) on
 * `stream`.  Per-trajectory terms and randomness are indexed by step: row block t of every
 * (T*N, ...) array belongs to step t.
 */
#define MMF_LOOP_MAX_MEAS 4
typedef struct MmfPfLoopArgs {
  int32_t T, N, M, d;
  int32_t n_meas;            /* measurement networks (modalities), 1..MMF_LOOP_MAX_MEAS       */
  int32_t resample_mode;     /* 0 none, 1 systematic, 2 multinomial                           */
  int32_t precision;         /* MMF_PREC_*                                                    */
  int32_t n_res_dyn, n_res_meas;
  int32_t logw_stride;       /* row stride of the modality log-weight arrays                  */
  const float* dyn_packed;   /* packed dynamics network                                       */
  const float* dyn_bias;     /* (T*N, 64)                                                     */
  const float* meas_packed[MMF_LOOP_MAX_MEAS];
  const float* meas_bias[MMF_LOOP_MAX_MEAS];   /* (T*N, 64) each                              */
  const float* meas_logw[MMF_LOOP_MAX_MEAS];   /* first element of modality k's log-weight    */
                                               /* column in a (T*N, logw_stride) array, or null */
  const float* noise;        /* (T, N, M, d) standard normal                                  */
  const float* scale_tril;   /* (d, d)                                                        */
  const float* uniforms;     /* (T, N) systematic / (T, N, M) multinomial / null              */
  float* states_a;           /* (N, M, d) belief on entry                                     */
  float* states_b;           /* (N, M, d) scratch                                             */
  float* logw_a;             /* (N, M) log-weights on entry                                   */
  float* logw_b;             /* (N, M) scratch                                                */
  float* loglik;             /* (N, M) scratch                                                */
  float* estimates;          /* (T, N, d) out                                                 */
  int32_t* range_flag;       /* device status word or null (MMF_FLAG_*)                       */
  int32_t* final_location;   /* HOST int32 out or null: bit 0 belief states in states_b,      */
                             /* bit 1 log-weights in logw_b                                   */
  void* const* events;       /* HOST array of hipEvent_t or null: recorded around every launch */
                             /* of the sampled steps, [sample][dynamics, measure.., resample][start,end] */
  int32_t event_stride;      /* steps t with t % stride == stride / 2 are sampled (<= 1: every  */
                             /* step); `events` holds 2*(2+n_meas) entries per sampled step    */
  float* loglik_steps;       /* (T, N, M) or null: step t's fused log-likelihoods are kept here  */
                             /* instead of the shared `loglik` scratch (parity certificates)     */
  int32_t* indices_steps;    /* (T, N, M) int32 or null: ancestors drawn at every resampling step */
  uint64_t noise_seed;       /* noise_mode 2: key of the counter-based generator (include/mmf_philox.h)       */
  uint32_t noise_step0;      /* noise_mode 2: step t of the loop draws counter step noise_step0 + t          */
  uint32_t noise_traj0;      /* noise_mode 2: global index of this shard's first trajectory                  */
  int32_t noise_mode;        /* 0: `noise` tensor; 2: generated inside the dynamics kernel (`noise` may be null) */
  float soft_alpha;          /* 0 or 1: plain resampling; 0 < alpha < 1 (resample_mode != 0): torchfilter's soft      */
                             /* resampling (mmf_pf_reweight_resample_soft) -- the survivors carry importance weights, */
                             /* so every step reads and writes the log-weights                                        */
  int32_t estimate_argmax;   /* != 0: estimates = the particle with the largest pre-resampling weight                 */
                             /* (mmf_pf_argmax_estimate; torchfilter's estimation_method = "argmax")                  */
  float* estimate_scratch;   /* (N, d), needed with estimate_argmax: K1's weighted mean lands here instead            */
  int32_t persistent;        /* != 0: the whole loop as ONE persistent launch (small problems: mmf_pf_persistent_plan > 0; */
                             /* plain systematic resampling, weighted-average estimates, no events / per-step records).    */
                             /* Same results, bit for bit, as the launch-per-step loop.                                    */
  int32_t n_sync_words;      /* 4-byte words of sync_words (>= mmf_pf_persistent_sync_words(N, M, d, n_meas))              */
  uint32_t* sync_words;      /* persistent: device workspace of the in-launch hand-offs -- tagged 8-byte granules of the   */
                             /* particle rows and log-likelihoods --, zeroed by the call; an allocation of its own         */
  float* cov_steps;          /* ABI 42. (T, N, d, d) or null: every step's belief record (mmf_pf_reweight_resample_belief);  */
  float* ess_steps;          /* (T, N) or null                                                                             */
  float* log_evidence_steps; /* (T, N) or null.  Recording does not change eligibility for the persistent form, whose K1   */
                             /* workgroups write the records straight to these arrays; all null: the kernels without it    */
} MmfPfLoopArgs;             /* host struct holding device pointers                           */

int mmf_pf_forward_loop(const MmfPfLoopArgs* args /* host */, void* stream);

/* The step loop with ESS-triggered resampling (mmf_pf_reweight_resample_adaptive's definition, per trajectory and step).  The
 * threshold and the per-step decisions are arguments of this entry point so that MmfPfLoopArgs keeps its layout (ABI 42);
 * everything else is read from the unchanged struct: resample_mode (1 or 2; 0 -> MMF_EINVAL), soft_alpha, estimate_argmax,
 * loglik_steps / indices_steps, the belief records, persistent.  Every step reads and writes the log-weights (as soft
 * resampling makes the loop do), and final_location reports where they ended up.  The persistent form (same eligibility:
 * plain systematic resampling, weighted-average estimates, mmf_pf_persistent_plan > 0) takes the adaptive branch in its K1
 * role; a kept trajectory publishes its rows to the dynamics role as an identity gather and carries its log-weights to its
 * own next step through logw_a / logw_b (the same workgroup, in program order).  Same bits as the loop of launches.
 *   ess_threshold    in (0, 1]; otherwise MMF_EINVAL
 *   resampled_steps  (T, N) int32 1 / 0, or null */
int mmf_pf_forward_loop_adaptive(const MmfPfLoopArgs* args /* host */, float ess_threshold,
                                 int32_t* resampled_steps, void* stream);

/* The step loop that runs the dynamics network ONCE PER DISTINCT RESAMPLED ANCESTOR.  Systematic resampling copies a
 * surviving particle into CONSECUTIVE output slots (the ancestor sequence is non-decreasing): a run.  The dynamics network's
 * output is a pure function of the particle's state and its trajectory's control -- a particle is a column of the MFMA tiles
 * and columns do not mix -- so every copy of an ancestor gets the same head outputs bit for bit; only the noise added in the
 * epilogue differs, and that chain is separable (x' = [x + (dir + b) sigmoid(gate + b)] + scale_tril eps).  With a workspace:
 *   - K1 of steps 0 .. T-2 is mmf_pf_resample_runs: the RUN TABLE instead of the gather (no state row is read for the
 *     gather or stored: 4 B per slot + 8 B per run instead of 8 d B per particle);
 *   - the dynamics launch of steps 1 .. T-1 is mmf_pf_dynamics_runs: a tile is 64 (small problems: 32) runs of one trajectory,
 *     its columns read the ancestors' rows from the buffer the previous step PROPAGATED, and the epilogue expands every run
 *     into its output slots, each with its own noise (tensor row or counter-based draw of the SLOT);
 *   - step 0's dynamics and step T-1's K1 are the kernels of mmf_pf_forward_loop (the belief on entry and on return is a
 *     full particle set); states_a / states_b ping-pong as propagated buffers, final_location as ever.
 * Purely additive to ABI 42, as the adaptive loop was: new symbols and a struct of their own, MmfPfLoopArgs keeps its layout.
 * Every output of the loop -- estimates, records, indices_steps, loglik_steps, the belief on return -- has the bits
 * mmf_pf_forward_loop produces (tests/test_gpu_dedup_dynamics.py).  The path is taken when mmf_pf_dedup_plan() == 1 -- plain
 * systematic resampling (resample_mode 1, soft_alpha 0 or 1), M a multiple of 64, d = 2 or 3, the run variant of K1 fits LDS --
 * and every workspace pointer is set; otherwise (and with ws == null) the call IS mmf_pf_forward_loop.  The persistent form
 * (args->persistent) is unchanged; only its fallback to launches takes the workspace. */
typedef struct MmfPfDedupWorkspace {
  int32_t* rank;       /* (N, M)      index of the run every output slot belongs to                  */
  int32_t* run_anc;    /* (N, M + 1)  ancestor particle of every run                                 */
  int32_t* run_start;  /* (N, M + 1)  first output slot of every run; run_start[n][n_runs[n]] = M    */
  int32_t* n_runs;     /* (N)         number of runs = distinct ancestors                            */
} MmfPfDedupWorkspace;   /* host struct holding device pointers; mmf_pf_dedup_workspace_words(N, M) int32 in all */
int mmf_pf_forward_loop_dedup(const MmfPfLoopArgs* args /* host */, const MmfPfDedupWorkspace* ws /* host or null */,
                              void* stream);
/* 1: the sizes / modes take the run path, 0: they do not, MMF_EINVAL: M < 1 or d < 1.  `recording`: a belief record is kept. */
int mmf_pf_dedup_plan(int M, int d, int resample_mode, float soft_alpha, int recording);
size_t mmf_pf_dedup_workspace_words(int N, int M);
/* K1, plain systematic resampling (mode 1, M_out == M), writing the run table instead of the gathered particles.  estimate,
 * cov / ess / log_evidence (each or null), indices_out (or null) and logw_out (or null: uniform by definition) are bit for
 * bit what mmf_pf_reweight_resample_belief writes on the same inputs; rank / run_anc / run_start / n_runs as in
 * MmfPfDedupWorkspace.  Limits: the search-free K1's (12 B of LDS per particle: M <= 13,000), larger -> MMF_ETOOLARGE. */
int mmf_pf_resample_runs(const float* loglik, const float* logw_in, const float* states_in, const float* u,
                         float* estimate, float* logw_out, int32_t* indices_out, int32_t* rank, int32_t* run_anc,
                         int32_t* run_start, int32_t* n_runs, int N, int M, int d, float* cov, float* ess,
                         float* log_evidence, void* stream);
/* mmf_pf_dynamics over a run table: states_out[n][k] = drift(states_prev[n][run_anc[n][rank[n][k]]]) + scale_tril eps[n][k],
 * the network evaluated once per run.  M a multiple of 64, n_res = 3, d = 2 or 3, states_out != states_prev. */
int mmf_pf_dynamics_runs(const float* packed, int n_res, int precision, const float* states_prev,
                         const float* traj_bias, const float* noise, const float* scale_tril, const int32_t* rank,
                         const int32_t* run_anc, const int32_t* run_start, const int32_t* n_runs, float* states_out,
                         int* range_flag, int N, int M, int d, void* stream);
int mmf_pf_dynamics_runs_philox(const float* packed, int n_res, int precision, const float* states_prev,
                                const float* traj_bias, unsigned long long seed, unsigned step, unsigned traj0,
                                const float* scale_tril, const int32_t* rank, const int32_t* run_anc,
                                const int32_t* run_start, const int32_t* n_runs, float* states_out, int* range_flag,
                                int N, int M, int d, void* stream);
/* How mmf_pf_dynamics_runs deals its real tiles where a workgroup builds a dense list of them (tiles are claimed, N <= 2048,
 * at most 2048 entries per workgroup): a trajectory holds ceil(clamp(n_runs, 1, M) / tile) real tiles, the real tiles of
 * the launch are numbered trajectory-major, and number k belongs to workgroup k mod grid.  Writes the first `cap` entries of
 * workgroup b's list to `out` as tile numbers q' N + traj (tile q = (q' + traj) mod (M / tile) of trajectory traj) and
 * returns the list's length.  HOST pointers; the kernel calls the same functions (csrc/particle_net_deal.h).  MMF_EINVAL:
 * a null pointer, M % tile != 0, b outside [0, grid), N / M / tile / grid < 1.  Additive to ABI 42. */
int mmf_pf_dedup_deal(const int32_t* n_runs, int N, int M, int tile, int grid, int b, int32_t* out, int cap);

/* The step loop that KEEPS ITS HISTORY for particle smoothing (mmf_pf_smooth): the set every step propagated, the log-weights
 * every step's K1 started from, and -- through args->loglik_steps / args->indices_steps -- the log-likelihoods and the
 * ancestors.  Upstream torchfilter overwrites particle_states / particle_log_weights at every step and leaves keeping them
 * to the caller.  Purely additive to ABI 42: a new symbol and a struct of its own, MmfPfLoopArgs keeps its layout.  The
 * forward side needs no kernel change, only pointers: the dynamics launch of step t writes slice t of states_steps, the
 * measurement launches and K1 read it there, and K1 gathers into the scratch buffers states_a / states_b (never into a
 * history slice: the run-table path's last K1 included).  Without resampling the next dynamics launch reads slice t
 * directly and ONE device-to-device copy after the last step puts the belief where final_location says; the run-table path
 * reads the ancestors' rows from slice t - 1.  Where logw_in_steps is given, K1's logw_out of step t is slice t + 1 (the
 * last step's goes to logw_a / logw_b as ever); a kept trajectory of the adaptive loop already writes identity ancestors and
 * carried weights.  Every output the loop had before -- estimates, records, indices_steps, loglik_steps, the belief on return,
 * resampled_steps, final_location -- has the same bits with the history attached.
 * The call takes the loop of launches: the persistent form keeps no history (as it keeps no indices_steps) and
 * args->persistent is ignored.
 *   ess_threshold    0: off (mmf_pf_forward_loop / _dedup); otherwise as mmf_pf_forward_loop_adaptive
 *   resampled_steps  (T, N) int32 or null (adaptive only)
 *   ws               the run-table workspace of mmf_pf_forward_loop_dedup, or null
 * MMF_EINVAL: null args / history / states_steps / logw_in0, null args->loglik_steps, null args->indices_steps with
 * resample_mode != 0, null logw_in_steps where weights travel, and whatever the loop it stands for refuses. */
typedef struct MmfPfHistory {
  float*   states_steps;   /* (T, N, M, d)  the set step t PROPAGATED (what K1 of step t read)              */
  float*   logw_in_steps;  /* (T, N, M) or null: the log-weights K1 of step t started from.  Required where */
                           /* weights travel (resample_mode 0, soft alpha, ESS threshold); null allowed for  */
                           /* plain resampling, where they are uniform for t > 0 and step 0's are the belief's */
  float*   logw_in0;       /* (N, M): copy of the belief's log-weights on entry (written by the call)        */
} MmfPfHistory;
int mmf_pf_forward_loop_history(const MmfPfLoopArgs* args /* host */, const MmfPfHistory* history /* host */,
                                float ess_threshold, int32_t* resampled_steps,
                                const MmfPfDedupWorkspace* ws /* host or null */, void* stream);

/* REGULARISED (post-resampling) particle filter (Musso, Oudjane & Le Gland 2001): after a step resampled, every survivor is
 * drawn from the kernel density of the weighted set instead of being copied, x <- x[a] + h C^{1/2} eps, so that the copies of
 * an ancestor separate before the process noise does it.  Upstream torchfilter copies the survivors verbatim.  Purely additive
 * to ABI 42: new symbols and structs of their own.  The ONE definition every path follows (fp32, per trajectory n):
 *   inputs    mu (d), C (d, d), ess: what mmf_pf_reweight_resample_belief writes for the pre-resampling weighted set
 *             (estimate, cov, ess -- same bits); x (M, d): the set K1 gathered; scale > 0, floor (d floats >= 0), shrink 0 / 1
 *   bandwidth h = scale * powf(4 / ((d + 2) ess), 1 / (d + 4)): mmf_pf_density's Silverman factor on the ESS (not on M: after
 *             a step that spent its weight on few particles the kernel must be wide)
 *   factor    L = clamped Cholesky factor of C + diag(floor^2), column by column:
 *               s_j = C_jj + floor_j^2 - sum_{k<j} L_jk^2,           L_jj = s_j > 0 ? sqrt(s_j) : 0
 *               L_ij = L_jj > 0 ? (C_ij - sum_{k<j} L_ik L_jk) / L_jj : 0      (i > j)
 *             a collapsed direction gets no jitter unless floor gives it one; H = h L (each entry one rounded product)
 *   step      shrink == 0: x'_i = x_i + sum_{k<=i} H_ik eps_k          (the set's covariance becomes about (1 + h^2) C)
 *             shrink != 0: x'_i = mu_i + a (x_i - mu_i) + sum_{k<=i} H_ik eps_k, a = sqrt(max(1 - h^2, 0))  (Liu & West: mean
 *             and covariance are preserved).  Evaluated as an fma chain in ascending k, starting from x_i (or from
 *             fma(a, x_i - mu_i, mu_i)): no other rounding, so the noise source does not change the bits
 *   unchanged a trajectory whose ess is not finite or < 1, or whose C has a non-finite entry, is not written at all (NaN rows
 *             stay NaN); neither is one with resampled[n] == 0 (an ESS-triggered step kept it: it has no copies to separate)
 *   noise     eps standard normal: noise_mode 0, a tensor (N, M, d); noise_mode 2, generated in the kernel from
 *             (noise_seed, noise_step, noise_traj0 + n, m) on the Philox stream MMF_PHILOX_STREAM_JITTER (include/mmf_philox.h),
 *             the first d of the particle's four normals -- what mmf_philox_normals_stream materialises
 * Ancestors, log-weights, the estimate and the belief record of the step are K1's: this call touches the gathered set only.
 *   bandwidth (N) or null      h; NaN where ess is not finite or < 1; 0 where resampled[n] == 0
 *   factor    (N, d, d) or null  H, the factor that was applied (upper triangle 0); all 0 where the row was left unchanged
 * A streaming kernel (8 d bytes per particle with counter noise, 12 d with a tensor): a wave takes 256 consecutive particles
 * of one trajectory, four per lane as d 16-byte vectors (the last M mod 4 particles of a row element by element), computes
 * h and H once in uniform registers, and the grid is sized by the bytes (at most 8192 one-wave workgroups, grid-stride), not by
 * the trajectories.  No atomics: every output particle is written by one lane, so two calls and any batch give the same bits.
 * MMF_EINVAL: null args / states / cov / ess, null noise with noise_mode 0, shrink without mean, d outside 1..4, M < 1, N < 0,
 * scale not finite or <= 0, a negative or NaN floor, noise_mode other than 0 / 2; N == 0 is a successful no-op. */
typedef struct MmfPfRegulariseArgs {
  int32_t N, M, d;
  int32_t shrink;            /* != 0: Liu & West shrinkage towards `mean`                                          */
  float* states;             /* (N, M, d) in place                                                                 */
  const float* cov;          /* (N, d, d)                                                                          */
  const float* ess;          /* (N)                                                                                */
  const float* mean;         /* (N, d): required with shrink, otherwise unused (may be null)                       */
  const int32_t* resampled;  /* (N) 1 / 0, or null: every trajectory resampled                                     */
  const float* noise;        /* noise_mode 0: (N, M, d) standard normal                                            */
  uint64_t noise_seed;       /* noise_mode 2                                                                       */
  uint32_t noise_step;
  uint32_t noise_traj0;      /* global index of this shard's first trajectory                                      */
  int32_t noise_mode;        /* 0: `noise` tensor; 2: generated in the kernel                                      */
  float scale;
  float floor[MMF_MAX_STATE_DIM];
  float* bandwidth;          /* (N) out or null                                                                    */
  float* factor;             /* (N, d, d) out or null                                                              */
} MmfPfRegulariseArgs;       /* host struct holding device pointers                                                */
int mmf_pf_regularise(const MmfPfRegulariseArgs* args /* host */, void* stream);

/* The step loop with regularised resampling: after the K1 launch of every step (plain, soft or ESS-triggered resampling) one
 * mmf_pf_regularise launch on the buffer K1 gathered into, with K1's weighted mean (estimate_scratch under estimate_argmax),
 * covariance and ESS -- K1 is called in its recording form, so the size limits of a recording call apply -- and, with a
 * threshold, its decisions.  Always the loop of launches: the persistent form (args->persistent is ignored) and the run-table
 * path are not eligible -- jittered particles have no runs.  Everything the loop wrote before -- estimates, records,
 * ancestors, log-weights, the history -- is what the same loop writes from the jittered belief; the history holds the
 * propagated sets and K1's ancestors as ever.
 *   history          as mmf_pf_forward_loop_history (and what it refuses), or null
 *   ess_threshold    0: off; otherwise as mmf_pf_forward_loop_adaptive, with resampled_steps (T, N) or null
 *   reg              scale / floor / shrink as above; noise (T, N, M, d), or noise_mode 2 with step t drawing counter step
 *                    noise_step0 + t; cov (N, d, d) / ess (N) / resampled (N) scratch for what args (cov_steps, ess_steps)
 *                    and resampled_steps do not record (each required only then); bandwidth_steps (T, N) or null
 * MMF_EINVAL: null args / reg, args->resample_mode == 0, a missing scratch, and whatever the loop and mmf_pf_regularise refuse. */
typedef struct MmfPfLoopRegularise {
  float scale;
  float floor[MMF_MAX_STATE_DIM];
  int32_t shrink;
  const float* noise;        /* (T, N, M, d) or null with noise_mode 2                                             */
  uint64_t noise_seed;
  uint32_t noise_step0;
  uint32_t noise_traj0;
  int32_t noise_mode;
  float* cov;                /* (N, d, d) scratch, or null where args->cov_steps is given                          */
  float* ess;                /* (N) scratch, or null where args->ess_steps is given                                */
  int32_t* resampled;        /* (N) scratch, or null without a threshold or where resampled_steps is given         */
  float* bandwidth_steps;    /* (T, N) out or null                                                                 */
} MmfPfLoopRegularise;       /* host struct holding device pointers                                                */
int mmf_pf_forward_loop_regularised(const MmfPfLoopArgs* args /* host */, const MmfPfHistory* history /* host or null */,
                                    float ess_threshold, int32_t* resampled_steps,
                                    const MmfPfLoopRegularise* reg /* host */, void* stream);

/* The persistent form of the step loop (MmfPfLoopArgs.persistent): at the sizes the reference itself runs (32
 * trajectories x 300 particles: door_models/pf.py:24-27, eval_helpers.py:125-142) a step is bound by the fixed cost
 * of its four launches; one launch whose workgroups keep ONE network's weights in LDS for all T steps and hand
 * particles over through L2 (tagged 8-byte granules: the data is the flag; no grid barrier) removes it.
 *   mmf_pf_persistent_plan: number of workgroups it would use (0: not eligible -- too many tiles per wave, or
 *   M > 2048; MMF_EINVAL: invalid sizes), and optionally the workgroups per network role, K1 workgroups and tiles
 *   per trajectory.                                                                                               */
int mmf_pf_persistent_plan(int N, int M, int n_meas, int* G_out, int* GK_out, int* tiles_per_trajectory_out);
size_t mmf_pf_persistent_sync_words(int N, int M, int d, int n_meas);

/* estimation_method = "argmax" of torchfilter's ParticleFilter: per trajectory the particle with
 * the largest pre-resampling log-weight logw_in + loglik (logw_in null: uniform), first index on ties (torch.argmax).
 *   loglik (N, M), logw_in (N, M) | null, states (N, M, d) -> estimate (N, d)                                  */
int mmf_pf_argmax_estimate(const float* loglik, const float* logw_in, const float* states, float* estimate,
                           int N, int M, int d, void* stream);

/* Counter-based process noise (include/mmf_philox.h: Philox4x32-10 + a fixed-order Box-Muller, a pure
 * function of (seed, step, global trajectory index, particle)): replaces the
 * MultivariateNormal(...).rsample() torchfilter draws inside every step without a
 * (T, N, M, d) tensor.  mmf_pf_dynamics_philox = mmf_pf_dynamics with the noise generated in the kernel's
 * epilogue; mmf_philox_normals materialises the same draws (N, M, d) (initial particles, step-by-step use,
 * tests); mmf_philox_uniforms the resampling uniforms (T, N) of steps step0 .. step0 + T - 1.
 */
int mmf_pf_dynamics_philox(const float* packed, int n_res, int precision, const float* states_in,
                           const float* traj_bias, unsigned long long seed, unsigned step, unsigned traj0,
                           const float* scale_tril, float* states_out, int* range_flag, int N, int M, int d,
                           void* stream);
int mmf_philox_normals(unsigned long long seed, unsigned step, unsigned traj0, float* out, int N, int M, int d,
                       void* stream);
/* the same block on another stream of the generator (MMF_PHILOX_STREAM_*; stream 0 IS mmf_philox_normals): what
 * mmf_pf_regularise draws in noise_mode 2 is stream MMF_PHILOX_STREAM_JITTER */
int mmf_philox_normals_stream(unsigned long long seed, unsigned philox_stream, unsigned step, unsigned traj0, float* out,
                              int N, int M, int d, void* stream);
int mmf_philox_uniforms(unsigned long long seed, unsigned step0, unsigned traj0, float* out, int T, int N,
                        void* stream);


/* Open-loop rollout of the dynamics model: replaces torchfilter's DynamicsModel.forward_loop (external
 * dependency; call sites crossmodal/eval_helpers.py:135-137, scripts/door_task/eval_dynamics.py:36-38):
 *     x_t = f(x_{t-1}, u_t),  t = 1 .. T      (no process noise: the mean prediction)
 * as T launches of the K2 dynamics kernel enqueued by one C call, each reading the previous step's row
 * of the output.
 *  packed     packed dynamics network (mmf_pack_particle_net)
 *  x0         (N, d) initial states
 *  traj_bias  (T, N, 64) hoisted control term of every step (one K7 launch over the T*N controls)
 *  out        (T, N, d) predicted states
 */
int mmf_dynamics_forward_loop(const float* packed, int n_res, int precision, const float* x0,
                              const float* traj_bias, float* out, int32_t* range_flag, int T, int N, int d,
                              void* stream);

/* ---------------------------------------------------------------- particle smoothing: ancestry trace + moments
 * The estimate E[x_t | y_1..s] for an endpoint s >= t from a filter run's history (mmf_pf_forward_loop_history, or the same
 * arrays stacked step by step).  Upstream torchfilter's ParticleFilter reports the filtered estimate only and leaves
 * particle_states / particle_log_weights to the caller after each step; this is what a caller would build on them.
 * Ancestry (genealogy) smoothing with a fixed-lag option: for particle m of the endpoint the path index is b_s[m] = m,
 * b_t[m] = A_t[b_{t+1}[m]] (A_t: the ancestors step t drew, identity where nothing was resampled), and the smoothed moments
 * of step t are those of {X_t[b_t[m]]} under the endpoint's normalised weights w_s = softmax_m(loglik_s + logw_in_s).
 * With lag L the endpoint of step t is s(t) = min(t + L, T - 1); L >= T - 1 is the full smoother, L = 0 the filter's own
 * weighted set.  One workgroup per (trajectory, endpoint): endpoint s < T - 1 walks back L steps and writes step s - L,
 * endpoint T - 1 writes every step it passes (itself included); endpoints with s - L < 0 are not launched.  b lives in
 * registers (several particles per thread beyond 1024), the weights in LDS.
 * Arithmetic: K1's pivot form (mmf_pf_reweight_resample_belief) -- pivot p = the row of the first highest-weight path,
 * e_m = exp(a_m - max), S = sum e, m1 = sum e (x - p), M2 = sum e (x - p)(x - p)^T, mean = p + m1 / S,
 * cov = M2 / S - (m1 / S)(m1 / S)^T, stored symmetric bit for bit; a path with a_m = -inf contributes exactly zero.
 * Reductions in a fixed order (DPP wave sums, then the waves' partials in LDS in wave order; no float atomics): two runs
 * give the same bits.  unique: a bitmap of M bits in LDS (integer atomics) and a popcount, over the paths with a_m > -inf.
 * Ancestors are clamped to [0, M): a corrupted index gives a wrong number, never a fault.
 * Limits: 1 <= d <= 4; M <= 65536 and mmf_pf_smooth_lds_bytes(M) <= 160 KiB (4 B per particle + the bitmap: M <= 39,400),
 * larger -> MMF_ETOOLARGE.  lag < 0, T < 0, N < 0, M < 1 or a null args / states_steps / loglik_steps / mean -> MMF_EINVAL.
 * N == 0 or T == 0 is a successful no-op. */
typedef struct MmfPfSmoothArgs {
  int32_t T, N, M, d, lag;          /* lag >= 0; lag >= T-1: full smoother */
  const float* states_steps;        /* (T, N, M, d) */
  const float* loglik_steps;        /* (T, N, M)    */
  const float* logw_in_steps;       /* (T, N, M) or null = uniform for t > 0 */
  const float* logw_in0;            /* (N, M) or null = uniform; read for step 0 when logw_in_steps is null */
  const int32_t* indices_steps;     /* (T, N, M) or null = identity */
  float* mean;                      /* (T, N, d)    */
  float* cov;                       /* (T, N, d, d) or null */
  int32_t* unique;                  /* (T, N) or null: distinct particles of step t on the endpoint's paths */
} MmfPfSmoothArgs;                  /* host struct holding device pointers */
int mmf_pf_smooth(const MmfPfSmoothArgs* args /* host */, void* stream);
/* Dynamic LDS bytes mmf_pf_smooth requests for M particles (monotone in M). */
size_t mmf_pf_smooth_lds_bytes(int M);

/* ---------------------------------------------------------------- marginal particle smoothing (forward filter, backward smoother)
 * The ancestry smoother above re-weights the particles of step t by how many of the endpoint's paths still pass through
 * them; far from the endpoint that is a handful (unique[t]).  The forward-filter backward-smoothing recursion (FFBSm;
 * Doucet, Godsill & Andrieu 2000) keeps EVERY particle of step t and re-weights it through the transition density, so it
 * reads no ancestors and holds for every resampling mode (plain, multinomial, soft, ESS-triggered, none).  Upstream
 * torchfilter's ParticleFilter has no smoother; a caller writing this one in torch ops on the kept sets materialises an
 * (M, M, d) tensor per trajectory and step.  Purely additive to ABI 42: a struct and a symbol of its own.
 * From a history of T steps: X_t (N, M, d) the set step t propagated, W_t = softmax_m(loglik_t + logw_in_t) the filter's
 * weights on it (a particle with -inf has weight exactly 0, and whatever its rows hold never reaches a result),
 * F_t[i] = f(X_t[i], u_{t+1}), t = 0 .. T - 2, the dynamics mean of particle i under the control step t + 1 was propagated
 * with (pred_steps: the caller evaluates it, e.g. with one mmf_pf_dynamics call without noise over all (T - 1) N
 * trajectories), L the lower-triangular scale_tril (d, d) of the process noise, one for all particles and steps.
 *   lp_t[i, j]   = -1/2 || L^-1 (X_{t+1}[j] - F_t[i]) ||^2        (the Gaussian constant cancels)
 *   logD_t[j]    = logsumexp_i( log W_t[i] + lp_t[i, j] )
 *   W_{T-1|T}    = W_{T-1}
 *   W_{t|T}[i]   = sum_j W_{t+1|T}[j] exp( log W_t[i] + lp_t[i, j] - logD_t[j] ),   renormalised to sum 1
 * The difference X - F is formed first, in fp32, and then whitened with L^-1 (computed in the kernels by forward
 * substitution from the device copy of L: no host round trip): with states O(1) and noise 0.005 .. 0.05 wide the whitened
 * coordinates are 20 .. 200, and differencing THEM -- or expanding the square -- would cost 1e-4 .. 1e-2 absolute in the
 * exponent.  Every term of the second sum is at most W_{t+1|T}[j]: it needs no maximum and cannot overflow.  A column j
 * with W_{t+1|T}[j] = 0 is skipped (its logD may be -inf).
 * Four kinds of launch behind the one call: the weights (a_t - max a_t per step and trajectory); logD for all steps at once
 * (a thread owns a column j, the rows i stream through LDS in chunks of fixed size, log-sum-exp with a running maximum
 * rescaled once per group of rows); the backward sweep, T - 1 launches (a thread owns a row i, the columns stream through
 * LDS; every workgroup sums the unnormalised W_{t+1|T} of its trajectory itself, in one fixed order); the moments.  LDS use
 * does not depend on M.  exp / log are the hardware's base-2 forms: this smoother has no strict bit-exact twin.
 * Moments in the pivot form of mmf_pf_smooth (pivot = the row of the first largest smoothed weight), cov symmetric bit for
 * bit; ess = 1 / sum W_{t|T}^2, the diagnostic in the place of unique.  All reductions in a fixed order, no float atomics:
 * two runs give the same bits, and trajectory n's results do not depend on N.
 * Limits: 1 <= d <= 4, 1 <= M <= 65536, N <= 65535, beyond -> MMF_ETOOLARGE (d outside 1 .. 4 included).  A null args /
 * states_steps / loglik_steps / scale_tril / weights / mean, a null pred_steps / logd with T >= 2, T < 0, N < 0, M < 1 or
 * d < 1 -> MMF_EINVAL.  N == 0 or T == 0 is a successful no-op; T == 1 runs the weights and the moments only.  All decided
 * on the host before any HIP call.  A non-positive or non-finite diagonal of L makes every result NaN; it never faults. */
typedef struct MmfPfSmoothMarginalArgs {
  int32_t T, N, M, d;
  const float* states_steps;        /* (T, N, M, d)     X_t                                                  */
  const float* pred_steps;          /* (T - 1, N, M, d) F_t; unread (may be null) for T < 2                  */
  const float* loglik_steps;        /* (T, N, M)                                                             */
  const float* logw_in_steps;       /* (T, N, M) or null = uniform                                           */
  const float* scale_tril;          /* (d, d) DEVICE, row-major; the upper triangle is not read              */
  float* logd;                      /* workspace (T - 1, N, M): logD_t; unread (may be null) for T < 2       */
  float* weights;                   /* (T, N, M)    W_{t|T}                                                  */
  float* mean;                      /* (T, N, d)                                                             */
  float* cov;                       /* (T, N, d, d) or null                                                  */
  float* ess;                       /* (T, N) or null                                                        */
} MmfPfSmoothMarginalArgs;          /* host struct holding device pointers */
int mmf_pf_smooth_marginal(const MmfPfSmoothMarginalArgs* args /* host */, void* stream);

/* ---------------------------------------------------------------- backward-simulation particle smoothing (forward filter, backward simulation)
 * The two smoothers above return marginals: moments, and per-step weights W_{t|T}.  Forward filtering, backward simulation
 * (FFBSi; Godsill, Doucet & West 2004) draws WHOLE trajectories from the joint smoothing distribution
 * p(x_{0:T-1} | y_{0:T-1}), which is what any function of the path needs (was the door ever open, path length, pairwise
 * moments for an EM refit of the noise).  Upstream torchfilter's ParticleFilter has no smoother and no path sampler; a caller
 * writing this one in torch ops on the kept sets runs T dependent steps of an (N, S, M, d) broadcast, a cumsum and a
 * search each.  Purely additive to ABI 42: a struct and a symbol of its own.
 * From a history of T steps, as for the marginal smoother: X_t (N, M, d), W_t = softmax_m(loglik_t + logw_in_t),
 * F_t[i] = f(X_t[i], u_{t+1}) (pred_steps), L the one process-noise scale_tril (d, d); and uniforms u (T, N, S) in [0, 1).
 * For trajectory n and draw s:
 *   v_{T-1}[i] = log W_{T-1}[i]
 *   v_t[i]     = log W_t[i] - 1/2 || L^-1 (X_{t+1}[j_{t+1}] - F_t[i]) ||^2        t = T-2 .. 0
 *   p_t[i]     = exp(v_t[i] - max_i v_t),   c_t[i] = sum_{k <= i} p_t[k]          (ascending i)
 *   j_t        = the smallest i with c_t[i] > u[t, n, s] * c_t[M-1]
 * The inequality is strict: a particle of weight zero (loglik = -inf included) is never chosen, and whatever its rows hold
 * never reaches a result.  Where rounding leaves no such i, j_t is the last i with p_t[i] > 0.  The difference X - F is
 * formed before it is whitened (the marginal smoother's rule, for its reason); log W_t is taken relative to the step's
 * largest log-weight, and the softmax's normaliser cancels in the draw.  exp is the hardware's base-2 form.
 * A draw is dead where every v_t[i] is -inf, a v is NaN, or the diagonal of L is not positive and finite: it gets index -1
 * and NaN states at that step and at every earlier one; it never faults.  mean and cov of a step with a dead draw are NaN.
 * Outputs: indices (T, N, S) int32; trajectories (T, N, S, d) = X_t[n, j_t] copied bit for bit; mean (T, N, d) the plain
 * average over the S draws; cov (T, N, d, d) or null: 1/S, about the mean, in the pivot form of the other smoothers (the
 * pivot is draw 0), symmetric bit for bit.
 * Two launches behind the one call.  The sampler is ONE launch for all steps over (draw blocks, N): a workgroup owns
 * trajectory n and a block of B draws and walks t = T-1 .. 0 itself; no workgroup talks to another.  Per step a thread owns
 * a contiguous segment of rows, which stream through LDS in chunks of fixed size (LDS use does not depend on M); per draw it
 * keeps an online (max, sum) over its segment; the workgroup combines the pairs in thread order, scans them, and the
 * segment that holds u * total is walked once more for j_t.  The moments: one workgroup per (t, n).
 * All reductions in a fixed order, no float atomics: two calls give the same bits, and the result for (n, s) depends only
 * on trajectory n's history and u[:, n, s] -- not on N, on S or on which workgroup took the draw.
 * Limits: 1 <= d <= 4, 1 <= M <= 65536, N <= 65535, 1 <= S <= 65535, beyond -> MMF_ETOOLARGE.  A null args / states_steps /
 * loglik_steps / scale_tril / uniforms / indices / trajectories / mean, a null pred_steps with T >= 2, T < 0, N < 0, or
 * M, S or d below 1 -> MMF_EINVAL (an invalid call is invalid whatever its size).  N == 0 or T == 0 is a successful no-op.
 * All decided on the host before any HIP call. */
typedef struct MmfPfSmoothSimulateArgs {
  int32_t T, N, M, d, S;
  const float* states_steps;        /* (T, N, M, d)     X_t                                                  */
  const float* pred_steps;          /* (T - 1, N, M, d) F_t; unread (may be null) for T < 2                  */
  const float* loglik_steps;        /* (T, N, M)                                                             */
  const float* logw_in_steps;       /* (T, N, M) or null = uniform                                           */
  const float* scale_tril;          /* (d, d) DEVICE, row-major; the upper triangle is not read              */
  const float* uniforms;            /* (T, N, S) in [0, 1)                                                   */
  int32_t* indices;                 /* (T, N, S)    j_t, -1 where the draw is dead                           */
  float* trajectories;              /* (T, N, S, d) X_t[n, j_t]                                              */
  float* mean;                      /* (T, N, d)                                                             */
  float* cov;                       /* (T, N, d, d) or null                                                  */
} MmfPfSmoothSimulateArgs;          /* host struct holding device pointers */
int mmf_pf_smooth_simulate(const MmfPfSmoothSimulateArgs* args /* host */, void* stream);

/* ---------------------------------------------------------------- two-slice smoothing moments (the E-step of an EM refit of the process noise)
 * The smoothers above return per-step marginals or sampled paths.  Refitting the process noise Q = L L^T by EM needs the
 * expected transition residual and its second moment under the TWO-SLICE smoothing distribution p(x_t, x_{t+1} | y_{1:T})
 * over particle pairs; the M-step is then a mean and a Cholesky factor.  Upstream torchfilter's ParticleFilter has no
 * smoother and nothing that estimates Q; a caller can approximate the moments from mmf_pf_smooth_simulate's paths with
 * 1 / sqrt(S) Monte-Carlo noise on top, or sum all M^2 pairs in torch ops over an (M, M, d) tensor per trajectory and step.
 * Purely additive to ABI 42: a struct and two symbols of its own.
 * From a history of T steps, as for mmf_pf_smooth_marginal (X_t, F_t = pred_steps, W_t = softmax_m(loglik_t + logw_in_t),
 * lp_t[i, j] and logD_t[j] exactly as that section defines them, L the device scale_tril), and from two results of a
 * preceding mmf_pf_smooth_marginal call on the SAME history and L: its normalised weights W_{t|T} (T, N, M) and its logd
 * workspace (T - 1, N, M).  For t = 0 .. T - 2 and trajectory n:
 *   xi_t[i, j]  ~ W_t[i] exp( lp_t[i, j] - logD_t[j] ) W_{t+1|T}[j]          normalised to sum 1 over (i, j)
 *   e_t[i, j]   = X_{t+1}[j] - F_t[i]                                        formed in fp32, before anything else
 *   residual_mean[t, n]          = sum_ij xi e                               (T - 1, N, d)
 *   residual_second_moment[t, n] = sum_ij xi e e^T                           (T - 1, N, d, d), RAW (not centred)
 * The rules of the marginal smoother carry over.  A row i with W_t[i] = 0 (loglik + logw_in = -inf) is skipped and so is
 * a column j with W_{t+1|T}[j] = 0: whatever their rows of X / F hold, inf included, never reaches a result.  The kernel
 * divides by the total of xi that it sums itself, so any per-(t, n) constant in log W_t cancels; log W_t is taken relative
 * to the step's largest log-weight -- the basis logD was computed in, so every term is at most W_{t+1|T}[j] and nothing
 * overflows.  That maximum is taken by EACH WORKGROUP ITSELF from the step's M log-weights (M reads beside its 64 M pairs):
 * no launch of its own and no (T - 1, N, M) array for it.  exp / log are the hardware's base-2 forms with L^-1 scaled by
 * sqrt(log2(e) / 2) (pf_smooth_math.h): no strict bit-exact twin.  The difference e is formed first and whitened after,
 * for the marginal smoother's reason; the same e enters the sums, so nothing is expanded into x x^T - x f^T - ...: with
 * states O(1) and noise 0.005 .. 0.05 wide that cancellation would cost the second moment three to five digits.
 * Two launches behind the one call.  Pairs: ONE launch over (row tile of 64, trajectory, step) -- all T - 1 steps are
 * independent (the grid's z holds 65535 of them per launch) -- a thread owns row i with F_t[i] and log2 W_t[i] in registers,
 * the columns stream through LDS in chunks of fixed size (LDS use does not depend on M) with log2 W_{t+1|T}[j] -
 * logD_t[j] log2(e) beside them; per pair one whitened distance, one exp2, and 1 + d + d (d + 1) / 2 sums (the total, p e,
 * the upper triangle of p e e^T).  Each sum is wave-summed and lane 0 writes the tile's partials to
 * workspace (T - 1, N, tiles, 1 + d + d (d + 1) / 2), tiles = ceil(M / 64).  Reduce: one workgroup per (t, n) adds the
 * tiles' partials in tile order, divides by the total, and writes both outputs; the second moment's lower triangle is a
 * copy of the upper: symmetric bit for bit.  All reductions in a fixed order, no float atomics: two calls give the same
 * bits, and trajectory n's results do not depend on N.
 * Limits: 1 <= d <= 4, 1 <= M <= 65536, N <= 65535, beyond -> MMF_ETOOLARGE.  A null args / states_steps / loglik_steps /
 * scale_tril / weights, with T >= 2 a null pred_steps / logd / workspace / residual_mean / residual_second_moment, T < 0,
 * N < 0, M < 1 or d < 1 -> MMF_EINVAL (an invalid call is invalid whatever its size).  N == 0 or T < 2 (no transition)
 * writes nothing and returns 0.  All decided on the host before any HIP call.  A non-positive or non-finite diagonal of L
 * makes every output NaN; it never faults. */
typedef struct MmfPfSmoothPairArgs {
  int32_t T, N, M, d;
  const float* states_steps;        /* (T, N, M, d)     X_t                                                  */
  const float* pred_steps;          /* (T - 1, N, M, d) F_t; unread (may be null) for T < 2                  */
  const float* loglik_steps;        /* (T, N, M)                                                             */
  const float* logw_in_steps;       /* (T, N, M) or null = uniform                                           */
  const float* scale_tril;          /* (d, d) DEVICE, row-major; the upper triangle is not read              */
  const float* weights;             /* (T, N, M)     W_{t|T} as mmf_pf_smooth_marginal left them             */
  const float* logd;                /* (T - 1, N, M) logD_t as mmf_pf_smooth_marginal left it                */
  float* workspace;                 /* mmf_pf_smooth_pair_workspace_floats(T, N, M, d) floats                */
  float* residual_mean;             /* (T - 1, N, d)                                                         */
  float* residual_second_moment;    /* (T - 1, N, d, d)                                                      */
} MmfPfSmoothPairArgs;              /* host struct holding device pointers */
int mmf_pf_smooth_pair_moments(const MmfPfSmoothPairArgs* args /* host */, void* stream);
/* Floats of the workspace above: (T - 1) N ceil(M / 64) (1 + d + d (d + 1) / 2); 0 for T < 2, N < 1 or sizes outside the limits. */
size_t mmf_pf_smooth_pair_workspace_floats(int T, int N, int M, int d);

/* ---------------------------------------------------------------- MAP path smoothing (Viterbi over the particle history)
 * The smoothers above return moments or random draws.  None returns the single most probable state SEQUENCE, which is the
 * estimate to report where the posterior is multimodal (is the door open or closed?): the smoothed mean lies between the
 * modes, in a state the system was never in, and a backward-simulation draw is a legitimate path but a random one.  This is
 * the MAP sequence estimate over the particle grid of Godsill, Doucet & West (2001): a max-plus (Viterbi) recursion over the
 * same M^2 particle pairs per trajectory and step that the marginal smoother walks.  Upstream torchfilter's ParticleFilter
 * has no smoother; in torch ops the recursion materialises an (M, M, d) tensor per trajectory and step.  Purely additive to
 * ABI 42: a struct and a symbol of its own.
 * From a history of T steps, as for mmf_pf_smooth_marginal: X_t (N, M, d), F_t[i] = f(X_t[i], u_{t+1}), t = 0 .. T - 2
 * (pred_steps), loglik_t, L the one lower-triangular scale_tril; and logw_in_0, of step 0 ONLY: the particles' own incoming
 * log-weights stand in for log p(x_0) (null: 0; after initialize_beliefs they are uniform, a flat prior over the step-0 set).
 * The incoming weights of later steps are the filter's importance weights and enter no density.  Natural logarithms, with
 * c = sum_k log L_kk + (d / 2) log 2 pi:
 *   lp_t[i, j]  = -1/2 || L^-1 (X_{t+1}[j] - F_t[i]) ||^2        (the difference first, then whitened: the marginal smoother's rule)
 *   v_0[j]      = loglik_0[j] + logw_in_0[j]
 *   top_t       = max_j v_t[j]                                    (exact: a maximum has no rounding)
 *   v_t[j]      = loglik_t[j] + max_i( (v_{t-1}[i] - top_{t-1}) + lp_{t-1}[i, j] )        t >= 1
 *   psi_t[j]    = the FIRST i attaining that maximum (ties to the lower index);  psi_0 = -1
 *   i_{T-1}     = first argmax_j v_{T-1}[j];   i_t = psi_{t+1}[i_{t+1}]
 *   path[t]     = X_t[i_t]
 *   log_posterior = sum_t top_t - (T - 1) c   =   v_0[i_0] + sum_{t >= 1} ( loglik_t[i_t] + lp_{t-1}[i_{t-1}, i_t] - c )
 * The rescaling by top_{t-1} is part of the definition: without it v grows to 1e5 .. 1e6 over a run (whitened distances are
 * 20 .. 200) and fp32 no longer resolves the decisions.
 * A particle with loglik = -inf (dead, or the padding of a step with fewer particles) has v = -inf, psi = -1 and is never
 * chosen; whatever its rows of X / F hold is not read.  A column none of whose candidates is above -inf is dead likewise.  A
 * trajectory with a step where every particle is dead gets indices = -1, a NaN path and log_posterior = -inf; the reads stay
 * in range and nothing faults, and the other trajectories of the call are unaffected.  A non-positive or non-finite diagonal
 * of L makes every floating output NaN and every index -1.
 * Launches behind the one call: step 0 element-wise; the forward pass, T - 1 launches over (column tile of 64, trajectory),
 * t = 1 .. T - 1, on the plan of the marginal smoother's logD kernel (a wave per workgroup, a thread owns a column j of step t,
 * the rows i of step t - 1 -- F_{t-1}[i] and v_{t-1}[i] - top_{t-1} -- stream through LDS in chunks of fixed size and are
 * consumed in groups of 8: the group's maximum first, the index resolved only where the group improves the running maximum,
 * strictly, so that the first index wins across groups, chunks and tiles); every workgroup takes top_{t-1} of its trajectory
 * itself (M reads) and the first one stores it into step_max; the backtrack, one wave per trajectory: the first maximum of
 * v_{T-1}, one lane walks psi backwards, writes indices and path and sums top_t in ascending t.  LDS use does not depend on
 * M.  The recursion has no exp and no log; inside the forward kernel the values live in base 2 (the shared whitener's
 * scaling), every output is in natural logarithms.  No float atomics, no contraction left to the compiler outside the shared
 * whitener: two calls give the same bits, and trajectory n's outputs do not depend on N.
 * v, step_max and backpointers are outputs as defined above, not scratch.
 * Limits: 1 <= d <= 4, 1 <= M <= 65536, N <= 65535, beyond -> MMF_ETOOLARGE.  A null args / states_steps / loglik_steps /
 * scale_tril / v / step_max / backpointers / indices / path / log_posterior, a null pred_steps with T >= 2, T < 0, N < 0,
 * M < 1 or d < 1 -> MMF_EINVAL (an invalid call is invalid whatever its size); an output that overlaps an input or another
 * output -> MMF_EINVAL.  N == 0 or T == 0 is a successful no-op; T == 1 runs step 0 and the backtrack only.  All decided on
 * the host before any HIP call. */
typedef struct MmfPfSmoothMapArgs {
  int32_t T, N, M, d;
  const float* states_steps;        /* (T, N, M, d)     X_t                                                  */
  const float* pred_steps;          /* (T - 1, N, M, d) F_t; unread (may be null) for T < 2                  */
  const float* loglik_steps;        /* (T, N, M)                                                             */
  const float* logw_in_steps;       /* (T, N, M) or null = 0; only step 0 is read                            */
  const float* scale_tril;          /* (d, d) DEVICE, row-major; the upper triangle is not read              */
  float* v;                         /* (T, N, M)    v_t                                                      */
  float* step_max;                  /* (T, N)       top_t                                                    */
  int32_t* backpointers;            /* (T, N, M)    psi_t                                                    */
  int32_t* indices;                 /* (T, N)       i_t, -1 where the trajectory is dead                     */
  float* path;                      /* (T, N, d)    X_t[n, i_t]                                              */
  float* log_posterior;             /* (N)                                                                   */
} MmfPfSmoothMapArgs;               /* host struct holding device pointers */
int mmf_pf_smooth_map(const MmfPfSmoothMapArgs* args /* host */, void* stream);

/* ---------------------------------------------------------------- Particle-posterior quantiles, credible intervals and PIT
 * Upstream torchfilter's ParticleFilter leaves particle_states / particle_log_weights to the caller, and the evaluation of
 * crossmodal/eval_helpers.py:148-160 judges the posterior mean alone.  Everything above that judges the belief is Gaussian
 * (a covariance, NEES, the moment-matched ellipsoid); for a bimodal set the ellipsoid covers the empty ground between the
 * modes.  This is the non-parametric counterpart: per-dimension weighted quantiles of a particle set (median, credible
 * intervals) and the weighted CDF at a query point (the probability integral transform of the true state), on K1's integer
 * fixed-point weights.  In torch ops it is sort + cumsum + searchsorted + gather over (R, M, d), with an fp32 cumulative sum
 * whose crossings depend on the summation order.  Purely additive to ABI 42: a struct and two symbols of their own.
 * Per row r (R rows, e.g. T * N, of M particles) and state dimension k, with x_m = states[r, m, k]:
 *   a_m   = log_a[r, m] + log_b[r, m]      one fp32 add; a null addend is 0, both null: uniform weights
 *   t_m   = a_m - max_m a_m                one fp32 subtract (the maximum skips NaN);  e_m = expf(t_m)
 *   q_m   = (uint32) floor(e_m * 2^24)     in [0, 2^24]: K1's fixed point.  a_m = -inf or NaN gives q_m = 0 exactly: such a
 *                                          particle is never returned, whatever its state row holds (the histories carry NaN
 *                                          rows for dead particles).  Particles below 2^-24 of the row's heaviest count as
 *                                          weightless, as in K1.
 *   Qtot  = sum_m q_m                      64-bit integers.  A row without a live particle (max a is -inf, NaN or +inf, i.e.
 *                                          Qtot = 0) gives NaN quantiles and a NaN cdf.
 *   quantile p:  the particles ascending by x_m, c_j the inclusive integer sums of q in that order,
 *                thr = max(1, ceil((double) p * (double) Qtot));  the result is the x of the first j with c_j >= thr -- the
 *                inverted weighted CDF, always a particle's own value, bit for bit.  p = 0: the smallest particle with q > 0;
 *                p = 1: the largest.  (Equal x may sort in any order: the integer CDF at the end of a tie group is the same.)
 *   cdf[r, k]  = (float) ((double) sum_{m : x_m <= query[r, k]} q_m / (double) Qtot);  a NaN query gives NaN.
 * Every sum is an integer sum, so the result does not depend on thread count, scan order or R:
 *   - two calls give the same bits;
 *   - a row computed alone (R = 1) has the bits it has in a batch;
 *   - with equal weights the quantile is sort(x)[max(1, ceil(p M)) - 1] exactly and the cdf is count / M rounded once.
 * One launch: a workgroup per (row, dimension) packs (order-preserving uint32 key of x) << 32 | q into one uint64 per
 * particle in LDS, padded to the next power of two P >= max(M, 64) with all-ones keys of weight 0, sorts them (bitonic; a
 * thread owns P / threads consecutive slots and runs the short strides in registers), scans q in integers and searches once
 * per p.  The cdf sum is a reduction before the sort: Q == 0 with a query does not sort.  One wave for P <= 512, 256 threads
 * beyond.  mmf_pf_quantiles_lds_bytes(M): the dynamic LDS of that workgroup, 8 B per padded slot and one spare slot per thread
 * -- monotone in M, at most 160 KiB at the limit M = 16384 (for M beyond it: the value at the limit; 0 for M < 1).
 * Limits, all decided on the host before any HIP call: null args / states, d outside 1 .. 4, M < 1, R < 0, Q outside
 * 0 .. MMF_QUANTILES_MAX, a p outside [0, 1] or NaN, nothing requested (Q == 0 and no query), quantiles null with Q > 0 (with
 * Q == 0 it is not written), exactly one of query / cdf null, an output overlapping an input or the other output -> MMF_EINVAL;
 * M > 16384 or R * d beyond a 32-bit grid -> MMF_ETOOLARGE; R == 0 is a successful no-op. */
#define MMF_QUANTILES_MAX 16
typedef struct MmfPfQuantilesArgs {
  int32_t R, M, d, Q;             /* R rows (e.g. T*N) of M particles; Q in 0 .. MMF_QUANTILES_MAX */
  float probs[MMF_QUANTILES_MAX]; /* host values, each in [0, 1] */
  const float* states;            /* (R, M, d) */
  const float* log_a;             /* (R, M) or null = 0 */
  const float* log_b;             /* (R, M) or null = 0 (history: log_weights_in + log_likelihoods) */
  const float* query;             /* (R, d) or null */
  float* quantiles;               /* (R, Q, d); null iff Q == 0 */
  float* cdf;                     /* (R, d); null iff query is null */
} MmfPfQuantilesArgs;             /* host struct holding device pointers */
int mmf_pf_quantiles(const MmfPfQuantilesArgs* args /* host */, void* stream);
size_t mmf_pf_quantiles_lds_bytes(int M);

/* ---------------------------------------------------------------- Particle-posterior scores: CRPS and the energy score
 * The evaluation of crossmodal/eval_helpers.py:148-160 scores point estimates only (the squared error of the posterior
 * mean); the quantiles above judge calibration only, and a filter that always answers "somewhere in the room" has a uniform
 * PIT.  These are the two standard strictly proper scoring rules taken on the weighted particle set itself (Gneiting &
 * Raftery 2007): they reward calibration and sharpness together, are in the state's own units, reduce to the absolute /
 * Euclidean error for a point mass and have a closed form for a Gaussian.  Both are E|X - y| - 1/2 E|X - X'|; the second
 * expectation runs over all M^2 pairs of a set, which in torch ops is an (M, M, d) tensor or a chunked loop over one.
 * Purely additive to ABI 42: a struct and two symbols of their own.
 * Per row r (R rows, e.g. T * N, of M particles x_m = states[r, m, :]) with a truth y = truth[r, :]:
 *   a_m      = log_a[r, m] + log_b[r, m]     one fp32 add; a null addend is 0, both null: uniform weights
 *   w_m      = expf(a_m - max_m a_m)         one fp32 subtract (the maximum skips NaN); 0 where a_m is -inf or NaN
 *   W_m      = w_m / sum w                   in double, once, at the end
 *   crps[k]  = sum_m W_m |x_mk - y_k| - 1/2 spread[k]                             k < d
 *   spread[k]= sum_m sum_l W_m W_l |x_mk - x_lk|                                  Gini's mean difference of dimension k
 *   energy   = sum_m W_m |(x_m - y) / s|_2 - 1/2 spread[d]
 *   spread[d]= sum_m sum_l W_m W_l |(x_m - x_l) / s|_2
 * s = scale[0 .. d): a per-dimension scale that makes the Euclidean norm meaningful across units; it enters energy and
 * spread[d] only, crps stays in each dimension's own units (the kernel multiplies by the fp32 reciprocal 1 / s_k).
 * The weights are plain floats, NOT K1's 2^24 fixed point: nothing is selected here, so there is nothing for integer sums
 * to protect, and an fp64 evaluation of these lines differs from the kernel by the ulps of expf and of the fp32 pair terms.
 *   - a particle with w_m = 0 contributes nothing, whatever its state row holds (the histories carry NaN rows for dead
 *     particles): the zero weight selects the term away, it does not multiply it;
 *   - a row without a live particle (sum w = 0: max a is -inf, NaN or +inf) gives NaN everywhere;
 *   - a NaN y_k gives NaN in crps[k] and in energy; the other dimensions and spread stay finite;
 *   - spread needs no truth; crps or energy without one is refused.
 * Determinism: every sum is taken in a fixed order and there are no floating-point atomics -- two calls give the same bits,
 * and a row's result depends on neither R nor the other rows (the plan is a function of M alone).
 * Kernel plan: no (M, M) array in memory.  A row is dealt to nb = ceil(M / 512) workgroups in equal i-chunks; a thread holds
 * one i-particle (M <= 512, up to 512 threads) or two (beyond, up to 256 threads) in registers and walks j-tiles of 1024
 * particles staged through LDS as structure-of-arrays (d coordinate planes and w), four j per broadcast 16-byte read; the d
 * differences of a pair feed the d absolute-value accumulators and the one norm.  fp32 accumulators over runs of 64 pairs,
 * flushed to double; 2 d + 3 double sums per workgroup (the pair sums, the truth sums, sum w), reduced in a fixed order.  With
 * nb == 1 the workgroup writes the row; otherwise it writes its sums to the workspace and a finishing kernel adds a row's nb
 * partial sums in order.  mmf_pf_scores_workspace_bytes(R, M, d): 88 R nb bytes for M > 512, 0 up to 512 (and for R, M or
 * d below 1).
 * Limits, all decided on the host before any HIP call: null args / states, d outside 1 .. 4, M < 1, R < 0, a scale[k < d]
 * that is not positive and finite, all three outputs null, crps or energy without truth, a workspace that is needed and null,
 * smaller than the query's answer or not 8-byte aligned, an output (or the workspace) overlapping an input or another
 * output -> MMF_EINVAL; M > 16384 or R * nb beyond a 32-bit grid -> MMF_ETOOLARGE; R == 0 is a successful no-op.
 * Coordinates whose squared difference overflows fp32 (beyond 1e19) are outside what the energy score serves. */
typedef struct MmfPfScoresArgs {
  int32_t R, M, d;                  /* R rows (e.g. T*N) of M particles */
  float scale[MMF_MAX_STATE_DIM];   /* host values, scale[k < d] > 0 and finite; 1 for plain Euclidean distance */
  const float* states;              /* (R, M, d) */
  const float* log_a;               /* (R, M) or null = 0 */
  const float* log_b;               /* (R, M) or null = 0 (history: log_weights_in + log_likelihoods) */
  const float* truth;               /* (R, d); null allowed with spread alone */
  float* crps;                      /* (R, d) or null */
  float* energy;                    /* (R) or null */
  float* spread;                    /* (R, d + 1) or null */
  void* workspace;                  /* device, 8-byte aligned, mmf_pf_scores_workspace_bytes(R, M, d) bytes; unused when that is 0 */
  size_t workspace_bytes;
} MmfPfScoresArgs;                  /* host struct holding device pointers */
int mmf_pf_scores(const MmfPfScoresArgs* args /* host */, void* stream);
size_t mmf_pf_scores_workspace_bytes(int R, int M, int d);

/* ---------------------------------------------------------------- Particle-posterior density: log score, mode, entropy
 * The evaluation of crossmodal/eval_helpers.py:148-160 scores point estimates only; the scores above rank a belief as a
 * distribution but not by the logarithmic score, the "NLL" the filtering literature reports, and the only per-step point
 * estimate of a multimodal belief is its mean, which lies between the modes.  All three missing figures -- the log score of
 * the truth, the mode (the particle where the density is highest) and the entropy -- are functions of a kernel density
 * estimate of the weighted set evaluated at M + 1 points: M^2 pairs per set with an exp each, in torch ops an (M, M, d)
 * tensor or a chunked logsumexp loop over one.  Purely additive to ABI 42: a struct and two symbols of their own.
 * Per row r (R rows, e.g. T * N, of M particles x_m = states[r, m, :]) with an optional truth y = truth[r, :]:
 *   a_m, w_m = expf(a_m - max a), W_m = w_m / sum w      exactly as in "Particle-posterior scores"
 *   n_eff    = 1 / sum W_m^2
 *   mu_k     = sum W_m x_mk      sigma_k^2 = sum W_m (x_mk - mu_k)^2     two passes, in double, live particles only, no
 *                                                                       Bessel term
 *   c        = rule 1 (Silverman): (4 / ((d + 2) n_eff))^(1/(d+4))      rule 2 (Scott): n_eff^(-1/(d+4))
 *   h_k      = max(sigma_k c, min_bandwidth[k])       rules 1, 2;   rule 0: h_k = bandwidth[k] as given
 *   log p(q) = log sum_m W_m exp(-1/2 sum_k ((q_k - x_mk) / h_k)^2) - sum_k log h_k - (d/2) log 2 pi
 *   log_density[m] = log p(x_m) where w_m > 0, -inf where w_m = 0
 *   log_score      = log p(y)
 *   entropy        = - sum_{m live} W_m log p(x_m)     the resubstitution estimate; the zero weight selects a dead term away
 *   mode_index     = the lowest live m whose log_density[m] (the float that is written) is the row maximum
 *   mode           = a bit copy of states[r, mode_index, :]
 *   bandwidth_out[k] = h_k
 * A Gaussian product kernel, one bandwidth per dimension: the form that stays meaningful when the dimensions have different
 * units.  No full-covariance bandwidth and no leave-one-out.
 *   - a row without a live particle gives NaN in every float output and mode_index = -1;
 *   - a NaN y_k gives NaN in log_score only;
 *   - a dead particle's NaN row never reaches a sum.
 * log p is a true log-sum-exp: the running maximum is taken over the exponents log w_m - 1/2 z themselves, so it is finite
 * wherever the fp64 definition is finite and 1/2 sum ((q - x) / h)^2 is representable in fp32 -- a truth 5 sigma off a
 * collapsed set is the normal case of a log score.  The kernel takes the coordinates relative to float(mu_k) before it
 * multiplies them by the fp32 reciprocal 1 / h_k (h_k rounded to float), and works in base 2: e = log2 w_m - z (1/2 log2 e).
 * Determinism: every sum is taken in a fixed order and there are no floating-point atomics -- two calls give the same bits,
 * a row's result depends on neither R nor the other rows (the plan is a function of M alone), the particle outputs are the
 * same bits with and without a truth, and whichever outputs are null, the others are the bits of the full call.
 * Kernel plan: no (M, M) array in memory.  A row is dealt to nb = ceil(M / 512) workgroups in equal i-chunks; every workgroup
 * forms the row's max a, sum w, sum w^2, mu, sigma^2 and h itself, in one fixed order.  A thread holds one query particle
 * (M <= 512) or two in registers and walks j-tiles of 1024 particles staged through LDS as structure-of-arrays (d planes of
 * (x - mu) / h, one of log2 w), four j per broadcast 16-byte read; per query a running maximum and an fp32 sum rescaled once
 * per four j.  The truth is one more query per row, its j dealt over the threads of the row's first workgroup.  Entropy terms
 * in double and the (value, index) of the mode are reduced in a fixed order; with nb == 1 the workgroup writes the row,
 * otherwise it leaves a partial in the workspace and a finishing kernel takes a row's nb partials in block order.
 * mmf_pf_density_workspace_bytes(R, M, d): 16 R nb bytes for M > 512, 0 up to 512 (and for R, M or d below 1).
 * Limits, all decided on the host before any HIP call: null args / states, d outside 1 .. 4, M < 1, R < 0, rule outside
 * 0 .. 2, a bandwidth[k < d] (rule 0) or min_bandwidth[k < d] (rules 1, 2) that is not positive and finite, all six outputs
 * null, log_score without truth, a workspace that is needed and null, smaller than the query's answer or not 8-byte aligned,
 * an output (or the workspace) overlapping an input or another output -> MMF_EINVAL; M > 16384 or R * nb beyond a 32-bit
 * grid -> MMF_ETOOLARGE; R == 0 is a successful no-op. */
typedef struct MmfPfDensityArgs {
  int32_t R, M, d;                          /* R rows (e.g. T*N) of M particles */
  int32_t rule;                             /* 0: bandwidth[] as given; 1: Silverman; 2: Scott */
  float bandwidth[MMF_MAX_STATE_DIM];       /* host values, read with rule 0: bandwidth[k < d] > 0 and finite */
  float min_bandwidth[MMF_MAX_STATE_DIM];   /* host values, read with rules 1, 2: the floor of h_k, > 0 and finite */
  const float* states;                      /* (R, M, d) */
  const float* log_a;                       /* (R, M) or null = 0 */
  const float* log_b;                       /* (R, M) or null = 0 (history: log_weights_in + log_likelihoods) */
  const float* truth;                       /* (R, d); null allowed without log_score */
  float* log_density;                       /* (R, M) or null */
  float* log_score;                         /* (R) or null */
  float* entropy;                           /* (R) or null */
  float* mode;                              /* (R, d) or null */
  int32_t* mode_index;                      /* (R) or null */
  float* bandwidth_out;                     /* (R, d) or null */
  void* workspace;                          /* device, 8-byte aligned, mmf_pf_density_workspace_bytes(R, M, d) bytes; unused when that is 0 */
  size_t workspace_bytes;
} MmfPfDensityArgs;                         /* host struct holding device pointers */
int mmf_pf_density(const MmfPfDensityArgs* args /* host */, void* stream);
size_t mmf_pf_density_workspace_bytes(int R, int M, int d);

/* ---------------------------------------------------------------- Particle-posterior modes: quick-shift partition and masses
 * The evaluation of crossmodal/eval_helpers.py:148-160 scores one point estimate per step, and every summary above describes
 * the particle set as a whole: the density's `mode` is one particle and knows no second one.  The question a multimodal
 * belief raises first -- how many hypotheses does it hold, where is each, how much probability does each carry -- is answered
 * by quick shift (Vedaldi & Soatto, ECCV 2008) on the kernel density above: every particle points to its nearest neighbour
 * of higher density within a radius, the roots of that forest are the modes and a tree's weight is the mode's mass.  It is
 * deterministic, iterates nothing and has one parameter in bandwidth units; in torch ops it is an (M, M, d) broadcast and a
 * Python loop over clusters.  Purely additive to ABI 42: a struct and two symbols of their own.
 * Per row r (R rows, e.g. T * N, of M particles x_m = states[r, m, :]) with l_m = log_density[r, m] and h_k = bandwidth[r, k]
 * -- the arrays mmf_pf_density writes, but inputs here, whoever wrote them -- and the host scalars tau = link_radius (finite,
 * > 0, in bandwidth units) and K = max_modes (1 .. 8):
 *   a_m, t_m = a_m - max a, w_m = live_weight(t_m)     exactly as in "Particle-posterior scores"
 *   takes part     w_m > 0 and l_m is not NaN; every other particle is dead: parent = labels = -1, and its state row (NaN by
 *                  convention) is never read into anything
 *   j > i          l_j > l_i, or l_j == l_i and j < i: the fp32 values as given, compared as floats -- a strict total
 *                  order, so the links form no cycle, duplicated particles included
 *   D2(i, j)       = sum_k ((x_ik - x_jk) / h_k)^2; the kernel: the fp32 difference, times the fp32 reciprocal 1 / h_k, squared
 *                  and summed over k in order -- a set far from the origin partitions exactly as the same set at the origin
 *   parent[i]      among the j that take part with j > i and D2(i, j) <= tau^2 (fp32 tau * tau): the one of least D2, the
 *                  lowest j among equals; -1 (a root) if there is none
 *   labels[i]      the root of i's tree, a particle index; labels[root] == root
 *   count          the number of roots; 0 in a row where no particle takes part
 *   q_m            = (uint64) floor(w_m 2^40): exact for any float w_m <= 1, a row's sum stays below 2^54
 *   Q_root         = sum of q_m over labels[m] == root;   mass = Q_root / sum_m q_m, formed in double, written as float:
 *                  every sum is an integer, so its order cannot matter
 *   reported       the min(count, K) roots of greatest Q_root, the lower root first among equals, in that order; for rank c
 *                  index[r, c] the root, modes[r, c, :] a bit copy of its state, mass[r, c] its mass,
 *                  mean[r, c, :] = sum over its members of q_m x_m / Q_root in double, in one fixed order;
 *                  ranks beyond count hold -1 / NaN / 0 / NaN; a reported mode with Q_root = 0 has mass 0 and mean NaN
 * Determinism: two calls give the same bits, a row's result depends on neither R nor the other rows, and whichever outputs
 * are null, the others are the bits of the full call.  No floating-point atomics; the q_m are added into their roots with
 * 64-bit integer atomics, whose result does not depend on their order.
 * Kernel plan: no (M, M) array in memory.  The link pass is dealt like the scores and the density: nb = ceil(M / 512)
 * workgroups to a row, one i-particle of a thread in registers (M <= 512) or two, j-tiles of 1024 particles through LDS as
 * structure-of-arrays (d coordinate planes and one of l, NaN for a particle that does not take part), four j per broadcast
 * 16-byte read; per pair d subtract / multiply / accumulate steps, the order test, the radius test and a strict < against
 * the running best with j ascending, which is the lowest-j rule.  Every i writes its own parent: no partials, no finishing
 * launch of this pass.  The finish is one workgroup per row: parent into LDS, ceil(log2 M) double-buffered rounds of pointer
 * jumping leave labels; the q_m are added into their roots in LDS up to M = 8192 (MMF_PF_MODES_LDS_MASS_M: labels and masses
 * together fit the 160 KiB) and in the workspace beyond; K arg-max reductions on (Q_root, -root), each below the one before,
 * and the K d means in the fixed order of the other summaries' sums.
 * mmf_pf_modes_workspace_bytes(R, M, d): 8 R M bytes for M > 8192 (the masses) and 4 R M for the links, rounded up to 8
 * (read when parent is null, asked for always); 0 for R, M or d below 1.
 * Limits, all decided on the host before any HIP call: null args / states / log_density / bandwidth, d outside 1 .. 4, M < 1,
 * R < 0, max_modes outside 1 .. 8, a link_radius that is not finite and positive, all seven outputs null, a workspace that is
 * null, smaller than the query's answer or not 8-byte aligned, an output (or the workspace) overlapping an input or another
 * output -> MMF_EINVAL; M > 16384 or R * nb beyond a 32-bit grid -> MMF_ETOOLARGE; R == 0 is a successful no-op. */
#define MMF_PF_MODES_MAX 8
#define MMF_PF_MODES_LDS_MASS_M 8192
typedef struct MmfPfModesArgs {
  int32_t R, M, d;                  /* R rows (e.g. T*N) of M particles */
  int32_t max_modes;                /* K, 1 .. MMF_PF_MODES_MAX */
  float link_radius;                /* tau > 0 and finite, in bandwidth units */
  const float* states;              /* (R, M, d) */
  const float* log_a;               /* (R, M) or null = 0 */
  const float* log_b;               /* (R, M) or null = 0 (history: log_weights_in + log_likelihoods) */
  const float* log_density;         /* (R, M): mmf_pf_density's log_density, or any other ordering of the particles */
  const float* bandwidth;           /* (R, d): mmf_pf_density's bandwidth_out */
  int32_t* parent;                  /* (R, M) or null */
  int32_t* labels;                  /* (R, M) or null */
  int32_t* count;                   /* (R) or null */
  int32_t* index;                   /* (R, K) or null */
  float* modes;                     /* (R, K, d) or null */
  float* mass;                      /* (R, K) or null */
  float* mean;                      /* (R, K, d) or null */
  void* workspace;                  /* device, 8-byte aligned, mmf_pf_modes_workspace_bytes(R, M, d) bytes */
  size_t workspace_bytes;
} MmfPfModesArgs;                   /* host struct holding device pointers */
int mmf_pf_modes(const MmfPfModesArgs* args /* host */, void* stream);
size_t mmf_pf_modes_workspace_bytes(int R, int M, int d);

/* ---------------------------------------------------------------- Per-modality attribution of the crossmodal fusion
 * The crossmodal particle filter fuses its modalities as logsumexp_k(beta_k + l_k) (crossmodal/base_models/crossmodal_pf.py:106-139),
 * here in the epilogue of mmf_pf_measure, so the unimodal log-likelihoods never leave the chip; every summary above describes
 * the fused belief and none says which sensor it came from.  The reference looks at that by hand (likelihood maps with and
 * without the image, scripts/door_task/vis_pf_likelihoods.ipynb), and crossmodal_pf.py:123-129 computes per-modality normalised
 * likelihoods it never uses -- a modality whose likelihoods are larger in scale wins whatever beta says, so beta alone is not
 * the answer; the evidence-weighted share is.  Purely additive to ABI 42: a struct and a symbol of their own.
 * Per row r (R rows, e.g. T * N, of M particles x_m = states[r, m, :]) with the incoming log-weights a_m = log_w[r, m] (null:
 * 0, uniform), the K log-likelihood columns l_km = loglik[k][r, m] of the enabled modalities (mmf_pf_measure_multi evaluates
 * them on the same particles in one launch) and the modality log-weights beta_k = modality_logw[r * logw_stride + k] (null: 0,
 * as without a weight model):
 *   s_km = beta_k + l_km        L_m = logsumexp_k s_km           A = logsumexp_m a_m
 *   u_km = a_m + l_km           v_m = a_m + L_m
 *   W^k_m = exp(u_km - logsumexp_m u_k)      modality k's own posterior on the shared particles
 *   W_m   = exp(v_m  - logsumexp_m v)        the fused posterior: the filter's pre-resampling weights
 *   log_evidence[k]   = logsumexp_m u_km - A, k < K;   log_evidence[K] = logsumexp_m v_m - A (fused)
 *   responsibility[k] = rho_k = exp(beta_k + log_evidence[k] - log_evidence[K]) = sum_m W_m exp(s_km - L_m); they sum to 1
 *   ess[k]            = 1 / sum_m (W^k_m)^2;   ess[K] of W
 *   mean[k, :]        = sum_m W^k_m x_m;       mean[K, :] of W
 *   divergence[k]     = KL(W^k || W) = sum_{m: W^k_m > 0} W^k_m (log W^k_m - log W_m)
 *   overlap[j, k]     = sum_m sqrt(W^j_m W^k_m), the Bhattacharyya coefficient; stored symmetric bit for bit, 1 on the diagonal
 * Hence W = sum_k rho_k W^k and mean[K] = sum_k rho_k mean[k]; 0 <= divergence[k] <= -log rho_k; K = 1 gives rho = 1 and
 * divergence 0; identical columns give rho = softmax(beta), divergence 0 and overlap 1; modalities with disjoint support
 * give overlap 0 exactly and divergence[k] = -log rho_k.
 * Weights are those of "Particle-posterior scores", one pair of fp32 operations per log-weight: u = a + l, t = u - max_m u
 * (the maximum skips NaN), w = expf(t) where t <= 0, else 0 -- a NaN or -inf carries no weight; likewise inside L_m, formed in
 * fp32 as max_k s + logf(sum_k w(s_k - max_k s)): a NaN l_km counts as -inf.  A particle with a_m = -inf or NaN is dead under
 * every distribution and its state row (NaN by convention) is never read into a sum.  Normalised in double, once, at the end.
 *   - a modality with no weight on any live particle: log_evidence = -inf, responsibility = 0, and NaN in its ess, mean,
 *     divergence and its row and column of overlap;
 *   - a modality with beta_k = -inf (a weight model that knows of a blackout): responsibility = 0; its evidence, ess, mean
 *     and overlaps are those of its own posterior, and its divergence is +inf where it alone weighs a particle;
 *   - no modality with weight under a finite beta_k: the fused log_evidence = -inf, its ess and mean and every divergence NaN;
 *   - a row without a live particle (A is -inf or NaN): NaN everywhere.
 * Determinism: every sum is taken in a fixed order and there are no floating-point atomics -- two calls give the same bits,
 * a row's result depends on neither R nor the other rows (the plan is a function of M alone), and whichever outputs are
 * null, the others are the bits of the full call; an output that is null is not touched.
 * Kernel plan: a reduction.  One workgroup per row, a thread to every four particles, rounded up to a wave of 64, 512 threads
 * at most.  Pass 1 takes the K + 2 row maxima (of u_k, v and a) from the log columns; pass 2 reads the log columns again
 * (from L2: the same workgroup has just read them, at most 320 KiB) and the state rows, and keeps (K + 1)(2 + d) + K +
 * K (K - 1) / 2 + 1 sums per thread -- sum w, sum w^2, sum w x per distribution; sum w^k (t^k - t) per modality; sum
 * sqrtf(w^j w^k) per pair; sum exp(a - max a).  A thread loads four of its particles before it uses one; its sums are fp32
 * over those four, flushed to double; the 64 lanes of a wave are added as one more fp32 run (DPP, a fixed tree), the waves
 * ascending in double.  The finish is spread over 3 K + 1 threads; its logarithms of the totals are fp32 (an absolute 1e-7 in
 * numbers written as floats), its quotients double.  4 (1 + K + d) bytes per particle from memory, once; no workspace and no
 * finishing launch.
 * Limits, all decided on the host before any HIP call: null args / states / loglik[k < K], K outside 1 .. MMF_LOOP_MAX_MEAS,
 * d outside 1 .. 4, M < 1, R < 0, a modality_logw with logw_stride < K, all six outputs null, an output overlapping an input
 * or another output -> MMF_EINVAL; M > 16384 or R beyond a 32-bit grid -> MMF_ETOOLARGE; R == 0 is a successful no-op. */
typedef struct MmfPfModalitiesArgs {
  int32_t R, M, d;                  /* R rows (e.g. T*N) of M particles */
  int32_t K;                        /* enabled modalities, 1 .. MMF_LOOP_MAX_MEAS */
  int32_t logw_stride;              /* floats from one row of modality_logw to the next, >= K; not read when that is null */
  const float* states;              /* (R, M, d) */
  const float* log_w;               /* (R, M) or null = uniform (history: log_weights_in) */
  const float* loglik[MMF_LOOP_MAX_MEAS];  /* (R, M) each, the first K: the unimodal log-likelihoods, no beta added */
  const float* modality_logw;       /* (R, logw_stride), the first K of a row; or null = 0 */
  float* log_evidence;              /* (R, K + 1) or null */
  float* responsibility;            /* (R, K) or null */
  float* ess;                       /* (R, K + 1) or null */
  float* mean;                      /* (R, K + 1, d) or null */
  float* divergence;                /* (R, K) or null */
  float* overlap;                   /* (R, K, K) or null */
} MmfPfModalitiesArgs;              /* host struct holding device pointers */
int mmf_pf_modalities(const MmfPfModalitiesArgs* args /* host */, void* stream);

/* ---------------------------------------------------------------- Particle-posterior distances: two sets against each other
 * The evaluation of crossmodal/eval_helpers.py:148-160 compares a filter with the truth only, through the posterior mean;
 * every summary above judges ONE weighted particle set.  Nothing compares two posteriors: the filtered set of a step against
 * its smoothed set, 300 particles against 4096, one arithmetic mode, resampling scheme or modality mask against another.
 * These are the standard two-sample distances, per state dimension on the two weighted empirical CDFs and multivariate as the
 * energy distance (Szekely & Rizzo).  In torch ops the first is a cat + sort + two cumsums per dimension whose fp32 crossings
 * depend on the summation order, the second three cdists with an (Ma, Mb) array each.  Purely additive to ABI 42: a struct
 * and three symbols of their own.
 * There are R row pairs; row r of set A has Ma particles x_m = states_a[r, m, :], row r of set B has Mb particles
 * y_l = states_b[r, l, :], both of dimension d.  Ma != Mb is the normal case.  Each set has its own log-weights
 * a = log_a + log_b (one fp32 add; a null addend is 0, both null: uniform weights) and its own maximum.
 * Per dimension k, on K1's fixed-point weights (as "Particle-posterior quantiles"):
 *   q            = (uint32) floor(expf(a - max a) * 2^24), 0 for a = -inf or NaN, per set
 *   F_a, F_b     the two weighted empirical CDFs: 64-bit integer prefix sums of q, divided once, in double, by the set's total
 *   z_0 <= z_1 <= ..   the coordinates k of the particles with q > 0 of BOTH sets, ascending;  D_j = F_a(z_j) - F_b(z_j)
 *   wasserstein[r, k] = sum_j (z_{j+1} - z_j) |D_j|     the 1-Wasserstein (earth mover's) distance, in the state's own units
 *   cramer[r, k]      = sum_j (z_{j+1} - z_j) D_j^2     the Cramer distance, the integral of (F_a - F_b)^2: half the
 *                                                        one-dimensional energy distance, and without its cancellation
 *   ks[r, k]          = max_j |D_j| over the j that end a tie group (z_{j+1} > z_j)   Kolmogorov-Smirnov, in [0, 1]
 *   - the gaps are taken in double (exact for fp32 operands), the sums in double in one fixed order;
 *   - a particle with q = 0 is not in the union, whatever its state row holds (the histories carry NaN rows for dead
 *     particles); a tie may sort in any order: inside a tie group the gap is 0 and ks looks at group ends only;
 *   - every CDF value is an integer sum: two calls give the same bits, a row pair computed alone has the bits it has in a
 *     batch, and two identical sets give exactly 0 in all three.
 * Multivariate, on plain float weights (as "Particle-posterior scores": w = expf(a - max a), normalised once in double), with
 * s = scale[0 .. d) dividing the coordinates inside the norm (the kernel multiplies by the fp32 reciprocal):
 *   terms[r, :] = (E|(X - Y) / s|_2, E|(X - X') / s|_2, E|(Y - Y') / s|_2)     over all Ma Mb, Ma^2 and Mb^2 pairs
 *   energy[r]   = sqrt(max(2 terms[0] - terms[1] - terms[2], 0))               combined in double from the three double sums
 *   - all three expectations go through one device function with one dealing, a function of Ma and Mb alone: the same arrays
 *     passed as A and as B give energy == 0 exactly, two calls give the same bits, a row pair does not depend on R;
 *   - a zero weight selects its term away and never multiplies it.
 * Resolution of energy: it is the root of a difference of three sums of like size, so its floor is set by the fp32 pair
 * terms and the expf of the weights RELATIVE TO terms -- each of the three is good to a few 1e-7 of itself, energy^2
 * therefore to that share of 2 terms[0] + terms[1] + terms[2] -- not to energy: two posteriors closer than about 1e-3 of
 * their own spread are below it.  For near-identical posteriors read cramer and wasserstein, which have no cancellation.
 * A row pair in which either set has no live particle gives NaN in every output; everything else is finite.
 * Kernel plan: (1) a workgroup per (row pair, dimension) packs (order-preserving uint32 key of the coordinate) << 32 |
 * set bit | q into one uint64 per live particle of both sets in LDS -- q = 0 and the padding take the all-ones key --, padded
 * to the next power of two P >= max(Ma + Mb, 64), sorts them as mmf_pf_quantiles does, scans q in integers once per set and
 * makes one pass over the gaps between live neighbours; one wave for P <= 512, 256 threads beyond.  (2) the pair plan of
 * mmf_pf_scores on a cross product: one device function cross(I-set, J-set), i-particles in registers, the J-set in tiles of
 * 1024 through LDS, fp32 runs of 64 pairs flushed to double, dealt by the plan of the I-set (ceil(M / 512) workgroups);
 * (A, A) and (A, B) share one load of the A particles, (B, B) follows.  With Ma and Mb both <= 512 one workgroup takes the
 * row pair and writes it; otherwise every workgroup writes its sums to the workspace and a finishing kernel adds a row
 * pair's partial sums in order.  No floating-point atomics.
 * mmf_pf_distance_workspace_bytes(R, Ma, Mb, d): 24 R (nb_a + nb_b) bytes when Ma or Mb exceeds 512, else 0 (and 0 for an
 * argument below 1).  mmf_pf_distance_lds_bytes(Ma, Mb): the dynamic LDS of the sorting workgroup, 8 B per padded slot and one
 * spare slot per thread -- monotone in Ma + Mb, at most 160 KiB at the limit (beyond it: the value at the limit; 0 for an
 * argument below 1).
 * Limits, all decided on the host before any HIP call: null args / states_a / states_b, d outside 1 .. 4, Ma < 1, Mb < 1,
 * R < 0, a scale[k < d] that is not positive and finite, all five outputs null, a workspace that is needed (energy or terms
 * asked for, and the query's answer is not 0) and null, smaller than the query's answer or not 8-byte aligned, an output (or
 * the workspace) overlapping an input of either set or another output -> MMF_EINVAL; Ma + Mb > 16384 -- the union sort's
 * limit, and the one limit of the whole entry -- or a grid beyond 32 bits -> MMF_ETOOLARGE; R == 0 is a successful no-op.
 * wasserstein, cramer and ks all null skips the first kernel; energy and terms both null skips the second. */
typedef struct MmfPfDistanceArgs {
  int32_t R, Ma, Mb, d;                        /* R row pairs (e.g. T*N) of Ma against Mb particles */
  float scale[MMF_MAX_STATE_DIM];              /* host values, scale[k < d] > 0 and finite; 1 for plain Euclidean distance */
  const float *states_a, *log_a_a, *log_b_a;   /* (R, Ma, d), (R, Ma) or null = 0 */
  const float *states_b, *log_a_b, *log_b_b;   /* (R, Mb, d), (R, Mb) or null = 0 */
  float *wasserstein, *cramer, *ks;            /* (R, d) each, or null */
  float* energy;                               /* (R) or null */
  float* terms;                                /* (R, 3) or null */
  void* workspace;                             /* device, 8-byte aligned, mmf_pf_distance_workspace_bytes(R, Ma, Mb, d) bytes */
  size_t workspace_bytes;
} MmfPfDistanceArgs;                           /* host struct holding device pointers */
int mmf_pf_distance(const MmfPfDistanceArgs* args /* host */, void* stream);
size_t mmf_pf_distance_workspace_bytes(int R, int Ma, int Mb, int d);
size_t mmf_pf_distance_lds_bytes(int Ma, int Mb);

/* ---------------------------------------------------------------- Predictive mixtures: k-step-ahead forecasts, scored exactly
 * Everything above judges the present or the past of a run.  The predict step of torchfilter's particle filter (un-vendored:
 * SURVEY appendix A.2) -- x' = f(x, u) + L eps -- is what a forecast iterates, and after the LAST propagation of a roll-out the
 * noise need not be drawn: the predictive distribution is the Gaussian mixture with one shared covariance
 *   p(x) = sum_i W_i N(x; F_i, Q),   Q = L L^T,   sigma_k = sqrt(Q_kk)
 * whose mean, covariance, logarithmic score, PIT and CRPS are closed forms: strictly proper scores without a bandwidth, where
 * "Particle-posterior density" needs a kernel density estimate.  Purely additive to ABI 42: a struct and two symbols of their own.
 * Per row r (R rows, e.g. (T - h) * N, of M centres F_i = centres[r, i, :]) with an optional truth y = truth[r, :]:
 *   a_i, w_i = expf(a_i - max a), W_i = w_i / sum w      exactly as in "Particle-posterior scores"
 *   mean[k]          = sum_i W_i F_ik
 *   covariance[k, l] = sum_i W_i (F_ik - mean_k)(F_il - mean_l) + Q_kl          the difference before the product
 *   log_score        = logsumexp_i(log W_i - 1/2 |L^-1 (y - F_i)|^2) - sum_k log L_kk - d/2 log 2 pi
 *   pit[k]           = sum_i W_i Phi((y_k - F_ik) / sigma_k)
 *   spread[k]        = sum_i sum_j W_i W_j A(F_ik - F_jk; sqrt(2) sigma_k)      all M^2 pairs of a row
 *   crps[k]          = sum_i W_i A(y_k - F_ik; sigma_k) - 1/2 spread[k]
 *   A(m; s)          = m erf(m / (s sqrt 2)) + s sqrt(2 / pi) exp(-m^2 / (2 s^2))   E|Z| for Z ~ N(m, s^2)
 * One component gives the Gaussian closed forms.  mean, covariance, log_score and pit are taken in double throughout, the
 * log-sum-exp about the largest exponent, so a truth 50 sigma away has a finite log score.  The pair terms are fp32:
 * A(m; s) = s sqrt(2) g(m / (s sqrt 2)) with g(t) = t erf(t) + exp(-t^2) / sqrt(pi) evaluated as |t| + exp(-t^2) p(1 / (1 + |t| / 2)),
 * p a fitted polynomial of degree 9: within 7e-7 of g, relative, everywhere, and every term of the sums is positive.
 *   - scale_tril is read as a lower triangle with a positive diagonal; it is device memory and not checked;
 *   - a particle with w_i = 0 contributes nothing, whatever its row of centres holds (NaN, by convention): the zero weight
 *     selects the term away, it does not multiply it;
 *   - a row without a live particle gives NaN everywhere;
 *   - a NaN y_k gives NaN in log_score and in crps[k] and pit[k]; everything else stays finite;
 *   - mean, covariance and spread need no truth; log_score, pit or crps without one is refused.
 * Determinism: every sum is taken in a fixed order and there are no floating-point atomics -- two calls give the same bits, a
 * row's result depends on neither R nor the other rows, and the bits of an output do not depend on which others are asked for.
 * Kernel plan: (1) mean, covariance, log_score and pit: one workgroup of 256 threads per row, two passes over the row, sums
 * in double in the order of pf_summary.h; skipped when none of the four is asked for.  (2) spread and crps: the pair plan of
 * mmf_pf_scores with g in place of |.| -- nb = ceil(M / 512) workgroups to a row, one or two i-particles of a thread in
 * registers, j-tiles of 1024 through LDS as structure-of-arrays read as broadcasts, dead particles staged as zeros with zero
 * weight, fp32 runs of 64 pairs flushed to double, 2 d + 1 double sums per workgroup; with nb == 1 the workgroup writes the
 * row, otherwise a finishing kernel adds a row's nb partial sums in order.  Skipped when neither is asked for.
 * mmf_pf_predictive_workspace_bytes(R, M, d): 72 R nb bytes for M > 512, 0 up to 512 (and for R, M or d below 1); read only
 * when spread or crps is asked for.
 * Limits, all decided on the host before any HIP call: null args / centres / scale_tril, d outside 1 .. 4, M < 1, R < 0, all
 * six outputs null, log_score, pit or crps without truth, a workspace that is needed and null, smaller than the query's answer
 * or not 8-byte aligned, an output (or the workspace) overlapping an input or another output -> MMF_EINVAL; M > 16384 or
 * R * nb beyond a 32-bit grid -> MMF_ETOOLARGE; R == 0 is a successful no-op. */
typedef struct MmfPfPredictiveArgs {
  int32_t R, M, d;                  /* R rows (e.g. (T-h)*N) of M mixture components */
  const float* centres;             /* (R, M, d) */
  const float* log_a;               /* (R, M) or null = 0 */
  const float* log_b;               /* (R, M) or null = 0 (history: log_weights_in + log_likelihoods) */
  const float* scale_tril;          /* (d, d), the process noise's L */
  const float* truth;               /* (R, d); null allowed with mean, covariance and spread */
  float* mean;                      /* (R, d) or null */
  float* covariance;                /* (R, d, d) or null */
  float* log_score;                 /* (R) or null */
  float* pit;                       /* (R, d) or null */
  float* spread;                    /* (R, d) or null */
  float* crps;                      /* (R, d) or null */
  void* workspace;                  /* device, 8-byte aligned, mmf_pf_predictive_workspace_bytes(R, M, d) bytes; unused when that is 0 */
  size_t workspace_bytes;
} MmfPfPredictiveArgs;              /* host struct holding device pointers */
int mmf_pf_predictive(const MmfPfPredictiveArgs* args /* host */, void* stream);
size_t mmf_pf_predictive_workspace_bytes(int R, int M, int d);

/* ---------------------------------------------------------------- Particle-posterior belief maps: the density rasterised on a grid
 * The one analysis tool of the reference beside the RMSE tables of crossmodal/eval_helpers.py:148-160 is
 * scripts/door_task/vis_pf_likelihoods.ipynb: a grid over two state dimensions around the true state, one map per modality.
 * Every summary above reduces a particle set to numbers; this one is the picture of a multimodal belief: the 2-D marginal
 * of the product-kernel density of "Particle-posterior density" on Gx x Gy cells.  In torch ops two (R, M, G) factor
 * tensors and a bmm.  Purely additive to ABI 42: a struct and one symbol of their own, no workspace.
 * Per row r (R rows, e.g. T * N, of M particles x_m = states[r, m, :]) with the host values (dx, dy) = dims, (Gx, Gy) = cells,
 * (step_x, step_y) = step and the device values (c_x, c_y) = center[r, :], (h_x, h_y) = bandwidth[r, :]:
 *   a_m, w_m = expf(a_m - max a), W_m = w_m / sum w      exactly as in "Particle-posterior scores"
 *   u_i = fmaf(float(i) - 0.5f (Gx - 1), step_x, c_x)    the cell centres, in fp32; v_j likewise.  With an odd cell count the
 *                                                        middle cell is the centre, bit for bit
 *   density[r, j, i] = (2 pi h_x h_y)^-1 sum_{m live} W_m exp(-1/2 ((u_i - x_m,dx) / h_x)^2) exp(-1/2 ((v_j - x_m,dy) / h_y)^2)
 * (R, Gy, Gx), x fastest.  The other d - 2 dimensions are not read: the map is the marginal of the density mmf_pf_density
 * evaluates when bandwidth holds the two entries of its bandwidth_out.  The kernel forms an offset relative to the centre
 * before anything is scaled -- (float(i) - 0.5f (Gx - 1)) step_x - (x_m,dx - c_x), then times the fp32 reciprocal of h_x -- so a
 * set far from the origin maps like the same set at the origin; it accumulates the unnormalised w_m and scales a cell once,
 * by float(1 / (2 pi h_x h_y sum w)).
 *   - a particle with w_m = 0 is selected away, never multiplied away: its state row (NaN, by convention) is not read and
 *     reaches no operand;
 *   - a row without a live particle, a NaN in the row's centre, a bandwidth of the row that is not positive and finite:
 *     that row's map is NaN, and only that row's.
 * Determinism: every sum is taken in a fixed order and there are no floating-point atomics -- two calls give the same bits,
 * and a row's bits depend on neither R nor the other rows (the plan is a function of (M, Gx, Gy) alone).
 * Kernel plan: a workgroup of four waves per row and 64 x 64 block of cells (a 128-cell axis is two blocks), each wave
 * holding the block as 2 x 2 accumulator tiles of the exact-fp32 MFMA v_mfma_f32_32x32x2_f32, the tile's columns along x.  Every
 * workgroup forms max a and sum w (in double) over the whole row itself.  The waves take four contiguous chunks of
 * ceil(M / 4) particles, staged 64 at a time through LDS as (x - c_x, y - c_y, w), dead particles as zeros; per MFMA of two
 * particles a lane forms A = w exp(..v..) and B = exp(..u..) with one v_exp_f32 each: 128 M exponentials and 4096 M
 * multiply-adds per full block.  The waves meet once at the end through LDS and are added in wave order.
 * Limits, all decided on the host before any HIP call: null args / states / center / bandwidth / density, d outside 2 .. 4,
 * a dims[k] outside 0 .. d - 1 or dims[0] == dims[1], a cells[k] outside 2 .. 128, a step[k] that is not positive and finite,
 * M < 1, R < 0, the output overlapping an input -> MMF_EINVAL; M > 16384 or R times the blocks of a map beyond a 32-bit grid
 * -> MMF_ETOOLARGE; R == 0 is a successful no-op. */
typedef struct MmfPfRasterArgs {
  int32_t R, M, d;                  /* R rows (e.g. T*N) of M particles */
  int32_t dims[2];                  /* host values: the state dimensions along x and y, distinct, in 0 .. d - 1 */
  int32_t cells[2];                 /* host values: (Gx, Gy), each in 2 .. 128 */
  float step[2];                    /* host values: the cells' widths along x and y, positive and finite */
  const float* states;              /* (R, M, d) */
  const float* log_a;               /* (R, M) or null = 0 */
  const float* log_b;               /* (R, M) or null = 0 (history: log_weights_in + log_likelihoods) */
  const float* center;              /* (R, 2): where the row's window sits, along dims[0] and dims[1] */
  const float* bandwidth;           /* (R, 2): the kernel's bandwidths along dims[0] and dims[1] */
  float* density;                   /* (R, Gy, Gx) */
} MmfPfRasterArgs;                  /* host struct holding device pointers */
int mmf_pf_raster(const MmfPfRasterArgs* args /* host */, void* stream);

/* ---------------------------------------------------------------- K6, fused: one network call of the training backward
 * Recompute (the forward pass's f16x3 arithmetic), backward data path and weight / bias gradients of ONE per-particle
 * network over N * M rows in one kernel (the dynamics network: three launches -- encoder forward, trunk, encoder
 * backward), replacing mmf_particle_net_train_forward + _backward + _weight_grads of the reference's training step
 * (/root/reference/crossmodal/train_helpers.py:124-162 over door_models/dynamics.py:102-134, door_models/pf.py:63-107).
 *  packed_dual  mmf_pack_particle_net(.., MMF_PREC_F16X3_DUAL)
 *  kind         0 dynamics (n_res 3): g_next (N M, d) = dL / d x' in, d_raw (N M, d + 1) = dL / d (dir, gate) out,
 *               act / g_act scratch (N M, 64) fp32;  1 measurement (n_res 2): d_out (N M) = dL / d log-likelihood
 *  d_states     out (N M, d): the gradient THROUGH the network (the dynamics' direct path x' = x + .. is the caller's),
 *               plus d_states_base when that is given
 *  dz_first_h, sc_first, dz_join_h, sc_join, h_last_h: out, the compact (N M, 64) f16 rows + (N M) fp32 row scales the
 *               narrow reductions read (first-layer / join pre-activation gradients, head input)
 *  pw, pb       (NL, n_slots, 64, 64) / (NL, n_slots, 64) ACCUMULATED in place, slot = workgroup (grid =
 *               min(n_slots, 256, ceil(N M / 128))): zero them before the first call, sum over slots after the last
 */
typedef struct MmfTrainFusedArgs {
  const float* packed_dual;
  int32_t n_res, kind, d, N, M, n_slots;
  const float* states;
  const float* traj_bias;
  const float* d_out;
  const float* g_next;
  float* d_raw;
  float* act;
  float* g_act;
  float* d_states;
  void* dz_first_h;
  float* sc_first;
  void* dz_join_h;
  float* sc_join;
  void* h_last_h;
  float* pw;
  float* pb;
  const float* d_states_base; /* null, or (N M, d) values ADDED to what is written to d_states (may be d_states itself: the
                                 caller's running gradient is updated in place, no separate add pass) */
} MmfTrainFusedArgs;

int mmf_particle_net_train_fused(const MmfTrainFusedArgs* args /* host */, void* stream);
/* The same for several MEASUREMENT networks of one step in ONE launch (blockIdx.y = network; they differentiate
 * independently of each other): same d, rows, depth and n_slots, each with its own outputs and row slots.  At the
 * reference's training size (960 rows) a call is one tile per wave -- its latency -- whatever runs beside it. */
int mmf_particle_net_train_fused_multi(const MmfTrainFusedArgs* nets /* host, n */, int n, void* stream);

/* ---------------------------------------------------------------- K6: the particle filter's training recursion
 * One C call for the forward recursion of a train-mode (no resampling) particle filter over T steps and
 * one for its backward -- the caller /root/reference/crossmodal/train_helpers.py:124-162
 * (torchfilter.train.train_filter: forward_loop over a subsequence, MSE, backward) at any size, including
 * the reference's own 32 x 30 particles x 16 steps where per-launch host work dominates.
 *
 * forward (per step t):  x_t = f(x_{t-1}) + L eps_t  (K2 dynamics);  ll = logsumexp_k(ll_k(x_t) + beta_k)
 *   (K2 measurement);  logw_t = logw_{t-1} + ll - logsumexp,  est_t = sum_m exp(logw_t) x_t  (K1 mode 0).
 *   Only the particle sets states (T+1, N, M, d) and log-weights logw (T+1, N, M) are kept.
 * backward (t = T-1 .. 0): the K6 kernels on RECOMPUTED activations -- the step's stashes are rebuilt by
 *   mmf_particle_net_train_forward from states[t] / states[t+1] for `chunk_traj` trajectories at a time,
 *   into ONE reused pair of buffers (stash, dz) + the ReLU sign bits; weight-gradient partials accumulate in
 *   place over steps and chunks.  Peak memory: the chunk buffers + (T+1) particle sets, whatever T.
 *   (Chunks small enough to keep stash + dz inside the 256 MiB Infinity Cache were measured and lose to
 *   large ones -- DESIGN.md, K6: the caller picks chunk_traj for memory, not for cache residency.)
 *
 * Buffers (device, fp32, caller-owned).  K = n_meas networks (modalities), NLd = 3 + 2 n_res_dyn, NLm likewise.
 *  in:   dyn_* / meas_*[k]: packed      forward blob (mmf_pack_particle_net, `precision` for the forward pass),
 *                           packed_f32  exact-f32 blob (recompute), packed_t  blob of the transposed layers,
 *                           head_w (n_out, 64)
 *        dyn_bias (T, N, 64), meas_bias[k] (T, N, 64), meas_logw[k] = &beta[0][0][k] of a (T, N, logw_stride)
 *        array or null, noise (T, N, M, d), scale_tril (d, d), g_estimates (T, N, d)  [backward]
 *  io:   states (T+1, N, M, d), logw (T+1, N, M): slot 0 = initial belief (caller), slot t+1 = after step t
 *  out:  estimates (T, N, d)  [forward]
 *        backward: d_states0 (N, M, d), d_logw0 (N, M);
 *        per network: pw (NL+1, n_splits, 64, 64), pb (NL+1, n_splits, 64) weight / bias partials summed over
 *        steps; p_first (T, N n_slices, 64, 4), p_head (T, N n_slices, 4, 64), p_dout (T, N n_slices, 4),
 *        p_traj (T, N n_slices, 64): the narrow reductions per step (the caller adds slices / steps;
 *        d traj_bias[t][n] = sum_s p_traj[t][n][s], d beta_k[t][n] = sum_s p_dout_k[t][n][s][0])
 *  kept:  ll_steps (T, K, N, M) per-modality log-likelihoods ll_k = raw_k + b_k + beta_k of every step
 *  scratch: stash, dz (max(NLd, NLm) + 1, chunk_traj M, 64); raw (chunk_traj M, 8); d_raw (chunk_traj M, 8);
 *        loglik (N, M); g_states_a, g_states_b (N, M, d); g_logw_a, g_logw_b (N, M); d_tmp (chunk_traj M, d)
 */
typedef struct MmfTrainNet {
  const float* packed;      /* forward pass blob                                   */
  const float* packed_f32;  /* recompute blob (MMF_PREC_F32)                        */
  const float* packed_t;    /* transposed layers (backward data path)              */
  const float* head_w;      /* (n_out, 64)                                         */
  float* pw;                /* (NL+1, n_splits, 64, 64)                             */
  float* pb;                /* (NL+1, n_splits, 64)                                 */
  float* p_first;           /* (T, N n_slices, 64, 4)                               */
  float* p_head;            /* (T, N n_slices, 4, 64)                               */
  float* p_dout;            /* (T, N n_slices, 4)                                   */
  float* p_traj;            /* (T, N n_slices, 64)                                  */
  const float* packed_dual; /* ABI 37, fused = 1: MMF_PREC_F16X3_DUAL blob            */
} MmfTrainNet;

typedef struct MmfPfTrainArgs {
  int32_t T, N, M, d, n_meas, n_res_dyn, n_res_meas, logw_stride, precision;
  int32_t chunk_traj, n_splits, n_slices;
  MmfTrainNet dyn;
  MmfTrainNet meas[MMF_LOOP_MAX_MEAS];
  const float* dyn_bias;
  const float* meas_bias[MMF_LOOP_MAX_MEAS];
  const float* meas_logw[MMF_LOOP_MAX_MEAS];
  const float* noise;
  const float* scale_tril;
  const float* g_estimates;
  float* states;
  float* logw;
  float* estimates;
  float* d_states0;
  float* d_logw0;
  float* stash;
  uint32_t* mask;            /* scratch (max(NLd, NLm) + 1, chunk_traj M, 2): ReLU sign bits of the recomputed activations */
  float* dz;
  float* raw;
  float* d_raw;
  float* loglik;
  float* ll_steps;           /* (T, K, N, M): every step's per-modality log-likelihoods (forward -> backward) */
  float* g_states_a;
  float* g_states_b;
  float* g_logw_a;
  float* g_logw_b;
  float* d_tmp;
  int32_t* range_flag;
  float* dz_scale;           /* scratch: fp32 row scales of `dz` -- (max(NLd, NLm) + 1, chunk_traj M); fused: (sets, 2, chunk_traj M).
                                ABI 39: `stash` and `dz` are ALWAYS f16 arrays (activations as f16, pre-activation gradients as f16
                                relative to the largest magnitude of their 32-row tile, kept here; the weight-gradient products
                                of the f16 values are exact: f16 MFMA, fp32 accumulate).  The fp32 buffers of ABI 34 (`compact = 0`)
                                and the three-pass f16x3 recompute / backward of ABI 36 (`recompute_f16x3`, `backward_f16x3`) are
                                gone: superseded by `fused`, timings kept in profiles/r05/bench_train_fused_ab.txt */
  int32_t fused;             /* ABI 37.  1 (needs precision = MMF_PREC_F16X3): every network's recompute (in the forward pass's
                                own three-product f16 arithmetic, on `packed`), backward data path and weight gradients run as ONE
                                kernel per network call (mmf_particle_net_train_fused: layer inputs and pre-activation gradients
                                never reach HBM); each MmfTrainNet then carries `packed_dual`, and pw / pb are (NL, n_splits, 64, 64)
                                / (NL, n_splits, 64) partials, ZEROED by the caller, one slot per workgroup (n_splits <= 256 = the
                                largest grid).  stash / dz / dz_scale then only hold the three rows-by-64 slots the narrow
                                reductions read (layer slots 2 and NL).  fused_act, fused_g_act: scratch (chunk_traj M, 64) fp32.
                                0: three passes per network call with EXACT fp32 products (recompute on `packed_f32`, transposed
                                layers `packed_t` an MMF_PREC_F32 blob) over the f16 buffers -- the f32 engine mode's training path
                                and the cross-check of the fused kernel (MMF_TRAIN_FUSED=0) */
  float* fused_act;
  float* fused_g_act;
  int32_t fused_sets;        /* ABI 38.  >= n_meas > 1: stash / dz / dz_scale / d_tmp hold one set of row slots per
                                measurement network -- (sets, C, 64), (sets, 2, C, 64), (sets, 2, C), (sets, C, d) with
                                C = chunk_traj M -- and a step's measurement networks run as ONE launch
                                (mmf_particle_net_train_fused_multi).  0 / 1: one launch per network */
} MmfPfTrainArgs;

int mmf_pf_train_forward(const MmfPfTrainArgs* args /* host */, void* stream);
int mmf_pf_train_backward(const MmfPfTrainArgs* args /* host */, void* stream);

/* After mmf_pf_train_backward: one network's partial sums -> its parameter gradients in the order and layout of the
 * nn.Module parameters the reference's optimiser walks (train_helpers.py:124-162: torch autograd produces them per
 * parameter), plus the gradient of its hoisted per-trajectory term and of its modality log-weight column.
 *  grads      flat: w_in (64, d) | b_in (64) | encoder block1 w (64, 64), b | block2 w, b | join w (64, join_in: columns
 *             outside [join_state_off, +64) are zero) | per residual block: block1 w, b, block2 w, b | head w (n_out, 64) |
 *             head b (n_out)
 *  bias_grad  (T N, 64);  d_beta (T N, beta_stride) or null: column beta_col is written
 *  pw (NL + 1, S, 64, 64), pb (NL + 1, S, 64), p_first (T, N SL, 64, 4), p_head (T, N SL, 4, 64), p_dout (T, N SL, 4),
 *  p_traj (T, N SL, 64): MmfTrainNet's buffers (NL = 3 + 2 n_res); fused: the first-layer bias is column d of p_first
 *  scratch    32 x 516 floats */
typedef struct MmfPfTrainFinalizeArgs {
  int32_t T, N, SL, S, n_res, d, n_out, join_in, join_state_off, fused, beta_stride, beta_col;
  const float *pw, *pb, *p_first, *p_head, *p_dout, *p_traj;
  float *grads, *bias_grad, *d_beta, *scratch;
} MmfPfTrainFinalizeArgs;
int mmf_pf_train_finalize(const MmfPfTrainFinalizeArgs* args /* host */, void* stream);

/* ---------------------------------------------------------------- Training on the particle set: the mixture log score and its gradients
 * /root/reference/crossmodal/train_helpers.py:124-162 (torchfilter.train.train_filter) trains a filter on the mean-squared
 * error of its estimates and nothing else; the differentiable-filter literature (Jonschkowski et al. 2018, Kloss et al. 2021)
 * trains particle filters on the negative log-likelihood of the true state under a Gaussian mixture placed on the particles,
 * which sees spread and multimodality where the mean's MSE is blind.  Two additions, purely additive to ABI 42 (a struct and two
 * symbols of their own; MmfPfTrainArgs keeps its size):
 *
 * (1) mmf_pf_train_backward_sets: mmf_pf_train_backward with the direct loss gradients of every step's weighted set.
 *   g_states_steps[t] (N, M, d) and g_logw_steps[t] (N, M) are dL/d states[t+1] and dL/d logw[t+1] of MmfPfTrainArgs -- the set
 *   after step t, the one est_t is taken from, with normalised log-weights.  In the t = T-1 .. 0 loop the log-weight gradient
 *   handed to mmf_pf_reweight_backward is (the later step's) + g_logw_steps[t] -- at the last step g_logw_steps[t] alone --
 *   and the state gradient is (through est_t) + (the later step's) + g_states_steps[t], in that order.  Either pointer may be
 *   null; both null is mmf_pf_train_backward: the same launches, the same bits (one body serves both symbols).
 *
 * (2) mmf_pf_set_nll: the loss itself.  Per row r (R rows, e.g. T * N: one step of one trajectory) of M particles
 *   x_m = states[r, m, :] with log-weights a_m = logw[r, m] (not necessarily normalised), the true state y = truth[r, :] and the
 *   component scales sigma_j = scale[j] > 0 (device memory, not checked), the mixture sum_m p_m N(y; x_m, diag sigma^2):
 *     z_mj = (y_j - x_mj) / sigma_j              e_m = a_m - 1/2 sum_j z_mj^2
 *     nll  = logsumexp_m a_m - logsumexp_m e_m + sum_j log sigma_j + (d / 2) log 2 pi
 *     r = softmax(e)      p = softmax(a)
 *     g_states[r, m, j]  = g -r_m z_mj / sigma_j           d nll / d x_mj
 *     g_logw[r, m]       = g (p_m - r_m)                   d nll / d a_m
 *     g_log_scale[r, j]  = g (1 - sum_m r_m z_mj^2)        d nll / d log sigma_j, PER ROW: the caller sums the rows (and divides
 *                                                          by sigma_j for d / d sigma_j)
 *   with g = g_nll[r] (null: 1), multiplied last: a power of two scales every gradient exactly.  nll is what
 *   -mmf_pf_density's log_score reports with bandwidth = sigma fixed, so a filter is trained on what it is evaluated with.
 *   Both log-sum-exps are true ones, each about its own maximum: a truth 50 sigma from every particle, or sigma = 1e-3 with the
 *   truth 1.0 away, gives a finite nll and finite gradients.  The exponents and the sums are fp32, the last combination double.
 *   - a_m = -inf (or NaN) is a dead particle: it contributes exactly nothing, its state row (NaN, by convention) is not read,
 *     and its gradients are written as 0;
 *   - a row without a live particle, with a NaN in y, or whose every e_m is -inf: nll = NaN and all gradients of the row are 0.
 *   A forward call asks for nll alone; a backward call asks for gradients and recomputes (4 (d + 1) bytes read per particle,
 *   as many written).  Determinism: fixed summation order, no floating-point atomics -- two calls give the same bits, and row
 *   r's bits depend on neither R, nor its place in the batch, nor on which outputs are asked for.
 *   Kernel plan: up to M = 256 a wave owns a row (four rows to a workgroup of 256 threads: the reference trains on hundreds of
 *   rows of 30 particles), beyond that a workgroup of 512 threads does; three passes over the row (the maxima, the sums, the
 *   per-particle gradients), which re-read it through the caches -- nothing is staged per particle in LDS, so M is bounded only
 *   by int32.  Wave sums are the DPP butterfly, the waves are added in ascending order.
 *   Limits, decided on the host before any HIP call: null args / states / logw / truth / scale, all four outputs null, d outside
 *   1 .. 4, M < 1, R < 0, an output overlapping an input or another output -> MMF_EINVAL; R == 0 is a successful no-op. */
typedef struct MmfPfSetNllArgs {
  int32_t R, M, d;                  /* R rows (e.g. T*N) of M particles */
  const float* states;              /* (R, M, d) */
  const float* logw;                /* (R, M) */
  const float* truth;               /* (R, d) */
  const float* scale;               /* (d), device: the component scales sigma */
  const float* g_nll;               /* (R) or null = 1 */
  float* nll;                       /* (R) or null */
  float* g_states;                  /* (R, M, d) or null */
  float* g_logw;                    /* (R, M) or null */
  float* g_log_scale;               /* (R, d) or null */
} MmfPfSetNllArgs;                  /* host struct holding device pointers */
int mmf_pf_set_nll(const MmfPfSetNllArgs* args /* host */, void* stream);
int mmf_pf_train_backward_sets(const MmfPfTrainArgs* args /* host */, const float* g_states_steps /* (T, N, M, d) or null */,
                               const float* g_logw_steps /* (T, N, M) or null */, void* stream);

/* ---------------------------------------------------------------- Training on the particle set's scores: the gradients of CRPS and the energy score
 * The training loss of crossmodal/train_helpers.py:124-162 (torchfilter.train.train_filter) is the mean-squared error of the
 * estimates; the section above adds the mixture log score, which needs a kernel bandwidth that changes what is optimised and
 * whose gradient saturates for a truth several sigma from every particle.  CRPS and the energy score ("Particle-posterior
 * scores" above; Gneiting & Raftery 2007) are strictly proper with no bandwidth at all, in the state's own units, and their
 * gradient is bounded (|d / d x_m| <= W_m); they are the second loss on the weighted sets that mmf_pf_train_backward_sets
 * carries into the native recursion.  Purely additive to ABI 42: a struct and two symbols of their own.
 * The forward pass is NOT new: it is mmf_pf_scores as it stands, so a filter is trained on the bits it is evaluated with.
 * mmf_pf_scores_backward is its reverse.  Per row r of M particles x_m = states[r, m, :] with the truth y = truth[r, :],
 * the forward's own weights (a_m = log_a + log_b, w_m = live weight of a_m - max a, W = w / sum w) and s = scale, for the
 * loss L = sum_k g_k crps[k] + g_E energy with g_k = g_crps[r, k], g_E = g_energy[r]:
 *   t_mk = |x_mk - y_k|          s_mk = sum_l W_l |x_mk - x_lk|
 *   t_mE = |(x_m - y) / s|_2     s_mE = sum_l W_l |(x_m - x_l) / s|_2
 *   c_m  = sum_k g_k (t_mk - s_mk) + g_E (t_mE - s_mE)
 *   g_logw[r, m]      = W_m (c_m - sum_l W_l c_l)                              dL / da_m (the same for log_a and log_b)
 *   g_states[r, m, k] = W_m [ g_k (sgn(x_mk - y_k) - sum_l W_l sgn(x_mk - x_lk))
 *                           + g_E (u_k(x_m - y) - sum_l W_l u_k(x_m - x_l)) ]
 *   u_k(e) = e_k / (s_k^2 |e / s|_2), and 0 where e = 0;   sgn(0) = 0
 * (the 1/2 of the definition and the symmetry of the pair sum cancel; coinciding particles contribute 0).
 *   - a particle with w_m = 0 is dead: its state row is not read into any sum and both its gradients are WRITTEN as +0;
 *   - a row without a live particle has all gradients 0;
 *   - a term whose forward value is NaN -- crps[k] where y_k is NaN, energy where any y_k is NaN -- contributes nothing,
 *     whatever its upstream gradient holds (NaN included); the row's other terms contribute as defined;
 *   - the truth gets no gradient, and neither does the scale: it is a choice of units, not a parameter;
 *   - a null g_crps or g_energy leaves that score's terms out; the upstream gradients multiply inside c_m and the bracket,
 *     so scaling all of a row's upstream gradients by one power of two scales its outputs exactly.
 * Determinism: every sum is taken in a fixed order and there are no floating-point atomics -- two calls give the same bits,
 * and a row's bits depend on neither R, nor its place in the batch, nor which of the two outputs is asked for.
 * Kernel plan: the pair plan of mmf_pf_scores, no (M, M) array anywhere.  nb = ceil(M / 512) workgroups to a row, one or two
 * i-particles of a thread in registers, j-tiles of 1024 particles through LDS as structure-of-arrays, four j per broadcast
 * 16-byte read.  Every workgroup takes the row maximum and sum w over the whole row itself, in one fixed order.  Per
 * i-particle up to 3 d + 1 pair sums with w unnormalised (d absolute, d sign, one norm, d norm-gradient; one reciprocal
 * square root per pair, a pair at distance 0 selected away), fp32 over runs of 64 pairs and flushed to double; the division
 * by sum w is taken once, in double.  The kernel is compiled per null upstream gradient: a CRPS-only loss forms no norm, an
 * energy-only loss no sign sums.  g_states is written by the pair kernel; with nb == 1 so is g_logw, otherwise c_m, W_m and
 * the workgroups' partial sums of W c go to the workspace and a finishing kernel, a thread per particle, adds a row's nb
 * partial sums in order.  mmf_pf_scores_backward_workspace_bytes(R, M, d): 8 R (nb + 2 M) bytes for M > 512, 0 up to 512
 * (and for R, M or d below 1); it is needed for M > 512 whichever output is asked for.
 * Limits, all decided on the host before any HIP call: null args / states / truth, both upstream gradients null, both
 * outputs null, d outside 1 .. 4, M < 1, R < 0, a scale[k < d] that is not positive and finite, a workspace that is needed
 * and null, smaller than the query's answer or not 8-byte aligned, an output (or the workspace) overlapping an input or
 * another output -> MMF_EINVAL; M > 16384 or a grid beyond 32 bits -> MMF_ETOOLARGE; R == 0 is a successful no-op.
 * Two states closer than 1e-19 in every scaled coordinate count as coinciding in the energy terms. */
typedef struct MmfPfScoresBackwardArgs {
  int32_t R, M, d;                  /* R rows (e.g. T*N) of M particles */
  float scale[MMF_MAX_STATE_DIM];   /* host values, as in MmfPfScoresArgs */
  const float* states;              /* (R, M, d) */
  const float* log_a;               /* (R, M) or null = 0 */
  const float* log_b;               /* (R, M) or null = 0 */
  const float* truth;               /* (R, d) */
  const float* g_crps;              /* (R, d) or null: no CRPS terms */
  const float* g_energy;            /* (R) or null: no energy terms */
  float* g_states;                  /* (R, M, d) or null */
  float* g_logw;                    /* (R, M) or null */
  void* workspace;                  /* device, 8-byte aligned, mmf_pf_scores_backward_workspace_bytes(R, M, d) bytes; unused when that is 0 */
  size_t workspace_bytes;
} MmfPfScoresBackwardArgs;          /* host struct holding device pointers */
int mmf_pf_scores_backward(const MmfPfScoresBackwardArgs* args /* host */, void* stream);
size_t mmf_pf_scores_backward_workspace_bytes(int R, int M, int d);

/* ---------------------------------------------------------------- K7: per-trajectory MLP programs
 * The N-row networks around the filters (vector encoders layers.py:11-40,66-95; PF weight
 * model crossmodal_pf.py:74-106; virtual sensor kf.py:81-126; EKF weight model
 * crossmodal_kf.py:134-167; hoisted join-layer halves) as ONE launch per model: a list of
 * instructions interpreted per 16 rows by a workgroup.  Vectors (<= 128 wide) live in MMF_TRAJ_SLOTS
 * LDS slots.
 *   LOAD        slot[dst][0:out_dim] = io[io][row*io_stride + io_off + 0:out_dim]
 *   LINEAR      slot[dst] = act(W cat(slot[src[s]][src_off[s] : src_off[s]+src_dim[s]] ..) + b (+ slot[res]));  W is stored
 *               in `weights` at w_off as the A fragments of v_mfma_f32_16x16x4_f32: per source s, per group g of 16
 *               input columns (zero-padded), per tile mt of 16 outputs (out_pad = out_dim <= 64 ? 64 : 128):
 *               [g][mt][lane = 16 q + i][ks] = W[16 mt + i][first column of s + 16 g + 4 ks + q]; the bias (128
 *               floats, zero-padded) at b_off
 *   STORE       io[io][row*io_stride + io_off + 0:out_dim] = act(slot[src[0]])
 *   STORE_DIAG  io[io][row*io_stride + io_off + 0:d*d] = diag(act(slot[src[0]][0:d])), d = out_dim
 * Round 5 -- the reverse mode of a program is ANOTHER program over the same slot file (train_helpers.py:124-162: the
 * reference differentiates these networks with torch autograd, a GEMM + a reduction + an element-wise launch per
 * nn.Linear), built by trajprog.py from the forward list; it needs four more instructions, and LOAD / LINEAR write at
 * slot[dst][dst_off + ..] (LOAD applies `act`):
 *   MASK        slot[dst][dst_off + c] = io[..][c] > 0 ? slot[dst][dst_off + c] : 0     (backward of a ReLU, from the stashed output)
 *   ADD         slot[dst][dst_off + c] += slot[src[0]][src_off[0] + c]
 *   ZERO        slot[dst][dst_off + c] = 0
 *   LOAD_ADD    slot[dst][dst_off + c] += io[..][c]                     c < out_dim throughout
 * The transposed layers are LINEARs over a second blob; parameter gradients are mmf_traj_weight_grads over the rows
 * the two programs stashed.
 */
#define MMF_TRAJ_MAX_IO 8
#define MMF_TRAJ_SLOTS 8
#define MMF_TRAJ_LOAD 0
#define MMF_TRAJ_LINEAR 1
#define MMF_TRAJ_STORE 2
#define MMF_TRAJ_STORE_DIAG 3
#define MMF_TRAJ_MASK 4
#define MMF_TRAJ_ADD 5
#define MMF_TRAJ_ZERO 6
#define MMF_TRAJ_LOAD_ADD 7
#define MMF_TRAJ_ACT_NONE 0
#define MMF_TRAJ_ACT_RELU 1
#define MMF_TRAJ_ACT_SIGMOID 2
#define MMF_TRAJ_ACT_SQRT_SQ_PLUS 3   /* sqrt(x*x + fparam): kf.py:117-126 */

typedef struct MmfTrajInstr {
  int32_t op, dst;
  int32_t src[4];       /* source slots, -1 = unused */
  int32_t src_off[4];   /* first feature read from each source slot (multiple of 4) */
  int32_t src_dim[4];
  int32_t out_dim;
  int32_t w_off, b_off; /* float offsets into `weights`; b_off = -1: no bias */
  int32_t res;          /* residual slot or -1 */
  int32_t act;
  int32_t io, io_stride, io_off;
  float fparam;
  int32_t dst_off;      /* first feature written in slot[dst] (multiple of 4; LINEAR reads its residual there too) */
} MmfTrajInstr;

/*  prog     (n_instr) MmfTrajInstr on the DEVICE
 *  weights  device blob the instructions index
 *  io       HOST array of MMF_TRAJ_MAX_IO device pointers (inputs and outputs; unused = null)
 *  R        rows
 *  n_slots  LDS vector slots the program uses (1 + its largest slot index, <= MMF_TRAJ_SLOTS)
 *  vec_width  64 when no vector of the program is wider, else 128: the launch sizes its LDS for
 *           n_slots x 16 rows x vec_width (4 .. 66 KiB per workgroup of four waves, one 16-row task at a time)
 */
int mmf_traj_program(const MmfTrajInstr* prog, int n_instr, const float* weights,
                     float* const* io, int R, int n_slots, int vec_width, void* stream);

/* The weight blob of a program, gathered on the device from the parameters where they lie (an optimiser updates them in
 * place, so the descriptor table is built once per program): per part
 *   MMF_TRAJ_PACK_LAYER       fragments of W[0:rows][col0 : col0 + dim] (W row-major with row stride ld) for one source
 *   MMF_TRAJ_PACK_TRANSPOSED  fragments of the transposed block: output o < rows is column col0 + o of W, input
 *                             k < dim its row k -- the layer the reverse program multiplies by
 *   MMF_TRAJ_PACK_BIAS        128 floats, the first `rows` from src
 * written at blob + dst_off in the LINEAR layout above (out_pad = 64 | 128). */
#define MMF_TRAJ_PACK_LAYER 0
#define MMF_TRAJ_PACK_TRANSPOSED 1
#define MMF_TRAJ_PACK_BIAS 2
typedef struct MmfTrajPackDesc {
  uint64_t src;          /* device address of the fp32 parameter */
  int32_t kind, rows, ld, col0, dim, out_pad;
  int32_t dst_off, reserved;
} MmfTrajPackDesc;
int mmf_traj_pack(const MmfTrajPackDesc* desc /* device */, int n_desc, float* blob, void* stream);

/* Parameter gradients of a program's LINEARs from the rows its forward (every LOADed / LINEAR output: `stash`) and
 * its reverse program (every pre-activation gradient: `dz`) wrote: per descriptor
 *   grads[grad_off + o * grad_ld + k] = sum_row dz[row][dz_col + o] * stash[row][x_col + k]   o < out_dim, k < x_dim
 *   grads[bias_off + o]               = sum_row dz[row][dz_col + o]                            (bias_off >= 0)
 * on v_mfma_f32_16x16x4_f32 with rows as the contraction, in a fixed order (row slices in ascending order: no atomics).
 * Replaces autograd's Linear backward (one GEMM and one column reduction per nn.Linear).
 *  desc      (n_desc) on the DEVICE;  stash (R, stash_ld), dz (R, dz_ld) fp32
 *  grads     flat output, every descriptor's block written (not accumulated)
 *  partials  (n_slices, n_grads) scratch when n_slices > 1 (rows are cut into n_slices equal runs, <= 64), else null
 */
typedef struct MmfTrajGradDesc {
  int32_t x_col, x_dim, dz_col, out_dim;
  int32_t grad_off, grad_ld, bias_off, reserved;
} MmfTrajGradDesc;
int mmf_traj_weight_grads(const MmfTrajGradDesc* desc, int n_desc, const float* stash, int stash_ld, const float* dz,
                          int dz_ld, float* grads, int n_grads, float* partials, int n_slices, int R, void* stream);

/* The 8192 -> 64 linear layer behind the convolutions of a training step (door_models/layers.py:59-60, the
 * nn.Linear(8 * 32 * 32, units) of the image encoder), forward and both backward products in exact fp32 on
 * v_mfma_f32_16x16x4_f32, fixed summation order; replaces the library GEMMs of torch's Linear forward / backward.
 *  x (R, K) fp32, w (64, K) row-major = nn.Linear.weight, b (64) or null, K % 512 == 0
 *   forward:  y (R, 64) = x w^T + b; partial: scratch (K / 512, R, 64) -- the K chunks meet in ascending order
 *   backward: dx (R, K) = g w (null: skipped);  dw (64, K) = g^T x;  db (64) = column sums of g (null: skipped) */
int mmf_fc64_train_forward(const float* x, const float* w, const float* b, float* y, float* partial, int R, int K,
                           void* stream);
int mmf_fc64_train_backward(const float* g, const float* x, const float* w, float* dx, float* dw, float* db, int R,
                            int K, void* stream);

/* ---------------------------------------------------------------- K3: EKF algebra + fusion
 * Replaces torchfilter's EKF predict/update (A S A^T + L L^T; K = S-(S- + R)^-1;
 * mu = mu- + K(z - mu-); S = (I-K)S-) for K sub-filters and the reference's
 * fusion of their beliefs: crossmodal (base_models/crossmodal_kf.py:153-167 via
 * utility.py:4-11) or unimodal information form (base_models/unimodal_kf.py:204-242).
 * One trajectory per lane, all d x d algebra in registers.
 *
 *  A        (K, N, d, d)  dynamics Jacobians
 *  mu_pred  (K, N, d)     predicted means
 *  q_tril   (K, d, d)     dynamics noise scale_tril per sub-filter (Q = L L^T)
 *  z        (K, N, d)     virtual-sensor observations
 *  r_tril   (K, N, d, d)  virtual-sensor scale matrices (R = T T^T; need not be triangular)
 *  fuse_w   (K, N, d)     crossmodal weights (fusion 1) or null
 *  mu       (K, N, d)     out: corrected sub-filter means
 *  Sigma    (K, N, d, d)  in: previous covariances; out: corrected covariances
 *  mu_f     (N, d), Sigma_f (N, d, d)  fused belief (fusion != 0), else may be null
 *  fusion   0 none, 1 crossmodal, 2 unimodal
 *  feedback 0: sub-filters keep their own beliefs (the reference's effective behaviour,
 *           SURVEY.md appendix C Q1); 1: fused belief is written back into every sub-filter
 */
int mmf_ekf_step(const float* A, const float* mu_pred, const float* q_tril, const float* z,
                 const float* r_tril, const float* fuse_w, float* mu, float* Sigma,
                 float* mu_f, float* Sigma_f, int N, int d, int K, int fusion, int feedback,
                 void* stream);

/* mmf_ekf_step whose write-back is gated by a DEVICE word: `feedback` applies only where *feedback_gate != 0
 * (null = always).  Carries the reference's batch-global blackout test -- DoorCrossmodalKalmanFilter.forward
 * takes the branch WITHOUT write-back as soon as any frame of the batch is blacked out
 * (/root/reference/crossmodal/door_models/crossmodal_kf.py:59-62) -- into the
 * native step loop without a host read per step. */
int mmf_ekf_step_gated(const float* A, const float* mu_pred, const float* q_tril, const float* z,
                       const float* r_tril, const float* fuse_w, float* mu, float* Sigma,
                       float* mu_f, float* Sigma_f, int N, int d, int K, int fusion, int feedback,
                       const int32_t* feedback_gate, void* stream);

/* K6: reverse mode of mmf_ekf_step without fusion (fusion = 0; the fusions of the K sub-filters
 * are a handful of element-wise torch ops on (K, N, d) and keep their autograd form).  Inputs as
 * the forward call's, Sigma_in = the covariances BEFORE the step; g_mu (K, N, d) / g_Sigma
 * (K, N, d, d): gradients of the corrected beliefs (either may be null = zero).  Outputs (any may
 * be null): g_A, g_mu_pred, g_z, g_r_tril, g_Sigma_in, shaped like their forward operands.
 * Used by the "hip" training backend for every EKF the reference trains end to end
 * (crossmodal/train_helpers.py:124-162; base_models/crossmodal_kf.py:88-151).
 */
int mmf_ekf_step_backward(const float* A, const float* mu_pred, const float* q_tril, const float* z,
                          const float* r_tril, const float* Sigma_in, const float* g_mu,
                          const float* g_Sigma, float* g_A, float* g_mu_pred, float* g_z,
                          float* g_r_tril, float* g_Sigma_in, int N, int d, int K, void* stream);

/* ---------------------------------------------------------------- unscented transform (UKF)
 * torchfilter's UnscentedKalmanFilter / VirtualSensorUnscentedKalmanFilter (absent, un-pinned
 * dependency of the reference, cf. crossmodal/door_models/kf.py:14-28 for the EKF sibling):
 * sigma points of N Gaussian beliefs, and the weighted moments of the propagated points.
 *  mu (N, d), Sigma (N, d, d); scale = sqrt(d + lambda);
 *  points (N, 2d+1, d): [mu, mu + scale L[:, i], mu - scale L[:, i]] with L = chol(Sigma)
 *  not_pd: int32 on the device or null, OR-ed with 1 when a covariance is not positive definite
 */
int mmf_ukf_sigma_points(const float* mu, const float* Sigma, float scale, float* points,
                         int32_t* not_pd, int N, int d, void* stream);
/*  points (N, 2d+1, d) propagated sigma points; wm0 / wc0: mean / covariance weight of point 0,
 *  wi: weight of every other point; q_tril (d, d): dynamics noise (Q = L L^T)
 *  -> mu_pred (N, d), Sigma_pred (N, d, d) = sum_i wc_i (X_i - mu)(X_i - mu)^T + Q
 *  The mean weights must be NORMALISED, wm0 + 2 d wi = 1 (Julier's and Merwe's are; so is any set that reproduces a
 *  constant): the sums are taken about point 0, mu = X_0 + wi sum_i (X_i - X_0), which keeps fp32 accurate where
 *  wm0 ~ -1e4 (Merwe's default alpha = 1e-2) would cancel.  A wm0 off by more than a few float32 ulps of the largest
 *  of wm0, 2 d wi (both arrive rounded to float32) is refused with MMF_EINVAL.
 */
int mmf_ukf_moments(const float* points, float wm0, float wc0, float wi, const float* q_tril,
                    float* mu_pred, float* Sigma_pred, int N, int d, void* stream);

/* R11: fusion of K virtual sensors before a single EKF (crossmodal_kf.py:291-359 mode 1;
 * unimodal_kf.py:56-115 mode 2, quirk Q5 preserved: see csrc/ekf.hip).
 *  z (K, N, d), tril (K, N, d, d), w (K, N, d) (mode 1) -> z_out (N, d), tril_out (N, d, d)
 */
int mmf_fuse_virtual_sensors(const float* z, const float* tril, const float* w, float* z_out,
                             float* tril_out, int N, int d, int K, int mode, void* stream);

/* All T steps of a fused EKF in one call (host loop; replaces torchfilter's Filter.forward_loop
 * over crossmodal_kf.py:88-151 / unimodal_kf.py:162-250): per step, mmf_dynamics_jacobian for
 * each of the K sub-filters at its current belief mean, then mmf_ekf_step.  Step-indexed
 * arrays are laid out (T, K, N, ...) so that step t's block is what mmf_ekf_step takes.
 */
typedef struct MmfEkfLoopArgs {
  int32_t T, N, d, K;
  int32_t fusion, feedback;  /* as mmf_ekf_step                                              */
  int32_t n_res_dyn;
  int32_t precision;         /* of dyn_packed (the Jacobian launches)                          */
  int32_t* range_flag;       /* device status word or null: MMF_FLAG_RANGE (f16x3), MMF_FLAG_GAVE_UP (persistent) */
  const float* dyn_packed[MMF_LOOP_MAX_MEAS];  /* blobs of the dynamics networks (mmf_pack_particle_net) */
  const float* dyn_bias[MMF_LOOP_MAX_MEAS];    /* (T*N, 64) hoisted control terms               */
  const float* q_tril;       /* (K, d, d)                                                      */
  const float* z;            /* (T, K, N, d)      virtual-sensor observations                  */
  const float* r_tril;       /* (T, K, N, d, d)   virtual-sensor scale matrices                */
  const float* fuse_w;       /* (T, K, N, d) crossmodal weights (fusion 1) or null             */
  float* mu;                 /* (K, N, d)     sub-filter means, in/out                          */
  float* Sigma;              /* (K, N, d, d)  sub-filter covariances, in/out                    */
  float* mu_pred;            /* (K, N, d)     scratch                                           */
  float* A;                  /* (K, N, d, d)  scratch                                           */
  float* Sigma_f;            /* (N, d, d)     fused covariance of the last step (fusion != 0)   */
  float* estimates;          /* (T, N, d) out: fused mean, or sub-filter 0's mean for fusion 0  */
  const int32_t* feedback_gate; /* (T) device words or null: step t writes the fused belief back (feedback) only where
                                gate[t] != 0 -- the reference's batch-global blackout branch
                                (door_models/crossmodal_kf.py:59-62) decided on the device, no host read per step  */
  int32_t persistent;        /* ABI 40. != 0: the whole loop as ONE persistent launch (mmf_ekf_persistent_plan > 0);
                                mu_pred and A are not touched; same bits as the loop of launches                  */
  int32_t n_sync_words;      /* 4-byte words of sync_words (>= mmf_ekf_persistent_sync_words(N, K, d))            */
  uint32_t* sync_words;      /* persistent: device workspace of the in-launch hand-offs between the K sub-filters'
                                workgroups (tagged 8-byte granules), zeroed by the call; a hand-off that times
                                out ORs MMF_FLAG_GAVE_UP into range_flag: discard this loop, run it as launches   */
} MmfEkfLoopArgs;            /* host struct holding device pointers                            */

int mmf_ekf_forward_loop(const MmfEkfLoopArgs* args /* host */, void* stream);

/* ABI 42.  mmf_ekf_forward_loop that also keeps the posterior covariance as every step leaves it (upstream torchfilter's
 * belief_covariance after each forward of crossmodal_kf.py:88-151 / unimodal_kf.py:162-250):
 *   Sigma_steps (T, N, d, d), required: the fused Sigma_f for fusion != 0 (also where feedback is gated off), sub-filter 0's
 *   Sigma for fusion 0 -- the matrix that goes with estimates[t].
 * Written by whichever form runs: the persistent launch stores the matrix it holds in registers next to the estimate, the
 * loop of launches copies it after each step.  An argument of its own and not a field: MmfEkfLoopArgs keeps its size, so a
 * binding built against ABI 40 / 41 still describes it. */
int mmf_ekf_forward_loop_belief(const MmfEkfLoopArgs* args /* host */, float* Sigma_steps, void* stream);

/* The persistent form of the EKF step loop (MmfEkfLoopArgs.persistent; csrc/ekf_persistent.inc): a wave owns 8
 * trajectories of ONE sub-filter for all T steps -- belief in registers, the dynamics network's weights in LDS, per step
 * the forward-mode Jacobian tile and the d x d algebra; K > 1 sub-filters meet once per step and trajectory through L2.
 * Replaces the 2 T launches of mmf_ekf_forward_loop (crossmodal_kf.py:88-151, unimodal_kf.py:162-250).
 *   mmf_ekf_persistent_plan: number of workgroups it would use (0: not eligible -- more than two rounds of tiles per wave,
 *   or a device with too few CUs to keep every workgroup resident).  d must be 2 or 3, n_res_dyn 3. */
int mmf_ekf_persistent_plan(int N, int K);
size_t mmf_ekf_persistent_sync_words(int N, int K, int d);

/* ---------------------------------------------------------------- innovation statistics and NIS gating of the Kalman step
 * Replaces the update of upstream torchfilter's ExtendedKalmanFilter (_update_step; the recursion behind every Kalman filter
 * of the reference, external dependency), which forms the innovation and its covariance, uses them for the
 * gain and discards them: neither it nor the filters built on it (crossmodal_kf.py:88-151, unimodal_kf.py:162-250) can report
 * a likelihood, a consistency statistic, or refuse an outlying measurement.  Purely additive to ABI 42: two symbols and a
 * struct of their own; MmfEkfLoopArgs keeps its size.
 * Per sub-filter k and trajectory n of one step (observation matrix = I), with S- = A Sigma A^T + L L^T and R = T T^T:
 *   nu = z - mu-          S = S- + R          nis = nu^T S^-1 nu          loglik = -1/2 (nis + log det S + d log 2 pi)
 *   accepted = nis_gate < 0 (no gating)  or  nis <= nis_gate;  a NaN nis is rejected.
 * An accepted measurement leaves the bits of mmf_ekf_step_gated; a rejected one leaves mu = mu-, Sigma = S-, the values the
 * step formed on the way, bit for bit.  Fusion and write-back then run unchanged on what every sub-filter holds: a rejected
 * sub-filter enters the fusion with its predicted belief.  nis and loglik are written for rejected measurements too.
 * nis is an fma chain over S^-1 nu with the inverse the gain uses; log det S comes from a Cholesky factorisation of S in
 * registers with the deterministic log of mmf_detmath.h (an S that is not positive definite -> loglik NaN).
 *   nis, loglik (K, N) float, accepted (K, N) int32 (1 / 0): any of them may be null.
 * mmf_ekf_step_innov: the other operands as mmf_ekf_step_gated's (feedback_gate may be null), and its argument checks;
 *   also MMF_EINVAL: d outside 1..4, K outside 1..4, a NaN nis_gate, an output (mu, Sigma, mu_f, Sigma_f, nis, loglik,
 *   accepted) whose bytes overlap an input's or another output's.  N == 0 is a successful no-op.  All decided on the host
 *   before any HIP call.
 * mmf_ekf_forward_loop_innov: mmf_ekf_forward_loop[_belief] with that step, as the LOOP OF LAUNCHES: args->persistent is
 *   ignored -- the persistent launch (csrc/ekf_persistent.inc) keeps no innovation and is not taken, as the particle filter's
 *   is not taken for a recorded history.  innov is required, Sigma_steps (T, N, d, d) may be null.  Argument checks as
 *   mmf_ekf_forward_loop's, d in 1..4, and no record on top of an operand of the loop; T == 0 or N == 0 is a successful no-op. */
int mmf_ekf_step_innov(const float* A, const float* mu_pred, const float* q_tril, const float* z,
                       const float* r_tril, const float* fuse_w, float* mu, float* Sigma,
                       float* mu_f, float* Sigma_f, int N, int d, int K, int fusion, int feedback,
                       const int32_t* feedback_gate, float nis_gate, float* nis, float* loglik, int32_t* accepted,
                       void* stream);
typedef struct MmfEkfInnovArgs {
  float nis_gate;            /* < 0: no gating                                                  */
  float* nis_steps;          /* (T, K, N) or null                                               */
  float* loglik_steps;       /* (T, K, N) or null                                               */
  int32_t* accepted_steps;   /* (T, K, N) or null                                               */
} MmfEkfInnovArgs;           /* host struct holding device pointers                             */
int mmf_ekf_forward_loop_innov(const MmfEkfLoopArgs* args /* host */, const MmfEkfInnovArgs* innov /* host */,
                               float* Sigma_steps /* or null */, void* stream);

/* ---------------------------------------------------------------- RTS smoothing of an extended Kalman filter's recorded run
 * E[x_t | y_1..T] of a Gaussian belief by the Rauch-Tung-Striebel backward sweep.  Upstream torchfilter's
 * ExtendedKalmanFilter (the recursion behind every Kalman filter of the reference; external dependency) keeps
 * no history and has no smoother, and the evaluation that this project restates (crossmodal/eval_helpers.py:139-142 runs
 * forward_loop over a recorded trajectory, :148-160 scores its estimates) reports the FILTERED means although all T
 * observations are at hand.  Purely additive to ABI 42: a struct and a symbol of its own.
 * Steps t = 0 .. T - 1 are the steps of mmf_ekf_forward_loop; (m_t, S_t) the filtered belief step t left; L the constant
 * process-noise factor; A_t, x^_{t+1} the dynamics Jacobian and prediction at (m_t, u_{t+1}).  For t < T - 1:
 *   P-_{t+1} = A_t S_t A_t^T + L L^T          G_t = S_t A_t^T (P-_{t+1})^-1
 *   m^s_t = m_t + G_t (m^s_{t+1} - x^_{t+1})  P^s_t = S_t + G_t (P^s_{t+1} - P-_{t+1}) G_t^T
 * from (m^s_{T-1}, P^s_{T-1}) = (m_{T-1}, S_{T-1}).  lag >= 0: E[x_t | y_1..min(t + lag, T - 1)] -- the same step from the
 * FILTERED belief of step e = min(t + lag, T - 1), for s = e - 1 .. t; lag = 0 returns (mu, Sigma) bit for bit, any
 * lag >= T - 1 the full sweep's bits (both sweeps run one device function).  lag < 0: the full sweep.
 * Two-slice moments (full sweep only) of the linearised residual r_t = x_{t+1} - x^_{t+1} - A_t (x_t - m_t), with
 * C_t = G_t P^s_{t+1}:
 *   resid_mean[t] = e_t = m^s_{t+1} - x^_{t+1} - A_t (m^s_t - m_t)
 *   resid_m2[t]   = P^s_{t+1} - A_t C_t - (A_t C_t)^T + A_t P^s_t A_t^T + e_t e_t^T          RAW (not centred)
 * -- the quantities mmf_pf_smooth_pair_moments leaves for a particle filter, under the same names.
 * Three kernels (csrc/ekf_smooth.hip): gains (one thread per transition: P-, G, the inversion), then the full sweep (one
 * lane per trajectory, T - 1 dependent steps) or the fixed-lag sweep (one thread per (t, n), at most lag steps).  fp32,
 * every product-sum an explicit fma in a fixed order: two calls give the same bits and trajectory n's results do not
 * depend on N.  T == 1 copies (mu, Sigma) to the outputs.
 * Limits: 1 <= d <= 4, otherwise MMF_EINVAL; T N <= 2^31 - 257, beyond -> MMF_ETOOLARGE.  A null args / mu / Sigma /
 * q_tril / mu_s / Sigma_s, with T >= 2 a null A / mu_pred / gain / Sigma_pred, T < 0, N < 0, one of resid_mean / resid_m2
 * without the other, either of them with lag >= 0, or an output whose bytes overlap an input's or another output's
 * -> MMF_EINVAL.  T == 0 or N == 0 is a successful no-op.  All decided on the host before any HIP call. */
typedef struct MmfEkfSmoothArgs {
  int32_t T, N, d;
  int32_t lag;               /* < 0: the full smoother                                          */
  const float* mu;           /* (T, N, d)         filtered means                                */
  const float* Sigma;        /* (T, N, d, d)      filtered covariances                          */
  const float* A;            /* (T - 1, N, d, d)  Jacobians at (m_t, u_{t+1})                   */
  const float* mu_pred;      /* (T - 1, N, d)     predictions f(m_t, u_{t+1})                   */
  const float* q_tril;       /* (d, d) DEVICE, row-major                                        */
  float* mu_s;               /* (T, N, d)         out: smoothed means                           */
  float* Sigma_s;            /* (T, N, d, d)      out: smoothed covariances                     */
  float* gain;               /* (T - 1, N, d, d)  out: G_t (written by the gains kernel, read by the sweeps) */
  float* Sigma_pred;         /* (T - 1, N, d, d)  workspace: P-_{t+1}                           */
  float* resid_mean;         /* (T - 1, N, d)     or null: not computed                         */
  float* resid_m2;           /* (T - 1, N, d, d)  or null: not computed                         */
} MmfEkfSmoothArgs;          /* host struct holding device pointers                             */
int mmf_ekf_smooth(const MmfEkfSmoothArgs* args /* host */, void* stream);

/* ---------------------------------------------------------------- LSTM baselines: the recurrence
 * The two-layer nn.LSTM(in_dim, 512, 2) of DoorLSTMFilter / PushLSTMFilter over a whole (T, N, in_dim) sequence, the
 * hidden state carried in and out (crossmodal/door_models/lstm.py:94, push_models/lstm.py:96: `lstm_out,
 * self.lstm_hidden = self.lstm(fused_features, self.lstm_hidden)`).  PyTorch's gate order and formulas: gates i, f, g, o
 * of W_ih x + b_ih + W_hh h + b_hh, sigma on i, f, o and tanh on g (both the deterministic forms of mmf_detmath.h:
 * mmf_det_sigmoid, absolute error <= 3e-7, and mmf_det_tanh, RELATIVE error <= 3.3e-7 measured and held to 7e-7 -- small
 * pre-activations and cell states keep their digits), c' = f c + i g, h' = o tanh(c').  Exact fp32 products
 * (v_mfma_f32_32x32x2_f32) in every MMF_PRECISION mode: a step is bound by the hand-off between workgroups, not by its
 * ~0.2 GFLOP at N = 32.  csrc/lstm.hip.
 *
 *   mmf_lstm_blob_floats(in_dim): floats of the packed weights; in_dim a multiple of 8 in [8, 512], else 0.  Layout:
 *     per layer l (K_0 = in_dim + 512, K_1 = 1024), per workgroup g < 64, 32 x K_l floats [k / 2][k & 1][row q], row
 *     q = gate * 8 + j standing for row gate * 512 + 8 g + j of [W_ih | W_hh]; then (b_ih + b_hh) per layer as [g][q]:
 *     2048 (K_0 + K_1 + 2) floats in all.
 *   mmf_lstm_pack: the eight nn.LSTM tensors (weight_ih_l0 (2048, in_dim), weight_hh_l0 (2048, 512), bias_ih_l0,
 *     bias_hh_l0 (2048), then the same of layer 1 with in_dim = 512) -> that layout, in one device pass.
 *   mmf_lstm_persistent_plan(N, T): workgroups of the persistent form (> 0), 0 when not eligible (N > 256, a device
 *     without room for 128 resident workgroups, or no device), MMF_EINVAL for N < 1 or T < 1.
 *   mmf_lstm_sync_words(N): 4-byte words of MmfLstmArgs.sync_words: [abort word, padded to 16 B][64 progress words]
 *     [2 layers][2 parities][512][N] 8-byte granules; 0 for N < 1.
 *   mmf_lstm_forward: the whole sequence; persistent != 0 -> ONE launch (falls back to the loop of launches where the
 *     plan is 0), otherwise T + 1 launches.  Both forms give the same bits.  T = 0: no launch, hT / cT are copies of
 *     h0 / c0, and x and h2 (both empty) may be null.  Refused with MMF_EINVAL, nothing written: in_dim not a multiple
 *     of 8 in [8, 512], N < 1, T < 0, hT == h0 or cT == c0, n_sync_words < mmf_lstm_sync_words(N), a null pointer.
 */
#define MMF_LSTM_HIDDEN 512
#define MMF_LSTM_LAYERS 2

typedef struct MmfLstmArgs {
  int32_t T, N, in_dim;
  int32_t persistent;        /* != 0: ONE persistent launch where mmf_lstm_persistent_plan(N, T) > 0                 */
  const float* x;            /* (T, N, in_dim) layer-0 input (T = 0: may be null)                                   */
  const float* h0;           /* (2, N, 512) initial hidden state                                                    */
  const float* c0;           /* (2, N, 512) initial cell state                                                      */
  float* hT;                 /* (2, N, 512) out: final hidden state (not h0)                                        */
  float* cT;                 /* (2, N, 512) out: final cell state (not c0)                                          */
  float* h2;                 /* (T, N, 512) out: layer 1's hidden state at every step (nn.LSTM's output; T = 0: may
                                be null)                                                                            */
  const float* packed;       /* mmf_lstm_pack                                                                       */
  int32_t* range_flag;       /* or null; MMF_FLAG_GAVE_UP = "a hand-off of the persistent launch timed out: discard the
                                outputs and run the call again as launches"                                         */
  uint32_t* sync_words;      /* device workspace (mmf_lstm_sync_words), zeroed by the call; word 0 is the abort word */
  size_t n_sync_words;       /* 4-byte words of sync_words                                                          */
} MmfLstmArgs;               /* host struct holding device pointers                                                 */

size_t mmf_lstm_blob_floats(int in_dim);
int mmf_lstm_pack(const float* w_ih0, const float* w_hh0, const float* b_ih0, const float* b_hh0, const float* w_ih1,
                  const float* w_hh1, const float* b_ih1, const float* b_hh1, float* packed, int in_dim, void* stream);
int mmf_lstm_persistent_plan(int N, int T);
size_t mmf_lstm_sync_words(int N);
int mmf_lstm_forward(const MmfLstmArgs* args /* host */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMF_H */
