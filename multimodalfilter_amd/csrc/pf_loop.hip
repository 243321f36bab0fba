// Host-side step loop of the particle filter: one C call enqueues every kernel of T filter
// steps (dynamics, one measurement launch per modality, reweight + resample) on the caller's
// stream, back to back.  Replaces the Python loop of torchfilter's Filter.forward_loop
// (external dependency; call site /root/reference/crossmodal/eval_helpers.py:139-142) for the
// fused models: no interpreter work, tensor allocation or pointer marshalling between steps,
// so small problems (the reference's own evaluation: a few dozen trajectories x 300
// particles) are bound by kernel time instead of ~0.15 ms/step of host overhead.

#include "mmf_common.h"

// ess_threshold > 0: ESS-triggered resampling (mmf_pf_forward_loop_adaptive), resampled_steps (T, N) or null
// ws (mmf_pf_forward_loop_dedup): the run-table workspace, or null.  With it, plain systematic resampling (mmf_pf_dedup_plan)
// runs the dynamics network once per DISTINCT resampled ancestor: K1 of steps 0 .. T-2 writes the run table instead of
// gathering (mmf_pf_resample_runs), the dynamics launch of steps 1 .. T-1 consumes it (mmf_pf_dynamics_runs) reading the
// ancestors' rows from the buffer the previous step propagated; step 0's dynamics (the incoming belief is a full particle
// set) and step T-1's K1 (the belief the caller sees is complete) are the kernels of every other loop.  Same bits.
// h (mmf_pf_forward_loop_history): the same launches with other pointers.  Step t propagates into slice t of
// h->states_steps (`prop`) instead of `other`, K1 still gathers into `cur` -- a scratch buffer, never a history slice --, and
// where a step reads what the previous one PROPAGATED (no resampling, the run table) it reads slice t - 1 (`rd`).  `cur` /
// `other` / `lw_cur` / `lw_other` keep swapping as names, so final_location is what it is without a history.  Same bits.
// reg (mmf_pf_forward_loop_regularised): after the K1 launch of every resampling branch one mmf_pf_regularise launch on the
// buffer K1 gathered into (`cur`), with K1's weighted mean, covariance and ESS -- K1 in its recording form, into the step's
// slices of the records or into reg's scratch -- and, with a threshold, its decisions.  No run table: jittered particles
// have no runs.  The launch sits inside K1's pair of timing events.
static int pf_enqueue_steps(const MmfPfLoopArgs* a, void* stream, bool with_events, float ess_threshold = 0.f,
                            int32_t* resampled_steps = nullptr, const MmfPfDedupWorkspace* ws = nullptr,
                            const MmfPfHistory* h = nullptr, const MmfPfLoopRegularise* reg = nullptr) {
  if (!a) return MMF_EINVAL;
  const bool adaptive = ess_threshold > 0.f;
  if (reg) {
    if (a->resample_mode == 0 || ws) return MMF_EINVAL;
    if ((!a->cov_steps && !reg->cov) || (!a->ess_steps && !reg->ess)) return MMF_EINVAL;
    if (adaptive && !resampled_steps && !reg->resampled) return MMF_EINVAL;
    if (reg->noise_mode != 0 && reg->noise_mode != 2) return MMF_EINVAL;
    if (reg->noise_mode == 0 && !reg->noise) return MMF_EINVAL;
  }
  if (a->T < 0 || a->N < 1 || a->M < 1 || a->n_meas < 1 || a->n_meas > MMF_LOOP_MAX_MEAS) return MMF_EINVAL;
  if (a->resample_mode < 0 || a->resample_mode > 2) return MMF_EINVAL;
  if (!a->dyn_packed || !a->dyn_bias || (!a->noise && a->noise_mode != 2) || !a->scale_tril || !a->states_a || !a->states_b ||
      !a->logw_a || !a->logw_b || !a->loglik || !a->estimates)
    return MMF_EINVAL;
  if (a->resample_mode != 0 && !a->uniforms) return MMF_EINVAL;
  const bool soft = a->resample_mode != 0 && a->soft_alpha > 0.f && a->soft_alpha < 1.f;
  if (a->estimate_argmax && !a->estimate_scratch) return MMF_EINVAL;
  const bool runs = ws && ws->rank && ws->run_anc && ws->run_start && ws->n_runs && !adaptive &&
                    mmf_pf_dedup_plan(a->M, a->d, a->resample_mode, a->soft_alpha,
                                      a->cov_steps || a->ess_steps || a->log_evidence_steps) == 1;
  const size_t row = static_cast<size_t>(a->N);
  const size_t nm = row * a->M;
  float* cur = a->states_a;   // belief on entry
  float* other = a->states_b;
  float* lw_cur = a->logw_a;
  float* lw_other = a->logw_b;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (h) {  // the belief's log-weights on entry: step 0's slice and the copy of its own
    const size_t bytes = nm * sizeof(float);
    hipError_t e = hipMemcpyAsync(h->logw_in0, lw_cur, bytes, hipMemcpyDeviceToDevice, hs);
    if (e == hipSuccess && h->logw_in_steps && a->T > 0)
      e = hipMemcpyAsync(h->logw_in_steps, lw_cur, bytes, hipMemcpyDeviceToDevice, hs);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  int ev = 0;  // optional timing events: [sample][dynamics, measure x n_meas, resample][start, end]
  const int stride = a->event_stride > 1 ? a->event_stride : 1;
  bool sampled = false;  // an event record costs a barrier packet: long loops sample every stride-th step
  auto mark = [&]() {
    if (sampled && with_events) {
      hipError_t e = hipEventRecord(static_cast<hipEvent_t>(a->events[ev++]), hs);
      if (e != hipSuccess) return static_cast<int>(e);
    }
    return 0;
  };
  for (int t = 0; t < a->T; ++t) {
    int rc;
    sampled = a->events && t % stride == stride / 2;  // the middle step of every stride-long window
    if ((rc = mark())) return rc;
    const bool runs_in = runs && t > 0;            // the previous step left a run table and its propagated rows in `cur`
    const bool runs_out = runs && t + 1 < a->T;    // this step leaves them for the next
    const size_t slice = static_cast<size_t>(t) * nm * a->d;
    float* prop = h ? h->states_steps + slice : other;  // where this step's propagated set lives
    // what the dynamics launch reads: a gathered set in `cur`, or -- with a history -- the slice the previous step propagated
    const float* rd = h && t > 0 && (a->resample_mode == 0 || runs_in) ? h->states_steps + (slice - nm * a->d) : cur;
    // the log-weights K1 starts from and leaves: with a history, slices t and t + 1 (the last step's go where they always went)
    const float* lw_in = h && h->logw_in_steps && t > 0 ? h->logw_in_steps + t * nm : lw_cur;
    float* lw_out = h && h->logw_in_steps && t + 1 < a->T ? h->logw_in_steps + (t + 1) * nm : lw_other;
    if (runs_in && a->noise_mode == 2)
      rc = mmf_pf_dynamics_runs_philox(a->dyn_packed, a->n_res_dyn, a->precision, rd, a->dyn_bias + t * row * MMF_UNITS,
                                       a->noise_seed, a->noise_step0 + static_cast<unsigned>(t), a->noise_traj0, a->scale_tril,
                                       ws->rank, ws->run_anc, ws->run_start, ws->n_runs, prop, a->range_flag, a->N, a->M,
                                       a->d, stream);
    else if (runs_in)
      rc = mmf_pf_dynamics_runs(a->dyn_packed, a->n_res_dyn, a->precision, rd, a->dyn_bias + t * row * MMF_UNITS,
                                a->noise + t * nm * a->d, a->scale_tril, ws->rank, ws->run_anc, ws->run_start, ws->n_runs,
                                prop, a->range_flag, a->N, a->M, a->d, stream);
    else if (a->noise_mode == 2)
      rc = mmf_pf_dynamics_philox(a->dyn_packed, a->n_res_dyn, a->precision, rd, a->dyn_bias + t * row * MMF_UNITS,
                                  a->noise_seed, a->noise_step0 + static_cast<unsigned>(t), a->noise_traj0, a->scale_tril,
                                  prop, a->range_flag, a->N, a->M, a->d, stream);
    else
      rc = mmf_pf_dynamics(a->dyn_packed, a->n_res_dyn, a->precision, rd, a->dyn_bias + t * row * MMF_UNITS,
                           a->noise + t * nm * a->d, a->scale_tril, prop, a->range_flag, a->N, a->M, a->d,
                           stream);
    if (rc) return rc;
    if ((rc = mark())) return rc;
    // parity certificates keep every step's log-likelihoods and ancestors (null on the timed path)
    float* ll = a->loglik_steps ? a->loglik_steps + t * nm : a->loglik;
    int32_t* anc = a->indices_steps ? a->indices_steps + t * nm : nullptr;
    {
      for (int k = 0; k < a->n_meas; ++k) {
        const float* lw = a->meas_logw[k] ? a->meas_logw[k] + t * row * a->logw_stride : nullptr;
        if ((rc = mark())) return rc;
        rc = mmf_pf_measure(a->meas_packed[k], a->n_res_meas, a->precision, prop,
                            a->meas_bias[k] + t * row * MMF_UNITS, lw, a->logw_stride, ll, k > 0,
                            a->range_flag, a->N, a->M, a->d, stream);
        if (rc) return rc;
        if ((rc = mark())) return rc;
      }
    }
    float* est = a->estimates + t * row * a->d;
    // this step's slices of the belief record (null: the non-recording kernels)
    float* cov = a->cov_steps ? a->cov_steps + t * row * a->d * a->d : nullptr;
    float* ess = a->ess_steps ? a->ess_steps + t * row : nullptr;
    float* lev = a->log_evidence_steps ? a->log_evidence_steps + t * row : nullptr;
    int32_t* took = resampled_steps ? resampled_steps + t * row : nullptr;
    if (reg) {  // the jitter reads K1's covariance, ESS and decisions: scratch where the caller records none
      if (!cov) cov = reg->cov;
      if (!ess) ess = reg->ess;
      if (adaptive && !took) took = reg->resampled;
    }
    if (a->estimate_argmax) {
      // the particle with the largest pre-resampling weight; K1's weighted mean goes to the scratch.  In the plain
      // resampling loop the incoming weights are uniform from the second step on (see below)
      const bool uniform_in = a->resample_mode != 0 && !soft && !adaptive && t > 0;
      rc = mmf_pf_argmax_estimate(ll, uniform_in ? nullptr : lw_in, prop, est, a->N, a->M, a->d, stream);
      if (rc) return rc;
      est = a->estimate_scratch;
    }
    if ((rc = mark())) return rc;
    if (adaptive) {
      // a kept trajectory carries its weights forward, so the log-weights travel every step (as with soft resampling)
      const float* u = a->uniforms + t * (a->resample_mode == 1 ? row : nm);
      rc = mmf_pf_reweight_resample_adaptive(ll, lw_in, prop, u, est, cur, lw_out, anc, a->N, a->M, a->d, a->resample_mode,
                                             soft ? a->soft_alpha : 1.0f, ess_threshold, took, cov, ess, lev, stream);
      if (rc) return rc;
    } else if (soft) {
      // torchfilter's soft resampling: survivors carry importance weights, so the log-weights travel every step
      const float* u = a->uniforms + t * (a->resample_mode == 1 ? row : nm);
      rc = mmf_pf_reweight_resample_belief(ll, lw_in, prop, u, est, cur, lw_out, anc, a->N, a->M, a->M, a->d,
                                           a->resample_mode, a->soft_alpha, cov, ess, lev, stream);
      if (rc) return rc;
    } else if (a->resample_mode == 0) {
      rc = mmf_pf_reweight_resample_belief(ll, lw_in, prop, nullptr, est, nullptr, lw_out, nullptr, a->N,
                                           a->M, a->M, a->d, 0, 1.0f, cov, ess, lev, stream);
      if (rc) return rc;
      float* s = cur; cur = other; other = s;  // propagated particles are the new belief
    } else if (runs_out) {
      // the run table instead of the gathered particles: the propagated rows stay where they are and become `cur`
      // (the incoming weights are uniform from the second step on and no step but the last writes them: see below)
      // (a history that keeps the log-weights has the uniform -log M written into its next slice)
      rc = mmf_pf_resample_runs(ll, t == 0 ? lw_cur : nullptr, prop, a->uniforms + t * row, est,
                                h && h->logw_in_steps ? lw_out : nullptr, anc, ws->rank,
                                ws->run_anc, ws->run_start, ws->n_runs, a->N, a->M, a->d, cov, ess, lev, stream);
      if (rc) return rc;
      float* s = cur; cur = other; other = s;
    } else {
      const float* u = a->uniforms + t * (a->resample_mode == 1 ? row : nm);
      // every step of this loop resamples, so from the second step on the incoming weights are the
      // uniform -log M the previous step would have written, and only the last step's are ever read
      // again: 8 of the 40 B per particle-step stay out of HBM
      rc = mmf_pf_reweight_resample_belief(ll, t == 0 ? lw_cur : nullptr, prop, u, est, cur,
                                           t == a->T - 1 || (h && h->logw_in_steps) ? lw_out : nullptr, anc, a->N, a->M, a->M, a->d,
                                           a->resample_mode, 1.0f, cov, ess, lev, stream);
      if (rc) return rc;  // resampled particles land back in `cur`
    }
    if (reg) {  // every branch that gets here with reg gathered into `cur` (resample_mode != 0, no run table)
      MmfPfRegulariseArgs r{};
      r.N = a->N; r.M = a->M; r.d = a->d; r.shrink = reg->shrink;
      r.states = cur; r.cov = cov; r.ess = ess; r.mean = est; r.resampled = adaptive ? took : nullptr;
      r.noise = reg->noise_mode == 0 ? reg->noise + t * nm * a->d : nullptr;
      r.noise_seed = reg->noise_seed; r.noise_step = reg->noise_step0 + static_cast<unsigned>(t);
      r.noise_traj0 = reg->noise_traj0; r.noise_mode = reg->noise_mode;
      r.scale = reg->scale;
      for (int i = 0; i < MMF_MAX_STATE_DIM; ++i) r.floor[i] = reg->floor[i];
      r.bandwidth = reg->bandwidth_steps ? reg->bandwidth_steps + t * row : nullptr;
      if ((rc = mmf_pf_regularise(&r, stream))) return rc;
    }
    if ((rc = mark())) return rc;
    float* l = lw_cur; lw_cur = lw_other; lw_other = l;
  }
  if (h && a->resample_mode == 0 && a->T > 0) {
    // no step gathered: the belief is the last slice of the history; one copy puts it where final_location says
    const hipError_t e = hipMemcpyAsync(cur, h->states_steps + static_cast<size_t>(a->T - 1) * nm * a->d,
                                        nm * a->d * sizeof(float), hipMemcpyDeviceToDevice, hs);
    if (e != hipSuccess) return static_cast<int>(e);
  }
  // tell the caller where the belief ended up: bit 0 = states in states_b, bit 1 = log-weights in logw_b
  if (a->final_location)
    *a->final_location = (cur == a->states_b ? 1 : 0) | (lw_cur == a->logw_b ? 2 : 0);
  return 0;
}


extern "C" int mmf_pf_forward_loop(const MmfPfLoopArgs* a, void* stream) {
  MmfPfLoopArgs launches;
  if (a && a->persistent) {  // ONE launch for all T steps (small problems)
    const int rc = mmf_internal_pf_persistent(a, stream);
    if (rc != MMF_INTERNAL_NOT_RESIDENT) return rc;
    // this device cannot hold the persistent grid (a partition, or fewer CUs than planned for): the loop of launches
    // computes the same bits
    launches = *a;
    launches.persistent = 0;
    a = &launches;
  }
  return pf_enqueue_steps(a, stream, true);
}

extern "C" int mmf_pf_forward_loop_dedup(const MmfPfLoopArgs* a, const MmfPfDedupWorkspace* ws, void* stream) {
  MmfPfLoopArgs launches;
  if (a && a->persistent) {  // the persistent launch is what it was; only its fallback to launches takes the workspace
    const int rc = mmf_internal_pf_persistent(a, stream);
    if (rc != MMF_INTERNAL_NOT_RESIDENT) return rc;
    launches = *a;
    launches.persistent = 0;
    a = &launches;
  }
  return pf_enqueue_steps(a, stream, true, 0.f, nullptr, ws);
}

extern "C" int mmf_pf_forward_loop_adaptive(const MmfPfLoopArgs* a, float ess_threshold, int32_t* resampled_steps, void* stream) {
  if (!a || a->resample_mode == 0) return MMF_EINVAL;  // a threshold needs a resampling mode
  if (!(ess_threshold > 0.f && ess_threshold <= 1.f)) return MMF_EINVAL;
  MmfPfLoopArgs launches;
  if (a->persistent) {  // eligibility as mmf_pf_forward_loop's: plain systematic resampling, weighted-average estimates
    const int rc = mmf_internal_pf_persistent(a, stream, ess_threshold, resampled_steps);
    if (rc != MMF_INTERNAL_NOT_RESIDENT) return rc;
    launches = *a;
    launches.persistent = 0;
    a = &launches;
  }
  return pf_enqueue_steps(a, stream, true, ess_threshold, resampled_steps);
}

// The loop that keeps its history for mmf_pf_smooth (include/mmf.h): always the loop of launches -- the persistent form
// keeps no per-step arrays, as with indices_steps -- whichever of the three loops above the other arguments select.
extern "C" int mmf_pf_forward_loop_history(const MmfPfLoopArgs* a, const MmfPfHistory* h, float ess_threshold,
                                           int32_t* resampled_steps, const MmfPfDedupWorkspace* ws, void* stream) {
  if (!a || !h || !h->states_steps || !h->logw_in0 || !a->loglik_steps) return MMF_EINVAL;
  if (a->resample_mode != 0 && !a->indices_steps) return MMF_EINVAL;
  const bool adaptive = ess_threshold != 0.f;
  if (adaptive && (a->resample_mode == 0 || !(ess_threshold > 0.f && ess_threshold <= 1.f))) return MMF_EINVAL;
  const bool soft = a->resample_mode != 0 && a->soft_alpha > 0.f && a->soft_alpha < 1.f;
  if ((a->resample_mode == 0 || soft || adaptive) && !h->logw_in_steps) return MMF_EINVAL;  // the weights travel
  MmfPfLoopArgs launches = *a;
  launches.persistent = 0;
  return pf_enqueue_steps(&launches, stream, true, adaptive ? ess_threshold : 0.f, adaptive ? resampled_steps : nullptr, ws, h);
}

// The loop with regularised resampling (include/mmf.h): always the loop of launches, no run table; with a history the
// checks of mmf_pf_forward_loop_history, with a threshold those of mmf_pf_forward_loop_adaptive.
extern "C" int mmf_pf_forward_loop_regularised(const MmfPfLoopArgs* a, const MmfPfHistory* h, float ess_threshold,
                                               int32_t* resampled_steps, const MmfPfLoopRegularise* reg, void* stream) {
  if (!a || !reg || a->resample_mode == 0) return MMF_EINVAL;
  const bool adaptive = ess_threshold != 0.f;
  if (adaptive && !(ess_threshold > 0.f && ess_threshold <= 1.f)) return MMF_EINVAL;
  if (h) {
    if (!h->states_steps || !h->logw_in0 || !a->loglik_steps || !a->indices_steps) return MMF_EINVAL;
    const bool soft = a->soft_alpha > 0.f && a->soft_alpha < 1.f;
    if ((soft || adaptive) && !h->logw_in_steps) return MMF_EINVAL;  // the weights travel
  }
  MmfPfLoopArgs launches = *a;
  launches.persistent = 0;
  return pf_enqueue_steps(&launches, stream, true, adaptive ? ess_threshold : 0.f, adaptive ? resampled_steps : nullptr, nullptr,
                          h, reg);
}

// Open-loop rollout x_t = f(x_{t-1}, u_t): replaces torchfilter's DynamicsModel.forward_loop (call
// sites /root/reference/crossmodal/eval_helpers.py:135-137, scripts/door_task/eval_dynamics.py:36-38).
extern "C" int mmf_dynamics_forward_loop(const float* packed, int n_res, int precision, const float* x0,
                                         const float* traj_bias, float* out, int32_t* range_flag, int T, int N,
                                         int d, void* stream) {
  if (!packed || !x0 || !traj_bias || !out || T < 0 || N < 1) return MMF_EINVAL;
  const size_t row = static_cast<size_t>(N);
  const float* cur = x0;
  for (int t = 0; t < T; ++t) {
    float* nxt = out + t * row * d;
    const int rc = mmf_pf_dynamics(packed, n_res, precision, cur, traj_bias + t * row * MMF_UNITS, nullptr, nullptr,
                                   nxt, range_flag, N, 1, d, stream);
    if (rc) return rc;
    cur = nxt;
  }
  return 0;
}
