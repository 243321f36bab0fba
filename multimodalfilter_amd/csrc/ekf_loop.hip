// Host-side step loop of the fused extended Kalman filters: one C call enqueues, for every
// time step, the forward-mode Jacobian launch of each sub-filter's dynamics network (K5) and
// the predict / correct / fuse launch (K3).  Replaces the Python loop of torchfilter's
// Filter.forward_loop over CrossmodalKalmanFilter.forward / UnimodalKalmanFilter.forward
// (/root/reference/crossmodal/base_models/crossmodal_kf.py:88-151, unimodal_kf.py:162-250; call
// site eval_helpers.py:139-142): the EKF algebra is a few microseconds per step, so the
// recursion was bound by ~20 launches and tensor shuffles of interpreter work per step.
#include "mmf_common.h"

// Sigma_steps: (T, N, d, d) or null -- every step's posterior covariance (mmf_ekf_forward_loop_belief)
// innov: null, or the innovation record of mmf_ekf_forward_loop_innov -- K3 is then the step of mmf_ekf_step_innov and the
// loop is the loop of launches, whatever a->persistent says
static int ekf_forward_loop(const MmfEkfLoopArgs* a, float* Sigma_steps, const MmfEkfInnovArgs* innov, void* stream) {
  if (!a) return MMF_EINVAL;
  if (a->T < 0 || a->N < (innov ? 0 : 1) || a->K < 1 || a->K > MMF_LOOP_MAX_MEAS || a->d < 1) return MMF_EINVAL;
  if (innov && a->d > MMF_MAX_STATE_DIM) return MMF_EINVAL;
  if (a->fusion < 0 || a->fusion > 2) return MMF_EINVAL;
  if (!a->q_tril || !a->z || !a->r_tril || !a->mu || !a->Sigma || !a->mu_pred || !a->A || !a->estimates)
    return MMF_EINVAL;
  if (a->fusion == 1 && !a->fuse_w) return MMF_EINVAL;
  if (a->fusion != 0 && (!a->Sigma_f)) return MMF_EINVAL;
  for (int k = 0; k < a->K; ++k)
    if (!a->dyn_packed[k] || !a->dyn_bias[k]) return MMF_EINVAL;
  if (innov) {
    if (innov->nis_gate != innov->nis_gate) return MMF_EINVAL;
    const size_t rows = static_cast<size_t>(a->T) * a->K * a->N, kn = static_cast<size_t>(a->K) * a->N;
    const size_t tn = static_cast<size_t>(a->T) * a->N, v = sizeof(float) * a->d, m = v * a->d;
    const void* ins[] = {a->q_tril, a->z, a->r_tril, a->fuse_w, a->feedback_gate};
    const size_t in_bytes[] = {a->K * m, rows * v, rows * m, a->fusion == 1 ? rows * v : 0, a->T * sizeof(int32_t)};
    const void* state[] = {a->mu, a->Sigma, a->mu_pred, a->A, a->fusion ? a->Sigma_f : nullptr, a->estimates, Sigma_steps};
    const size_t state_bytes[] = {kn * v, kn * m, kn * v, kn * m, a->N * m, tn * v, tn * m};
    const void* outs[] = {innov->nis_steps, innov->loglik_steps, innov->accepted_steps};
    for (int o = 0; o < 3; ++o) {  // no record on top of an input, of the loop's state and outputs, or of another record
      const size_t nb = rows * sizeof(float);
      auto hits = [&](const void* q, size_t nq) { return mmf_bytes_overlap(outs[o], nb, q, nq); };
      for (int i = 0; i < 5; ++i)
        if (hits(ins[i], in_bytes[i])) return MMF_EINVAL;
      for (int i = 0; i < 7; ++i)
        if (hits(state[i], state_bytes[i])) return MMF_EINVAL;
      for (int q = 0; q < o; ++q)
        if (hits(outs[q], nb)) return MMF_EINVAL;
    }
    if (a->T == 0 || a->N == 0) return 0;
  }
  if (!innov && a->persistent && a->T > 0) {  // ONE launch for all T steps (ekf_persistent.inc); same bits
    const int rc = mmf_internal_ekf_persistent(a, Sigma_steps, stream);
    if (rc != MMF_INTERNAL_NOT_RESIDENT) return rc;
    // this device cannot hold the persistent grid, or the problem is not eligible: the loop of launches
  }
  const size_t N = static_cast<size_t>(a->N), d = static_cast<size_t>(a->d), K = static_cast<size_t>(a->K);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  for (int t = 0; t < a->T; ++t) {
    {  // every sub-filter's Jacobian in one launch (they are ~45 us of latency each on their own)
      const float* bias[MMF_LOOP_MAX_MEAS];
      for (size_t k = 0; k < K; ++k) bias[k] = a->dyn_bias[k] + t * N * MMF_UNITS;
      const int rc = mmf_dynamics_jacobian_multi(a->dyn_packed, a->n_res_dyn, a->precision, a->mu, bias, a->mu_pred,
                                                 a->A, a->range_flag, a->K, a->N, a->d, stream);
      if (rc) return rc;
    }
    float* est = a->estimates + t * N * d;
    const float* fuse_w = a->fuse_w ? a->fuse_w + t * K * N * d : nullptr;
    const int32_t* gate = a->feedback_gate ? a->feedback_gate + t : nullptr;
    const int rc =
        innov ? mmf_ekf_step_innov(a->A, a->mu_pred, a->q_tril, a->z + t * K * N * d, a->r_tril + t * K * N * d * d, fuse_w,
                                   a->mu, a->Sigma, a->fusion ? est : nullptr, a->fusion ? a->Sigma_f : nullptr, a->N, a->d,
                                   a->K, a->fusion, a->feedback, gate, innov->nis_gate,
                                   innov->nis_steps ? innov->nis_steps + t * K * N : nullptr,
                                   innov->loglik_steps ? innov->loglik_steps + t * K * N : nullptr,
                                   innov->accepted_steps ? innov->accepted_steps + t * K * N : nullptr, stream)
              : mmf_ekf_step_gated(a->A, a->mu_pred, a->q_tril, a->z + t * K * N * d, a->r_tril + t * K * N * d * d, fuse_w,
                                   a->mu, a->Sigma, a->fusion ? est : nullptr, a->fusion ? a->Sigma_f : nullptr, a->N, a->d,
                                   a->K, a->fusion, a->feedback, gate, stream);
    if (rc) return rc;
    if (a->fusion == 0) {  // a single (enabled) sub-filter: its corrected mean is the estimate
      const hipError_t e = hipMemcpyAsync(est, a->mu, N * d * sizeof(float), hipMemcpyDeviceToDevice, hs);
      if (e != hipSuccess) return static_cast<int>(e);
    }
    if (Sigma_steps) {  // the step's posterior covariance: the fused one, or sub-filter 0's (the first block of Sigma)
      const hipError_t e = hipMemcpyAsync(Sigma_steps + t * N * d * d, a->fusion ? a->Sigma_f : a->Sigma,
                                          N * d * d * sizeof(float), hipMemcpyDeviceToDevice, hs);
      if (e != hipSuccess) return static_cast<int>(e);
    }
  }
  return 0;
}

extern "C" int mmf_ekf_forward_loop(const MmfEkfLoopArgs* a, void* stream) {
  return ekf_forward_loop(a, nullptr, nullptr, stream);
}

extern "C" int mmf_ekf_forward_loop_belief(const MmfEkfLoopArgs* a, float* Sigma_steps, void* stream) {
  if (!Sigma_steps) return MMF_EINVAL;
  return ekf_forward_loop(a, Sigma_steps, nullptr, stream);
}

extern "C" int mmf_ekf_forward_loop_innov(const MmfEkfLoopArgs* a, const MmfEkfInnovArgs* innov, float* Sigma_steps,
                                          void* stream) {
  if (!innov) return MMF_EINVAL;
  return ekf_forward_loop(a, Sigma_steps, innov, stream);
}
