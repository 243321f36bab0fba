// The mixture log score of a weighted particle set against a true state, with its closed-form gradients (include/mmf.h,
// "Training on the particle set"): per row, with z_mj = (y_j - x_mj) / sigma_j and e_m = a_m - 1/2 sum_j z_mj^2,
//   nll = logsumexp a - logsumexp e + sum_j log sigma_j + d/2 log 2 pi,    r = softmax(e), p = softmax(a)
//   d nll / d x_mj = -r_m z_mj / sigma_j,   d nll / d a_m = p_m - r_m,   d nll / d log sigma_j = 1 - sum_m r_m z_mj^2
//   plan      a row is a wave's (kRowsPerBlock rows to a workgroup of 256 threads) up to kWaveM particles and a workgroup's of
//             kBlockThreads threads beyond: the reference trains on hundreds of rows of 30 particles, where a workgroup per row
//             would leave 7 of 8 waves idle, evaluation-sized sets have thousands.  A function of M alone, and both forms run the
//             same row body, so a row has the same bits wherever it stands in whatever batch
//   passes    (1) max a and max e over the live particles  (2) sum exp(a - max a), sum exp(e - max e), sum exp(e - max e) z_j^2
//             (3) the per-particle gradients.  Every pass re-reads the row from global memory (L1 / L2 hits after the first):
//             nothing is staged per particle, so M is not bounded by LDS.  A forward call (nll alone) stops after (2)
//   reduce    a thread's terms in ascending m (stride = the group's threads), the DPP butterfly of mmf_common.h over a wave,
//             the waves ascending through one LDS word each.  No atomics; the two log-sum-exps are combined in double
//   dead      a_m = -inf (or NaN) is selected away before its state row is read, and its gradients are written as 0; a row
//             without a live particle, with a NaN in y or with no finite e gives nll = NaN and zero gradients
#include <cmath>

#include "mmf_common.h"

namespace {

constexpr int kWaveM = 256;          // a wave owns a row up to here (4 particles of a lane a pass); tests/_set_loss_cases.WAVE_M
constexpr int kRowsPerBlock = 4;     // waves = rows of a workgroup of the wave form
constexpr int kBlockThreads = 512;   // threads of a row's workgroup beyond kWaveM
constexpr int kBlockWaves = kBlockThreads / MMF_WAVE;
constexpr int kSlots = 4 + MMF_MAX_STATE_DIM;  // group reductions of a row: max a, max e, sum a, sum e, d z-moments

struct KArgs {
  const float* states;   // (R, M, d)
  const float* logw;     // (R, M)
  const float* truth;    // (R, d)
  const float* scale;    // (d)
  const float* g_nll;    // (R) or null = 1
  float* nll;            // (R) or null
  float* g_states;       // (R, M, d) or null
  float* g_logw;         // (R, M) or null
  float* g_log_scale;    // (R, d) or null
  int R, M;
};

// the value of every thread of the group reduced, in every thread.  WAVES == 1: the wave alone, no LDS and no barrier (the
// other waves of the workgroup own other rows and may have left)
template <int WAVES, bool MAX>
__device__ __forceinline__ float group_reduce(float v, float* slot, int tid) {
  v = MAX ? mmf::wave_max(v) : mmf::wave_sum(v);
  if (WAVES == 1) return v;
  if ((tid & (MMF_WAVE - 1)) == 0) slot[tid / MMF_WAVE] = v;
  __syncthreads();
  v = slot[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) v = MAX ? fmaxf(v, slot[w]) : __fadd_rn(v, slot[w]);
  return v;
}

// z_j of particle x, and 1/2 |z|^2
template <int D>
__device__ __forceinline__ float half_sq(const float* __restrict__ x, const float (&y)[D], const float (&inv)[D], float (&z)[D]) {
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    z[j] = (y[j] - x[j]) * inv[j];
    q = fmaf(z[j], z[j], q);
  }
  return 0.5f * q;
}

// one row by a group of WAVES waves; tid counts inside the group, red: kSlots x WAVES floats of LDS (unused for one wave)
template <int D, int WAVES>
__device__ __forceinline__ void row_body(const KArgs& a, int r, int tid, float (*red)[WAVES]) {
  auto slot = [&](int k) { return WAVES > 1 ? red[k] : nullptr; };  // (one wave: no LDS behind it)
  constexpr int kThreads = WAVES * MMF_WAVE;
  const int M = a.M;
  const size_t row = static_cast<size_t>(r) * M;
  const float* __restrict__ X = a.states + row * D;
  const float* __restrict__ A = a.logw + row;
  float y[D], inv[D];
  bool y_ok = true;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    y[j] = a.truth[static_cast<size_t>(r) * D + j];
    inv[j] = 1.0f / a.scale[j];
    y_ok = y_ok && !(y[j] != y[j]);
  }

  // ---- (1) the two maxima, over the live particles (fmaxf skips a NaN)
  float amax = -INFINITY, emax = -INFINITY;
  for (int m = tid; m < M; m += kThreads) {
    const float am = A[m];
    if (!(am > -INFINITY)) continue;  // dead (or NaN): its row is not read
    float z[D];
    const float q = half_sq<D>(X + static_cast<size_t>(m) * D, y, inv, z);
    amax = fmaxf(amax, am);
    emax = fmaxf(emax, am - q);
  }
  amax = group_reduce<WAVES, true>(amax, slot(0), tid);
  emax = group_reduce<WAVES, true>(emax, slot(1), tid);
  const bool ok = y_ok && amax > -INFINITY && amax < INFINITY && emax > -INFINITY;

  // ---- (2) the sums about them
  float sa = 0.f, se = 0.f, sz[D];
#pragma unroll
  for (int j = 0; j < D; ++j) sz[j] = 0.f;
  if (ok) {
    for (int m = tid; m < M; m += kThreads) {
      const float am = A[m];
      if (!(am > -INFINITY)) continue;
      float z[D];
      const float q = half_sq<D>(X + static_cast<size_t>(m) * D, y, inv, z);
      sa += expf(am - amax);
      const float we = expf((am - q) - emax);
      se += we;
#pragma unroll
      for (int j = 0; j < D; ++j) sz[j] = fmaf(we, z[j] * z[j], sz[j]);
    }
  }
  sa = group_reduce<WAVES, false>(sa, slot(2), tid);
  se = group_reduce<WAVES, false>(se, slot(3), tid);
#pragma unroll
  for (int j = 0; j < D; ++j) sz[j] = group_reduce<WAVES, false>(sz[j], slot(4 + j), tid);

  const float g = a.g_nll ? a.g_nll[r] : 1.0f;
  if (tid == 0) {
    if (a.nll) {
      double v = NAN;
      if (ok) {
        v = (static_cast<double>(amax) + log(static_cast<double>(sa))) - (static_cast<double>(emax) + log(static_cast<double>(se)));
#pragma unroll
        for (int j = 0; j < D; ++j) v += log(static_cast<double>(a.scale[j]));
        v += 0.5 * D * 1.8378770664093453;  // log 2 pi
      }
      a.nll[r] = static_cast<float>(v);
    }
    if (a.g_log_scale) {
#pragma unroll
      for (int j = 0; j < D; ++j) a.g_log_scale[static_cast<size_t>(r) * D + j] = ok ? (1.0f - sz[j] / se) * g : 0.f;
    }
  }

  // ---- (3) the per-particle gradients; the upstream gradient multiplies last, so a power of two scales them exactly
  if (!a.g_states && !a.g_logw) return;
  const float inv_sa = ok ? 1.0f / sa : 0.f, inv_se = ok ? 1.0f / se : 0.f;
  float* __restrict__ GX = a.g_states ? a.g_states + row * D : nullptr;
  float* __restrict__ GA = a.g_logw ? a.g_logw + row : nullptr;
  for (int m = tid; m < M; m += kThreads) {
    const float am = A[m];
    float gx[D], ga = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) gx[j] = 0.f;
    if (ok && am > -INFINITY) {
      float z[D];
      const float q = half_sq<D>(X + static_cast<size_t>(m) * D, y, inv, z);
      const float p = expf(am - amax) * inv_sa, rm = expf((am - q) - emax) * inv_se;
      ga = (p - rm) * g;
#pragma unroll
      for (int j = 0; j < D; ++j) gx[j] = -(rm * z[j] * inv[j]) * g;
    }
    if (GA) GA[m] = ga;
    if (GX) {
#pragma unroll
      for (int j = 0; j < D; ++j) GX[static_cast<size_t>(m) * D + j] = gx[j];
    }
  }
}

template <int D>
__global__ __launch_bounds__(kRowsPerBlock * MMF_WAVE) void pf_set_nll_wave_kernel(KArgs a) {
  const int r = blockIdx.x * kRowsPerBlock + threadIdx.x / MMF_WAVE;
  if (r >= a.R) return;  // (the whole wave)
  row_body<D, 1>(a, r, threadIdx.x & (MMF_WAVE - 1), nullptr);
}

template <int D>
__global__ __launch_bounds__(kBlockThreads) void pf_set_nll_block_kernel(KArgs a) {
  __shared__ float red[kSlots][kBlockWaves];
  row_body<D, kBlockWaves>(a, blockIdx.x, threadIdx.x, red);
}

template <int D>
int run(const KArgs& k, hipStream_t s) {
  if (k.M <= kWaveM) {
    pf_set_nll_wave_kernel<D><<<(k.R + kRowsPerBlock - 1) / kRowsPerBlock, kRowsPerBlock * MMF_WAVE, 0, s>>>(k);
  } else {
    pf_set_nll_block_kernel<D><<<k.R, kBlockThreads, 0, s>>>(k);
  }
  MMF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int mmf_pf_set_nll(const MmfPfSetNllArgs* a, void* stream) {
  if (!a || !a->states || !a->logw || !a->truth || !a->scale) return MMF_EINVAL;
  if (a->R < 0 || a->M < 1 || a->d < 1 || a->d > MMF_MAX_STATE_DIM) return MMF_EINVAL;
  if (!a->nll && !a->g_states && !a->g_logw && !a->g_log_scale) return MMF_EINVAL;
  {
    const size_t R = a->R, M = a->M, d = a->d, f = sizeof(float);
    const void* outs[4] = {a->nll, a->g_states, a->g_logw, a->g_log_scale};
    const size_t out_bytes[4] = {R * f, R * M * d * f, R * M * f, R * d * f};
    const void* ins[5] = {a->states, a->logw, a->truth, a->scale, a->g_nll};
    const size_t in_bytes[5] = {R * M * d * f, R * M * f, R * d * f, d * f, R * f};
    if (mmf_outputs_overlap(outs, out_bytes, 4, ins, in_bytes, 5)) return MMF_EINVAL;
  }
  if (a->R == 0) return 0;
  KArgs k{};
  k.states = a->states; k.logw = a->logw; k.truth = a->truth; k.scale = a->scale; k.g_nll = a->g_nll;
  k.nll = a->nll; k.g_states = a->g_states; k.g_logw = a->g_logw; k.g_log_scale = a->g_log_scale;
  k.R = a->R; k.M = a->M;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (a->d) {
    case 1: return run<1>(k, s);
    case 2: return run<2>(k, s);
    case 3: return run<3>(k, s);
    default: return run<4>(k, s);
  }
}
