// Per-modality attribution of the crossmodal particle filter's fusion (include/mmf.h, "Per-modality attribution"): for every
// weighted set the K unimodal posteriors W^k on the shared particles beside the fused one W, as evidences, responsibilities,
// effective sample sizes, means, KL(W^k || W) and the Bhattacharyya overlaps between modalities.  The live-weight and
// dead-particle rules of pf_summary.h, every sum in a fixed order; normalised once, at the end, in double.
//   plan      one workgroup per row, a thread to every kBatch particles, rounded up to a wave, kThreads at most: a function of M
//             alone.  No workspace, no finishing launch
//   pass 1    the K + 2 row maxima (of u_k = a + l_k, of v = a + L and of a) over the log columns: 4 (1 + K) bytes per particle
//   pass 2    the log columns again (out of L2: a row's columns are at most 320 KiB and the same workgroup has just read
//             them) and the state rows: the (K + 1) live weights of a particle, then (K + 1)(2 + d) + K + K (K - 1) / 2 + 1
//             sums -- sum w, sum w^2 and sum w x per distribution, sum w^k (t^k - t) per modality, sum sqrt(w^j w^k) per pair,
//             sum exp(a - max a).  Both passes load kBatch particles of a thread before they use one (the loads of a batch are
//             in flight together); a thread's sums are fp32 over a batch, flushed to double
//   reduce    the 64 lanes' totals of a wave as one more fp32 run (mmf::wave_sum, DPP: an order of its own, fixed), the
//             waves ascending in double, total s by thread s
//   finish    from the totals in LDS, in double: thread q the evidence, ESS and mean of distribution q, thread K + 1 + k the
//             responsibility and divergence of modality k, thread 2 K + 1 + j row j of the overlaps

#include <cmath>

#include "pf_summary.h"

namespace {

using namespace mmf::summary;  // the weights and the host's checks

constexpr int kMaxK = MMF_LOOP_MAX_MEAS;
constexpr int kThreads = 512;  // threads of a workgroup at most
constexpr int kBatch = 4;      // particles of a thread that are loaded together, and that an fp32 sum takes before it is flushed
static_assert(kMaxK == 4, "one kernel per number of modalities");

struct MArgs {
  const float* states;         // (R, M, d)
  const float* log_w;          // (R, M) or null
  const float* loglik[kMaxK];  // (R, M) each
  const float* beta;           // (R, beta_stride) or null
  float* log_evidence;         // (R, K + 1) or null
  float* responsibility;       // (R, K) or null
  float* ess;                  // (R, K + 1) or null
  float* mean;                 // (R, K + 1, d) or null
  float* divergence;           // (R, K) or null
  float* overlap;              // (R, K, K) or null
  int M, beta_stride;
};

// where the sums stand: distribution q (q == K: the fused one) at q (2 + D): sum w, sum w^2, sum w x_0 .. x_{D-1}
template <int K, int D>
struct Sums {
  static constexpr int kDist = 2 + D;
  static constexpr int kDiv = (K + 1) * kDist;         // K of them
  static constexpr int kPair = kDiv + K;               // K (K - 1) / 2 of them, (j, k > j) in row order
  static constexpr int kPrior = kPair + K * (K - 1) / 2;
  static constexpr int kCount = kPrior + 1;
  __host__ __device__ static constexpr int pair(int j, int k) { return kPair + j * (2 * K - j - 1) / 2 + (k - j - 1); }
};

// L = logsumexp_k (beta_k + l_k) over the terms that carry weight (a NaN or -inf term carries none; no term at all: -inf)
template <int K>
__device__ __forceinline__ float fuse(const float* l, const float* beta) {
  float s[K], top = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    s[k] = beta[k] + l[k];
    top = fmaxf(top, s[k]);  // (a NaN is skipped)
  }
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) sum += live_weight(s[k] - top);
  return top + logf(sum);
}

// a batch of a thread's particles, m0 + i threads: the log columns (a particle beyond the row: a = -inf, which carries no
// weight anywhere) and, with X, the state rows
template <int K, int D, bool X>
__device__ __forceinline__ void load_batch(const MArgs& a, size_t row, int m0, int threads, float* am, float (*l)[K], float (*x)[D]) {
#pragma unroll
  for (int i = 0; i < kBatch; ++i) {
    const int m = m0 + i * threads;
    const bool in = m < a.M;
    am[i] = in ? (a.log_w ? a.log_w[row + m] : 0.f) : -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) l[i][k] = in ? a.loglik[k][row + m] : 0.f;
    if constexpr (X)
#pragma unroll
      for (int c = 0; c < D; ++c) x[i][c] = in ? a.states[(row + m) * D + c] : 0.f;
  }
}

template <int K, int D>
__global__ __launch_bounds__(kThreads) void pf_modalities_kernel(MArgs a) {
  using S = Sums<K, D>;
  constexpr int Q = K + 1, NS = S::kCount, kWaves = kThreads / MMF_WAVE;
  __shared__ double wave_part[kWaves][NS];  // (row 0 is reused for the totals)
  __shared__ float wave_top[kWaves][Q + 1];
  __shared__ float row_top[Q + 1];  // the maxima again, for the finish to index by a run-time q
  const int tid = threadIdx.x, threads = blockDim.x, waves = threads / MMF_WAVE, M = a.M;
  const int r = blockIdx.x;
  const size_t row = static_cast<size_t>(r) * M;
  float beta[K];
#pragma unroll
  for (int k = 0; k < K; ++k) beta[k] = a.beta ? a.beta[static_cast<size_t>(r) * a.beta_stride + k] : 0.f;

  // ---- pass 1: the row maxima of u_k (top[k]), of v (top[K]) and of a (top[Q])
  float top[Q + 1];
#pragma unroll
  for (int q = 0; q <= Q; ++q) top[q] = -INFINITY;
  for (int m0 = tid; m0 < M; m0 += threads * kBatch) {
    float am[kBatch], l[kBatch][K];
    load_batch<K, D, false>(a, row, m0, threads, am, l, nullptr);
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      if (m0 + i * threads >= M) continue;
#pragma unroll
      for (int k = 0; k < K; ++k) top[k] = fmaxf(top[k], am[i] + l[i][k]);  // (a NaN is skipped)
      top[K] = fmaxf(top[K], am[i] + fuse<K>(l[i], beta));
      top[Q] = fmaxf(top[Q], am[i]);
    }
  }
#pragma unroll
  for (int q = 0; q <= Q; ++q) {
    const float v = mmf::wave_max(top[q]);
    if ((tid & (MMF_WAVE - 1)) == 0) wave_top[tid / MMF_WAVE][q] = v;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q <= Q; ++q) {
    float v = wave_top[0][q];
    for (int w = 1; w < waves; ++w) v = fmaxf(v, wave_top[w][q]);
    top[q] = v;
  }

  // ---- pass 2: the sums.  A dead particle (a = -inf or NaN) has t = -inf or NaN under every distribution, so no weight, and
  // its state row, though loaded, is selected away from every sum
  double v[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) v[s] = 0.0;
  for (int m0 = tid; m0 < M; m0 += threads * kBatch) {
    float am[kBatch], l[kBatch][K], x[kBatch][D];
    load_batch<K, D, true>(a, row, m0, threads, am, l, x);
    float acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = 0.f;
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      if (m0 + i * threads >= M) continue;  // (a wave whose slots are all beyond the row skips the arithmetic)
      acc[S::kPrior] += live_weight(am[i] - top[Q]);
      float t[Q], w[Q];
#pragma unroll
      for (int k = 0; k < K; ++k) t[k] = (am[i] + l[i][k]) - top[k];
      t[K] = (am[i] + fuse<K>(l[i], beta)) - top[K];
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        w[q] = live_weight(t[q]);
        const bool on = w[q] > 0.f;  // (selected away, not multiplied by 0)
        float* sum = acc + q * S::kDist;
        sum[0] += w[q];
        sum[1] = fmaf(w[q], w[q], sum[1]);
#pragma unroll
        for (int c = 0; c < D; ++c) sum[2 + c] = on ? fmaf(w[q], x[i][c], sum[2 + c]) : sum[2 + c];
      }
#pragma unroll
      for (int k = 0; k < K; ++k) acc[S::kDiv + k] = w[k] > 0.f ? fmaf(w[k], t[k] - t[K], acc[S::kDiv + k]) : acc[S::kDiv + k];
#pragma unroll
      for (int j = 0; j < K; ++j)
#pragma unroll
        for (int k = j + 1; k < K; ++k) acc[S::pair(j, k)] += __builtin_amdgcn_sqrtf(w[j] * w[k]);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) v[s] += static_cast<double>(acc[s]);
  }

  // ---- over the workgroup: the lanes of a wave in fp32, the waves in double; total s by thread s, left in wave_part[0]
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const float lanes = mmf::wave_sum(static_cast<float>(v[s]));
    if ((tid & (MMF_WAVE - 1)) == 0) wave_part[tid / MMF_WAVE][s] = static_cast<double>(lanes);
  }
  __syncthreads();
  if (tid < NS) {
    const double s = sum_of_waves(wave_part, tid, waves);
    wave_part[0][tid] = s;  // (thread s alone reads and writes column s)
  }
  if (tid == 0)
#pragma unroll
    for (int q = 0; q <= Q; ++q) row_top[q] = top[q];
  __syncthreads();
  if (tid >= Q + 2 * K) return;

  // ---- the row's outputs, in double: a few of them per thread
  const double* tot = wave_part[0];
  const bool dead = !(tot[S::kPrior] > 0.0);  // no live particle in the row
  // (the logarithm of a total in fp32: an absolute 1e-7 in a log-evidence that is written as a float)
  const auto log_of = [](double s) { return static_cast<double>(logf(static_cast<float>(s))); };
  const double A = static_cast<double>(top[Q]) + log_of(tot[S::kPrior]);
  const auto weight = [&](int q) { return tot[q * S::kDist]; };
  const auto evidence = [&](int q) {
    const double sw = weight(q);
    return dead ? static_cast<double>(NAN) : sw > 0.0 ? static_cast<double>(row_top[q]) + log_of(sw) - A : -static_cast<double>(INFINITY);
  };
  const size_t R = static_cast<size_t>(r);
  if (tid < Q) {
    const int q = tid;
    const double sw = weight(q);
    const bool has = sw > 0.0;
    if (a.log_evidence) a.log_evidence[R * Q + q] = static_cast<float>(evidence(q));
    if (a.ess) a.ess[R * Q + q] = has ? static_cast<float>(sw * sw / tot[q * S::kDist + 1]) : NAN;
    if (a.mean)
#pragma unroll
      for (int c = 0; c < D; ++c) a.mean[(R * Q + q) * D + c] = has ? static_cast<float>(tot[q * S::kDist + 2 + c] / sw) : NAN;
  } else if (tid < Q + K) {
    const int k = tid - Q;
    const double sw = weight(k), sf = weight(K);
    const bool has = sw > 0.0;
    if (a.responsibility) {
      const double b = a.beta ? static_cast<double>(a.beta[R * a.beta_stride + k]) : 0.0;
      // (beta_k = -inf: no share, whatever the fused evidence is -- -inf itself where no other modality carries weight)
      a.responsibility[R * K + k] = dead ? NAN : has && b > -INFINITY ? expf(static_cast<float>(b + evidence(k) - evidence(K))) : 0.f;
    }
    if (a.divergence) a.divergence[R * K + k] = has && sf > 0.0 ? static_cast<float>(tot[S::kDiv + k] / sw - log_of(sw) + log_of(sf)) : NAN;
  } else if (a.overlap) {
    const int j = tid - Q - K;
    const double sj = weight(j);
    for (int k = 0; k < K; ++k) {
      const double sk = weight(k);
      const int lo = j < k ? j : k, hi = j < k ? k : j;
      const bool has = sj > 0.0 && sk > 0.0;
      // (j, k) and (k, j) are formed by two threads from the same doubles in the same operations: the same bits
      a.overlap[(R * K + j) * K + k] = !has ? NAN : j == k ? 1.f : static_cast<float>(tot[S::pair(lo, hi)] / sqrt(sj * sk));
    }
  }
}

// the threads of a row's workgroup: one to a batch of kBatch particles, rounded up to a wave, kThreads at most -- up to 2048
// particles a thread loads its share at once; a small set keeps few waves, whose reductions and barriers are what it costs.
// A function of M alone, so a row has the same bits whatever the batch
inline int threads_of(int M) {
  const int lanes = (M + kBatch - 1) / kBatch;
  return lanes >= kThreads ? kThreads : (lanes + MMF_WAVE - 1) / MMF_WAVE * MMF_WAVE;
}

template <int K, int D>
int run(const MArgs& k, unsigned grid, int threads, hipStream_t s) {
  pf_modalities_kernel<K, D><<<grid, threads, 0, s>>>(k);
  MMF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int mmf_pf_modalities(const MmfPfModalitiesArgs* a, void* stream) {
  if (!a || check_rows(a->states, a->R, a->M, a->d)) return MMF_EINVAL;
  if (a->K < 1 || a->K > kMaxK) return MMF_EINVAL;
  for (int k = 0; k < a->K; ++k)
    if (!a->loglik[k]) return MMF_EINVAL;
  if (a->modality_logw && a->logw_stride < a->K) return MMF_EINVAL;
  if (!a->log_evidence && !a->responsibility && !a->ess && !a->mean && !a->divergence && !a->overlap) return MMF_EINVAL;
  if (const int rc = check_size(a->R, a->M, 1)) return rc;
  {
    const size_t R = a->R, M = a->M, d = a->d, K = a->K, f = sizeof(float);
    const void* outs[6] = {a->log_evidence, a->responsibility, a->ess, a->mean, a->divergence, a->overlap};
    const size_t out_bytes[6] = {R * (K + 1) * f, R * K * f, R * (K + 1) * f, R * (K + 1) * d * f, R * K * f, R * K * K * f};
    const void* ins[3 + kMaxK] = {a->states, a->log_w, a->modality_logw};
    size_t in_bytes[3 + kMaxK] = {R * M * d * f, R * M * f, R > 0 ? ((R - 1) * static_cast<size_t>(a->logw_stride) + K) * f : 0};
    for (size_t k = 0; k < K; ++k) {
      ins[3 + k] = a->loglik[k];
      in_bytes[3 + k] = R * M * f;
    }
    if (mmf_outputs_overlap(outs, out_bytes, 6, ins, in_bytes, 3 + static_cast<int>(K))) return MMF_EINVAL;
  }
  if (a->R == 0) return 0;
  MArgs k{};
  k.states = a->states; k.log_w = a->log_w; k.beta = a->modality_logw; k.beta_stride = a->logw_stride;
  for (int i = 0; i < a->K; ++i) k.loglik[i] = a->loglik[i];
  k.log_evidence = a->log_evidence; k.responsibility = a->responsibility; k.ess = a->ess;
  k.mean = a->mean; k.divergence = a->divergence; k.overlap = a->overlap;
  k.M = a->M;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(a->R);
  const int threads = threads_of(a->M);
  return mmf::with_state_dim(a->d, [&](auto D) {
    constexpr int kD = decltype(D)::value;
    switch (a->K) {
      case 1: return run<1, kD>(k, grid, threads, s);
      case 2: return run<2, kD>(k, grid, threads, s);
      case 3: return run<3, kD>(k, grid, threads, s);
      default: return run<4, kD>(k, grid, threads, s);
    }
  });
}
