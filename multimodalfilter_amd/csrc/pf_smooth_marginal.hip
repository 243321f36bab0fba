// Marginal particle smoothing: the forward-filter backward-smoothing recursion over a filter run's history (include/mmf.h,
// "marginal particle smoothing").  Where the ancestry smoother of pf_smooth.hip follows the resampling lottery backwards,
// this one re-weights every particle of step t through the transition density N(X_{t+1}[j]; F_t[i], L L^T): O(M^2) pairs per
// trajectory and step, VALU work (the difference X - F is formed before it is whitened, so there is no K = d product an MFMA
// could take).  Four kernels behind one C call:
//   weights  one workgroup per (step, trajectory): a - max a into `weights` (the last step: exp of it)
//   logd     one launch over (column tile, trajectory, step): a thread owns a column j, the rows i stream through LDS
//   sweep    T - 1 launches over (row tile, trajectory), t = T - 2 .. 0: a thread owns a row i, the columns j stream through
//            LDS; W_{t|T}[i] replaces a_t[i] - max in `weights` (only the thread that owns row i touches it in that launch)
//   moments  one workgroup per (step, trajectory): normalises `weights` in place; mean, covariance, ESS
// Between the kernels `weights` holds UNNORMALISED values; every reader divides by the sum it takes itself, in one fixed order.
// The exponent lives in base 2: L^-1 is scaled by sqrt(log2(e) / 2), so that v_exp_f32 takes la2 - |z|^2 as it stands.

#include <cmath>

#include "pf_smooth_math.h"

namespace {

using namespace mmf::smooth_math;  // the log-weights, the transition density, the staged chunks, the pivot-form moments

struct MarginalArgs {
  const float* states;   // (T, N, M, D)
  const float* pred;     // (T - 1, N, M, D)
  const float* loglik;   // (T, N, M)
  const float* logw;     // (T, N, M) or null
  const float* tril;     // (D, D)
  float* logd;           // (T - 1, N, M), natural logarithm
  float* weights;        // (T, N, M)
  float* mean;           // (T, N, D)
  float* cov;            // (T, N, D, D) or null
  float* ess;            // (T, N) or null
  int T, N, M;
  int t0;                // logd: the step of blockIdx.z == 0; sweep: the step
};

// ---- weights: la = (loglik + logw_in) - max per (step, trajectory); -inf stays -inf.  The last step gets exp(la): the
// filter's own weights, unnormalised, which is what the sweep starts from.
__global__ __launch_bounds__(kMomentThreads) void pf_marginal_weights_kernel(MarginalArgs a) {
  __shared__ float wmax[kMomentWaves];
  const int tid = threadIdx.x, t = blockIdx.x, n = blockIdx.y, M = a.M;
  const size_t row0 = (static_cast<size_t>(t) * a.N + n) * M;
  const float* ll = a.loglik + row0;
  const float* lw = a.logw ? a.logw + row0 : nullptr;
  float* out = a.weights + row0;
  float mx = -INFINITY;
  for (int m = tid; m < M; m += kMomentThreads) mx = fmaxf(mx, log_weight(ll, lw, m));
  mx = mmf::wave_max(mx);
  if ((tid & (MMF_WAVE - 1)) == 0) wmax[tid >> 6] = mx;
  __syncthreads();
  mx = wmax[0];
  for (int w = 1; w < kMomentWaves; ++w) mx = fmaxf(mx, wmax[w]);
  const bool last = t == a.T - 1;
  for (int m = tid; m < M; m += kMomentThreads) {
    const float av = log_weight(ll, lw, m);
    const float la = av == -INFINITY ? -INFINITY : av - mx;  // (every value -inf: stays -inf, the step's results are NaN)
    out[m] = last ? exp2_hw(la * kLog2e) : la;
  }
}

// ---- logd: logD_t[j] = logsumexp_i(la_t[i] + lp_t[i, j]) for the columns of one tile
template <int D>
__global__ __launch_bounds__(kPairThreads) void pf_marginal_logd_kernel(MarginalArgs a) {
  __shared__ float4 lds[kPairChunk * Staged<D>::kFloat4s];
  const int tid = threadIdx.x, n = blockIdx.y, t = a.t0 + static_cast<int>(blockIdx.z), M = a.M;
  const size_t nm = static_cast<size_t>(a.N) * M;
  const size_t rows_t = static_cast<size_t>(t) * nm + static_cast<size_t>(n) * M;        // step t: the rows i
  const size_t cols_t = static_cast<size_t>(t + 1) * nm + static_cast<size_t>(n) * M;    // step t + 1: the columns j
  const int j = blockIdx.x * kPairThreads + tid;
  float W[D][D];
  whitener<D>(a.tril, W);
  float x[D];
  {
    const float* X = a.states + (cols_t + min(j, M - 1)) * D;
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = X[c];
  }
  float mx = -INFINITY, sum = 0.f;
  for (int c0 = 0; c0 < M; c0 += kPairChunk) {
    __syncthreads();  // the previous chunk has been consumed
#pragma unroll
    for (int k = 0; k < kPairChunk / kPairThreads; ++k) {
      const int s = k * kPairThreads + tid, i = c0 + s;
      Staged<D> row;
      row.w = i < M ? a.weights[rows_t + i] * kLog2e : -INFINITY;
      const bool dead = row.w == -INFINITY;  // its row may hold anything: it is not read
#pragma unroll
      for (int c = 0; c < D; ++c) row.x[c] = dead ? 0.f : a.pred[(rows_t + i) * D + c];
      row.store(lds, s);
    }
    __syncthreads();
    const int rows = padded_chunk(M, c0);
    for (int i0 = 0; i0 < rows; i0 += kPairGroup) {
      float v[kPairGroup];
      float top = mx;
#pragma unroll
      for (int u = 0; u < kPairGroup; ++u) {
        Staged<D> row;
        row.load(lds, i0 + u);
        v[u] = minus_sq_dist<D>(row.w, x, row.x, W);
        top = fmaxf(top, v[u]);
      }
      const float ref = rescale_ref(top);
      sum = sum * exp2_hw(mx - ref);
#pragma unroll
      for (int u = 0; u < kPairGroup; ++u) sum = sum + exp2_hw(v[u] - ref);
      mx = top;
    }
  }
  if (j < M) a.logd[rows_t + j] = (mx + log2_hw(sum)) * kLn2;
}

// ---- sweep, step t: W_{t|T}[i] = sum_j W_{t+1|T}[j] exp(la_t[i] + lp_t[i, j] - logD_t[j]) for the rows of one tile
template <int D>
__global__ __launch_bounds__(kPairThreads) void pf_marginal_sweep_kernel(MarginalArgs a) {
  __shared__ float4 lds[kPairChunk * Staged<D>::kFloat4s];
  const int tid = threadIdx.x, n = blockIdx.y, t = a.t0, M = a.M;
  const size_t nm = static_cast<size_t>(a.N) * M;
  const size_t rows_t = static_cast<size_t>(t) * nm + static_cast<size_t>(n) * M;
  const size_t cols_t = static_cast<size_t>(t + 1) * nm + static_cast<size_t>(n) * M;
  const int i = blockIdx.x * kPairThreads + tid;
  float W[D][D];
  whitener<D>(a.tril, W);
  float f[D];
  const float la = i < M ? a.weights[rows_t + i] * kLog2e : -INFINITY;
  {
    const bool dead = la == -INFINITY;
    const float* F = a.pred + (rows_t + min(i, M - 1)) * D;
#pragma unroll
    for (int c = 0; c < D; ++c) f[c] = dead ? 0.f : F[c];
  }
  float acc = 0.f, total = 0.f;
  for (int c0 = 0; c0 < M; c0 += kPairChunk) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPairChunk / kPairThreads; ++k) {
      const int s = k * kPairThreads + tid, j = c0 + s;
      Staged<D> col;
      const float w = j < M ? a.weights[cols_t + j] : 0.f;
      const bool skip = w == 0.f;  // no weight: the column is skipped, its logD may be -inf and its row anything
      col.w = skip ? -INFINITY : log2_hw(w) - a.logd[rows_t + j] * kLog2e;
#pragma unroll
      for (int c = 0; c < D; ++c) col.x[c] = skip ? 0.f : a.states[(cols_t + j) * D + c];
      col.store(lds, s);
      total = total + w;  // the same columns in the same order in every workgroup of the trajectory
    }
    __syncthreads();
    const int cols = padded_chunk(M, c0);
    for (int j0 = 0; j0 < cols; j0 += kPairGroup) {
#pragma unroll
      for (int u = 0; u < kPairGroup; ++u) {
        Staged<D> col;
        col.load(lds, j0 + u);
        acc = acc + exp2_hw(minus_sq_dist<D>(la + col.w, col.x, f, W));
      }
    }
  }
  total = mmf::wave_sum(total);
  if (i < M) a.weights[rows_t + i] = la == -INFINITY ? 0.f : acc / total;
}

// ---- moments: `weights` normalised in place; mean, covariance and ESS in the pivot form of pf_smooth.hip
template <int D>
__global__ __launch_bounds__(kMomentThreads) void pf_marginal_moments_kernel(MarginalArgs a) {
#pragma clang fp contract(off)
  constexpr int NS = moment_sums(D);
  __shared__ float partial[(kMomentSums + 2) * kMomentWaves];
  __shared__ float total[kMomentSums + 2];
  __shared__ float wtop[kMomentWaves];
  __shared__ int witop[kMomentWaves];
  const int tid = threadIdx.x, lane = tid & (MMF_WAVE - 1), wave = tid >> 6;
  const int t = blockIdx.x, n = blockIdx.y, M = a.M;
  const size_t row0 = (static_cast<size_t>(t) * a.N + n) * M;
  float* w = a.weights + row0;
  const float* X = a.states + row0 * D;
  bool bad = false;
#pragma unroll
  for (int r = 0; r < D; ++r) {
    const float g = a.tril[r * D + r];
    bad = bad || !(g > 0.f) || !(g < INFINITY);
  }
  // the pivot: the first largest weight
  float bv = -INFINITY, s1 = 0.f, s2 = 0.f;
  int bi = 0x7fffffff;
  for (int m = tid; m < M; m += kMomentThreads) {
    const float e = w[m];
    if (e > bv) { bv = e; bi = m; }
    s1 = s1 + e;
    s2 = s2 + e * e;
  }
  s1 = mmf::wave_sum(s1);
  s2 = mmf::wave_sum(s2);
  if (lane == 0) {
    partial[NS * kMomentWaves + wave] = s1;
    partial[(NS + 1) * kMomentWaves + wave] = s2;
  }
  first_max(bv, bi, wtop, witop, tid, kMomentWaves, M);  // (its barrier orders the partials too)
  float S = 0.f, S2 = 0.f;
  for (int k = 0; k < kMomentWaves; ++k) { S = S + partial[NS * kMomentWaves + k]; S2 = S2 + partial[(NS + 1) * kMomentWaves + k]; }
  if (bad) S = NAN;
  float p[D], acc[NS];
#pragma unroll
  for (int c = 0; c < D; ++c) p[c] = X[static_cast<size_t>(bi) * D + c];
#pragma unroll
  for (int v = 0; v < NS; ++v) acc[v] = 0.f;
  for (int m = tid; m < M; m += kMomentThreads) {
    const float e = w[m];
    // a particle of zero weight contributes exactly zero, whatever its row holds
    if (e != 0.f) pivot_accumulate<D>(acc, e, X + static_cast<size_t>(m) * D, p);
    w[m] = e / S;
  }
  block_sums(acc, partial, total, kMomentWaves, kMomentWaves, tid);
  __syncthreads();
  const size_t out = static_cast<size_t>(t) * a.N + n;
  write_moments<D>(a.mean, a.cov, out, tid, p, total, S);
  if (a.ess && tid == 0) a.ess[out] = (S * S) / S2;
}

}  // namespace

extern "C" int mmf_pf_smooth_marginal(const MmfPfSmoothMarginalArgs* a, void* stream) {
  if (!a || !a->states_steps || !a->loglik_steps || !a->scale_tril || !a->weights || !a->mean) return MMF_EINVAL;
  if (a->T < 0 || a->N < 0 || a->M < 1 || a->d < 1) return MMF_EINVAL;
  if (a->T >= 2 && (!a->pred_steps || !a->logd)) return MMF_EINVAL;
  if (!sizes_in_range(a->M, a->N, a->d)) return MMF_ETOOLARGE;
  if (a->N == 0 || a->T == 0) return 0;
  MarginalArgs k{};
  k.states = a->states_steps; k.pred = a->pred_steps; k.loglik = a->loglik_steps; k.logw = a->logw_in_steps;
  k.tril = a->scale_tril; k.logd = a->logd; k.weights = a->weights; k.mean = a->mean; k.cov = a->cov; k.ess = a->ess;
  k.T = a->T; k.N = a->N; k.M = a->M;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int T = a->T, N = a->N;
  const int tiles = (a->M + kPairThreads - 1) / kPairThreads;
  return mmf::with_state_dim(a->d, [&](auto D) -> int {
    constexpr int d = decltype(D)::value;
    if (const int rc = mmf::launch(pf_marginal_weights_kernel, dim3(T, N), kMomentThreads, 0, s, k)) return rc;
    if (const int rc = launch_steps(pf_marginal_logd_kernel<d>, tiles, N, T - 1, s, k)) return rc;
    for (int t = T - 2; t >= 0; --t) {
      k.t0 = t;
      if (const int rc = mmf::launch(pf_marginal_sweep_kernel<d>, dim3(tiles, N), kPairThreads, 0, s, k)) return rc;
    }
    return mmf::launch(pf_marginal_moments_kernel<d>, dim3(T, N), kMomentThreads, 0, s, k);
  });
}
