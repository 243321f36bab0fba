// Two-slice smoothing moments: the expected transition residual e = X_{t+1}[j] - F_t[i] and its raw second moment under
// xi_t[i, j] ~ W_t[i] exp(lp_t[i, j] - logD_t[j]) W_{t+1|T}[j] (include/mmf.h, "two-slice smoothing moments") -- the E-step
// of an EM refit of the process noise.  It reads what mmf_pf_smooth_marginal left (W_{t|T} and logD) and makes the marginal
// sweep's O(M^2) pass once more, over ALL steps at once (they are independent), keeping 1 + d + d (d + 1) / 2 weighted sums
// per thread where the sweep keeps one.  Two kernels behind one C call:
//   pairs   one launch over (row tile, trajectory, step): a thread owns a row i, the columns j stream through LDS in the
//           marginal kernels' chunks and layout; the wave's sums go to the workspace, one set per tile
//   reduce  one workgroup per (step, trajectory): the tiles' sets added in tile order, divided by the total
// log W_t relative to the step's maximum: every pairs workgroup takes that maximum itself from the M log-weights.
// VALU work, like the marginal kernels: expanding e e^T into x x^T - x f^T - f x^T + f f^T would turn the inner sum into
// a GEMM an MFMA could take, but with states O(1), clouds up to 0.3 wide and noise 0.005 .. 0.05 wide the second moment
// (1e-5 .. 1e-3 of the products) would lose three to five digits in the cancellation: the difference is formed first.

#include <cmath>

#include "pf_smooth_math.h"

namespace {

using namespace mmf::smooth_math;  // the log-weights, the transition density, the staged chunks, moment_sums / tri_index

constexpr int sums_of(int d) { return 1 + moment_sums(d); }  // the total, p e, the upper triangle of p e e^T

struct PairArgs {
  const float* states;   // (T, N, M, D)
  const float* pred;     // (T - 1, N, M, D)
  const float* loglik;   // (T, N, M)
  const float* logw;     // (T, N, M) or null
  const float* tril;     // (D, D)
  const float* weights;  // (T, N, M)      W_{t|T}
  const float* logd;     // (T - 1, N, M), natural logarithm
  float* partial;        // (T - 1, N, tiles, sums_of(D))
  float* mean;           // (T - 1, N, D)
  float* second;         // (T - 1, N, D, D)
  int T, N, M, tiles;
  int t0;                // pairs: the step of blockIdx.z == 0
};

// ---- pairs: the unnormalised sums over the rows of one tile and all columns
template <int D>
__global__ __launch_bounds__(kPairThreads) void pf_pair_sums_kernel(PairArgs a) {
  constexpr int NS = sums_of(D);
  __shared__ float4 lds[kPairChunk * Staged<D>::kFloat4s];
  const int tid = threadIdx.x, n = blockIdx.y, t = a.t0 + static_cast<int>(blockIdx.z), M = a.M;
  const size_t nm = static_cast<size_t>(a.N) * M;
  const size_t rows_t = static_cast<size_t>(t) * nm + static_cast<size_t>(n) * M;        // step t: the rows i
  const size_t cols_t = static_cast<size_t>(t + 1) * nm + static_cast<size_t>(n) * M;    // step t + 1: the columns j
  const int i = blockIdx.x * kPairThreads + tid;
  float W[D][D];
  whitener<D>(a.tril, W);
  // log W_t relative to the step's maximum (the basis logD was computed in): the workgroup takes the maximum itself
  const float* ll = a.loglik + rows_t;
  const float* lw = a.logw ? a.logw + rows_t : nullptr;
  float mx = -INFINITY;
  for (int m = tid; m < M; m += kPairThreads) mx = fmaxf(mx, log_weight(ll, lw, m));
  mx = mmf::wave_max(mx);
  const float la = i < M ? log2_weight(log_weight(ll, lw, i), mx) : -INFINITY;
  float f[D];
  {
    const bool dead = la == -INFINITY;  // no weight: the row is skipped, its prediction may hold anything
    const float* F = a.pred + (rows_t + min(i, M - 1)) * D;
#pragma unroll
    for (int c = 0; c < D; ++c) f[c] = dead ? 0.f : F[c];
  }
  float acc[NS];
#pragma unroll
  for (int v = 0; v < NS; ++v) acc[v] = 0.f;
  for (int c0 = 0; c0 < M; c0 += kPairChunk) {
    __syncthreads();  // the previous chunk has been consumed
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
    }
    __syncthreads();
    const int cols = padded_chunk(M, c0);
    for (int j0 = 0; j0 < cols; j0 += kPairGroup) {
#pragma unroll
      for (int u = 0; u < kPairGroup; ++u) {
        Staged<D> col;
        col.load(lds, j0 + u);
        float e[D];
        const float p = exp2_hw(minus_sq_dist_dx<D>(la + col.w, col.x, f, W, e));
        acc[0] = acc[0] + p;
        int v = 1 + D;
#pragma unroll
        for (int r = 0; r < D; ++r) {
          const float pe = p * e[r];
          acc[1 + r] = acc[1 + r] + pe;
#pragma unroll
          for (int c = r; c < D; ++c, ++v) acc[v] = fmaf(pe, e[c], acc[v]);
        }
      }
    }
  }
  float* out = a.partial + ((static_cast<size_t>(t) * a.N + n) * a.tiles + blockIdx.x) * NS;
#pragma unroll
  for (int v = 0; v < NS; ++v) {
    const float r = mmf::wave_sum(acc[v]);
    if (tid == 0) out[v] = r;
  }
}

// ---- reduce: the tiles' partials in tile order, divided by the total
template <int D>
__global__ __launch_bounds__(kPairThreads) void pf_pair_reduce_kernel(PairArgs a) {
  constexpr int NS = sums_of(D);
  static_assert(NS <= kPairThreads && D * D <= kPairThreads, "one thread per sum, one per output entry");
  __shared__ float total[NS];
  const int tid = threadIdx.x, t = blockIdx.x, n = blockIdx.y;
  const size_t out = static_cast<size_t>(t) * a.N + n;
  if (tid < NS) {
    const float* in = a.partial + out * a.tiles * NS + tid;
    float r = 0.f;
    for (int k = 0; k < a.tiles; ++k) r = r + in[static_cast<size_t>(k) * NS];
    total[tid] = r;
  }
  __syncthreads();
  const float S = total[0];
  if (tid < D) a.mean[out * D + tid] = total[1 + tid] / S;
  if (tid < D * D) {
    const int r = tid / D, c = tid % D, i = min(r, c), j = max(r, c);
    a.second[out * D * D + tid] = total[1 + tri_index<D>(i, j)] / S;
  }
}

}  // namespace

extern "C" size_t mmf_pf_smooth_pair_workspace_floats(int T, int N, int M, int d) {
  if (T < 2 || N < 1 || M < 1 || d < 1 || !sizes_in_range(M, N, d)) return 0;
  const size_t tiles = (static_cast<size_t>(M) + kPairThreads - 1) / kPairThreads;
  return static_cast<size_t>(T - 1) * N * tiles * sums_of(d);
}

extern "C" int mmf_pf_smooth_pair_moments(const MmfPfSmoothPairArgs* a, void* stream) {
  if (!a || !a->states_steps || !a->loglik_steps || !a->scale_tril || !a->weights) return MMF_EINVAL;
  if (a->T < 0 || a->N < 0 || a->M < 1 || a->d < 1) return MMF_EINVAL;
  if (a->T >= 2 && (!a->pred_steps || !a->logd || !a->workspace || !a->residual_mean || !a->residual_second_moment)) return MMF_EINVAL;
  if (!sizes_in_range(a->M, a->N, a->d)) return MMF_ETOOLARGE;
  if (a->N == 0 || a->T < 2) return 0;
  PairArgs k{};
  k.states = a->states_steps; k.pred = a->pred_steps; k.loglik = a->loglik_steps; k.logw = a->logw_in_steps;
  k.tril = a->scale_tril; k.weights = a->weights; k.logd = a->logd;
  k.partial = a->workspace; k.mean = a->residual_mean; k.second = a->residual_second_moment;
  k.T = a->T; k.N = a->N; k.M = a->M;
  k.tiles = (a->M + kPairThreads - 1) / kPairThreads;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int T = a->T, N = a->N, tiles = k.tiles;
  return mmf::with_state_dim(a->d, [&](auto D) -> int {
    constexpr int d = decltype(D)::value;
    if (const int rc = launch_steps(pf_pair_sums_kernel<d>, tiles, N, T - 1, s, k)) return rc;
    return mmf::launch(pf_pair_reduce_kernel<d>, dim3(T - 1, N), kPairThreads, 0, s, k);
  });
}
