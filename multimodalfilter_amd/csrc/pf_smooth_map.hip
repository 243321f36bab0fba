// MAP path smoothing: the most probable index path through a filter run's history (include/mmf.h, "MAP path smoothing";
// Godsill, Doucet & West 2001).  A max-plus (Viterbi) recursion over the M^2 particle pairs per trajectory and step that the
// marginal smoother of pf_smooth_marginal.hip walks with a log-sum-exp, on the same transition density
// N(X_{t+1}[j]; F_t[i], L L^T).  Three kinds of launch behind one C call:
//   first      element-wise over (column tile, trajectory): v_0 = loglik_0 + logw_in_0, psi_0 = -1
//   forward    T - 1 launches over (column tile, trajectory), t = 1 .. T - 1: a thread owns a column j of step t, the rows i of
//              step t - 1 -- F_{t-1}[i] and v_{t-1}[i] - top_{t-1} -- stream through LDS; every workgroup takes top_{t-1} of
//              its trajectory itself (a maximum is exact in any order) and the one with blockIdx.x == 0 stores it
//   backtrack  one wave per trajectory: the first maximum of v_{T-1}, one lane walks psi backwards, the sum of the top_t
// Inside the forward kernel the values live in base 2 (L^-1 is scaled by sqrt(log2(e) / 2), pf_smooth_math.h); every output is
// in natural logarithms.  No exp, no log, no float atomics; every sum in one fixed order.

#include <cmath>

#include "pf_smooth_math.h"

namespace {

using namespace mmf::smooth_math;  // the log-weights, the first maximum, the transition density, the staged chunks

struct MapArgs {
  const float* states;   // (T, N, M, D)
  const float* pred;     // (T - 1, N, M, D)
  const float* loglik;   // (T, N, M)
  const float* logw;     // (T, N, M) or null: step 0 alone is read
  const float* tril;     // (D, D)
  float* v;              // (T, N, M), natural logarithm
  float* step_max;       // (T, N)
  int* psi;              // (T, N, M)
  int* indices;          // (T, N)
  float* path;           // (T, N, D)
  float* logpost;        // (N)
  int T, N, M;
  int t0;                // forward: the step t
};

// a diagonal entry of L that is not a positive finite number: every floating output is NaN, every index -1
template <int D>
__device__ __forceinline__ bool bad_factor(const float* __restrict__ tril) {
  bool bad = false;
#pragma unroll
  for (int r = 0; r < D; ++r) {
    const float g = tril[r * D + r];
    bad = bad || !(g > 0.f) || !(g < INFINITY);
  }
  return bad;
}

// ---- first: v_0[j] = loglik_0[j] + logw_in_0[j], psi_0 = -1
template <int D>
__global__ __launch_bounds__(kPairThreads) void pf_map_first_kernel(MapArgs a) {
  const int n = blockIdx.y, M = a.M, j = blockIdx.x * kPairThreads + threadIdx.x;
  if (j >= M) return;
  const size_t row0 = static_cast<size_t>(n) * M;
  a.v[row0 + j] = bad_factor<D>(a.tril) ? NAN : log_weight(a.loglik + row0, a.logw ? a.logw + row0 : nullptr, j);
  a.psi[row0 + j] = -1;
}

// ---- forward, step t: v_t[j] = loglik_t[j] + max_i((v_{t-1}[i] - top_{t-1}) + lp_{t-1}[i, j]) for the columns of one tile,
// psi_t[j] the first i that attains it
template <int D>
__global__ __launch_bounds__(kPairThreads) void pf_map_forward_kernel(MapArgs a) {
#pragma clang fp contract(off)
  __shared__ float4 lds[kPairChunk * Staged<D>::kFloat4s];
  const int tid = threadIdx.x, n = blockIdx.y, t = a.t0, M = a.M;
  const size_t nm = static_cast<size_t>(a.N) * M;
  const size_t rows_t = static_cast<size_t>(t - 1) * nm + static_cast<size_t>(n) * M;  // step t - 1: the rows i
  const size_t cols_t = static_cast<size_t>(t) * nm + static_cast<size_t>(n) * M;      // step t: the columns j
  const int j = blockIdx.x * kPairThreads + tid;
  const bool bad = bad_factor<D>(a.tril);
  float W[D][D];
  whitener<D>(a.tril, W);
  // top_{t-1}: M reads beside the workgroup's 64 M pairs
  float top = -INFINITY;
  for (int m = tid; m < M; m += kPairThreads) top = fmaxf(top, a.v[rows_t + m]);
  top = mmf::wave_max(top);
  if (bad) top = NAN;
  if (blockIdx.x == 0 && tid == 0) a.step_max[static_cast<size_t>(t - 1) * a.N + n] = top;
  const float ll = j < M ? a.loglik[cols_t + j] : -INFINITY;
  const bool dead_col = ll == -INFINITY;  // its row may hold anything: it is not read
  float x[D];
  {
    const float* X = a.states + (cols_t + min(j, M - 1)) * D;
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = dead_col ? 0.f : X[c];
  }
  float best = -INFINITY;
  int arg = -1;
  for (int c0 = 0; c0 < M; c0 += kPairChunk) {
    __syncthreads();  // the previous chunk has been consumed
#pragma unroll
    for (int k = 0; k < kPairChunk / kPairThreads; ++k) {
      const int s = k * kPairThreads + tid, i = c0 + s;
      Staged<D> row;
      const float vi = i < M ? a.v[rows_t + i] : -INFINITY;
      row.w = vi == -INFINITY ? -INFINITY : (vi - top) * kLog2e;
      const bool dead = row.w == -INFINITY;
#pragma unroll
      for (int c = 0; c < D; ++c) row.x[c] = dead ? 0.f : a.pred[(rows_t + i) * D + c];
      row.store(lds, s);
    }
    __syncthreads();
    const int rows = padded_chunk(M, c0);
    for (int i0 = 0; i0 < rows; i0 += kPairGroup) {
      float g[kPairGroup];
      float gm = -INFINITY;
#pragma unroll
      for (int u = 0; u < kPairGroup; ++u) {
        Staged<D> row;
        row.load(lds, i0 + u);
        g[u] = minus_sq_dist<D>(row.w, x, row.x, W);
        gm = fmaxf(gm, g[u]);
      }
      // rows ascend: only a strictly larger group moves the maximum, and inside it the first row that holds the value wins
      if (gm > best) {
        best = gm;
        int first = kPairGroup - 1;
#pragma unroll
        for (int u = kPairGroup - 2; u >= 0; --u) first = g[u] == gm ? u : first;
        arg = c0 + i0 + first;
      }
    }
  }
  if (j < M) {
    const bool none = dead_col || arg < 0;
    a.v[cols_t + j] = bad ? NAN : (none ? -INFINITY : ll + best * kLn2);
    a.psi[cols_t + j] = bad || none ? -1 : arg;
  }
}

// ---- backtrack: i_{T-1} = first argmax v_{T-1}, i_t = psi_{t+1}[i_{t+1}], path[t] = X_t[i_t], log_posterior = sum_t top_t - (T - 1) c
template <int D>
__global__ __launch_bounds__(kPairThreads) void pf_map_backtrack_kernel(MapArgs a) {
#pragma clang fp contract(off)
  __shared__ float wv[1];
  __shared__ int wi[1];
  const int tid = threadIdx.x, n = blockIdx.x, T = a.T, N = a.N, M = a.M;
  const size_t nm = static_cast<size_t>(N) * M;
  const float* last = a.v + static_cast<size_t>(T - 1) * nm + static_cast<size_t>(n) * M;
  const bool bad = bad_factor<D>(a.tril);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int m = tid; m < M; m += kPairThreads) {
    const float e = last[m];
    if (e > bv) { bv = e; bi = m; }
  }
  first_max(bv, bi, wv, wi, tid, 1, M);
  if (tid != 0) return;
  const float top = bad ? NAN : bv;
  a.step_max[static_cast<size_t>(T - 1) * N + n] = top;
  float c = 0.5f * D * logf(6.283185307179586f);
#pragma unroll
  for (int r = 0; r < D; ++r) c = c + logf(a.tril[r * D + r]);
  float sum = 0.f;
  for (int t = 0; t < T; ++t) sum = sum + a.step_max[static_cast<size_t>(t) * N + n];
  const bool alive = !bad && bv > -INFINITY;  // a step where every particle is dead leaves every later one dead
  a.logpost[n] = bad ? NAN : (alive ? sum - static_cast<float>(T - 1) * c : -INFINITY);
  int i = alive ? bi : -1;
  for (int t = T - 1; t >= 0; --t) {
    if (i < 0 || i >= M) i = -1;  // (reads stay in range whatever psi holds)
    const size_t out = static_cast<size_t>(t) * N + n;
    a.indices[out] = i;
    const size_t row = static_cast<size_t>(t) * nm + static_cast<size_t>(n) * M + (i < 0 ? 0 : i);
#pragma unroll
    for (int k = 0; k < D; ++k) a.path[out * D + k] = i < 0 ? NAN : a.states[row * D + k];
    if (t > 0) i = i < 0 ? -1 : a.psi[row];
  }
}

}  // namespace

extern "C" int mmf_pf_smooth_map(const MmfPfSmoothMapArgs* a, void* stream) {
  if (!a || !a->states_steps || !a->loglik_steps || !a->scale_tril || !a->v || !a->step_max || !a->backpointers || !a->indices ||
      !a->path || !a->log_posterior)
    return MMF_EINVAL;
  if (a->T < 0 || a->N < 0 || a->M < 1 || a->d < 1) return MMF_EINVAL;
  if (a->T >= 2 && !a->pred_steps) return MMF_EINVAL;
  if (!sizes_in_range(a->M, a->N, a->d)) return MMF_ETOOLARGE;
  {
    const size_t T = a->T, N = a->N, M = a->M, d = a->d, f = sizeof(float);
    const void* ins[5] = {a->states_steps, a->pred_steps, a->loglik_steps, a->logw_in_steps, a->scale_tril};
    const size_t in_bytes[5] = {T * N * M * d * f, (T ? T - 1 : 0) * N * M * d * f, T * N * M * f, T * N * M * f, d * d * f};
    const void* outs[6] = {a->v, a->step_max, a->backpointers, a->indices, a->path, a->log_posterior};
    const size_t out_bytes[6] = {T * N * M * f, T * N * f, T * N * M * sizeof(int32_t), T * N * sizeof(int32_t), T * N * d * f, N * f};
    for (int o = 0; o < 6; ++o) {
      for (int i = 0; i < 5; ++i)
        if (mmf_bytes_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) return MMF_EINVAL;
      for (int p = 0; p < o; ++p)
        if (mmf_bytes_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p])) return MMF_EINVAL;
    }
  }
  if (a->N == 0 || a->T == 0) return 0;
  MapArgs k{};
  k.states = a->states_steps; k.pred = a->pred_steps; k.loglik = a->loglik_steps; k.logw = a->logw_in_steps;
  k.tril = a->scale_tril; k.v = a->v; k.step_max = a->step_max; k.psi = a->backpointers; k.indices = a->indices;
  k.path = a->path; k.logpost = a->log_posterior;
  k.T = a->T; k.N = a->N; k.M = a->M;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int T = a->T, N = a->N;
  const int tiles = (a->M + kPairThreads - 1) / kPairThreads;
  return mmf::with_state_dim(a->d, [&](auto D) -> int {
    constexpr int d = decltype(D)::value;
    if (const int rc = mmf::launch(pf_map_first_kernel<d>, dim3(tiles, N), kPairThreads, 0, s, k)) return rc;
    for (int t = 1; t < T; ++t) {
      k.t0 = t;
      if (const int rc = mmf::launch(pf_map_forward_kernel<d>, dim3(tiles, N), kPairThreads, 0, s, k)) return rc;
    }
    return mmf::launch(pf_map_backtrack_kernel<d>, N, kPairThreads, 0, s, k);
  });
}
