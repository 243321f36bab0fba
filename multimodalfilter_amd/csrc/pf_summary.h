// What the summaries of a weighted particle set share (pf_quantiles.hip, pf_scores.hip, pf_density.hip, pf_modes.hip,
// pf_distance.hip, pf_predictive.hip, pf_raster.hip): the log-weight
// a_m = log_a[m] + log_b[m] (a null pointer: 0) and the row maximum, the live-weight rule, the dealing of the O(M^2) pair
// kernels, the sum of doubles over a workgroup in its fixed order, and the host's argument, aliasing and workspace checks.
// Two rules keep a dead particle out of every sum, and they live here and nowhere else:
//   live weight    w_m = exp(a_m - max a) where a_m - max a <= 0, else 0: a NaN a_m and an empty row's -inf - -inf carry no weight
//   dead particle  a particle with w_m = 0 is selected away, never multiplied by 0: its state row (NaN, by convention) is not read
//                  into a sum, and the pair kernels stage it as zeros
// The weighted-CDF sort of pf_quantiles.hip and pf_distance.hip (its plan, keys, fixed-point weight, scan and register stages)
// is pf_sort.h, over this file.  Not shared, on purpose: the j-tile staging loops, the pair loops and the finish kernels.  The
// staging loops of pf_density.hip and pf_modes.hip differ in what they store and in their padding; those of pf_scores.hip,
// pf_predictive.hip and pf_distance.hip are alike, but one definition moved their register counts across occupancy steps
// (profiles/summary_sort/README.md).
#pragma once
#include <cmath>

#include "mmf_launch.h"

namespace mmf {
namespace summary {

constexpr int kMaxM = 16384;  // particles per row that the entry points serve

// ---- the pair kernels (pf_scores.hip, pf_density.hip, pf_modes.hip, pf_distance.hip, pf_predictive.hip)
constexpr int kIBlock = 512;   // i-particles of a workgroup at most
constexpr int kJTile = 1024;   // j-particles of an LDS tile
constexpr int kRun = 64;       // pairs an fp32 sum takes before it is flushed to double
constexpr int kMaxWaves = kIBlock / MMF_WAVE;

// how a row of M particles is dealt out: nb = ceil(M / 512) workgroups in equal i-chunks; a thread holds ipt i-particles in
// registers: one, in up to 512 threads, while the row is one workgroup, two in up to 256 beyond.  A function of M alone, so a
// row has the same bits whatever the batch
struct Plan {
  int nb, chunk, ipt, threads;
};
inline Plan plan_of(int M) {
  Plan p;
  p.nb = (M + kIBlock - 1) / kIBlock;
  p.chunk = (M + p.nb - 1) / p.nb;
  p.ipt = p.nb == 1 ? 1 : 2;
  const int lanes = (p.chunk + p.ipt - 1) / p.ipt;
  p.threads = (lanes + MMF_WAVE - 1) / MMF_WAVE * MMF_WAVE;
  return p;
}

// ---- weights
__device__ __forceinline__ float log_weight(const float* log_a, const float* log_b, size_t at) {
  const float la = log_a ? log_a[at] : 0.f, lb = log_b ? log_b[at] : 0.f;
  return la + lb;
}

// the live-weight rule, t = a_m - max a
__device__ __forceinline__ float live_weight(float t) { return t <= 0.f ? expf(t) : 0.f; }  // (a NaN t: 0)

// the maximum of v over the workgroup, in every thread (exact in any order; fmaxf skips a NaN).  scratch: one LDS word per
// wave, not touched by a workgroup of one wave (a compile-time `waves` folds the whole tail away)
__device__ __forceinline__ float block_max(float v, float* scratch, int tid, int waves) {
  v = mmf::wave_max(v);
  if (waves == 1) return v;
  if ((tid & (MMF_WAVE - 1)) == 0) scratch[tid / MMF_WAVE] = v;
  __syncthreads();
  v = scratch[0];
  for (int w = 1; w < waves; ++w) v = fmaxf(v, scratch[w]);
  return v;
}

// ---- sums of K doubles over the workgroup, in one order: a butterfly in each wave (offsets 1, 2, .. 32), then the waves
// ascending.  scratch: STRIDE >= K doubles per wave (the array's type, not a pointer and a run-time stride: with those the
// register counts of pf_density_kernel<1, 2> and <4, 2> moved across an occupancy step)
// the butterfly: every wave leaves its K sums in scratch[wave]; the caller's barrier comes next
template <int K, int STRIDE>
__device__ __forceinline__ void wave_sums(const double* v, double (*scratch)[STRIDE], int tid) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = v[k];
#pragma unroll
    for (int off = 1; off < MMF_WAVE; off <<= 1) s += __shfl_xor(s, off, MMF_WAVE);
    if ((tid & (MMF_WAVE - 1)) == 0) scratch[tid / MMF_WAVE][k] = s;
  }
}
// sum k of what wave_sums left
template <int STRIDE>
__device__ __forceinline__ double sum_of_waves(const double (*scratch)[STRIDE], int k, int waves) {
  double s = scratch[0][k];
  for (int w = 1; w < waves; ++w) s += scratch[w][k];
  return s;
}
// both, with every total in every thread (the same bits in all of them)
template <int K, int STRIDE>
__device__ __forceinline__ void block_sum(double* v, double (*scratch)[STRIDE], int tid, int waves) {
  __syncthreads();  // the scratch's last readers are done
  wave_sums<K>(v, scratch, tid);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = sum_of_waves(scratch, k, waves);
}

// component c of four j read at once
__device__ __forceinline__ float pick(float4 v, int c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// ---- host: the checks every entry point opens with, in this order around its own (which all answer MMF_EINVAL)
inline int check_rows(const void* states, int R, int M, int d) {
  return !states || R < 0 || M < 1 || d < 1 || d > MMF_MAX_STATE_DIM ? MMF_EINVAL : 0;
}
// per_row: the workgroups of a row
inline int check_size(int R, int M, int per_row) {
  return M > kMaxM || static_cast<long long>(R) * per_row > 0x7fffffffll ? MMF_ETOOLARGE : 0;
}

// the per-dimension scale of a Euclidean norm (scores, distance): every scale[k < d] positive and finite
inline int check_scale(const float* scale, int d) {
  for (int k = 0; k < d; ++k)
    if (!(scale[k] > 0.f && scale[k] < INFINITY)) return MMF_EINVAL;  // (a NaN fails)
  return 0;
}
// its reciprocals, 1 beyond d; does any of them scale at all?
inline bool inv_scale_of(const float* scale, int d, float (&inv_scale)[MMF_MAX_STATE_DIM]) {
  bool scaled = false;
  for (int i = 0; i < MMF_MAX_STATE_DIM; ++i) {
    inv_scale[i] = i < d ? 1.0f / scale[i] : 1.0f;
    scaled = scaled || inv_scale[i] != 1.0f;
  }
  return scaled;
}

// `need` bytes of workspace (0: none is read) aligned to `align`
inline bool workspace_ok(const void* ws, size_t have, size_t need, size_t align) {
  return need == 0 || (ws && have >= need && reinterpret_cast<uintptr_t>(ws) % align == 0);
}

// does an output overlap one of the inputs -- states (R, M, d), log_a and log_b (R, M), the point (R, d): the truth or the
// query -- or another output?
template <int N>
inline bool outputs_alias(const void* states, const void* log_a, const void* log_b, const void* point, size_t R, size_t M, size_t d,
                          const void* const (&outs)[N], const size_t (&out_bytes)[N]) {
  const size_t f = sizeof(float);
  const void* ins[4] = {states, log_a, log_b, point};
  const size_t in_bytes[4] = {R * M * d * f, R * M * f, R * M * f, R * d * f};
  return mmf_outputs_overlap(outs, out_bytes, N, ins, in_bytes, 4);
}

}  // namespace summary
}  // namespace mmf
