// What the four particle smoothers share (pf_smooth.hip, pf_smooth_marginal.hip, pf_smooth_simulate.hip, pf_smooth_pairs.hip):
// the log-weights of a step, the first-maximum search, the pivot-form moment sums, the transition-density arithmetic of
// N(X_{t+1}[j]; F_t[i], L L^T), the staged chunks of the O(M^2) pair kernels, and the host's size checks and step batches.
// The exponent lives in base 2: L^-1 is scaled by sqrt(log2(e) / 2), so that v_exp_f32 takes la2 - |z|^2 as it stands.
#pragma once
#include <cmath>

#include "mmf_launch.h"

namespace mmf {
namespace smooth_math {

constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

__device__ __forceinline__ float exp2_hw(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float log2_hw(float x) { return __builtin_amdgcn_logf(x); }

// ---- log-weights: a = loglik + logw_in (logw_in may be null)
__device__ __forceinline__ float log_weight(const float* ll, const float* lw, int m) { return lw ? ll[m] + lw[m] : ll[m]; }

// log2 of the unnormalised weight of a particle, relative to the step's largest: -inf stays -inf (every value -inf included)
__device__ __forceinline__ float log2_weight(float a, float amax) { return a == -INFINITY ? -INFINITY : (a - amax) * kLog2e; }

// what an online (max, sum) rescales to: nothing alive so far gives exp2(-inf - 0) = 0, not exp2(nan)
__device__ __forceinline__ float rescale_ref(float top) { return top == -INFINITY ? 0.f : top; }

// ---- the first largest value of a workgroup and its index, ties to the lower index.  Every thread brings the first maximum
// (bv, bi) of its own elements (ascending index per thread: the first of equal values stays) and leaves with the
// workgroup's: every thread combines the waves' candidates in the same order.  wv, wi: one LDS word per wave each.  No
// finite or +inf value (every one -inf or NaN): index 0, the result is NaN either way and the reads stay in range.
__device__ __forceinline__ void first_max(float& bv, int& bi, float* wv, int* wi, int tid, int waves, int M) {
  auto better = [](float v, int i, float w, int j) { return v > w || (v == w && i < j); };
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((tid & (MMF_WAVE - 1)) == 0) { wv[tid >> 6] = bv; wi[tid >> 6] = bi; }
  __syncthreads();
  bv = wv[0];
  bi = wi[0];
  for (int k = 1; k < waves; ++k)
    if (better(wv[k], wi[k], bv, bi)) { bv = wv[k]; bi = wi[k]; }
  if (bi < 0 || bi >= M) bi = 0;
}

// ---- pivot-form moments: m1 = sum e (x - p) and the upper triangle of M2 = sum e (x - p)(x - p)^T around a pivot row p,
// mean = p + m1 / S, cov = M2 / S - (m1 / S)(m1 / S)^T.  Every sum in one fixed order, no contraction.
constexpr int moment_sums(int d) { return d + d * (d + 1) / 2; }
constexpr int kMomentThreads = 256;  // the workgroup of the marginal and the simulation moments
constexpr int kMomentWaves = kMomentThreads / MMF_WAVE;
constexpr int kMomentSums = moment_sums(MMF_MAX_STATE_DIM);

// where moment_sums keeps (i, j), i <= j, of the upper triangle (row-major, behind the D first moments)
template <int D>
__device__ __forceinline__ constexpr int tri_index(int i, int j) { return D + i * D - i * (i - 1) / 2 + (j - i); }

template <int D>
__device__ __forceinline__ void pivot_accumulate(float (&acc)[moment_sums(D)], float e, const float* x, const float (&p)[D]) {
#pragma clang fp contract(off)
  float dx[D];
#pragma unroll
  for (int c = 0; c < D; ++c) dx[c] = x[c] - p[c];
  int v = D;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    acc[i] = acc[i] + e * dx[i];
#pragma unroll
    for (int j = i; j < D; ++j, ++v) acc[v] = acc[v] + (e * dx[i]) * dx[j];
  }
}

// NS register sums of every thread -> total[0 .. NS): wave sums, then the waves' partials (partial[v * stride + wave]) added
// in wave order.  total is readable after the caller's next barrier (what else waits for the partials goes before it).
template <int NS>
__device__ __forceinline__ void block_sums(const float (&acc)[NS], float* partial, float* total, int stride, int waves, int tid) {
#pragma clang fp contract(off)
#pragma unroll
  for (int v = 0; v < NS; ++v) {
    const float r = mmf::wave_sum(acc[v]);
    if ((tid & (MMF_WAVE - 1)) == 0) partial[v * stride + (tid >> 6)] = r;
  }
  __syncthreads();
  if (tid < NS) {
    float r = 0.f;
    for (int w = 0; w < waves; ++w) r = r + partial[tid * stride + w];
    total[tid] = r;
  }
}

// mean (D) and cov (D x D, or null) of output slot `out` from the totals, S the sum of the weights
template <int D>
__device__ __forceinline__ void write_moments(float* mean, float* cov, size_t out, int tid, const float (&p)[D], const float* total,
                                              float S) {
#pragma clang fp contract(off)
  if (tid < D) mean[out * D + tid] = p[tid] + total[tid] / S;
  if (cov && tid < D * D) {
    const int r = tid / D, c = tid % D, i = min(r, c), j = max(r, c);
    cov[out * D * D + tid] = total[tri_index<D>(i, j)] / S - (total[i] / S) * (total[j] / S);
  }
}

// ---- the transition density
// sqrt(log2(e) / 2) L^-1 by forward substitution, column by column (uniform over the workgroup).  A diagonal entry that is
// not a positive finite number makes every entry NaN, and with them every result.
template <int D>
__device__ __forceinline__ void whitener(const float* __restrict__ tril, float (&W)[D][D]) {
  const float s = sqrtf(0.5f * kLog2e);
  bool bad = false;
#pragma unroll
  for (int r = 0; r < D; ++r) {
    const float g = tril[r * D + r];
    bad = bad || !(g > 0.f) || !(g < INFINITY);
  }
#pragma unroll
  for (int c = 0; c < D; ++c)
#pragma unroll
    for (int r = 0; r < D; ++r) {
      float acc = r == c ? s : 0.f;
      if (r < c) { W[r][c] = 0.f; continue; }
#pragma unroll
      for (int k = c; k < r; ++k) acc = acc - tril[r * D + k] * W[k][c];
      W[r][c] = bad ? NAN : acc / tril[r * D + r];
    }
}

// |sqrt(log2(e) / 2) L^-1 (x - f)|^2 subtracted from `from`: the difference first, then the whitening
template <int D>
__device__ __forceinline__ float minus_sq_dist(float from, const float (&x)[D], const float (&f)[D], const float (&W)[D][D]) {
  float dx[D];
#pragma unroll
  for (int c = 0; c < D; ++c) dx[c] = x[c] - f[c];
#pragma unroll
  for (int r = 0; r < D; ++r) {
    float z = W[r][0] * dx[0];
#pragma unroll
    for (int c = 1; c <= r; ++c) z = fmaf(W[r][c], dx[c], z);
    from = fmaf(-z, z, from);
  }
  return from;
}

// the same, and the difference dx = x - f handed back (pf_smooth_pairs.hip: the residual whose moments it takes).  Its own
// body: with minus_sq_dist as a call of this one the marginal sweep's instructions came out in another order and the marginal
// recursion measured 1.3 % slower at 32 x 4096 x 20 (profiles/smooth_shared/README.md, "what stays")
template <int D>
__device__ __forceinline__ float minus_sq_dist_dx(float from, const float (&x)[D], const float (&f)[D], const float (&W)[D][D],
                                                  float (&dx)[D]) {
#pragma unroll
  for (int c = 0; c < D; ++c) dx[c] = x[c] - f[c];
#pragma unroll
  for (int r = 0; r < D; ++r) {
    float z = W[r][0] * dx[0];
#pragma unroll
    for (int c = 1; c <= r; ++c) z = fmaf(W[r][c], dx[c], z);
    from = fmaf(-z, z, from);
  }
  return from;
}

// ---- the pair kernels (pf_smooth_marginal.hip, pf_smooth_pairs.hip): rows or columns stream through LDS in chunks
constexpr int kPairThreads = 64;    // threads of a pair-kernel workgroup: one column (logd) or row (sweep, pairs) each
constexpr int kPairChunk = 256;     // rows / columns staged in LDS at a time, whatever M is
constexpr int kPairGroup = 8;       // pairs evaluated in one unrolled group (logd: between two rescalings of the running maximum)
static_assert(kPairThreads == MMF_WAVE, "a pair workgroup is one wave: its sums are wave sums");
static_assert(kPairChunk % kPairThreads == 0 && kPairChunk % kPairGroup == 0, "a chunk is staged and consumed whole");

// one staged row or column: D coordinates and the log2-weight that goes with them, in 4 (D < 4) or 8 floats
template <int D>
struct Staged {
  static constexpr int kFloat4s = D < 4 ? 1 : 2;
  float x[D];
  float w;
  __device__ __forceinline__ void store(float4* lds, int i) const {
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < D; ++c) v[c] = x[c];
    v[D] = w;
    lds[i * kFloat4s] = make_float4(v[0], v[1], v[2], v[3]);
    if (D == 4) lds[i * kFloat4s + 1] = make_float4(v[4], v[5], v[6], v[7]);
  }
  // every lane reads the same address: a broadcast, no bank conflict
  __device__ __forceinline__ void load(const float4* lds, int i) {
    const float4 a = lds[i * kFloat4s];
    const float v[5] = {a.x, a.y, a.z, a.w, D < 4 ? 0.f : reinterpret_cast<const float*>(lds)[i * 4 * kFloat4s + 4]};
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = v[c];
    w = v[D];
  }
};

// the staged entries of the chunk at c0 that are walked: whole groups, the padding entries carry no weight
__device__ __forceinline__ int padded_chunk(int M, int c0) { return min(kPairChunk, (M - c0 + kPairGroup - 1) / kPairGroup * kPairGroup); }

// ---- host
inline bool sizes_in_range(int M, int N, int d) { return d <= MMF_MAX_STATE_DIM && M <= 65536 && N <= 65535; }

// kernel over `steps` independent steps: the grid's z holds 65535 of them, args.t0 is the step of blockIdx.z == 0
template <class A>
int launch_steps(void (*kernel)(A), int tiles, int N, int steps, hipStream_t s, A& args) {
  constexpr int kMaxGridZ = 65535;
  for (int t0 = 0; t0 < steps; t0 += kMaxGridZ) {
    args.t0 = t0;
    if (const int rc = mmf::launch(kernel, dim3(tiles, N, steps - t0 < kMaxGridZ ? steps - t0 : kMaxGridZ), kPairThreads, 0, s, args))
      return rc;
  }
  return 0;
}

}  // namespace smooth_math
}  // namespace mmf
