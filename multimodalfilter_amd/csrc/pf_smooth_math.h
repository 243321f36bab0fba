// The transition-density arithmetic of the particle smoothers that evaluate N(X_{t+1}[j]; F_t[i], L L^T)
// (pf_smooth_marginal.hip, pf_smooth_simulate.hip): one definition of the whitener and of the whitened squared distance.
// The exponent lives in base 2: L^-1 is scaled by sqrt(log2(e) / 2), so that v_exp_f32 takes la2 - |z|^2 as it stands.
#pragma once
#include <cmath>

#include "mmf_common.h"

namespace mmf {
namespace smooth_math {

constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

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

// the same, and the difference dx = x - f handed back (pf_smooth_pairs.hip: the residual whose moments it takes)
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

__device__ __forceinline__ float exp2_hw(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float log2_hw(float x) { return __builtin_amdgcn_logf(x); }

constexpr int kPairThreads = 64;    // threads of a pair-kernel workgroup: one column (logd) or row (sweep, pairs) each
constexpr int kPairChunk = 256;     // rows / columns staged in LDS at a time, whatever M is
constexpr int kPairGroup = 8;       // pairs evaluated in one unrolled group (logd: between two rescalings of the running maximum)

// one staged row or column of the pair kernels (pf_smooth_marginal.hip, pf_smooth_pairs.hip): D coordinates and the
// log2-weight that goes with them, in 4 (D < 4) or 8 floats
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

}  // namespace smooth_math
}  // namespace mmf
