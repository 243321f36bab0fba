// The weighted-CDF sort of a particle set (pf_quantiles.hip, pf_distance.hip): one uint64 per particle in LDS,
// (order-preserving uint32 of the coordinate) << 32 | K1's integer fixed-point weight q = floor(exp(a - max a) 2^24), padded
// to P = 2^k slots with all-ones keys of weight 0, and sorted ascending by one workgroup, so that every CDF is an integer sum
// in sorted order and does not depend on the thread count, the scan order or the number of rows.
//   sort       bitonic over the P uint64s: a thread owns E = P / THREADS consecutive slots; the stages whose stride is below E
//              run in its registers, the others through LDS.  Slot i lives at i + i / E: the E-slot runs of neighbouring lanes
//              start 8 (E + 1) bytes apart, an odd number of 8-byte bank pairs, so the run loads and stores are conflict-free
//   scan       thread sums, the wave scan of K1 (mmf::wave_inclusive_scan), wave totals through LDS
// The callers keep what is theirs: how a slot is filled and what is read off the sorted runs -- and, each, one textual copy of
// the sort's body over slot and local_stages ("---- bitonic sort, ascending": keep the two alike).  As a __forceinline__
// function here the body left every register, spill and LDS figure of the 18 kernels in place (one: 436 -> 438) and all bits
// equal, but at 32 x 4096 x 20 (pf_quantiles_kernel<256, 16>) hip_quantiles_only measured 0.1660 ms in the middle of three
// runs against 0.1632 + 0.0023 ms, the slowest of the parent's four plus their spread, and about 1 % more than the parent
// over three such calls; with the body in the kernels 34 of their 35 kernels are the parent's, byte for byte
// (profiles/summary_sort/README.md)
#pragma once
#include <type_traits>

#include "pf_summary.h"

namespace mmf {
namespace sort {

using u64 = unsigned long long;

constexpr int kMaxWaves = 4;
constexpr u64 kPadKey = 0xFFFFFFFF00000000ull;

// threads and slots per thread of the workgroup that sorts M particles: one wave up to P = 512 (8 slots per lane), 256 threads
// beyond.  Measured at P = 512 on the 32 x 300 x 100 history: 256 threads x 2 slots 0.083 ms, 128 x 4 0.076 ms, 64 x 8 0.067 ms;
// at P = 4096: 256 x 16 0.162 ms, 128 x 32 0.214 ms, 64 x 64 0.314 ms (profiles/quantiles/README.md)
struct Plan {
  int threads, E;
};
inline Plan plan_of(int M) {
  int P = MMF_WAVE;
  while (P < M) P <<= 1;
  const int threads = P <= 8 * MMF_WAVE ? MMF_WAVE : 256;
  return {threads, P / threads};
}
inline size_t slots_of(const Plan& p) {
  return static_cast<size_t>(p.threads) * p.E + (p.E > 1 ? p.threads : 0);  // the padding slot after every run of E
}

// f(THREADS, E) with the plan as compile-time constants: the nine forms that plan_of gives up to summary::kMaxM
template <class F>
auto with_plan(const Plan& p, F&& f) {
  static_assert(summary::kMaxM == 256 * 64, "one case per plan");
  using W = std::integral_constant<int, MMF_WAVE>;
  using B = std::integral_constant<int, 256>;
  if (p.threads == MMF_WAVE) {
    switch (p.E) {
      case 1: return f(W{}, std::integral_constant<int, 1>{});
      case 2: return f(W{}, std::integral_constant<int, 2>{});
      case 4: return f(W{}, std::integral_constant<int, 4>{});
      default: return f(W{}, std::integral_constant<int, 8>{});
    }
  }
  switch (p.E) {
    case 4: return f(B{}, std::integral_constant<int, 4>{});
    case 8: return f(B{}, std::integral_constant<int, 8>{});
    case 16: return f(B{}, std::integral_constant<int, 16>{});
    case 32: return f(B{}, std::integral_constant<int, 32>{});
    default: return f(B{}, std::integral_constant<int, 64>{});
  }
}

// the fixed-point weight under the live-weight rule (pf_summary.h), t = a_m - max a
__device__ __forceinline__ unsigned fixed_weight(float t) {
  const float e = expf(t);
  return t <= 0.f ? static_cast<unsigned>(floorf(e * 16777216.0f)) : 0u;  // (a NaN t: 0)
}

// a total order on the bit patterns that agrees with < on the numbers: negatives inverted, the others with the sign bit set
__device__ __forceinline__ unsigned key_of(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float value_of(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

template <int E>
__device__ __forceinline__ int slot(int i) {
  return E > 1 ? i + i / E : i;
}

// inclusive scan of per-thread values below 2^40 over the workgroup, and its total
template <int THREADS>
__device__ __forceinline__ u64 block_scan(u64 v, u64* scratch, int tid, u64& total) {
  const int lane = tid & (MMF_WAVE - 1), wave = tid / MMF_WAVE;
  u64 incl = mmf::wave_inclusive_scan(v, lane);
  if (lane == MMF_WAVE - 1) scratch[wave] = incl;
  __syncthreads();
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / MMF_WAVE; ++w) {
    const u64 t = scratch[w];
    if (w < wave) incl += t;
    total += t;
  }
  __syncthreads();
  return incl;
}

// the stages of phase k whose stride is jmax, jmax / 2, .. 1, all below E: inside the E consecutive slots from `base`
template <int E>
__device__ __forceinline__ void local_stages(u64 (&v)[E], int base, int k, int jmax) {
#pragma unroll
  for (int j = E / 2; j >= 1; j >>= 1) {
    if (j > jmax) continue;
#pragma unroll
    for (int l = 0; l < E; ++l) {
      if (l & j) continue;
      const bool up = ((base + l) & k) == 0;
      const u64 lo = v[l], hi = v[l + j];
      const bool swap = (lo > hi) == up;
      v[l] = swap ? hi : lo;
      v[l + j] = swap ? lo : hi;
    }
  }
}

}  // namespace sort
}  // namespace mmf
