// Weighted quantiles and the weighted CDF of a particle set, per row and state dimension (include/mmf.h, "Particle-posterior
// quantiles"): K1's integer fixed-point weights q_m = floor(exp(a_m - max a) 2^24), so that every sum is an integer sum and the
// selection does not depend on the thread count, the scan order or the number of rows.  One kernel, one workgroup per
// (row, dimension):
//   weights    a = log_a + log_b held in registers, the row maximum, q_m under the live-weight rule (sort::fixed_weight)
//   cdf        the integer sum of q_m over x_m <= query, reduced before the sort; Q == 0 ends here
//   keys       (order-preserving uint32 of x_m) << 32 | q_m, one uint64 per particle in LDS, padded to P = 2^k >= M with
//              all-ones keys of weight 0
//   sort       the bitonic sort of pf_sort.h (its plan, slots and register stages; the body's text is here): a thread ends with
//              its E = P / THREADS consecutive sorted slots in registers
//   scan       the thread sums of the sorted runs (sort::block_scan)
//   search     per p: thr = max(1, ceil(p Qtot)) in double; the one thread whose run crosses thr walks it and stores the value
// The weights are recomputed by each of the d workgroups of a row (M reads, M exp beside a sort of P log^2 P compare-exchanges).

#include <cmath>

#include "pf_sort.h"

namespace {

namespace summary = mmf::summary;
namespace sort = mmf::sort;
using sort::u64;

struct QArgs {
  const float* states;  // (R, M, d)
  const float* log_a;   // (R, M) or null
  const float* log_b;   // (R, M) or null
  const float* query;   // (R, d) or null
  float* quantiles;     // (R, Q, d) or null
  float* cdf;           // (R, d) or null
  int M, d, Q;
  float probs[MMF_QUANTILES_MAX];
};

template <int THREADS, int E>
__global__ __launch_bounds__(THREADS) void pf_quantiles_kernel(QArgs a) {
  extern __shared__ u64 lds[];
  __shared__ u64 wave_tot[sort::kMaxWaves];
  __shared__ float wave_top[sort::kMaxWaves];
  const int tid = threadIdx.x, M = a.M, d = a.d;
  const int r = blockIdx.x / d, k = blockIdx.x - r * d;
  const size_t row = static_cast<size_t>(r) * M;
  const float* x = a.states + row * d + k;

  // a_m = log_a[m] + log_b[m]; particle m = tid + u THREADS.  The row's own pointers: the row offset stays in scalar registers
  const float *la = a.log_a ? a.log_a + row : nullptr, *lb = a.log_b ? a.log_b + row : nullptr;
  float av[E];
  float top = -INFINITY;
#pragma unroll
  for (int u = 0; u < E; ++u) {
    const int m = tid + u * THREADS;
    av[u] = m < M ? summary::log_weight(la, lb, m) : -INFINITY;
    top = fmaxf(top, av[u]);  // (a NaN is skipped)
  }
  top = summary::block_max(top, wave_top, tid, THREADS / MMF_WAVE);
  if constexpr (THREADS > MMF_WAVE) __syncthreads();  // (not needed; without it the sort of 4096 particles measured 1.7 % slower)

  const bool want_cdf = a.query != nullptr;
  const float query = want_cdf ? a.query[static_cast<size_t>(r) * d + k] : 0.f;
  u64 qsum = 0, below = 0;
#pragma unroll
  for (int u = 0; u < E; ++u) {
    const int m = tid + u * THREADS;
    u64 packed = sort::kPadKey;
    if (m < M) {
      const unsigned q = sort::fixed_weight(av[u] - top);
      const float xv = x[static_cast<size_t>(m) * d];
      qsum += q;
      if (xv <= query) below += q;
      packed = (static_cast<u64>(sort::key_of(xv)) << 32) | q;
    }
    if (a.Q > 0) lds[sort::slot<E>(m)] = packed;
  }
  u64 Qtot, below_tot = 0;
  sort::block_scan<THREADS>(qsum, wave_tot, tid, Qtot);
  if (want_cdf) sort::block_scan<THREADS>(below, wave_tot, tid, below_tot);
  const bool dead = !(top > -INFINITY) || !(top < INFINITY) || Qtot == 0;  // no live particle in the row
  if (want_cdf && tid == 0) {
    const float c = static_cast<float>(static_cast<double>(below_tot) / static_cast<double>(Qtot));
    a.cdf[static_cast<size_t>(r) * d + k] = dead || query != query ? NAN : c;
  }
  if (a.Q == 0) return;
  if (dead) {
    for (int i = tid; i < a.Q; i += THREADS) a.quantiles[(static_cast<size_t>(r) * a.Q + i) * d + k] = NAN;
    return;
  }

  // ---- bitonic sort, ascending (pf_sort.h: one textual copy here and in pf_distance.hip)
  constexpr int P = THREADS * E;
  const int base = tid * E;
  u64 v[E];
  __syncthreads();
  if constexpr (E > 1) {
#pragma unroll
    for (int l = 0; l < E; ++l) v[l] = lds[sort::slot<E>(base) + l];
#pragma unroll
    for (int kk = 2; kk <= E; kk <<= 1) sort::local_stages<E>(v, base, kk, kk / 2);
    for (int kk = 2 * E; kk <= P; kk <<= 1) {
#pragma unroll
      for (int l = 0; l < E; ++l) lds[sort::slot<E>(base) + l] = v[l];
      __syncthreads();
      for (int j = kk / 2; j >= E; j >>= 1) {
#pragma unroll
        for (int u = 0; u < E / 2; ++u) {
          const int p = tid + u * THREADS;
          const int i = 2 * p - (p & (j - 1));  // pair p of stride j: 2 j (p / j) + p % j
          const bool up = (i & kk) == 0;
          const u64 lo = lds[sort::slot<E>(i)], hi = lds[sort::slot<E>(i + j)];
          if ((lo > hi) == up) {
            lds[sort::slot<E>(i)] = hi;
            lds[sort::slot<E>(i + j)] = lo;
          }
        }
        __syncthreads();
      }
#pragma unroll
      for (int l = 0; l < E; ++l) v[l] = lds[sort::slot<E>(base) + l];
      sort::local_stages<E>(v, base, kk, E / 2);
    }
  } else {
    for (int kk = 2; kk <= P; kk <<= 1)
      for (int j = kk / 2; j >= 1; j >>= 1) {
        if (tid < P / 2) {
          const int i = 2 * tid - (tid & (j - 1));  // pair tid of stride j: 2 j (tid / j) + tid % j
          const bool up = (i & kk) == 0;
          const u64 lo = lds[i], hi = lds[i + j];
          if ((lo > hi) == up) {
            lds[i] = hi;
            lds[i + j] = lo;
          }
        }
        __syncthreads();
      }
    v[0] = lds[tid];
  }

  // ---- the integer CDF in sorted order: this thread's run covers (excl, excl + mine]
  u64 mine = 0;
#pragma unroll
  for (int l = 0; l < E; ++l) mine += v[l] & 0xFFFFFFFFull;
  u64 total;
  const u64 excl = sort::block_scan<THREADS>(mine, wave_tot, tid, total) - mine;
#pragma unroll 1
  for (int i = 0; i < a.Q; ++i) {
    const double want = ceil(static_cast<double>(a.probs[i]) * static_cast<double>(total));
    const u64 thr = want < 1.0 ? 1ull : static_cast<u64>(want);
    if (excl < thr && thr <= excl + mine) {
      u64 c = excl;
      unsigned key = 0;
      bool found = false;
#pragma unroll
      for (int l = 0; l < E; ++l) {
        c += v[l] & 0xFFFFFFFFull;
        const bool hit = !found && c >= thr;
        key = hit ? static_cast<unsigned>(v[l] >> 32) : key;
        found = found || hit;
      }
      a.quantiles[(static_cast<size_t>(r) * a.Q + i) * d + k] = sort::value_of(key);
    }
  }
}

}  // namespace

extern "C" size_t mmf_pf_quantiles_lds_bytes(int M) {
  if (M < 1) return 0;
  if (M > summary::kMaxM) M = summary::kMaxM;
  return sort::slots_of(sort::plan_of(M)) * sizeof(u64);
}

extern "C" int mmf_pf_quantiles(const MmfPfQuantilesArgs* a, void* stream) {
  if (!a || summary::check_rows(a->states, a->R, a->M, a->d) || a->Q < 0 || a->Q > MMF_QUANTILES_MAX) return MMF_EINVAL;
  for (int i = 0; i < a->Q; ++i)
    if (!(a->probs[i] >= 0.f && a->probs[i] <= 1.f)) return MMF_EINVAL;
  if (a->Q == 0 && !a->query) return MMF_EINVAL;
  if (a->Q > 0 && !a->quantiles) return MMF_EINVAL;
  if ((a->query != nullptr) != (a->cdf != nullptr)) return MMF_EINVAL;
  if (const int rc = summary::check_size(a->R, a->M, a->d)) return rc;
  {
    const size_t R = a->R, M = a->M, d = a->d, Q = a->Q, f = sizeof(float);
    const void* outs[2] = {a->quantiles, a->cdf};
    const size_t out_bytes[2] = {R * Q * d * f, R * d * f};
    if (summary::outputs_alias(a->states, a->log_a, a->log_b, a->query, R, M, d, outs, out_bytes)) return MMF_EINVAL;
  }
  if (a->R == 0) return 0;
  QArgs k{};
  k.states = a->states; k.log_a = a->log_a; k.log_b = a->log_b; k.query = a->query;
  k.quantiles = a->quantiles; k.cdf = a->cdf;
  k.M = a->M; k.d = a->d; k.Q = a->Q;
  for (int i = 0; i < a->Q; ++i) k.probs[i] = a->probs[i];
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(a->R) * static_cast<unsigned>(a->d);
  const sort::Plan p = sort::plan_of(a->M);
  return sort::with_plan(p, [&](auto T, auto E) {
    constexpr int kT = decltype(T)::value, kE = decltype(E)::value;
    return mmf::launch(pf_quantiles_kernel<kT, kE>, grid, kT, sort::slots_of(p) * sizeof(u64), s, k);
  });
}
