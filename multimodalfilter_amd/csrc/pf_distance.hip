// Two-sample distances between two weighted particle sets, per row pair (include/mmf.h, "Particle-posterior distances"):
// per state dimension the 1-Wasserstein distance, the Cramer distance and the Kolmogorov-Smirnov statistic between the two
// weighted empirical CDFs, and in the Euclidean norm the energy distance with its three expectations.  Two kernels:
//   cdf     pf_distance_cdf_kernel<THREADS, E>, a workgroup per (row pair, dimension), on K1's integer fixed-point weights
//           q = floor(exp(a - max a) 2^24) -- each set under its own maximum -- so that both CDFs are integer sums:
//     keys    (order-preserving uint32 of the coordinate) << 32 | set bit | q, one uint64 per live particle of BOTH sets in
//             LDS; a particle with q = 0 (its state row is not read) and every padding slot take the all-ones key; padded to
//             P = 2^k >= max(Ma + Mb, 64)
//     sort    the bitonic sort of pf_sort.h (its plan, slots and register stages; the body's text is here) for Ma + Mb slots:
//             a thread ends with its E = P / THREADS consecutive sorted slots in registers
//     scans   two integer scans in sorted order, one per set, selected by the set bit
//     gaps    one pass over the gaps between live neighbours: F_a - F_b from the two integer sums divided once in double,
//             max for ks, the block_sum order of pf_summary.h for the two sums
//   pairs   pf_distance_pairs_kernel<D, IPT, SCALED>, the plan of pf_scores.hip on a cross product, on its plain float
//           weights: cross(I-set, J-set) keeps the i-particles in registers and walks the J-set in tiles of 1024 through LDS
//           (structure-of-arrays, 16-byte broadcast reads, fp32 runs of 64 pairs flushed to double); instantiated for
//           (A, A), (A, B) -- one load of the A particles serves both -- and (B, B), each dealt by plan_of(M of its I-set).
//           Both plans one workgroup: one workgroup takes all three and writes the row.  Otherwise a launch per I-set writes
//           partial sums to the workspace and pf_distance_finish_kernel, a thread per row pair, adds them in order.  No atomics.

#include <cmath>

#include "pf_sort.h"

namespace {

namespace summary = mmf::summary;
namespace sort = mmf::sort;
using sort::u64;

// ================================================================================================ the CDF kernel
constexpr unsigned kSetB = 0x80000000u;   // the set bit: below the key, above q <= 2^24
constexpr unsigned kQMask = 0x01FFFFFFu;

struct CArgs {
  const float *states_a, *log_a_a, *log_b_a;  // (R, Ma, d), (R, Ma) or null
  const float *states_b, *log_a_b, *log_b_b;  // (R, Mb, d), (R, Mb) or null
  float *wasserstein, *cramer, *ks;           // (R, d) each, or null
  int Ma, Mb, d;
};

template <int THREADS, int E>
__global__ __launch_bounds__(THREADS) void pf_distance_cdf_kernel(CArgs a) {
  extern __shared__ u64 lds[];
  __shared__ u64 wave_tot[sort::kMaxWaves];
  __shared__ float wave_top[2][sort::kMaxWaves];
  __shared__ double wave_sum[sort::kMaxWaves][2];
  constexpr int kWaves = THREADS / MMF_WAVE;
  const int tid = threadIdx.x, Ma = a.Ma, M = a.Ma + a.Mb, d = a.d;
  const int r = blockIdx.x / d, k = blockIdx.x - r * d;
  const size_t row_a = static_cast<size_t>(r) * Ma, row_b = static_cast<size_t>(r) * a.Mb;
  const float *xa = a.states_a + row_a * d + k, *xb = a.states_b + row_b * d + k;
  const float *laa = a.log_a_a ? a.log_a_a + row_a : nullptr, *lba = a.log_b_a ? a.log_b_a + row_a : nullptr;
  const float *lab = a.log_a_b ? a.log_a_b + row_b : nullptr, *lbb = a.log_b_b ? a.log_b_b + row_b : nullptr;

  // slot m = tid + u THREADS: particle m of set A below Ma, particle m - Ma of set B below M; each set's own maximum
  float av[E];
  float top_a = -INFINITY, top_b = -INFINITY;
#pragma unroll
  for (int u = 0; u < E; ++u) {
    const int m = tid + u * THREADS;
    av[u] = -INFINITY;
    if (m < Ma) {
      av[u] = summary::log_weight(laa, lba, m);
      top_a = fmaxf(top_a, av[u]);  // (a NaN is skipped)
    } else if (m < M) {
      av[u] = summary::log_weight(lab, lbb, m - Ma);
      top_b = fmaxf(top_b, av[u]);
    }
  }
  top_a = summary::block_max(top_a, wave_top[0], tid, kWaves);
  top_b = summary::block_max(top_b, wave_top[1], tid, kWaves);

#pragma unroll
  for (int u = 0; u < E; ++u) {
    const int m = tid + u * THREADS;
    u64 packed = sort::kPadKey;
    if (m < M) {
      const bool in_a = m < Ma;
      const unsigned q = sort::fixed_weight(av[u] - (in_a ? top_a : top_b));
      if (q > 0u) {  // (a dead particle's state row is not read)
        const float xv = in_a ? xa[static_cast<size_t>(m) * d] : xb[static_cast<size_t>(m - Ma) * d];
        packed = (static_cast<u64>(sort::key_of(xv)) << 32) | (in_a ? 0u : kSetB) | q;
      }
    }
    lds[sort::slot<E>(m)] = packed;
  }

  // ---- bitonic sort, ascending (pf_sort.h: one textual copy here and in pf_quantiles.hip)
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

  // ---- the two integer CDFs in sorted order: this thread's run covers (excl, excl + mine] of each
  u64 mine_a = 0, mine_b = 0;
#pragma unroll
  for (int l = 0; l < E; ++l) {
    const unsigned lo = static_cast<unsigned>(v[l]);
    const u64 q = lo & kQMask;
    mine_a += (lo & kSetB) ? 0ull : q;
    mine_b += (lo & kSetB) ? q : 0ull;
  }
  u64 Qa, Qb;
  u64 ca = sort::block_scan<THREADS>(mine_a, wave_tot, tid, Qa) - mine_a;
  u64 cb = sort::block_scan<THREADS>(mine_b, wave_tot, tid, Qb) - mine_b;  // (its closing barrier: every thread has its run)

  // ---- the slot after this thread's run
  lds[tid] = v[0];
  __syncthreads();
  const u64 after = tid + 1 < THREADS ? lds[tid + 1] : sort::kPadKey;

  const size_t out = static_cast<size_t>(r) * d + k;
  if (Qa == 0 || Qb == 0) {  // a set without a live particle
    if (tid == 0) {
      if (a.wasserstein) a.wasserstein[out] = NAN;
      if (a.cramer) a.cramer[out] = NAN;
      if (a.ks) a.ks[out] = NAN;
    }
    return;
  }

  // ---- the gaps between live neighbours
  const double qa = static_cast<double>(Qa), qb = static_cast<double>(Qb);
  double s[2] = {0.0, 0.0};
  double worst = 0.0;
#pragma unroll
  for (int l = 0; l < E; ++l) {
    const u64 cur = v[l], nxt = l + 1 < E ? v[l + 1 < E ? l + 1 : l] : after;
    const unsigned lo = static_cast<unsigned>(cur);
    const u64 q = lo & kQMask;
    ca += (lo & kSetB) ? 0ull : q;
    cb += (lo & kSetB) ? q : 0ull;
    const unsigned key = static_cast<unsigned>(cur >> 32), key_next = static_cast<unsigned>(nxt >> 32);
    if (key != 0xFFFFFFFFu && key_next != 0xFFFFFFFFu) {
      const double gap = static_cast<double>(sort::value_of(key_next)) - static_cast<double>(sort::value_of(key));
      const double delta = static_cast<double>(ca) / qa - static_cast<double>(cb) / qb;
      const double ad = fabs(delta);
      s[0] += gap * ad;
      s[1] += gap * (delta * delta);
      if (gap > 0.0) worst = fmax(worst, ad);  // (the end of a tie group)
    }
  }
  summary::block_sum<2>(s, wave_sum, tid, kWaves);
  // (rounding to float is monotone: the maximum of the rounded values is the rounded maximum)
  const float top = summary::block_max(static_cast<float>(worst), wave_top[0], tid, kWaves);
  if (tid == 0) {
    if (a.wasserstein) a.wasserstein[out] = static_cast<float>(s[0]);
    if (a.cramer) a.cramer[out] = static_cast<float>(s[1]);
    if (a.ks) a.ks[out] = top;
  }
}

int launch_cdf(const CArgs& k, int R, hipStream_t s) {
  const unsigned grid = static_cast<unsigned>(R) * static_cast<unsigned>(k.d);
  const sort::Plan p = sort::plan_of(k.Ma + k.Mb);
  return sort::with_plan(p, [&](auto T, auto E) {
    constexpr int kT = decltype(T)::value, kE = decltype(E)::value;
    return mmf::launch(pf_distance_cdf_kernel<kT, kE>, grid, kT, sort::slots_of(p) * sizeof(u64), s, k);
  });
}

// ================================================================================================ the pair kernel
using summary::kIBlock;
using summary::kJTile;
using summary::kMaxWaves;
using summary::kRun;
using summary::Plan;

constexpr int kSums = 3;  // the stride of a workspace entry.  I = A: sum AA, sum AB, sum w_a;  I = B: sum BB, sum w_b, unused

// one weighted particle set of the row pair, its row offset applied
struct Set {
  const float *states, *log_a, *log_b;
  int M;
};

struct PArgs {
  Set a, b;       // row 0 of each
  float* energy;  // (R) or null
  float* terms;   // (R, 3) or null
  double* ws;     // (R, nb_a + nb_b, kSums) unless both plans are one workgroup
  int nb_a, chunk_a, nb_b, chunk_b;
  float inv_scale[MMF_MAX_STATE_DIM];
};
enum Mode { kWholeRow = 0, kFromA = 1, kFromB = 2 };

__device__ __forceinline__ Set row_of(const Set& s, int r, int d) {
  const size_t row = static_cast<size_t>(r) * s.M;
  return {s.states + row * d, s.log_a ? s.log_a + row : nullptr, s.log_b ? s.log_b + row : nullptr, s.M};
}

// the row maximum of a_m = log_a[m] + log_b[m]
__device__ __forceinline__ float top_of(const Set& s, float* scratch, int tid, int threads) {
  float top = -INFINITY;
  for (int m = tid; m < s.M; m += threads) top = fmaxf(top, summary::log_weight(s.log_a, s.log_b, m));  // (a NaN is skipped)
  return summary::block_max(top, scratch, tid, threads / MMF_WAVE);
}

// this thread's i-particles of the chunk [i0, i1) of a set; a dead one is held as zeros
template <int D, int IPT>
__device__ __forceinline__ void load_i(const Set& s, float top, int i0, int i1, int tid, int threads, float (&xi)[IPT][D],
                                       float (&wi)[IPT]) {
#pragma unroll
  for (int u = 0; u < IPT; ++u) {
    const int i = i0 + tid + u * threads;
    wi[u] = i < i1 ? summary::live_weight(summary::log_weight(s.log_a, s.log_b, i) - top) : 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) xi[u][k] = wi[u] > 0.f ? s.states[static_cast<size_t>(i) * D + k] : 0.f;
  }
}

// sum_i w_i sum_j w_j |(x_i - x_j) / s| over this thread's i-particles and the whole J-set: the one pair loop
template <int D, int IPT, bool SCALED>
__device__ __forceinline__ double cross(const float (&xi)[IPT][D], const float (&wi)[IPT], const Set& J, float top_j,
                                        const float* inv_scale, float* tile, int tid, int threads) {
  double pair[IPT];
#pragma unroll
  for (int u = 0; u < IPT; ++u) pair[u] = 0.0;
  for (int j0 = 0; j0 < J.M; j0 += kJTile) {
    const int n = min(kJTile, J.M - j0), npad = (n + kRun - 1) / kRun * kRun;
    __syncthreads();  // the tile before this one has been read
    for (int j = tid; j < npad; j += threads) {
      const float w = j < n ? summary::live_weight(summary::log_weight(J.log_a, J.log_b, j0 + j) - top_j) : 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) tile[k * kJTile + j] = w > 0.f ? J.states[static_cast<size_t>(j0 + j) * D + k] : 0.f;
      tile[D * kJTile + j] = w;
    }
    __syncthreads();
    for (int jr = 0; jr < npad; jr += kRun) {
      float acc[IPT];
#pragma unroll
      for (int u = 0; u < IPT; ++u) acc[u] = 0.f;
#pragma unroll 4
      for (int q = 0; q < kRun; q += 4) {
        float4 xj[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xj[k] = *reinterpret_cast<const float4*>(&tile[k * kJTile + jr + q]);
        const float4 wj = *reinterpret_cast<const float4*>(&tile[D * kJTile + jr + q]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float w = summary::pick(wj, c);
#pragma unroll
          for (int u = 0; u < IPT; ++u) {
            float n2 = 0.f, first = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
              const float e = xi[u][k] - summary::pick(xj[k], c);
              const float z = SCALED ? e * inv_scale[k] : e;
              if (k == 0) first = z;
              n2 = fmaf(z, z, n2);
            }
            const float norm = D == 1 ? fabsf(first) : __builtin_amdgcn_sqrtf(n2);
            acc[u] = fmaf(w, norm, acc[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < IPT; ++u) pair[u] += static_cast<double>(acc[u]);
    }
  }
  double v = 0.0;
#pragma unroll
  for (int u = 0; u < IPT; ++u)
    if (wi[u] > 0.f) v += static_cast<double>(wi[u]) * pair[u];  // (selected away, not multiplied by 0)
  return v;
}

template <int IPT>
__device__ __forceinline__ double weight_sum(const float (&wi)[IPT]) {
  double v = 0.0;
#pragma unroll
  for (int u = 0; u < IPT; ++u)
    if (wi[u] > 0.f) v += static_cast<double>(wi[u]);
  return v;
}

// sums: sum AA, sum AB, sum w_a, sum BB, sum w_b
__device__ __forceinline__ void write_row(const PArgs& a, int r, const double* sums) {
  const double Sa = sums[2], Sb = sums[4];
  const bool dead = !(Sa > 0.0) || !(Sb > 0.0);  // a set without a live particle
  const double t0 = sums[1] / (Sa * Sb), t1 = sums[0] / (Sa * Sa), t2 = sums[3] / (Sb * Sb);
  if (a.terms) {
    float* t = a.terms + static_cast<size_t>(r) * 3;
    t[0] = dead ? NAN : static_cast<float>(t0);
    t[1] = dead ? NAN : static_cast<float>(t1);
    t[2] = dead ? NAN : static_cast<float>(t2);
  }
  if (a.energy) {
    const double e2 = (2.0 * t0 - t1) - t2;
    a.energy[r] = dead ? NAN : static_cast<float>(sqrt(e2 > 0.0 ? e2 : 0.0));
  }
}

template <int D, int IPT, bool SCALED>
__global__ __launch_bounds__(kIBlock / IPT) void pf_distance_pairs_kernel(PArgs a, int mode) {
  __shared__ __attribute__((aligned(16))) float tile[(D + 1) * kJTile];
  __shared__ double wave_sum[kMaxWaves][kSums];
  __shared__ double row_sum[2 * kSums];
  __shared__ float wave_top[2][kMaxWaves];
  const int tid = threadIdx.x, threads = blockDim.x;
  const int nb = mode == kFromB ? a.nb_b : mode == kFromA ? a.nb_a : 1;
  const int r = blockIdx.x / nb, b = blockIdx.x - r * nb;
  const Set A = row_of(a.a, r, D), B = row_of(a.b, r, D);
  const float top_a = top_of(A, wave_top[0], tid, threads), top_b = top_of(B, wave_top[1], tid, threads);
  float xi[IPT][D], wi[IPT];
  double v[kSums];

  if (mode != kFromB) {  // I = A: (A, A) and (A, B) on one load of the i-particles
    const int i0 = b * a.chunk_a;
    load_i<D, IPT>(A, top_a, i0, min(A.M, i0 + a.chunk_a), tid, threads, xi, wi);
    v[0] = cross<D, IPT, SCALED>(xi, wi, A, top_a, a.inv_scale, tile, tid, threads);
    v[1] = cross<D, IPT, SCALED>(xi, wi, B, top_b, a.inv_scale, tile, tid, threads);
    v[2] = weight_sum(wi);
    summary::block_sum<kSums>(v, wave_sum, tid, threads / MMF_WAVE);
    if (tid < kSums) {
      if (mode == kFromA) a.ws[(static_cast<size_t>(r) * (a.nb_a + a.nb_b) + b) * kSums + tid] = v[tid];
      row_sum[tid] = v[tid];
    }
  }
  if (mode != kFromA) {  // I = B: (B, B)
    const int i0 = b * a.chunk_b;
    load_i<D, IPT>(B, top_b, i0, min(B.M, i0 + a.chunk_b), tid, threads, xi, wi);
    v[0] = cross<D, IPT, SCALED>(xi, wi, B, top_b, a.inv_scale, tile, tid, threads);
    v[1] = weight_sum(wi);
    v[2] = 0.0;
    summary::block_sum<kSums>(v, wave_sum, tid, threads / MMF_WAVE);
    if (tid < kSums) {
      if (mode == kFromB) a.ws[(static_cast<size_t>(r) * (a.nb_a + a.nb_b) + a.nb_a + b) * kSums + tid] = v[tid];
      row_sum[kSums + tid] = v[tid];
    }
  }
  if (mode != kWholeRow) return;
  __syncthreads();
  if (tid == 0) write_row(a, r, row_sum);
}

__global__ __launch_bounds__(MMF_WAVE) void pf_distance_finish_kernel(PArgs a, int R) {
  const int r = blockIdx.x * MMF_WAVE + threadIdx.x;
  if (r >= R) return;
  const double* ws = a.ws + static_cast<size_t>(r) * (a.nb_a + a.nb_b) * kSums;
  double sums[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int b = 0; b < a.nb_a; ++b)
    for (int k = 0; k < 3; ++k) sums[k] += ws[b * kSums + k];
  for (int b = 0; b < a.nb_b; ++b)
    for (int k = 0; k < 2; ++k) sums[3 + k] += ws[(a.nb_a + b) * kSums + k];
  write_row(a, r, sums);
}

template <int D, int IPT, bool SCALED>
int run_pairs(const PArgs& k, int mode, unsigned grid, int threads, hipStream_t s) {
  pf_distance_pairs_kernel<D, IPT, SCALED><<<grid, threads, 0, s>>>(k, mode);
  MMF_CHECK_LAUNCH();
  return 0;
}

int launch_pairs(const PArgs& k, int d, bool scaled, int mode, unsigned grid, int ipt, int threads, hipStream_t s) {
  return mmf::with_state_dim(d, [&](auto D) {
    return mmf::with_bool(scaled, [&](auto S) {
      constexpr int kD = decltype(D)::value;
      constexpr bool kS = decltype(S)::value;
      return ipt == 1 ? run_pairs<kD, 1, kS>(k, mode, grid, threads, s) : run_pairs<kD, 2, kS>(k, mode, grid, threads, s);
    });
  });
}

inline int clamp_m(int M) { return M < 1 ? 1 : M > summary::kMaxM ? summary::kMaxM : M; }

}  // namespace

extern "C" size_t mmf_pf_distance_lds_bytes(int Ma, int Mb) {
  if (Ma < 1 || Mb < 1) return 0;
  const long long M = static_cast<long long>(Ma) + Mb;
  return sort::slots_of(sort::plan_of(M > summary::kMaxM ? summary::kMaxM : static_cast<int>(M))) * sizeof(u64);
}

extern "C" size_t mmf_pf_distance_workspace_bytes(int R, int Ma, int Mb, int d) {
  if (R < 1 || Ma < 1 || Mb < 1 || d < 1) return 0;
  const Plan pa = summary::plan_of(clamp_m(Ma)), pb = summary::plan_of(clamp_m(Mb));
  if (pa.nb == 1 && pb.nb == 1) return 0;
  return static_cast<size_t>(R) * (pa.nb + pb.nb) * kSums * sizeof(double);
}

extern "C" int mmf_pf_distance(const MmfPfDistanceArgs* a, void* stream) {
  if (!a || summary::check_rows(a->states_a, a->R, a->Ma, a->d) || summary::check_rows(a->states_b, a->R, a->Mb, a->d))
    return MMF_EINVAL;
  if (summary::check_scale(a->scale, a->d)) return MMF_EINVAL;
  const bool want_cdf = a->wasserstein || a->cramer || a->ks, want_pairs = a->energy || a->terms;
  if (!want_cdf && !want_pairs) return MMF_EINVAL;
  if (static_cast<long long>(a->Ma) + a->Mb > summary::kMaxM) return MMF_ETOOLARGE;  // one limit: the union sort's
  const Plan pa = summary::plan_of(a->Ma), pb = summary::plan_of(a->Mb);
  int per_row = a->d;  // the largest grid of the entry: d workgroups to a row pair, or a plan's nb
  if (pa.nb > per_row) per_row = pa.nb;
  if (pb.nb > per_row) per_row = pb.nb;
  if (const int rc = summary::check_size(a->R, a->Ma + a->Mb, per_row)) return rc;
  const size_t ws_bytes = want_pairs ? mmf_pf_distance_workspace_bytes(a->R, a->Ma, a->Mb, a->d) : 0;
  if (!summary::workspace_ok(a->workspace, a->workspace_bytes, ws_bytes, alignof(double))) return MMF_EINVAL;
  {
    const size_t R = a->R, Ma = a->Ma, Mb = a->Mb, d = a->d, f = sizeof(float);
    const void* outs[6] = {a->wasserstein, a->cramer, a->ks, a->energy, a->terms, ws_bytes > 0 ? a->workspace : nullptr};
    const size_t out_bytes[6] = {R * d * f, R * d * f, R * d * f, R * f, R * 3 * f, ws_bytes};
    const void* ins[6] = {a->states_a, a->log_a_a, a->log_b_a, a->states_b, a->log_a_b, a->log_b_b};
    const size_t in_bytes[6] = {R * Ma * d * f, R * Ma * f, R * Ma * f, R * Mb * d * f, R * Mb * f, R * Mb * f};
    if (mmf_outputs_overlap(outs, out_bytes, 6, ins, in_bytes, 6)) return MMF_EINVAL;
  }
  if (a->R == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (want_cdf) {
    CArgs k{};
    k.states_a = a->states_a; k.log_a_a = a->log_a_a; k.log_b_a = a->log_b_a;
    k.states_b = a->states_b; k.log_a_b = a->log_a_b; k.log_b_b = a->log_b_b;
    k.wasserstein = a->wasserstein; k.cramer = a->cramer; k.ks = a->ks;
    k.Ma = a->Ma; k.Mb = a->Mb; k.d = a->d;
    if (const int rc = launch_cdf(k, a->R, s)) return rc;
  }
  if (!want_pairs) return 0;
  PArgs k{};
  k.a = {a->states_a, a->log_a_a, a->log_b_a, a->Ma};
  k.b = {a->states_b, a->log_a_b, a->log_b_b, a->Mb};
  k.energy = a->energy; k.terms = a->terms;
  k.ws = ws_bytes > 0 ? static_cast<double*>(a->workspace) : nullptr;
  k.nb_a = pa.nb; k.chunk_a = pa.chunk; k.nb_b = pb.nb; k.chunk_b = pb.chunk;
  const bool scaled = summary::inv_scale_of(a->scale, a->d, k.inv_scale);
  const unsigned R = static_cast<unsigned>(a->R);
  if (pa.nb == 1 && pb.nb == 1)  // one workgroup takes the row pair: the threads of the larger plan, one i-particle each
    return launch_pairs(k, a->d, scaled, kWholeRow, R, 1, pa.threads > pb.threads ? pa.threads : pb.threads, s);
  if (const int rc = launch_pairs(k, a->d, scaled, kFromA, R * pa.nb, pa.ipt, pa.threads, s)) return rc;
  if (const int rc = launch_pairs(k, a->d, scaled, kFromB, R * pb.nb, pb.ipt, pb.threads, s)) return rc;
  pf_distance_finish_kernel<<<(a->R + MMF_WAVE - 1) / MMF_WAVE, MMF_WAVE, 0, s>>>(k, a->R);
  MMF_CHECK_LAUNCH();
  return 0;
}
