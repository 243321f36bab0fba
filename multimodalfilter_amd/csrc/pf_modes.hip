// Modes of a weighted particle set by quick shift (include/mmf.h, "Particle-posterior modes"): every particle links to its
// nearest neighbour of higher density within a radius, over all M^2 pairs of a row; the roots of the forest are the modes and
// a tree's weight is the mode's mass.  The plain float live weights of pf_summary.h; the links, the labels, the count and the
// ranking are integers, the masses integer sums, the means sums of doubles in one fixed order.
//   plan      the dealing of pf_summary.h: nb workgroups to a row, IPT i-particles of a thread in registers
//   link      j-tiles of 1024 particles through LDS as structure-of-arrays: d planes of x as it is and one of the level l =
//             log_density, NaN for a particle that does not take part (a NaN compares false both ways: it is above nothing
//             and nothing is above it; its coordinates are staged as 0); four j per broadcast ds_read_b128.  Per pair d
//             times (subtract, multiply by 1 / h, fma) -- the difference first, so a set far from the origin partitions as
//             the same set at the origin --, the order test, the radius test and a strict < against the running best: j
//             ascends, so the first of equal distances stays.  Every i writes its own parent
//   finish    one workgroup of 512 to a row, everything in dynamic LDS: the links (a root points at itself, a dead particle
//             at -1), ceil(log2 M) double-buffered rounds of pointer jumping, q_m = floor(w_m 2^40) added into the roots with
//             64-bit integer atomics -- in LDS up to kLdsMassM particles, in the workspace beyond --, K arg-max reductions on
//             (Q_root, -root), each strictly below the one before, and per reported mode the d sums of q_m x_m in double
//             through summary::block_sum

#include <climits>
#include <cmath>

#include "pf_summary.h"

namespace {

using namespace mmf::summary;  // the dealing, the weights, block_max, block_sum, pick and the host's checks

constexpr int kMaxModes = MMF_PF_MODES_MAX;
constexpr int kLdsMassM = MMF_PF_MODES_LDS_MASS_M;  // up to here the masses sit in LDS beside the two label buffers
constexpr int kFinishThreads = kIBlock;             // kMaxWaves waves: the scratch of block_sum
constexpr float kMassScale = 1099511627776.0f;      // 2^40: w <= 1 times it is exact in fp32
typedef unsigned long long u64;

struct MArgs {
  const float* states;       // (R, M, d)
  const float* log_a;        // (R, M) or null
  const float* log_b;        // (R, M) or null
  const float* log_density;  // (R, M)
  const float* bandwidth;    // (R, d)
  int* parent;               // (R, M): the caller's, or the workspace's when the caller has none
  int* labels;               // (R, M) or null
  int* count;                // (R) or null
  int* index;                // (R, K) or null
  float* modes;              // (R, K, d) or null
  float* mass;               // (R, K) or null
  float* mean;               // (R, K, d) or null
  u64* ws_mass;              // (R, M) for M > kLdsMassM
  int M, nb, chunk, K;
  float tau2;
};

// the level of the particle at `at`: its log density where it takes part, else NaN
__device__ __forceinline__ float level_of(const MArgs& a, size_t at, float top) {
  const float w = live_weight(log_weight(a.log_a, a.log_b, at) - top);
  return w > 0.f ? a.log_density[at] : NAN;
}

// q_m of the particle at `at` where it takes part, else 0; *part: does it?
__device__ __forceinline__ u64 mass_of(const MArgs& a, size_t at, float top, bool* part) {
  const float w = live_weight(log_weight(a.log_a, a.log_b, at) - top);
  const float l = a.log_density[at];
  *part = w > 0.f && l == l;
  return *part ? static_cast<u64>(w * kMassScale) : 0ull;
}

__device__ __forceinline__ float row_top(const MArgs& a, size_t row, float* scratch, int tid, int threads, int waves) {
  float top = -INFINITY;
  for (int m = tid; m < a.M; m += threads) top = fmaxf(top, log_weight(a.log_a, a.log_b, row + m));  // (a NaN is skipped)
  return block_max(top, scratch, tid, waves);
}

template <int D, int IPT>
__global__ __launch_bounds__(kIBlock / IPT) void pf_modes_link_kernel(MArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[(D + 1) * kJTile];
  __shared__ float wave_f[kMaxWaves];
  const int tid = threadIdx.x, threads = blockDim.x, M = a.M, waves = threads / MMF_WAVE;
  const int r = blockIdx.x / a.nb, b = blockIdx.x - r * a.nb;
  const size_t row = static_cast<size_t>(r) * M;
  const float top = row_top(a, row, wave_f, tid, threads, waves);
  float ih[D];
#pragma unroll
  for (int k = 0; k < D; ++k) ih[k] = 1.0f / a.bandwidth[static_cast<size_t>(r) * D + k];

  // ---- this thread's i-particles
  const int i0 = b * a.chunk, i1 = min(M, i0 + a.chunk);
  float xi[IPT][D], li[IPT], best[IPT];
  int bj[IPT];
#pragma unroll
  for (int u = 0; u < IPT; ++u) {
    const int i = i0 + tid + u * threads;
    li[u] = i < i1 ? level_of(a, row + i, top) : NAN;
#pragma unroll
    for (int k = 0; k < D; ++k) xi[u][k] = li[u] == li[u] ? a.states[(row + i) * D + k] : 0.f;
    best[u] = INFINITY;
    bj[u] = -1;
  }

  // ---- pairs: the nearest j above i within the radius
  for (int j0 = 0; j0 < M; j0 += kJTile) {
    const int n = min(kJTile, M - j0), npad = (n + 3) & ~3;
    __syncthreads();  // the tile before this one has been read
    for (int j = tid; j < npad; j += threads) {
      const float l = j < n ? level_of(a, row + j0 + j, top) : NAN;
#pragma unroll
      for (int k = 0; k < D; ++k) tile[k * kJTile + j] = l == l ? a.states[(row + j0 + j) * D + k] : 0.f;
      tile[D * kJTile + j] = l;
    }
    __syncthreads();
#pragma unroll 2
    for (int q = 0; q < npad; q += 4) {
      float4 xj[D];
#pragma unroll
      for (int k = 0; k < D; ++k) xj[k] = *reinterpret_cast<const float4*>(&tile[k * kJTile + q]);
      const float4 lj = *reinterpret_cast<const float4*>(&tile[D * kJTile + q]);
#pragma unroll
      for (int u = 0; u < IPT; ++u) {
        const int i = i0 + tid + u * threads;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          float z = 0.f;
#pragma unroll
          for (int k = 0; k < D; ++k) {
            const float t = (xi[u][k] - pick(xj[k], c)) * ih[k];
            z = fmaf(t, t, z);
          }
          const float l = pick(lj, c);
          const int j = j0 + q + c;
          // (bitwise, not short-circuit: compares and selects, no branch per pair)
          const bool above = (l > li[u]) | ((l == li[u]) & (j < i));
          const bool take = above & (z <= a.tau2) & (z < best[u]);
          best[u] = take ? z : best[u];
          bj[u] = take ? j : bj[u];
        }
      }
    }
  }
#pragma unroll
  for (int u = 0; u < IPT; ++u) {
    const int i = i0 + tid + u * threads;
    if (i < i1) a.parent[row + i] = bj[u];
  }
}

struct FinishScratch {  // the head of the finish kernel's dynamic LDS; a multiple of 16 bytes
  double sums[kMaxWaves][MMF_MAX_STATE_DIM];
  u64 q[kMaxWaves];
  int i[kMaxWaves];
  float f[kMaxWaves];
};
static_assert(sizeof(FinishScratch) % 16 == 0, "the label buffers behind it are read as they are laid out");

inline size_t finish_lds_bytes(int M) {
  const size_t mpad = (static_cast<size_t>(M) + 3) & ~static_cast<size_t>(3);
  return sizeof(FinishScratch) + 2 * mpad * sizeof(int) + (M <= kLdsMassM ? static_cast<size_t>(M) * sizeof(u64) : 0);
}

// the sum of v over the workgroup, in every thread (integers: exact in any order)
__device__ __forceinline__ u64 block_sum_u64(u64 v, FinishScratch* s, int tid) {
#pragma unroll
  for (int off = 1; off < MMF_WAVE; off <<= 1) v += __shfl_xor(v, off, MMF_WAVE);
  __syncthreads();  // the scratch's last readers are done
  if ((tid & (MMF_WAVE - 1)) == 0) s->q[tid / MMF_WAVE] = v;
  __syncthreads();
  v = s->q[0];
  for (int w = 1; w < kMaxWaves; ++w) v += s->q[w];
  return v;
}

// (Q, root) ranks above (bq, bi): the greater mass, the lower root among equals
__device__ __forceinline__ bool heavier(u64 q, int i, u64 bq, int bi) { return q > bq || (q == bq && i < bi); }

template <int D>
__global__ __launch_bounds__(kFinishThreads) void pf_modes_finish_kernel(MArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  FinishScratch* s = reinterpret_cast<FinishScratch*>(lds);
  const int tid = threadIdx.x, M = a.M, mpad = (M + 3) & ~3, K = a.K;
  constexpr int threads = kFinishThreads, waves = kMaxWaves;
  const int lane = tid & (MMF_WAVE - 1), wave = tid / MMF_WAVE;
  const int r = blockIdx.x;
  const size_t row = static_cast<size_t>(r) * M;
  int* cur = reinterpret_cast<int*>(lds + sizeof(FinishScratch));
  int* nxt = cur + mpad;
  const bool lds_mass = M <= kLdsMassM;
  u64* Q = lds_mass ? reinterpret_cast<u64*>(nxt + mpad) : a.ws_mass + row;
  const float top = row_top(a, row, s->f, tid, threads, waves);

  // ---- the links: a root points at itself, a dead particle at -1; the row's total mass and its number of roots
  u64 total = 0, roots = 0;
  for (int m = tid; m < M; m += threads) {
    bool part;
    total += mass_of(a, row + m, top, &part);
    const int p = a.parent[row + m];
    cur[m] = part ? (p < 0 ? m : p) : -1;
    roots += part && p < 0 ? 1u : 0u;
    Q[m] = 0ull;
  }
  total = block_sum_u64(total, s, tid);
  roots = block_sum_u64(roots, s, tid);
  const int count = static_cast<int>(roots);
  if (tid == 0 && a.count) a.count[r] = count;

  // ---- pointer jumping: after round k a link spans 2^k of the tree's own links, or ends at the root
  __syncthreads();
  for (int span = 1; span < M; span <<= 1) {
    for (int m = tid; m < M; m += threads) {
      const int v = cur[m];
      nxt[m] = v < 0 ? -1 : cur[v];
    }
    __syncthreads();
    int* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (a.labels)
    for (int m = tid; m < M; m += threads) a.labels[row + m] = cur[m];

  // ---- the masses of the roots: integer sums, so the order of the atomics cannot matter
  for (int m = tid; m < M; m += threads) {
    const int root = cur[m];
    if (root < 0) continue;
    bool part;
    const u64 q = mass_of(a, row + m, top, &part);
    if (q != 0ull) atomicAdd(&Q[root], q);
  }
  __syncthreads();
  if (!a.index && !a.modes && !a.mass && !a.mean) return;

  // ---- the K heaviest roots, one reduction each: rank c is the heaviest root strictly below rank c - 1
  u64 prev_q = 0;
  int prev_i = -1;
  for (int c = 0; c < K; ++c) {
    u64 bq = 0;
    int bi = INT_MAX;
    if (c < count) {  // (uniform over the workgroup)
      for (int m = tid; m < M; m += threads) {
        if (cur[m] != m) continue;
        const u64 q = __hip_atomic_load(&Q[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (c > 0 && !heavier(prev_q, prev_i, q, m)) continue;  // reported already
        if (bi == INT_MAX || heavier(q, m, bq, bi)) {
          bq = q;
          bi = m;
        }
      }
#pragma unroll
      for (int off = 1; off < MMF_WAVE; off <<= 1) {
        const u64 oq = __shfl_xor(bq, off, MMF_WAVE);
        const int oi = __shfl_xor(bi, off, MMF_WAVE);
        if (oi != INT_MAX && (bi == INT_MAX || heavier(oq, oi, bq, bi))) {
          bq = oq;
          bi = oi;
        }
      }
      __syncthreads();  // the scratch's last readers are done
      if (lane == 0) {
        s->q[wave] = bq;
        s->i[wave] = bi;
      }
      __syncthreads();
      bq = s->q[0];
      bi = s->i[0];
      for (int w = 1; w < waves; ++w)
        if (s->i[w] != INT_MAX && (bi == INT_MAX || heavier(s->q[w], s->i[w], bq, bi))) {
          bq = s->q[w];
          bi = s->i[w];
        }
    }
    const bool none = bi == INT_MAX;  // a rank beyond the count: -1 / NaN / 0 / NaN
    const size_t at = static_cast<size_t>(r) * K + c;
    if (tid == 0) {
      if (a.index) a.index[at] = none ? -1 : bi;
      if (a.mass) a.mass[at] = none || bq == 0ull ? 0.f : static_cast<float>(static_cast<double>(bq) / static_cast<double>(total));
      if (a.modes) {
        const unsigned* src = reinterpret_cast<const unsigned*>(a.states) + (row + (none ? 0 : bi)) * D;
        unsigned* dst = reinterpret_cast<unsigned*>(a.modes) + at * D;
        for (int k = 0; k < D; ++k) dst[k] = none ? 0x7fc00000u : src[k];  // a bit copy
      }
    }
    if (a.mean) {
      double v[D];
#pragma unroll
      for (int k = 0; k < D; ++k) v[k] = 0.0;
      if (!none) {  // (uniform over the workgroup)
        for (int m = tid; m < M; m += threads) {
          if (cur[m] != bi) continue;
          bool part;
          const double q = static_cast<double>(mass_of(a, row + m, top, &part));
#pragma unroll
          for (int k = 0; k < D; ++k) v[k] += q * static_cast<double>(a.states[(row + m) * D + k]);
        }
        block_sum<D>(v, s->sums, tid, waves);
      }
      if (tid == 0)
        for (int k = 0; k < D; ++k) a.mean[at * D + k] = none ? NAN : static_cast<float>(v[k] / static_cast<double>(bq));
    }
    prev_q = bq;
    prev_i = bi;
  }
}

template <int D, int IPT>
int run_link(const MArgs& k, unsigned grid, int threads, hipStream_t s) {
  pf_modes_link_kernel<D, IPT><<<grid, threads, 0, s>>>(k);
  MMF_CHECK_LAUNCH();
  return 0;
}

inline size_t link_ws_bytes(size_t R, size_t M) { return (R * M * sizeof(int32_t) + 7) & ~static_cast<size_t>(7); }
inline size_t mass_ws_bytes(size_t R, size_t M) { return M > static_cast<size_t>(kLdsMassM) ? R * M * sizeof(u64) : 0; }

}  // namespace

extern "C" size_t mmf_pf_modes_workspace_bytes(int R, int M, int d) {
  if (R < 1 || M < 1 || d < 1) return 0;
  return mass_ws_bytes(R, M) + link_ws_bytes(R, M);
}

extern "C" int mmf_pf_modes(const MmfPfModesArgs* a, void* stream) {
  if (!a || check_rows(a->states, a->R, a->M, a->d)) return MMF_EINVAL;
  if (!a->log_density || !a->bandwidth) return MMF_EINVAL;
  if (a->max_modes < 1 || a->max_modes > kMaxModes) return MMF_EINVAL;
  if (!(a->link_radius > 0.f && a->link_radius < INFINITY)) return MMF_EINVAL;  // (a NaN fails)
  if (!a->parent && !a->labels && !a->count && !a->index && !a->modes && !a->mass && !a->mean) return MMF_EINVAL;
  const Plan p = plan_of(a->M <= kMaxM ? a->M : kMaxM);  // (a larger M: check_size refuses it)
  if (const int rc = check_size(a->R, a->M, p.nb)) return rc;
  const size_t ws_bytes = mmf_pf_modes_workspace_bytes(a->R, a->M, a->d);
  if (!workspace_ok(a->workspace, a->workspace_bytes, ws_bytes, alignof(u64))) return MMF_EINVAL;
  {
    const size_t R = a->R, M = a->M, d = a->d, K = a->max_modes, f = sizeof(float), i = sizeof(int32_t);
    const void* outs[8] = {a->parent, a->labels, a->count, a->index, a->modes, a->mass, a->mean, a->workspace};
    const size_t out_bytes[8] = {R * M * i, R * M * i, R * i, R * K * i, R * K * d * f, R * K * f, R * K * d * f, ws_bytes};
    const void* ins[5] = {a->states, a->log_a, a->log_b, a->log_density, a->bandwidth};
    const size_t in_bytes[5] = {R * M * d * f, R * M * f, R * M * f, R * M * f, R * d * f};
    if (mmf_outputs_overlap(outs, out_bytes, 8, ins, in_bytes, 5)) return MMF_EINVAL;
  }
  if (a->R == 0) return 0;
  MArgs k{};
  k.states = a->states; k.log_a = a->log_a; k.log_b = a->log_b; k.log_density = a->log_density; k.bandwidth = a->bandwidth;
  unsigned char* ws = static_cast<unsigned char*>(a->workspace);
  const size_t mass_bytes = mass_ws_bytes(a->R, a->M);
  k.ws_mass = mass_bytes > 0 ? reinterpret_cast<u64*>(ws) : nullptr;
  k.parent = a->parent ? a->parent : reinterpret_cast<int*>(ws + mass_bytes);
  k.labels = a->labels; k.count = a->count; k.index = a->index; k.modes = a->modes; k.mass = a->mass; k.mean = a->mean;
  k.M = a->M; k.nb = p.nb; k.chunk = p.chunk; k.K = a->max_modes;
  k.tau2 = a->link_radius * a->link_radius;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(a->R) * static_cast<unsigned>(p.nb);
  const int rc = mmf::with_state_dim(a->d, [&](auto D) {
    constexpr int kD = decltype(D)::value;
    return p.ipt == 1 ? run_link<kD, 1>(k, grid, p.threads, s) : run_link<kD, 2>(k, grid, p.threads, s);
  });
  if (rc != 0 || !(a->labels || a->count || a->index || a->modes || a->mass || a->mean)) return rc;
  const size_t lds = finish_lds_bytes(a->M);
  return mmf::with_state_dim(a->d, [&](auto D) {
    return mmf::launch(pf_modes_finish_kernel<decltype(D)::value>, dim3(a->R), dim3(kFinishThreads), lds, s, k);
  });
}
