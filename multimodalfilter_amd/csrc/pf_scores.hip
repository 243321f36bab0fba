// CRPS per state dimension and the energy score of a weighted particle set against a true state, with their sharpness terms
// (include/mmf.h, "Particle-posterior scores"): E|X - y| - 1/2 E|X - X'|, the second expectation over all M^2 pairs of a row.
// Plain float weights w_m = exp(a_m - max a) -- nothing is selected, so K1's integer fixed point has nothing to protect --
// and every sum in a fixed order, the outer ones in double; normalised by sum w and (sum w)^2 once, at the end, in double.
//   plan      a row's particles are dealt to nb = ceil(M / 512) workgroups in equal i-chunks; a thread holds IPT i-particles
//             in registers: one, in up to 512 threads, while the row is one workgroup (M <= 512), two in up to 256 beyond
//   weights   every workgroup takes the row maximum itself (exact in any order) and forms the w it needs; a particle with
//             w = 0 is staged with a zero state row, so its NaNs never reach a sum
//   pairs     j-tiles of 1024 particles through LDS as structure-of-arrays (d coordinate planes and w): a thread reads four
//             j at a time with one ds_read_b128 per plane, every lane the same address (a broadcast); the d differences of
//             a pair feed the d |.| accumulators and the one norm.  fp32 accumulators over runs of 64 j, flushed to double
//   truth     sum_i w_i |x_i - y| and sum_i w_i |(x_i - y) / s| over the workgroup's own i-particles, in double
//   reduce    2 d + 3 doubles per thread: butterfly over the wave, the waves in order through LDS
//   finish    nb == 1: the workgroup writes the row's outputs.  nb > 1: it writes its sums to the workspace and
//             pf_scores_finish_kernel, a thread per row, adds the nb partial sums in order.  No atomics.

#include <cmath>

#include "mmf_launch.h"

namespace {

constexpr int kMaxM = 16384;
constexpr int kIBlock = 512;   // i-particles of a workgroup at most
constexpr int kJTile = 1024;   // j-particles of an LDS tile
constexpr int kRun = 64;       // pairs an fp32 accumulator takes before it is flushed to double
constexpr int kSums = 2 * MMF_MAX_STATE_DIM + 3;  // pair sums (d + 1), truth sums (d + 1), sum w: the stride of a workspace entry
constexpr int kMaxWaves = kIBlock / MMF_WAVE;

struct SArgs {
  const float* states;  // (R, M, d)
  const float* log_a;   // (R, M) or null
  const float* log_b;   // (R, M) or null
  const float* truth;   // (R, d) or null
  float* crps;          // (R, d) or null
  float* energy;        // (R) or null
  float* spread;        // (R, d + 1) or null
  double* ws;           // (R, nb, kSums) for nb > 1
  int M, d, nb, chunk;
  float inv_scale[MMF_MAX_STATE_DIM];
};

// how a row of M particles is dealt out; a function of M alone, so a row has the same bits whatever the batch
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

// sums[0 .. d]: sum_i sum_j w_i w_j |x_ik - x_jk|, the norm last; [d + 1 .. 2 d + 1]: sum_i w_i |x_ik - y_k|, the norm last;
// [2 d + 2]: sum w
__device__ __forceinline__ void write_row(const SArgs& a, int r, const double* sums) {
  const int d = a.d;
  const double S = sums[2 * d + 2];
  const bool dead = !(S > 0.0);  // no live particle in the row
  const double S2 = S * S;
  if (a.spread)
    for (int k = 0; k <= d; ++k) a.spread[static_cast<size_t>(r) * (d + 1) + k] = dead ? NAN : static_cast<float>(sums[k] / S2);
  if (a.crps)
    for (int k = 0; k < d; ++k)
      a.crps[static_cast<size_t>(r) * d + k] = dead ? NAN : static_cast<float>(sums[d + 1 + k] / S - 0.5 * (sums[k] / S2));
  if (a.energy) a.energy[r] = dead ? NAN : static_cast<float>(sums[2 * d + 1] / S - 0.5 * (sums[d] / S2));
}

__device__ __forceinline__ float weight_of(const SArgs& a, size_t at, float top) {
  const float la = a.log_a ? a.log_a[at] : 0.f, lb = a.log_b ? a.log_b[at] : 0.f;
  const float t = (la + lb) - top;
  return t <= 0.f ? expf(t) : 0.f;  // (a NaN t: 0)
}

template <int D, int IPT, bool SCALED>
__global__ __launch_bounds__(kIBlock / IPT) void pf_scores_kernel(SArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[(D + 1) * kJTile];
  __shared__ double wave_sum[kMaxWaves][2 * D + 3];
  __shared__ float wave_top[kMaxWaves];
  const int tid = threadIdx.x, threads = blockDim.x, M = a.M;
  const int lane = tid & (MMF_WAVE - 1), wave = tid / MMF_WAVE, waves = threads / MMF_WAVE;
  const int r = blockIdx.x / a.nb, b = blockIdx.x - r * a.nb;
  const size_t row = static_cast<size_t>(r) * M;

  // ---- the row maximum of a_m = log_a[m] + log_b[m]
  float top = -INFINITY;
  for (int m = tid; m < M; m += threads) {
    const float la = a.log_a ? a.log_a[row + m] : 0.f, lb = a.log_b ? a.log_b[row + m] : 0.f;
    top = fmaxf(top, la + lb);  // (a NaN is skipped)
  }
  top = mmf::wave_max(top);
  if (lane == 0) wave_top[wave] = top;
  __syncthreads();
  top = wave_top[0];
  for (int w = 1; w < waves; ++w) top = fmaxf(top, wave_top[w]);

  // ---- this thread's i-particles
  const int i0 = b * a.chunk, i1 = min(M, i0 + a.chunk);
  float xi[IPT][D], wi[IPT];
#pragma unroll
  for (int u = 0; u < IPT; ++u) {
    const int i = i0 + tid + u * threads;
    wi[u] = i < i1 ? weight_of(a, row + i, top) : 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) xi[u][k] = wi[u] > 0.f ? a.states[(row + i) * D + k] : 0.f;
  }

  // ---- pairs: pair[u][k] = sum_j w_j |x_ik - x_jk|, pair[u][D] = sum_j w_j |(x_i - x_j) / s|
  double pair[IPT][D + 1];
#pragma unroll
  for (int u = 0; u < IPT; ++u)
#pragma unroll
    for (int k = 0; k <= D; ++k) pair[u][k] = 0.0;
  for (int j0 = 0; j0 < M; j0 += kJTile) {
    const int n = min(kJTile, M - j0), npad = (n + kRun - 1) / kRun * kRun;
    __syncthreads();  // the tile before this one has been read
    for (int j = tid; j < npad; j += threads) {
      const float w = j < n ? weight_of(a, row + j0 + j, top) : 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) tile[k * kJTile + j] = w > 0.f ? a.states[(row + j0 + j) * D + k] : 0.f;
      tile[D * kJTile + j] = w;
    }
    __syncthreads();
    for (int jr = 0; jr < npad; jr += kRun) {
      float acc[IPT][D + 1];
#pragma unroll
      for (int u = 0; u < IPT; ++u)
#pragma unroll
        for (int k = 0; k <= D; ++k) acc[u][k] = 0.f;
#pragma unroll 4
      for (int q = 0; q < kRun; q += 4) {
        float4 xj[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xj[k] = *reinterpret_cast<const float4*>(&tile[k * kJTile + jr + q]);
        const float4 wj = *reinterpret_cast<const float4*>(&tile[D * kJTile + jr + q]);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const float w = c == 0 ? wj.x : c == 1 ? wj.y : c == 2 ? wj.z : wj.w;
#pragma unroll
          for (int u = 0; u < IPT; ++u) {
            float n2 = 0.f, first = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
              const float x = c == 0 ? xj[k].x : c == 1 ? xj[k].y : c == 2 ? xj[k].z : xj[k].w;
              const float e = xi[u][k] - x;
              acc[u][k] = fmaf(w, fabsf(e), acc[u][k]);
              const float z = SCALED ? e * a.inv_scale[k] : e;
              if (k == 0) first = z;
              n2 = fmaf(z, z, n2);
            }
            const float norm = D == 1 ? fabsf(first) : __builtin_amdgcn_sqrtf(n2);
            acc[u][D] = fmaf(w, norm, acc[u][D]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < IPT; ++u)
#pragma unroll
        for (int k = 0; k <= D; ++k) pair[u][k] += static_cast<double>(acc[u][k]);
    }
  }

  // ---- this thread's share of the 2 D + 3 sums
  double v[2 * D + 3];
#pragma unroll
  for (int k = 0; k < 2 * D + 3; ++k) v[k] = 0.0;
#pragma unroll
  for (int u = 0; u < IPT; ++u) {
    if (!(wi[u] > 0.f)) continue;  // (selected away, not multiplied by 0)
    const double w = static_cast<double>(wi[u]);
#pragma unroll
    for (int k = 0; k <= D; ++k) v[k] += w * pair[u][k];
    if (a.truth) {
      double n2 = 0.0;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double e = static_cast<double>(xi[u][k]) - static_cast<double>(a.truth[static_cast<size_t>(r) * D + k]);
        v[D + 1 + k] += w * fabs(e);
        const double z = e * static_cast<double>(a.inv_scale[k]);
        n2 += z * z;
      }
      v[2 * D + 1] += w * sqrt(n2);
    }
    v[2 * D + 2] += w;
  }

  // ---- over the workgroup: a butterfly in each wave, then the waves in order
#pragma unroll
  for (int k = 0; k < 2 * D + 3; ++k) {
    double s = v[k];
#pragma unroll
    for (int off = 1; off < MMF_WAVE; off <<= 1) s += __shfl_xor(s, off, MMF_WAVE);
    if (lane == 0) wave_sum[wave][k] = s;
  }
  __syncthreads();
  if (tid < 2 * D + 3) {
    double s = wave_sum[0][tid];
    for (int w = 1; w < waves; ++w) s += wave_sum[w][tid];
    if (a.nb > 1) a.ws[static_cast<size_t>(blockIdx.x) * kSums + tid] = s;
    wave_sum[0][tid] = s;
  }
  if (a.nb > 1) return;
  __syncthreads();
  if (tid == 0) write_row(a, r, wave_sum[0]);
}

__global__ __launch_bounds__(MMF_WAVE) void pf_scores_finish_kernel(SArgs a, int R) {
  const int r = blockIdx.x * MMF_WAVE + threadIdx.x;
  if (r >= R) return;
  double sums[kSums];
  const int q = 2 * a.d + 3;
  for (int k = 0; k < q; ++k) {
    double s = 0.0;
    for (int b = 0; b < a.nb; ++b) s += a.ws[(static_cast<size_t>(r) * a.nb + b) * kSums + k];
    sums[k] = s;
  }
  write_row(a, r, sums);
}

template <int D, int IPT, bool SCALED>
int run(const SArgs& k, unsigned grid, int threads, hipStream_t s) {
  pf_scores_kernel<D, IPT, SCALED><<<grid, threads, 0, s>>>(k);
  MMF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t mmf_pf_scores_workspace_bytes(int R, int M, int d) {
  if (R < 1 || M < 1 || d < 1) return 0;
  const Plan p = plan_of(M);
  return p.nb > 1 ? static_cast<size_t>(R) * p.nb * kSums * sizeof(double) : 0;
}

extern "C" int mmf_pf_scores(const MmfPfScoresArgs* a, void* stream) {
  if (!a || !a->states) return MMF_EINVAL;
  if (a->R < 0 || a->M < 1 || a->d < 1 || a->d > MMF_MAX_STATE_DIM) return MMF_EINVAL;
  for (int k = 0; k < a->d; ++k)
    if (!(a->scale[k] > 0.f && a->scale[k] < INFINITY)) return MMF_EINVAL;  // (a NaN fails)
  if (!a->crps && !a->energy && !a->spread) return MMF_EINVAL;
  if ((a->crps || a->energy) && !a->truth) return MMF_EINVAL;
  if (a->M > kMaxM) return MMF_ETOOLARGE;
  const Plan p = plan_of(a->M);
  if (static_cast<long long>(a->R) * p.nb > 0x7fffffffll) return MMF_ETOOLARGE;
  const size_t ws_bytes = mmf_pf_scores_workspace_bytes(a->R, a->M, a->d);
  if (ws_bytes > 0 && (!a->workspace || a->workspace_bytes < ws_bytes)) return MMF_EINVAL;
  if (ws_bytes > 0 && reinterpret_cast<uintptr_t>(a->workspace) % alignof(double) != 0) return MMF_EINVAL;
  {
    const size_t R = a->R, M = a->M, d = a->d, f = sizeof(float);
    const void* ins[4] = {a->states, a->log_a, a->log_b, a->truth};
    const size_t in_bytes[4] = {R * M * d * f, R * M * f, R * M * f, R * d * f};
    const void* outs[4] = {a->crps, a->energy, a->spread, a->workspace};
    const size_t out_bytes[4] = {R * d * f, R * f, R * (d + 1) * f, ws_bytes};
    for (int o = 0; o < 4; ++o) {
      for (int i = 0; i < 4; ++i)
        if (mmf_bytes_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) return MMF_EINVAL;
      for (int o2 = o + 1; o2 < 4; ++o2)
        if (mmf_bytes_overlap(outs[o], out_bytes[o], outs[o2], out_bytes[o2])) return MMF_EINVAL;
    }
  }
  if (a->R == 0) return 0;
  SArgs k{};
  k.states = a->states; k.log_a = a->log_a; k.log_b = a->log_b; k.truth = a->truth;
  k.crps = a->crps; k.energy = a->energy; k.spread = a->spread;
  k.ws = ws_bytes > 0 ? static_cast<double*>(a->workspace) : nullptr;
  k.M = a->M; k.d = a->d; k.nb = p.nb; k.chunk = p.chunk;
  bool scaled = false;
  for (int i = 0; i < MMF_MAX_STATE_DIM; ++i) {
    k.inv_scale[i] = i < a->d ? 1.0f / a->scale[i] : 1.0f;
    scaled = scaled || k.inv_scale[i] != 1.0f;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(a->R) * static_cast<unsigned>(p.nb);
  const int rc = mmf::with_state_dim(a->d, [&](auto D) {
    return mmf::with_bool(scaled, [&](auto S) {
      constexpr int kD = decltype(D)::value;
      constexpr bool kS = decltype(S)::value;
      return p.ipt == 1 ? run<kD, 1, kS>(k, grid, p.threads, s) : run<kD, 2, kS>(k, grid, p.threads, s);
    });
  });
  if (rc != 0 || p.nb == 1) return rc;
  pf_scores_finish_kernel<<<(a->R + MMF_WAVE - 1) / MMF_WAVE, MMF_WAVE, 0, s>>>(k, a->R);
  MMF_CHECK_LAUNCH();
  return 0;
}
