// CRPS per state dimension and the energy score of a weighted particle set against a true state, with their sharpness terms
// (include/mmf.h, "Particle-posterior scores"): E|X - y| - 1/2 E|X - X'|, the second expectation over all M^2 pairs of a row.
// The plain float live weights of pf_summary.h -- nothing is selected, so K1's integer fixed point has nothing to protect --
// and every sum in a fixed order, the outer ones in double; normalised by sum w and (sum w)^2 once, at the end, in double.
//   plan      the dealing of pf_summary.h: nb workgroups to a row, IPT i-particles of a thread in registers
//   weights   every workgroup takes the row maximum itself and forms the w it needs
//   pairs     j-tiles of 1024 particles through LDS as structure-of-arrays (d coordinate planes and w): a thread reads four
//             j at a time with one ds_read_b128 per plane, every lane the same address (a broadcast); the d differences of
//             a pair feed the d |.| accumulators and the one norm.  fp32 accumulators over runs of 64 j, flushed to double
//   truth     sum_i w_i |x_i - y| and sum_i w_i |(x_i - y) / s| over the workgroup's own i-particles, in double
//   reduce    2 d + 3 doubles per thread: summary::wave_sums, then thread k takes sum k of the waves
//   finish    nb == 1: the workgroup writes the row's outputs.  nb > 1: it writes its sums to the workspace and
//             pf_scores_finish_kernel, a thread per row, adds the nb partial sums in order.  No atomics.

#include <cmath>

#include "pf_summary.h"

namespace {

using namespace mmf::summary;  // the dealing, the weights, block_max, the ordered sums, pick and the host's checks

constexpr int kSums = 2 * MMF_MAX_STATE_DIM + 3;  // pair sums (d + 1), truth sums (d + 1), sum w: the stride of a workspace entry

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
  return live_weight(log_weight(a.log_a, a.log_b, at) - top);
}

template <int D, int IPT, bool SCALED>
__global__ __launch_bounds__(kIBlock / IPT) void pf_scores_kernel(SArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[(D + 1) * kJTile];
  __shared__ double wave_sum[kMaxWaves][2 * D + 3];
  __shared__ float wave_top[kMaxWaves];
  const int tid = threadIdx.x, threads = blockDim.x, M = a.M;
  const int r = blockIdx.x / a.nb, b = blockIdx.x - r * a.nb;
  const size_t row = static_cast<size_t>(r) * M;

  // ---- the row maximum of a_m = log_a[m] + log_b[m]
  float top = -INFINITY;
  for (int m = tid; m < M; m += threads) top = fmaxf(top, log_weight(a.log_a, a.log_b, row + m));  // (a NaN is skipped)
  top = block_max(top, wave_top, tid, threads / MMF_WAVE);

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
          const float w = pick(wj, c);
#pragma unroll
          for (int u = 0; u < IPT; ++u) {
            float n2 = 0.f, first = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
              const float e = xi[u][k] - pick(xj[k], c);
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

  // ---- over the workgroup: thread k takes sum k (block_sum's order; its totals in every thread measured 4 to 8 % slower at
  // 32 x 300 x 100)
  wave_sums<2 * D + 3>(v, wave_sum, tid);
  __syncthreads();
  if (tid < 2 * D + 3) {
    const double s = sum_of_waves(wave_sum, tid, threads / MMF_WAVE);
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
  if (!a || check_rows(a->states, a->R, a->M, a->d) || check_scale(a->scale, a->d)) return MMF_EINVAL;
  if (!a->crps && !a->energy && !a->spread) return MMF_EINVAL;
  if ((a->crps || a->energy) && !a->truth) return MMF_EINVAL;
  const Plan p = plan_of(a->M <= kMaxM ? a->M : kMaxM);  // (a larger M: check_size refuses it)
  if (const int rc = check_size(a->R, a->M, p.nb)) return rc;
  const size_t ws_bytes = mmf_pf_scores_workspace_bytes(a->R, a->M, a->d);
  if (!workspace_ok(a->workspace, a->workspace_bytes, ws_bytes, alignof(double))) return MMF_EINVAL;
  {
    const size_t R = a->R, M = a->M, d = a->d, f = sizeof(float);
    const void* outs[4] = {a->crps, a->energy, a->spread, a->workspace};
    const size_t out_bytes[4] = {R * d * f, R * f, R * (d + 1) * f, ws_bytes};
    if (outputs_alias(a->states, a->log_a, a->log_b, a->truth, R, M, d, outs, out_bytes)) return MMF_EINVAL;
  }
  if (a->R == 0) return 0;
  SArgs k{};
  k.states = a->states; k.log_a = a->log_a; k.log_b = a->log_b; k.truth = a->truth;
  k.crps = a->crps; k.energy = a->energy; k.spread = a->spread;
  k.ws = ws_bytes > 0 ? static_cast<double*>(a->workspace) : nullptr;
  k.M = a->M; k.d = a->d; k.nb = p.nb; k.chunk = p.chunk;
  const bool scaled = inv_scale_of(a->scale, a->d, k.inv_scale);
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
