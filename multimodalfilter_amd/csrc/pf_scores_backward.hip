// The gradients of CRPS per state dimension and of the energy score of a weighted particle set (include/mmf.h, "Training on
// the particle set's scores"): the reverse of pf_scores.hip, whose forward it leaves alone.  Per row, with the forward's own
// weights w (pf_summary.h), W = w / sum w, the upstream gradients g_k, g_E and s = scale:
//   c_m            = sum_k g_k (|x_mk - y_k| - sum_l W_l |x_mk - x_lk|) + g_E (|(x_m - y)/s| - sum_l W_l |(x_m - x_l)/s|)
//   g_logw[m]      = W_m (c_m - sum_l W_l c_l)
//   g_states[m, k] = W_m [g_k (sgn(x_mk - y_k) - sum_l W_l sgn(x_mk - x_lk)) + g_E (u_k(x_m - y) - sum_l W_l u_k(x_m - x_l))]
//   plan      the dealing of pf_summary.h: nb workgroups to a row, IPT i-particles of a thread in registers
//   weights   every workgroup takes the row maximum AND sum w over the whole row itself, in one fixed order, so that it can
//             normalise and write g_states without a second pass
//   pairs     j-tiles of 1024 particles through LDS as structure-of-arrays (d coordinate planes and w), four j per broadcast
//             ds_read_b128 and plane.  Per i-particle up to 3 d + 1 sums over j, w unnormalised: d of w |e_k| and d of
//             w sgn(e_k) (CRPS), one of w |z| and d of w z_k / |z| with z = e / s (ENERGY); one v_rsq_f32 per pair, a pair at
//             distance 0 selected away.  fp32 accumulators over runs of 64 j, flushed to double
//   finish    the truth terms and the division by sum w per i-particle in double.  g_states is written here.  nb == 1: the
//             workgroup sums W c and writes g_logw.  nb > 1: it writes c_m, W_m and its partial sum of W c to the workspace
//             and pf_scores_backward_finish_kernel, a thread per particle, adds the nb partial sums in order.  No atomics
//   variants  compiled per null upstream gradient: CRPS alone forms no norm, ENERGY alone no sign sums.  The outputs are not
//             specialised: a row's bits depend on neither of them being asked for

#include <cfloat>
#include <cmath>

#include "pf_summary.h"

namespace {

using namespace mmf::summary;  // the dealing, the weights, block_max, the ordered sums, pick and the host's checks

constexpr int kFinishThreads = 256;  // particles of a workgroup of the finishing kernel

struct BArgs {
  const float* states;    // (R, M, d)
  const float* log_a;     // (R, M) or null
  const float* log_b;     // (R, M) or null
  const float* truth;     // (R, d)
  const float* g_crps;    // (R, d) or null
  const float* g_energy;  // (R) or null
  float* g_states;        // (R, M, d) or null
  float* g_logw;          // (R, M) or null
  double* ws;             // (R, nb + 2 M) for nb > 1: a row's nb partial sums of W c, then c_m, then W_m
  int M, nb, chunk;
  float inv_scale[MMF_MAX_STATE_DIM];
};

__device__ __forceinline__ float weight_of(const BArgs& a, size_t at, float top) {
  return live_weight(log_weight(a.log_a, a.log_b, at) - top);
}

// a gradient as it is written: -0 (a dropped term's 0 * negative) as +0
__device__ __forceinline__ float written(double v) { return v == 0.0 ? 0.f : static_cast<float>(v); }

__device__ __forceinline__ size_t ws_row(const BArgs& a, int r) { return static_cast<size_t>(r) * (a.nb + 2 * static_cast<size_t>(a.M)); }

template <int D, int IPT, bool CRPS, bool ENERGY, bool SCALED>
__global__ __launch_bounds__(kIBlock / IPT) void pf_scores_backward_kernel(BArgs a) {
  constexpr int kE = CRPS ? 2 * D : 0;                 // the first ENERGY sum: the norm, then its d gradients
  constexpr int kAcc = kE + (ENERGY ? D + 1 : 0);      // pair sums of an i-particle
  __shared__ __attribute__((aligned(16))) float tile[(D + 1) * kJTile];
  __shared__ double wave_sum[kMaxWaves][1];
  __shared__ float wave_top[kMaxWaves];
  const int tid = threadIdx.x, threads = blockDim.x, M = a.M;
  const int r = blockIdx.x / a.nb, b = blockIdx.x - r * a.nb;
  const size_t row = static_cast<size_t>(r) * M;

  // ---- the row maximum of a_m = log_a[m] + log_b[m], and sum w over the whole row (the same bits in every workgroup of it)
  float top = -INFINITY;
  for (int m = tid; m < M; m += threads) top = fmaxf(top, log_weight(a.log_a, a.log_b, row + m));  // (a NaN is skipped)
  top = block_max(top, wave_top, tid, threads / MMF_WAVE);
  double total[1] = {0.0};
  for (int m = tid; m < M; m += threads) total[0] += static_cast<double>(weight_of(a, row + m, top));
  block_sum<1>(total, wave_sum, tid, threads / MMF_WAVE);
  const double S = total[0];

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

  // ---- pairs: pair[u][k] = sum_j w_j |e_k|, [D + k] = sum_j w_j sgn(e_k), [kE] = sum_j w_j |z|, [kE + 1 + k] = sum_j w_j z_k / |z|
  double pair[IPT][kAcc];
#pragma unroll
  for (int u = 0; u < IPT; ++u)
#pragma unroll
    for (int k = 0; k < kAcc; ++k) pair[u][k] = 0.0;
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
      float acc[IPT][kAcc];
#pragma unroll
      for (int u = 0; u < IPT; ++u)
#pragma unroll
        for (int k = 0; k < kAcc; ++k) acc[u][k] = 0.f;
#pragma unroll 2
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
            float z[D], n2 = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
              const float e = xi[u][k] - pick(xj[k], c);
              if (CRPS) {
                acc[u][k] = fmaf(w, fabsf(e), acc[u][k]);
                float sw = e > 0.f ? w : 0.f;  // w sgn(e), sgn(0) = 0
                sw = e < 0.f ? -w : sw;
                acc[u][D + k] += sw;
              }
              if (ENERGY) {
                z[k] = SCALED ? e * a.inv_scale[k] : e;
                n2 = fmaf(z[k], z[k], n2);
              }
            }
            if (ENERGY) {
              // coinciding particles (and a squared distance below the normal range, which v_rsq_f32 does not take) give 0
              const float rinv = n2 >= FLT_MIN ? __builtin_amdgcn_rsqf(n2) : 0.f;
              acc[u][kE] = fmaf(w, n2 * rinv, acc[u][kE]);
              const float wr = w * rinv;
#pragma unroll
              for (int k = 0; k < D; ++k) acc[u][kE + 1 + k] = fmaf(wr, z[k], acc[u][kE + 1 + k]);
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < IPT; ++u)
#pragma unroll
        for (int k = 0; k < kAcc; ++k) pair[u][k] += static_cast<double>(acc[u][k]);
    }
  }

  // ---- the truth and the upstream gradients of this row; a term whose forward value is NaN is taken out: its truth
  // coordinate reads as 0 and its upstream gradient, whatever it holds, as 0
  double y[D], gk[D], gE = 0.0;
  bool all_ok = true;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const float yk = a.truth[static_cast<size_t>(r) * D + k];
    const bool ok = yk == yk;
    all_ok = all_ok && ok;
    y[k] = ok ? static_cast<double>(yk) : 0.0;
    gk[k] = 0.0;
    if (CRPS && ok) gk[k] = static_cast<double>(a.g_crps[static_cast<size_t>(r) * D + k]);
  }
  if (ENERGY && all_ok) gE = static_cast<double>(a.g_energy[r]);

  // ---- per i-particle: c_m and the state gradient, normalised by sum w in double
  double cm[IPT], Wm[IPT], part[1] = {0.0};
#pragma unroll
  for (int u = 0; u < IPT; ++u) {
    const int i = i0 + tid + u * threads;
    cm[u] = 0.0;
    Wm[u] = 0.0;
    double gx[D];
#pragma unroll
    for (int k = 0; k < D; ++k) gx[k] = 0.0;
    if (wi[u] > 0.f) {  // (selected away, not multiplied by 0)
      const double W = static_cast<double>(wi[u]) / S;
      double c = 0.0, e[D];
#pragma unroll
      for (int k = 0; k < D; ++k) e[k] = static_cast<double>(xi[u][k]) - y[k];
      if (CRPS) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const double sg = e[k] > 0.0 ? 1.0 : e[k] < 0.0 ? -1.0 : 0.0;
          c += gk[k] * (fabs(e[k]) - pair[u][k] / S);
          gx[k] = gk[k] * (sg - pair[u][D + k] / S);
        }
      }
      if (ENERGY) {
        double zz[D], n2 = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) {
          zz[k] = e[k] * static_cast<double>(a.inv_scale[k]);
          n2 += zz[k] * zz[k];
        }
        const double nrm = sqrt(n2);
        c += gE * (nrm - pair[u][kE] / S);
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const double uk = nrm > 0.0 ? zz[k] / nrm : 0.0;
          gx[k] += gE * ((uk - pair[u][kE + 1 + k] / S) * static_cast<double>(a.inv_scale[k]));
        }
      }
      cm[u] = c;
      Wm[u] = W;
      part[0] += W * c;
#pragma unroll
      for (int k = 0; k < D; ++k) gx[k] *= W;
    }
    if (i < i1 && a.g_states) {
#pragma unroll
      for (int k = 0; k < D; ++k) a.g_states[(row + i) * D + k] = written(gx[k]);  // (a dead particle: +0)
    }
  }

  // ---- sum_l W_l c_l: this workgroup's share, in block_sum's order
  block_sum<1>(part, wave_sum, tid, threads / MMF_WAVE);
  if (a.nb > 1) {
    double* ws = a.ws + ws_row(a, r);
    if (tid == 0) ws[b] = part[0];
#pragma unroll
    for (int u = 0; u < IPT; ++u) {
      const int i = i0 + tid + u * threads;
      if (i < i1) {
        ws[a.nb + i] = cm[u];
        ws[a.nb + M + i] = Wm[u];
      }
    }
    return;
  }
  if (!a.g_logw) return;
#pragma unroll
  for (int u = 0; u < IPT; ++u) {
    const int i = i0 + tid + u * threads;
    if (i < i1) a.g_logw[row + i] = Wm[u] > 0.0 ? written(Wm[u] * (cm[u] - part[0])) : 0.f;
  }
}

// nb > 1: g_logw[m] = W_m (c_m - sum_b partial_b), the partial sums added in ascending b by every thread
__global__ __launch_bounds__(kFinishThreads) void pf_scores_backward_finish_kernel(BArgs a, int per_row) {
  const int r = blockIdx.x / per_row, m = (blockIdx.x - r * per_row) * kFinishThreads + threadIdx.x;
  if (m >= a.M) return;
  const double* ws = a.ws + ws_row(a, r);
  double C = 0.0;
  for (int b = 0; b < a.nb; ++b) C += ws[b];
  const double c = ws[a.nb + m], W = ws[a.nb + a.M + m];
  a.g_logw[static_cast<size_t>(r) * a.M + m] = W > 0.0 ? written(W * (c - C)) : 0.f;
}

template <int D, int IPT, bool CRPS, bool ENERGY, bool SCALED>
int run(const BArgs& k, unsigned grid, int threads, hipStream_t s) {
  pf_scores_backward_kernel<D, IPT, CRPS, ENERGY, SCALED><<<grid, threads, 0, s>>>(k);
  MMF_CHECK_LAUNCH();
  return 0;
}

template <int D, bool CRPS, bool ENERGY, bool SCALED>
int run_ipt(const BArgs& k, const Plan& p, unsigned grid, hipStream_t s) {
  return p.ipt == 1 ? run<D, 1, CRPS, ENERGY, SCALED>(k, grid, p.threads, s) : run<D, 2, CRPS, ENERGY, SCALED>(k, grid, p.threads, s);
}

}  // namespace

extern "C" size_t mmf_pf_scores_backward_workspace_bytes(int R, int M, int d) {
  if (R < 1 || M < 1 || d < 1) return 0;
  const Plan p = plan_of(M);
  return p.nb > 1 ? static_cast<size_t>(R) * (p.nb + 2 * static_cast<size_t>(M)) * sizeof(double) : 0;
}

extern "C" int mmf_pf_scores_backward(const MmfPfScoresBackwardArgs* a, void* stream) {
  if (!a || check_rows(a->states, a->R, a->M, a->d) || !a->truth || check_scale(a->scale, a->d)) return MMF_EINVAL;
  if (!a->g_crps && !a->g_energy) return MMF_EINVAL;
  if (!a->g_states && !a->g_logw) return MMF_EINVAL;
  const Plan p = plan_of(a->M <= kMaxM ? a->M : kMaxM);  // (a larger M: check_size refuses it)
  const int per_row = (a->M <= kMaxM ? a->M : kMaxM) / kFinishThreads + 1;  // >= the finishing kernel's workgroups of a row, >= nb
  if (const int rc = check_size(a->R, a->M, per_row)) return rc;
  const size_t ws_bytes = mmf_pf_scores_backward_workspace_bytes(a->R, a->M, a->d);
  if (!workspace_ok(a->workspace, a->workspace_bytes, ws_bytes, alignof(double))) return MMF_EINVAL;
  {
    const size_t R = a->R, M = a->M, d = a->d, f = sizeof(float);
    const void* outs[3] = {a->g_states, a->g_logw, a->workspace};
    const size_t out_bytes[3] = {R * M * d * f, R * M * f, ws_bytes};
    const void* ins[6] = {a->states, a->log_a, a->log_b, a->truth, a->g_crps, a->g_energy};
    const size_t in_bytes[6] = {R * M * d * f, R * M * f, R * M * f, R * d * f, R * d * f, R * f};
    if (mmf_outputs_overlap(outs, out_bytes, 3, ins, in_bytes, 6)) return MMF_EINVAL;
  }
  if (a->R == 0) return 0;
  BArgs k{};
  k.states = a->states; k.log_a = a->log_a; k.log_b = a->log_b; k.truth = a->truth;
  k.g_crps = a->g_crps; k.g_energy = a->g_energy; k.g_states = a->g_states; k.g_logw = a->g_logw;
  k.ws = ws_bytes > 0 ? static_cast<double*>(a->workspace) : nullptr;
  k.M = a->M; k.nb = p.nb; k.chunk = p.chunk;
  const bool scaled = inv_scale_of(a->scale, a->d, k.inv_scale);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(a->R) * static_cast<unsigned>(p.nb);
  const int rc = mmf::with_state_dim(a->d, [&](auto D) {
    constexpr int kD = decltype(D)::value;
    if (!a->g_energy) return run_ipt<kD, true, false, false>(k, p, grid, s);  // (the scale enters the norm alone)
    return mmf::with_bool(scaled, [&](auto S) {
      constexpr bool kS = decltype(S)::value;
      return a->g_crps ? run_ipt<kD, true, true, kS>(k, p, grid, s) : run_ipt<kD, false, true, kS>(k, p, grid, s);
    });
  });
  if (rc != 0 || p.nb == 1 || !a->g_logw) return rc;
  const int blocks = (a->M + kFinishThreads - 1) / kFinishThreads;
  pf_scores_backward_finish_kernel<<<static_cast<unsigned>(a->R) * static_cast<unsigned>(blocks), kFinishThreads, 0, s>>>(k, blocks);
  MMF_CHECK_LAUNCH();
  return 0;
}
