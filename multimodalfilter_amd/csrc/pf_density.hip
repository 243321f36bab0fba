// Gaussian product-kernel density of a weighted particle set (include/mmf.h, "Particle-posterior density"): the log density at
// every particle of the set and at a true state, the resubstitution entropy and the mode, over all M^2 pairs of a row.
// The plain float live weights of pf_summary.h; every sum in a fixed order, no atomics.
//   plan      the dealing of pf_summary.h: nb workgroups to a row, IPT query particles of a thread in registers
//   moments   every workgroup of a row forms max a, sum w, sum w^2, mu and sigma^2 over the WHOLE row itself, two passes in
//             double in one fixed order: M loads beside M^2 / nb pairs, no workgroup waits on another, all hold the same bits
//   pairs     j-tiles of 1024 particles through LDS as structure-of-arrays: d planes of (x - mu) / h and one of log2 w (-inf
//             for a dead particle, whose coordinates are staged as 0); four j per broadcast ds_read_b128.  Per pair d
//             subtract-multiplies into z, e = log2 w - z (1/2 log2 e), v_exp_f32.  A running maximum of e per query; the
//             running fp32 sum is rescaled once per four j -- one more exp2 per four pairs, no branch -- and flushed to a
//             double, kept relative to the maximum at the flush, every 64 j: the rounding of the sum does not grow with M
//   truth     one more query per row: workgroup 0 splits the row's j over its threads, each with its own running (max, sum),
//             combined by a butterfly over the wave and the waves in order.  The particle outputs do not see it
//   reduce    entropy terms in double and (value, index) of the mode: butterfly over the wave, the waves in order through LDS;
//             the moments through summary::block_sum
//   finish    nb == 1: the workgroup writes the row.  nb > 1: partials to the workspace and pf_density_finish_kernel, a
//             thread per row, takes them in block order

#include <climits>
#include <cmath>

#include "pf_summary.h"

namespace {

using namespace mmf::summary;  // the dealing, the weights, block_max, block_sum, pick and the host's checks

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kHalfLog2e = 0.7213475204444817f;
constexpr double kLn2 = 0.6931471805599453;
constexpr double kHalfLog2Pi = 0.9189385332046727;
constexpr float kNoMax = -3.0e38f;  // start of a running maximum: finite, so that -inf - max is -inf and not NaN

struct Partial {  // what a workgroup of a row with nb > 1 leaves in the workspace
  double entropy;
  float best;
  int index;  // -1: no live particle in the chunk
};

struct DArgs {
  const float* states;  // (R, M, d)
  const float* log_a;   // (R, M) or null
  const float* log_b;   // (R, M) or null
  const float* truth;   // (R, d) or null
  float* log_density;   // (R, M) or null
  float* log_score;     // (R) or null
  float* entropy;       // (R) or null
  float* mode;          // (R, d) or null
  int* mode_index;      // (R) or null
  float* bandwidth_out; // (R, d) or null
  Partial* ws;          // (R, nb) for nb > 1
  int M, d, nb, chunk, rule, pairs;
  float bandwidth[MMF_MAX_STATE_DIM], min_bandwidth[MMF_MAX_STATE_DIM];
};

// w_m and log2 w_m (-inf where w_m = 0) of the particle at `at`
__device__ __forceinline__ float weight_of(const DArgs& a, size_t at, float top, float* l2w) {
  const float t = log_weight(a.log_a, a.log_b, at) - top;
  const float w = live_weight(t);
  *l2w = w > 0.f ? t * kLog2e : -INFINITY;
  return w;
}

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// an online (max, sum of 2^(e - max)) takes another one in: both sums rescaled to the larger maximum
__device__ __forceinline__ void merge(float& m, float& s, float om, float os) {
  const float mn = fmaxf(m, om);
  const float mine = s * __builtin_amdgcn_exp2f(m - mn), theirs = os * __builtin_amdgcn_exp2f(om - mn);
  s = mine + theirs;
  m = mn;
}

// log p at a query from its running maximum and sum: cst = -log S - sum log h - d/2 log 2 pi
__device__ __forceinline__ double log_p(float mx, double s, double cst) {
  return static_cast<double>(mx) * kLn2 + static_cast<double>(logf(static_cast<float>(s))) + cst;
}

__device__ __forceinline__ void write_mode(const DArgs& a, int r, int index, double entropy) {
  if (a.entropy) a.entropy[r] = index < 0 ? NAN : static_cast<float>(entropy);
  if (a.mode_index) a.mode_index[r] = index;
  if (a.mode) {
    const unsigned* src = reinterpret_cast<const unsigned*>(a.states) + (static_cast<size_t>(r) * a.M + (index < 0 ? 0 : index)) * a.d;
    unsigned* dst = reinterpret_cast<unsigned*>(a.mode) + static_cast<size_t>(r) * a.d;
    for (int k = 0; k < a.d; ++k) dst[k] = index < 0 ? 0x7fc00000u : src[k];  // a bit copy; NaN without a live particle
  }
}

template <int D, int IPT>
__global__ __launch_bounds__(kIBlock / IPT) void pf_density_kernel(DArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[(D + 1) * kJTile];
  __shared__ double wave_sum[kMaxWaves][MMF_MAX_STATE_DIM + 2];
  __shared__ float wave_f[2][kMaxWaves];
  __shared__ int wave_i[kMaxWaves];
  const int tid = threadIdx.x, threads = blockDim.x, M = a.M;
  const int lane = tid & (MMF_WAVE - 1), wave = tid / MMF_WAVE, waves = threads / MMF_WAVE;
  const int r = blockIdx.x / a.nb, b = blockIdx.x - r * a.nb;
  const size_t row = static_cast<size_t>(r) * M;
  if (!a.pairs && b != 0) return;  // the truth and the bandwidth alone are workgroup 0's

  // ---- the row maximum of a_m = log_a[m] + log_b[m]
  float top = -INFINITY;
  for (int m = tid; m < M; m += threads) top = fmaxf(top, log_weight(a.log_a, a.log_b, row + m));  // (a NaN is skipped)
  top = block_max(top, wave_f[0], tid, waves);

  // ---- the row's moments, live particles only, two passes in double: sum w, sum w^2, sum w x; then sum w (x - mu)^2
  double v[D + 2];
#pragma unroll
  for (int k = 0; k < D + 2; ++k) v[k] = 0.0;
  for (int m = tid; m < M; m += threads) {
    float l2w;
    const float w = weight_of(a, row + m, top, &l2w);
    if (!(w > 0.f)) continue;  // (selected away, not multiplied by 0)
    const double dw = static_cast<double>(w);
    v[0] += dw;
    v[1] += dw * dw;
#pragma unroll
    for (int k = 0; k < D; ++k) v[2 + k] += dw * static_cast<double>(a.states[(row + m) * D + k]);
  }
  block_sum<D + 2>(v, wave_sum, tid, waves);
  const double S = v[0];
  if (!(S > 0.0)) {  // no live particle in the row: NaN everywhere, mode_index -1
    for (int i = b * a.chunk + tid; i < min(M, (b + 1) * a.chunk); i += threads)
      if (a.log_density) a.log_density[row + i] = NAN;
    if (tid == 0) {
      if (b == 0) {
        if (a.log_score) a.log_score[r] = NAN;
        if (a.bandwidth_out)
          for (int k = 0; k < D; ++k) a.bandwidth_out[static_cast<size_t>(r) * D + k] = NAN;
      }
      if (a.pairs) {
        if (a.nb > 1) a.ws[blockIdx.x] = Partial{static_cast<double>(NAN), -INFINITY, -1};
        else write_mode(a, r, -1, NAN);
      }
    }
    return;
  }
  double mu[D], m2[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    mu[k] = v[2 + k] / S;
    m2[k] = 0.0;
  }
  const double n_eff = S * S / v[1];
  if (a.rule != 0) {
    for (int m = tid; m < M; m += threads) {
      float l2w;
      const float w = weight_of(a, row + m, top, &l2w);
      if (!(w > 0.f)) continue;
      const double dw = static_cast<double>(w);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const double e = static_cast<double>(a.states[(row + m) * D + k]) - mu[k];
        m2[k] += dw * e * e;
      }
    }
    block_sum<D>(m2, wave_sum, tid, waves);
  }
  // ---- the bandwidths; the coordinates are taken relative to mu before they are divided by h
  const double c = a.rule == 0 ? 1.0 : a.rule == 1 ? pow(4.0 / ((D + 2) * n_eff), 1.0 / (D + 4)) : pow(n_eff, -1.0 / (D + 4));
  float muf[D], ih[D], hf[D];
  double cst = -log(S) - D * kHalfLog2Pi;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double h = a.rule == 0 ? static_cast<double>(a.bandwidth[k])
                                 : fmax(sqrt(m2[k] / S) * c, static_cast<double>(a.min_bandwidth[k]));
    hf[k] = static_cast<float>(h);
    ih[k] = 1.0f / hf[k];
    muf[k] = static_cast<float>(mu[k]);
    cst -= log(static_cast<double>(hf[k]));
  }
  if (b == 0 && tid == 0 && a.bandwidth_out)
#pragma unroll
    for (int k = 0; k < D; ++k) a.bandwidth_out[static_cast<size_t>(r) * D + k] = hf[k];

  // ---- the truth: workgroup 0, the row's j dealt over its threads
  if (b == 0 && a.log_score) {
    float yq[D];
    bool nan_y = false;
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const float y = a.truth[static_cast<size_t>(r) * D + k];
      nan_y = nan_y || y != y;
      yq[k] = (y - muf[k]) * ih[k];
    }
    float tm = kNoMax, ts = 0.f;
    for (int m = tid; m < M; m += threads) {
      float l2w;
      const float w = weight_of(a, row + m, top, &l2w);
      if (!(w > 0.f)) continue;
      float z = 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const float e = yq[k] - (a.states[(row + m) * D + k] - muf[k]) * ih[k];
        z = fmaf(e, e, z);
      }
      merge(tm, ts, fmaf(z, -kHalfLog2e, l2w), 1.f);
    }
#pragma unroll
    for (int off = 1; off < MMF_WAVE; off <<= 1) merge(tm, ts, __shfl_xor(tm, off, MMF_WAVE), __shfl_xor(ts, off, MMF_WAVE));
    __syncthreads();  // wave_f's last readers are done
    if (lane == 0) {
      wave_f[0][wave] = tm;
      wave_f[1][wave] = ts;
    }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < waves; ++w) merge(tm, ts, wave_f[0][w], wave_f[1][w]);
      a.log_score[r] = nan_y ? NAN : static_cast<float>(log_p(tm, static_cast<double>(ts), cst));
    }
  }
  if (!a.pairs) return;

  // ---- this thread's query particles
  const int i0 = b * a.chunk, i1 = min(M, i0 + a.chunk);
  float qi[IPT][D], wi[IPT], mx[IPT], sum[IPT], base[IPT];
  double acc[IPT];  // the sum of the runs before this one, relative to base, the maximum at the last flush
#pragma unroll
  for (int u = 0; u < IPT; ++u) {
    const int i = i0 + tid + u * threads;
    float l2w;
    wi[u] = i < i1 ? weight_of(a, row + i, top, &l2w) : 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) qi[u][k] = wi[u] > 0.f ? (a.states[(row + i) * D + k] - muf[k]) * ih[k] : 0.f;
    mx[u] = base[u] = kNoMax;
    sum[u] = 0.f;
    acc[u] = 0.0;
  }

  // ---- pairs: a running maximum and the sum of 2^(e - maximum) per query, e = log2 w_j - 1/2 log2(e) |q - x_j|^2
  for (int j0 = 0; j0 < M; j0 += kJTile) {
    const int n = min(kJTile, M - j0), npad = (n + 3) & ~3;
    __syncthreads();  // the tile before this one has been read
    for (int j = tid; j < npad; j += threads) {
      float l2w = -INFINITY;
      const float w = j < n ? weight_of(a, row + j0 + j, top, &l2w) : 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) tile[k * kJTile + j] = w > 0.f ? (a.states[(row + j0 + j) * D + k] - muf[k]) * ih[k] : 0.f;
      tile[D * kJTile + j] = l2w;
    }
    __syncthreads();
    for (int jr = 0; jr < npad; jr += kRun) {
      const int jend = min(npad, jr + kRun);
#pragma unroll 2
      for (int q = jr; q < jend; q += 4) {
        float4 xj[D];
#pragma unroll
        for (int k = 0; k < D; ++k) xj[k] = *reinterpret_cast<const float4*>(&tile[k * kJTile + q]);
        const float4 lj = *reinterpret_cast<const float4*>(&tile[D * kJTile + q]);
#pragma unroll
        for (int u = 0; u < IPT; ++u) {
          float e[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float z = 0.f;
#pragma unroll
            for (int k = 0; k < D; ++k) {
              const float t = qi[u][k] - pick(xj[k], c);
              z = fmaf(t, t, z);
            }
            e[c] = fmaf(z, -kHalfLog2e, pick(lj, c));
          }
          const float mn = fmaxf(fmaxf(mx[u], fmaxf(e[0], e[1])), fmaxf(e[2], e[3]));
          float s = sum[u] * __builtin_amdgcn_exp2f(mx[u] - mn);
#pragma unroll
          for (int c = 0; c < 4; ++c) s += __builtin_amdgcn_exp2f(e[c] - mn);
          sum[u] = s;
          mx[u] = mn;
        }
      }
#pragma unroll
      for (int u = 0; u < IPT; ++u) {
        acc[u] = acc[u] * static_cast<double>(__builtin_amdgcn_exp2f(base[u] - mx[u])) + static_cast<double>(sum[u]);
        base[u] = mx[u];
        sum[u] = 0.f;
      }
    }
  }

  // ---- the log density at the query particles, this thread's entropy terms and its best particle
  double ent = 0.0;
  float best = -INFINITY;
  int best_i = INT_MAX;
#pragma unroll
  for (int u = 0; u < IPT; ++u) {
    const int i = i0 + tid + u * threads;
    if (i >= i1) continue;
    const bool live = wi[u] > 0.f;
    const double lp = log_p(mx[u], acc[u], cst);
    const float ld = live ? static_cast<float>(lp) : -INFINITY;
    if (a.log_density) a.log_density[row + i] = ld;
    if (!live) continue;  // (selected away)
    ent += static_cast<double>(wi[u]) * lp;
    if (better(ld, i, best, best_i)) {
      best = ld;
      best_i = i;
    }
  }
  if (!a.entropy && !a.mode && !a.mode_index) return;

  // ---- over the workgroup: a butterfly in each wave, then the waves in order
#pragma unroll
  for (int off = 1; off < MMF_WAVE; off <<= 1) {
    ent += __shfl_xor(ent, off, MMF_WAVE);
    const float ov = __shfl_xor(best, off, MMF_WAVE);
    const int oi = __shfl_xor(best_i, off, MMF_WAVE);
    if (better(ov, oi, best, best_i)) {
      best = ov;
      best_i = oi;
    }
  }
  __syncthreads();  // the scratch's last readers are done
  if (lane == 0) {
    wave_sum[wave][0] = ent;
    wave_f[0][wave] = best;
    wave_i[wave] = best_i;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < waves; ++w) {
    ent += wave_sum[w][0];
    if (better(wave_f[0][w], wave_i[w], best, best_i)) {
      best = wave_f[0][w];
      best_i = wave_i[w];
    }
  }
  const double entropy = -(ent / S);
  const int index = best_i == INT_MAX ? -1 : best_i;
  if (a.nb > 1) a.ws[blockIdx.x] = Partial{entropy, best, index};
  else write_mode(a, r, index, entropy);
}

__global__ __launch_bounds__(MMF_WAVE) void pf_density_finish_kernel(DArgs a, int R) {
  const int r = blockIdx.x * MMF_WAVE + threadIdx.x;
  if (r >= R) return;
  double entropy = 0.0;
  float best = -INFINITY;
  int index = -1;
  for (int b = 0; b < a.nb; ++b) {
    const Partial p = a.ws[static_cast<size_t>(r) * a.nb + b];
    entropy += p.entropy;
    if (p.index >= 0 && (index < 0 || better(p.best, p.index, best, index))) {
      best = p.best;
      index = p.index;
    }
  }
  write_mode(a, r, index, entropy);
}

template <int D, int IPT>
int run(const DArgs& k, unsigned grid, int threads, hipStream_t s) {
  pf_density_kernel<D, IPT><<<grid, threads, 0, s>>>(k);
  MMF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t mmf_pf_density_workspace_bytes(int R, int M, int d) {
  if (R < 1 || M < 1 || d < 1) return 0;
  const Plan p = plan_of(M);
  return p.nb > 1 ? static_cast<size_t>(R) * p.nb * sizeof(Partial) : 0;
}

extern "C" int mmf_pf_density(const MmfPfDensityArgs* a, void* stream) {
  if (!a || check_rows(a->states, a->R, a->M, a->d)) return MMF_EINVAL;
  if (a->rule < 0 || a->rule > 2) return MMF_EINVAL;
  const float* read = a->rule == 0 ? a->bandwidth : a->min_bandwidth;
  for (int k = 0; k < a->d; ++k)
    if (!(read[k] > 0.f && read[k] < INFINITY)) return MMF_EINVAL;  // (a NaN fails)
  const bool pairs = a->log_density || a->entropy || a->mode || a->mode_index;
  if (!pairs && !a->log_score && !a->bandwidth_out) return MMF_EINVAL;
  if (a->log_score && !a->truth) return MMF_EINVAL;
  const Plan p = plan_of(a->M <= kMaxM ? a->M : kMaxM);  // (a larger M: check_size refuses it)
  if (const int rc = check_size(a->R, a->M, p.nb)) return rc;
  const size_t ws_bytes = mmf_pf_density_workspace_bytes(a->R, a->M, a->d);
  if (!workspace_ok(a->workspace, a->workspace_bytes, ws_bytes, alignof(Partial))) return MMF_EINVAL;
  {
    const size_t R = a->R, M = a->M, d = a->d, f = sizeof(float);
    const void* outs[7] = {a->log_density, a->log_score, a->entropy, a->mode, a->mode_index, a->bandwidth_out, a->workspace};
    const size_t out_bytes[7] = {R * M * f, R * f, R * f, R * d * f, R * sizeof(int32_t), R * d * f, ws_bytes};
    if (outputs_alias(a->states, a->log_a, a->log_b, a->truth, R, M, d, outs, out_bytes)) return MMF_EINVAL;
  }
  if (a->R == 0) return 0;
  DArgs k{};
  k.states = a->states; k.log_a = a->log_a; k.log_b = a->log_b; k.truth = a->truth;
  k.log_density = a->log_density; k.log_score = a->log_score; k.entropy = a->entropy;
  k.mode = a->mode; k.mode_index = a->mode_index; k.bandwidth_out = a->bandwidth_out;
  k.ws = ws_bytes > 0 ? static_cast<Partial*>(a->workspace) : nullptr;
  k.M = a->M; k.d = a->d; k.nb = p.nb; k.chunk = p.chunk; k.rule = a->rule; k.pairs = pairs ? 1 : 0;
  for (int i = 0; i < MMF_MAX_STATE_DIM; ++i) {
    k.bandwidth[i] = a->rule == 0 && i < a->d ? a->bandwidth[i] : 1.0f;
    k.min_bandwidth[i] = a->rule != 0 && i < a->d ? a->min_bandwidth[i] : 1.0f;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(a->R) * static_cast<unsigned>(p.nb);
  const int rc = mmf::with_state_dim(a->d, [&](auto D) {
    constexpr int kD = decltype(D)::value;
    return p.ipt == 1 ? run<kD, 1>(k, grid, p.threads, s) : run<kD, 2>(k, grid, p.threads, s);
  });
  if (rc != 0 || p.nb == 1 || !(a->entropy || a->mode || a->mode_index)) return rc;
  pf_density_finish_kernel<<<(a->R + MMF_WAVE - 1) / MMF_WAVE, MMF_WAVE, 0, s>>>(k, a->R);
  MMF_CHECK_LAUNCH();
  return 0;
}
