// Scores of a predictive Gaussian mixture with one shared covariance (include/mmf.h, "Predictive mixtures"): per row the
// mixture sum_i W_i N(x; F_i, L L^T) -- the centres F are the particles after a noise-free propagation -- and its mean,
// covariance, logarithmic score, PIT and CRPS in closed form.  The weights and the dead-particle rule are pf_summary.h's.
//   A(m; s) = E|Z|, Z ~ N(m, s^2) = s sqrt(2) g(m / (s sqrt(2))),   g(t) = t erf(t) + exp(-t^2) / sqrt(pi), even, >= 1 / sqrt(pi)
//   pairs   pf_predictive_pairs_kernel<D, IPT>, the plan of pf_scores.hip with g in place of |.|: spread_k = sum_i sum_j W_i W_j
//           A(F_ik - F_jk; sqrt(2) sigma_k) = 2 sigma_k sum sum W W g((F_ik - F_jk) / (2 sigma_k)).  The dealing of
//           pf_summary.h, j-tiles of 1024 through LDS as structure-of-arrays read as broadcasts, dead particles staged as zeros
//           with zero weight, fp32 runs of 64 pairs flushed to double; the truth term sum_i W_i A(y_k - F_ik; sigma_k) over the
//           workgroup's own i-particles.  2 d + 1 double sums per workgroup in one order; nb == 1 writes the row, nb > 1 goes
//           through the workspace and pf_predictive_finish_kernel.  No atomics.  Runs only when spread or crps is asked for.
//   g       |t| + exp(-t^2) p(1 / (1 + |t| / 2)), p of degree 9 fitted to 1 / sqrt(pi) - |t| erfcx(|t|) on all of [0, inf): one
//           v_rcp_f32, one v_exp_f32, sixteen plain operations that pack two wide, no branch; within 7e-7 of g relative to g
//           in fp32, and |t| to fp32 beyond |t| of about 4.  Every term of the pair sum is positive, so that is also the
//           bound on the sum.
//   rows    pf_predictive_row_kernel<D>, a workgroup of 256 threads per row, everything in double: pass 1 sum w, sum w F, sum w
//           Phi and the largest exponent; pass 2 the central second moments (difference first) and the log-sum-exp about that
//           exponent.  Every figure is computed whichever outputs are asked for, so an output's bits do not depend on the others.

#include <cmath>

#include "pf_summary.h"

namespace {

using namespace mmf::summary;  // the dealing, the weights, block_max, the ordered sums, pick and the host's checks

constexpr int kSums = 2 * MMF_MAX_STATE_DIM + 1;  // pair sums (d), truth sums (d), sum w: the stride of a workspace entry
constexpr int kRowThreads = 256;
constexpr int kRowWaves = kRowThreads / MMF_WAVE;
constexpr int kRowSums = 16;  // >= 2 d + 1 (pass 1) and d (d + 1) / 2 + 1 (pass 2)

struct PArgs {
  const float* centres;  // (R, M, d)
  const float* log_a;    // (R, M) or null
  const float* log_b;    // (R, M) or null
  const float* tril;     // (d, d), the lower triangle is read
  const float* truth;    // (R, d) or null
  float* mean;           // (R, d) or null
  float* covariance;     // (R, d, d) or null
  float* log_score;      // (R) or null
  float* pit;            // (R, d) or null
  float* spread;         // (R, d) or null
  float* crps;           // (R, d) or null
  double* ws;            // (R, nb, kSums) for nb > 1
  int M, d, nb, chunk;
};

// sigma_k = sqrt((L L^T)_kk), in double from the fp32 lower triangle
__device__ __forceinline__ double sigma_of(const float* tril, int d, int k) {
  double q = 0.0;
  for (int c = 0; c <= k; ++c) {
    const double l = static_cast<double>(tril[k * d + c]);
    q += l * l;
  }
  return sqrt(q);
}

// g(t) = t erf(t) + exp(-t^2) / sqrt(pi)
__device__ __forceinline__ float g_of(float t) {
  const float x = fabsf(t);
  const float s = __builtin_amdgcn_rcpf(fmaf(0.5f, x, 1.0f));
  float p = -7.535947114e-02f;
  p = fmaf(p, s, 4.756424725e-01f);
  p = fmaf(p, s, -1.098466277e+00f);
  p = fmaf(p, s, 1.011966348e+00f);
  p = fmaf(p, s, -2.436499447e-01f);
  p = fmaf(p, s, 2.984257936e-01f);
  p = fmaf(p, s, 1.238287091e-01f);
  p = fmaf(p, s, 7.184085250e-02f);
  p = fmaf(p, s, -3.893237226e-05f);
  p = fmaf(p, s, 1.896274853e-07f);
  const float e = __builtin_amdgcn_exp2f(x * x * -1.4426950408889634f);  // exp(-t^2); 0 once that is below fp32
  return fmaf(e, p, x);
}

// sums[0 .. d): sum_i sum_j w_i w_j g((F_ik - F_jk) / (2 sigma_k)); [d .. 2 d): sum_i w_i g((y_k - F_ik) / (sigma_k sqrt 2));
// [2 d]: sum w
__device__ __forceinline__ void write_row(const PArgs& a, int r, const double* sums) {
  const int d = a.d;
  const double S = sums[2 * d];
  const bool dead = !(S > 0.0);  // no live particle in the row
  for (int k = 0; k < d; ++k) {
    const double sigma = sigma_of(a.tril, d, k);
    const double spread = 2.0 * sigma * (sums[k] / (S * S));
    const size_t at = static_cast<size_t>(r) * d + k;
    if (a.spread) a.spread[at] = dead ? NAN : static_cast<float>(spread);
    if (a.crps) {
      const bool no_truth = a.truth[at] != a.truth[at];
      a.crps[at] = dead || no_truth ? NAN : static_cast<float>(sigma * 1.4142135623730951 * (sums[d + k] / S) - 0.5 * spread);
    }
  }
}

__device__ __forceinline__ float weight_of(const PArgs& a, size_t at, float top) {
  return live_weight(log_weight(a.log_a, a.log_b, at) - top);
}

template <int D, int IPT>
__global__ __launch_bounds__(kIBlock / IPT) void pf_predictive_pairs_kernel(PArgs a) {
  __shared__ __attribute__((aligned(16))) float tile[(D + 1) * kJTile];
  __shared__ double wave_sum[kMaxWaves][2 * D + 1];
  __shared__ float wave_top[kMaxWaves];
  const int tid = threadIdx.x, threads = blockDim.x, M = a.M;
  const int r = blockIdx.x / a.nb, b = blockIdx.x - r * a.nb;
  const size_t row = static_cast<size_t>(r) * M;

  // ---- the row maximum of a_m = log_a[m] + log_b[m]
  float top = -INFINITY;
  for (int m = tid; m < M; m += threads) top = fmaxf(top, log_weight(a.log_a, a.log_b, row + m));  // (a NaN is skipped)
  top = block_max(top, wave_top, tid, threads / MMF_WAVE);

  // ---- 1 / (2 sigma_k) of the pairs and 1 / (sigma_k sqrt 2) of the truth
  float inv_pair[D], inv_truth[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double sigma = sigma_of(a.tril, D, k);
    inv_pair[k] = static_cast<float>(0.5 / sigma);
    inv_truth[k] = static_cast<float>(0.7071067811865476 / sigma);
  }

  // ---- this thread's i-particles
  const int i0 = b * a.chunk, i1 = min(M, i0 + a.chunk);
  float xi[IPT][D], wi[IPT];
#pragma unroll
  for (int u = 0; u < IPT; ++u) {
    const int i = i0 + tid + u * threads;
    wi[u] = i < i1 ? weight_of(a, row + i, top) : 0.f;
#pragma unroll
    for (int k = 0; k < D; ++k) xi[u][k] = wi[u] > 0.f ? a.centres[(row + i) * D + k] : 0.f;
  }

  // ---- pairs: pair[u][k] = sum_j w_j g((F_ik - F_jk) / (2 sigma_k))
  double pair[IPT][D];
#pragma unroll
  for (int u = 0; u < IPT; ++u)
#pragma unroll
    for (int k = 0; k < D; ++k) pair[u][k] = 0.0;
  for (int j0 = 0; j0 < M; j0 += kJTile) {
    const int n = min(kJTile, M - j0), npad = (n + kRun - 1) / kRun * kRun;
    __syncthreads();  // the tile before this one has been read
    for (int j = tid; j < npad; j += threads) {
      const float w = j < n ? weight_of(a, row + j0 + j, top) : 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) tile[k * kJTile + j] = w > 0.f ? a.centres[(row + j0 + j) * D + k] : 0.f;
      tile[D * kJTile + j] = w;
    }
    __syncthreads();
    for (int jr = 0; jr < npad; jr += kRun) {
      float acc[IPT][D];
#pragma unroll
      for (int u = 0; u < IPT; ++u)
#pragma unroll
        for (int k = 0; k < D; ++k) acc[u][k] = 0.f;
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
          for (int u = 0; u < IPT; ++u)
#pragma unroll
            for (int k = 0; k < D; ++k) acc[u][k] = fmaf(w, g_of((xi[u][k] - pick(xj[k], c)) * inv_pair[k]), acc[u][k]);
        }
      }
#pragma unroll
      for (int u = 0; u < IPT; ++u)
#pragma unroll
        for (int k = 0; k < D; ++k) pair[u][k] += static_cast<double>(acc[u][k]);
    }
  }

  // ---- this thread's share of the 2 D + 1 sums
  double v[2 * D + 1];
#pragma unroll
  for (int k = 0; k < 2 * D + 1; ++k) v[k] = 0.0;
#pragma unroll
  for (int u = 0; u < IPT; ++u) {
    if (!(wi[u] > 0.f)) continue;  // (selected away, not multiplied by 0)
    const double w = static_cast<double>(wi[u]);
#pragma unroll
    for (int k = 0; k < D; ++k) v[k] += w * pair[u][k];
    if (a.truth) {
#pragma unroll
      for (int k = 0; k < D; ++k)
        v[D + k] += w * static_cast<double>(g_of((a.truth[static_cast<size_t>(r) * D + k] - xi[u][k]) * inv_truth[k]));
    }
    v[2 * D] += w;
  }

  // ---- over the workgroup: thread k takes sum k
  wave_sums<2 * D + 1>(v, wave_sum, tid);
  __syncthreads();
  if (tid < 2 * D + 1) {
    const double s = sum_of_waves(wave_sum, tid, threads / MMF_WAVE);
    if (a.nb > 1) a.ws[static_cast<size_t>(blockIdx.x) * kSums + tid] = s;
    wave_sum[0][tid] = s;
  }
  if (a.nb > 1) return;
  __syncthreads();
  if (tid == 0) write_row(a, r, wave_sum[0]);
}

__global__ __launch_bounds__(MMF_WAVE) void pf_predictive_finish_kernel(PArgs a, int R) {
  const int r = blockIdx.x * MMF_WAVE + threadIdx.x;
  if (r >= R) return;
  double sums[kSums];
  const int q = 2 * a.d + 1;
  for (int k = 0; k < q; ++k) {
    double s = 0.0;
    for (int b = 0; b < a.nb; ++b) s += a.ws[(static_cast<size_t>(r) * a.nb + b) * kSums + k];
    sums[k] = s;
  }
  write_row(a, r, sums);
}

// the maximum of v over the workgroup, in every thread (exact in any order; fmax skips a NaN)
__device__ __forceinline__ double block_max_double(double v, double* scratch, int tid) {
#pragma unroll
  for (int off = 1; off < MMF_WAVE; off <<= 1) v = fmax(v, __shfl_xor(v, off, MMF_WAVE));
  if ((tid & (MMF_WAVE - 1)) == 0) scratch[tid / MMF_WAVE] = v;
  __syncthreads();
  v = scratch[0];
  for (int w = 1; w < kRowWaves; ++w) v = fmax(v, scratch[w]);
  return v;
}

template <int D>
__global__ __launch_bounds__(kRowThreads) void pf_predictive_row_kernel(PArgs a) {
  __shared__ double wave_sum[kRowWaves][kRowSums];
  __shared__ double wave_dmax[kRowWaves];
  __shared__ float wave_top[kRowWaves];
  constexpr int kTri = D * (D + 1) / 2;
  const int tid = threadIdx.x, M = a.M, r = blockIdx.x;
  const size_t row = static_cast<size_t>(r) * M;

  float top = -INFINITY;
  for (int m = tid; m < M; m += kRowThreads) top = fmaxf(top, log_weight(a.log_a, a.log_b, row + m));  // (a NaN is skipped)
  top = block_max(top, wave_top, tid, kRowWaves);

  // ---- L (lower triangle), sigma, and the truth
  double L[D][D], sigma[D], y[D];
  bool no_truth = false;
#pragma unroll
  for (int j = 0; j < D; ++j) {
#pragma unroll
    for (int c = 0; c < D; ++c) L[j][c] = c <= j ? static_cast<double>(a.tril[j * D + c]) : 0.0;
    sigma[j] = sigma_of(a.tril, D, j);
    y[j] = a.truth ? static_cast<double>(a.truth[static_cast<size_t>(r) * D + j]) : 0.0;
    no_truth = no_truth || y[j] != y[j];
  }

  // the exponent of particle m in the log score: t_m - 1/2 |L^-1 (y - F_m)|^2 (forward substitution)
  auto exponent = [&](double t, const double* x) {
    double z[D], n2 = 0.0;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double e = y[j] - x[j];
#pragma unroll
      for (int c = 0; c < j; ++c) e -= L[j][c] * z[c];
      z[j] = e / L[j][j];
      n2 += z[j] * z[j];
    }
    return t - 0.5 * n2;
  };

  // ---- pass 1: sum w, sum w F, sum w Phi((y - F) / sigma), the largest exponent
  double v[kRowSums];
#pragma unroll
  for (int k = 0; k < kRowSums; ++k) v[k] = 0.0;
  double emax = -INFINITY;
  for (int m = tid; m < M; m += kRowThreads) {
    const float t = log_weight(a.log_a, a.log_b, row + m) - top;
    const float wf = live_weight(t);
    if (!(wf > 0.f)) continue;  // (selected away, not multiplied by 0: its row is not read)
    const double w = static_cast<double>(wf);
    double x[D];
#pragma unroll
    for (int k = 0; k < D; ++k) x[k] = static_cast<double>(a.centres[(row + m) * D + k]);
    v[0] += w;
#pragma unroll
    for (int k = 0; k < D; ++k) v[1 + k] += w * x[k];
    if (a.truth) {
#pragma unroll
      for (int k = 0; k < D; ++k) v[1 + D + k] += w * (0.5 * erfc((x[k] - y[k]) / sigma[k] * 0.7071067811865476));
      emax = fmax(emax, exponent(static_cast<double>(t), x));
    }
  }
  block_sum<2 * D + 1>(v, wave_sum, tid, kRowWaves);
  emax = block_max_double(emax, wave_dmax, tid);
  const double S = v[0];
  const bool dead = !(S > 0.0);  // no live particle in the row
  double mu[D], phi[D];
#pragma unroll
  for (int k = 0; k < D; ++k) {
    mu[k] = v[1 + k] / S;
    phi[k] = v[1 + D + k] / S;
  }

  // ---- pass 2: sum w (F - mu)(F - mu)^T, upper triangle row-major, and sum exp(exponent - emax)
#pragma unroll
  for (int k = 0; k < kRowSums; ++k) v[k] = 0.0;
  for (int m = tid; m < M; m += kRowThreads) {
    const float t = log_weight(a.log_a, a.log_b, row + m) - top;
    const float wf = live_weight(t);
    if (!(wf > 0.f)) continue;
    const double w = static_cast<double>(wf);
    double x[D], e[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      x[k] = static_cast<double>(a.centres[(row + m) * D + k]);
      e[k] = x[k] - mu[k];
    }
    int q = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i; j < D; ++j) v[q++] += w * (e[i] * e[j]);
    if (a.truth) v[kTri] += exp(exponent(static_cast<double>(t), x) - emax);
  }
  block_sum<kTri + 1>(v, wave_sum, tid, kRowWaves);
  if (tid != 0) return;

  if (a.mean)
    for (int k = 0; k < D; ++k) a.mean[static_cast<size_t>(r) * D + k] = dead ? NAN : static_cast<float>(mu[k]);
  if (a.covariance) {
    int q = 0;
    for (int i = 0; i < D; ++i)
      for (int j = i; j < D; ++j) {
        double Q = 0.0;
        for (int c = 0; c <= i; ++c) Q += L[i][c] * L[j][c];
        const float c_ij = dead ? NAN : static_cast<float>(v[q] / S + Q);
        ++q;
        a.covariance[(static_cast<size_t>(r) * D + i) * D + j] = c_ij;
        a.covariance[(static_cast<size_t>(r) * D + j) * D + i] = c_ij;
      }
  }
  if (a.pit)
    for (int k = 0; k < D; ++k) a.pit[static_cast<size_t>(r) * D + k] = dead || y[k] != y[k] ? NAN : static_cast<float>(phi[k]);
  if (a.log_score) {
    double log_det = 0.0;
    for (int j = 0; j < D; ++j) log_det += log(L[j][j]);
    a.log_score[r] = dead || no_truth ? NAN
                                      : static_cast<float>(emax + log(v[kTri]) - log(S) - log_det - 0.5 * D * 1.8378770664093453);
  }
}

template <int D, int IPT>
int run_pairs(const PArgs& k, unsigned grid, int threads, hipStream_t s) {
  pf_predictive_pairs_kernel<D, IPT><<<grid, threads, 0, s>>>(k);
  MMF_CHECK_LAUNCH();
  return 0;
}

template <int D>
int run_rows(const PArgs& k, unsigned grid, hipStream_t s) {
  pf_predictive_row_kernel<D><<<grid, kRowThreads, 0, s>>>(k);
  MMF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" size_t mmf_pf_predictive_workspace_bytes(int R, int M, int d) {
  if (R < 1 || M < 1 || d < 1) return 0;
  const Plan p = plan_of(M);
  return p.nb > 1 ? static_cast<size_t>(R) * p.nb * kSums * sizeof(double) : 0;
}

extern "C" int mmf_pf_predictive(const MmfPfPredictiveArgs* a, void* stream) {
  if (!a || check_rows(a->centres, a->R, a->M, a->d)) return MMF_EINVAL;
  if (!a->scale_tril) return MMF_EINVAL;
  const bool want_rows = a->mean || a->covariance || a->log_score || a->pit, want_pairs = a->spread || a->crps;
  if (!want_rows && !want_pairs) return MMF_EINVAL;
  if ((a->log_score || a->pit || a->crps) && !a->truth) return MMF_EINVAL;
  const Plan p = plan_of(a->M <= kMaxM ? a->M : kMaxM);  // (a larger M: check_size refuses it)
  if (const int rc = check_size(a->R, a->M, p.nb)) return rc;
  const size_t ws_bytes = want_pairs ? mmf_pf_predictive_workspace_bytes(a->R, a->M, a->d) : 0;
  if (!workspace_ok(a->workspace, a->workspace_bytes, ws_bytes, alignof(double))) return MMF_EINVAL;
  {
    const size_t R = a->R, M = a->M, d = a->d, f = sizeof(float);
    const void* outs[7] = {a->mean, a->covariance, a->log_score, a->pit, a->spread, a->crps, a->workspace};
    const size_t out_bytes[7] = {R * d * f, R * d * d * f, R * f, R * d * f, R * d * f, R * d * f, ws_bytes};
    const void* ins[5] = {a->centres, a->log_a, a->log_b, a->truth, a->scale_tril};
    const size_t in_bytes[5] = {R * M * d * f, R * M * f, R * M * f, R * d * f, R > 0 ? d * d * f : 0};
    if (mmf_outputs_overlap(outs, out_bytes, 7, ins, in_bytes, 5)) return MMF_EINVAL;
  }
  if (a->R == 0) return 0;
  PArgs k{};
  k.centres = a->centres; k.log_a = a->log_a; k.log_b = a->log_b; k.tril = a->scale_tril; k.truth = a->truth;
  k.mean = a->mean; k.covariance = a->covariance; k.log_score = a->log_score; k.pit = a->pit;
  k.spread = a->spread; k.crps = a->crps;
  k.ws = ws_bytes > 0 ? static_cast<double*>(a->workspace) : nullptr;
  k.M = a->M; k.d = a->d; k.nb = p.nb; k.chunk = p.chunk;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (want_rows) {
    const int rc = mmf::with_state_dim(a->d, [&](auto D) { return run_rows<decltype(D)::value>(k, static_cast<unsigned>(a->R), s); });
    if (rc != 0) return rc;
  }
  if (!want_pairs) return 0;
  const unsigned grid = static_cast<unsigned>(a->R) * static_cast<unsigned>(p.nb);
  const int rc = mmf::with_state_dim(a->d, [&](auto D) {
    constexpr int kD = decltype(D)::value;
    return p.ipt == 1 ? run_pairs<kD, 1>(k, grid, p.threads, s) : run_pairs<kD, 2>(k, grid, p.threads, s);
  });
  if (rc != 0 || p.nb == 1) return rc;
  pf_predictive_finish_kernel<<<(a->R + MMF_WAVE - 1) / MMF_WAVE, MMF_WAVE, 0, s>>>(k, a->R);
  MMF_CHECK_LAUNCH();
  return 0;
}
