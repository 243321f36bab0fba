// Rauch-Tung-Striebel smoothing of an extended Kalman filter's recorded run (include/mmf.h, "RTS smoothing"): from the
// filtered beliefs (m_t, S_t), the Jacobians A_t and predictions x^_{t+1} of the T - 1 transitions and the constant
// process-noise factor L,
//   P-_{t+1} = A_t S_t A_t^T + L L^T      G_t = S_t A_t^T (P-_{t+1})^-1
//   m^s_t = m_t + G_t (m^s_{t+1} - x^_{t+1})      P^s_t = S_t + G_t (P^s_{t+1} - P-_{t+1}) G_t^T
// One trajectory per lane, the d x d algebra of K3 (ekf_algebra.h) in registers.  Three kernels behind one C call, the
// serial one holding only what is serial:
//   gains      one thread per (t, n) of the (T - 1) N transitions: P- and G, the inversion included
//   sweep      one lane per trajectory, t = T - 2 .. 0: (m^s, P^s) carried in registers, step t - 1's operands loaded
//              before step t's arithmetic (they do not depend on the chain); the two-slice moments from the same pass
//   lag sweep  one thread per (t, n): from the filtered belief of step min(t + lag, T - 1) at most `lag` steps back
// Both sweeps call rts_step, so a lag >= T - 1 gives the full sweep's bits.
// HBM bytes per trajectory-step (d = 3): gains read A 36 + S 36 and write G 36 + P- 36; the sweep reads m 12 + S 36 +
// G 36 + P- 36 + x^ 12 and writes 48: ~330 B for ~0.5 kFLOP -- launch- and latency-bound at every size a filter runs at.
#include "ekf_algebra.h"

namespace {

using namespace mmf_ekf;

struct SmoothArgs {
  const float* mu;        // (T, N, D)
  const float* Sigma;     // (T, N, D, D)
  const float* A;         // (T - 1, N, D, D)
  const float* mu_pred;   // (T - 1, N, D)
  const float* q_tril;    // (D, D)
  float* mu_s;            // (T, N, D)
  float* Sigma_s;         // (T, N, D, D)
  float* gain;            // (T - 1, N, D, D)
  float* Sigma_pred;      // (T - 1, N, D, D)
  float* resid_mean;      // (T - 1, N, D) or null
  float* resid_m2;        // (T - 1, N, D, D) or null
  int T, N, lag;
};

template <int D>
__device__ __forceinline__ void load_vec(const float* p, float (&v)[D]) {
#pragma unroll
  for (int i = 0; i < D; ++i) v[i] = p[i];
}

template <int D>
__device__ __forceinline__ void store_vec(float* p, const float (&v)[D]) {
#pragma unroll
  for (int i = 0; i < D; ++i) p[i] = v[i];
}

// ---- gains: P-_{t+1} and G_t of every transition; nothing here depends on the sweep
template <int D>
__global__ __launch_bounds__(256) void ekf_smooth_gains_kernel(SmoothArgs a) {
#pragma clang fp contract(off)
  const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;  // t * N + n
  if (row >= static_cast<size_t>(a.T - 1) * a.N) return;
  const Mat<D> At = load_mat<D>(a.A + row * D * D);
  const Mat<D> St = load_mat<D>(a.Sigma + row * D * D);
  const Mat<D> L = load_mat<D>(a.q_tril);
  const Mat<D> AS = matmul<D>(At, St);
  Mat<D> Pp = matmul_nt<D>(AS, At);
  const Mat<D> Q = matmul_nt<D>(L, L);
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) Pp.a[i][j] += Q.a[i][j];
  const Mat<D> SAt = matmul_nt<D>(St, At);
  const Mat<D> G = matmul<D>(SAt, inverse<D>(Pp));
  store_mat<D>(a.gain + row * D * D, G);
  store_mat<D>(a.Sigma_pred + row * D * D, Pp);
}

// what one backward step reads that does not depend on the chain
template <int D, bool MOMENTS>
struct StepOperands {
  float m[D], xp[D];
  Mat<D> S, G, Pp, A;  // A: moments only
};

template <int D, bool MOMENTS>
__device__ __forceinline__ StepOperands<D, MOMENTS> load_operands(const SmoothArgs& a, int t, int n) {
  const size_t row = static_cast<size_t>(t) * a.N + n;
  StepOperands<D, MOMENTS> o;
  load_vec<D>(a.mu + row * D, o.m);
  load_vec<D>(a.mu_pred + row * D, o.xp);
  o.S = load_mat<D>(a.Sigma + row * D * D);
  o.G = load_mat<D>(a.gain + row * D * D);
  o.Pp = load_mat<D>(a.Sigma_pred + row * D * D);
  if constexpr (MOMENTS) o.A = load_mat<D>(a.A + row * D * D);
  return o;
}

// one backward step: (ms, Ps) hold the smoothed belief of step t + 1 on entry and that of step t on return
template <int D>
__device__ __forceinline__ void rts_step(const float (&mt)[D], const Mat<D>& St, const Mat<D>& G, const Mat<D>& Pp,
                                         const float (&xp)[D], float (&ms)[D], Mat<D>& Ps) {
#pragma clang fp contract(off)
  float dm[D];
  Mat<D> dP;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    dm[i] = ms[i] - xp[i];
#pragma unroll
    for (int j = 0; j < D; ++j) dP.a[i][j] = Ps.a[i][j] - Pp.a[i][j];
  }
  const Mat<D> GdP = matmul<D>(G, dP);
  const Mat<D> GdPGt = matmul_nt<D>(GdP, G);
#pragma unroll
  for (int i = 0; i < D; ++i) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) s = __builtin_fmaf(G.a[i][j], dm[j], s);
    ms[i] = mt[i] + s;
#pragma unroll
    for (int j = 0; j < D; ++j) Ps.a[i][j] = St.a[i][j] + GdPGt.a[i][j];
  }
}

// two-slice moments of the linearised residual r_t = x_{t+1} - x^_{t+1} - A_t (x_t - m_t), C_t = G_t P^s_{t+1}:
//   e = m^s_{t+1} - x^_{t+1} - A_t (m^s_t - m_t);   M2 = P^s_{t+1} - A C - (A C)^T + A P^s_t A^T + e e^T
template <int D>
__device__ __forceinline__ void transition_moments(const StepOperands<D, true>& o, const float (&ms1)[D], const Mat<D>& Ps1,
                                                   const float (&ms0)[D], const Mat<D>& Ps0, float (&e)[D], Mat<D>& M2) {
#pragma clang fp contract(off)
  float dm[D];
#pragma unroll
  for (int i = 0; i < D; ++i) dm[i] = ms0[i] - o.m[i];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) s = __builtin_fmaf(o.A.a[i][j], dm[j], s);
    e[i] = (ms1[i] - o.xp[i]) - s;
  }
  const Mat<D> AC = matmul<D>(o.A, matmul<D>(o.G, Ps1));
  const Mat<D> APA = matmul_nt<D>(matmul<D>(o.A, Ps0), o.A);
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j)
      M2.a[i][j] = __builtin_fmaf(e[i], e[j], ((Ps1.a[i][j] - AC.a[i][j]) - AC.a[j][i]) + APA.a[i][j]);
}

// ---- full sweep: one lane per trajectory; T == 1 copies the filtered belief
template <int D, bool MOMENTS>
__global__ __launch_bounds__(64) void ekf_smooth_sweep_kernel(SmoothArgs a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  float ms[D];
  const size_t last = static_cast<size_t>(a.T - 1) * a.N + n;
  load_vec<D>(a.mu + last * D, ms);
  Mat<D> Ps = load_mat<D>(a.Sigma + last * D * D);
  store_vec<D>(a.mu_s + last * D, ms);
  store_mat<D>(a.Sigma_s + last * D * D, Ps);
  if (a.T < 2) return;
  StepOperands<D, MOMENTS> cur = load_operands<D, MOMENTS>(a, a.T - 2, n);
  for (int t = a.T - 2; t >= 0; --t) {
    StepOperands<D, MOMENTS> nxt = cur;
    if (t > 0) nxt = load_operands<D, MOMENTS>(a, t - 1, n);  // in flight during this step's arithmetic
    float ms1[D];
    Mat<D> Ps1;
    if constexpr (MOMENTS) {
#pragma unroll
      for (int i = 0; i < D; ++i) ms1[i] = ms[i];
      Ps1 = Ps;
    }
    rts_step<D>(cur.m, cur.S, cur.G, cur.Pp, cur.xp, ms, Ps);
    const size_t row = static_cast<size_t>(t) * a.N + n;
    store_vec<D>(a.mu_s + row * D, ms);
    store_mat<D>(a.Sigma_s + row * D * D, Ps);
    if constexpr (MOMENTS) {
      float e[D];
      Mat<D> M2;
      transition_moments<D>(cur, ms1, Ps1, ms, Ps, e, M2);
      store_vec<D>(a.resid_mean + row * D, e);
      store_mat<D>(a.resid_m2 + row * D * D, M2);
    }
    cur = nxt;
  }
}

// ---- fixed-lag sweep: E[x_t | y_1..min(t + lag, T - 1)] for every (t, n), each walking at most `lag` steps back
template <int D>
__global__ __launch_bounds__(256) void ekf_smooth_lag_kernel(SmoothArgs a) {
  const size_t row = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;  // t * N + n
  if (row >= static_cast<size_t>(a.T) * a.N) return;
  const int t = static_cast<int>(row / a.N), n = static_cast<int>(row % a.N);
  const int end = (a.lag < a.T - 1 - t) ? t + a.lag : a.T - 1;
  const size_t from = static_cast<size_t>(end) * a.N + n;
  float ms[D];
  load_vec<D>(a.mu + from * D, ms);
  Mat<D> Ps = load_mat<D>(a.Sigma + from * D * D);
  for (int s = end - 1; s >= t; --s) {
    const StepOperands<D, false> o = load_operands<D, false>(a, s, n);
    rts_step<D>(o.m, o.S, o.G, o.Pp, o.xp, ms, Ps);
  }
  store_vec<D>(a.mu_s + row * D, ms);
  store_mat<D>(a.Sigma_s + row * D * D, Ps);
}

template <int D>
int launch(const SmoothArgs& a, hipStream_t s) {
  const size_t transitions = static_cast<size_t>(a.T - 1) * a.N, rows = static_cast<size_t>(a.T) * a.N;
  if (transitions > 0) {
    ekf_smooth_gains_kernel<D><<<static_cast<unsigned>((transitions + 255) / 256), 256, 0, s>>>(a);
    MMF_CHECK_LAUNCH();
  }
  if (a.lag >= 0) {
    ekf_smooth_lag_kernel<D><<<static_cast<unsigned>((rows + 255) / 256), 256, 0, s>>>(a);
  } else if (a.resid_mean != nullptr) {
    ekf_smooth_sweep_kernel<D, true><<<(a.N + 63) / 64, 64, 0, s>>>(a);
  } else {
    ekf_smooth_sweep_kernel<D, false><<<(a.N + 63) / 64, 64, 0, s>>>(a);
  }
  MMF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int mmf_ekf_smooth(const MmfEkfSmoothArgs* args, void* stream) {
  if (!args) return MMF_EINVAL;
  const int T = args->T, N = args->N, d = args->d;
  if (T < 0 || N < 0 || d < 1 || d > MMF_MAX_STATE_DIM) return MMF_EINVAL;
  if (!args->mu || !args->Sigma || !args->q_tril || !args->mu_s || !args->Sigma_s) return MMF_EINVAL;
  if (T >= 2 && (!args->A || !args->mu_pred || !args->gain || !args->Sigma_pred)) return MMF_EINVAL;
  if ((args->resid_mean == nullptr) != (args->resid_m2 == nullptr)) return MMF_EINVAL;
  if (args->resid_mean != nullptr && args->lag >= 0) return MMF_EINVAL;
  // the kernels index rows and transitions in size_t and their grids in 32 bits of blocks of 256
  if (static_cast<int64_t>(T) * N > 0x7fffffffLL - 256) return MMF_ETOOLARGE;
  const size_t rows = static_cast<size_t>(T) * N, trans = T >= 2 ? static_cast<size_t>(T - 1) * N : 0;
  const size_t v = sizeof(float) * d, m = v * d;
  const void* ins[] = {args->mu, args->Sigma, args->A, args->mu_pred, args->q_tril};
  const size_t in_bytes[] = {rows * v, rows * m, trans * m, trans * v, m};
  const void* outs[] = {args->mu_s, args->Sigma_s, args->gain, args->Sigma_pred, args->resid_mean, args->resid_m2};
  const size_t out_bytes[] = {rows * v, rows * m, trans * m, trans * m, trans * v, trans * m};
  for (int o = 0; o < 6; ++o) {
    for (int i = 0; i < 5; ++i)
      if (mmf_bytes_overlap(outs[o], out_bytes[o], ins[i], in_bytes[i])) return MMF_EINVAL;
    for (int p = 0; p < o; ++p)
      if (mmf_bytes_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p])) return MMF_EINVAL;
  }
  if (T == 0 || N == 0) return 0;
  SmoothArgs a;
  a.mu = args->mu; a.Sigma = args->Sigma; a.A = args->A; a.mu_pred = args->mu_pred; a.q_tril = args->q_tril;
  a.mu_s = args->mu_s; a.Sigma_s = args->Sigma_s; a.gain = args->gain; a.Sigma_pred = args->Sigma_pred;
  a.resid_mean = args->resid_mean; a.resid_m2 = args->resid_m2;
  a.T = T; a.N = N; a.lag = args->lag;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (d) {
    case 1: return launch<1>(a, s);
    case 2: return launch<2>(a, s);
    case 3: return launch<3>(a, s);
    default: return launch<4>(a, s);
  }
}
