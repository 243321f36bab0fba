// Particle smoothing: ancestry trace of a filter run's history and the weighted moments along it (include/mmf.h,
// "particle smoothing").  torchfilter's ParticleFilter leaves particle_states / particle_log_weights to the caller after
// each step and reports the filtered estimate only; this is the estimate E[x_t | y_1..s] a caller builds on the kept sets.
// One workgroup per (trajectory, endpoint).  The endpoint's weights are computed once and stay in LDS; every thread keeps
// the path indices b of its PER particles in registers and chases them one step back with one 4-byte gather per particle
// (b = A_t[b]); a step that is written gathers the rows X_t[b] and reduces the pivot-form sums in a fixed order.

#include <cmath>

#include "pf_smooth_math.h"

namespace {

using namespace mmf::smooth_math;  // log_weight, first_max, the pivot-form moment pieces

constexpr int kSmoothThreads = 1024;            // most threads of a workgroup: 16 waves
constexpr int kSmoothWaves = kSmoothThreads / MMF_WAVE;
constexpr int kSmoothSums = moment_sums(MMF_MAX_STATE_DIM);
constexpr int kSmoothMaxPer = 40;               // particles per thread at the largest M the LDS plan takes

// dynamic LDS, in 4-byte words: weights (M) | bitmap (ceil(M / 32)) | partial sums (kSmoothSums x waves) | totals
// (kSmoothSums + 2, padded to 16) | pivot row (4) | wave maxima (waves) | their indices (waves) | 4 words: [1] the count of distinct particles, [0] unused
struct SmoothLds {
  size_t weights, bitmap, partial, total, pivot, wmax, widx, misc, end;
};
SmoothLds smooth_lds(int M) {
  SmoothLds l;
  const size_t m = M > 0 ? static_cast<size_t>(M) : 0;
  l.weights = 0;
  l.bitmap = l.weights + m;
  l.partial = l.bitmap + (m + 31) / 32;
  l.total = l.partial + static_cast<size_t>(kSmoothSums + 1) * kSmoothWaves;
  l.pivot = l.total + 16;
  l.wmax = l.pivot + 4;
  l.widx = l.wmax + kSmoothWaves;
  l.misc = l.widx + kSmoothWaves;
  l.end = (l.misc + 4) * sizeof(float);
  return l;
}

struct SmoothArgs {
  const float* states;    // (T, N, M, D)
  const float* loglik;    // (T, N, M)
  const float* logw;      // (T, N, M) or null
  const float* logw0;     // (N, M) or null
  const int32_t* anc;     // (T, N, M) or null
  float* mean;            // (T, N, D)
  float* cov;             // (T, N, D, D) or null
  int32_t* unique;        // (T, N) or null
  int T, N, M, lag;       // lag <= T - 1
  unsigned o_bitmap, o_partial, o_total, o_pivot, o_wmax, o_widx, o_misc;  // LDS offsets in words
};

// a weight below zero marks a path whose log-weight is -inf: it contributes nothing and is not counted
constexpr float kDeadPath = -1.0f;

template <int D, int PER>
__global__ __launch_bounds__(kSmoothThreads) void pf_smooth_kernel(SmoothArgs a) {
#pragma clang fp contract(off)
  extern __shared__ float smem[];
  float* const w_lds = smem;
  unsigned* const bitmap = reinterpret_cast<unsigned*>(smem + a.o_bitmap);
  float* const partial = smem + a.o_partial;
  float* const total = smem + a.o_total;
  float* const pivot = smem + a.o_pivot;
  float* const wmax = smem + a.o_wmax;
  int* const widx = reinterpret_cast<int*>(smem + a.o_widx);
  int* const misc = reinterpret_cast<int*>(smem + a.o_misc);  // [1] count of distinct particles

  constexpr int NS = moment_sums(D);
  const int tid = threadIdx.x, threads = blockDim.x, lane = tid & (MMF_WAVE - 1), wave = tid >> 6, waves = threads >> 6;
  const int n = blockIdx.y, M = a.M;
  const int s = a.lag + static_cast<int>(blockIdx.x);  // the endpoint: lag .. T - 1
  const bool last = s == a.T - 1;                      // the last endpoint writes every step it passes
  const int t_stop = s - a.lag;                        // >= 0: endpoints that would stop before step 0 are not launched
  const size_t nm = static_cast<size_t>(a.N) * M;
  const size_t row0 = static_cast<size_t>(n) * M;

  // ---- the endpoint's weights: a = loglik + logw_in, first maximum, e = exp(a - max)
  const float* ll = a.loglik + s * nm + row0;
  const float* lw = a.logw ? a.logw + s * nm + row0 : (s == 0 && a.logw0 ? a.logw0 + row0 : nullptr);
  float mx = -INFINITY;
  int pm = 0x7fffffff;  // the pivot path: the first highest-weight one
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int m = k * threads + tid;
    if (m < M) {
      const float av = log_weight(ll, lw, m);
      if (av > mx) { mx = av; pm = m; }
    }
  }
  first_max(mx, pm, wmax, widx, tid, waves, M);
  float ssum = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const int m = k * threads + tid;
    if (m < M) {
      const float av = log_weight(ll, lw, m);  // read again (L2) instead of kept: PER registers fewer
      const bool dead = av == -INFINITY;
      const float e = dead ? 0.f : expf(av - mx);
      w_lds[m] = dead ? kDeadPath : e;
      ssum = ssum + e;
    }
  }
  ssum = mmf::wave_sum(ssum);
  if (lane == 0) partial[NS * kSmoothWaves + wave] = ssum;
  __syncthreads();
  if (tid == 0) {
    float S = 0.f;
    for (int w = 0; w < waves; ++w) S = S + partial[NS * kSmoothWaves + w];
    total[NS] = S;
  }
  // (the first barrier of the first written step orders total[NS] and w_lds before their readers)

  int b[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) b[k] = min(k * threads + tid, M - 1);

  for (int t = s; t >= t_stop; --t) {
    if (last || t == t_stop) {
      const float* X = a.states + (static_cast<size_t>(t) * nm + row0) * D;
      // the pivot: the row the first highest-weight path sits on at this step
#pragma unroll
      for (int k = 0; k < PER; ++k)
        if (k * threads + tid == pm) {
#pragma unroll
          for (int c = 0; c < D; ++c) pivot[c] = X[static_cast<size_t>(b[k]) * D + c];
        }
      for (int i = tid; i < (M + 31) / 32; i += threads) bitmap[i] = 0u;
      if (tid == 0) misc[1] = 0;
      __syncthreads();
      float p[D], acc[NS];
#pragma unroll
      for (int c = 0; c < D; ++c) p[c] = pivot[c];
#pragma unroll
      for (int v = 0; v < NS; ++v) acc[v] = 0.f;
#pragma unroll
      for (int k = 0; k < PER; ++k) {
        const int m = k * threads + tid;
        if (m < M) {
          const float e = w_lds[m];
          if (e >= 0.f) atomicOr(&bitmap[b[k] >> 5], 1u << (b[k] & 31));
          // a path of zero weight contributes exactly zero, whatever its row holds
          if (e > 0.f) pivot_accumulate<D>(acc, e, X + static_cast<size_t>(b[k]) * D, p);
        }
      }
      block_sums(acc, partial, total, kSmoothWaves, waves, tid);
      if (a.unique) {
        int c = 0;
        for (int i = tid; i < (M + 31) / 32; i += threads) c += __popc(bitmap[i]);
        if (c) atomicAdd(&misc[1], c);
      }
      __syncthreads();
      const size_t out = static_cast<size_t>(t) * a.N + n;
      write_moments<D>(a.mean, a.cov, out, tid, p, total, total[NS]);
      if (a.unique && tid == 0) a.unique[out] = misc[1];
      __syncthreads();  // the next written step reuses pivot, bitmap, partial and total
    }
    if (t > t_stop && a.anc) {
      const int32_t* A = a.anc + (static_cast<size_t>(t - 1) * nm + row0);
#pragma unroll
      for (int k = 0; k < PER; ++k) b[k] = min(max(A[b[k]], 0), M - 1);  // a corrupted index gives a wrong number, not a fault
    }
  }
}

template <int D, int PER>
int launch_smooth(const SmoothArgs& k, int endpoints, int threads, size_t lds, hipStream_t s) {
  return mmf::launch(pf_smooth_kernel<D, PER>, dim3(endpoints, k.N), threads, lds, s, k);
}

}  // namespace

extern "C" size_t mmf_pf_smooth_lds_bytes(int M) { return smooth_lds(M).end; }

extern "C" int mmf_pf_smooth(const MmfPfSmoothArgs* a, void* stream) {
  if (!a || !a->states_steps || !a->loglik_steps || !a->mean) return MMF_EINVAL;
  if (a->T < 0 || a->N < 0 || a->M < 1 || a->d < 1 || a->d > MMF_MAX_STATE_DIM || a->lag < 0) return MMF_EINVAL;
  const SmoothLds l = smooth_lds(a->M);
  if (a->M > 65536 || l.end > mmf::kLdsPerCu || a->M > kSmoothMaxPer * kSmoothThreads) return MMF_ETOOLARGE;
  if (a->N == 0 || a->T == 0) return 0;
  if (a->N > 65535) return MMF_ETOOLARGE;  // trajectories are the grid's y
  SmoothArgs k{};
  k.states = a->states_steps; k.loglik = a->loglik_steps; k.logw = a->logw_in_steps; k.logw0 = a->logw_in0;
  k.anc = a->indices_steps; k.mean = a->mean; k.cov = a->cov; k.unique = a->unique;
  k.T = a->T; k.N = a->N; k.M = a->M;
  k.lag = a->lag < a->T - 1 ? a->lag : a->T - 1;  // the full smoother: the last endpoint alone walks everything
  k.o_bitmap = static_cast<unsigned>(l.bitmap); k.o_partial = static_cast<unsigned>(l.partial);
  k.o_total = static_cast<unsigned>(l.total); k.o_pivot = static_cast<unsigned>(l.pivot);
  k.o_wmax = static_cast<unsigned>(l.wmax); k.o_widx = static_cast<unsigned>(l.widx); k.o_misc = static_cast<unsigned>(l.misc);
  const int endpoints = a->T - k.lag;  // s = lag .. T - 1: every launched workgroup writes at least one step
  const int threads = a->M >= kSmoothThreads ? kSmoothThreads : (a->M + MMF_WAVE - 1) / MMF_WAVE * MMF_WAVE;
  const int per = (a->M + threads - 1) / threads;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return mmf::with_state_dim(a->d, [&](auto D) {
    constexpr int d = decltype(D)::value;
    if (per <= 1) return launch_smooth<d, 1>(k, endpoints, threads, l.end, s);
    if (per <= 4) return launch_smooth<d, 4>(k, endpoints, threads, l.end, s);
    if (per <= 16) return launch_smooth<d, 16>(k, endpoints, threads, l.end, s);
    return launch_smooth<d, kSmoothMaxPer>(k, endpoints, threads, l.end, s);
  });
}
