// Backward-simulation particle smoothing: whole trajectories drawn from the joint smoothing distribution of a filter run's
// history (include/mmf.h, "backward-simulation particle smoothing").  Where the marginal smoother of pf_smooth_marginal.hip
// re-weights every particle of step t against every particle of step t + 1, a draw conditions on the ONE particle it chose at
// step t + 1: M transition densities per draw and step, and a categorical draw over them.  Two kernels behind one C call:
//   simulate  one launch for all steps over (draw block, trajectory): a workgroup owns kSimDraws draws of one trajectory and
//             walks t = T - 1 .. 0 itself (step t needs the draw's own j_{t+1}); no workgroup talks to another
//   moments   one workgroup per (step, trajectory): mean and covariance over the S draws
// A step of the simulate kernel: a thread owns a contiguous segment of ceil(M / kSimThreads) rows; the rows (F_t[i], log2 of
// the weight) stream through LDS in chunks of kSimRows rows per thread; per draw the thread keeps an online (max, sum) over
// its segment, rescaled once per chunk.  The workgroup then takes the maximum per draw, scans the rescaled sums in thread
// order, finds the first thread whose inclusive sum exceeds u * total, and that thread's wave re-walks the one segment (a
// row per lane, a wave scan) for j_t.  One density per (row, draw, step) plus one segment per draw.

#include <climits>
#include <cmath>

#include "pf_smooth_math.h"

namespace {

using namespace mmf::smooth_math;

constexpr int kSimThreads = 256;
constexpr int kSimWaves = kSimThreads / MMF_WAVE;
#ifndef MMF_SIM_DRAWS
#define MMF_SIM_DRAWS 2        // (the build sets nothing; profiles/simulate_smooth/ was measured by compiling this file with 1 .. 16)
#endif
constexpr int kSimDraws = MMF_SIM_DRAWS;  // B: draws of a workgroup, the tuning constant (DESIGN.md has the values measured)
constexpr int kSimRows = 4;    // rows of a thread's segment staged per chunk, at most: a chunk is kSimThreads * kSimRows rows, whatever M is
static_assert(kSimDraws <= MMF_WAVE && kSimDraws <= kSimThreads, "one thread per draw sets a step up");

struct SimulateArgs {
  const float* states;    // (T, N, M, D)
  const float* pred;      // (T - 1, N, M, D)
  const float* loglik;    // (T, N, M)
  const float* logw;      // (T, N, M) or null
  const float* tril;      // (D, D)
  const float* uniforms;  // (T, N, S)
  int* indices;           // (T, N, S)
  float* traj;            // (T, N, S, D)
  float* mean;            // (T, N, D)
  float* cov;             // (T, N, D, D) or null
  int T, N, M, S;
};

// inclusive sum scan across the 64 lanes, in the data movement of mmf::wave_inclusive_scan_u32: one fixed tree
__device__ __forceinline__ float wave_inclusive_scan_f32(float v) {
#pragma clang fp contract(off)
  v = v + mmf::dpp_f32<mmf::kDppRowShr1>(0.f, v);
  v = v + mmf::dpp_f32<mmf::kDppRowShr2>(0.f, v);
  v = v + mmf::dpp_f32<mmf::kDppRowShr4>(0.f, v);
  v = v + mmf::dpp_f32<mmf::kDppRowShr8>(0.f, v);
  v = v + mmf::dpp_f32<mmf::kDppRowBcast15, 0xa>(0.f, v);
  v = v + mmf::dpp_f32<mmf::kDppRowBcast31, 0xc>(0.f, v);
  return v;
}

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

// ---- simulate: kSimDraws joint draws of trajectory blockIdx.y, all steps
// ROWS: the rows of a segment staged per chunk, 1, 2 or kSimRows: min(kSimRows, the segment rounded up to a power of two)
template <int D, int ROWS>
__global__ __launch_bounds__(kSimThreads) void pf_simulate_kernel(SimulateArgs a) {
  constexpr int B = kSimDraws;
  constexpr int kSimPitch = kSimThreads + ROWS;  // float4s between two rows of one thread in LDS: conflict-free both ways
  __shared__ float4 rows[ROWS * kSimPitch];              // (F_t[i], w) for D < 4; F_t[i] for D == 4
  __shared__ float rows_w[D == 4 ? ROWS * kSimPitch : 1];
  __shared__ float4 tgt[B];                                   // X_{t+1}[j_{t+1}] of every draw (zeros at the last step)
  __shared__ float unif[B];
  __shared__ int chosen[B];                                   // j_{t+1}, or -1: the draw is dead
  __shared__ int sel[B], last[B];                             // the thread whose segment holds u * total / the last one with weight
  __shared__ float amax_w[kSimWaves];
  __shared__ float top_w[B][kSimWaves], sum_w[B][kSimWaves];
  const int tid = threadIdx.x, lane = tid & (MMF_WAVE - 1), wave = tid >> 6;
  const int n = blockIdx.y, s0 = blockIdx.x * B, M = a.M, S = a.S, T = a.T;
  const int seg = (M + kSimThreads - 1) / kSimThreads;       // rows of a thread's segment: thread k owns [k seg, (k + 1) seg)
  const size_t nm = static_cast<size_t>(a.N) * M;
  float W[D][D];
  whitener<D>(a.tril, W);                                     // NaN where L is unusable: every v is NaN then, every draw dead
  if (tid < B) {
    chosen[tid] = 0;
    tgt[tid] = make_float4(0.f, 0.f, 0.f, 0.f);               // the last step: x - f = 0, v is the weight itself
  }
  for (int t = T - 1; t >= 0; --t) {
    const size_t row0 = static_cast<size_t>(t) * nm + static_cast<size_t>(n) * M;
    const float* ll = a.loglik + row0;
    const float* lw = a.logw ? a.logw + row0 : nullptr;
    const float* F = t < T - 1 ? a.pred + row0 * D : nullptr;
    // the step's largest log-weight
    float amax = -INFINITY;
    for (int i = tid; i < M; i += kSimThreads) amax = fmaxf(amax, log_weight(ll, lw, i));
    amax = mmf::wave_max(amax);
    if (lane == 0) amax_w[wave] = amax;
    if (tid < B) {
      const int s = s0 + tid;
      unif[tid] = s < S ? a.uniforms[(static_cast<size_t>(t) * a.N + n) * S + s] : 0.f;
      sel[tid] = INT_MAX;
      last[tid] = -1;
    }
    __syncthreads();
    amax = amax_w[0];
#pragma unroll
    for (int w = 1; w < kSimWaves; ++w) amax = fmaxf(amax, amax_w[w]);
    // the pass: an online (max, sum) per draw over this thread's segment
    float top[B], sum[B];
#pragma unroll
    for (int b = 0; b < B; ++b) { top[b] = -INFINITY; sum[b] = 0.f; }
    for (int k0 = 0; k0 < seg; k0 += ROWS) {
      __syncthreads();  // the previous chunk has been consumed
#pragma unroll
      for (int q = 0; q < ROWS; ++q) {
        const int slot = q * kSimThreads + tid, owner = slot / ROWS, r = slot % ROWS;
        const int i = owner * seg + k0 + r;
        float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        float w = -INFINITY;
        if (k0 + r < seg && i < M) w = log2_weight(log_weight(ll, lw, i), amax);
        if (F && w != -INFINITY) {  // a dead row may hold anything: it is not read
#pragma unroll
          for (int c = 0; c < D; ++c) v[c] = F[static_cast<size_t>(i) * D + c];
        }
        v[D] = w;
        rows[r * kSimPitch + owner] = make_float4(v[0], v[1], v[2], v[3]);
        if (D == 4) rows_w[r * kSimPitch + owner] = w;
      }
      __syncthreads();
      float f[ROWS][D], w[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const float4 x = rows[r * kSimPitch + tid];
        const float v[5] = {x.x, x.y, x.z, x.w, D < 4 ? 0.f : rows_w[r * kSimPitch + tid]};
#pragma unroll
        for (int c = 0; c < D; ++c) f[r][c] = v[c];
        w[r] = v[D];
      }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        const float4 x4 = tgt[b];  // every lane reads the same address: a broadcast
        const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
        float x[D], v[ROWS];
#pragma unroll
        for (int c = 0; c < D; ++c) x[c] = xs[c];
        float hi = top[b];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          v[r] = minus_sq_dist<D>(w[r], x, f[r], W);
          hi = fmaxf(hi, v[r]);  // (a NaN is not a maximum; it reaches the sum through its own exp2)
        }
        const float ref = rescale_ref(hi);
        float acc = sum[b] * exp2_hw(top[b] - ref);
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc = acc + exp2_hw(v[r] - ref);
        sum[b] = acc;
        top[b] = hi;
      }
    }
    // the workgroup's maximum per draw
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const float m = mmf::wave_max(top[b]);
      if (lane == 0) top_w[b][wave] = m;
    }
    __syncthreads();
    float gtop[B], part[B], incl[B], excl[B], goal[B];
    bool dead[B];
#pragma unroll
    for (int b = 0; b < B; ++b) {
      float m = top_w[b][0];
#pragma unroll
      for (int w = 1; w < kSimWaves; ++w) m = fmaxf(m, top_w[b][w]);
      gtop[b] = m;
      part[b] = top[b] == -INFINITY ? sum[b] : sum[b] * exp2_hw(top[b] - m);  // (no maximum: the sum is 0, or NaN)
      incl[b] = wave_inclusive_scan_f32(part[b]);
      if (lane == MMF_WAVE - 1) sum_w[b][wave] = incl[b];
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < B; ++b) {
#pragma clang fp contract(off)
      float before = 0.f, total = 0.f;  // the waves' totals in wave order: every thread takes the same sums
#pragma unroll
      for (int w = 0; w < kSimWaves; ++w) {
        if (w == wave) before = total;
        total = total + sum_w[b][w];
      }
      incl[b] = before + incl[b];
      const float prev = mmf::dpp_f32<mmf::kDppWaveShr1>(before, incl[b]);  // the inclusive sum of thread tid - 1, bit for bit
      excl[b] = lane == 0 ? before : prev;
      dead[b] = chosen[b] < 0 || !(total > 0.f) || !(total < INFINITY);
      goal[b] = unif[b] * total;
      // the first thread WITH WEIGHT whose inclusive sum exceeds the goal (sums of different trees are monotone only up to
      // rounding: a thread without weight is never taken); one integer atomic per wave
      const unsigned long long over = __ballot(!dead[b] && part[b] > 0.f && incl[b] > goal[b]);
      if (over != 0 && lane == 0) atomicMin(&sel[b], wave * MMF_WAVE + __builtin_ctzll(over));
    }
    __syncthreads();
    bool none = false;
#pragma unroll
    for (int b = 0; b < B; ++b) none = none || (!dead[b] && sel[b] == INT_MAX);
    if (none) {  // (uniform over the workgroup) rounding left u * total at or above every sum: the last thread with weight
#pragma unroll
      for (int b = 0; b < B; ++b)
        if (!dead[b] && sel[b] == INT_MAX && part[b] > 0.f) atomicMax(&last[b], tid);
      __syncthreads();
    }
    // the re-walk: the wave of the chosen thread takes its segment a row per lane; a dead draw goes to wave b mod waves
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const bool fallback = !dead[b] && sel[b] == INT_MAX;
      const int owner = dead[b] ? -1 : (fallback ? last[b] : sel[b]);
      if ((owner < 0 ? b % kSimWaves : owner >> 6) != wave) continue;  // (uniform over the wave)
      int j = -1;
      if (owner >= 0) {
        const float rest = fallback ? INFINITY : __shfl(goal[b] - excl[b], owner & (MMF_WAVE - 1));
        const float4 x4 = tgt[b];
        const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
        float x[D];
#pragma unroll
        for (int c = 0; c < D; ++c) x[c] = xs[c];
        const int first = owner * seg;
        int lastpos = -1;
        float base = 0.f;
        for (int q0 = 0; q0 < seg && j < 0; q0 += MMF_WAVE) {
          const int i = first + q0 + lane;
          float f[D], w = -INFINITY;
#pragma unroll
          for (int c = 0; c < D; ++c) f[c] = 0.f;
          if (q0 + lane < seg && i < M) w = log2_weight(log_weight(ll, lw, i), amax);
          if (F && w != -INFINITY) {
#pragma unroll
            for (int c = 0; c < D; ++c) f[c] = F[static_cast<size_t>(i) * D + c];
          }
          const float p = exp2_hw(minus_sq_dist<D>(w, x, f, W) - gtop[b]);
          const float c = base + wave_inclusive_scan_f32(p);
          const unsigned long long hit = __ballot(c > rest && p > 0.f), pos = __ballot(p > 0.f);  // (never a row without weight)
          if (hit) j = first + q0 + __builtin_ctzll(hit);
          if (pos) lastpos = first + q0 + 63 - __builtin_clzll(pos);
          base = lane_value(c, MMF_WAVE - 1);
        }
        if (j < 0) j = lastpos;                      // rounding: the last row of the segment with weight
        if (j < 0) j = min(first, M - 1);            // (not reached: the segment's sum was positive) the reads stay in range
      }
      if (lane == 0) {
        const int s = s0 + b;
        const size_t out = (static_cast<size_t>(t) * a.N + n) * S + s;
        float x[4] = {0.f, 0.f, 0.f, 0.f};
        if (j >= 0) {
          const float* X = a.states + (row0 + j) * D;
#pragma unroll
          for (int c = 0; c < D; ++c) x[c] = X[c];
        }
        if (s < S) {
          a.indices[out] = j;
#pragma unroll
          for (int c = 0; c < D; ++c) a.traj[out * D + c] = j >= 0 ? x[c] : NAN;
        }
        chosen[b] = j;
        tgt[b] = make_float4(x[0], x[1], x[2], x[3]);
      }
    }
    __syncthreads();  // every wave has read sel / last before the next step resets them
  }
}

// ---- moments over the draws: the pivot form of the other smoothers with equal weights; the pivot is draw 0
template <int D>
__global__ __launch_bounds__(kMomentThreads) void pf_simulate_moments_kernel(SimulateArgs a) {
#pragma clang fp contract(off)
  constexpr int NS = moment_sums(D);
  __shared__ float partial[kMomentSums * kMomentWaves];
  __shared__ float total[kMomentSums];
  const int tid = threadIdx.x, t = blockIdx.x, n = blockIdx.y, S = a.S;
  const size_t out = static_cast<size_t>(t) * a.N + n;
  const float* X = a.traj + out * S * D;
  float p[D], acc[NS];
#pragma unroll
  for (int c = 0; c < D; ++c) p[c] = X[c];
#pragma unroll
  for (int v = 0; v < NS; ++v) acc[v] = 0.f;
  // every draw weighs one (the multiplication by it is exact); a dead draw: NaN, and so is the step
  for (int s = tid; s < S; s += kMomentThreads) pivot_accumulate<D>(acc, 1.f, X + static_cast<size_t>(s) * D, p);
  block_sums(acc, partial, total, kMomentWaves, kMomentWaves, tid);
  __syncthreads();
  write_moments<D>(a.mean, a.cov, out, tid, p, total, static_cast<float>(S));
}

}  // namespace

extern "C" int mmf_pf_smooth_simulate(const MmfPfSmoothSimulateArgs* a, void* stream) {
  if (!a || !a->states_steps || !a->loglik_steps || !a->scale_tril || !a->uniforms || !a->indices || !a->trajectories || !a->mean)
    return MMF_EINVAL;
  if (a->T < 0 || a->N < 0 || a->M < 1 || a->d < 1 || a->S < 1) return MMF_EINVAL;
  if (a->T >= 2 && !a->pred_steps) return MMF_EINVAL;
  if (!sizes_in_range(a->M, a->N, a->d) || a->S > 65535) return MMF_ETOOLARGE;
  if (a->N == 0 || a->T == 0) return 0;
  SimulateArgs k{};
  k.states = a->states_steps; k.pred = a->pred_steps; k.loglik = a->loglik_steps; k.logw = a->logw_in_steps;
  k.tril = a->scale_tril; k.uniforms = a->uniforms; k.indices = a->indices; k.traj = a->trajectories;
  k.mean = a->mean; k.cov = a->cov;
  k.T = a->T; k.N = a->N; k.M = a->M; k.S = a->S;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int N = a->N, blocks = (a->S + kSimDraws - 1) / kSimDraws;
  return mmf::with_state_dim(a->d, [&](auto D) -> int {
    constexpr int d = decltype(D)::value;
    const int seg = (a->M + kSimThreads - 1) / kSimThreads;
    const int rc = seg >= 3   ? mmf::launch(pf_simulate_kernel<d, kSimRows>, dim3(blocks, N), kSimThreads, 0, s, k)
                   : seg == 2 ? mmf::launch(pf_simulate_kernel<d, 2>, dim3(blocks, N), kSimThreads, 0, s, k)
                              : mmf::launch(pf_simulate_kernel<d, 1>, dim3(blocks, N), kSimThreads, 0, s, k);
    if (rc) return rc;
    return mmf::launch(pf_simulate_moments_kernel<d>, dim3(a->T, N), kMomentThreads, 0, s, k);
  });
}
