// Regularised (post-resampling) particle filter: kernel jitter of the set K1 gathered (include/mmf.h: mmf_pf_regularise,
// the definition; Musso, Oudjane & Le Gland 2001, Liu & West's shrinkage).  Upstream torchfilter's ParticleFilter copies the
// survivors of a resampling step verbatim (external dependency of the reference; call site
// /root/reference/crossmodal/eval_helpers.py:139-142): x <- x[a] + h L eps separates them.
//
// A streaming kernel: 8 d bytes per particle with counter noise, 12 d with a noise tensor, a few dozen VALU instructions.
//   - work item = 256 consecutive particles of ONE trajectory = one wave, four particles per lane: the lane's 4 d floats are
//     d 16-byte vectors, contiguous, so a wave's d loads cover one contiguous 1024 d bytes.  A row of M d floats starts at any
//     4-byte boundary (M d need not be a multiple of four), so the vector type is declared 4-byte aligned: global_load_dwordx4
//     / global_store_dwordx4 take it.  The last M mod 4 particles of a row go element by element.
//   - the d x d factor H = h L and the bandwidth are computed once per work item from uniform (scalar) loads and held in
//     SGPRs (v_readfirstlane): no per-particle reload
//   - grid = min(N * ceil(M / 256), 8192) one-wave workgroups, grid-stride: sized by the bytes, not by the trajectories
//     (32 x 4096: 512 waves over the 256 CUs; 8192 waves = 2048 workgroups' worth of 256 threads)
//   - no atomics, no LDS: every particle is read and written by one lane, so two calls and any batch give the same bits
#include <cmath>

#include "mmf_common.h"
#include "../../include/mmf_detmath.h"
#include "../../include/mmf_philox.h"

namespace {

typedef float vec4 __attribute__((ext_vector_type(4), aligned(4)));

constexpr int kLanes = 64, kPerLane = 4, kPerItem = kLanes * kPerLane;
constexpr int kMaxGrid = 8192;  // one-wave workgroups: 32 waves per CU, as many as the registers of the widest form allow

struct RegKernelArgs {
  float* states;
  const float* cov;
  const float* ess;
  const float* mean;
  const int32_t* resampled;
  const float* noise;
  float* bandwidth;
  float* factor;
  unsigned long long seed;
  unsigned step, traj0;
  int M, chunks;
  long long items;
  float scale;
  float floor2[MMF_MAX_STATE_DIM];  // floor_j^2
};

__device__ __forceinline__ float uniform_f32(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// x (D floats of one particle) -> x': an fma chain in ascending k from x_i, or from fma(a, x_i - mu_i, mu_i)
template <int D, bool SHRINK>
__device__ __forceinline__ void jitter(float* x, const float* e, const float (&H)[D][D], const float (&mu)[D], float shrink_a) {
#pragma clang fp contract(off)
  float out[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    float acc = SHRINK ? __builtin_fmaf(shrink_a, x[i] - mu[i], mu[i]) : x[i];
#pragma unroll
    for (int k = 0; k < D; ++k)
      if (k <= i) acc = __builtin_fmaf(H[i][k], e[k], acc);
    out[i] = acc;
  }
#pragma unroll
  for (int i = 0; i < D; ++i) x[i] = out[i];
}

template <int D, int MODE, bool SHRINK>
__global__ __launch_bounds__(kLanes) void pf_regularise_kernel(const RegKernelArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x;
  for (long long w = blockIdx.x; w < a.items; w += gridDim.x) {
    const int n = static_cast<int>(w / a.chunks);
    const int c = static_cast<int>(w - static_cast<long long>(n) * a.chunks);
    // ---- the trajectory's bandwidth and factor: uniform loads, the same instructions in every lane
    const float ess = a.ess[n];
    const bool kept = a.resampled && a.resampled[n] == 0;
    const bool ess_ok = ess - ess == 0.f && ess >= 1.f;  // finite and in K1's range
    float C[D][D];
    bool finite = true;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) {
        C[i][j] = a.cov[static_cast<size_t>(n) * D * D + i * D + j];
        finite = finite && C[i][j] - C[i][j] == 0.f;
      }
    const float h = ess_ok ? a.scale * powf(4.0f / (static_cast<float>(D + 2) * ess), 1.0f / static_cast<float>(D + 4)) : NAN;
    float L[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) L[i][j] = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      float s = C[j][j] + a.floor2[j];
#pragma unroll
      for (int k = 0; k < D; ++k)
        if (k < j) s -= L[j][k] * L[j][k];
      const float dj = s > 0.f ? sqrtf(s) : 0.f;
      L[j][j] = dj;
#pragma unroll
      for (int i = 0; i < D; ++i)
        if (i > j) {
          float t = C[i][j];
#pragma unroll
          for (int k = 0; k < D; ++k)
            if (k < j) t -= L[i][k] * L[j][k];
          L[i][j] = dj > 0.f ? t / dj : 0.f;
        }
    }
    const bool move = ess_ok && finite && !kept;
    float H[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) H[i][j] = move ? uniform_f32(h * L[i][j]) : 0.f;
    if (c == 0 && lane == 0) {
      if (a.bandwidth) a.bandwidth[n] = kept ? 0.f : h;
      if (a.factor)
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
          for (int j = 0; j < D; ++j) a.factor[static_cast<size_t>(n) * D * D + i * D + j] = H[i][j];
    }
    if (!move) continue;  // the row is not written at all
    float mu[D], shrink_a = 1.f;
#pragma unroll
    for (int i = 0; i < D; ++i) mu[i] = 0.f;
    if (SHRINK) {
      shrink_a = uniform_f32(sqrtf(fmaxf(1.0f - h * h, 0.f)));
#pragma unroll
      for (int i = 0; i < D; ++i) mu[i] = a.mean[static_cast<size_t>(n) * D + i];
    }
    // ---- the lane's four particles
    const int m0 = c * kPerItem + lane * kPerLane;
    if (m0 >= a.M) continue;
    const size_t off = (static_cast<size_t>(n) * a.M + m0) * D;
    float* xr = a.states + off;
    const unsigned traj = a.traj0 + static_cast<unsigned>(n);
    if (m0 + kPerLane <= a.M) {
      float x[kPerLane * D], e[kPerLane * D];
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const vec4 v = reinterpret_cast<const vec4*>(xr)[k];
        x[4 * k] = v.x; x[4 * k + 1] = v.y; x[4 * k + 2] = v.z; x[4 * k + 3] = v.w;
      }
      if (MODE == 0) {
#pragma unroll
        for (int k = 0; k < D; ++k) {
          const vec4 v = reinterpret_cast<const vec4*>(a.noise + off)[k];
          e[4 * k] = v.x; e[4 * k + 1] = v.y; e[4 * k + 2] = v.z; e[4 * k + 3] = v.w;
        }
      } else {
#pragma unroll
        for (int p = 0; p < kPerLane; ++p) {
          float z[4];
          mmf_philox_normal4_stream(a.seed, MMF_PHILOX_STREAM_JITTER, a.step, traj, static_cast<unsigned>(m0 + p), z);
#pragma unroll
          for (int i = 0; i < D; ++i) e[p * D + i] = z[i];
        }
      }
#pragma unroll
      for (int p = 0; p < kPerLane; ++p) jitter<D, SHRINK>(x + p * D, e + p * D, H, mu, shrink_a);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        vec4 v;
        v.x = x[4 * k]; v.y = x[4 * k + 1]; v.z = x[4 * k + 2]; v.w = x[4 * k + 3];
        reinterpret_cast<vec4*>(xr)[k] = v;
      }
    } else {
      for (int p = 0; p < a.M - m0; ++p) {  // the last M mod 4 particles of the row
        float x[D], e[D];
#pragma unroll
        for (int i = 0; i < D; ++i) x[i] = xr[p * D + i];
        if (MODE == 0) {
#pragma unroll
          for (int i = 0; i < D; ++i) e[i] = a.noise[off + p * D + i];
        } else {
          float z[4];
          mmf_philox_normal4_stream(a.seed, MMF_PHILOX_STREAM_JITTER, a.step, traj, static_cast<unsigned>(m0 + p), z);
#pragma unroll
          for (int i = 0; i < D; ++i) e[i] = z[i];
        }
        jitter<D, SHRINK>(x, e, H, mu, shrink_a);
#pragma unroll
        for (int i = 0; i < D; ++i) xr[p * D + i] = x[i];
      }
    }
  }
}

template <int D>
int launch_regularise(const RegKernelArgs& k, int mode, bool shrink, unsigned grid, hipStream_t s) {
  if (mode == 0 && !shrink) pf_regularise_kernel<D, 0, false><<<grid, kLanes, 0, s>>>(k);
  else if (mode == 0) pf_regularise_kernel<D, 0, true><<<grid, kLanes, 0, s>>>(k);
  else if (!shrink) pf_regularise_kernel<D, 2, false><<<grid, kLanes, 0, s>>>(k);
  else pf_regularise_kernel<D, 2, true><<<grid, kLanes, 0, s>>>(k);
  MMF_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int mmf_pf_regularise(const MmfPfRegulariseArgs* a, void* stream) {
  if (!a || !a->states || !a->cov || !a->ess) return MMF_EINVAL;
  if (a->N < 0 || a->M < 1 || a->d < 1 || a->d > MMF_MAX_STATE_DIM) return MMF_EINVAL;
  if (a->noise_mode != 0 && a->noise_mode != 2) return MMF_EINVAL;
  if (a->noise_mode == 0 && !a->noise) return MMF_EINVAL;
  if (a->shrink && !a->mean) return MMF_EINVAL;
  if (!(a->scale > 0.f) || !std::isfinite(a->scale)) return MMF_EINVAL;
  for (int i = 0; i < a->d; ++i)
    if (!(a->floor[i] >= 0.f) || !std::isfinite(a->floor[i])) return MMF_EINVAL;
  if (a->N == 0) return 0;
  RegKernelArgs k{};
  k.states = a->states; k.cov = a->cov; k.ess = a->ess; k.mean = a->mean; k.resampled = a->resampled;
  k.noise = a->noise; k.bandwidth = a->bandwidth; k.factor = a->factor;
  k.seed = a->noise_seed; k.step = a->noise_step; k.traj0 = a->noise_traj0;
  k.M = a->M;
  k.chunks = (a->M + kPerItem - 1) / kPerItem;
  k.items = static_cast<long long>(a->N) * k.chunks;
  k.scale = a->scale;
  for (int i = 0; i < MMF_MAX_STATE_DIM; ++i) k.floor2[i] = i < a->d ? a->floor[i] * a->floor[i] : 0.f;
  const unsigned grid = static_cast<unsigned>(k.items < kMaxGrid ? k.items : kMaxGrid);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (a->d) {
    case 1: return launch_regularise<1>(k, a->noise_mode, a->shrink != 0, grid, s);
    case 2: return launch_regularise<2>(k, a->noise_mode, a->shrink != 0, grid, s);
    case 3: return launch_regularise<3>(k, a->noise_mode, a->shrink != 0, grid, s);
    default: return launch_regularise<4>(k, a->noise_mode, a->shrink != 0, grid, s);
  }
}
