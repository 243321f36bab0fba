// Belief maps: the 2-D marginal of the Gaussian product-kernel density of a weighted particle set on a grid of cells
// (include/mmf.h, "Particle-posterior belief maps").  The kernel is separable, so a row's map is Ky^T diag(w) Kx: one
// exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, an fmaf chain) per 32 x 32 cells and two particles, every lane forming its own
// A and B operand with one v_exp_f32 each.  The plain float live weights of pf_summary.h; every sum in a fixed order, no atomics.
//   plan      a workgroup of four waves per row and 64 x 64 block of cells (a 128-cell axis is two blocks); a wave holds the
//             block as 2 x 2 accumulator tiles of 32 x 32.  The tile's columns (the lane's l & 31) are x, the fastest
//             axis of the output, so that a store instruction writes two runs of 128 bytes
//   weights   every workgroup forms max a and sum w over the WHOLE row itself (M loads beside M 64^2 multiply-adds), the sum
//             in double in the order of pf_summary.h; the maps accumulate the unnormalised w_m and 1 / (2 pi hx hy sum w)
//             scales a cell once at the end
//   particles the four waves take four contiguous chunks of ceil(M / 4) particles; a wave stages 64 of its particles at a
//             time through LDS as (x - cx, y - cy, w), a dead particle (and the padding) as zeros: its state is not read
//   pairs     per MFMA of two particles m = m0 + (l >> 5): A = w_m exp2(-1/2 log2(e) ((off_y[l & 31] - ey_m) / hy)^2),
//             B = exp2(-1/2 log2(e) ((off_x[l & 31] - ex_m) / hx)^2), off the cell's offset from the centre: two A and
//             two B exponentials per four MFMAs
//   reduce    the waves meet once, through LDS, one half of the block at a time (32 KiB); wave w adds the four partial
//             tiles of its eight accumulator rows in wave order, scales and stores them

#include <cmath>

#include "pf_summary.h"

namespace {

using namespace mmf::summary;  // the weights, block_max, block_sum and the host's checks

constexpr int kCells = 64;             // cells of a workgroup's block along each axis
constexpr int kTile = 32;              // cells of an MFMA tile along each axis
constexpr int kTiles = kCells / kTile;
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * MMF_WAVE;
constexpr int kStage = MMF_WAVE;       // particles a wave stages at a time
constexpr int kMaxCells = 128;         // cells of a map along each axis at most
constexpr float kHalfLog2e = 0.7213475204444817f;
constexpr double kTwoPi = 6.283185307179586;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct RArgs {
  const float* states;     // (R, M, d)
  const float* log_a;      // (R, M) or null
  const float* log_b;      // (R, M) or null
  const float* center;     // (R, 2)
  const float* bandwidth;  // (R, 2)
  float* density;          // (R, Gy, Gx)
  int M, d, dx, dy, Gx, Gy, bx, by;  // bx, by: the blocks of a map along x and y
  float step_x, step_y;
};

// exp(-1/2 ((off - e) / h)^2): the offset relative to the centre before it is scaled
__device__ __forceinline__ float factor(float off, float e, float ih) {
  const float t = (off - e) * ih;
  return __builtin_amdgcn_exp2f(-(t * t) * kHalfLog2e);
}

__global__ __launch_bounds__(kThreads) void pf_raster_kernel(RArgs a) {
  __shared__ float stage[kWaves][3][kStage];
  __shared__ float part[kWaves][kTiles][16][MMF_WAVE];
  __shared__ double wave_sum[kWaves][1];
  __shared__ float wave_f[kWaves];
  const int tid = threadIdx.x, M = a.M, Gx = a.Gx, Gy = a.Gy;
  const int lane = tid & (MMF_WAVE - 1), wave = tid / MMF_WAVE, col = lane & (kTile - 1), half = lane / kTile;
  const int per_map = a.bx * a.by;
  const int r = blockIdx.x / per_map, b = blockIdx.x - r * per_map;
  const int i0 = (b % a.bx) * kCells, j0 = (b / a.bx) * kCells;  // the block's first cell along x and y
  const int ntx = (min(kCells, Gx - i0) + kTile - 1) / kTile, nty = (min(kCells, Gy - j0) + kTile - 1) / kTile;
  const size_t row = static_cast<size_t>(r) * M;
  float* out = a.density + static_cast<size_t>(r) * Gy * Gx;

  // ---- the row maximum of a_m = log_a[m] + log_b[m] and the sum of the live weights
  float top = -INFINITY;
  for (int m = tid; m < M; m += kThreads) top = fmaxf(top, log_weight(a.log_a, a.log_b, row + m));  // (a NaN is skipped)
  top = block_max(top, wave_f, tid, kWaves);
  double v[1] = {0.0};
  for (int m = tid; m < M; m += kThreads) {
    const float w = live_weight(log_weight(a.log_a, a.log_b, row + m) - top);
    if (w > 0.f) v[0] += static_cast<double>(w);
  }
  block_sum<1>(v, wave_sum, tid, kWaves);
  const double S = v[0];
  const float cx = a.center[2 * static_cast<size_t>(r)], cy = a.center[2 * static_cast<size_t>(r) + 1];
  const float hx = a.bandwidth[2 * static_cast<size_t>(r)], hy = a.bandwidth[2 * static_cast<size_t>(r) + 1];
  // no live particle, a NaN centre, a bandwidth that is not positive and finite: a NaN map (the same in every thread)
  if (!(S > 0.0) || cx != cx || cy != cy || !(hx > 0.f && hx < INFINITY) || !(hy > 0.f && hy < INFINITY)) {
    for (int c = tid; c < kCells * kCells; c += kThreads) {
      const int i = i0 + (c & (kCells - 1)), j = j0 + c / kCells;
      if (i < Gx && j < Gy) out[static_cast<size_t>(j) * Gx + i] = NAN;
    }
    return;
  }
  const float ihx = 1.0f / hx, ihy = 1.0f / hy;
  const float norm = static_cast<float>(1.0 / (kTwoPi * static_cast<double>(hx) * static_cast<double>(hy) * S));

  // ---- this lane's cells: their offsets from the centre, (i - (G - 1) / 2) step
  float offx[kTiles], offy[kTiles];
#pragma unroll
  for (int t = 0; t < kTiles; ++t) {
    offx[t] = (static_cast<float>(i0 + t * kTile + col) - 0.5f * static_cast<float>(Gx - 1)) * a.step_x;
    offy[t] = (static_cast<float>(j0 + t * kTile + col) - 0.5f * static_cast<float>(Gy - 1)) * a.step_y;
  }

  // ---- pairs: this wave's chunk of the particles, 64 at a time through LDS; every wave makes the same number of rounds
  const int chunk = (M + kWaves - 1) / kWaves;
  const int m_end = min(M, (wave + 1) * chunk);
  f32x16 acc[kTiles][kTiles];  // [y tile][x tile]
#pragma unroll
  for (int ty = 0; ty < kTiles; ++ty)
#pragma unroll
    for (int tx = 0; tx < kTiles; ++tx)
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[ty][tx][k] = 0.f;
  for (int s0 = 0; s0 < chunk; s0 += kStage) {
    const int m0 = wave * chunk + s0, m = m0 + lane;
    float w = 0.f, ex = 0.f, ey = 0.f;
    if (m < m_end) {
      w = live_weight(log_weight(a.log_a, a.log_b, row + m) - top);
      if (w > 0.f) {  // (a dead particle is selected away: its state is not read)
        ex = a.states[(row + m) * a.d + a.dx] - cx;
        ey = a.states[(row + m) * a.d + a.dy] - cy;
      }
    }
    __syncthreads();  // the round before this one has been read
    stage[wave][0][lane] = ex;
    stage[wave][1][lane] = ey;
    stage[wave][2][lane] = w;
    __syncthreads();
    const int n = min(kStage, m_end - m0);  // (an odd count: the particle after the last is staged as zeros)
    for (int p = 0; p < n; p += 2) {  // (the same trips in both halves of the wave: an MFMA is the whole wave's)
      const int q = p + half;
      const float qx = stage[wave][0][q], qy = stage[wave][1][q], qw = stage[wave][2][q];
      float kx[kTiles], ky[kTiles];
#pragma unroll
      for (int t = 0; t < kTiles; ++t) {
        kx[t] = factor(offx[t], qx, ihx);
        ky[t] = qw * factor(offy[t], qy, ihy);
      }
#pragma unroll
      for (int ty = 0; ty < kTiles; ++ty)
#pragma unroll
        for (int tx = 0; tx < kTiles; ++tx)
          if (ty < nty && tx < ntx) acc[ty][tx] = __builtin_amdgcn_mfma_f32_32x32x2f32(ky[ty], kx[tx], acc[ty][tx], 0, 0, 0);
    }
  }

  // ---- the waves meet: one y half of the block at a time; wave w takes x tile w & 1 and accumulator rows 8 (w >> 1) .. + 8
#pragma unroll
  for (int ty = 0; ty < kTiles; ++ty) {
    __syncthreads();  // the half before this one has been read
#pragma unroll
    for (int tx = 0; tx < kTiles; ++tx)
#pragma unroll
      for (int k = 0; k < 16; ++k) part[wave][tx][k][lane] = acc[ty][tx][k];
    __syncthreads();
    const int tx = wave & 1;
    if (ty >= nty || tx >= ntx) continue;
    const int i = i0 + tx * kTile + col;
    for (int k = 8 * (wave >> 1); k < 8 * (wave >> 1) + 8; ++k) {
      float s = part[0][tx][k][lane];
      for (int w = 1; w < kWaves; ++w) s += part[w][tx][k][lane];
      const int j = j0 + ty * kTile + (k & 3) + 8 * (k >> 2) + 4 * half;  // the C/D layout of the 32 x 32 MFMA
      if (i < Gx && j < Gy) out[static_cast<size_t>(j) * Gx + i] = s * norm;
    }
  }
}

}  // namespace

extern "C" int mmf_pf_raster(const MmfPfRasterArgs* a, void* stream) {
  if (!a || check_rows(a->states, a->R, a->M, a->d)) return MMF_EINVAL;
  if (a->d < 2 || !a->center || !a->bandwidth || !a->density) return MMF_EINVAL;
  for (int k = 0; k < 2; ++k) {
    if (a->dims[k] < 0 || a->dims[k] >= a->d) return MMF_EINVAL;
    if (a->cells[k] < 2 || a->cells[k] > kMaxCells) return MMF_EINVAL;
    if (!(a->step[k] > 0.f && a->step[k] < INFINITY)) return MMF_EINVAL;  // (a NaN fails)
  }
  if (a->dims[0] == a->dims[1]) return MMF_EINVAL;
  const int bx = (a->cells[0] + kCells - 1) / kCells, by = (a->cells[1] + kCells - 1) / kCells;
  if (const int rc = check_size(a->R, a->M, bx * by)) return rc;
  {
    const size_t R = a->R, M = a->M, d = a->d, f = sizeof(float);
    const void* outs[1] = {a->density};
    const size_t out_bytes[1] = {R * a->cells[0] * a->cells[1] * f};
    if (outputs_alias(a->states, a->log_a, a->log_b, nullptr, R, M, d, outs, out_bytes)) return MMF_EINVAL;
    const void* ins[2] = {a->center, a->bandwidth};
    const size_t in_bytes[2] = {R * 2 * f, R * 2 * f};
    if (mmf_outputs_overlap(outs, out_bytes, 1, ins, in_bytes, 2)) return MMF_EINVAL;
  }
  if (a->R == 0) return 0;
  RArgs k{};
  k.states = a->states; k.log_a = a->log_a; k.log_b = a->log_b; k.center = a->center; k.bandwidth = a->bandwidth;
  k.density = a->density;
  k.M = a->M; k.d = a->d; k.dx = a->dims[0]; k.dy = a->dims[1]; k.Gx = a->cells[0]; k.Gy = a->cells[1]; k.bx = bx; k.by = by;
  k.step_x = a->step[0]; k.step_y = a->step[1];
  const unsigned grid = static_cast<unsigned>(a->R) * static_cast<unsigned>(bx * by);
  pf_raster_kernel<<<grid, kThreads, 0, static_cast<hipStream_t>(stream)>>>(k);
  MMF_CHECK_LAUNCH();
  return 0;
}
