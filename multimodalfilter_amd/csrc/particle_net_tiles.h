// Tile machinery of the per-particle networks (K2 / K5 / K6): types, blob layout, the register-resident
// 64 x 64 layer chains on v_mfma_f32_32x32x2_f32 (exact fp32) and v_mfma_f32_32x32x16_f16 (f16x3).  Shared by
// particle_net.hip (inference kernels, K6 step kernels, the persistent loop) and particle_net_fused.hip (the fused
// training kernel); every definition is internal to the including translation unit.
#pragma once
#include <hip/hip_fp16.h>

#include <utility>

#include "mmf_common.h"
#include "../../include/mmf_detmath.h"
#include "../../include/mmf_philox.h"

namespace {

enum Kind { kDynamics = 0, kMeasure = 1, kJacobian = 2 };


using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using half8 = __attribute__((ext_vector_type(8))) _Float16;
using half2v = __attribute__((ext_vector_type(2))) _Float16;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

constexpr int kUnits = MMF_UNITS;
constexpr int kW0Cols = 8;                    // first layer padded to K = 8 (state dims, 1, zeros)
constexpr int kHeadRows = MMF_MAX_STATE_DIM + 1;
constexpr int kLayerFloats = kUnits * kUnits;
constexpr float kF16SplitMax = 65504.0f;      // hi = RTZ_f16(x) must stay finite and unsaturated

__host__ __device__ constexpr int num_layers(int n_res) { return 3 + 2 * n_res; }
__host__ __device__ constexpr int off_w0() { return 0; }
__host__ __device__ constexpr int off_layers() { return kUnits * kW0Cols; }
__host__ __device__ constexpr int off_bias(int n_res) { return off_layers() + num_layers(n_res) * kLayerFloats; }
__host__ __device__ constexpr int off_whead(int n_res) { return off_bias(n_res) + num_layers(n_res) * kUnits; }
__host__ __device__ constexpr int off_bhead(int n_res) { return off_whead(n_res) + kHeadRows * kUnits; }
__host__ __device__ constexpr int blob_floats(int n_res) { return off_bhead(n_res) + 8; }

// feature row held by accumulator register r of a 32-row tile, for lane half h
__host__ __device__ constexpr int rowmap(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ------------------------------------------------------------------------------ packing
// f16x3 layers: feature index fed by element i of lane half h in k-step s (16 features per
// step): the rows accumulator registers 8(s&1) .. 8(s&1)+7 of input tile s>>1 hold
__host__ __device__ constexpr int kmap16(int s, int h, int i) {
  return 32 * (s >> 1) + 16 * (s & 1) + (i & 3) + 8 * (i >> 2) + 4 * h;
}

// ---- the dual-use weight image of the fused training kernel (MMF_PREC_F16X3_DUAL): a 64 x 64 layer as 64 rows of
// 256 B = [hi halves of the row | lo halves], 16-byte chunk `ch` of row `row` at byte 256 row + 16 (ch ^ swizzle(row)).
// Inside a row the columns are stored in 4-element runs ordered so that the 8 k-values one lane feeds a k-step of
// v_mfma_f32_32x32x16_f16 (kmap16) are ONE chunk: run index = 4 (c >> 4) + 2 ((c >> 2) & 1) + ((c >> 3) & 1).
// The swizzle makes the forward's row reads (ds_read_b128, lane = row) and the backward's transposed reads
// (ds_read_b64_tr_b16: 4 rows x 16 columns per 16 lanes) both bank-conflict free (checked by enumeration:
// scripts/debug/lds_bank_check.py).
__host__ __device__ constexpr int dual_swizzle(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__host__ __device__ constexpr int dual_off(int row, int ch) { return 256 * row + 16 * (ch ^ dual_swizzle(row)); }

__device__ __forceinline__ unsigned short f16_bits_rz(float x) {
  return __half_as_ushort(__float2half_rn(x));
}

// ------------------------------------------------------------------------------ layer pieces
template <int CT>
struct Act {  // one 64-feature activation for 32*CT particles: [row tile][col tile]
  f32x16 v[2][CT];
};

// quad broadcast of lane (l & ~3) -- the primal column of a Jacobian group
__device__ __forceinline__ float quad_first(float x) {
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x00, 0xf, 0xf, true));
}

// The arithmetic of a Jacobian column group's epilogue (jacobian_outputs), spelled out (explicit fused multiply-adds, no
// implicit contraction): the launch kernel and the persistent EKF loop must produce the same bits whatever surrounds it.
// x' = x + dir sigmoid(gate);  d x'_i / d x_c = d dir_i s + dir_i s (1 - s) d gate + [i == c]
__device__ __forceinline__ float jac_primal(float x, float dir, float sg) {
#pragma clang fp contract(off)
  return __builtin_fmaf(dir, sg, x);
}
__device__ __forceinline__ float jac_tangent(float ddir, float sg, float dir, float dgate, float delta) {
#pragma clang fp contract(off)
  const float u = (dir * (sg * (1.0f - sg))) * dgate;
  return __builtin_fmaf(ddir, sg, u) + delta;
}

template <int CT>
__device__ __forceinline__ void mfma_layer(const float* __restrict__ Wl, const Act<CT>& in,
                                           Act<CT>& acc, int lane) {
  // The blob in LDS is loop-invariant across tiles; without a compiler barrier LICM hoists
  // every layer's fragment reads out of the tile loop (hundreds of VGPRs -> scratch spills).
  asm volatile("" ::: "memory");
#pragma unroll
  for (int t = 0; t < 2; ++t) {
#pragma unroll
    for (int s4 = 0; s4 < 8; ++s4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(Wl + ((t * 8 + s4) * 64 + lane) * 4);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int s = s4 * 4 + ks;
#pragma unroll
        for (int c = 0; c < CT; ++c)
          acc.v[t][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ks], in.v[s >> 4][c][s & 15],
                                                             acc.v[t][c], 0, 0, 0);
      }
    }
  }
}

// acc (+)= bias (LDS, natural order).  `scale` zeroes the bias on Jacobian tangent columns.
template <int CT, bool ADD>
__device__ __forceinline__ void add_bias(const float* __restrict__ bl, Act<CT>& acc, int h, float scale) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(bl + 32 * t + 8 * g + 4 * h);
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (ADD) acc.v[t][c][4 * g + e] += b[e] * scale;
          else acc.v[t][c][4 * g + e] = b[e] * scale;
        }
    }
}

// acc += bias two elements at a time (v_pk_add_f32): the f16x3 path's skip accumulators
template <int CT>
__device__ __forceinline__ void add_bias_packed(const float* __restrict__ bl, Act<CT>& acc, int h) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(bl + 32 * t + 8 * g + 4 * h);
#pragma unroll
      for (int c = 0; c < CT; ++c)
#pragma unroll
        for (int e = 0; e < 4; e += 2) {
          f32x2 v = {acc.v[t][c][4 * g + e], acc.v[t][c][4 * g + e + 1]};
          v += f32x2{b[e], b[e + 1]};
          acc.v[t][c][4 * g + e] = v[0];
          acc.v[t][c][4 * g + e + 1] = v[1];
        }
    }
}

// max(v, 0) as ONE instruction: on accumulator outputs hipcc adds a canonicalising v_max in
// front of fmaxf (2 ops per element).  On the raw bits, max((int)v, 0) is the same function
// for every non-NaN float (negative floats are negative ints; -0.0 -> +0.0) and is a single
// v_max_i32.  (Not inline asm: hipcc pads no MFMA->VALU wait states around asm operands.)
__device__ __forceinline__ float relu1(float v) {
  return __int_as_float(max(__float_as_int(v), 0));
}

// f16x3 layers: ReLU AND saturation at the largest f16 in ONE instruction (v_med3_f32; no canonicalisation is
// emitted in front of the builtin).  An activation beyond the f16 range then splits into hi = 65504 (0x7BFF,
// which the range tracking reports) and a finite residual instead of hi = +inf, lo = -inf, whose products are
// NaN: the failure mode of the mode is a raised flag over FINITE outputs.  v_med3_f32 returns min3 when an
// operand is NaN, i.e. it would swallow a NaN: the two ReLUs that see externally supplied numbers first (the
// first layer on the particle states, the one after the join layer on the per-trajectory term) therefore stay
// NaN-keeping (the first layer's inputs are tested directly, the ReLU after the join layer is relu_keepnan), so
// that a NaN / inf input reaches the next operand split and raises the flag there (0x7C00 / 0x7E00 >= 0x7BFF),
// and every later ReLU clamps whatever those produce.
__device__ __forceinline__ float relu_sat(float v) { return __builtin_amdgcn_fmed3f(v, 0.f, kF16SplitMax); }
// ReLU that keeps a NaN of EITHER sign (relu1 turns a negative NaN into 0), used once per network: IEEE-754 maximum
// propagates a NaN operand and orders -0 below +0, so maximum(v, 0) is v <= 0 ? +0 : v for every number and a NaN for
// every NaN -- ONE v_maximum3_f32 v, v, 0, 0 on gfx950, where the compare + select took two instructions
__device__ __forceinline__ float relu_keepnan(float v) { return __builtin_elementwise_maximum(v, 0.f); }
// signed operands (dynamics trunk entry, Jacobian tangents): saturate both ways; a NaN becomes -65504 (flagged)
__device__ __forceinline__ float clamp_sat(float v) { return __builtin_amdgcn_fmed3f(v, -kF16SplitMax, kF16SplitMax); }

template <int CT, bool JAC, bool SAT = false>
__device__ __forceinline__ void relu(Act<CT>& a, bool primal) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = a.v[t][c][r];
        if (JAC) {
          // tangent columns follow the primal's mask (sub-gradient 0 at 0, as autograd)
          const float pv = quad_first(v);
          const float keep = pv > 0.f ? v : 0.f;
          a.v[t][c][r] = primal ? (SAT ? relu_sat(v) : relu1(v)) : (SAT ? clamp_sat(keep) : keep);
        } else {
          a.v[t][c][r] = SAT ? relu_sat(v) : relu1(v);
        }
      }
}

// saturate a signed activation in place (f16x3: the one operand split that follows no ReLU)
template <int CT>
__device__ __forceinline__ void saturate(Act<CT>& a) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) a.v[t][c][r] = clamp_sat(a.v[t][c][r]);
}

// y = relu(W2 relu(W1 x + b1) + b2 + x), in place in x, h as scratch (resblocks.Linear)
template <int CT, bool JAC>
__device__ __forceinline__ void res_block(const float* __restrict__ lds, int n_res, int l1,
                                          Act<CT>& x, Act<CT>& hbuf, int lane, bool primal) {
  const int h = lane >> 5;
  const float bs = (JAC && !primal) ? 0.f : 1.f;
  add_bias<CT, false>(lds + off_bias(n_res) + l1 * kUnits, hbuf, h, bs);
  mfma_layer<CT>(lds + off_layers() + l1 * kLayerFloats, x, hbuf, lane);
  relu<CT, JAC>(hbuf, primal);
  add_bias<CT, true>(lds + off_bias(n_res) + (l1 + 1) * kUnits, x, h, bs);
  mfma_layer<CT>(lds + off_layers() + (l1 + 1) * kLayerFloats, hbuf, x, lane);
  relu<CT, JAC>(x, primal);
}

// ------------------------------------------------------------------------------ f16x3 path
// Each fp32 operand is split exactly into two halves x = hi + lo + O(2^-22 x) (round-toward-
// zero, so the split never overflows to inf) and a product is evaluated as
// hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 with fp32 accumulation: 3 MFMAs at 16x the
// f32-MFMA rate, ~22-bit operands (measured parity: tests/test_gpu_kernels.py).
template <int CT>
struct SplitAct {
  half8 hi[4][CT], lo[4][CT];  // [k-step][col tile]
};


// hi = RTZ_f16(x); lo = RTZ_f16(x - hi).  `neg_one` is -1.0f held in an SGPR the optimiser
// cannot see through, so that fma(float(hi), neg_one, x) selects v_fma_mix_f32 (f16 source read
// straight from the packed register, f32 arithmetic): 4 instructions per pair instead of
// cvt_pkrtz + 2 cvt_f32_f16 + pk_add + cvt_pkrtz.  (v_fma_mixlo/hi_f16 would fold the final
// conversion as well but issue at half rate on gfx950: scripts/ubench/valu_rate.hip.)
// x - hi is exact in fp32 (the residual has <= 13 significant bits).
using half2v = __attribute__((ext_vector_type(2))) _Float16;
using f32x2v = __attribute__((ext_vector_type(2))) float;
__device__ __forceinline__ void split_pair(float x0, float x1, float neg_one, unsigned& hi, unsigned& lo) {
  const half2v h = __builtin_convertvector(f32x2v{x0, x1}, half2v);  // v_cvt_pk_f16_f32: round to nearest even
  const float r0 = __builtin_fmaf(static_cast<float>(h[0]), neg_one, x0);
  const float r1 = __builtin_fmaf(static_cast<float>(h[1]), neg_one, x1);
  const half2v l = __builtin_convertvector(f32x2v{r0, r1}, half2v);
  hi = __builtin_bit_cast(unsigned, h);
  lo = __builtin_bit_cast(unsigned, l);
}

// Range tracking on the packed hi halves: round-to-nearest maps every |x| >= 65504 to 0x7BFF or to
// +inf (0x7C00), both >= the threshold below.  The running maximum is kept AS f16, with the IEEE-754 maximum of three
// packed operands (v_pk_maximum3_f16): two instructions fold a fragment's four registers (eight halves) into it, half
// of what one two-operand maximum per pair costs (fmaxf on the fp32 values costs 3 ops per pair once canonicalisation
// is counted).  Negative halves and -0 lose against the running value, which starts at +0 -- right after a ReLU; the
// one split that sees signed values (dynamics trunk entry, no ReLU after the join layer) passes SIGNED and masks the
// sign bits first.  A NaN half of either sign propagates through every later link, so the test at the end of the tile
// (range_saturated) looks at the magnitude bits: there the i16 order is the f16 order, with every NaN on top.
using short2v = __attribute__((ext_vector_type(2))) short;
constexpr short kF16Saturated = 0x7BFF;  // also below +inf (0x7C00) and every NaN pattern

// one fragment's four hi registers folded into the running maximum: a three-way maximum beside the chain, one link on it
__device__ __forceinline__ half2v range_fold(half2v amax, unsigned h0, unsigned h1, unsigned h2, unsigned h3) {
  const half2v m = __builtin_elementwise_maximum(
      __builtin_elementwise_maximum(__builtin_bit_cast(half2v, h0), __builtin_bit_cast(half2v, h1)), __builtin_bit_cast(half2v, h2));
  return __builtin_elementwise_maximum(__builtin_elementwise_maximum(amax, m), __builtin_bit_cast(half2v, h3));
}
// Pin the running maximum (no instruction is emitted): left alone, the compiler sinks every v_pk_maximum3_f16 to the
// flag test at the end of the tile and keeps the hi fragments of all seven layers alive for it -- in scratch.
__device__ __forceinline__ void range_pin(half2v& amax) {
  unsigned pin = __builtin_bit_cast(unsigned, amax);
  asm volatile("" : "+v"(pin));
  amax = __builtin_bit_cast(half2v, pin);
}
__device__ __forceinline__ bool range_saturated(half2v amax) {
  const short2v m = __builtin_bit_cast(short2v, __builtin_bit_cast(unsigned, amax) & 0x7fff7fffu);  // a NaN of either sign counts
  return m[0] >= kF16Saturated || m[1] >= kF16Saturated;
}

template <int CT, bool SIGNED = false>
__device__ __forceinline__ void split_act(const Act<CT>& x, SplitAct<CT>& o, float neg_one, half2v& amax) {
#pragma unroll
  for (int tp = 0; tp < 2; ++tp)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        u32x4 h, l;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          unsigned hh, ll;
          split_pair(x.v[tp][c][8 * u + 2 * p], x.v[tp][c][8 * u + 2 * p + 1], neg_one, hh, ll);
          h[p] = hh;
          l[p] = ll;
        }
        constexpr unsigned kMask = SIGNED ? 0x7fff7fffu : 0xffffffffu;
        amax = range_fold(amax, h[0] & kMask, h[1] & kMask, h[2] & kMask, h[3] & kMask);
        o.hi[2 * tp + u][c] = __builtin_bit_cast(half8, h);
        o.lo[2 * tp + u][c] = __builtin_bit_cast(half8, l);
      }
  range_pin(amax);
}

template <int CT>
__device__ __forceinline__ void mfma_layer_f16(const float* __restrict__ Wl, const SplitAct<CT>& in,
                                               Act<CT>& acc, int lane) {
  asm volatile("" ::: "memory");  // see mfma_layer: keep LICM from hoisting the fragment reads
  const unsigned char* base = reinterpret_cast<const unsigned char*>(Wl) + lane * 16;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const half8 ahi = *reinterpret_cast<const half8*>(base + ((t * 4 + s) * 2 + 0) * 1024);
      const half8 alo = *reinterpret_cast<const half8*>(base + ((t * 4 + s) * 2 + 1) * 1024);
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        acc.v[t][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, in.hi[s][c], acc.v[t][c], 0, 0, 0);
        acc.v[t][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ahi, in.lo[s][c], acc.v[t][c], 0, 0, 0);
        acc.v[t][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(alo, in.hi[s][c], acc.v[t][c], 0, 0, 0);
      }
    }
}

// JAC: the tile holds groups of {primal, tangents}: tangent columns take no bias, follow the primal's
// ReLU mask and are signed (their splits mask the sign bits for the range tracking).
template <int CT, bool SIGNED = false, bool JAC = false>
__device__ __forceinline__ void res_block_f16(const float* __restrict__ lds, int n_res, int l1,
                                              Act<CT>& x, Act<CT>& hbuf, SplitAct<CT>& sp, int lane,
                                              float neg_one, half2v& amax, bool primal = true) {
  const int h = lane >> 5;
  const float bs = (JAC && !primal) ? 0.f : 1.f;
  if constexpr (SIGNED) saturate<CT>(x);  // no ReLU in front of this split: saturate the signed values themselves
  split_act<CT, SIGNED || JAC>(x, sp, neg_one, amax);
  add_bias<CT, false>(lds + off_bias(n_res) + l1 * kUnits, hbuf, h, bs);
  mfma_layer_f16<CT>(lds + off_layers() + l1 * kLayerFloats, sp, hbuf, lane);
  relu<CT, JAC, true>(hbuf, primal);
  split_act<CT, JAC>(hbuf, sp, neg_one, amax);
  if constexpr (JAC) add_bias<CT, true>(lds + off_bias(n_res) + (l1 + 1) * kUnits, x, h, bs);
  else add_bias_packed<CT>(lds + off_bias(n_res) + (l1 + 1) * kUnits, x, h);
  mfma_layer_f16<CT>(lds + off_layers() + (l1 + 1) * kLayerFloats, sp, x, lane);
  relu<CT, JAC, true>(x, primal);
}

// ------------------------------------------------------------------ f16x3, pipelined halves
// The 64-particle tile is processed as two 32-particle halves whose layers are offset by half
// a layer: while the matrix pipe runs the 24 MFMAs of one half's layer, the wave issues the
// other half's ReLU / operand split / range tracking in their shadow.  An MFMA holds the
// SIMD's vector issue for 8 of its 32 cycles; up to six of these VALU instructions per MFMA
// are free when they are placed between independent MFMAs (scripts/ubench/mfma_fill.hip), and
// the split needs 4.7.  The order is pinned with sched_group_barrier; left to the scheduler
// (and in the unpipelined kernel, where a layer's VALU depends on its own MFMAs) the two kinds
// of work run back to back.
template <int... Is, class F>
__device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(static_cast<F&&>(f), std::make_integer_sequence<int, N>{});
}

template <int C, bool SAT = true>
__device__ __forceinline__ void relu_half(Act<2>& a) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) a.v[t][C][r] = SAT ? relu_sat(a.v[t][C][r]) : relu_keepnan(a.v[t][C][r]);
}

template <int C>
__device__ __forceinline__ void saturate_half(Act<2>& a) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) a.v[t][C][r] = clamp_sat(a.v[t][C][r]);
}

template <int C, bool SIGNED>
__device__ __forceinline__ void split_half(const Act<2>& x, SplitAct<2>& o, float neg_one, half2v& amax) {
#pragma unroll
  for (int tp = 0; tp < 2; ++tp)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      u32x4 h, l;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        unsigned hh, ll;
        split_pair(x.v[tp][C][8 * u + 2 * p], x.v[tp][C][8 * u + 2 * p + 1], neg_one, hh, ll);
        h[p] = hh;
        l[p] = ll;
      }
      constexpr unsigned kMask = SIGNED ? 0x7fff7fffu : 0xffffffffu;
      amax = range_fold(amax, h[0] & kMask, h[1] & kMask, h[2] & kMask, h[3] & kMask);
      o.hi[2 * tp + u][C] = __builtin_bit_cast(half8, h);
      o.lo[2 * tp + u][C] = __builtin_bit_cast(half8, l);
    }
  range_pin(amax);
}

template <int C, bool ADD>
__device__ __forceinline__ void bias_half(const float* __restrict__ bl, Act<2>& acc, int h) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(bl + 32 * t + 8 * g + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // ADD, the skip + bias, stays one v_add_f32 per element here: in pairs (add_bias_packed's v_pk_add_f32) the
        // compiler takes a third of them apart again under the MFMAs, the run-table kernels grow by four registers and
        // the step measured no faster -- with the pairs slower than without (profiles/k2_vector/README.md)
        if (ADD) acc.v[t][C][4 * g + e] += b[e];
        else acc.v[t][C][4 * g + e] = b[e];
      }
    }
}

// The A fragments (weights) of fragment group g + 1 are read from LDS while group g's MFMAs
// run; the last group of a stage reads the first group of the NEXT stage (`next`), so no stage
// opens with an exposed LDS round trip.
struct FragPair {
  half8 hi, lo;
};
__device__ __forceinline__ FragPair load_frag(const float* __restrict__ Wl, int lane, int g) {
  const unsigned char* base = reinterpret_cast<const unsigned char*>(Wl) + lane * 16 + g * 2048;
  FragPair f;
  f.hi = *reinterpret_cast<const half8*>(base);
  f.lo = *reinterpret_cast<const half8*>(base + 1024);
  return f;
}

template <int C>
__device__ __forceinline__ void mfma_half(const float* __restrict__ Wl, const float* __restrict__ next,
                                          FragPair& cur, const SplitAct<2>& in, Act<2>& acc, int lane) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int g = t * 4 + s;
      const FragPair nxt = g < 7 ? load_frag(Wl, lane, g + 1) : load_frag(next, lane, 0);
      acc.v[t][C] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.hi, in.hi[s][C], acc.v[t][C], 0, 0, 0);
      acc.v[t][C] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.hi, in.lo[s][C], acc.v[t][C], 0, 0, 0);
      acc.v[t][C] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur.lo, in.hi[s][C], acc.v[t][C], 0, 0, 0);
      cur = nxt;
    }
}

// One region's issue order: 8 fragment groups of {2 LDS reads, 3 x (1 MFMA, VPM VALU)}.
template <int VPM>
__device__ __forceinline__ void pin_mfma_valu_interleave() {
#pragma unroll
  for (int g = 0; g < 8; ++g) {
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);  // DS read
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // MFMA
      __builtin_amdgcn_sched_group_barrier(0x002, VPM, 0);  // VALU
    }
  }
}

// ------------------------------------------------------------------------------ the network, piece by piece
// One body for the three forms that must agree bit for bit: particle_net_kernel (particle_net.hip: K2 dynamics, K2
// measurement, K5 Jacobian), small_tile (pf_persistent.inc) and jacobian_tile (ekf_persistent.inc).  A caller keeps
// what is its own -- where the first-layer inputs come from, when the per-trajectory row is requested, where the
// outputs go -- and the PIPE / row-pipelined schedules keep their own trunks; everything else is here, once.

// encoder layer 0, pre-activation: W0 [x; 1] as KS0 = (D + 2) / 2 k-steps; lane (j, h) feeds component 2s + h in b[s]
template <int CT, int KS0>
__device__ __forceinline__ void first_layer(const float* __restrict__ lds, const float (&b)[KS0][CT], Act<CT>& X, int lane) {
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < CT; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) X.v[t][c][r] = 0.f;
#pragma unroll
  for (int s = 0; s < KS0; ++s) {
    const int comp = 2 * s + h;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float w = lds[off_w0() + (32 * t + j) * kW0Cols + comp];
#pragma unroll
      for (int c = 0; c < CT; ++c) X.v[t][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, b[s][c], X.v[t][c], 0, 0, 0);
    }
  }
}

// f16x3: a NaN / inf particle state.  The first layer's exact-f32 MFMAs turn it into NaNs of either sign, and a
// negative NaN would pass the ReLU as 0 -- report the input itself (a handful of compares per tile).
template <int CT, int KS0>
__device__ __forceinline__ void seed_nonfinite(const float (&b)[KS0][CT], half2v& amax) {
  bool bad = false;
#pragma unroll
  for (int s = 0; s < KS0; ++s)
#pragma unroll
    for (int c = 0; c < CT; ++c) bad |= !(fabsf(b[s][c]) <= 3.0e38f);
  if (bad) amax = __builtin_bit_cast(half2v, 0x7fff7fffu);  // a NaN: every later link of the chain keeps it
}

// The join layer's accumulator starts from the hoisted per-trajectory term: the lane's 32 features of one (N, 64) row.
// Request and use are separate so that a caller can ask for the row where the latency hides best.
struct JoinRow {
  f32x4 v[2][4];
};
__device__ __forceinline__ JoinRow load_join_row(const float* __restrict__ row, int lane) {
  JoinRow r;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) r.v[t][g] = *reinterpret_cast<const f32x4*>(row + 32 * t + 8 * g + 4 * (lane >> 5));
  return r;
}
// column tile c of acc = the row; `keep` = false zeroes it (the tangent columns of a Jacobian group take no bias)
template <int CT>
__device__ __forceinline__ void join_init(Act<CT>& acc, int c, const JoinRow& r, bool keep = true) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc.v[t][c][4 * g + e] = keep ? r.v[t][g][e] : 0.f;
}

// The 64 x 64 layers, unpipelined.  On entry X holds the first layer's pre-activation; on exit H holds the trunk's
// output, activated (what the head reads).  `join(acc)` writes the per-trajectory term of the join layer (join_init).
// Same contract as rowpipe_net_f16 (particle_net.hip), which computes the same bits on another schedule.
template <int CT, int NRES, int KIND, int PREC, class Join>
__device__ __forceinline__ void net_unpipelined(const float* __restrict__ lds, Act<CT>& X, Act<CT>& H, Join&& join, int lane,
                                                float neg_one, half2v& amax, bool primal) {
  constexpr bool JAC = KIND == kJacobian, F16 = PREC == MMF_PREC_F16X3;
  SplitAct<F16 ? CT : 0> SP;
  relu<CT, JAC>(X, primal);
  // ---- encoder residual block (layers 0, 1)
  if constexpr (F16) res_block_f16<CT, false, JAC>(lds, NRES, 0, X, H, SP, lane, neg_one, amax, primal);
  else res_block<CT, JAC>(lds, NRES, 0, X, H, lane, primal);
  // ---- join layer (2)
  join(H);
  if constexpr (F16) {
    split_act<CT, JAC>(X, SP, neg_one, amax);
    mfma_layer_f16<CT>(lds + off_layers() + 2 * kLayerFloats, SP, H, lane);
  } else {
    mfma_layer<CT>(lds + off_layers() + 2 * kLayerFloats, X, H, lane);
  }
  if constexpr (KIND == kMeasure) {
    if constexpr (F16) {  // consumes the per-trajectory term: keep a NaN of either sign for the next split to report
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
          for (int r = 0; r < 16; ++r) H.v[t][c][r] = relu_keepnan(H.v[t][c][r]);
    } else {
      relu<CT, JAC>(H, primal);
    }
  }
  // ---- residual trunk: activations now live in H, X is scratch
#pragma unroll
  for (int i = 0; i < NRES; ++i) {
    if constexpr (F16) {
      // without a ReLU after the join layer (dynamics) the trunk's first split sees signed values
      if (i == 0 && KIND != kMeasure) res_block_f16<CT, true, JAC>(lds, NRES, 3, H, X, SP, lane, neg_one, amax, primal);
      else res_block_f16<CT, false, JAC>(lds, NRES, 3 + 2 * i, H, X, SP, lane, neg_one, amax, primal);
    } else {
      res_block<CT, JAC>(lds, NRES, 3 + 2 * i, H, X, lane, primal);
    }
  }
}

// f16x3: an operand beyond the f16 range cannot be split exactly.  Inner activations saturate at 65504 (relu_sat,
// hi = 0x7BFF), a non-finite state or per-trajectory term arrives as hi = inf / NaN (>= 0x7C00) and is clamped by the
// next relu_sat -- either way the tile's outputs stay finite and the flag says they are invalid (engine.check_range).
__device__ __forceinline__ void report_range(int* range_flag, half2v amax) {
  if (range_flag != nullptr && range_saturated(amax)) atomicOr(range_flag, MMF_FLAG_RANGE);
}

// head (64 -> NOUT) on the VALU, bias not included: each lane holds 32 of the 64 features of its columns, the two lane
// halves meet in one shuffle.  Explicit fused multiply-adds in this order: oracle/strict restates the chain.
template <int NRES, int NOUT, int CT>
__device__ __forceinline__ void head(const float* __restrict__ lds, const Act<CT>& H, int lane, float (&out)[NOUT][CT]) {
#pragma unroll
  for (int o = 0; o < NOUT; ++o) {
    float part[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) part[c] = 0.f;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(lds + off_whead(NRES) + o * kUnits + 32 * t + 8 * g + 4 * (lane >> 5));
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
          for (int e = 0; e < 4; ++e) part[c] = __builtin_fmaf(w[e], H.v[t][c][4 * g + e], part[c]);
      }
#pragma unroll
    for (int c = 0; c < CT; ++c) out[o][c] = part[c] + __shfl_xor(part[c], 32);
  }
}

// Dynamics epilogue of one particle: x' = x + (dir + b) sigmoid(gate + b) + scale_tril eps, in two halves.
// dynamics_drift: the noise-free part v0 = x + (dir + b) sigmoid(gate + b) -- a pure function of the particle's state and its
// trajectory's control, so every copy of a resampled ancestor shares it (the run-consuming kernel evaluates it once per run).
// mine: the head's D directions and gate, bh: the head's bias.
template <int D, int PREC>
__device__ __forceinline__ void dynamics_drift(const float (&mine)[D + 1], const float* __restrict__ bh, const float (&x)[D],
                                               float (&v0)[D]) {
  const float gate = mine[D] + bh[D];
  float sg;
  // exact-fp32 mode = the bit-reproducible mode: shared deterministic sigmoid (mmf_detmath.h)
  if constexpr (PREC == MMF_PREC_F32) sg = mmf_det_sigmoid(gate);
  else sg = 1.0f / (1.0f + expf(-gate));
#pragma unroll
  for (int i = 0; i < D; ++i) v0[i] = __builtin_fmaf(mine[i] + bh[i], sg, x[i]);
}
// dynamics_diffuse: the noise chain on top of it, xn = v0 + scale_tril eps.  eps: the caller's noise row, replaced by the
// counter-based draw for (seed, step, traj, particle) when `philox`; tril: D x D, row-major (a pointer or a register array).
template <int D, class Tril>
__device__ __forceinline__ void dynamics_diffuse(const float (&v0)[D], float (&eps)[D], const Tril& tril, bool noisy, bool philox,
                                                 unsigned long long seed, unsigned step, unsigned traj, unsigned particle,
                                                 float (&xn)[D]) {
  if (philox) {
    // counter-based noise: a pure function of (seed, step, trajectory, particle) -- nothing is read
    float z[4];
    mmf_philox_normal4(seed, step, traj, particle, z);
#pragma unroll
    for (int i = 0; i < D; ++i) eps[i] = z[i];
  }
#pragma unroll
  for (int i = 0; i < D; ++i) {
    float v = v0[i];
    if (noisy) {
#pragma unroll
      for (int k = 0; k < D; ++k) v = __builtin_fmaf(tril[i * D + k], eps[k], v);
    }
    xn[i] = v;
  }
}
// both halves: what every kernel that propagates one particle per column calls
template <int D, int PREC, class Tril>
__device__ __forceinline__ void dynamics_update(const float (&mine)[D + 1], const float* __restrict__ bh, const float (&x)[D],
                                                float (&eps)[D], const Tril& tril, bool noisy, bool philox,
                                                unsigned long long seed, unsigned step, unsigned traj, unsigned particle,
                                                float (&xn)[D]) {
  float v0[D];
  dynamics_drift<D, PREC>(mine, bh, x, v0);
  dynamics_diffuse<D>(v0, eps, tril, noisy, philox, seed, step, traj, particle, xn);
}

// Jacobian epilogue of one column of a group {primal, e_1 .. e_3} (role = column & 3): the lane's own D values --
// role 0: x'_i (x: the trajectory's state, read by role 0 only), role c + 1: d x'_i / d x_c.  Every lane of a quad calls it.
template <int D>
__device__ __forceinline__ void jacobian_outputs(const float (&mine)[D + 1], const float* __restrict__ bh, const float (&x)[D],
                                                 int role, float (&own)[D]) {
  float dirp[D];
#pragma unroll
  for (int i = 0; i < D; ++i) dirp[i] = quad_first(mine[i] + bh[i]);
  const float gatep = quad_first(mine[D] + bh[D]);
  const float sg = 1.0f / (1.0f + expf(-gatep));
  const float dgate = mine[D];  // tangent columns carry no bias
#pragma unroll
  for (int i = 0; i < D; ++i) {
    const float prim = jac_primal(x[i], dirp[i], sg);
    const float dv = jac_tangent(mine[i], sg, dirp[i], dgate, (i == role - 1) ? 1.f : 0.f);
    own[i] = role == 0 ? prim : dv;
  }
}

}  // namespace
