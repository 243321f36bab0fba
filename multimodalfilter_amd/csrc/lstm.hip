// The recurrence of the LSTM baselines (crossmodal/door_models/lstm.py:13-100, push_models/lstm.py:13-102): the
// two-layer nn.LSTM(in_dim, 512, 2) of DoorLSTMFilter / PushLSTMFilter over (T, N, in_dim), PyTorch's gate order and
// formulas -- gates i, f, g, o of W_ih x + b_ih + W_hh h + b_hh; c' = f c + i g, h' = o tanh(c').  sigma and tanh are
// mmf_det_sigmoid (absolute error <= 3e-7) and mmf_det_tanh (RELATIVE error <= 3.3e-7, so that cell states of 1e-4 keep
// their digits) of mmf_detmath.h.
//
// Work split.  A workgroup owns 8 hidden units of ONE layer, i.e. the 32 gate rows {i, f, g, o} x 8 of those units, and
// keeps that slice of [W_ih | W_hh] in LDS: 64 workgroups per layer, 128 in all.  Per step it forms the 32 x N gate
// pre-activations as 32-column tiles on v_mfma_f32_32x32x2_f32 (exact fp32 products in both MMF_PRECISION modes: at
// these sizes a step is bound by the exchange between workgroups, ~0.2 GFLOP per step at N = 32, so the f16x3 split
// would buy nothing and only widen the error).  The K axis of a tile is split over the four waves in a FIXED way (wave w:
// k pairs [w K/8, (w+1) K/8), ascending) and the four partial tiles are added as ((p0 + p1) + (p2 + p3)) + (b_ih + b_hh):
// the gate pre-activation does not depend on which form of the loop evaluates it.
//
// Two forms, one kernel (lstm_rounds_kernel): the layers run as a wavefront -- in round r, layer 0 does step r and layer 1
// step r - 1 -- and every hidden vector goes from its producer to its readers as 8-byte {value, tag = step + 1} granules
// (mmf_granule.h), double-buffered by step parity.
//  * persistent: ONE launch for all T + 1 rounds; the weights stay in LDS and the cell state c in registers for the whole
//    sequence; readers spin (bounded, with the abort word) on the granules they need.  Layer 0 may not overwrite the
//    parity slot of h0[s - 2] before every layer-1 workgroup has finished step s - 2: a per-workgroup progress word.
//  * loop of launches: one launch per round (T + 1 launches), the weights staged from the packed blob and c from cT every
//    launch; the granules of the previous round are there when the launch starts, so no spin waits.
// Both run the same device function on the same operands in the same order: the same bits.
#include "mmf_common.h"
#include "mmf_launch.h"
#include "mmf_granule.h"
#include "../../include/mmf_detmath.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kH = MMF_LSTM_HIDDEN;           // 512
constexpr int kUnitsPerWg = 8;                // hidden units of one workgroup
constexpr int kRows = 4 * kUnitsPerWg;        // gate rows of one workgroup (row q = gate * 8 + unit)
constexpr int kWgPerLayer = kH / kUnitsPerWg; // 64
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * MMF_WAVE;   // 256 = 8 units x 32 columns: one (unit, column) cell per thread and tile
constexpr int kTile = 32;                     // columns (trajectories) per MFMA tile
constexpr int kMaxTiles = 8;                  // columns per workgroup and launch: 256
constexpr int kCols = kTile * kMaxTiles;
constexpr int kMaxK = 2 * kH;                 // [W_ih | W_hh] of layer 1; layer 0's in_dim + 512 is capped to it
constexpr int kBatch = 32;                    // k pairs whose operands are requested before their MFMAs (in flight together)
constexpr int kPartStride = kTile + 1;        // padded rows of the partial tiles
constexpr size_t kLdsBytes = (static_cast<size_t>(kRows) * kMaxK + kWaves * kRows * kPartStride) * sizeof(float);
constexpr int kProgressWords = 64;            // one per layer-1 workgroup
constexpr int kSyncHeader = 4 + kProgressWords;  // [abort word, padded to 16 B][progress words]

struct LstmKernelArgs {
  int T, N, in_dim, round_begin, round_end, persistent;
  const float* x;         // (T, N, in_dim)
  const float* h0;        // (2, N, 512)
  const float* c0;        // (2, N, 512)
  float* hT;              // (2, N, 512)
  float* cT;              // (2, N, 512): also the running cell state between the launches of the loop form
  float* h2;              // (T, N, 512)
  const float* packed;    // mmf_lstm_pack
  mmf::Granule* hx;       // [layer][parity][512][N] granules
  unsigned* abort_word;
  unsigned* progress;     // [64]: layer-1 workgroup g has finished its reads of step progress[g] - 1
  int* range_flag;        // MMF_FLAG_GAVE_UP: a hand-off timed out
};

__host__ __device__ inline int layer_k(int layer, int in_dim) { return layer ? 2 * kH : in_dim + kH; }
__host__ __device__ inline size_t layer_weight_offset(int layer, int in_dim) {
  return layer ? static_cast<size_t>(kRows) * kWgPerLayer * layer_k(0, in_dim) : 0;
}
__host__ __device__ inline size_t bias_offset(int in_dim) {
  return static_cast<size_t>(kRows) * kWgPerLayer * (layer_k(0, in_dim) + layer_k(1, in_dim));
}

// B operand (k, column) of layer `layer` at step s: [x_s ; h_{s-1}], granules checked against their tag
struct Operand {
  float v;
  bool ok;
};

__device__ __forceinline__ Operand load_operand(const LstmKernelArgs& a, int layer, int s, int in, int k, int col) {
  Operand o{0.0f, true};
  if (col >= a.N) return o;
  const size_t N = static_cast<size_t>(a.N);
  if (k < in) {
    if (layer == 0) {
      o.v = a.x[(static_cast<size_t>(s) * N + col) * in + k];
    } else {  // layer 0's h at this step
      const mmf::Granule g = mmf::ld_granule(a.hx + ((0 * 2 + (s & 1)) * static_cast<size_t>(kH) + k) * N + col);
      o.v = mmf::granule_value(g);
      o.ok = mmf::granule_tag(g) == static_cast<unsigned>(s + 1);
    }
  } else {
    const int u = k - in;
    if (s == 0) {
      o.v = a.h0[(static_cast<size_t>(layer) * N + col) * kH + u];
    } else {  // this layer's own h of the previous step
      const mmf::Granule g = mmf::ld_granule(a.hx + ((layer * 2 + ((s - 1) & 1)) * static_cast<size_t>(kH) + u) * N + col);
      o.v = mmf::granule_value(g);
      o.ok = mmf::granule_tag(g) == static_cast<unsigned>(s);
    }
  }
  return o;
}

// one failed poll of a wave: true when it must give up (spin budget spent, or another workgroup gave up)
__device__ __forceinline__ bool spin_stop(const LstmKernelArgs& a, unsigned& spins, int lane) {
  __builtin_amdgcn_s_sleep(1);
  return mmf::spin_stop(a.abort_word, spins, lane);
}

// one wave's partial of a 32 x 32 gate tile: the k pairs [kp0, kp1) of the LDS weight slice against the operand columns
// col0 .. col0 + 31; false when a reader gave up
__device__ __forceinline__ bool tile_partial(const LstmKernelArgs& a, const float* w, int layer, int s, int in, int kp0, int kp1,
                                             int col0, int lane, f32x16& acc) {
  const int col = col0 + (lane & 31);
  const int khalf = lane >> 5;
  for (int kb = kp0; kb < kp1; kb += kBatch) {
    float bv[kBatch];
    unsigned spins = 0;
    for (;;) {
      bool ok = true;
#pragma unroll
      for (int i = 0; i < kBatch; ++i) {
        bv[i] = 0.0f;
        if (kb + i < kp1) {
          const Operand o = load_operand(a, layer, s, in, 2 * (kb + i) + khalf, col);
          bv[i] = o.v;
          ok &= o.ok;
        }
      }
      if (__all(ok)) break;
      if (spin_stop(a, spins, lane)) return false;
    }
#pragma unroll
    for (int i = 0; i < kBatch; ++i)
      if (kb + i < kp1) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[(kb + i) * 64 + lane], bv[i], acc, 0, 0, 0);
  }
  return true;
}

__global__ void __launch_bounds__(kThreads) lstm_rounds_kernel(LstmKernelArgs a) {
  extern __shared__ float lds[];
  float* w = lds;                                         // [K/2][2][32]: lane l of k pair kp reads w[kp * 64 + l]
  float* part = lds + static_cast<size_t>(kRows) * kMaxK; // [4 waves][32 rows][33]
  __shared__ int gave_up;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int layer = blockIdx.x / kWgPerLayer, g = blockIdx.x % kWgPerLayer;
  const int in = layer ? kH : a.in_dim;
  const int K = layer_k(layer, a.in_dim);
  const int s_begin = max(0, a.round_begin - layer), s_end = min(a.T, a.round_end - layer);
  if (s_begin >= s_end) return;  // workgroup-uniform
  const int n_base = blockIdx.y * kCols;
  const int tiles = min(kMaxTiles, (a.N - n_base + kTile - 1) / kTile);

  {  // this workgroup's weight slice -> LDS
    const float4* src = reinterpret_cast<const float4*>(a.packed + layer_weight_offset(layer, a.in_dim) + static_cast<size_t>(g) * kRows * K);
    float4* dst = reinterpret_cast<float4*>(w);
    const int n4 = kRows * K / 4;
    for (int i = tid; i < n4; i += kThreads) dst[i] = src[i];
  }
  if (tid == 0) gave_up = 0;
  const int j = tid >> 5, nl = tid & 31;  // the cell of this thread in every tile: unit g * 8 + j, column nl of the tile
  const int u = g * kUnitsPerWg + j;
  const float* bias = a.packed + bias_offset(a.in_dim) + (static_cast<size_t>(layer) * kWgPerLayer + g) * kRows;
  const float b_i = bias[0 * kUnitsPerWg + j], b_f = bias[1 * kUnitsPerWg + j], b_g = bias[2 * kUnitsPerWg + j],
              b_o = bias[3 * kUnitsPerWg + j];
  const size_t N = static_cast<size_t>(a.N);
  float c[kMaxTiles];
#pragma unroll
  for (int ct = 0; ct < kMaxTiles; ++ct) {
    const int n = n_base + ct * kTile + nl;
    c[ct] = 0.0f;
    if (ct < tiles && n < a.N) c[ct] = (s_begin == 0 ? a.c0 : a.cT)[(static_cast<size_t>(layer) * N + n) * kH + u];
  }
  __syncthreads();

  const int kp_per_wave = K / 8;  // K / 2 k pairs over four waves
  for (int s = s_begin; s < s_end; ++s) {
    if (a.persistent && layer == 0 && s >= 2) {
      // the parity slot written below holds h0[s - 2]: every layer-1 workgroup must have finished reading it
      if (wave == 0) {
        unsigned spins = 0;
        for (;;) {
          const unsigned p = __hip_atomic_load(a.progress + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (__all(p >= static_cast<unsigned>(s - 1))) break;
          if (spin_stop(a, spins, lane)) {
            if (lane == 0) gave_up = 1;
            break;
          }
        }
      }
      __syncthreads();
      if (gave_up) break;
    }
#pragma unroll
    for (int ct = 0; ct < kMaxTiles; ++ct) {
      if (ct >= tiles) break;
      const int col0 = n_base + ct * kTile;
      f32x16 acc = {};
      if (!tile_partial(a, w, layer, s, in, wave * kp_per_wave, (wave + 1) * kp_per_wave, col0, lane, acc) && lane == 0) {
        gave_up = 1;
        __hip_atomic_store(a.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // the other waves stop polling
      }
      // C/D map of the 32x32 tile: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        part[(wave * kRows + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * kPartStride + (lane & 31)] = acc[r];
      __syncthreads();
      if (gave_up) break;  // workgroup-uniform after the barrier
      const int n = col0 + nl;
      auto pre = [&](int gate, float b) {
        const int row = gate * kUnitsPerWg + j;
        const float p0 = part[(0 * kRows + row) * kPartStride + nl], p1 = part[(1 * kRows + row) * kPartStride + nl];
        const float p2 = part[(2 * kRows + row) * kPartStride + nl], p3 = part[(3 * kRows + row) * kPartStride + nl];
        return __fadd_rn(__fadd_rn(__fadd_rn(p0, p1), __fadd_rn(p2, p3)), b);
      };
      const float ig = mmf_det_sigmoid(pre(0, b_i)), fg = mmf_det_sigmoid(pre(1, b_f));
      const float gg = mmf_det_tanh(pre(2, b_g)), og = mmf_det_sigmoid(pre(3, b_o));
      const float cn = __builtin_fmaf(fg, c[ct], __fmul_rn(ig, gg));
      const float hn = __fmul_rn(og, mmf_det_tanh(cn));
      c[ct] = cn;
      if (n < a.N) {
        mmf::st_granule(a.hx + ((layer * 2 + (s & 1)) * static_cast<size_t>(kH) + u) * N + n, hn, static_cast<unsigned>(s + 1));
        if (layer == 1) a.h2[(static_cast<size_t>(s) * N + n) * kH + u] = hn;
        if (s == a.T - 1) a.hT[(static_cast<size_t>(layer) * N + n) * kH + u] = hn;
      }
      __syncthreads();  // the partial tiles are rewritten by the next tile
    }
    if (gave_up) break;
    if (a.persistent && layer == 1 && tid == 0)  // every read of step s is done (the barrier above)
      __hip_atomic_store(a.progress + g, static_cast<unsigned>(s + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (gave_up) {
    if (tid == 0) mmf::give_up(a.abort_word, a.range_flag);
    return;
  }
#pragma unroll
  for (int ct = 0; ct < kMaxTiles; ++ct) {
    const int n = n_base + ct * kTile + nl;
    if (ct < tiles && n < a.N) a.cT[(static_cast<size_t>(layer) * N + n) * kH + u] = c[ct];
  }
}

// packed layout (mmf.h): per layer, per workgroup g, [k pair][k & 1][row q = gate * 8 + unit]; then the summed biases
__global__ void lstm_pack_kernel(const float* w_ih0, const float* w_hh0, const float* w_ih1, const float* w_hh1,
                                 const float* b_ih0, const float* b_hh0, const float* b_ih1, const float* b_hh1,
                                 float* packed, int in_dim, size_t total) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t w1 = layer_weight_offset(1, in_dim), bo = bias_offset(in_dim);
  if (i >= bo) {  // (b_ih + b_hh) of layer, workgroup, row
    const size_t e = i - bo;
    const int layer = static_cast<int>(e / (kWgPerLayer * kRows));
    const int g = static_cast<int>(e / kRows % kWgPerLayer), q = static_cast<int>(e % kRows);
    const int grow = (q / kUnitsPerWg) * kH + g * kUnitsPerWg + q % kUnitsPerWg;
    packed[i] = layer ? __fadd_rn(b_ih1[grow], b_hh1[grow]) : __fadd_rn(b_ih0[grow], b_hh0[grow]);
    return;
  }
  const int layer = i >= w1 ? 1 : 0;
  const size_t e = i - (layer ? w1 : 0);
  const int in = layer ? kH : in_dim, K = layer_k(layer, in_dim);
  const size_t per_wg = static_cast<size_t>(kRows) * K;
  const int g = static_cast<int>(e / per_wg);
  const size_t r = e % per_wg;
  const int kp = static_cast<int>(r / 64), kh = static_cast<int>(r / kRows % 2), q = static_cast<int>(r % kRows);
  const int k = 2 * kp + kh;
  const size_t grow = static_cast<size_t>(q / kUnitsPerWg) * kH + g * kUnitsPerWg + q % kUnitsPerWg;
  const float* wi = layer ? w_ih1 : w_ih0;
  const float* wh = layer ? w_hh1 : w_hh0;
  packed[i] = k < in ? wi[grow * in + k] : wh[grow * kH + (k - in)];
}

bool valid_in_dim(int in_dim) { return in_dim >= 8 && in_dim <= kH && in_dim % 8 == 0; }

// workgroups of the persistent form on this device (0: not eligible)
int lstm_persistent_plan(int N) {
  if (N > kCols) return 0;
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return n;
  }();
  // every workgroup resident (one per CU: LDS), a sixteenth of the device left alone
  const int blocks = 2 * kWgPerLayer;
  if (cus - cus / 16 < blocks) return 0;
  return blocks;
}

}  // namespace

extern "C" size_t mmf_lstm_blob_floats(int in_dim) {
  if (!valid_in_dim(in_dim)) return 0;
  return bias_offset(in_dim) + 2 * static_cast<size_t>(4 * kH);
}

extern "C" int mmf_lstm_pack(const float* w_ih0, const float* w_hh0, const float* b_ih0, const float* b_hh0,
                             const float* w_ih1, const float* w_hh1, const float* b_ih1, const float* b_hh1,
                             float* packed, int in_dim, void* stream) {
  if (!w_ih0 || !w_hh0 || !b_ih0 || !b_hh0 || !w_ih1 || !w_hh1 || !b_ih1 || !b_hh1 || !packed) return MMF_EINVAL;
  if (!valid_in_dim(in_dim)) return MMF_EINVAL;
  const size_t total = mmf_lstm_blob_floats(in_dim);
  const int threads = 256;
  lstm_pack_kernel<<<static_cast<unsigned>((total + threads - 1) / threads), threads, 0, static_cast<hipStream_t>(stream)>>>(
      w_ih0, w_hh0, w_ih1, w_hh1, b_ih0, b_hh0, b_ih1, b_hh1, packed, in_dim, total);
  MMF_CHECK_LAUNCH();
  return 0;
}

extern "C" int mmf_lstm_persistent_plan(int N, int T) {
  if (N < 1 || T < 1) return MMF_EINVAL;
  return lstm_persistent_plan(N);
}

extern "C" size_t mmf_lstm_sync_words(int N) {
  if (N < 1) return 0;
  return kSyncHeader + 2 * (2 * 2 * static_cast<size_t>(kH) * N);
}

extern "C" int mmf_lstm_forward(const MmfLstmArgs* a, void* stream) {
  if (!a) return MMF_EINVAL;
  if (a->T < 0 || a->N < 1 || !valid_in_dim(a->in_dim)) return MMF_EINVAL;
  if (!a->h0 || !a->c0 || !a->hT || !a->cT || !a->packed || !a->sync_words) return MMF_EINVAL;
  if (a->T > 0 && (!a->x || !a->h2)) return MMF_EINVAL;  // T = 0: both are empty, and an empty tensor has no address
  if (a->hT == a->h0 || a->cT == a->c0) return MMF_EINVAL;
  if (a->n_sync_words < mmf_lstm_sync_words(a->N)) return MMF_EINVAL;
  if (static_cast<size_t>(a->T) * a->N * kH >= (static_cast<size_t>(1) << 40)) return MMF_ETOOLARGE;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const size_t state_bytes = 2 * static_cast<size_t>(a->N) * kH * sizeof(float);
  if (a->T == 0) {  // nothing to run: the state passes through
    hipError_t e = hipMemcpyAsync(a->hT, a->h0, state_bytes, hipMemcpyDeviceToDevice, hs);
    if (e == hipSuccess) e = hipMemcpyAsync(a->cT, a->c0, state_bytes, hipMemcpyDeviceToDevice, hs);
    return static_cast<int>(e);
  }
  hipError_t e = hipMemsetAsync(a->sync_words, 0, mmf_lstm_sync_words(a->N) * sizeof(unsigned), hs);  // every tag 0
  if (e != hipSuccess) return static_cast<int>(e);
  LstmKernelArgs k{};
  k.T = a->T; k.N = a->N; k.in_dim = a->in_dim;
  k.x = a->x; k.h0 = a->h0; k.c0 = a->c0; k.hT = a->hT; k.cT = a->cT; k.h2 = a->h2; k.packed = a->packed;
  unsigned* words = a->sync_words;
  k.abort_word = words;
  k.progress = words + 4;
  k.hx = reinterpret_cast<mmf::Granule*>(words + kSyncHeader);
  k.range_flag = a->range_flag;
  if (a->persistent) {
    const int blocks = lstm_persistent_plan(a->N);
    const int rc = blocks > 0 ? mmf::resident(lstm_rounds_kernel, blocks, kThreads, kLdsBytes) : MMF_INTERNAL_NOT_RESIDENT;
    if (rc == 0) {
      k.round_begin = 0; k.round_end = a->T + 1; k.persistent = 1;
      return mmf::launch(lstm_rounds_kernel, dim3(blocks, 1), kThreads, kLdsBytes, hs, k);
    }
    if (rc != MMF_INTERNAL_NOT_RESIDENT) return rc;  // a query failed
    // not eligible here: the loop of launches
  }
  const unsigned groups = static_cast<unsigned>((a->N + kCols - 1) / kCols);
  k.persistent = 0;
  for (int r = 0; r <= a->T; ++r) {
    k.round_begin = r; k.round_end = r + 1;
    if (const int rc = mmf::launch(lstm_rounds_kernel, dim3(2 * kWgPerLayer, groups), kThreads, kLdsBytes, hs, k)) return rc;
  }
  return 0;
}
