// K6 (per-particle networks): training-mode forward that stashes every layer's input, and the
// data path of the backward pass.  Included at the end of particle_net.hip (shares its tile
// machinery).  Exact fp32 products on the f32 MFMA; 32-particle tiles (CT = 1).
//
// Replaces autograd through R1 / R2 over N*M rows (the reference trains through
// torchfilter.train.* on /root/reference/crossmodal/door_models/dynamics.py:102-134 and
// door_models/pf.py:63-107; ~20 saved (R, 64) activations per network and as many rocBLAS
// launches each way).  The backward of the residual MLP is the same residual network run in
// reverse with transposed weights, ReLU masks in place of ReLUs and no biases:
//     block  a -> h = relu(W1 a + b1) -> a' = relu(a + W2 h + b2)
//     dz2 = da' * [a' > 0];  dh = W2^T dz2;  dz1 = dh * [h > 0];  da = dz2 + W1^T dz1
// so `packed_t` is a blob packed by mmf_pack_particle_net from the TRANSPOSED layer weights and
// the chain reuses mfma_layer unchanged.  The masks travel as BITS (8 B per particle and layer, written
// by the forward next to the stash): the backward data path reads no activation at all.  The kernel writes the pre-activation gradients dz_l
// of every layer; everything that reduces over particles (weight and bias gradients
// dW_l = dz_l^T in_l, the per-trajectory bias gradient, d states = dz_in W_in) is a plain
// GEMM / column sum over the two stashes, left to the caller (rocBLAS through torch.mm).
//
// Stash layouts: `stash` (NL + 1, R, 64): [l] = input of 64x64 layer l (post-ReLU), [NL] = input
// of the head.  `dz` (NL + 1, R, 64): [l] = gradient w.r.t. layer l's pre-activation output,
// [NL] = gradient w.r.t. the first (d -> 64) layer's pre-activation.

#include "particle_net_train_common.h"

namespace {

struct TrainArgs {
  const float* packed;     // forward: f32 blob; backward: blob of the transposed layers
  const float* head_w;     // backward: (NOUT, 64) head weights
  const float* states;     // forward: (R, D)
  const float* traj_bias;  // forward: (N, 64)
  const float* stash_in;   // backward
  const float* d_out;      // backward: (R, NOUT)
  float* stash;            // forward out
  unsigned* mask;          // forward out / backward in: (NL + 1, R, 2) ReLU sign bits of the stashed activations
  float* out;              // forward out: (R, NOUT) head outputs incl. bias
  float* dz;               // backward out
  float* d_states;         // backward out: (R, D) = dz_in W_in
  float* dz_scale;         // COMPACT backward out: (NL + 1, R) row magnitudes of dz
  int R, M, D;
};

// QUAD (K6 for K5, the dynamics Jacobian): rows come in groups of four {primal x, tangents e_1..e_3};
// tangent rows take no bias (first layer, every 64x64 layer, the per-trajectory term, the head) and
// follow the primal row's ReLU masks (DPP quad broadcast), exactly as the forward-mode kernel K5
// does -- so their head outputs are the columns of d(dir, gate)/dx and the same backward kernel
// (masks read from the primal's stash rows) yields the Jacobian's dependence on the weights.
// (Round 4's three-product f16 variants of this kernel and of the backward below -- recompute / transposed layers in the
// forward pass's arithmetic, three passes over f16 buffers -- were superseded by the fused kernel of particle_net_fused.hip
// in round 5 and deleted in round 6; profiles/r05/bench_train_fused_ab.txt keeps their timings.)
template <int D, int NRES, int KIND, bool QUAD = false, bool COMPACT = false>
__global__ __launch_bounds__(512, 2) void particle_net_train_fwd_kernel(TrainArgs a) {
  const int kThreads = blockDim.x, kWavesPerBlock = kThreads / MMF_WAVE;  // 512, or 256 for small launches
  constexpr int NOUT = (KIND == kMeasure) ? 1 : D + 1;
  constexpr int NL = num_layers(NRES);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  {
    const float4* src = reinterpret_cast<const float4*>(a.packed);
    float4* dst = reinterpret_cast<float4*>(lds);
    if (kThreads == 512) mmf::stage_to_lds<blob_floats(NRES) / 4, 512, 4>(src, dst, threadIdx.x);
    else mmf::stage_to_lds<blob_floats(NRES) / 4, 256, 4>(src, dst, threadIdx.x);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int wave_global = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int waves_total = gridDim.x * kWavesPerBlock;
  const int ntiles = (a.R + 31) / 32;
  const size_t layer_stride = static_cast<size_t>(a.R) * kUnits;
  const size_t mask_stride = static_cast<size_t>(a.R) * 2;
  auto layer = [&](const float* W, const Act<1>& in, Act<1>& out) { mfma_layer<1>(W, in, out, lane); };
  auto keep = [&](size_t layer_off, const Act<1>& v, int row, bool valid) {
    if constexpr (COMPACT) stash_store_h(reinterpret_cast<_Float16*>(a.stash) + layer_off, v, row, valid, h);
    else stash_store(a.stash + layer_off, v, row, valid, h);
  };

  for (int tile = wave_global; tile < ntiles; tile += waves_total) {
    asm volatile("" ::: "memory");
    const int base = tile * 32;
    const bool valid = base + j < a.R;
    const int row = valid ? base + j : a.R - 1;
    const int traj = row / a.M;
    const bool primal = !QUAD || (row & 3) == 0;
    const float bs = primal ? 1.f : 0.f;

    // the per-trajectory term of the join layer (read where it is used: the exact-fp32 layers have no 32 registers to
    // spare for requesting it at the top of the tile -- they would spill)
    f32x4 tbv[2][4];
    const float* tb = a.traj_bias + static_cast<size_t>(traj) * kUnits + 4 * h;
    Act<1> X, H;
    zero_act(X);
    constexpr int KS0 = (D + 2) / 2;
#pragma unroll
    for (int s = 0; s < KS0; ++s) {
      const int comp = 2 * s + h;
      const float b = comp < D ? a.states[static_cast<size_t>(row) * D + comp] : (comp == D ? bs : 0.f);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const float w = lds[off_w0() + (32 * t + j) * kW0Cols + comp];
        X.v[t][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, b, X.v[t][0], 0, 0, 0);
      }
    }
    relu<1, QUAD>(X, primal);
    keep(0, X, row, valid);
    mask_store(a.mask, X, row, valid, h);                                   // input of layer 0

    add_bias<1, false>(lds + off_bias(NRES), H, h, bs);
    layer(lds + off_layers(), X, H);
    relu<1, QUAD>(H, primal);
    keep(layer_stride, H, row, valid);
    mask_store(a.mask + mask_stride, H, row, valid, h);                    // input of layer 1
    add_bias<1, true>(lds + off_bias(NRES) + kUnits, X, h, bs);
    layer(lds + off_layers() + kLayerFloats, H, X);
    relu<1, QUAD>(X, primal);
    keep(2 * layer_stride, X, row, valid);
    mask_store(a.mask + 2 * mask_stride, X, row, valid, h);                // input of the join layer

#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        tbv[t][g] = *reinterpret_cast<const f32x4*>(tb + 32 * t + 8 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) H.v[t][0][4 * g + e] = tbv[t][g][e] * bs;
      }
    layer(lds + off_layers() + 2 * kLayerFloats, X, H);
    if (KIND == kMeasure) relu<1, QUAD>(H, primal);
    keep(3 * layer_stride, H, row, valid);
    mask_store(a.mask + 3 * mask_stride, H, row, valid, h);                // input of layer 3

#pragma unroll
    for (int i = 0; i < NRES; ++i) {
      const int l1 = 3 + 2 * i;
      add_bias<1, false>(lds + off_bias(NRES) + l1 * kUnits, X, h, bs);
      layer(lds + off_layers() + l1 * kLayerFloats, H, X);
      relu<1, QUAD>(X, primal);
      keep((l1 + 1) * layer_stride, X, row, valid);
      mask_store(a.mask + (l1 + 1) * mask_stride, X, row, valid, h);
      add_bias<1, true>(lds + off_bias(NRES) + (l1 + 1) * kUnits, H, h, bs);
      layer(lds + off_layers() + (l1 + 1) * kLayerFloats, X, H);
      relu<1, QUAD>(H, primal);
      keep((l1 + 2) * layer_stride, H, row, valid);
      mask_store(a.mask + (l1 + 2) * mask_stride, H, row, valid, h);       // .. [NL] = head input
    }
    static_assert(3 + 2 * NRES == NL, "stash slots");

    // head: each lane holds 32 of the 64 features of its particle
    const float* bh = lds + off_bhead(NRES);
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
      float part = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const f32x4 w = *reinterpret_cast<const f32x4*>(lds + off_whead(NRES) + o * kUnits + 32 * t + 8 * g + 4 * h);
#pragma unroll
          for (int e = 0; e < 4; ++e) part += w[e] * H.v[t][0][4 * g + e];
        }
      part += __shfl_xor(part, 32);
      if (valid && h == 0) a.out[static_cast<size_t>(row) * NOUT + o] = part + bs * bh[o];
    }
  }
}

template <int NRES, int KIND, int NOUT, bool QUAD = false, bool COMPACT = false>
__global__ __launch_bounds__(512, 2) void particle_net_train_bwd_kernel(TrainArgs a) {
  const int kThreads = blockDim.x, kWavesPerBlock = kThreads / MMF_WAVE;  // 512, or 256 for small launches
  constexpr int NL = num_layers(NRES);
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* headw = lds + blob_floats(NRES);  // (NOUT, 64)
  {
    const float4* src = reinterpret_cast<const float4*>(a.packed);
    float4* dst = reinterpret_cast<float4*>(lds);
    if (kThreads == 512) mmf::stage_to_lds<blob_floats(NRES) / 4, 512, 4>(src, dst, threadIdx.x);
    else mmf::stage_to_lds<blob_floats(NRES) / 4, 256, 4>(src, dst, threadIdx.x);
    for (int i = threadIdx.x; i < NOUT * kUnits; i += kThreads) headw[i] = a.head_w[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
  const int wave_global = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int waves_total = gridDim.x * kWavesPerBlock;
  const int ntiles = (a.R + 31) / 32;
  const size_t ls = static_cast<size_t>(a.R) * kUnits;
  const size_t ms = static_cast<size_t>(a.R) * 2;
  const float* layers_t = lds + off_layers();
  // keep: store dz of `layer`; returns the largest magnitude of this lane's row (COMPACT), which `layer_t` reuses
  auto keep = [&](size_t layer, const Act<1>& v, int row, bool valid) -> float {
    if constexpr (COMPACT) {
      const float m = row_absmax(v);
      dz_store_h(reinterpret_cast<_Float16*>(a.dz) + layer * ls, a.dz_scale + layer * static_cast<size_t>(a.R), v, row, valid, h,
                 tile_absmax(m));
      return m;
    } else {
      stash_store(a.dz + layer * ls, v, row, valid, h);
      return 0.f;
    }
  };
  // acc += W^T in  (acc holds zeros or the residual path)
  auto layer_t = [&](const float* W, const Act<1>& in, Act<1>& acc, float) { mfma_layer<1>(W, in, acc, lane); };

  for (int tile = wave_global; tile < ntiles; tile += waves_total) {
    asm volatile("" ::: "memory");
    const int base = tile * 32;
    const bool valid = base + j < a.R;
    const int row = valid ? base + j : a.R - 1;
    const int mrow = QUAD ? (row & ~3) : row;  // ReLU masks: the primal row of the group

    // the ReLU masks of ALL layers of this tile, requested up front: read where they are used they are a chain of
    // NL + 1 dependent global loads per tile (~1 us each with two or three waves per SIMD to hide them: the kernel's bound)
    unsigned mw[NL + 1];
#pragma unroll
    for (int l = 0; l <= NL; ++l) mw[l] = a.mask[l * ms + static_cast<size_t>(mrow) * 2 + h];
    __builtin_amdgcn_sched_barrier(0);  // keep the requests here (the scheduler sinks loads to their uses)
    // gradient w.r.t. the head input: G[f] = sum_o Whead[o][f] d_out[o]
    float go[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) go[o] = valid ? a.d_out[static_cast<size_t>(row) * NOUT + o] : 0.f;
    Act<1> G, T;
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float s = 0.f;
#pragma unroll
        for (int o = 0; o < NOUT; ++o) s += headw[o * kUnits + 32 * t + rowmap(r, h)] * go[o];
        G.v[t][0][r] = s;
      }

    // residual blocks in reverse: trunk blocks NRES-1 .. 0, then the encoder block
#pragma unroll
    for (int b = NRES; b >= 0; --b) {
      const int l1 = b == 0 ? 0 : 3 + 2 * (b - 1);  // first layer of the block; its input is stash[l1]
      if (b == 0) {
        // join layer (2) sits between the encoder block and the trunk
        if (KIND == kMeasure) mask_by_word(mw[3], G);
        const float mj = keep(2, G, row, valid);
        zero_act(T);
        layer_t(layers_t + 2 * kLayerFloats, G, T, mj);
        G = T;
      }
      mask_by_word(mw[l1 + 2], G);                               // dz2 = da' * [a' > 0]
      const float m2 = keep(l1 + 1, G, row, valid);
      zero_act(T);
      layer_t(layers_t + (l1 + 1) * kLayerFloats, G, T, m2);     // dh = W2^T dz2
      mask_by_word(mw[l1 + 1], T);                               // dz1 = dh * [h > 0]
      const float m1 = keep(l1, T, row, valid);
      layer_t(layers_t + l1 * kLayerFloats, T, G, m1);           // da = dz2 + W1^T dz1
    }
    // first layer (d -> 64): dz_in = da0 * [a0 > 0]
    mask_by_word(mw[0], G);
    keep(NL, G, row, valid);
    // d states[i] = sum_f W_in[f][i] dz_in[f] (the blob's first-layer section holds W_in itself):
    // each lane owns 32 of the 64 features of its particle
    for (int i = 0; i < a.D; ++i) {
      float part = 0.f;
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) part += lds[off_w0() + (32 * t + rowmap(r, h)) * kW0Cols + i] * G.v[t][0][r];
      part += __shfl_xor(part, 32);
      if (valid && h == 0) a.d_states[static_cast<size_t>(row) * a.D + i] = part;
    }
  }
}

// Weight and bias gradients of all 64x64 layers: dW_l = dz_l^T stash_l (a GEMM with K = all R
// particles) and db_l = column sums of dz_l.  Grid (splits, layers); a workgroup owns one slice
// of the particles, its four waves the four 32x32 tiles of the 64x64 product.  Both MFMA
// operands are read straight from the row-major (R, 64) stashes: lane i of a k-step takes
// element [particle 2s + h][32 tile + i] -- 128 contiguous bytes per half-wave.  Partial sums
// per slice go to `partial_w` / `partial_b`; the caller adds the slices up (no float atomics).
__global__ __launch_bounds__(256) void weight_grad_kernel(const float* __restrict__ dz, const float* __restrict__ stash,
                                                          float* __restrict__ partial_w, float* __restrict__ partial_b,
                                                          int R, int slice, int accumulate) {
  const int split = blockIdx.x, layer = blockIdx.y, S = gridDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5, mt = wave >> 1, nt = wave & 1;
  const size_t ls = static_cast<size_t>(R) * kUnits;
  const float* A = dz + layer * ls + 32 * mt + i;
  const float* B = stash + layer * ls + 32 * nt + i;
  const int p0 = split * slice, p1 = min(R, p0 + slice);
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float bsum = 0.f;
  constexpr int U = 8;  // k-steps (pairs of particles) in flight
  for (int p = p0; p < p1; p += 2 * U) {
    float av[U], bv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = p + 2 * u + h;
      const bool ok = q < p1;
      av[u] = ok ? A[static_cast<size_t>(q) * kUnits] : 0.f;
      bv[u] = ok ? B[static_cast<size_t>(q) * kUnits] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
      bsum += av[u];
    }
  }
  float* pw = partial_w + ((static_cast<size_t>(layer) * S + split) * kUnits + 32 * mt) * kUnits + 32 * nt + i;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float* q = pw + static_cast<size_t>(rowmap(r, h)) * kUnits;
    *q = accumulate ? *q + acc[r] : acc[r];  // this (layer, split) block belongs to this workgroup alone
  }
  if (nt == 0) {
    bsum += __shfl_xor(bsum, 32);
    if (h == 0) {
      float* q = partial_b + (static_cast<size_t>(layer) * S + split) * kUnits + 32 * mt + i;
      *q = accumulate ? *q + bsum : bsum;
    }
  }
}

// The narrow reductions of the backward (first-layer and head weight gradients, head bias gradient,
// per-trajectory join-bias gradient) in ONE pass over the rows: thread (column c, row lane rl) walks
// the rows rl, rl + 4, .. of its slice of one trajectory; the four row lanes meet in LDS.
__global__ __launch_bounds__(256) void small_grads_kernel(const float* __restrict__ dz_first, const float* __restrict__ dz_join,
                                                          const float* __restrict__ h_last, const float* __restrict__ states,
                                                          const float* __restrict__ d_out, float* __restrict__ p_first,
                                                          float* __restrict__ p_head, float* __restrict__ p_dout,
                                                          float* __restrict__ p_traj, int M, int d, int n_out) {
  __shared__ float red[4][10][kUnits];
  const int sl = blockIdx.x, n = blockIdx.y, S = gridDim.x;
  const int c = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int len = (M + S - 1) / S;
  const int m0 = sl * len, m1 = min(M, m0 + len);
  float first[4] = {0.f, 0.f, 0.f, 0.f}, head[4] = {0.f, 0.f, 0.f, 0.f}, dsum[4] = {0.f, 0.f, 0.f, 0.f}, tb = 0.f;
  constexpr int UN = 4;  // rows in flight per thread: the loop is a latency chain otherwise
  for (int m = m0 + rl; m < m1; m += 4 * UN) {
    float a[UN], j[UN], hv[UN], sv[UN][4], gv[UN][4];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int mm = m + 4 * u;
      const bool ok = mm < m1;
      const size_t r = static_cast<size_t>(n) * M + (ok ? mm : m);
      a[u] = ok ? dz_first[r * kUnits + c] : 0.f;
      j[u] = ok ? dz_join[r * kUnits + c] : 0.f;
      hv[u] = ok ? h_last[r * kUnits + c] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sv[u][i] = i < d ? states[r * d + i] : 0.f;
        gv[u][i] = (ok && i < n_out) ? d_out[r * n_out + i] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      tb += j[u];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        first[i] += a[u] * sv[u][i];
        head[i] += gv[u][i] * hv[u];
        dsum[i] += gv[u][i];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    red[rl][i][c] = first[i];
    red[rl][4 + i][c] = head[i];
  }
  red[rl][8][c] = tb;
  if (c < 4) red[rl][9][c] = dsum[c];
  __syncthreads();
  if (rl == 0) {
    const size_t slot = static_cast<size_t>(n) * S + sl;
    auto total = [&](int k) { return red[0][k][c] + red[1][k][c] + red[2][k][c] + red[3][k][c]; };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      p_first[(slot * kUnits + c) * 4 + i] = total(i);
      p_head[(slot * 4 + i) * kUnits + c] = total(4 + i);
    }
    p_traj[slot * kUnits + c] = total(8);
    if (c < 4) p_dout[slot * 4 + c] = total(9);
  }
}

// ---- COMPACT buffers: the two reductions over rows on f16 rows of 128 B.
// A 2-byte load per lane (the fp32 kernels' one-feature-per-lane mapping on f16 data) runs at a third of the fp32
// kernel's rate (measured 990 us against 358 for the 8 layers of 262,144 rows): the load path works per instruction,
// not per byte.  Here lane (i, h) loads ONE DWORD = features (2i, 2i + 1) of a row, so one load instruction brings two
// whole rows; eight such loads give the lane 8 consecutive rows of its feature pair = after four v_perm the A (dz)
// or B (stash) operand of v_mfma_f32_32x32x16_f16 for the even and for the odd feature, and a wave forms the FULL
// 64 x 64 product of 16 rows with four MFMAs on the (even | odd) x (even | odd) combinations.  f16 x f16 products are
// exact in the fp32 accumulator, so nothing is lost against converting to fp32 first (the first version did, on the
// 16x slower f32 MFMA: 200 us, MFMA-bound); a 32-row tile's product is accumulated apart and enters the running sum
// multiplied by the tile's dz scale.  The four waves of a workgroup take interleaved tiles and meet in LDS.
__device__ __forceinline__ float half_lo(uint32_t w) { return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(w & 0xffffu))); }
__device__ __forceinline__ float half_hi(uint32_t w) { return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(w >> 16))); }

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
// the low (HI = false) or high halves of 8 dwords as one MFMA operand: element e <-> dword e
template <bool HI>
__device__ __forceinline__ half8 gather_halves(const uint32_t (&w)[8]) {
  constexpr uint32_t sel = HI ? 0x07060302u : 0x05040100u;
  const u32x4 v = {__builtin_amdgcn_perm(w[1], w[0], sel), __builtin_amdgcn_perm(w[3], w[2], sel),
                   __builtin_amdgcn_perm(w[5], w[4], sel), __builtin_amdgcn_perm(w[7], w[6], sel)};
  return __builtin_bit_cast(half8, v);
}

__global__ __launch_bounds__(256) void weight_grad_h_kernel(const uint32_t* __restrict__ dz, const uint32_t* __restrict__ stash,
                                                            const float* __restrict__ dz_scale, float* __restrict__ partial_w,
                                                            float* __restrict__ partial_b, int R, int slice, int accumulate) {
  __shared__ float tile[2][kUnits * kUnits];   // 32 KB: where the four waves' partial products meet
  __shared__ float bcol[4][kUnits];
  const int split = blockIdx.x, layer = blockIdx.y, S = gridDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  constexpr int kRowWords = kUnits / 2;
  const size_t lw = static_cast<size_t>(R) * kRowWords;
  const uint32_t* A = dz + layer * lw + i;
  const uint32_t* B = stash + layer * lw + i;
  const float* Sc = dz_scale + static_cast<size_t>(layer) * R;
  const int p0 = split * slice, p1 = min(R, p0 + slice);  // slice: a multiple of 32 rows = whole tiles
  f32x16 acc[2][2], part[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
  float bsum[2] = {0.f, 0.f}, bpart[2];
  // two register sets of one 32-row tile each: the loads of the next tile are issued before this one's MFMAs.
  // Loads are UNCONDITIONAL on a clamped row and zeroed by select where they are used: a load under `if (row < end)`
  // becomes an exec-masked block and hipcc then waits for ALL outstanding loads (vmcnt(0)) before the first MFMA;
  // the scheduling fences keep each batch of loads ahead of the other set's MFMAs (left alone the scheduler sinks
  // every load next to its use).
  uint32_t aw[2][2][8], bw[2][2][8];  // [set][k-step of the tile][row]
  float sc[2];
  auto load = [&](int set, int t0) {  // the tile's rows t0 + 16 kk + 8 h + j
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const size_t qc = static_cast<size_t>(min(t0 + 16 * kk + 8 * h + j, R - 1));
        aw[set][kk][j] = A[qc * kRowWords];
        bw[set][kk][j] = B[qc * kRowWords];
      }
    sc[set] = Sc[min(t0, R - 1)];
  };
  auto multiply = [&](int set, int t0) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[a][b][r] = 0.f;
    bpart[0] = bpart[1] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
      for (int j = 0; j < 8; ++j)  // rows of the next slice / past R
        aw[set][kk][j] = (t0 + 16 * kk + 8 * h + j < p1) ? aw[set][kk][j] : 0u;
      const half8 a0 = gather_halves<false>(aw[set][kk]), a1 = gather_halves<true>(aw[set][kk]);
      const half8 b0 = gather_halves<false>(bw[set][kk]), b1 = gather_halves<true>(bw[set][kk]);
      part[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b0, part[0][0], 0, 0, 0);
      part[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, b1, part[0][1], 0, 0, 0);
      part[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b0, part[1][0], 0, 0, 0);
      part[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, b1, part[1][1], 0, 0, 0);
      // column sums of dz (the bias gradient): this lane's 8 rows of its two features
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        bpart[0] += half_lo(aw[set][kk][j]);
        bpart[1] += half_hi(aw[set][kk][j]);
      }
    }
    // the tile's product x its dz scale into the running sums
    const float s = sc[set];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = __builtin_fmaf(s, part[a][b][r], acc[a][b][r]);
    bsum[0] = __builtin_fmaf(s, bpart[0], bsum[0]);
    bsum[1] = __builtin_fmaf(s, bpart[1], bsum[1]);
  };
  int t0 = p0 + 32 * wave;  // this wave's tiles: t0, t0 + 128, ..
  load(0, t0);
  for (; t0 < p1; t0 += 256) {
    load(1, t0 + 128);  // clamped to row R - 1 past the end, zeroed at the use
    __builtin_amdgcn_sched_barrier(0);
    multiply(0, t0);
    __builtin_amdgcn_sched_barrier(0);
    load(0, t0 + 256);
    __builtin_amdgcn_sched_barrier(0);
    multiply(1, t0 + 128);  // a tile past the end is all zeros (no branch: one would cost the waitcnt its bookkeeping)
    __builtin_amdgcn_sched_barrier(0);
  }
  // acc[a][b][r] of lane (i, h) = dW[2 rowmap(r, h) + a][2 i + b].  Waves 2, 3 park their products in LDS, waves 0, 1
  // add them to their own and park the sums, then all threads add the two halves: (w0 + w2) + (w1 + w3)
  bsum[0] += __shfl_xor(bsum[0], 32);
  bsum[1] += __shfl_xor(bsum[1], 32);
  if (h == 0) *reinterpret_cast<float2*>(&bcol[wave][2 * i]) = make_float2(bsum[0], bsum[1]);
  if (wave >= 2) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        *reinterpret_cast<float2*>(&tile[wave - 2][(2 * rowmap(r, h) + a) * kUnits + 2 * i]) = make_float2(acc[a][0][r], acc[a][1][r]);
  }
  __syncthreads();
  if (wave < 2) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float2* q = reinterpret_cast<float2*>(&tile[wave][(2 * rowmap(r, h) + a) * kUnits + 2 * i]);
        const float2 o = *q;
        *q = make_float2(acc[a][0][r] + o.x, acc[a][1][r] + o.y);
      }
  }
  __syncthreads();
  float* pw = partial_w + (static_cast<size_t>(layer) * S + split) * kUnits * kUnits;
  for (int e = threadIdx.x; e < kUnits * kUnits / 4; e += 256) {
    const float4 t0v = reinterpret_cast<const float4*>(tile[0])[e], t1v = reinterpret_cast<const float4*>(tile[1])[e];
    float4 v = make_float4(t0v.x + t1v.x, t0v.y + t1v.y, t0v.z + t1v.z, t0v.w + t1v.w);
    float4* q = reinterpret_cast<float4*>(pw) + e;  // this (layer, split) block belongs to this workgroup alone
    if (accumulate) {
      const float4 o = *q;
      v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
    }
    *q = v;
  }
  if (threadIdx.x < kUnits) {
    const int c = threadIdx.x;
    const float v = (bcol[0][c] + bcol[2][c]) + (bcol[1][c] + bcol[3][c]);
    float* q = partial_b + (static_cast<size_t>(layer) * S + split) * kUnits + c;
    *q = accumulate ? *q + v : v;
  }
}

// small_grads_kernel on f16 rows: thread (i, h) of wave rl owns features (2i, 2i + 1) of the rows 2 rl + h, + 8, ..
__global__ __launch_bounds__(256) void small_grads_h_kernel(const uint32_t* __restrict__ dz_first, const uint32_t* __restrict__ dz_join,
                                                            const uint32_t* __restrict__ h_last, const float* __restrict__ states,
                                                            const float* __restrict__ d_out, float* __restrict__ p_first,
                                                            float* __restrict__ p_head, float* __restrict__ p_dout,
                                                            float* __restrict__ p_traj, int M, int d, int n_out,
                                                            const float* __restrict__ sc_first, const float* __restrict__ sc_join) {
  __shared__ float red[8][10][kUnits];
  const int sl = blockIdx.x, n = blockIdx.y, S = gridDim.x;
  const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6, i2 = lane & 31, h = lane >> 5;
  constexpr int kRowWords = kUnits / 2;
  const int len = (M + S - 1) / S;
  const int m0 = sl * len, m1 = min(M, m0 + len);
  float first[2][4] = {}, head[2][4] = {}, dsum[4] = {0.f, 0.f, 0.f, 0.f}, tb[2] = {0.f, 0.f};
  constexpr int UN = 4;  // rows in flight per thread
  for (int m = m0 + 2 * rl + h; m < m1; m += 8 * UN) {
    uint32_t a[UN], j[UN], hv[UN];
    float sa[UN], sj[UN], sv[UN][4], gv[UN][4];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int mm = m + 8 * u;
      const bool ok = mm < m1;
      const size_t r = static_cast<size_t>(n) * M + (ok ? mm : m);
      a[u] = ok ? dz_first[r * kRowWords + i2] : 0u;
      j[u] = ok ? dz_join[r * kRowWords + i2] : 0u;
      hv[u] = ok ? h_last[r * kRowWords + i2] : 0u;
      sa[u] = ok ? sc_first[r] : 0.f;
      sj[u] = ok ? sc_join[r] : 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        sv[u][i] = i < d ? states[r * d + i] : (i == d ? 1.f : 0.f);  // column d: the first layer's bias gradient
        gv[u][i] = (ok && i < n_out) ? d_out[r * n_out + i] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const float av[2] = {half_lo(a[u]) * sa[u], half_hi(a[u]) * sa[u]};
      const float hh[2] = {half_lo(hv[u]), half_hi(hv[u])};
      tb[0] += half_lo(j[u]) * sj[u];
      tb[1] += half_hi(j[u]) * sj[u];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          first[e][i] += av[e] * sv[u][i];
          head[e][i] += gv[u][i] * hh[e];
        }
        dsum[i] += gv[u][i];
      }
    }
  }
  const int rr = 2 * rl + h;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      red[rr][i][2 * i2 + e] = first[e][i];
      red[rr][4 + i][2 * i2 + e] = head[e][i];
    }
  red[rr][8][2 * i2] = tb[0];
  red[rr][8][2 * i2 + 1] = tb[1];
  if (i2 < 4) red[rr][9][i2] = dsum[0] * (i2 == 0) + dsum[1] * (i2 == 1) + dsum[2] * (i2 == 2) + dsum[3] * (i2 == 3);
  __syncthreads();
  if (rl == 0) {
    const int c = lane;
    const size_t slot = static_cast<size_t>(n) * S + sl;
    auto total = [&](int k) {
      return ((red[0][k][c] + red[1][k][c]) + (red[2][k][c] + red[3][k][c])) + ((red[4][k][c] + red[5][k][c]) + (red[6][k][c] + red[7][k][c]));
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      p_first[(slot * kUnits + c) * 4 + i] = total(i);
      p_head[(slot * 4 + i) * kUnits + c] = total(4 + i);
    }
    p_traj[slot * kUnits + c] = total(8);
    if (c < 4) p_dout[slot * 4 + c] = total(9);
  }
}

template <int D, int NRES, int KIND, bool QUAD = false, bool COMPACT = false>
int launch_train_fwd(const TrainArgs& a, hipStream_t s) {
  const size_t lds = static_cast<size_t>(blob_floats(NRES)) * sizeof(float);
  const int ntiles = (a.R + 31) / 32;
  // one workgroup per CU (LDS): up to 2048 tiles a 4-wave workgroup (one wave per SIMD, which already runs
  // the f32 MFMA at its issue rate) spreads the launch over twice as many CUs as an 8-wave one would
  const int wpb = ntiles <= 2048 ? 4 : 8;
  int grid = (ntiles + wpb - 1) / wpb;
  grid = grid > 256 ? 256 : (grid < 1 ? 1 : grid);
  auto k = particle_net_train_fwd_kernel<D, NRES, KIND, QUAD, COMPACT>;
  return mmf::launch(k, grid, wpb * 64, lds, s, a);
}

template <int NRES, int KIND, int NOUT, bool QUAD = false, bool COMPACT = false>
int launch_train_bwd(const TrainArgs& a, hipStream_t s) {
  const size_t lds = (static_cast<size_t>(blob_floats(NRES)) + NOUT * kUnits) * sizeof(float);
  const int ntiles = (a.R + 31) / 32;
  const int wpb = ntiles <= 2048 ? 4 : 8;  // see launch_train_fwd
  int grid = (ntiles + wpb - 1) / wpb;
  grid = grid > 256 ? 256 : (grid < 1 ? 1 : grid);
  auto k = particle_net_train_bwd_kernel<NRES, KIND, NOUT, QUAD, COMPACT>;
  return mmf::launch(k, grid, wpb * 64, lds, s, a);
}

}  // namespace

extern "C" int mmf_particle_net_train_forward(const float* packed, int n_res, int kind, const float* states,
                                              const float* traj_bias, float* stash, uint32_t* mask, float* out, int N,
                                              int M, int d, void* stream) {
  if (!packed || !states || !traj_bias || !stash || !mask || !out) return MMF_EINVAL;
  if (N < 0 || M < 1 || (kind != kDynamics && kind != kMeasure && kind != kJacobian)) return MMF_EINVAL;
  if (kind == kJacobian && M != 4) return MMF_EINVAL;  // groups of {primal, e_1, e_2, e_3}
  if (static_cast<long long>(N) * M > 0x7fffffffLL / 64) return MMF_ETOOLARGE;
  if (N == 0) return 0;
  TrainArgs a{};
  a.packed = packed; a.states = states; a.traj_bias = traj_bias; a.stash = stash; a.mask = mask; a.out = out;
  a.R = N * M; a.M = M;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (kind == kJacobian && n_res == 3 && d == 2) return launch_train_fwd<2, 3, kDynamics, true>(a, s);
  if (kind == kJacobian && n_res == 3 && d == 3) return launch_train_fwd<3, 3, kDynamics, true>(a, s);
  if (kind == kDynamics && n_res == 3 && d == 2) return launch_train_fwd<2, 3, kDynamics>(a, s);
  if (kind == kDynamics && n_res == 3 && d == 3) return launch_train_fwd<3, 3, kDynamics>(a, s);
  if (kind == kMeasure && n_res == 2 && d == 2) return launch_train_fwd<2, 2, kMeasure>(a, s);
  if (kind == kMeasure && n_res == 2 && d == 3) return launch_train_fwd<3, 2, kMeasure>(a, s);
  return MMF_EINVAL;
}

extern "C" int mmf_particle_net_train_backward(const float* packed_t, const float* head_w, int n_res, int kind,
                                               const uint32_t* mask, const float* d_out, float* dz,
                                               float* d_states, int R, int d, void* stream) {
  if (!packed_t || !head_w || !mask || !d_out || !dz || !d_states) return MMF_EINVAL;
  if (d < 1 || d > MMF_MAX_STATE_DIM) return MMF_EINVAL;
  if (R < 0 || (kind != kDynamics && kind != kMeasure && kind != kJacobian)) return MMF_EINVAL;
  if (R > 0x7fffffff / 64) return MMF_ETOOLARGE;
  if (R == 0) return 0;
  TrainArgs a{};
  a.packed = packed_t; a.head_w = head_w; a.mask = const_cast<uint32_t*>(mask); a.d_out = d_out; a.dz = dz; a.d_states = d_states;
  a.R = R; a.M = 1; a.D = d;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (kind == kJacobian && n_res == 3 && d == 2) return launch_train_bwd<3, kDynamics, 3, true>(a, s);
  if (kind == kJacobian && n_res == 3 && d == 3) return launch_train_bwd<3, kDynamics, 4, true>(a, s);
  if (kind == kMeasure && n_res == 2) return launch_train_bwd<2, kMeasure, 1>(a, s);
  if (kind == kDynamics && n_res == 3 && d == 2) return launch_train_bwd<3, kDynamics, 3>(a, s);
  if (kind == kDynamics && n_res == 3 && d == 3) return launch_train_bwd<3, kDynamics, 4>(a, s);
  return MMF_EINVAL;
}

extern "C" int mmf_particle_net_weight_grads_acc(const float* dz, const float* stash, float* partial_w,
                                                 float* partial_b, int n_layers, int R, int n_splits, int accumulate,
                                                 void* stream) {
  if (!dz || !stash || !partial_w || !partial_b) return MMF_EINVAL;
  if (n_layers < 1 || R < 0 || n_splits < 1 || n_splits > 65535) return MMF_EINVAL;
  if (R > 0x7fffffff / 64) return MMF_ETOOLARGE;
  int slice = (R + n_splits - 1) / n_splits;
  slice += slice & 1;  // pairs of particles per k-step
  if (slice < 2) slice = 2;
  weight_grad_kernel<<<dim3(n_splits, n_layers), 256, 0, static_cast<hipStream_t>(stream)>>>(dz, stash, partial_w,
                                                                                          partial_b, R, slice, accumulate);
  MMF_CHECK_LAUNCH();
  return 0;
}

extern "C" int mmf_particle_net_weight_grads(const float* dz, const float* stash, float* partial_w,
                                             float* partial_b, int n_layers, int R, int n_splits, void* stream) {
  return mmf_particle_net_weight_grads_acc(dz, stash, partial_w, partial_b, n_layers, R, n_splits, 0, stream);
}

extern "C" int mmf_particle_net_small_grads(const float* dz_first, const float* dz_join, const float* h_last,
                                            const float* states, const float* d_out, float* p_first, float* p_head,
                                            float* p_dout, float* p_traj, int N, int M, int d, int n_out,
                                            int n_slices, void* stream) {
  if (!dz_first || !dz_join || !h_last || !states || !d_out || !p_first || !p_head || !p_dout || !p_traj) return MMF_EINVAL;
  if (N < 0 || M < 1 || d < 1 || d > 4 || n_out < 1 || n_out > 4 || n_slices < 1 || n_slices > 65535 || N > 65535) return MMF_EINVAL;
  if (N == 0) return 0;
  small_grads_kernel<<<dim3(n_slices, N), 256, 0, static_cast<hipStream_t>(stream)>>>(
      dz_first, dz_join, h_last, states, d_out, p_first, p_head, p_dout, p_traj, M, d, n_out);
  MMF_CHECK_LAUNCH();
  return 0;
}

// ---- COMPACT forms of the four passes (internal: the exact-fp32 three-pass backward of mmf_pf_train_backward -- the f32
// engine mode's training path and the cross-check of the fused kernel; buffers `stash` / `dz` are f16 arrays of the
// fp32 versions' SHAPES, `dz_scale` (NL + 1, R) fp32; every product is an exact fp32 product on the f32 MFMA)
int mmf_internal_train_forward_h(const float* packed, int n_res, int kind, const float* states, const float* traj_bias,
                                 void* stash_h, uint32_t* mask, float* out, int N, int M, int d, void* stream) {
  if (!packed || !states || !traj_bias || !stash_h || !mask || !out || N < 0 || M < 1) return MMF_EINVAL;
  if (N == 0) return 0;
  TrainArgs a{};
  a.packed = packed; a.states = states; a.traj_bias = traj_bias; a.stash = static_cast<float*>(stash_h); a.mask = mask; a.out = out;
  a.R = N * M; a.M = M;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (kind == kDynamics && n_res == 3 && d == 2) return launch_train_fwd<2, 3, kDynamics, false, true>(a, s);
  if (kind == kDynamics && n_res == 3 && d == 3) return launch_train_fwd<3, 3, kDynamics, false, true>(a, s);
  if (kind == kMeasure && n_res == 2 && d == 2) return launch_train_fwd<2, 2, kMeasure, false, true>(a, s);
  if (kind == kMeasure && n_res == 2 && d == 3) return launch_train_fwd<3, 2, kMeasure, false, true>(a, s);
  return MMF_EINVAL;
}

int mmf_internal_train_backward_h(const float* packed_t, const float* head_w, int n_res, int kind, const uint32_t* mask,
                                  const float* d_out, void* dz_h, float* dz_scale, float* d_states, int R, int d, void* stream) {
  if (!packed_t || !head_w || !mask || !d_out || !dz_h || !dz_scale || !d_states || R < 0) return MMF_EINVAL;
  if (R == 0) return 0;
  TrainArgs a{};
  a.packed = packed_t; a.head_w = head_w; a.mask = const_cast<uint32_t*>(mask); a.d_out = d_out; a.dz = static_cast<float*>(dz_h);
  a.dz_scale = dz_scale; a.d_states = d_states; a.R = R; a.M = 1; a.D = d;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (kind == kMeasure && n_res == 2) return launch_train_bwd<2, kMeasure, 1, false, true>(a, s);
  if (kind == kDynamics && n_res == 3 && d == 2) return launch_train_bwd<3, kDynamics, 3, false, true>(a, s);
  if (kind == kDynamics && n_res == 3 && d == 3) return launch_train_bwd<3, kDynamics, 4, false, true>(a, s);
  return MMF_EINVAL;
}

int mmf_internal_weight_grads_h(const void* dz_h, const float* dz_scale, const void* stash_h, float* partial_w, float* partial_b,
                                int n_layers, int R, int n_splits, int accumulate, void* stream) {
  if (!dz_h || !dz_scale || !stash_h || !partial_w || !partial_b || n_layers < 1 || R < 0 || n_splits < 1 || n_splits > 65535) return MMF_EINVAL;
  if (R == 0) return 0;  // (the kernel clamps its loads to row R - 1)
  int slice = (R + n_splits - 1) / n_splits;
  slice = (slice + 31) / 32 * 32;  // whole 32-row tiles: a tile has ONE dz scale
  weight_grad_h_kernel<<<dim3(n_splits, n_layers), 256, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const uint32_t*>(dz_h), static_cast<const uint32_t*>(stash_h), dz_scale, partial_w, partial_b, R, slice, accumulate);
  MMF_CHECK_LAUNCH();
  return 0;
}

int mmf_internal_small_grads_h(const void* dz_first_h, const float* sc_first, const void* dz_join_h, const float* sc_join,
                               const void* h_last_h, const float* states, const float* d_out, float* p_first, float* p_head,
                               float* p_dout, float* p_traj, int N, int M, int d, int n_out, int n_slices, void* stream) {
  if (!dz_first_h || !dz_join_h || !h_last_h || !states || !d_out || !p_first || !p_head || !p_dout || !p_traj) return MMF_EINVAL;
  if (N <= 0) return N == 0 ? 0 : MMF_EINVAL;
  small_grads_h_kernel<<<dim3(n_slices, N), 256, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const uint32_t*>(dz_first_h), static_cast<const uint32_t*>(dz_join_h), static_cast<const uint32_t*>(h_last_h), states,
      d_out, p_first, p_head, p_dout, p_traj, M, d, n_out, sc_first, sc_join);
  MMF_CHECK_LAUNCH();
  return 0;
}
