// K6, image encoder, f16x3 weight gradients (included inside image_encoder.hip's anonymous namespace, after the f16x3 helpers).
//
// dW[co][ci][ky][kx] = sum over images and pixels of g[n][co][y][x] act[n][ci][y + ky - 1][x + kx - 1]: a GEMM with
// M = co, N = ci per tap, K = every pixel of every image -- the forward convolution's MACs again.  conv_wgrad_kernel runs it on
// exact fp32 products (v_mfma_f32_32x32x2_f32: 144 MFMAs of 64 cycles per image row and wave); in the reference-sized
// training step (profiles/r05/train_refsize_kernel_stats.csv) the weight gradients of the four 3x3 layers were 14 % of the
// kernel time.  Here the same contraction on v_mfma_f32_32x32x16_f16 with the three-product split of both operands
// (54 MFMAs of 32 cycles per row): K = 16 consecutive pixels of a row, lane (channel i, half h) holds pixels 8 h .. 8 h + 7 of
// each 16-pixel group of ITS channel's row -- two aligned float4 per group for g, a 10-pixel window per group and input row for
// the activations (the three kx taps are register shifts of it).
// Range: gradients have no fixed scale, so the whole tensor is multiplied by the power of two that brings its LARGEST magnitude
// (`g_absmax`, a device scalar the caller reduces first) to [2^14, 2^15): exact, every element within 2^-14 of the largest
// keeps a normal hi half, and the accumulators are multiplied back at the end.  db (column sums of g) stays an exact fp32 sum.
template <int CO, int CI>
__global__ __launch_bounds__(512) void conv_wgrad_h_kernel(const float* __restrict__ g, const float* __restrict__ act,
                                                           float* __restrict__ partial, float* __restrict__ partial_b, int N,
                                                           const float* __restrict__ g_absmax, int* __restrict__ range_flag) {
  extern __shared__ float red[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  float neg_one = -1.0f;
  asm volatile("" : "+s"(neg_one));
  float c = 1.f, inv = 1.f;
  {
    const float m = *g_absmax;
    const int e = (__float_as_int(m) >> 23) & 0xff;
    if (e > 30 && e < 255) {  // m c in [2^14, 2^15): c = 2^(141 - e); a tensor whose largest entry is below 2^-97 is left alone
      c = __int_as_float((268 - e) << 23);
      inv = __int_as_float((e - 14) << 23);
    }
  }
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;
  short2v amax = {0, 0};
  auto frag = [&](const float (&v)[8], half8& hi, half8& lo, bool tracked) {
    u32x4 hv, lv;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      unsigned a, b;
      split_pair(v[2 * p], v[2 * p + 1], neg_one, a, b);
      hv[p] = a; lv[p] = b;
      if (tracked) {  // activations are non-negative (post-ReLU) except the image: |x| through the sign-less compare
        track(amax, a & 0x7fff7fffu);
      }
    }
    hi = __builtin_bit_cast(half8, hv);
    lo = __builtin_bit_cast(half8, lv);
  };
  for (int u = blockIdx.x; u < 2 * N; u += gridDim.x) {
    const int n = u >> 1, y0 = 16 * (u & 1);
    const float* gn = g + (static_cast<size_t>(n) * CO + (i < CO ? i : 0)) * kImg * kImg + 8 * h;
    const float* an = act + (static_cast<size_t>(n) * CI + (i < CI ? i : 0)) * kImg * kImg + 8 * h;
#pragma unroll 1
    for (int y = y0 + wave; y < y0 + 16; y += 8) {
      half8 ahi[2], alo[2];
#pragma unroll
      for (int gi = 0; gi < 2; ++gi) {
        float a[8];
        const float4 t0 = i < CO ? *reinterpret_cast<const float4*>(gn + y * kImg + 16 * gi) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float4 t1 = i < CO ? *reinterpret_cast<const float4*>(gn + y * kImg + 16 * gi + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        a[0] = t0.x; a[1] = t0.y; a[2] = t0.z; a[3] = t0.w; a[4] = t1.x; a[5] = t1.y; a[6] = t1.z; a[7] = t1.w;
#pragma unroll
        for (int s = 0; s < 8; ++s) { bsum += a[s]; a[s] *= c; }
        frag(a, ahi[gi], alo[gi], false);
      }
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int yy = y + ky - 1;
        if (yy < 0 || yy >= kImg) continue;  // wave-uniform
#pragma unroll
        for (int gi = 0; gi < 2; ++gi) {
          // pixels base - 1 .. base + 8 of the activation row, base = 16 gi + 8 h: zero outside the row
          const int base = 16 * gi + 8 * h;
          const float* row = an + yy * kImg + 16 * gi;   // = &act[..][yy][base]
          const bool ok = i < CI;
          float w[10];
          const float4 t0 = ok ? *reinterpret_cast<const float4*>(row) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float4 t1 = ok ? *reinterpret_cast<const float4*>(row + 4) : make_float4(0.f, 0.f, 0.f, 0.f);
          w[0] = (ok && base > 0) ? row[-1] : 0.f;
          w[1] = t0.x; w[2] = t0.y; w[3] = t0.z; w[4] = t0.w; w[5] = t1.x; w[6] = t1.y; w[7] = t1.z; w[8] = t1.w;
          w[9] = (ok && base + 8 < kImg) ? row[8] : 0.f;
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float b[8] = {w[kx], w[kx + 1], w[kx + 2], w[kx + 3], w[kx + 4], w[kx + 5], w[kx + 6], w[kx + 7]};
            half8 bhi, blo;
            frag(b, bhi, blo, true);
            mma32<false>(acc[3 * ky + kx], ahi[gi], alo[gi], bhi, blo);
          }
        }
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] *= inv;
  wgrad_tree<9>(acc, red, wave, lane);
  wgrad_bias(bsum, red, partial_b, wave, lane);
  if (wave == 0) {
    // lane (column ci = i, half h), register r -> row co = (r & 3) + 8 (r >> 2) + 4 h
    float* p = partial + static_cast<size_t>(blockIdx.x) * kWgradTile;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int r = 0; r < 16; ++r) p[(tap * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * 32 + i] = acc[tap][r];
  }
  if (range_flag != nullptr && saturated(amax)) atomicOr(range_flag, MMF_FLAG_RANGE);
}

// ---- K6, image encoder, f16x3 data gradients of the 3x3 layers with 32 output channels ------------------------------------
// dgrad of a convolution = the convolution of the output gradient with the transposed, flipped weights, times the ReLU mask of
// the layer's INPUT activation (+ the skip path's gradient for the first layer of the residual block).  conv_kernel<.., MASK>
// runs it on exact fp32 products; here the two 32 <- 32 layers and the 32 <- 16 layer run on v_mfma_f32_32x32x16_f16 with
// the three-product split (round 2's per-layer forward kernel, which the resident kernel replaced on the forward side): the
// gradient band is staged ONCE as two f16 planes in a channel-innermost, XOR-swizzled LDS image (a B fragment = one
// ds_read_b128), scaled by the power of two that brings the tensor's largest magnitude (`in_absmax`, device scalar) to
// [2^14, 2^15); weights (2^8-scaled hi / lo fragments of W^T flipped, packed by mmf_pack_image_convs_backward) sit in LDS;
// persistent workgroups prefetch the next band into registers under the MFMAs.  8-row bands, one wave per two rows.
struct DgradHArgs {
  const float* packed;     // backward blob (bwd_layout)
  const float* in;         // (N, CIN, 32, 32) output gradient of the forward layer
  const float* in_absmax;  // device scalar: max |in|
  const float* skip;       // (N, 32, 32, 32) added before the mask, or null
  const float* mask;       // (N, 32, 32, 32) the layer's input activation: the gradient passes where it is > 0
  float* out;              // (N, 32, 32, 32)
  unsigned* out_absmax;    // device word (zeroed by the caller) that receives max |out| -- the next layer's `in_absmax` -- or null
  int N, hoff;
};

template <int CIN>
__device__ __forceinline__ int swz_h(int col) { return CIN == 32 ? (col >> 2) & 3 : (col >> 3) & 1; }

template <int CIN, bool SKIP>
__global__ __launch_bounds__(256) void conv_dgrad_h_kernel(DgradHArgs a) {
  constexpr int BAND = 8, THREADS = BAND * 32, COUT = 32;
  constexpr int RB = BAND + 2;
  constexpr int KC = CIN / 16;
  constexpr int CG = CIN / 8;                      // 16-byte chunks per pixel
  constexpr int PIX = CIN * 2;                     // bytes per pixel per plane
  constexpr int PLANE = RB * kWPh * PIX;           // bytes per plane
  constexpr int NW = 9 * KC * 2 * 64 * 16;         // weight bytes
  constexpr int XG = kImg / 4;                     // groups of 4 pixels per row
  constexpr int ITEMS = RB * CG * XG;              // staging items: 8 channels x 4 pixels
  constexpr int IPT = (ITEMS + THREADS - 1) / THREADS;
  constexpr int BPI = kImg / BAND;                 // bands per image
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];
  unsigned char* tile_hi = ldsb;
  unsigned char* tile_lo = ldsb + PLANE;
  unsigned char* wl = ldsb + 2 * PLANE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  float neg_one = -1.0f;
  asm volatile("" : "+s"(neg_one));
  float c = 1.f, inv = kWInv;  // input scale and what the accumulators are multiplied by (weights carry 2^8)
  {
    const float m = *a.in_absmax;
    const int e = (__float_as_int(m) >> 23) & 0xff;
    if (e > 30 && e < 255) {
      c = __int_as_float((268 - e) << 23);
      inv = __int_as_float((e - 14 - 8) << 23);
    }
  }
  {
    const float4* src = reinterpret_cast<const float4*>(a.packed + a.hoff);
    float4* dst = reinterpret_cast<float4*>(wl);
    for (int i = tid; i < NW / 16; i += THREADS) dst[i] = src[i];
    const u32x4 z = {0u, 0u, 0u, 0u};  // the two padding columns of every row are zero for the whole kernel
    for (int i = tid; i < RB * 2 * CG; i += THREADS) {
      const int cg = i % CG, side = (i / CG) & 1, rr = i / (2 * CG);
      const int off = (rr * kWPh + (side ? kWPh - 1 : 0)) * PIX + 16 * cg;
      *reinterpret_cast<u32x4*>(tile_hi + off) = z;
      *reinterpret_cast<u32x4*>(tile_lo + off) = z;
    }
  }
  const int nbands = BPI * a.N;
  const int it_xg[2] = {tid % XG, (tid + THREADS) % XG};
  const int it_cg[2] = {(tid / XG) % CG, ((tid + THREADS) / XG) % CG};
  const int it_rr[2] = {tid / (XG * CG), (tid + THREADS) / (XG * CG)};
  static_assert(IPT <= 2, "staging indices are precomputed for two rounds");
  f32x4 pf[IPT][8];
  auto prefetch = [&](int band) {  // unconditional loads (clamped addresses): the masking happens at commit time
    const int img = band / BPI, y0 = (band % BPI) * BAND;
    const float* in = a.in + static_cast<size_t>(img) * CIN * kImg * kImg;
#pragma unroll
    for (int it = 0; it < IPT; ++it) {
      const int y = min(max(y0 - 1 + min(it_rr[it], RB - 1), 0), kImg - 1);
      const float* p = in + ((it_cg[it] * 8) * kImg + y) * kImg + 4 * it_xg[it];
#pragma unroll
      for (int i = 0; i < 8; ++i) pf[it][i] = *reinterpret_cast<const f32x4*>(p + i * kImg * kImg);
    }
  };
  auto commit = [&](int band) {  // registers -> scale -> split -> swizzled LDS planes
    const int y0 = (band % BPI) * BAND;
#pragma unroll
    for (int it = 0; it < IPT; ++it) {
      if (tid + it * THREADS < ITEMS) {
        const int y = y0 - 1 + it_rr[it];
        const bool inside = y >= 0 && y < kImg;  // rows above / below the image are zero padding
#pragma unroll
        for (int px = 0; px < 4; ++px) {
          u32x4 hv, lv;
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const float x0 = inside ? pf[it][2 * p][px] * c : 0.f, x1 = inside ? pf[it][2 * p + 1][px] * c : 0.f;
            unsigned hh, ll;
            split_pair(x0, x1, neg_one, hh, ll);
            hv[p] = hh; lv[p] = ll;
          }
          const int cc = 4 * it_xg[it] + px + 1;
          const int off = (it_rr[it] * kWPh + cc) * PIX + 16 * (it_cg[it] ^ swz_h<CIN>(cc));
          *reinterpret_cast<u32x4*>(tile_hi + off) = hv;
          *reinterpret_cast<u32x4*>(tile_lo + off) = lv;
        }
      }
    }
  };

  float omax = 0.f;  // running max |out| of this lane: one atomic per wave at the end of the launch
  int band = blockIdx.x;
  if (band < nbands) prefetch(band);
  for (; band < nbands; band += gridDim.x) {
    __syncthreads();  // everyone finished reading the previous band's planes (and the weights landed)
    commit(band);
    __syncthreads();
    if (band + gridDim.x < nbands) prefetch(band + gridDim.x);  // in flight during the MFMAs
    const int img = band / BPI, y0 = (band % BPI) * BAND;
    const int r0 = 2 * wave;
    const size_t obase = static_cast<size_t>(img) * COUT * kImg * kImg;
    f32x16 acc[2];
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[rr][r] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap % 3;
      const int col = j + kx;
      const int sw = swz_h<CIN>(col);
#pragma unroll
      for (int kc = 0; kc < KC; ++kc) {
        const unsigned char* wp = wl + ((tap * KC + kc) * 2) * 1024 + lane * 16;
        const half8 ahi = *reinterpret_cast<const half8*>(wp);
        const half8 alo = *reinterpret_cast<const half8*>(wp + 1024);
        const int chunk = (2 * kc + h) ^ sw;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          const int off = ((r0 + rr + ky) * kWPh + col) * PIX + 16 * chunk;
          const half8 bhi = *reinterpret_cast<const half8*>(tile_hi + off);
          const half8 blo = *reinterpret_cast<const half8*>(tile_lo + off);
          mma32<false>(acc[rr], ahi, alo, bhi, blo);
        }
      }
    }
    // epilogue: lane (x = j, h), reg r -> channel (r & 3) + 8 (r >> 2) + 4 h; 128-byte row segments
#pragma unroll
    for (int rr = 0; rr < 2; ++rr)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = (r & 3) + 8 * (r >> 2) + 4 * h;
        const size_t o = obase + (static_cast<size_t>(ch) * kImg + (y0 + r0 + rr)) * kImg + j;
        float v = acc[rr][r] * inv;
        if (SKIP) v += a.skip[o];
        v = a.mask[o] > 0.f ? v : 0.f;
        a.out[o] = v;
        omax = fmaxf(omax, fabsf(v));
      }
  }
  if (a.out_absmax != nullptr) {
    omax = mmf::wave_max(omax);
    if (lane == 0) atomicMax(a.out_absmax, __float_as_uint(omax));  // non-negative floats order like their bit patterns
  }
}

template <int CIN, bool SKIP>
int launch_dgrad_h(const DgradHArgs& a, hipStream_t s) {
  constexpr int BAND = 8;
  constexpr size_t lds = 2 * (BAND + 2) * kWPh * CIN * 2 + 9 * (CIN / 16) * 2 * 64 * 16;
  static_assert(lds <= mmf::kLdsHalfCu, "two workgroups per CU");
  int gx = (kImg / BAND) * a.N;
  if (gx > 2 * device_cus()) gx = 2 * device_cus();  // persistent workgroups, two per CU
  return mmf::launch(conv_dgrad_h_kernel<CIN, SKIP>, gx, BAND * 32, lds, s, a);
}

// largest magnitude of a tensor into a device word (zeroed by the caller): non-negative floats order like their bit patterns;
// one atomic per workgroup (one per wave serialised 4,096 atomics on one word: 54 us for 67 MB)
__global__ __launch_bounds__(256) void absmax_kernel(const float* __restrict__ x, size_t n, unsigned* __restrict__ out) {
  __shared__ float red[4];
  float m = 0.f;
  for (size_t i = (static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x) * 4; i + 3 < n; i += static_cast<size_t>(gridDim.x) * 1024) {
    const float4 v = *reinterpret_cast<const float4*>(x + i);
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
  }
  m = mmf::wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) atomicMax(out, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}
