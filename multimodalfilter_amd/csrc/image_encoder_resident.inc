// K4, round 6: the WHOLE convolution stack of an image encoder as ONE resident producer / consumer kernel
// (included inside image_encoder.hip's anonymous namespace, after image_encoder_fused.inc whose helpers it uses).
//
//   /root/reference/crossmodal/door_models/layers.py:43-63  (push_models/layers.py:77-104)
//
//   image -> [5x5 stem, ReLU] -> A -> [conv 32->32, ReLU] -> B -> [conv 32->32 + A, ReLU] -> C -> [conv 32->16, ReLU] -> D
//         -> [conv 16->8] -> E (HBM, fp32: the split-K linear layer's input)
//
// Rounds 2-5 cut this chain in two launches at B: stem_conv2a wrote the 32-channel plane to HBM (128 KB per
// image-encoder) and conv2b_conv3 read it back and re-computed A from the image for the skip connection -- 2.1 GB of
// the 2.84 GB a 4096 x 2 launch sequence moved, against 36 MB of images in and 268 MB of E out.  Here A, B, C and D
// live in LDS row rings (two f16 planes each, hi / lo rows interleaved, the XOR-swizzled 16-byte chunks of
// image_encoder_fused.inc) and only the image and E cross HBM.
//
// One 512-thread workgroup per CU, persistent over images.  Rows of consecutive images form ONE stream (global row
// g = 32 * image + y lives in ring slot g % size), so the pipeline never drains between images.  Roles, two rows per
// step, one barrier per step; the stages trail each other by the rows their 3x3 windows need:
//
//   step s     Z waves (6, 7)   A rows 2s+3, 2s+4   5x5 stem from the image planes (one row each)
//                               E rows 2s-9, 2s-8   conv 16->8 from the D ring (one row each) -> HBM
//              XA waves (0, 1)  B rows 2s,   2s+1   conv 32->32 of A, weights in 144 VGPRs
//              XB waves (2, 3)  C rows 2s-3, 2s-2   conv 32->32 of B + skip (the A row, READ BACK from its ring
//                                                   instead of re-computed: the A ring is two slots deeper for it)
//              Y waves (4, 5)   D rows 2s-6, 2s-5   conv 32->16 of C (DPP-shifted accumulators, one fragment per ky)
//
// Waves w and w + 4 share a SIMD: each SIMD hosts one 54-MFMA X row (1,728 matrix-pipe cycles) beside a Y row (864)
// or a stem row + an E row (480) -- 2,592 / 2,208 cycles of matrix work per SIMD and step; the X waves' serial
// tails (ReLU, operand split, plane writes) fall under the partner's MFMAs and vice versa.
// Measured and NOT kept (profiles/r06/k4_software_pipelined_x_ab.txt): the X waves software-pipelined over rows (a row's
// epilogue in the MFMA gaps of the next row, rings one step deeper) -- correct, 3 vector instructions per gap as pinned, and
// no faster: the kernel executes its MFMAs at the rate a bare MFMA + LDS loop sustains on these boxes (~1.15 PFLOP/s of
// executed f16 products), with or without the tails in the gaps, with or without the step barrier (ablations ibid.).
// Ring hazards (a slot is written one barrier before it is read, and never while a reader of the same step holds it):
//   A: read 2s-3 .. 2s+2 (XA: 2s-1 .. 2s+2, XB's skip: 2s-3, 2s-2), written 2s+3, 2s+4  -> 8 slots
//   B: read 2s-4 .. 2s-1, written 2s, 2s+1                                               -> 6 slots
//   C: read 2s-7 .. 2s-4, written 2s-3, 2s-2                                             -> 6 slots
//   D: read 2s-10 .. 2s-7, written 2s-6, 2s-5                                            -> 6 slots
// Rows outside an image point at one shared all-zero row pair, so every loop is branch-free.
// LDS: image planes 10.5 KB + A 34.8 + B 26.1 + C 26.1 + D 13.1 + zero rows 4.4 + biases = 115,200 B.

// Whole-kernel ablations for scripts/debug/k4_ablate.sh (compiled out of the library): MMF_K4_ABLATE=<bits> at run time --
// 1: no conv 32->32 of A, 2: no conv 32->32 of B, 4: no conv 32->16, 8: no conv 16->8, 16: no stem, 32: no step barrier,
// 1024: Y / Z waves at priority 0 (results of 1 .. 32 are garbage: timing only; profiles/r06/k4_ablate_*.txt)
#ifdef MMF_K4_ABLATE
#define K4R_ON(bit) (!(a.ablate & (bit)))
#else
#define K4R_ON(bit) true
#endif

constexpr int kResA = 8, kResR = 6;          // ring slots
constexpr int kResRP = 2 * kRow32;           // a ring row: hi plane row, then lo plane row
constexpr int kResDRow16 = kWPh * 16;        // D: bytes per (plane, 8-channel chunk, row)
constexpr int kResDSlot = 4 * kResDRow16;    // D ring slot: [hi|lo][chunk 2][34 cols][8 halves]
constexpr size_t kLdsResident = 4 * kImgPlane + 128 + (kResA + 2 * kResR) * kResRP + kResR * kResDSlot + kResRP + 256;
static_assert(kLdsResident <= mmf::kLdsPerCu, "the resident K4 kernel must fit LDS");
static_assert(kResDSlot <= kResRP, "the shared zero row pair must cover a D slot");

// hi / lo halves of a pair of values as they are KEPT for the skip connection: f16x3 mode = the operand split itself;
// bf16 mode = bf16(x) (the product operand) and bf16(x - hi), so that hi + lo returns 16 bits of the activation
template <bool BF>
__device__ __forceinline__ void split2_keep(float x0, float x1, float neg_one, unsigned& hi, unsigned& lo) {
  if constexpr (BF) {
    const bf16x2 hh = __builtin_convertvector(f32x2{x0, x1}, bf16x2);
    const float r0 = x0 - static_cast<float>(hh[0]), r1 = x1 - static_cast<float>(hh[1]);
    hi = __builtin_bit_cast(unsigned, hh);
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, bf16x2));
  } else {
    split_pair(x0, x1, neg_one, hi, lo);
  }
}

// an A row (accumulator layout) -> ring row at byte offset `rowoff` of the hi plane (lo = + kRow32), swizzle of the
// 32x32x16 B fragments; BOTH halves are written in every mode (the skip connection reads them back)
template <bool BF>
__device__ __forceinline__ void write_row_a(unsigned char* phi, int rowoff, const Ctx& c, const f32x16& v, short2v& amax) {
  const int col = c.j + 1;
  const int sw = swz32(col);
  const int base = rowoff + col * kPix32 + 8 * c.h;
#pragma unroll
  for (int cg = 0; cg < 4; ++cg) {
    unsigned h0, l0, h1, l1;
    split2_keep<BF>(v[4 * cg], v[4 * cg + 1], c.neg_one, h0, l0);
    split2_keep<BF>(v[4 * cg + 2], v[4 * cg + 3], c.neg_one, h1, l1);
    const int off = base + 16 * (cg ^ sw);
    *reinterpret_cast<uint2*>(phi + off) = make_uint2(h0, h1);
    *reinterpret_cast<uint2*>(phi + off + kRow32) = make_uint2(l0, l1);
    if constexpr (!BF) {
      track(amax, h0);
      track(amax, h1);
    }
  }
}

// the skip row back from the A ring: lane (pixel j, half h) owns channels 8 cg + 4 h + e of its accumulator layout
template <bool BF>
__device__ __forceinline__ void read_skip_row(f32x16& sk, const unsigned char* phi, int rowoff, const Ctx& c) {
  const int col = c.j + 1;
  const int sw = swz32(col);
  const unsigned char* p = phi + rowoff + col * kPix32 + 8 * c.h;
  uint2 hv[4], lv[4];
#pragma unroll
  for (int cg = 0; cg < 4; ++cg) {
    hv[cg] = *reinterpret_cast<const uint2*>(p + 16 * (cg ^ sw));
    lv[cg] = *reinterpret_cast<const uint2*>(p + 16 * (cg ^ sw) + kRow32);
  }
#pragma unroll
  for (int cg = 0; cg < 4; ++cg) {
    const unsigned hw[2] = {hv[cg].x, hv[cg].y}, lw[2] = {lv[cg].x, lv[cg].y};
#pragma unroll
    for (int p2 = 0; p2 < 2; ++p2) {
      if constexpr (BF) {
        sk[4 * cg + 2 * p2] = __uint_as_float(hw[p2] << 16) + __uint_as_float(lw[p2] << 16);
        sk[4 * cg + 2 * p2 + 1] = __uint_as_float(hw[p2] & 0xffff0000u) + __uint_as_float(lw[p2] & 0xffff0000u);
      } else {
        const half2v hh = __builtin_bit_cast(half2v, hw[p2]), ll = __builtin_bit_cast(half2v, lw[p2]);
        sk[4 * cg + 2 * p2] = static_cast<float>(hh[0]) + static_cast<float>(ll[0]);
        sk[4 * cg + 2 * p2 + 1] = static_cast<float>(hh[1]) + static_cast<float>(ll[1]);
      }
    }
  }
}

// training forward: a 32-channel row in accumulator layout -> fp32 (C, 32, 32) planes of its image (lane (pixel j, half h),
// register r = channel (r & 3) + 8 (r >> 2) + 4 h: every store instruction writes two 128-byte runs)
__device__ __forceinline__ void keep_row32(float* plane0, int y, const Ctx& c, const f32x16& v) {
  float* p = plane0 + y * kImg + c.j;
#pragma unroll
  for (int r = 0; r < 16; ++r) p[((r & 3) + 8 * (r >> 2) + 4 * c.h) * kImg * kImg] = v[r];
}

// conv 32 -> 32 of ONE output row with the 36 weight fragments in registers: the only LDS reads of the 54-MFMA row
// are its activation fragments, requested two MFMA groups ahead (three rotating buffers).  rowoff[ky]: byte offsets
// of the input rows' hi plane rows (lo = + kRow32).
template <bool BF>
__device__ __forceinline__ void conv32_row_regw(f32x16& acc, const half8 (&W)[18][2], const unsigned char* phi,
                                                const int (&rowoff)[3], const Ctx& c) {
  half8 Bf[3][2];
  auto loadB = [&](int it, int buf) {
    const int tap = it >> 1, kc = it & 1, ky = tap / 3, kx = tap % 3;
    const int col = c.j + kx;
    const int off = rowoff[ky] + col * kPix32 + 16 * ((2 * kc + c.h) ^ swz32(col));
    Bf[buf][0] = *reinterpret_cast<const half8*>(phi + off);
    if constexpr (!BF) Bf[buf][1] = *reinterpret_cast<const half8*>(phi + off + kRow32);
  };
  constexpr int kReads = BF ? 1 : 2, kMfmas = BF ? 1 : 3;
  loadB(0, 0);
  loadB(1, 1);
  __builtin_amdgcn_sched_group_barrier(0x100, 2 * kReads, 0);
#pragma unroll
  for (int it = 0; it < 18; ++it) {
    if (it + 2 < 18) loadB(it + 2, (it + 2) % 3);
    mma32<BF>(acc, W[it][0], W[it][1], Bf[it % 3][0], Bf[it % 3][1]);
    if (it + 2 < 18) __builtin_amdgcn_sched_group_barrier(0x100, kReads, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, kMfmas, 0);
  }
}

template <bool BF>
__device__ __forceinline__ void load_conv32_weights(half8 (&W)[18][2], const float* blob, int off_floats, int lane) {
  const unsigned char* w = reinterpret_cast<const unsigned char*>(blob + off_floats) + lane * 16;
#pragma unroll
  for (int it = 0; it < 18; ++it) {
    W[it][0] = *reinterpret_cast<const half8*>(w + (2 * it) * 1024);
    if constexpr (!BF) W[it][1] = *reinterpret_cast<const half8*>(w + (2 * it + 1) * 1024);
  }
}

template <bool BF>
__global__ __launch_bounds__(kFusedThreads) void image_encoder_resident_kernel(FusedArgs a) {
  constexpr Layout L = layout();
  extern __shared__ __attribute__((aligned(16))) unsigned char ldsb[];
  K4F_WG_STAMP(0, 0);
  unsigned char* img_p = ldsb;                         // [parity][hi|lo][kImgPlane]
  unsigned char* a_p = ldsb + 4 * kImgPlane + 128;     // 10496: 16-byte aligned; hi rows (lo = + kRow32)
  unsigned char* b_p = a_p + kResA * kResRP;
  unsigned char* c_p = b_p + kResR * kResRP;
  unsigned char* d_p = c_p + kResR * kResRP;
  unsigned char* z_p = d_p + kResR * kResDSlot;        // the shared all-zero row pair
  float* bias_p = reinterpret_cast<float*>(z_p + kResRP);  // [conv2a | conv2b][lane half][16]: accumulator layout
  const int zoffA = static_cast<int>(z_p - a_p), zoffB = static_cast<int>(z_p - b_p), zoffC = static_cast<int>(z_p - c_p),
            zoffD = static_cast<int>(z_p - d_p);

  const int net = blockIdx.y;
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  Ctx c;
  c.lane = tid & 63; c.j = c.lane & 31; c.h = c.lane >> 5;
  c.neg_one = -1.0f;
  asm volatile("" : "+s"(c.neg_one));
  const float* blob = a.packed[net];
  {  // image planes, rings (incl. their column padding), zero rows: everything in front of the biases
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int i = tid; i < static_cast<int>(reinterpret_cast<unsigned char*>(bias_p) - ldsb) / 16; i += kFusedThreads)
      reinterpret_cast<u32x4*>(ldsb)[i] = z;
  }
  if (tid < 64)  // the biases enter accumulators that hold kWScale x the sum (f16x3 fragments are scaled)
    bias_p[tid] = (BF ? 1.0f : kWScale) * blob[(tid < 32 ? L.b2a : L.b2b) + (tid & 3) + 8 * ((tid & 15) >> 2) + 4 * ((tid >> 4) & 1)];
  const int gx = gridDim.x;
  const int n_mine = a.N > static_cast<int>(blockIdx.x) ? (a.N - static_cast<int>(blockIdx.x) + gx - 1) / gx : 0;
  const int gend = 32 * n_mine;               // global rows of this workgroup
  const int last_step = 16 * n_mine + 4;      // E row gend - 1 = 2 s - 9 leaves at s = 16 n + 4
  auto image_of = [&](int i) { return static_cast<size_t>(blockIdx.x) + static_cast<size_t>(i) * gx; };
  auto planes = [&](int i, int part) { return img_p + ((i & 1) * 2 + part) * kImgPlane; };
  short2v amax = {0, 0};
  __syncthreads();  // zeroed LDS before anything lands in it

  if (wave >= 6) {
    // ============================ Z waves: stem rows, E rows, the image planes ============================
    const int u = wave - 6, tz = 64 * u + c.lane;
    StemRegs st;
    load_stem<BF>(st, blob, c.lane, c.h);
    // conv 16->8 on v_mfma_f32_32x32x16_f16 with the three kx taps folded into M (round 6): M row 8 kx + co, N = the 32
    // pixels of the row, K = the 16 input channels of one ky -- 3 x 3 products = 9 MFMAs of 32 cycles per row (288) against
    // 30 of 16 cycles (480) for the two-taps-per-MFMA form on half-empty 16x16 tiles, and 6 LDS reads instead of 20
    half8 W4[3][2];
    f32x16 bias4;
    {
      const unsigned char* w = reinterpret_cast<const unsigned char*>(blob + L.g4x) + c.lane * 16;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        W4[ky][0] = *reinterpret_cast<const half8*>(w + (2 * ky) * 1024);
        W4[ky][1] = *reinterpret_cast<const half8*>(w + (2 * ky + 1) * 1024);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) bias4[r] = (r >> 2) == 1 ? kWScale * blob[L.b4 + (r & 3) + 4 * c.h] : 0.f;  // rides in the kx = 1 block
    }
    f32x4 pimg[2];
    auto load_image = [&](int i) {
#pragma unroll
      for (int e = 0; e < 2; ++e) pimg[e] = *reinterpret_cast<const f32x4*>(a.images + image_of(i) * 1024 + 4 * (tz + 128 * e));
    };
    auto store_image = [&](int i) {
#pragma unroll
      for (int e = 0; e < 2; ++e) commit_image<BF>(planes(i, 0), planes(i, 1), pimg[e], tz + 128 * e, c.neg_one);
    };
    auto produce = [&](int g) {  // A row g = relu(stem) -> ring slot g % 8
      const unsigned char* ih[1] = {planes(g >> 5, 0)};
      const unsigned char* il[1] = {planes(g >> 5, 1)};
      const int ys[1] = {g & 31};
      f32x16 acc[1];
      stem_rows<1, BF>(acc, ih, il, ys, c.j, st);
      write_row_a<BF>(a_p, (g & (kResA - 1)) * kResRP, c, acc[0], amax);
      if (a.keep_a1) keep_row32(a.keep_a1 + (static_cast<size_t>(net) * a.N + image_of(g >> 5)) * 32 * kImg * kImg, g & 31, c, acc[0]);
    };
    // E row ye = conv 16->8 of D rows ye - 1 .. ye + 1 (no ReLU).  Accumulator register r of lane (pixel j, half h) is
    // M row (r & 3) + 8 (r >> 2) + 4 h = tap kx = r >> 2 of channel (r & 3) + 4 h: P_kx[x'] = sum_ky W[ky][kx] D[y + ky - 1][x']
    // on the UNSHIFTED pixels, and the row is out[x] = P_0[x - 1] + P_1[x] + P_2[x + 1] -- wave-wide DPP shifts of the
    // accumulators, zeros entering at the image border (pixel 0 / 31 of either lane half)
    struct PendingE {
      f32x4 v;
      float* o;
      bool valid;
    } pe;
    pe.valid = false;
    pe.o = nullptr;
    auto conv4_row = [&](int g) {
      const int ye = g & 31;
      f32x16 acc = bias4;
      half8 bh[3], bl[3];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int yin = ye + ky - 1;
        const int rowoff = (yin >= 0 && yin < kImg) ? ((g + ky - 1) % kResR) * kResDSlot : zoffD;
        const unsigned char* p = d_p + rowoff + c.h * kResDRow16 + (c.j + 1) * 16;   // channel chunk h of pixel j
        bh[ky] = *reinterpret_cast<const half8*>(p);
        bl[ky] = *reinterpret_cast<const half8*>(p + 2 * kResDRow16);
      }
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) mma32<false>(acc, W4[ky][0], W4[ky][1], bh[ky], bl[ky]);
      auto shr = [](float v) {  // lane l <- lane l - 1 across the wave; lane 0 <- 0
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), mmf::kDppWaveShr1, 0xf, 0xf, false));
      };
      auto shl = [](float v) {  // lane l <- lane l + 1 across the wave; lane 63 <- 0
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, false));
      };
      pe.o = a.out_e + ((static_cast<size_t>(net) * a.N + image_of(g >> 5)) * 8 + 4 * c.h) * kImg * kImg + ye * kImg + c.j;
      pe.valid = true;
      // P_0 of pixel 31 and P_2 of pixel 0 belong to no output: zeroing them at the SOURCE makes the shifts bring zeros
      // across the lane-half boundary (lane 31 -> 32, lane 32 -> 31), and the DPP moves themselves stay unconditional
      // (a select around the shift became an exec-masked branch, and a DPP move does not read disabled lanes)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float left = shr(c.j == kImg - 1 ? 0.f : acc[r]);   // P_0[x - 1]
        const float right = shl(c.j == 0 ? 0.f : acc[8 + r]);     // P_2[x + 1]
        pe.v[r] = ((acc[4 + r] + left) + right) * kWInv;
      }
    };
    auto store_e = [&]() {  // channel 4 h + r of the row: 32 lanes = one 128-byte run per store
      if (pe.valid) {
#pragma unroll
        for (int r = 0; r < 4; ++r) pe.o[r * kImg * kImg] = pe.v[r];
      }
      pe.valid = false;
    };

    if (n_mine > 0) {
      load_image(0);
      store_image(0);
    }
    __syncthreads();  // image 0 is in LDS (both Z waves wrote their halves)
    if (n_mine > 0) {  // A rows 0 .. 2 feed step 0
      if (u == 0) { produce(0); produce(2); }
      else produce(1);
    }
    __syncthreads();
    // the younger half of the workgroup loses every issue arbitration to the X waves at equal priority, and its chains (stem
    // gathers, DPP combines, operand splits) are what the step barrier waits for: static priority 1 (1.20 -> 1.16 ms per
    // 4096 x 2, profiles/r06/k4_ablate_priorities.txt; raising the X waves instead changes nothing)
#ifdef MMF_K4_ABLATE
    if (!(a.ablate & 1024))
#endif
    __builtin_amdgcn_s_setprio(1);
#pragma unroll 1
    for (int s = 0; s <= last_step; ++s) {
      store_e();
      const int ge = 2 * s - 9 + u;
      if (ge >= 0 && ge < gend && K4R_ON(8)) conv4_row(ge);
      const int ga = 2 * s + 3 + u;
      if (ga < gend && K4R_ON(16)) produce(ga);
      // the next image's planes: its first stem row is produced at step 16 i + 14; the planes of its parity were last
      // read for row 32 i - 1 at step 16 i - 2
      const int i = s >> 4, k = s & 15;
      if (k == 4 && i + 1 < n_mine) load_image(i + 1);
      if (k == 8 && i + 1 < n_mine) store_image(i + 1);
      if (K4R_ON(32)) __syncthreads();
    }
    store_e();
  } else if (wave >= 4) {
    // ============================ Y waves: conv 32 -> 16 ============================
    const int u = wave - 4;
    const int j16 = c.lane & 15, q = c.lane >> 4;
    f32x4 bias3;
#pragma unroll
    for (int r = 0; r < 4; ++r) bias3[r] = (BF ? 1.0f : kWScale) * blob[L.b3 + 4 * q + r];
    half8 W3[9][2];
    {
      const unsigned char* w = reinterpret_cast<const unsigned char*>(blob + (BF ? L.q3 : L.g3)) + c.lane * 16;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        W3[tap][0] = *reinterpret_cast<const half8*>(w + (2 * tap) * 1024);
        if constexpr (!BF) W3[tap][1] = *reinterpret_cast<const half8*>(w + (2 * tap + 1) * 1024);
      }
    }
    auto conv3_row = [&](int g) {
      const int yd = g & 31;
      f32x4 acc[2] = {bias3, bias3};
      int rowoff[3];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int yin = yd + ky - 1;
        rowoff[ky] = (yin >= 0 && yin < kImg) ? ((g + ky - 1) % kResR) * kResRP : zoffC;
      }
      // Each C-row fragment is read ONCE per ky for all three kx: the three kx taps multiply the SAME unshifted pixels
      // into three accumulator sets, P_kx[x'] = sum_ky W[ky][kx] C[y + ky - 1][x'], and the row is out[x] = P_0[x - 1] +
      // P_1[x] + P_2[x + 1] -- the shifts are DPP row shifts of the accumulators (a lane row of 16 = the 16 pixels of a
      // tile for one channel quarter), the pixel that crosses the two tiles rotated in, zeros entering at the border
      f32x4 P[3][2];
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
        P[0][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
        P[1][pt] = acc[pt];
        P[2][pt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      half8 B3[2][2][2];  // [buffer][pixel tile][hi|lo]: the next ky's fragments are requested before this ky's MFMAs
      auto load3 = [&](int ky, int buf) {
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
          const int col = 16 * pt + j16 + 1;  // plane column of pixel 16 pt + j16 itself
          const int off = rowoff[ky] + col * kPix32 + 16 * (q ^ swz16(col));
          B3[buf][pt][0] = *reinterpret_cast<const half8*>(c_p + off);
          if constexpr (!BF) B3[buf][pt][1] = *reinterpret_cast<const half8*>(c_p + off + kRow32);
        }
      };
      load3(0, 0);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        if (ky + 1 < 3) load3(ky + 1, (ky + 1) & 1);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int pt = 0; pt < 2; ++pt)
            mma16<BF>(P[kx][pt], W3[3 * ky + kx][0], W3[3 * ky + kx][1], B3[ky & 1][pt][0], B3[ky & 1][pt][1]);
        if (ky + 1 < 3) __builtin_amdgcn_sched_group_barrier(0x100, BF ? 2 : 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, BF ? 6 : 18, 0);
      }
      {
        auto shr1 = [](float fill, float v) {  // lane j <- lane j - 1 of its row; lane 0 <- fill
          return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x111, 0xf, 0xf, false));
        };
        auto shl1 = [](float fill, float v) {  // lane j <- lane j + 1 of its row; lane 15 <- fill
          return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(fill), __float_as_int(v), 0x101, 0xf, 0xf, false));
        };
        auto ror = [](float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x121, 0xf, 0xf, false)); };   // lane 0 <- lane 15
        auto rol = [](float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x12F, 0xf, 0xf, false)); };   // lane 15 <- lane 0
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // x - 1: tile 0's first pixel takes the zero padding, tile 1's first pixel takes tile 0's pixel 15
          const float l0 = shr1(0.f, P[0][0][r]);
          const float l1 = shr1(ror(P[0][0][r]), P[0][1][r]);
          // x + 1: tile 0's last pixel takes tile 1's pixel 0, tile 1's last pixel the zero padding
          const float r0 = shl1(rol(P[2][1][r]), P[2][0][r]);
          const float r1 = shl1(0.f, P[2][1][r]);
          acc[0][r] = (P[1][0][r] + l0) + r0;
          acc[1][r] = (P[1][1][r] + l1) + r1;
        }
      }
      // lane (pixel j16, quarter q), register r -> channel 4 q + r, pixel 16 pt + j16 -> D ring slot g % 6:
      // [hi|lo][channel chunk q >> 1][col][8 halves], pixel at column + 1
      unsigned char* dq = d_p + (g % kResR) * kResDSlot + (q >> 1) * kResDRow16 + (j16 + 1) * 16 + 8 * (q & 1);
#pragma unroll
      for (int pt = 0; pt < 2; ++pt) {
        u32x2 hv, lv;
        if (a.keep_a3) {  // channel 4 q + r of pixel 16 pt + j16
          float* kp = a.keep_a3 + ((static_cast<size_t>(net) * a.N + image_of(g >> 5)) * 16 + 4 * q) * kImg * kImg + yd * kImg + 16 * pt + j16;
#pragma unroll
          for (int r = 0; r < 4; ++r) kp[r * kImg * kImg] = fmaxf(acc[pt][r], 0.f) * (BF ? 1.0f : kWInv);
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          unsigned hh, ll;
          constexpr float inv = BF ? 1.0f : kWInv;
          split_pair(fmaxf(acc[pt][2 * p], 0.f) * inv, fmaxf(acc[pt][2 * p + 1], 0.f) * inv, c.neg_one, hh, ll);
          track(amax, hh);
          hv[p] = hh;
          lv[p] = ll;
        }
        *reinterpret_cast<u32x2*>(dq + 256 * pt) = hv;
        *reinterpret_cast<u32x2*>(dq + 256 * pt + 2 * kResDRow16) = lv;
      }
    };
    __syncthreads();  // image 0
    __syncthreads();  // A rows 0 .. 2
    // the younger half of the workgroup loses every issue arbitration to the X waves at equal priority, and its chains (stem
    // gathers, DPP combines, operand splits) are what the step barrier waits for: static priority 1 (1.20 -> 1.16 ms per
    // 4096 x 2, profiles/r06/k4_ablate_priorities.txt; raising the X waves instead changes nothing)
#ifdef MMF_K4_ABLATE
    if (!(a.ablate & 1024))
#endif
    __builtin_amdgcn_s_setprio(1);
#pragma unroll 1
    for (int s = 0; s <= last_step; ++s) {
      const int g = 2 * s - 6 + u;
      if (g >= 0 && g < gend && K4R_ON(4)) conv3_row(g);
      if (K4R_ON(32)) __syncthreads();
    }
  } else {
    // ============================ X waves: the two conv 32 -> 32 ============================
    const bool second = wave >= 2;  // XA (waves 0, 1): A -> B;  XB (waves 2, 3): B (+ A) -> C
    const int u = wave & 1;
    half8 W2[18][2];
    load_conv32_weights<BF>(W2, blob, second ? (BF ? L.q2b : L.h2b) : (BF ? L.q2a : L.h2a), c.lane);
    const unsigned char* in_p = second ? b_p : a_p;
    const int zoff_in = second ? zoffB : zoffA;
    __syncthreads();  // image 0
    __syncthreads();  // A rows 0 .. 2
#pragma unroll 1
    for (int s = 0; s <= last_step; ++s) {
      const int g = second ? 2 * s - 3 + u : 2 * s + u;
      if (g >= 0 && g < gend) {
        const int y = g & 31;
        f32x16 acc;
#pragma unroll
        for (int cg = 0; cg < 4; ++cg) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(bias_p + (second ? 32 : 0) + 16 * c.h + 4 * cg);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[4 * cg + r] = v[r];
        }
        int rowoff[3];
        if (second) {
          rowoff[0] = y > 0 ? ((g - 1) % kResR) * kResRP : zoff_in;
          rowoff[1] = (g % kResR) * kResRP;
          rowoff[2] = y < kImg - 1 ? ((g + 1) % kResR) * kResRP : zoff_in;
        } else {
          rowoff[0] = y > 0 ? ((g - 1) & (kResA - 1)) * kResRP : zoff_in;
          rowoff[1] = (g & (kResA - 1)) * kResRP;
          rowoff[2] = y < kImg - 1 ? ((g + 1) & (kResA - 1)) * kResRP : zoff_in;
        }
        if (K4R_ON(second ? 2 : 1)) conv32_row_regw<BF>(acc, W2, in_p, rowoff, c);
        if (second) {
          f32x16 sk;
          read_skip_row<BF>(sk, a_p, (g & (kResA - 1)) * kResRP, c);
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r] * (BF ? 1.0f : kWInv) + sk[r], 0.f);
          write_row32<true, BF>(c_p, c_p + kRow32, (g % kResR) * 2, c, acc, amax);
          if (a.keep_a2) keep_row32(a.keep_a2 + (static_cast<size_t>(net) * a.N + image_of(g >> 5)) * 32 * kImg * kImg, y, c, acc);
        } else {
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[r] = fmaxf(acc[r], 0.f) * (BF ? 1.0f : kWInv);
          write_row32<false, BF>(b_p, b_p + kRow32, (g % kResR) * 2, c, acc, amax);
          if (a.keep_h) keep_row32(a.keep_h + (static_cast<size_t>(net) * a.N + image_of(g >> 5)) * 32 * kImg * kImg, y, c, acc);
        }
      }
      if (K4R_ON(32)) __syncthreads();
    }
  }
  K4F_WG_STAMP(0, 1);
  if (a.range_flag != nullptr && saturated(amax)) atomicOr(a.range_flag, MMF_FLAG_RANGE);
}

// image -> E in ONE launch (persistent 512-thread workgroups, one per CU, networks on blockIdx.y)
inline int launch_resident(const FusedArgs& a_in, int nets, bool bf16, hipStream_t s) {
  FusedArgs a = a_in;
  if (a.out_e == nullptr) return MMF_EINVAL;
#ifdef MMF_K4_ABLATE
  a.ablate = getenv("MMF_K4_ABLATE") ? atoi(getenv("MMF_K4_ABLATE")) : 0;
#endif
  auto k = bf16 ? image_encoder_resident_kernel<true> : image_encoder_resident_kernel<false>;
  int gx = device_cus() / nets;  // persistent workgroups per network
  if (gx > a.N) gx = a.N;
  if (gx < 1) gx = 1;
  return mmf::launch(k, dim3(gx, nets), kFusedThreads, kLdsResident, s, a);
}
