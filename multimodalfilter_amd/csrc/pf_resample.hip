// K1: particle reweight + normalise + weighted-mean estimate + fixed-point CDF + systematic /
// multinomial resample + gather, one kernel, one workgroup per trajectory.
//
// Replaces the post-measurement half of torchfilter's ParticleFilter.forward (external
// dependency of the reference; call sites /root/reference/crossmodal/eval_helpers.py:139-142;
// SURVEY.md 3.2 / T1).  The resampling definition is the integer one of
// oracle/resample.py (weights quantised to 2^-24 of the row max, u64 inclusive CDF), so the
// ancestor indices do not depend on the scan tree and match the oracle bit for bit.
//
// HBM traffic per particle (algorithmic): loglik 4 + logw 4 + states 4d read, states 4d written
// (+4 logw written in mode 0) = 32 B (d=3) / 24 B (d=2); everything else stays in LDS:
//   slot[i] (8 B/particle): first the fp32 unnormalised log-weight x_i, then (modes 1/2)
//   overwritten in place by the u64 inclusive CDF.
#include <cmath>

#include "mmf_common.h"
#include "mmf_launch.h"
#include "../../include/mmf_detmath.h"

// Phase stamps for scripts/ubench/k1_phases.hip (compiled out of the library): thread 0 of every
// workgroup stores s_memtime at phase boundaries into a buffer of its own.
#ifdef MMF_K1_PHASE_CLOCKS
__device__ unsigned long long g_k1_stamps[1024][8];
#define K1_STAMP(i)                                                                          \
  do {                                                                                       \
    if (threadIdx.x == 0 && blockIdx.x < 1024) {                                             \
      unsigned long long t_;                                                                 \
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");             \
      g_k1_stamps[blockIdx.x][i] = t_;                                                       \
    }                                                                                        \
  } while (0)
#else
#define K1_STAMP(i)
#endif

#include "pf_resample_systematic.inc"

namespace {
#include "pf_resample_cluster.inc"
int g_cluster_enabled = getenv("MMF_K1_CLUSTER") && getenv("MMF_K1_CLUSTER")[0] == '1';  // off: see mmf_pf_set_resample_cluster

constexpr int kBlock = mmf::kK1Block;  // 16 waves; M = 4096 -> one float4 chunk per thread
constexpr int kMaxWaves = mmf::kK1MaxWaves;
constexpr int kFixBits = mmf::kK1FixBits;
using Scratch = mmf::K1Scratch;  // lives behind the slots in dynamic LDS

// STAGE: the particle states are kept in LDS next to the CDF (M * 4D more bytes), so the gather
// of the resampling step reads LDS instead of going back to L2 / HBM for rows this workgroup
// has just streamed through.
// SOFT (torchfilter's ``soft_resample_alpha`` < 1): ancestors are drawn from the mixture
// alpha * w_i + (1 - alpha) / M, in fixed point q'_i = ((A q_i << 8) + (2^24 - A) floor((Q << 8) / M)) >> 32
// with A = floor(alpha 2^24) (so q'_i <= 2^24 and every bound of the integer scheme still holds), and the
// survivors carry the importance weights w / mixture, normalised (oracle/resample.py).
// REC: the belief record (covariance, ESS, log-evidence of the weighted set; mmf::K1Belief in pf_resample_systematic.inc),
// its sums in this kernel's own partition -- per thread over all its chunks, a butterfly per wave, the waves in order.
// The non-recording instantiation is the kernel as it was.
// ADAPT: ESS-triggered resampling (include/mmf.h, K1): the decision follows the sums' reductions; a kept trajectory writes
// mode 0's outputs and leaves before the search and the gather.  Without REC only sum e^2 of the record is accumulated.
struct BeliefOut { float* cov; float* ess; float* log_evidence; };  // (N, d, d), (N), (N); each or null
struct AdaptIn { float ess_floor; int32_t* resampled; };            // fl32(threshold * M); (N) 1 / 0 or null

template <int D, bool STAGE, bool SOFT = false, bool REC = false, bool ADAPT = false>
__global__ __launch_bounds__(kBlock) void pf_reweight_resample_kernel(
    const float* __restrict__ loglik, const float* __restrict__ logw_in,
    const float* __restrict__ states_in, const float* __restrict__ u,
    float* __restrict__ estimate, float* states_out, float* logw_out,
    int32_t* __restrict__ indices_out, int M, int M_out, int mode, float alpha, float lw_uniform,
    float log_uniform, BeliefOut rec, AdaptIn ad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // (the host's byte count of these sections is mmf::k1_search_lds, pf_resample_systematic.inc: the two must agree)
  const bool need_cdf = mode != 0;
  const int slot_bytes = need_cdf ? 8 : 4;
  const size_t slots_sz = (static_cast<size_t>(M) * slot_bytes + 15) & ~static_cast<size_t>(15);
  float* xf = reinterpret_cast<float*>(smem);                            // mode 0: x_i at [i]
  unsigned long long* cdf = reinterpret_cast<unsigned long long*>(smem);  // modes 1/2
  Scratch& sc = *reinterpret_cast<Scratch*>(smem + slots_sz);
  float* xs_lds = reinterpret_cast<float*>(smem + slots_sz + ((sizeof(Scratch) + 15) & ~static_cast<size_t>(15)));  // STAGE
  mmf::K1BeliefScratch& bsc = *reinterpret_cast<mmf::K1BeliefScratch*>(  // REC: behind the staged states
      smem + slots_sz + ((sizeof(Scratch) + 15) & ~static_cast<size_t>(15)) +
      (STAGE ? (static_cast<size_t>(M) * D * sizeof(float) + 15) & ~static_cast<size_t>(15) : 0));

  const int n = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (MMF_WAVE - 1);
  const int wave = tid >> 6;
  const int nwaves = blockDim.x >> 6;
  const int chunk = blockDim.x * 4;

  const float* ll = loglik + static_cast<size_t>(n) * M;
  // logw_in == nullptr: uniform weights -log M (what every resampling step leaves behind): nothing to read
  const float* lw = logw_in ? logw_in + static_cast<size_t>(n) * M : nullptr;
  // lw_uniform = float(-log(double(M))), rounded once on the host: the value mmf_pf_init_particles and
  // every resampling step write, and the one the oracle holds (device logf may differ by an ulp)
  const float* xs = states_in + static_cast<size_t>(n) * M * D;
  const bool vec = (M & 3) == 0;  // rows 16-B aligned -> float4 path

  auto x_store = [&](int i, float v) {
    if (need_cdf) reinterpret_cast<float*>(cdf + i)[0] = v; else xf[i] = v;
  };
  auto x_load = [&](int i) -> float {
    return need_cdf ? reinterpret_cast<const float*>(cdf + i)[0] : xf[i];
  };

  K1_STAMP(0);
  // the first chunk's particle states are requested before anything waits on memory: their
  // latency overlaps pass 1 (log-weights, row maximum, two barriers)
  float st0[4 * D];
  {
    const int i0 = tid * 4;
    if (vec && i0 + 3 < M) {
      const float4* p = reinterpret_cast<const float4*>(xs + static_cast<size_t>(i0) * D);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const float4 t = p[k];
        st0[4 * k] = t.x; st0[4 * k + 1] = t.y; st0[4 * k + 2] = t.z; st0[4 * k + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4 * D; ++k)
        st0[k] = (i0 * D + k < M * D) ? xs[static_cast<size_t>(i0) * D + k] : 0.f;
    }
  }

  // ---- pass 1: x_i = logw_i + loglik_i -> LDS, row max
  float mx = -INFINITY;
  int mi = 0x7fffffff;  // REC: the first of this thread's particles that holds its maximum
  for (int base = 0; base < M; base += chunk) {
    const int i0 = base + tid * 4;
    float v[4];
    if (vec && i0 + 3 < M) {
      const float4 a = *reinterpret_cast<const float4*>(ll + i0);
      const float4 b = lw ? *reinterpret_cast<const float4*>(lw + i0) : make_float4(lw_uniform, lw_uniform, lw_uniform, lw_uniform);
      v[0] = b.x + a.x; v[1] = b.y + a.y; v[2] = b.z + a.z; v[3] = b.w + a.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (i0 + j < M) ? (lw ? lw[i0 + j] : lw_uniform) + ll[i0 + j] : -INFINITY;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i0 + j < M) {
        x_store(i0 + j, v[j]);
        if constexpr (REC) { if (v[j] > mx || mi == 0x7fffffff) mi = i0 + j; }
        mx = fmaxf(mx, v[j]);
      }
  }
  const float mx_thread = mx;
  mx = mmf::wave_max(mx);
  if (lane == 0) sc.red[wave][0] = mx;
  __syncthreads();
  mx = sc.red[0][0];
  for (int w = 1; w < nwaves; ++w) mx = fmaxf(mx, sc.red[w][0]);
  if constexpr (REC) {  // the pivot: the smallest index holding the row maximum (indices < 2^24 are exact floats)
    const float cand = mmf::wave_max((mi != 0x7fffffff && mx_thread == mx) ? -static_cast<float>(mi) : -INFINITY);
    if (lane == 0) bsc.piv_wave[wave] = cand;
  }
  __syncthreads();
  float piv[D];
  mmf::K1Belief<D> bel;
  if constexpr (REC) {
    float best = bsc.piv_wave[0];
    for (int w = 1; w < nwaves; ++w) best = fmaxf(best, bsc.piv_wave[w]);
    const int p = best > -INFINITY ? static_cast<int>(-best) : 0;
#pragma unroll
    for (int c = 0; c < D; ++c) piv[c] = xs[static_cast<size_t>(p) * D + c];
    bel.reset();
  }
  K1_STAMP(1);

  // ---- pass 2: e_i = detexp(x_i - max); float sums for the estimate; integer CDF
  float S = 0.f, acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.f;
  float w2 = 0.f;  // ADAPT without REC: bel.s[0] alone
  unsigned long long carry = 0, qsum = 0;
  for (int base = 0; base < M; base += chunk) {
    const int i0 = base + tid * 4;
    float e[4];
    unsigned long long q[4], tsum = 0;
    float st[4 * D];
    if (base == 0) {
#pragma unroll
      for (int k = 0; k < 4 * D; ++k) st[k] = st0[k];
    } else if (vec && i0 + 3 < M) {
      const float4* p = reinterpret_cast<const float4*>(xs + static_cast<size_t>(i0) * D);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        const float4 t = p[k];
        st[4 * k] = t.x; st[4 * k + 1] = t.y; st[4 * k + 2] = t.z; st[4 * k + 3] = t.w;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4 * D; ++k)
        st[k] = (i0 * D + k < M * D) ? xs[static_cast<size_t>(i0) * D + k] : 0.f;
    }
    if (STAGE && need_cdf) {
#pragma unroll
      for (int k = 0; k < 4 * D; ++k)
        if (i0 * D + k < M * D) xs_lds[i0 * D + k] = st[k];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = i0 + j < M;
      e[j] = ok ? mmf::detexp(x_load(i0 + j) - mx) : 0.f;
      q[j] = static_cast<unsigned long long>(floorf(e[j] * 16777216.0f));
      tsum += q[j];
      S += e[j];
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = __builtin_fmaf(e[j], st[j * D + c], acc[c]);  // explicit: oracle/strict restates this chain
      if constexpr (REC) {
        const float xv = ok ? x_load(i0 + j) : -INFINITY;
        bel.add(xv == -INFINITY ? 0.f : e[j], st + j * D, piv);
      } else if constexpr (ADAPT) {
        const float xv = ok ? x_load(i0 + j) : -INFINITY;
        const float ev = xv == -INFINITY ? 0.f : e[j];
        w2 = __builtin_fmaf(ev, ev, w2);
      }
    }
    qsum += tsum;
    if (need_cdf && !SOFT) {
      const unsigned long long incl = mmf::wave_inclusive_scan(tsum, lane);
      if (lane == MMF_WAVE - 1) sc.wave_tot[wave] = incl;
      // the float sums of the estimate ride on the last chunk's two barriers instead of two of their own
      const bool last_chunk = base + chunk >= M;
      if (last_chunk) {
        const float Sw = mmf::wave_sum(S);
        float aw[D];
#pragma unroll
        for (int c = 0; c < D; ++c) aw[c] = mmf::wave_sum(acc[c]);
        if (lane == 0) {
          sc.red[wave][0] = Sw;
#pragma unroll
          for (int c = 0; c < D; ++c) sc.red[wave][1 + c] = aw[c];
        }
      }
      __syncthreads();
      if (last_chunk && tid <= D) {
        float t = 0.f;
        for (int w = 0; w < nwaves; ++w) t += sc.red[w][tid];
        sc.bcast[tid] = t;
      }
      unsigned long long before = carry, total = 0;
      for (int w = 0; w < nwaves; ++w) {
        const unsigned long long t = sc.wave_tot[w];
        if (w < wave) before += t;
        total += t;
      }
      unsigned long long run = before + incl - tsum;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        run += q[j];
        if (i0 + j < M) cdf[i0 + j] = run;
      }
      carry += total;
      __syncthreads();
    }
  }
  if (SOFT && need_cdf) {
    // Q first (the mixture needs it), then a second sweep: e and q again from the staged x_i (each
    // thread re-reads only the slots it overwrites), mixture weights, inclusive scan -> CDF
    const unsigned long long incl = mmf::wave_inclusive_scan(qsum, lane);
    if (lane == MMF_WAVE - 1) sc.wave_tot[wave] = incl;
    __syncthreads();
    unsigned long long Qall = 0;
    for (int w = 0; w < nwaves; ++w) Qall += sc.wave_tot[w];
    __syncthreads();
    const unsigned long long A = static_cast<unsigned long long>(floorf(alpha * 16777216.0f));
    const unsigned long long uni = (16777216ull - A) * ((Qall << 8) / static_cast<unsigned long long>(M));
    for (int base = 0; base < M; base += chunk) {
      const int i0 = base + tid * 4;
      unsigned long long q[4], tsum = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        q[j] = 0;
        if (i0 + j < M) {
          const float e = mmf::detexp(x_load(i0 + j) - mx);
          q[j] = (((A * static_cast<unsigned long long>(floorf(e * 16777216.0f))) << 8) + uni) >> (kFixBits + 8);
        }
        tsum += q[j];
      }
      const unsigned long long incl2 = mmf::wave_inclusive_scan(tsum, lane);
      if (lane == MMF_WAVE - 1) sc.wave_tot[wave] = incl2;
      __syncthreads();
      unsigned long long before = carry, total = 0;
      for (int w = 0; w < nwaves; ++w) {
        const unsigned long long t = sc.wave_tot[w];
        if (w < wave) before += t;
        total += t;
      }
      unsigned long long run = before + incl2 - tsum;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        run += q[j];
        if (i0 + j < M) cdf[i0 + j] = run;
      }
      carry += total;
      __syncthreads();
    }
  }
  if (!need_cdf || SOFT) {  // (plain resampling did this on its last chunk's barriers)
    S = mmf::wave_sum(S);
#pragma unroll
    for (int c = 0; c < D; ++c) acc[c] = mmf::wave_sum(acc[c]);
    if (lane == 0) {
      sc.red[wave][0] = S;
#pragma unroll
      for (int c = 0; c < D; ++c) sc.red[wave][1 + c] = acc[c];
    }
    __syncthreads();
    if (tid <= D) {
      float t = 0.f;
      for (int w = 0; w < nwaves; ++w) t += sc.red[w][tid];
      sc.bcast[tid] = t;
    }
    __syncthreads();
  }
  K1_STAMP(2);
  S = sc.bcast[0];
  if (tid < D) estimate[static_cast<size_t>(n) * D + tid] = sc.bcast[1 + tid] / S;
  if constexpr (REC) {  // a round of its own: this kernel is not the one on the small problems' critical path
#pragma unroll
    for (int k = 0; k < mmf::K1Belief<D>::kSums; ++k) {
      const float bw = mmf::wave_sum(bel.s[k]);
      if (lane == 0) bsc.red[wave][k] = bw;
    }
    __syncthreads();
    if (tid < mmf::K1Belief<D>::kSums) {
      float t = 0.f;
      for (int w = 0; w < nwaves; ++w) t += bsc.red[w][tid];
      bsc.tot[tid] = t;
    }
    __syncthreads();
    mmf::k1_belief_store<D>(bsc.tot, S, mx, rec.cov ? rec.cov + static_cast<size_t>(n) * D * D : nullptr,
                            rec.ess ? rec.ess + n : nullptr, rec.log_evidence ? rec.log_evidence + n : nullptr, tid);
  } else if constexpr (ADAPT) {  // sum e^2 in the record's partition: per thread, a butterfly per wave, the waves in order
    const float bw = mmf::wave_sum(w2);
    if (lane == 0) bsc.red[wave][0] = bw;
    __syncthreads();
    if (tid == 0) {
      float t = 0.f;
      for (int w = 0; w < nwaves; ++w) t += bsc.red[w][0];
      bsc.tot[0] = t;
    }
    __syncthreads();
  }
  if constexpr (ADAPT) {
    // S and sum e^2 are the broadcast totals (LDS), so every lane of every wave takes the same side
    const bool keep = mmf::k1_ess(S, bsc.tot[0]) >= ad.ess_floor;  // a NaN resamples, a tie keeps
    if (tid == 0 && ad.resampled != nullptr) ad.resampled[n] = keep ? 0 : 1;
    if (keep) {
      // mode 0's outputs (M_out == M).  The slots hold the CDF by now: x_i is formed again from the inputs (the same addition)
      const float logS = logf(S);
      float* lo = logw_out + static_cast<size_t>(n) * M;
      float* so = states_out + static_cast<size_t>(n) * M * D;
      int32_t* io = indices_out ? indices_out + static_cast<size_t>(n) * M : nullptr;
      for (int i = tid; i < M; i += blockDim.x) {
        const float x = (lw ? lw[i] : lw_uniform) + ll[i];
        lo[i] = (x - mx) - logS;
#pragma unroll
        for (int c = 0; c < D; ++c) so[static_cast<size_t>(i) * D + c] = STAGE ? xs_lds[i * D + c] : xs[static_cast<size_t>(i) * D + c];
        if (io) io[i] = i;
      }
      return;
    }
  }

  // ---- mode 0: normalised log-weights out, particles stay
  if (!need_cdf) {
    const float logS = logf(S);
    float* lo = logw_out + static_cast<size_t>(n) * M;
    float* so = states_out ? states_out + static_cast<size_t>(n) * M * D : nullptr;
    const bool copy = so != nullptr && so != xs;
    for (int i = tid; i < M; i += blockDim.x) {
      lo[i] = (xf[i] - mx) - logS;
      if (copy) {
#pragma unroll
        for (int c = 0; c < D; ++c) so[static_cast<size_t>(i) * D + c] = xs[static_cast<size_t>(i) * D + c];
      }
    }
    return;
  }

  // ---- modes 1/2: positions -> ancestor index by upper_bound in the LDS CDF -> gather
  const unsigned long long Q = cdf[M - 1];
  unsigned long long R = 0;
  if (mode == 1) {
    const unsigned long long U = static_cast<unsigned long long>(floorf(u[n] * 16777216.0f));
    R = (U * Q) >> kFixBits;
  }
  const bool pow2 = (M_out & (M_out - 1)) == 0;
  const int shift = __ffs(M_out) - 1;
  float* so = states_out + static_cast<size_t>(n) * M_out * D;
  // logw_out == nullptr (plain resampling only): the survivors' weights are -log M_out by definition
  float* lo = logw_out ? logw_out + static_cast<size_t>(n) * M_out : nullptr;
  int32_t* io = indices_out ? indices_out + static_cast<size_t>(n) * M_out : nullptr;
  const float* un = (mode == 2) ? u + static_cast<size_t>(n) * M_out : nullptr;
  const bool vec_out = (M_out & 3) == 0;
  const float mix_uniform = (1.0f - alpha) * S / static_cast<float>(M);
  float rsum = 0.f;

  for (int base = 0; base < M_out; base += chunk) {
    const int k0 = base + tid * 4;
    int idx[4];
    float g[4 * D];
    float lr[4] = {log_uniform, log_uniform, log_uniform, log_uniform};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + j;
      idx[j] = 0;
      if (k < M_out) {
        unsigned long long p;
        if (mode == 1) {
          const unsigned long long num = static_cast<unsigned long long>(k) * Q + R;
          p = pow2 ? (num >> shift) : (num / static_cast<unsigned long long>(M_out));
        } else {
          const unsigned long long U = static_cast<unsigned long long>(floorf(un[k] * 16777216.0f));
          p = (U * Q) >> kFixBits;
        }
        int lo_i = 0, hi_i = M;
        if (mode == 1 && j > 0) {
          // systematic positions are sorted and evenly spaced: the ancestor of output k sits at or
          // just above that of output k - 1 -- gallop from there (2-3 LDS reads on average
          // instead of log2 M) before the bisection
          lo_i = idx[j - 1];
          int step = 1;
          while (lo_i + step <= M && cdf[lo_i + step - 1] <= p) { lo_i += step; step <<= 1; }
          hi_i = min(M, lo_i + step - 1);
        }
        while (lo_i < hi_i) {
          const int mid = (lo_i + hi_i) >> 1;
          if (cdf[mid] <= p) lo_i = mid + 1; else hi_i = mid;
        }
        idx[j] = lo_i;
#pragma unroll
        for (int c = 0; c < D; ++c) g[j * D + c] = STAGE ? xs_lds[lo_i * D + c] : xs[static_cast<size_t>(lo_i) * D + c];
        if (SOFT) {  // importance weight of the survivor: w / (alpha w + (1 - alpha) / M), up to the common 1 / S
          const float e = mmf::detexp(((lw ? lw[lo_i] : lw_uniform) + ll[lo_i]) - mx);
          const float r = e / (alpha * e + mix_uniform);
          rsum += r;
          lr[j] = logf(r);
        }
      }
    }
    if (vec_out && k0 + 3 < M_out) {
      float4* p = reinterpret_cast<float4*>(so + static_cast<size_t>(k0) * D);
#pragma unroll
      for (int k = 0; k < D; ++k) p[k] = make_float4(g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]);
      if (lo) *reinterpret_cast<float4*>(lo + k0) = make_float4(lr[0], lr[1], lr[2], lr[3]);
      if (io) *reinterpret_cast<int4*>(io + k0) = make_int4(idx[0], idx[1], idx[2], idx[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + j;
        if (k < M_out) {
#pragma unroll
          for (int c = 0; c < D; ++c) so[static_cast<size_t>(k) * D + c] = g[j * D + c];
          if (lo) lo[k] = lr[j];
          if (io) io[k] = idx[j];
        }
      }
    }
  }
  K1_STAMP(3);
  if (SOFT) {  // normalise the survivors' weights (every thread revisits the outputs it wrote)
    rsum = mmf::wave_sum(rsum);
    __syncthreads();
    if (lane == 0) sc.red[wave][0] = rsum;
    __syncthreads();
    float t = 0.f;
    for (int w = 0; w < nwaves; ++w) t += sc.red[w][0];
    const float log_r = logf(t);
    for (int base = 0; base < M_out; base += chunk)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = base + tid * 4 + j;
        if (k < M_out) lo[k] -= log_r;
      }
  }
}


// ---- plain systematic resampling WITHOUT a search (the bench's and the reference's evaluation mode): the body is
// mmf::resample_systematic_trajectory (pf_resample_systematic.inc, shared with the persistent small-problem loop)
template <int D, bool STAGE, bool REC = false, bool ADAPT = false>
__global__ __launch_bounds__(kBlock) void pf_resample_systematic_kernel(
    const float* __restrict__ loglik, const float* __restrict__ logw_in, const float* __restrict__ states_in,
    const float* __restrict__ u, float* __restrict__ estimate, float* states_out, float* logw_out,
    int32_t* __restrict__ indices_out, int M, int M_out, float lw_uniform, float log_uniform, BeliefOut rec, AdaptIn ad) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n = blockIdx.x;
  mmf::K1Trajectory a{};
  a.ll[0] = loglik + static_cast<size_t>(n) * M;
  a.n_ll = 1;
  a.lw = logw_in ? logw_in + static_cast<size_t>(n) * M : nullptr;
  a.xs = states_in + static_cast<size_t>(n) * M * D;
  a.u = u[n];
  a.estimate = estimate + static_cast<size_t>(n) * D;
  a.so = states_out + static_cast<size_t>(n) * M_out * D;
  a.lo = logw_out ? logw_out + static_cast<size_t>(n) * M_out : nullptr;
  a.io = indices_out ? indices_out + static_cast<size_t>(n) * M_out : nullptr;
  if constexpr (REC) {
    a.cov = rec.cov ? rec.cov + static_cast<size_t>(n) * D * D : nullptr;
    a.ess = rec.ess ? rec.ess + n : nullptr;
    a.log_evidence = rec.log_evidence ? rec.log_evidence + n : nullptr;
  }
  if constexpr (ADAPT) {
    a.ess_floor = ad.ess_floor;
    a.resampled = ad.resampled ? ad.resampled + n : nullptr;
  }
  mmf::resample_systematic_trajectory<D, STAGE, false, false, REC, ADAPT>(smem, a, M, M_out, lw_uniform, log_uniform);
}

// K1 of a step whose successor is the run-consuming dynamics kernel (pf_loop.hip): the same body with RUNS -- the run table
// instead of the gathered particles; no staging (nothing is gathered)
struct RunTableOut { int32_t* rank; int32_t* run_anc; int32_t* run_start; int32_t* n_runs; };  // (N, M), (N, M + 1) x 2, (N)

template <int D, bool REC>
__global__ __launch_bounds__(kBlock) void pf_resample_runs_kernel(
    const float* __restrict__ loglik, const float* __restrict__ logw_in, const float* __restrict__ states_in,
    const float* __restrict__ u, float* __restrict__ estimate, float* logw_out, int32_t* __restrict__ indices_out,
    RunTableOut rt, int M, float lw_uniform, BeliefOut rec) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n = blockIdx.x;
  mmf::K1Trajectory a{};
  a.ll[0] = loglik + static_cast<size_t>(n) * M;
  a.n_ll = 1;
  a.lw = logw_in ? logw_in + static_cast<size_t>(n) * M : nullptr;
  a.xs = states_in + static_cast<size_t>(n) * M * D;
  a.u = u[n];
  a.estimate = estimate + static_cast<size_t>(n) * D;
  a.lo = logw_out ? logw_out + static_cast<size_t>(n) * M : nullptr;
  a.io = indices_out ? indices_out + static_cast<size_t>(n) * M : nullptr;
  a.rank = rt.rank + static_cast<size_t>(n) * M;
  a.run_anc = rt.run_anc + static_cast<size_t>(n) * (M + 1);
  a.run_start = rt.run_start + static_cast<size_t>(n) * (M + 1);
  a.n_runs = rt.n_runs + n;
  if constexpr (REC) {
    a.cov = rec.cov ? rec.cov + static_cast<size_t>(n) * D * D : nullptr;
    a.ess = rec.ess ? rec.ess + n : nullptr;
    a.log_evidence = rec.log_evidence ? rec.log_evidence + n : nullptr;
  }
  mmf::resample_systematic_trajectory<D, false, false, false, REC, false, true>(smem, a, M, M, lw_uniform, lw_uniform);
}

// dynamic LDS of the run variant: CDF slots, scratch, marks (+ the record's rows); no state is staged, so d does not enter
size_t runs_lds_bytes(int M, bool recording) { return mmf::k1_systematic_lds(M, M, 0, false, recording).end; }

}  // namespace

extern "C" int mmf_pf_dedup_plan(int M, int d, int resample_mode, float soft_alpha, int recording) {
  if (M < 1 || d < 1) return MMF_EINVAL;
  const bool soft = resample_mode != 0 && soft_alpha > 0.f && soft_alpha < 1.f;
  if (resample_mode != 1 || soft) return 0;
  if (M % 64 != 0 || (d != 2 && d != 3)) return 0;
  return runs_lds_bytes(M, recording != 0) <= mmf::kLdsPerCu ? 1 : 0;
}

extern "C" size_t mmf_pf_dedup_workspace_words(int N, int M) {
  if (N < 0 || M < 1) return 0;
  return static_cast<size_t>(N) * M + 2 * static_cast<size_t>(N) * (static_cast<size_t>(M) + 1) + static_cast<size_t>(N);
}

extern "C" int mmf_pf_resample_runs(const float* loglik, const float* logw_in, const float* states_in, const float* u,
                                    float* estimate, float* logw_out, int32_t* indices_out, int32_t* rank, int32_t* run_anc,
                                    int32_t* run_start, int32_t* n_runs, int N, int M, int d, float* cov, float* ess,
                                    float* log_evidence, void* stream) {
  if (!loglik || !states_in || !u || !estimate || !rank || !run_anc || !run_start || !n_runs) return MMF_EINVAL;
  if (N < 0 || M < 1 || d < 1 || d > MMF_MAX_STATE_DIM) return MMF_EINVAL;
  const bool recording = cov || ess || log_evidence;
  const size_t bytes = runs_lds_bytes(M, recording);
  if (M > 65536 || bytes > mmf::kLdsPerCu) return MMF_ETOOLARGE;
  if (N == 0) return 0;
  int block = ((M + 3) / 4 + MMF_WAVE - 1) / MMF_WAVE * MMF_WAVE;
  if (block > kBlock) block = kBlock;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float lw_uniform = static_cast<float>(-std::log(static_cast<double>(M)));
  const RunTableOut rt{rank, run_anc, run_start, n_runs};
  const BeliefOut rec{cov, ess, log_evidence};
  return mmf::with_state_dim(d, [&](auto D) {
    return mmf::with_bool(recording, [&](auto RC) {
      return mmf::launch(pf_resample_runs_kernel<decltype(D)::value, decltype(RC)::value>, N, block, bytes, s, loglik, logw_in,
                         states_in, u, estimate, logw_out, indices_out, rt, M, lw_uniform, rec);
    });
  });
}

extern "C" size_t mmf_pf_reweight_resample_lds_bytes(int M, int mode) {
  return mmf::k1_search_lds(M, mode, 0, false, false).end;
}

namespace {
int launch_reweight_resample(const float* loglik, const float* logw_in, const float* states_in, const float* u,
                             float* estimate, float* states_out, float* logw_out, int32_t* indices_out, int N,
                             int M, int M_out, int d, int mode, float alpha, BeliefOut rec, void* stream,
                             float ess_threshold = 0.f, int32_t* resampled = nullptr) {  // > 0: the adaptive call
  if (!loglik || !states_in || !estimate) return MMF_EINVAL;
  if (N < 0 || M < 1 || M_out < 1 || d < 1 || d > MMF_MAX_STATE_DIM || mode < 0 || mode > 2) return MMF_EINVAL;
  // the uniform-weight shortcuts (null logw_in / logw_out) belong to plain resampling
  if ((!logw_in || !logw_out) && (mode == 0 || alpha < 1.f)) return MMF_EINVAL;
  if (mode != 0 && (!u || !states_out || states_out == states_in)) return MMF_EINVAL;
  if (mode == 0 && M_out != M) return MMF_EINVAL;
  if (!(alpha > 0.f && alpha <= 1.f)) return MMF_EINVAL;
  if (M > 65536 || M_out > 65536) return MMF_ETOOLARGE;
  // a recording call keeps its sums' reduction rows behind everything else in LDS (the non-recording layout and
  // limits are untouched): M <= 20,200 in modes 1/2, 40,500 in mode 0
  const bool recording = rec.cov || rec.ess || rec.log_evidence;
  const bool adaptive = ess_threshold > 0.f;  // reduces sum e^2 through the record's rows: the recording call's layout and limits
  const AdaptIn ad{ess_threshold * static_cast<float>(M), resampled};  // the product rounded once, in fp32
  const bool rows = recording || adaptive;
  const size_t unstaged = mmf::k1_search_lds(M, mode, d, false, rows).end;
  if (unstaged > mmf::kLdsPerCu) return MMF_ETOOLARGE;
  if (N == 0) return 0;
  const bool soft = mode != 0 && alpha < 1.f;
  const size_t staged = mmf::k1_search_lds(M, mode, d, true, rows).end;
  const bool stage = mode != 0 && mmf::k1_stage_fits(N, staged);
  const size_t lds = stage ? staged : unstaged;
  // enough threads to give each one a float4 of work, at least one wave
  int block = ((M + 3) / 4 + MMF_WAVE - 1) / MMF_WAVE * MMF_WAVE;
  if (block > kBlock) block = kBlock;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float lw_uniform = static_cast<float>(-std::log(static_cast<double>(M)));
  const float log_uniform = static_cast<float>(-std::log(static_cast<double>(M_out)));
  if (mode == 1 && !soft && (d == 2 || d == 3)) {
    // few trajectories (round 6): a cluster of workgroups per trajectory, two meetings through L2, the same bits
    int dev = 0, cus = 0;
    if (g_cluster_enabled && !recording && !adaptive && hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) {
      const int C = cluster::plan(N, M, M_out, cus);
      if (C > 0) {
        // exchange area: kLanes launches' worth (consecutive launches never share one: a late reader of launch k cannot
        // meet launch k + 1's granules), tags from a counter that never repeats, zeroed once; per device
        constexpr int kLanes = 8, kMaxDevices = 16;
        static mmf::Granule* area[kMaxDevices] = {};
        static unsigned counter = 0;
        if (dev < 0 || dev >= kMaxDevices) return MMF_EINVAL;
        const size_t lane_granules = static_cast<size_t>(cus / 2) * cluster::kGranulesPerTraj;  // plan(): N <= cus / 2
        if (!area[dev]) {
          const size_t bytes = (kLanes * lane_granules + 2) * sizeof(mmf::Granule);
          if (hipMalloc(reinterpret_cast<void**>(&area[dev]), bytes) != hipSuccess) return MMF_EINVAL;
          if (hipMemsetAsync(area[dev], 0, bytes, s) != hipSuccess) return MMF_EINVAL;
        }
        ++counter;
        if (counter == 0) counter = 1;  // tag 0 is "never written"
        cluster::Args ca{};
        ca.loglik = loglik; ca.logw_in = logw_in; ca.states_in = states_in; ca.u = u; ca.estimate = estimate;
        ca.states_out = states_out; ca.logw_out = logw_out; ca.indices_out = indices_out;
        ca.exchange = area[dev] + (counter % kLanes) * lane_granules;
        ca.error_word = reinterpret_cast<unsigned*>(area[dev] + kLanes * lane_granules);
        ca.M = M; ca.M_out = M_out; ca.C = C; ca.tag = counter;
        ca.lw_uniform = lw_uniform; ca.log_uniform = log_uniform;
        const int threads = M / (4 * C);
        const size_t bytes = cluster::lds_bytes(M_out, threads, d);
        if (d == 3) cluster::pf_resample_cluster_kernel<3><<<dim3(C, N), threads, bytes, s>>>(ca);
        else cluster::pf_resample_cluster_kernel<2><<<dim3(C, N), threads, bytes, s>>>(ca);
        MMF_CHECK_LAUNCH();
        return 0;
      }
    }
  }
  if (mode == 1 && !soft && M <= 20000 && M_out <= 20000) {
    // plain systematic resampling: the search-free kernel (offspring boundaries + prefix sum of marks)
    const size_t base_sz = mmf::k1_systematic_lds(M, M_out, d, false, rows).end;
    if (base_sz <= mmf::kLdsPerCu) {
      const size_t with_states = mmf::k1_systematic_lds(M, M_out, d, true, rows).end;
      const bool st = mmf::k1_stage_fits(N, with_states);
      return mmf::with_state_dim(d, [&](auto D) {
        return mmf::with_bool(st, [&](auto ST) {
          return mmf::with_bool(recording, [&](auto RC) {
            return mmf::with_bool(adaptive, [&](auto AD) {
              return mmf::launch(pf_resample_systematic_kernel<decltype(D)::value, decltype(ST)::value, decltype(RC)::value, decltype(AD)::value>,
                                 N, block, st ? with_states : base_sz, s, loglik, logw_in, states_in, u, estimate, states_out,
                                 logw_out, indices_out, M, M_out, lw_uniform, log_uniform, rec, ad);
            });
          });
        });
      });
    }
  }
  return mmf::with_state_dim(d, [&](auto D) {
    return mmf::with_bool(stage, [&](auto ST) {
      return mmf::with_bool(soft, [&](auto SO) {
        return mmf::with_bool(recording, [&](auto RC) {
          return mmf::with_bool(adaptive, [&](auto AD) {
            return mmf::launch(pf_reweight_resample_kernel<decltype(D)::value, decltype(ST)::value, decltype(SO)::value, decltype(RC)::value, decltype(AD)::value>,
                               N, block, lds, s, loglik, logw_in, states_in, u, estimate, states_out, logw_out, indices_out, M,
                               M_out, mode, alpha, lw_uniform, log_uniform, rec, ad);
          });
        });
      });
    });
  });
}
}  // namespace

namespace {
// estimation_method = "argmax": one workgroup per trajectory; value = logw_in + loglik (ONE fp32 add, as the
// step-by-step path's torch expression), larger value wins, smaller index on ties (torch.argmax)
template <int D>
__global__ __launch_bounds__(256) void pf_argmax_estimate_kernel(const float* __restrict__ loglik,
                                                                 const float* __restrict__ logw_in,
                                                                 const float* __restrict__ states,
                                                                 float* __restrict__ estimate, int M, float lw_uniform) {
  __shared__ float best_v[256 / MMF_WAVE];
  __shared__ int best_i[256 / MMF_WAVE];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* ll = loglik + static_cast<size_t>(n) * M;
  const float* lw = logw_in ? logw_in + static_cast<size_t>(n) * M : nullptr;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = tid; i < M; i += blockDim.x) {
    const float v = (lw ? lw[i] : lw_uniform) + ll[i];
    if (v > bv || (v == bv && i < bi) || bi == 0x7fffffff) { bv = v; bi = i; }
  }
  auto better = [](float v, int i, float w, int j) { return v > w || (v == w && i < j); };
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
  if ((tid & (MMF_WAVE - 1)) == 0) { best_v[tid >> 6] = bv; best_i[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < static_cast<int>(blockDim.x >> 6); ++w)
      if (better(best_v[w], best_i[w], bv, bi)) { bv = best_v[w]; bi = best_i[w]; }
    if (bi >= M) bi = 0;  // every value NaN: torch.argmax would pick a NaN's index; the filter is lost either way
#pragma unroll
    for (int c = 0; c < D; ++c) estimate[static_cast<size_t>(n) * D + c] = states[(static_cast<size_t>(n) * M + bi) * D + c];
  }
}
}  // namespace

extern "C" int mmf_pf_argmax_estimate(const float* loglik, const float* logw_in, const float* states, float* estimate,
                                      int N, int M, int d, void* stream) {
  if (!loglik || !states || !estimate) return MMF_EINVAL;
  if (N < 0 || M < 1 || d < 1 || d > MMF_MAX_STATE_DIM) return MMF_EINVAL;
  if (N == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const float lw_uniform = static_cast<float>(-std::log(static_cast<double>(M)));
  switch (d) {
    case 1: pf_argmax_estimate_kernel<1><<<N, 256, 0, s>>>(loglik, logw_in, states, estimate, M, lw_uniform); break;
    case 2: pf_argmax_estimate_kernel<2><<<N, 256, 0, s>>>(loglik, logw_in, states, estimate, M, lw_uniform); break;
    case 3: pf_argmax_estimate_kernel<3><<<N, 256, 0, s>>>(loglik, logw_in, states, estimate, M, lw_uniform); break;
    default: pf_argmax_estimate_kernel<4><<<N, 256, 0, s>>>(loglik, logw_in, states, estimate, M, lw_uniform); break;
  }
  MMF_CHECK_LAUNCH();
  return 0;
}

extern "C" void mmf_pf_set_resample_cluster(int enabled) { g_cluster_enabled = enabled != 0; }
extern "C" int mmf_pf_get_resample_cluster(void) { return g_cluster_enabled; }

extern "C" int mmf_pf_reweight_resample(const float* loglik, const float* logw_in,
                                        const float* states_in, const float* u, float* estimate,
                                        float* states_out, float* logw_out, int32_t* indices_out,
                                        int N, int M, int M_out, int d, int mode, void* stream) {
  return mmf_pf_reweight_resample_belief(loglik, logw_in, states_in, u, estimate, states_out, logw_out, indices_out, N, M,
                                         M_out, d, mode, 1.0f, nullptr, nullptr, nullptr, stream);
}

extern "C" int mmf_pf_reweight_resample_soft(const float* loglik, const float* logw_in,
                                             const float* states_in, const float* u, float* estimate,
                                             float* states_out, float* logw_out, int32_t* indices_out,
                                             int N, int M, int M_out, int d, int mode, float alpha,
                                             void* stream) {
  if (mode == 0) return MMF_EINVAL;
  return mmf_pf_reweight_resample_belief(loglik, logw_in, states_in, u, estimate, states_out, logw_out, indices_out, N, M,
                                         M_out, d, mode, alpha, nullptr, nullptr, nullptr, stream);
}

extern "C" int mmf_pf_reweight_resample_belief(const float* loglik, const float* logw_in, const float* states_in,
                                               const float* u, float* estimate, float* states_out, float* logw_out,
                                               int32_t* indices_out, int N, int M, int M_out, int d, int mode,
                                               float alpha, float* cov, float* ess, float* log_evidence, void* stream) {
  if (mode == 0 && alpha != 1.f) return MMF_EINVAL;  // soft resampling needs a resampling mode
  return launch_reweight_resample(loglik, logw_in, states_in, u, estimate, states_out, logw_out, indices_out, N, M,
                                  M_out, d, mode, alpha, BeliefOut{cov, ess, log_evidence}, stream);
}

extern "C" int mmf_pf_reweight_resample_adaptive(const float* loglik, const float* logw_in, const float* states_in,
                                                 const float* u, float* estimate, float* states_out, float* logw_out,
                                                 int32_t* indices_out, int N, int M, int d, int mode, float alpha,
                                                 float ess_threshold, int32_t* resampled, float* cov, float* ess,
                                                 float* log_evidence, void* stream) {
  if (mode != 1 && mode != 2) return MMF_EINVAL;                            // a threshold needs a resampling mode
  if (!(ess_threshold > 0.f && ess_threshold <= 1.f)) return MMF_EINVAL;    // (a NaN fails both comparisons)
  if (!logw_out || logw_out == logw_in) return MMF_EINVAL;                  // a kept trajectory's weights go somewhere else
  if (!(alpha > 0.f && alpha <= 1.f)) return MMF_EINVAL;
  // everything else -- null pointers, the in-place gather, d, the size limits (those of a recording call) -- is the launcher's
  return launch_reweight_resample(loglik, logw_in, states_in, u, estimate, states_out, logw_out, indices_out, N, M, M, d,
                                  mode, alpha, BeliefOut{cov, ess, log_evidence}, stream, ess_threshold, resampled);
}
