// K1, plain systematic resampling WITHOUT a search, as a device function of ONE trajectory and one workgroup:
// shared by pf_resample_systematic_kernel (pf_resample.hip: one launch per filter step) and by the persistent
// small-problem loop (pf_persistent.inc: the K1 workgroups of ONE launch per forward_loop), so both evaluate the
// same operations in the same order and produce the same bits.
//
// Same fixed-point definition as the search kernel (oracle/resample.py), evaluated from the input side: particle i
// is the ancestor of the outputs k with cdf_{i-1} <= p_k < cdf_i, and since p_k = (k Q + R) // M_out is
// non-decreasing, #{k : p_k < cdf_i} = k_end(i) = ceil((cdf_i M_out - R) / Q) (0 when cdf_i M_out <= R, at most
// M_out).  The first particle of every run of equal k_end announces itself, marks[k_end(i - 1)] = i when
// k_end(i - 1) < k_end(i) -- one writer per entry, plain LDS stores -- and ancestor(k) is the inclusive prefix
// MAXIMUM of marks (one block scan on DPP).  No dependent chain of LDS reads per output, and a thread needs only
// the CDF entries of its own four particles, which it still holds in registers.
//
// The workgroup may be LARGER than the launch path's (float4 of work per thread, rounded up to waves): thread t
// owns particles 4t .. 4t+3 of every chunk either way, the surplus waves contribute the neutral element to every
// reduction (-inf to the max, +0.0 to the float sums -- x + 0.0 is exact --, 0 to the integer scans), so the
// result does not depend on the workgroup size.
//
// COH (persistent loop): every value another workgroup of the SAME launch wrote or will read travels as an 8-byte
// GRANULE {value, tag} moved by ONE agent-scope relaxed atomic (global_load / global_store_dwordx2 ... sc1: served
// by / written through to L2, never a stale per-CU L1 line; MI355X_MICROARCH.md, inter-workgroup visibility;
// cdna_hip_programming.md Guideline 16, R2: the data IS the flag).  tag = step + 1: a reader spins on its own
// granules until the tag is the step's, so no separate flag, fence or store drain sits on the chain.  The
// log-likelihood is the logaddexp chain over the modalities' own arrays (what the launch path's measurement
// kernels combine in their epilogues), evaluated by one thread per particle before pass 1.
#pragma once

#include "mmf_granule.h"
#include "mmf_launch.h"

#ifndef K1_STAMP  // phase stamps of scripts/ubench/k1_phases.hip (pf_resample.hip defines it under MMF_K1_PHASE_CLOCKS)
#define K1_STAMP(i)
#endif

namespace mmf {

constexpr int kK1Block = 1024;  // 16 waves; M = 4096 -> one float4 chunk per thread
constexpr int kK1MaxWaves = kK1Block / MMF_WAVE;
constexpr int kK1FixBits = 24;

struct K1Scratch {  // lives behind the slots in dynamic LDS
  float red[kK1MaxWaves][MMF_MAX_STATE_DIM + 1];
  unsigned long long wave_tot[kK1MaxWaves];
  float bcast[MMF_MAX_STATE_DIM + 2];
  unsigned wave_cnt[kK1MaxWaves];
  unsigned gave_up;  // COH: a reader timed out (zero on entry: the persistent loop's K1 workgroups clear it once)
};

// The belief record of a step (include/mmf.h, K1: covariance / ESS / log-evidence of the pre-resampling weighted set), compiled
// in by the REC flag of the kernels below.  One pass, next to the estimate's sums and in the same partition (so every form
// of K1 produces the same bits): with e_m = exp(a_m - max) and the FIRST highest-weight particle p as pivot,
//   W2 = sum e^2,  m1_i = sum e (x_i - p_i),  M2_ij = sum e (x_i - p_i)(x_j - p_j)   (i >= j)
//   covariance = M2 / S - (m1 / S)(m1 / S)^T,  ess = S^2 / W2,  log_evidence = max + log S.
// Deviations from a particle inside the cloud keep fp32 meaningful where raw moments of O(1) states lose a 1e-3-wide
// cloud entirely; the highest-weight particle is never far from the mass (a fixed particle is, once the weight collapses).
// A particle of weight exp(-inf) contributes exactly nothing (detexp clamps it to 2^-126 for the resampler's CDF).
template <int D>
struct K1Belief {
  static constexpr int kM2 = D * (D + 1) / 2;
  static constexpr int kSums = 1 + D + kM2;
  float s[kSums];  // [W2, m1[D], M2 (lower triangle, row by row)]
  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int k = 0; k < kSums; ++k) s[k] = 0.f;
  }
  __device__ __forceinline__ void add(float e, const float* x, const float* piv) {
    s[0] = __builtin_fmaf(e, e, s[0]);
    float dx[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      dx[i] = x[i] - piv[i];
      s[1 + i] = __builtin_fmaf(e, dx[i], s[1 + i]);
    }
    int k = 1 + D;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const float t = e * dx[i];
#pragma unroll
      for (int j = 0; j <= i; ++j, ++k) s[k] = __builtin_fmaf(t, dx[j], s[k]);
    }
  }
};
constexpr int kK1BeliefMaxSums = 1 + MMF_MAX_STATE_DIM + MMF_MAX_STATE_DIM * (MMF_MAX_STATE_DIM + 1) / 2;

struct K1BeliefScratch {  // REC / ADAPT only: behind everything else in dynamic LDS (mmf::k1_belief_lds_bytes)
  float red[kK1MaxWaves][kK1BeliefMaxSums];
  float tot[kK1BeliefMaxSums];
  float piv_wave[kK1MaxWaves];  // per wave: -(smallest index holding the row maximum), -inf: none
};
constexpr size_t k1_belief_lds_bytes() { return (sizeof(K1BeliefScratch) + 15) & ~static_cast<size_t>(15); }

// ---- The dynamic LDS of every form of K1, host side: the ONE place a launcher's byte count and stage decision come from.
// Behind the slots (offset 0) lie, each at the next multiple of 16 bytes: K1Scratch, the marks (search-free kernel only), the
// staged states (STAGE), the belief rows (REC / ADAPT).  `end` is the end of the last section in use -- the launch's dynamic LDS;
// nothing is rounded behind it.  The device prologues (resample_systematic_trajectory below, pf_reweight_resample_kernel in
// pf_resample.hip) keep their own offset arithmetic and must agree: a host sum below theirs is an out-of-bounds LDS write.
constexpr size_t k1_align16(size_t bytes) { return (bytes + 15) & ~static_cast<size_t>(15); }

struct K1Lds { size_t scratch, marks, states, belief, end; };

constexpr K1Lds k1_lds_sections(size_t slots_bytes, size_t marks_bytes, size_t states_bytes, bool with_belief_rows) {
  K1Lds p{};
  p.scratch = k1_align16(slots_bytes);
  p.end = p.scratch + sizeof(K1Scratch);
  p.marks = k1_align16(p.end);
  if (marks_bytes != 0) p.end = p.marks + marks_bytes;
  p.states = k1_align16(p.end);
  if (states_bytes != 0) p.end = p.states + states_bytes;
  p.belief = k1_align16(p.end);
  if (with_belief_rows) p.end = p.belief + k1_belief_lds_bytes();
  return p;
}
// the search-free kernels (resample_systematic_trajectory): u64 CDF slots; M_out + 4 marks, read as uint4 -- whole 16 bytes
constexpr K1Lds k1_systematic_lds(int M, int M_out, int d, bool staged, bool with_belief_rows) {
  return k1_lds_sections(static_cast<size_t>(M) * 8, k1_align16((static_cast<size_t>(M_out) + 4) * 4),
                         staged ? static_cast<size_t>(M) * d * sizeof(float) : 0, with_belief_rows);
}
// the search kernel (pf_reweight_resample_kernel): fp32 slots in mode 0, the u64 CDF in modes 1 / 2; no marks
constexpr K1Lds k1_search_lds(int M, int mode, int d, bool staged, bool with_belief_rows) {
  return k1_lds_sections(static_cast<size_t>(M) * (mode ? 8 : 4), 0, staged ? static_cast<size_t>(M) * d * sizeof(float) : 0,
                         with_belief_rows);
}
// The staging rule: the states go to LDS when occupancy does not pay for it -- always if every trajectory gets a CU of its own
// (N <= 256), otherwise only while two workgroups still fit a CU
constexpr bool k1_stage_fits(int N, size_t staged_bytes) { return staged_bytes <= (N <= 256 ? kLdsPerCu : kLdsHalfCu); }

// the outputs of one trajectory, from the reduced sums (threads 0 .. D*D - 1 write; symmetric bit for bit: entry (i, j) and
// (j, i) evaluate the same expression on the same operands)
template <int D>
__device__ __forceinline__ void k1_belief_store(const float* tot, float S, float mx, float* cov, float* ess, float* log_evidence, int tid) {
#pragma clang fp contract(off)
  if (cov != nullptr && tid < D * D) {
    const int i = tid / D, j = tid % D;
    const int hi = i > j ? i : j, lo = i > j ? j : i;
    const float m2 = tot[1 + D + hi * (hi + 1) / 2 + lo];
    const float bi = tot[1 + hi] / S, bj = tot[1 + lo] / S;
    cov[tid] = m2 / S - bi * bj;
  }
  if (tid == 0) {
    if (ess != nullptr) *ess = (S * S) / tot[0];
    if (log_evidence != nullptr) *log_evidence = mx + logf(S);
  }
}

// ADAPT (ESS-triggered resampling, include/mmf.h): the effective sample size from the reduced sums, the expression -- and so the
// bits -- k1_belief_store writes as the record's `ess`; a trajectory is KEPT iff k1_ess(...) >= fl32(threshold * M)
__device__ __forceinline__ float k1_ess(float S, float W2) {
#pragma clang fp contract(off)
  return (S * S) / W2;
}

__device__ __forceinline__ float ld_coherent(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_coherent(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the crossmodal combine of two modalities' log-likelihoods, as the measurement kernel's epilogue evaluates it
// (exact-fp32 mode: the shared deterministic logaddexp of include/mmf_detmath.h)
template <bool DET>
__device__ __forceinline__ float combine_loglik(float prev, float ll) {
  if constexpr (DET) {
    return mmf_det_logaddexp(prev, ll);
  } else {
    const float m = fmaxf(prev, ll);
    return (m == -INFINITY) ? m : m + logf(expf(prev - m) + expf(ll - m));
  }
}

struct K1Trajectory {  // pointers of ONE trajectory's rows
  const float* ll[MMF_LOOP_MAX_MEAS];  // [n_ll] log-likelihoods (M); COH: granules (M), n_ll > 1 combined in order
  int n_ll;
  const float* lw;       // (M) incoming log-weights or null (uniform)
  const float* xs;       // (M, D) propagated particles; COH: granules (M, D)
  float u;               // this trajectory's uniform
  float* estimate;       // (D)
  float* cov;            // REC: (D, D) covariance of the weighted set, or null
  float* ess;            // REC: effective sample size, or null
  float* log_evidence;   // REC: logsumexp of the unnormalised log-weights, or null
  float* so;             // (M_out, D) resampled particles; COH with so_tag != 0: granules (M_out, D) tagged so_tag
  float* lo;             // (M_out) or null (uniform by definition)
  int32_t* io;           // (M_out) ancestors or null
  unsigned in_tag;       // COH: the tag this step's log-likelihood / particle granules carry
  unsigned so_tag;       // COH: tag of the granules written (0: plain floats -- the loop's last step)
  unsigned* abort_word;  // COH: bounded spins
  int* range_flag;       // COH: MMF_FLAG_GAVE_UP = "a reader gave up" (engine.run_persistent), or null
  unsigned long long* stamps;  // COH diagnostic: [4] cycle stamps of thread 0, or null
  int spin_sleep;        // COH: s_sleep between polls (0: busy polling)
  float ess_floor;       // ADAPT: fl32(ess_threshold * M); the trajectory resamples iff !(ess >= ess_floor)
  int32_t* resampled;    // ADAPT: 1 (resampled) / 0 (kept) of this trajectory, or null
  int32_t* rank;         // RUNS: (M_out) index of the run every output slot belongs to
  int32_t* run_anc;      // RUNS: (M_out + 1) ancestor of every run
  int32_t* run_start;    // RUNS: (M_out + 1) first output slot of every run; run_start[n_runs] = M_out
  int32_t* n_runs;       // RUNS: number of runs = distinct ancestors of this trajectory
};

// returns false (workgroup-uniform) when a COH reader gave up waiting for its granules
// ADAPT: ESS-triggered resampling (include/mmf.h, K1; M_out == M): the decision follows pass 2's reductions, and a KEPT
// trajectory leaves before the announcements, the prefix maximum and the gather -- it writes mode 0's log-weights, its rows
// as they came and the identity ancestors.  Sum e^2 is the record's own (REC) or, without a record, the same chain alone.
// RUNS (launch path, plain resampling; not COH, not ADAPT, not STAGE): the RUN TABLE instead of the gathered particles.
// The ancestor sequence is non-decreasing, so the copies of an ancestor fill consecutive output slots -- a run; slot 0
// starts one, slot k > 0 does iff marks[k] != 0 (only particle 0 announces the value 0, and only at slot 0).  One more
// integer block scan (an inclusive count of the run starts, the prefix maximum's wave scan + carry structure) numbers the
// runs; per slot its run's index, per run its ancestor and first slot, per trajectory the number of runs.  No state row
// is gathered or stored (`so` is not touched): the next dynamics launch reads the ancestors' rows from `xs` itself
// (particle_net.hip, RUNS).  Estimates, the belief record, `io`, `lo` and every float reduction are untouched.
template <int D, bool STAGE, bool COH, bool DET, bool REC = false, bool ADAPT = false, bool RUNS = false>
__device__ __forceinline__ bool resample_systematic_trajectory(unsigned char* smem, const K1Trajectory& a, int M, int M_out,
                                                               float lw_uniform, float log_uniform) {
  // (the host's byte count of these sections is mmf::k1_systematic_lds above: the two must agree)
  const size_t slots_sz = (static_cast<size_t>(M) * 8 + 15) & ~static_cast<size_t>(15);
  unsigned long long* cdf = reinterpret_cast<unsigned long long*>(smem);  // first the fp32 x_i, then the u64 CDF
  K1Scratch& sc = *reinterpret_cast<K1Scratch*>(smem + slots_sz);
  const size_t sc_sz = (sizeof(K1Scratch) + 15) & ~static_cast<size_t>(15);
  unsigned* marks = reinterpret_cast<unsigned*>(smem + slots_sz + sc_sz);                       // [M_out + 4]
  const size_t marks_sz = ((static_cast<size_t>(M_out) + 4) * 4 + 15) & ~static_cast<size_t>(15);
  float* xs_lds = reinterpret_cast<float*>(smem + slots_sz + sc_sz + marks_sz);                 // STAGE: [M][D]
  const size_t xs_sz = STAGE ? (static_cast<size_t>(M) * D * sizeof(float) + 15) & ~static_cast<size_t>(15) : 0;
  K1BeliefScratch& bsc = *reinterpret_cast<K1BeliefScratch*>(smem + slots_sz + sc_sz + marks_sz + xs_sz);  // REC

  const int tid = threadIdx.x;
  const int lane = tid & (MMF_WAVE - 1), wave = tid >> 6;
  const int chunk = blockDim.x * 4;
  // waves that own particles (thread t owns 4t .. 4t+3 of a chunk): the launch path sizes its workgroup to exactly
  // these; a larger workgroup's surplus waves hold the neutral element of every reduction and are simply not read
  const int nwaves_owning = (((M < chunk ? M : chunk) + 3) / 4 + MMF_WAVE - 1) / MMF_WAVE;
  const int nwaves = nwaves_owning < static_cast<int>(blockDim.x >> 6) ? nwaves_owning : static_cast<int>(blockDim.x >> 6);
  // The float sums of the estimate are defined by the LAUNCH path's partition: a workgroup of ref_block = min(kK1Block,
  // M / 4 rounded up to a wave) threads, thread v owning particles 4v .. 4v+3 -- per-thread sums, a butterfly per wave of 64
  // threads, the waves added in order.  A SMALLER workgroup (the persistent loop's 512 threads at M <= 4 kK1Block = 4096)
  // reproduces it: its chunk c stands for threads c blockDim .. (c + 1) blockDim - 1 of that partition, so every chunk
  // keeps its own per-thread sums and reduces them into the rows of the waves it stands for.  (Integer sums, maxima and
  // the prefix maxima of the marks do not depend on the partition.)
  const int ref_block_raw = ((M + 3) / 4 + MMF_WAVE - 1) / MMF_WAVE * MMF_WAVE;
  const int ref_block = ref_block_raw < kK1Block ? ref_block_raw : kK1Block;
  const bool virt = static_cast<int>(blockDim.x) < ref_block;  // workgroup-uniform; needs M <= 4 ref_block (callers check)
  const int nwaves_red = virt ? ref_block / MMF_WAVE : nwaves;
  const int waves_here = static_cast<int>(blockDim.x >> 6);
  const float* ll = a.ll[0];
  const float* lw = a.lw;
  const float* xs = a.xs;
  const bool vec = !COH && (M & 3) == 0;
  // ADAPT, COH: the log-weights travel from step to step through global memory, written and read back by THIS workgroup
  // only -- agent-scope relaxed atomics (through L2, as every other re-read of the launch), ordered by the barriers between
  auto lw_at = [&](int i) -> float {
    if constexpr (COH && ADAPT) return ld_coherent(lw + i);
    else return lw[i];
  };
  auto state_at = [&](size_t e) -> float {
    if constexpr (COH) {
      // every granule carries its own tag, and the gather CHECKS it: that the row belongs to this step follows from
      // the value read, not from the order in which relaxed loads of different addresses happen to be served
      // (the log-likelihoods being present implies it causally -- each measurement tile waited for its rows -- but the
      // memory model gives a relaxed load of another address no such promise)
      const Granule* p = reinterpret_cast<const Granule*>(xs) + e;
      Granule g = ld_granule(p);
      unsigned spins = 0;
      while (granule_tag(g) != a.in_tag && spins < kGranuleSpinLimit) {
        if (a.spin_sleep) __builtin_amdgcn_s_sleep(1);
        g = ld_granule(p);
        ++spins;
      }
      if (granule_tag(g) != a.in_tag) {
        // timed out: the value read is NOT this step's row.  Report it the way the other spins do -- the abort word stops
        // the other roles, MMF_FLAG_GAVE_UP in the status word makes the host discard this loop and re-run it as launches
        __hip_atomic_store(a.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a.range_flag != nullptr) atomicOr(a.range_flag, MMF_FLAG_GAVE_UP);
      }
      return granule_value(g);
    } else {
      return xs[e];
    }
  };
  // first chunk's states in flight before anything waits; marks cleared (ordered by pass 1's barriers)
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
    } else if constexpr (COH) {
      // the propagated rows arrive BEFORE the log-likelihoods (the measurement networks sit in between): an owning
      // thread polls its own rows' granules now, so their L2 round trip lies under the wait for the log-likelihoods
      // instead of behind it.  (A reader that gives up here is caught by the log-likelihood spin's abort test.)
#pragma unroll
      for (int k = 0; k < 4 * D; ++k) st0[k] = 0.f;
      if (i0 < M) {
        unsigned spins = 0;
        for (;;) {
          bool ok = true;
#pragma unroll
          for (int k = 0; k < 4 * D; ++k)
            if (i0 * D + k < M * D) {
              const Granule g = ld_granule(reinterpret_cast<const Granule*>(xs) + static_cast<size_t>(i0) * D + k);
              ok &= granule_tag(g) == a.in_tag;
              st0[k] = granule_value(g);
            }
          if (ok) break;
          if (a.spin_sleep) __builtin_amdgcn_s_sleep(1);
          if ((++spins & 63u) == 0 && (spins > kGranuleSpinLimit || __hip_atomic_load(a.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) break;
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4 * D; ++k) st0[k] = (i0 * D + k < M * D) ? state_at(static_cast<size_t>(i0) * D + k) : 0.f;
    }
  }
  K1_STAMP(0);
  if constexpr (COH) {
    // x_i = logw_i + logaddexp_k(loglik_k,i) by ONE thread per particle (the launch path's measurement epilogues did
    // the combine on N*M lanes; four particles per thread here would put 4 x (2 exp + 1 log) on the chain), spinning
    // on the particle's own granules until every modality has delivered this step's value.  All modalities present
    // implies the particle's propagated state is complete too (each measurement tile waited for it).
    int gave_up = 0;
    for (int i = tid; i < M; i += blockDim.x) {
      Granule gk[MMF_LOOP_MAX_MEAS];
      unsigned spins = 0;
      for (;;) {
        bool ok = true;
#pragma unroll  // constant indices: the arrays stay in registers (a run-time index sends them to scratch)
        for (int k = 0; k < MMF_LOOP_MAX_MEAS; ++k)
          if (k < a.n_ll) {
            gk[k] = ld_granule(reinterpret_cast<const Granule*>(a.ll[k]) + i);
            ok &= granule_tag(gk[k]) == a.in_tag;
          }
        if (ok) break;
        if (a.spin_sleep) __builtin_amdgcn_s_sleep(1);
        if ((++spins & 63u) == 0 && (spins > kGranuleSpinLimit || __hip_atomic_load(a.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
          gave_up = 1;
          break;
        }
      }
      float v = granule_value(gk[0]);
#pragma unroll
      for (int k = 1; k < MMF_LOOP_MAX_MEAS; ++k)
        if (k < a.n_ll) v = combine_loglik<DET>(v, granule_value(gk[k]));
      reinterpret_cast<float*>(cdf + i)[0] = (lw ? lw_at(i) : lw_uniform) + v;
    }
    if (gave_up) sc.gave_up = 1u;
    __syncthreads();
    if (a.stamps && tid == 0) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); a.stamps[1] = t_; }
    if (sc.gave_up != 0u) {  // workgroup-uniform
      if (tid == 0) __hip_atomic_store(a.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return false;
    }
  }

  for (int k = tid; k < M_out + 4; k += blockDim.x) marks[k] = 0u;

  // ---- pass 1: x_i = logw_i + loglik_i -> LDS, row max
  float mx = -INFINITY;
  int mi = 0x7fffffff;  // REC: the first of this thread's particles that holds its maximum
  for (int base = 0; base < M; base += chunk) {
    const int i0 = base + tid * 4;
    float v[4];
    if (vec && i0 + 3 < M) {
      const float4 a4 = *reinterpret_cast<const float4*>(ll + i0);
      const float4 b = lw ? *reinterpret_cast<const float4*>(lw + i0) : make_float4(lw_uniform, lw_uniform, lw_uniform, lw_uniform);
      v[0] = b.x + a4.x; v[1] = b.y + a4.y; v[2] = b.z + a4.z; v[3] = b.w + a4.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if constexpr (COH) v[j] = (i0 + j < M) ? reinterpret_cast<const float*>(cdf + i0 + j)[0] : -INFINITY;  // formed above
        else v[j] = (i0 + j < M) ? (lw ? lw[i0 + j] : lw_uniform) + ll[i0 + j] : -INFINITY;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i0 + j < M) {
        reinterpret_cast<float*>(cdf + i0 + j)[0] = v[j];
        if constexpr (REC) { if (v[j] > mx || mi == 0x7fffffff) mi = i0 + j; }
        mx = fmaxf(mx, v[j]);
      }
  }
  const float mx_thread = mx;
  mx = wave_max(mx);
  if (lane == 0) sc.red[wave][0] = mx;
  __syncthreads();
  mx = sc.red[0][0];
  for (int w = 1; w < nwaves; ++w) mx = fmaxf(mx, sc.red[w][0]);
  if constexpr (REC) {  // the pivot: the smallest index holding the row maximum (indices < 2^24 are exact floats)
    const float cand = wave_max((mi != 0x7fffffff && mx_thread == mx) ? -static_cast<float>(mi) : -INFINITY);
    if (lane == 0) bsc.piv_wave[wave] = cand;
  }
  __syncthreads();
  float piv[D];
  if constexpr (REC) {
    float best = bsc.piv_wave[0];
    for (int w = 1; w < nwaves; ++w) best = fmaxf(best, bsc.piv_wave[w]);
    const int p = best > -INFINITY ? static_cast<int>(-best) : 0;  // (every value NaN: the filter is lost either way)
#pragma unroll
    for (int c = 0; c < D; ++c) piv[c] = state_at(static_cast<size_t>(p) * D + c);
  }
  K1_STAMP(1);

  // ---- pass 2: e_i, fixed-point q_i, float sums of the estimate, integer CDF (kept in LDS for multi-chunk rows)
  float S = 0.f, acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) acc[c] = 0.f;
  K1Belief<D> bel;  // REC
  if constexpr (REC) bel.reset();
  float w2 = 0.f;   // ADAPT without REC: bel.s[0] alone
  unsigned long long carry = 0;
  unsigned long long own[4] = {0, 0, 0, 0};  // CDF of this thread's particles in the LAST chunk
  unsigned long long own_prev = 0;           // ... and of the particle just before them
  for (int base = 0; base < M; base += chunk) {
    const int i0 = base + tid * 4;
    float e[4];
    unsigned long long q[4], tsum = 0;
    float st[4 * D];
    if (virt) {  // this chunk's threads are other threads of the reference partition: their sums start at zero
      S = 0.f;
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = 0.f;
      if constexpr (REC) bel.reset();
      if constexpr (ADAPT && !REC) w2 = 0.f;
    }
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
      for (int k = 0; k < 4 * D; ++k) st[k] = (i0 * D + k < M * D) ? state_at(static_cast<size_t>(i0) * D + k) : 0.f;
    }
    if (STAGE) {
#pragma unroll
      for (int k = 0; k < 4 * D; ++k)
        if (i0 * D + k < M * D) xs_lds[i0 * D + k] = st[k];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool ok = i0 + j < M;
      e[j] = ok ? detexp(reinterpret_cast<const float*>(cdf + i0 + j)[0] - mx) : 0.f;
      q[j] = static_cast<unsigned long long>(floorf(e[j] * 16777216.0f));
      tsum += q[j];
      S += e[j];
#pragma unroll
      for (int c = 0; c < D; ++c) acc[c] = __builtin_fmaf(e[j], st[j * D + c], acc[c]);  // explicit: oracle/strict restates this chain
      if constexpr (REC) {
        const float xv = ok ? reinterpret_cast<const float*>(cdf + i0 + j)[0] : -INFINITY;
        bel.add(xv == -INFINITY ? 0.f : e[j], st + j * D, piv);
      } else if constexpr (ADAPT) {
        const float xv = ok ? reinterpret_cast<const float*>(cdf + i0 + j)[0] : -INFINITY;
        const float ev = xv == -INFINITY ? 0.f : e[j];
        w2 = __builtin_fmaf(ev, ev, w2);
      }
    }
    const unsigned long long incl = wave_inclusive_scan(tsum, lane);
    if (lane == MMF_WAVE - 1) sc.wave_tot[wave] = incl;
    const bool last_chunk = base + chunk >= M;
    if (last_chunk || virt) {  // the float sums of the estimate ride on the last chunk's barriers (virt: on every chunk's)
      const float Sw = wave_sum(S);
      float aw[D];
#pragma unroll
      for (int c = 0; c < D; ++c) aw[c] = wave_sum(acc[c]);
      const int row = virt ? wave + (base / chunk) * waves_here : wave;  // the reference partition's wave
      if (lane == 0 && row < kK1MaxWaves) {
        sc.red[row][0] = Sw;
#pragma unroll
        for (int c = 0; c < D; ++c) sc.red[row][1 + c] = aw[c];
      }
      if constexpr (REC) {  // the record's sums: same partition, same order of the waves
#pragma unroll
        for (int k = 0; k < K1Belief<D>::kSums; ++k) {
          const float bw = wave_sum(bel.s[k]);
          if (lane == 0 && row < kK1MaxWaves) bsc.red[row][k] = bw;
        }
      } else if constexpr (ADAPT) {
        const float bw = wave_sum(w2);
        if (lane == 0 && row < kK1MaxWaves) bsc.red[row][0] = bw;
      }
    }
    __syncthreads();
    if (last_chunk && tid <= D) {
      float t = 0.f;
      for (int w = 0; w < nwaves_red; ++w) t += sc.red[w][tid];
      sc.bcast[tid] = t;
    }
    if constexpr (REC) {
      if (last_chunk && tid < K1Belief<D>::kSums) {
        float t = 0.f;
        for (int w = 0; w < nwaves_red; ++w) t += bsc.red[w][tid];
        bsc.tot[tid] = t;
      }
    } else if constexpr (ADAPT) {
      if (last_chunk && tid == 0) {
        float t = 0.f;
        for (int w = 0; w < nwaves_red; ++w) t += bsc.red[w][0];
        bsc.tot[0] = t;
      }
    }
    unsigned long long before = carry, total = 0;
    for (int w = 0; w < nwaves; ++w) {
      const unsigned long long t = sc.wave_tot[w];
      if (w < wave) before += t;
      total += t;
    }
    unsigned long long run = before + incl - tsum;
    own_prev = run;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      run += q[j];
      own[j] = run;
      if (!last_chunk && i0 + j < M) cdf[i0 + j] = run;  // earlier chunks wait in LDS for Q
    }
    carry += total;
    __syncthreads();
  }
  K1_STAMP(2);
  const unsigned long long Q = carry;  // every thread has added every chunk's total
  S = sc.bcast[0];
  if (tid < D) {
    const float est = sc.bcast[1 + tid] / S;
    a.estimate[tid] = est;
  }
  if constexpr (REC) k1_belief_store<D>(bsc.tot, S, mx, a.cov, a.ess, a.log_evidence, tid);

  float* so = a.so;
  float* lo = a.lo;
  int32_t* io = a.io;
  if constexpr (ADAPT) {
    // S and sum e^2 are the broadcast totals (LDS), so every lane of every wave takes the same side
    const bool keep = k1_ess(S, bsc.tot[0]) >= a.ess_floor;  // a NaN resamples, a tie keeps
    if (tid == 0 && a.resampled != nullptr) *a.resampled = keep ? 0 : 1;
    if (keep) {
      // mode 0's outputs: logw = (x - max) - log S, the rows as they came, ancestors 0 .. M - 1.  The slots of every chunk
      // but the last hold the CDF by now: their x_i are formed again from the inputs (the same single addition)
      const float logS = logf(S);
      const int last_base = ((M - 1) / chunk) * chunk;
      for (int i = tid; i < M; i += blockDim.x) {
        float x;
        if (i >= last_base) {
          x = reinterpret_cast<const float*>(cdf + i)[0];
        } else if constexpr (COH) {
          float v = granule_value(ld_granule(reinterpret_cast<const Granule*>(a.ll[0]) + i));  // (tags checked before pass 1)
#pragma unroll
          for (int k = 1; k < MMF_LOOP_MAX_MEAS; ++k)
            if (k < a.n_ll) v = combine_loglik<DET>(v, granule_value(ld_granule(reinterpret_cast<const Granule*>(a.ll[k]) + i)));
          x = (lw ? lw_at(i) : lw_uniform) + v;
        } else {
          x = (lw ? lw[i] : lw_uniform) + ll[i];
        }
        const float w = (x - mx) - logS;
        if constexpr (COH) st_coherent(lo + i, w);
        else lo[i] = w;
#pragma unroll
        for (int c = 0; c < D; ++c) {
          const float v = STAGE ? xs_lds[i * D + c] : state_at(static_cast<size_t>(i) * D + c);
          if (COH && a.so_tag != 0) st_granule(reinterpret_cast<Granule*>(so) + static_cast<size_t>(i) * D + c, v, a.so_tag);
          else so[static_cast<size_t>(i) * D + c] = v;
        }
        if (io) io[i] = i;
      }
      K1_STAMP(3);
      return true;
    }
  }

  // ---- offspring boundaries: the first particle of every run of equal k_end announces itself,
  // marks[k_end(i - 1)] = i  when  k_end(i - 1) < k_end(i)  -- one writer per entry, plain LDS stores
  {
    const unsigned long long U = static_cast<unsigned long long>(floorf(a.u * 16777216.0f));
    const unsigned long long R = (U * Q) >> kK1FixBits;
    const float rq = 1.0f / static_cast<float>(Q);
    const unsigned long long Mo = static_cast<unsigned long long>(M_out);
    // k_end(c) = #{k >= 0 : k Q + R < c M_out} = ceil((c M_out - R) / Q), at most M_out <= 2^15: a float32
    // quotient is within 1 of the floor (relative error 2^-22 on a value below 2^15); ONE u64 multiply corrects it
    auto k_end = [&](unsigned long long cdf_i) -> unsigned {
      const unsigned long long c = cdf_i * Mo;
      if (c <= R) return 0u;
      const unsigned long long num = c - R;
      const float numf = static_cast<float>(static_cast<unsigned>(num >> 32)) * 4294967296.0f + static_cast<float>(static_cast<unsigned>(num));
      long long fl = static_cast<long long>(numf * rq);
      long long rem = static_cast<long long>(num) - fl * static_cast<long long>(Q);
      if (rem < 0) { --fl; rem += static_cast<long long>(Q); }
      if (rem >= static_cast<long long>(Q)) { ++fl; rem -= static_cast<long long>(Q); }
      const unsigned long long ke = static_cast<unsigned long long>(fl) + (rem > 0 ? 1u : 0u);
      return static_cast<unsigned>(ke < Mo ? ke : Mo);
    };
    for (int base = 0; base < M; base += chunk) {
      const int i0 = base + tid * 4;
      if (i0 >= M) continue;
      const bool last_chunk = base + chunk >= M;
      unsigned long long c[5];
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j + 1] = last_chunk ? own[j] : cdf[i0 + j < M ? i0 + j : M - 1];
      // CDF just before this thread's first particle: its own running sum before q[0] (last chunk), LDS otherwise
      c[0] = last_chunk ? own_prev : (i0 == 0 ? 0ull : cdf[i0 - 1]);
      unsigned ke[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) ke[j] = k_end(c[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j < M && ke[j] < ke[j + 1] && ke[j] < static_cast<unsigned>(M_out)) marks[ke[j]] = static_cast<unsigned>(i0 + j);
    }
  }
  __syncthreads();

  if constexpr (COH) {
    if (a.stamps && tid == 0) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); a.stamps[2] = t_; }
  }
  // ---- ancestor(k) = the latest announcement at or before k = inclusive prefix MAX of marks; gather; store
  static_assert(!RUNS || (!COH && !ADAPT && !STAGE), "the run table belongs to the launch path's plain resampling");
  const bool vec_out = !COH && (M_out & 3) == 0;
  unsigned carry2 = 0;
  unsigned runs_before = 0;  // RUNS: run starts in the chunks before this one
  for (int base = 0; base < M_out; base += chunk) {
    const int k0 = base + tid * 4;
    unsigned m[4] = {0u, 0u, 0u, 0u};
    if (k0 < M_out) {
      const uint4 t = *reinterpret_cast<const uint4*>(marks + k0);  // marks is padded by 4 zero entries
      m[0] = t.x; m[1] = t.y; m[2] = t.z; m[3] = t.w;
    }
    unsigned starts[4] = {0u, 0u, 0u, 0u}, starts_incl = 0;  // RUNS
    if constexpr (RUNS) {
#pragma unroll
      for (int j = 0; j < 4; ++j) starts[j] = (k0 + j < M_out && (k0 + j == 0 || m[j] != 0u)) ? 1u : 0u;
      starts_incl = wave_inclusive_scan_u32(starts[0] + starts[1] + starts[2] + starts[3]);
      if (lane == MMF_WAVE - 1) sc.wave_tot[wave] = starts_incl;  // (pass 2 is done with these rows)
    }
    m[1] = max(m[1], m[0]); m[2] = max(m[2], m[1]); m[3] = max(m[3], m[2]);
    const unsigned incl = wave_inclusive_scan_max_u32(m[3]);
    if (lane == MMF_WAVE - 1) sc.wave_cnt[wave] = incl;
    __syncthreads();
    unsigned before = carry2, total = carry2;
    for (int w = 0; w < nwaves; ++w) {
      const unsigned t = sc.wave_cnt[w];
      if (w < wave) before = max(before, t);
      total = max(total, t);
    }
    carry2 = total;
    // everything announced before this thread's first output: previous waves / chunks and the lanes below
    const unsigned below = max(before, dpp_u32<kDppWaveShr1>(0u, incl));
    int idx[4];
    if constexpr (RUNS) {
      unsigned rb = runs_before, rt = 0;
      for (int w = 0; w < nwaves; ++w) {
        const unsigned t = static_cast<unsigned>(sc.wave_tot[w]);
        if (w < wave) rb += t;
        rt += t;
      }
      runs_before += rt;
      // run starts at or before slot k0 + j, minus one: the run's index
      int rk[4];
      unsigned cnt = rb + starts_incl - (starts[0] + starts[1] + starts[2] + starts[3]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        idx[j] = static_cast<int>(max(below, m[j]));
        cnt += starts[j];
        rk[j] = static_cast<int>(cnt) - 1;
        if (starts[j]) {  // this thread owns the run's first slot
          a.run_anc[rk[j]] = idx[j];
          a.run_start[rk[j]] = k0 + j;
        }
      }
      if (vec_out && k0 + 3 < M_out) {
        *reinterpret_cast<int4*>(a.rank + k0) = make_int4(rk[0], rk[1], rk[2], rk[3]);
        if (lo) *reinterpret_cast<float4*>(lo + k0) = make_float4(log_uniform, log_uniform, log_uniform, log_uniform);
        if (io) *reinterpret_cast<int4*>(io + k0) = make_int4(idx[0], idx[1], idx[2], idx[3]);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + j;
          if (k < M_out) {
            a.rank[k] = rk[j];
            if (lo) lo[k] = log_uniform;
            if (io) io[k] = idx[j];
          }
        }
      }
      if (base + chunk < M_out) __syncthreads();  // wave_cnt / wave_tot are reused by the next chunk
      continue;
    }
    float g[4 * D];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      idx[j] = static_cast<int>(max(below, m[j]));
      const int src = (k0 + j < M_out) ? idx[j] : 0;
#pragma unroll
      for (int c = 0; c < D; ++c) g[j * D + c] = STAGE ? xs_lds[src * D + c] : state_at(static_cast<size_t>(src) * D + c);
    }
    if (vec_out && k0 + 3 < M_out) {
      float4* p = reinterpret_cast<float4*>(so + static_cast<size_t>(k0) * D);
#pragma unroll
      for (int k = 0; k < D; ++k) p[k] = make_float4(g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]);
      if (lo) *reinterpret_cast<float4*>(lo + k0) = make_float4(log_uniform, log_uniform, log_uniform, log_uniform);
      if (io) *reinterpret_cast<int4*>(io + k0) = make_int4(idx[0], idx[1], idx[2], idx[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + j;
        if (k < M_out) {
#pragma unroll
          for (int c = 0; c < D; ++c) {
            if (COH && a.so_tag != 0) st_granule(reinterpret_cast<Granule*>(so) + static_cast<size_t>(k) * D + c, g[j * D + c], a.so_tag);
            else so[static_cast<size_t>(k) * D + c] = g[j * D + c];
          }
          if (lo) {
            if constexpr (COH && ADAPT) st_coherent(lo + k, log_uniform);
            else lo[k] = log_uniform;
          }
          if (io) io[k] = idx[j];
        }
      }
    }
    if (base + chunk < M_out) __syncthreads();  // wave_cnt is reused by the next chunk
  }
  if constexpr (RUNS) {
    if (tid == 0) {  // every thread has added every chunk's count
      *a.n_runs = static_cast<int>(runs_before);
      a.run_start[runs_before] = M_out;
    }
  }
  K1_STAMP(3);
  return true;
}

}  // namespace mmf
