// The particle filter's step loop for SMALL problems as ONE persistent launch per forward_loop.  Included at the
// end of particle_net.hip (shares its tile machinery) and pf_resample_systematic.inc (K1's body).
//
// Why: at the sizes the reference itself runs -- 32 trajectories x 300 particles, door_models/pf.py:24-27,
// eval_helpers.py:125-142 -- a filter step is four launches of 6-15 us each (profiles/r03/
// reference_sizes_kernel_stats.csv: dynamics 15.1, measurement 2 x 11.1, K1 5.9 us), and most of every launch is
// fixed cost: 117-150 KB of weights staged into LDS per workgroup, the first dependent loads, the drain.  Here the
// launch lives for all T steps and its workgroups have ROLES: G workgroups keep the dynamics network's weights in
// LDS, G more per measurement network, GK run K1 (one trajectory at a time each).  A step is a chain of hand-offs
// through L2 -- K1(t-1) -> dynamics(t) -> measurement_k(t) -> K1(t) -- per PARTICLE ROW (the recursion couples
// nothing else before K1, and K1 only a trajectory), so trajectories drift apart freely and no grid-wide barrier
// exists.
//
// Same arithmetic as the launch path, bit for bit: a tile is 32 particles of one trajectory through the network pieces
// of particle_net_tiles.h that particle_net_kernel<D, NRES, KIND, 1, PREC, 2, false> (the small-problem variant of the
// launch path) is built from -- a particle's column does not depend on what else sits in its tile --, each measurement network writes
// its own log-likelihood and K1 folds them with the epilogue's own logaddexp (combine_loglik), and K1 is
// mmf::resample_systematic_trajectory, whose result does not depend on the workgroup size
// (tests/test_gpu_models.py::test_persistent_step_loop_equals_loop_of_launches).
//
// Hand-offs (MI355X_MICROARCH.md, inter-workgroup visibility; cdna_hip_programming.md Guideline 16, form R2): every
// value one workgroup writes and another reads inside the launch -- a particle's state components, its
// log-likelihoods -- is an 8-byte GRANULE {fp32 value, u32 tag = step + 1} stored and loaded by ONE agent-scope
// relaxed atomic (global_store / global_load_dwordx2 ... sc1: written through to L2 / served by L2; no per-CU L1
// line can be stale, an aligned 8-byte access is not torn).  The data IS the flag: a reader polls its own
// granules until their tags are the step's -- no separate flag word, no fence, no store drain on the chain (the
// first version of this kernel signalled through per-tile / per-trajectory counters behind s_waitcnt vmcnt(0):
// 4.2 us per hop, 12.5 of a 46 us step at 32 x 300).  WAR hazards are excluded by the chain itself: a row is
// rewritten only by the stage whose input depends on every reader of the old value having finished.  Every spin
// is bounded: a reader that waits too long (or sees the abort word) sets the abort word and leaves, every other
// wave follows at its next poll, and the host re-runs the loop as launches (MMF_FLAG_GAVE_UP in the status word: engine.run_persistent).
// Correctness does not depend on placement or dispatch order; progress needs all workgroups resident, which the
// grid (<= 240 workgroups of one per CU, LDS-limited) guarantees on an otherwise idle 256-CU device.

#include "pf_resample_systematic.inc"

namespace {

using mmf::Granule;

constexpr int kPersistThreads = 512;
constexpr int kPersistWaves = kPersistThreads / MMF_WAVE;
constexpr int kPersistMaxRounds = 5;   // rounds of 32-particle tiles per wave and step up to which ONE launch beats the launches

struct PersistArgs {
  int T, N, M, n_meas, logw_stride;
  int G, GK, tpt;                      // workgroups per measurement network, K1 workgroups, tiles per trajectory
  int Gd;                              // workgroups of the dynamics network (the longest stage gets a SIMD per tile first)
  const float* dyn_packed;
  const float* dyn_bias;               // (T*N, 64)
  const float* meas_packed[MMF_LOOP_MAX_MEAS];
  const float* meas_bias[MMF_LOOP_MAX_MEAS];
  const float* meas_logw[MMF_LOOP_MAX_MEAS];
  const float* noise;                  // (T, N, M, D) or null (noise_mode 2)
  const float* scale_tril;
  const float* uniforms;               // (T, N)
  float* belief;                       // (N, M, D) plain: the call's input belief (step 0) and its output (last step)
  Granule* ga;                         // (N, M, D) granules: beliefs in between (written by K1, read by the dynamics)
  Granule* gb;                         // (N, M, D) granules: propagated particles (dynamics -> measurement, K1)
  Granule* gll;                        // (n_meas, N, M) granules: each modality's own log-likelihood
  const float* logw_in0;               // (N, M) log-weights on entry (read by step 0 only)
  float* logw_out_last;                // (N, M) written by the last step only
  float* estimates;                    // (T, N, D)
  float* cov_steps;                    // REC: (T, N, D, D) / (T, N) / (T, N) belief records, each or null: written by the K1
  float* ess_steps;                    // role straight to global memory -- nobody in the launch reads them back
  float* log_evidence_steps;
  int* range_flag;
  unsigned* abort_word;
  unsigned long long noise_seed;
  unsigned noise_step0, noise_traj0;
  int noise_mode;
  float lw_uniform;
  unsigned long long* stamps;          // MMF_PERSIST_STAMPS=<step> (diagnostic): [block][wave][4] cycle stamps of one step
  int stamp_step;
  int spin_sleep;                      // s_sleep between polls
  // ADAPT (ESS-triggered resampling): every step reads and writes the log-weights, ping-ponging as the loop of launches does
  // -- step t reads logw[t & 1] and writes the other; a trajectory's rows are written and read back by ITS K1 workgroup only
  float* logw[2];                      // {logw_a, logw_b}, (N, M) each
  float ess_floor;                     // fl32(ess_threshold * M)
  int32_t* resampled_steps;            // (T, N) 1 / 0, or null
};

__device__ __forceinline__ unsigned long long persist_clock() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}

struct SmallTile {
  const float* in_plain;    // (N*M, D) plain rows (dynamics, step 0), or null
  const Granule* in_g;      // (N*M, D) granules carrying in_tag
  unsigned in_tag, out_tag;
  const float* traj_bias;   // this step's (N, 64)
  const float* mod_logw;    // this step's first element of the modality column, or null
  const float* noise;       // this step's (N*M, D) or null
  const float* scale_tril;
  Granule* out_g;           // dynamics: (N*M, D) propagated rows; measurement: (N*M) log-likelihoods
  int logw_stride;
  int* range_flag;
  unsigned* abort_word;
  unsigned long long noise_seed;
  unsigned noise_step, noise_traj0;
  int noise_mode;
  unsigned long long* stamps;  // diagnostic: this wave's [4] stamps, or null
  int spin_sleep;
};

// 32 particles (rows row0 .. row0 + nvalid - 1 of trajectory `traj`, particle indices m0 ..) through one network.
// Built from particle_net_tiles.h's pieces, as particle_net_kernel's CT = 1 variant is: first_layer, seed_nonfinite,
// report_range, head, dynamics_update; the 64 x 64 layers are net_unpipelined (f32) or, for f16x3, rowpipe_net_f16<1>
// -- another schedule of the same per-accumulator MFMA chains, hence the same bits.  Its own: the inputs arrive as
// granules behind a bounded spin (mmf::spin_stop / give_up), the per-trajectory row, the noise and scale_tril are
// requested at the top of the tile, the step's start state is taken from the first layer's operands, the outputs leave
// as granules.
// Returns false when the wave gave up waiting for its input granules.
template <int D, int NRES, int KIND, int PREC>
__device__ __forceinline__ bool small_tile(const float* __restrict__ lds, const SmallTile& a, int traj, int row0, int m0,
                                           int nvalid, int lane, float neg_one) {
  constexpr bool F16 = PREC == MMF_PREC_F16X3;
  constexpr int NOUT = (KIND == kMeasure) ? 1 : D + 1;
  constexpr int KS0 = (D + 2) / 2;
  const int j = lane & 31, h = lane >> 5;
  const int col = j < nvalid ? j : nvalid - 1;
  const size_t row = static_cast<size_t>(row0) + col;
  const bool active = j < nvalid && h == 0;

  // ---- everything that does not depend on another workgroup is requested first: the per-trajectory term of the
  // join layer (32 floats per lane) and the process noise would otherwise be dependent loads in the middle / at the
  // end of the chain (~1-2 k cycles each at this occupancy)
  f32x4 tbv[2][4];  // mirrors load_join_row / join_init (through JoinRow the REC f16x3 d = 2 kernel spills two more VGPRs)
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const float* tb = a.traj_bias + static_cast<size_t>(traj) * kUnits + 32 * t + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) tbv[t][g] = *reinterpret_cast<const f32x4*>(tb + 8 * g);
  }
  float eps[D];
#pragma unroll
  for (int i = 0; i < D; ++i) eps[i] = 0.f;
  float logw_mod = 0.f;
  float tril[D * D];
#pragma unroll
  for (int i = 0; i < D * D; ++i) tril[i] = 0.f;
  if (KIND == kDynamics) {
    if (a.noise != nullptr || a.noise_mode == 2) {
#pragma unroll
      for (int i = 0; i < D * D; ++i) tril[i] = a.scale_tril[i];
    }
    if (active && a.noise_mode != 2 && a.noise) {
#pragma unroll
      for (int i = 0; i < D; ++i) eps[i] = a.noise[row * D + i];
    }
  } else if (a.mod_logw) {
    logw_mod = a.mod_logw[static_cast<size_t>(traj) * a.logw_stride];
  }

  // ---- first-layer inputs: lane (j, h) feeds components 2s + h of its column's state
  float b0[KS0][1];
  if (a.in_plain != nullptr) {
#pragma unroll
    for (int s = 0; s < KS0; ++s) {
      const int comp = 2 * s + h;
      b0[s][0] = comp < D ? a.in_plain[row * D + comp] : (comp == D ? 1.f : 0.f);
    }
  } else {
    unsigned spins = 0;
    for (;;) {
      bool ok = true;
#pragma unroll
      for (int s = 0; s < KS0; ++s) {
        const int comp = 2 * s + h;
        if (comp < D) {
          const Granule g = mmf::ld_granule(a.in_g + row * D + comp);
          ok &= mmf::granule_tag(g) == a.in_tag;
          b0[s][0] = mmf::granule_value(g);
        } else {
          b0[s][0] = comp == D ? 1.f : 0.f;
        }
      }
      if (__all(ok)) break;
      if (a.spin_sleep) __builtin_amdgcn_s_sleep(1);
      if (mmf::spin_stop(a.abort_word, spins, lane)) {  // wave-uniform
        if (lane == 0) mmf::give_up(a.abort_word, a.range_flag);
        return false;
      }
    }
  }
  if (a.stamps && lane == 0) a.stamps[1] = persist_clock();
  Act<1> X, H;
  first_layer<1>(lds, b0, X, lane);
  half2v amax = {0, 0};
  if constexpr (F16) seed_nonfinite<1>(b0, amax);
  auto join = [&](Act<1>& acc) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc.v[t][0][4 * g + e] = tbv[t][g][e];
  };
  if constexpr (F16) {
    SplitAct<1> SP;
    rowpipe_net_f16<1, NRES, KIND>(lds, X, H, SP, join, lane, neg_one, amax);
    report_range(a.range_flag, amax);
  } else {
    net_unpipelined<1, NRES, KIND, PREC>(lds, X, H, join, lane, neg_one, amax, true);
  }
  float out[NOUT][1];
  head<NRES>(lds, H, lane, out);
  const float* bh = lds + off_bhead(NRES);
  if (a.stamps && lane == 0) a.stamps[2] = persist_clock();
  if constexpr (KIND == kMeasure) {
    if (active) {
      float ll = out[0][0] + bh[0];
      if (a.mod_logw) ll += logw_mod;
      mmf::st_granule(a.out_g + row, ll, a.out_tag);  // this modality's OWN log-likelihood: K1 folds the modalities
    }
  } else {
    // the state the step started from: components 2s of this column sit in this lane's b0, components 2s + 1 in the
    // partner lane's (lane ^ 32) -- no second load
    float xo[D], mine[NOUT];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const float other_half = __shfl_xor(b0[i / 2][0], 32);
      xo[i] = (i & 1) ? other_half : b0[i / 2][0];
    }
#pragma unroll
    for (int o = 0; o < NOUT; ++o) mine[o] = out[o][0];
    if (active) {
      float xn[D];
      dynamics_update<D, PREC>(mine, bh, xo, eps, tril, a.noise != nullptr || a.noise_mode == 2, a.noise_mode == 2, a.noise_seed,
                               a.noise_step, a.noise_traj0 + static_cast<unsigned>(traj), static_cast<unsigned>(m0 + j), xn);
#pragma unroll
      for (int i = 0; i < D; ++i) mmf::st_granule(a.out_g + row * D + i, xn[i], a.out_tag);
    }
  }
  return true;
}

// REC: the K1 role also writes every step's belief record (mmf::K1Belief); the other roles are the same code
// ADAPT: the K1 role resamples a trajectory only where its ESS fell below the floor; a kept trajectory publishes its rows to
// the dynamics role through the same tagged granules (an identity gather) and carries its normalised log-weights to its own
// next step -- the same workgroup in program order (n = b - n_net_blocks + k GK), so no hand-off is added
template <int D, int PREC, bool REC = false, bool ADAPT = false>
__global__ __launch_bounds__(kPersistThreads, 2) void pf_persistent_loop_kernel(PersistArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int kNresDyn = 3, kNresMeas = 2;
  const int lane = threadIdx.x & (MMF_WAVE - 1);
  const int wave = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const int n_net_blocks = a.Gd + a.n_meas * a.G;
  const int ntiles = a.N * a.tpt;
  const size_t NM = static_cast<size_t>(a.N) * a.M;

  if (b < n_net_blocks) {
    // ------------------------------------------------------------------ a network role
    const int role = b < a.Gd ? 0 : 1 + (b - a.Gd) / a.G;   // 0: dynamics, 1 + k: measurement network k
    const int g = role == 0 ? b : (b - a.Gd) - (role - 1) * a.G;
    const int Grole = role == 0 ? a.Gd : a.G;
    // (constant indices into the kernel arguments' arrays: a run-time index would copy them to scratch)
    auto pick = [&](const float* const (&v)[MMF_LOOP_MAX_MEAS], int k) -> const float* {
      return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3];
    };
    const float* packed = role == 0 ? a.dyn_packed : pick(a.meas_packed, role - 1);
    const float* my_bias = role == 0 ? a.dyn_bias : pick(a.meas_bias, role - 1);
    const float* my_logw = role == 0 ? nullptr : pick(a.meas_logw, role - 1);
    if (role == 0) mmf::stage_to_lds<blob_floats(kNresDyn) / 4, kPersistThreads>(reinterpret_cast<const float4*>(packed), reinterpret_cast<float4*>(lds), threadIdx.x);
    else mmf::stage_to_lds<blob_floats(kNresMeas) / 4, kPersistThreads>(reinterpret_cast<const float4*>(packed), reinterpret_cast<float4*>(lds), threadIdx.x);
    __syncthreads();
    float neg_one = -1.0f;
    asm volatile("" : "+s"(neg_one));
    for (int t = 0; t < a.T; ++t) {
      SmallTile st{};
      st.scale_tril = a.scale_tril;
      st.range_flag = a.range_flag;
      st.abort_word = a.abort_word;
      st.spin_sleep = a.spin_sleep;
      st.logw_stride = a.logw_stride;
      st.traj_bias = my_bias + static_cast<size_t>(t) * a.N * kUnits;
      st.out_tag = static_cast<unsigned>(t + 1);
      if (role == 0) {
        // the belief after step t - 1: the call's input (plain) at t = 0, K1's granules tagged t afterwards
        st.in_plain = t == 0 ? a.belief : nullptr;
        st.in_g = a.ga;
        st.in_tag = static_cast<unsigned>(t);
        st.out_g = a.gb;
        st.noise = a.noise ? a.noise + static_cast<size_t>(t) * NM * D : nullptr;
        st.noise_seed = a.noise_seed; st.noise_step = a.noise_step0 + static_cast<unsigned>(t);
        st.noise_traj0 = a.noise_traj0; st.noise_mode = a.noise_mode;
      } else {
        st.in_g = a.gb;                      // this step's propagated rows
        st.in_tag = static_cast<unsigned>(t + 1);
        st.out_g = a.gll + static_cast<size_t>(role - 1) * NM;
        st.mod_logw = my_logw ? my_logw + static_cast<size_t>(t) * a.N * a.logw_stride : nullptr;
      }
      const bool stamp = a.stamps != nullptr && t == a.stamp_step;
      unsigned long long* my_stamps = stamp ? a.stamps + (static_cast<size_t>(b) * kPersistWaves + wave) * 6 : nullptr;
      for (int q = g + Grole * wave; q < ntiles; q += Grole * kPersistWaves) {
        const int n = q / a.tpt, jt = q - n * a.tpt;
        const int m0 = 32 * jt;
        const int nvalid = a.M - m0 < 32 ? a.M - m0 : 32;
        const int row0 = n * a.M + m0;
        if (stamp && lane == 0) { my_stamps[0] = persist_clock(); my_stamps[4] = __builtin_amdgcn_s_memrealtime(); }
        st.stamps = my_stamps;
        bool ok;
        if (role == 0) ok = small_tile<D, kNresDyn, kDynamics, PREC>(lds, st, n, row0, m0, nvalid, lane, neg_one);
        else ok = small_tile<D, kNresMeas, kMeasure, PREC>(lds, st, n, row0, m0, nvalid, lane, neg_one);
        if (!ok) return;
        if (stamp && lane == 0) { my_stamps[3] = persist_clock(); my_stamps[5] = __builtin_amdgcn_s_memrealtime(); }
      }
    }
    return;
  }

  // -------------------------------------------------------------------- K1 role: whole trajectories, one at a time
  unsigned char* smem = reinterpret_cast<unsigned char*>(lds);
  {
    const size_t slots_sz = (static_cast<size_t>(a.M) * 8 + 15) & ~static_cast<size_t>(15);
    mmf::K1Scratch& sc = *reinterpret_cast<mmf::K1Scratch*>(smem + slots_sz);
    if (threadIdx.x == 0) sc.gave_up = 0u;
    __syncthreads();
  }
  const float log_uniform = a.lw_uniform;  // M_out == M
  for (int t = 0; t < a.T; ++t) {
    const bool stamp = a.stamps != nullptr && t == a.stamp_step && threadIdx.x == 0;
    unsigned long long* my_stamps = stamp ? a.stamps + static_cast<size_t>(b) * kPersistWaves * 6 : nullptr;
    for (int n = b - n_net_blocks; n < a.N; n += a.GK) {
      if (stamp) my_stamps[0] = persist_clock();
      mmf::K1Trajectory tr{};
#pragma unroll
      for (int k = 0; k < MMF_LOOP_MAX_MEAS; ++k)
        tr.ll[k] = reinterpret_cast<const float*>(a.gll + static_cast<size_t>(k < a.n_meas ? k : 0) * NM + static_cast<size_t>(n) * a.M);
      tr.n_ll = a.n_meas;
      tr.lw = (t == 0 && a.logw_in0) ? a.logw_in0 + static_cast<size_t>(n) * a.M : nullptr;
      tr.xs = reinterpret_cast<const float*>(a.gb + static_cast<size_t>(n) * a.M * D);
      tr.u = a.uniforms[static_cast<size_t>(t) * a.N + n];
      tr.estimate = a.estimates + (static_cast<size_t>(t) * a.N + n) * D;
      const bool last = t == a.T - 1;
      tr.so = last ? a.belief + static_cast<size_t>(n) * a.M * D : reinterpret_cast<float*>(a.ga + static_cast<size_t>(n) * a.M * D);
      tr.so_tag = last ? 0u : static_cast<unsigned>(t + 1);
      tr.in_tag = static_cast<unsigned>(t + 1);
      tr.abort_word = a.abort_word;
      tr.range_flag = a.range_flag;
      tr.spin_sleep = a.spin_sleep;
      tr.stamps = my_stamps;
      tr.lo = (last && a.logw_out_last) ? a.logw_out_last + static_cast<size_t>(n) * a.M : nullptr;
      tr.io = nullptr;
      if constexpr (ADAPT) {
        tr.lw = ((t & 1) ? a.logw[1] : a.logw[0]) + static_cast<size_t>(n) * a.M;
        tr.lo = ((t & 1) ? a.logw[0] : a.logw[1]) + static_cast<size_t>(n) * a.M;
        tr.ess_floor = a.ess_floor;
        tr.resampled = a.resampled_steps ? a.resampled_steps + static_cast<size_t>(t) * a.N + n : nullptr;
      }
      if constexpr (REC) {
        const size_t tn = static_cast<size_t>(t) * a.N + n;
        tr.cov = a.cov_steps ? a.cov_steps + tn * D * D : nullptr;
        tr.ess = a.ess_steps ? a.ess_steps + tn : nullptr;
        tr.log_evidence = a.log_evidence_steps ? a.log_evidence_steps + tn : nullptr;
      }
      if (!mmf::resample_systematic_trajectory<D, true, true, PREC == MMF_PREC_F32, REC, ADAPT>(smem, tr, a.M, a.M, a.lw_uniform, log_uniform)) {
        if (threadIdx.x == 0 && a.range_flag != nullptr) atomicOr(a.range_flag, MMF_FLAG_GAVE_UP);
        return;
      }
      __syncthreads();  // the LDS of this trajectory is free again
      if (stamp) my_stamps[3] = persist_clock();
    }
  }
}

size_t persist_k1_lds_bytes(int M, int d, bool rec) {  // rec: the record's reduction rows (a recording or an adaptive loop)
  // + 32: this sum has always put the record's rows straight behind the UNROUNDED staged states plus 32 spare bytes, which
  // covers the rounding to 16 the device applies in front of them.  Kept as it is: the loop's LDS request, and with it what
  // the residency test sees, does not change.
  return mmf::k1_systematic_lds(M, M, d, true, false).end + 32 + (rec ? mmf::k1_belief_lds_bytes() : 0);
}

// residency check and launch of the instantiation for (precision, d)
template <bool REC, bool ADAPT>
int persistent_dispatch(int precision, int d, const PersistArgs& pa, size_t lds, int blocks, hipStream_t hs) {
  if (precision != MMF_PREC_F32 && precision != MMF_PREC_F16X3) return MMF_EINVAL;
  auto run = [&](auto k) {
    // the plan assumed one resident workgroup per CU: hold the launch to what the runtime says about THIS kernel
    // (MMF_INTERNAL_NOT_RESIDENT: mmf_pf_forward_loop takes the launch path)
    if (const int rc = mmf::resident(k, blocks, kPersistThreads, lds)) return rc;
    return mmf::launch(k, blocks, kPersistThreads, lds, hs, pa);
  };
  if (precision == MMF_PREC_F32) return d == 3 ? run(pf_persistent_loop_kernel<3, MMF_PREC_F32, REC, ADAPT>) : run(pf_persistent_loop_kernel<2, MMF_PREC_F32, REC, ADAPT>);
  return d == 3 ? run(pf_persistent_loop_kernel<3, MMF_PREC_F16X3, REC, ADAPT>) : run(pf_persistent_loop_kernel<2, MMF_PREC_F16X3, REC, ADAPT>);
}

}  // namespace

// Sizing of the persistent loop (also the eligibility test): 0 = this problem takes the launch-per-step path,
// MMF_EINVAL = not a problem at all.
namespace {
// workgroups of the dynamics role, of each measurement role, of K1; 0 = not eligible
int persistent_plan(int N, int M, int n_meas, int* Gd, int* G, int* GK, int* tpt_out) {
  // K1: the persistent workgroup's 512 threads stand for the launch path's partition of a trajectory (one float4 chunk per
  // thread of up to 1024 threads) only while that partition is a single chunk -- pf_resample_systematic.inc, `virt`
  if (M > 4 * mmf::kK1Block) return 0;
  const int tpt = (M + 31) / 32;
  const long long tiles = static_cast<long long>(N) * tpt;
  const int gk = N < 48 ? N : 48;
  // every workgroup of the grid must be RESIDENT (the roles spin on each other's output; there is no grid barrier): one
  // workgroup per CU (LDS), so the grid is bounded by the CUs of THIS device -- a partition (CPX / DPX / QPX) has 32 /
  // 128 of them, and a sixteenth is left to whatever else is running -- never by the 256 of a whole MI355X
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return n;
  }();
  const int resident = cus - cus / 16 < 240 ? cus - cus / 16 : 240;
  const int budget = resident - gk;
  if (budget < 1 + n_meas) return 0;
  // a tile per SIMD (four waves of a workgroup) where the chip has room, the dynamics network -- nine layers, the
  // longest stage of the chain -- first
  auto want = [&](int waves_per_wg) { long long w = (tiles + waves_per_wg - 1) / waves_per_wg; return static_cast<int>(w < 1 ? 1 : w); };
  int gd = want(4), gm = want(4);
  if (gd + n_meas * gm > budget) {
    gm = want(8) > (budget - gd) / n_meas ? want(8) : (budget - gd) / n_meas;  // measurement roles share what is left ...
    if (gd + n_meas * gm > budget) { gd = gm = budget / (1 + n_meas); }        // ... or everybody gets the same share
  }
  if (gd > 80) gd = 80;
  if (gm > 80) gm = 80;
  if (gd < 1 || gm < 1) return 0;
  if (M > 2048 || tiles > static_cast<long long>(gd < gm ? gd : gm) * kPersistWaves * 3) {
    // Round 6, several rounds of tiles per wave and step (32 x 4096: 4,096 tiles per network): the roles' workgroups
    // stream tiles trajectory by trajectory and the stages overlap ACROSS trajectories, so what counts is that the
    // network roles finish a step's tiles at the same rate -- the budget goes to them in proportion to their depth
    // (9 : 7 layers).  Beyond kPersistMaxRounds rounds the launch path's 64-particle pipelined tiles win.
    // Measured (profiles/r06/persistent_multi_round_ab.txt): 32 x 2048 +13 %, 64 x 1024 +16 %, 40 x 1500 +19 %, 24 x 3000 +47 %
    // over the launches; 128 x 1024 (8 rounds) -4 %; 8 / 16 x 4096 -8 / -4 % (too few trajectories in flight for the
    // stages to overlap, and K1's two chunks of polled granules on every trajectory's chain) -- hence both limits.
    if (M > 2048 && N < 24) return 0;
    gd = budget * 9 / (9 + 7 * n_meas);
    gm = (budget - gd) / n_meas;
    if (gd < 1 || gm < 1) return 0;
    static const int max_rounds = getenv("MMF_PF_PERSIST_MAX_ROUNDS") ? atoi(getenv("MMF_PF_PERSIST_MAX_ROUNDS")) : kPersistMaxRounds;
    if (tiles > static_cast<long long>(gm) * kPersistWaves * max_rounds) return 0;
  }
  *Gd = gd; *G = gm; *GK = gk; *tpt_out = tpt;
  return gd + n_meas * gm + gk;
}
}  // namespace

// Sizing of the persistent loop (also the eligibility test): 0 = this problem takes the launch-per-step path,
// MMF_EINVAL = not a problem at all.
extern "C" int mmf_pf_persistent_plan(int N, int M, int n_meas, int* G_out, int* GK_out, int* tpt_out) {
  if (N < 1 || M < 1 || n_meas < 1 || n_meas > MMF_LOOP_MAX_MEAS) return MMF_EINVAL;
  int gd, g, gk, tpt;
  const int blocks = persistent_plan(N, M, n_meas, &gd, &g, &gk, &tpt);
  if (blocks <= 0) return 0;
  if (G_out) *G_out = g;
  if (GK_out) *GK_out = gk;
  if (tpt_out) *tpt_out = tpt;
  return blocks;
}

// 4-byte words of the loop's device workspace: [abort word, padded to 16 B][belief granules (N, M, d)]
// [propagated-row granules (N, M, d)][log-likelihood granules (n_meas, N, M)]; zeroed by every call
extern "C" size_t mmf_pf_persistent_sync_words(int N, int M, int d, int n_meas) {
  if (N < 1 || M < 1 || d < 1 || n_meas < 1) return 0;
  const size_t NM = static_cast<size_t>(N) * M;
  return 4 + 2 * (2 * NM * d + static_cast<size_t>(n_meas) * NM);
}

int mmf_internal_pf_persistent(const MmfPfLoopArgs* a, void* stream, float ess_threshold, int32_t* resampled_steps) {
  if (!a || !a->sync_words) return MMF_EINVAL;
  const bool adaptive = ess_threshold > 0.f;
  if (adaptive && (!a->logw_a || !a->logw_b)) return MMF_EINVAL;
  if (a->resample_mode != 1 || (a->soft_alpha > 0.f && a->soft_alpha < 1.f) || a->estimate_argmax || a->events ||
      a->loglik_steps || a->indices_steps || a->n_res_dyn != 3 || a->n_res_meas != 2 || a->T < 1)
    return MMF_EINVAL;
  if (a->d != 2 && a->d != 3) return MMF_EINVAL;
  PersistArgs pa{};
  const int blocks = persistent_plan(a->N, a->M, a->n_meas, &pa.Gd, &pa.G, &pa.GK, &pa.tpt);
  if (blocks <= 0) return MMF_EINVAL;
  const size_t words = mmf_pf_persistent_sync_words(a->N, a->M, a->d, a->n_meas);
  if (static_cast<size_t>(a->n_sync_words) < words) return MMF_EINVAL;
  pa.T = a->T; pa.N = a->N; pa.M = a->M; pa.n_meas = a->n_meas; pa.logw_stride = a->logw_stride;
  pa.dyn_packed = a->dyn_packed; pa.dyn_bias = a->dyn_bias;
  for (int k = 0; k < a->n_meas; ++k) {
    if (!a->meas_packed[k] || !a->meas_bias[k]) return MMF_EINVAL;
    pa.meas_packed[k] = a->meas_packed[k]; pa.meas_bias[k] = a->meas_bias[k]; pa.meas_logw[k] = a->meas_logw[k];
  }
  pa.noise = a->noise_mode == 2 ? nullptr : a->noise;
  pa.scale_tril = a->scale_tril; pa.uniforms = a->uniforms;
  pa.belief = a->states_a;
  pa.logw_in0 = a->logw_a;
  // the launch path ping-pongs the two log-weight buffers every step and only the last step writes: into logw_b
  // for an odd number of steps, logw_a for an even one
  const bool last_into_b = ((a->T - 1) & 1) == 0;
  pa.logw_out_last = last_into_b ? a->logw_b : a->logw_a;
  pa.estimates = a->estimates; pa.range_flag = a->range_flag;
  pa.cov_steps = a->cov_steps; pa.ess_steps = a->ess_steps; pa.log_evidence_steps = a->log_evidence_steps;
  pa.logw[0] = a->logw_a; pa.logw[1] = a->logw_b;  // ADAPT: step t writes logw[(t + 1) & 1], so the last step's land where last_into_b says
  pa.ess_floor = ess_threshold * static_cast<float>(a->M);  // the product rounded once, in fp32
  pa.resampled_steps = resampled_steps;
  const bool rec = a->cov_steps || a->ess_steps || a->log_evidence_steps;  // the recording instantiation of the kernel
  const size_t NM = static_cast<size_t>(a->N) * a->M;
  unsigned* w = reinterpret_cast<unsigned*>(a->sync_words);
  pa.abort_word = w;
  pa.ga = reinterpret_cast<Granule*>(w + 4);
  pa.gb = pa.ga + NM * a->d;
  pa.gll = pa.gb + NM * a->d;
  pa.noise_seed = a->noise_seed; pa.noise_step0 = a->noise_step0; pa.noise_traj0 = a->noise_traj0; pa.noise_mode = a->noise_mode;
  pa.lw_uniform = static_cast<float>(-std::log(static_cast<double>(a->M)));
  hipStream_t hs = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(a->sync_words, 0, words * sizeof(unsigned), hs);  // every tag 0: no step has delivered
  if (e != hipSuccess) return static_cast<int>(e);
  // diagnostic (MMF_PERSIST_STAMPS=<step>): per-wave cycle stamps of one step -> stderr after a synchronise
  pa.spin_sleep = 1;  // s_sleep 1 between polls (busy polling measured no faster and starves the SIMD's other wave)
  static const char* stamp_env = getenv("MMF_PERSIST_STAMPS");
  const size_t n_stamps = static_cast<size_t>(blocks) * kPersistWaves * 6;
  if (stamp_env && a->T > atoi(stamp_env)) {
    if (hipMalloc(reinterpret_cast<void**>(&pa.stamps), n_stamps * 8) != hipSuccess) return MMF_EINVAL;
    (void)hipMemsetAsync(pa.stamps, 0, n_stamps * 8, hs);
    pa.stamp_step = atoi(stamp_env);
  }
  size_t lds = static_cast<size_t>(blob_floats(3)) * sizeof(float);
  const size_t k1 = persist_k1_lds_bytes(a->M, a->d, rec || adaptive);
  if (k1 > lds) lds = k1;
  if (lds > mmf::kLdsPerCu) return MMF_ETOOLARGE;
  const int rc = adaptive ? (rec ? persistent_dispatch<true, true>(a->precision, a->d, pa, lds, blocks, hs)
                                 : persistent_dispatch<false, true>(a->precision, a->d, pa, lds, blocks, hs))
                          : (rec ? persistent_dispatch<true, false>(a->precision, a->d, pa, lds, blocks, hs)
                                 : persistent_dispatch<false, false>(a->precision, a->d, pa, lds, blocks, hs));
  if (rc) return rc;
  if (pa.stamps) {
    std::vector<unsigned long long> h(n_stamps);
    (void)hipStreamSynchronize(hs);
    (void)hipMemcpy(h.data(), pa.stamps, n_stamps * 8, hipMemcpyDeviceToHost);
    (void)hipFree(pa.stamps);
    const char* names[] = {"dynamics", "measure0", "measure1", "measure2", "measure3", "k1"};
    for (int role = 0; role <= a->n_meas + 1; ++role) {
      const bool k1r = role == a->n_meas + 1;
      const int b0 = k1r ? pa.Gd + a->n_meas * pa.G : (role == 0 ? 0 : pa.Gd + (role - 1) * pa.G);
      const int b1 = k1r ? blocks : (role == 0 ? pa.Gd : b0 + pa.G);
      double busy = 0, mx = 0, wait = 0, comp = 0, real = 0;
      int cnt = 0;
      for (int bb = b0; bb < b1; ++bb)
        for (int wv = 0; wv < (k1r ? 1 : kPersistWaves); ++wv) {
          const unsigned long long* p = &h[(static_cast<size_t>(bb) * kPersistWaves + wv) * 6];
          if (!p[3]) continue;
          ++cnt;
          const double v = double(p[3] - p[0]);  // (stamps of ONE wave share a clock; different XCDs do not)
          busy += v;
          if (p[1] && p[2]) { wait += double(p[1] - p[0]); comp += double(p[2] - p[1]); }
          if (p[5] > p[4]) real += double(p[5] - p[4]);
          if (v > mx) mx = v;
        }
      if (cnt) fprintf(stderr, "persist stamps step %d %-9s waves %3d  arrive -> delivered: mean %.0f max %.0f cycles (waiting for input %.0f, computing %.0f); shader clock %.2f GHz\n",
                       pa.stamp_step, names[k1r ? 5 : role], cnt, busy / cnt, mx, wait / cnt, comp / cnt, real > 0 ? busy / real * 0.1 : 0.0);
    }
  }
  // a reader that gives up ORs MMF_FLAG_GAVE_UP into the status word: the host re-runs the loop as launches
  if (a->final_location) *a->final_location = last_into_b ? 2 : 0;
  return 0;
}
