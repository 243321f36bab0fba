// The extended Kalman filters' step loop as ONE persistent launch per forward_loop (round 6).  Included at the end of
// particle_net.hip (the Jacobian tile is its tile machinery) after pf_persistent.inc (granules, bounded spins).
//
//   torchfilter Filter.forward_loop over  /root/reference/crossmodal/base_models/crossmodal_kf.py:88-151  and
//   unimodal_kf.py:162-250  (call site eval_helpers.py:139-142)
//
// Why: an EKF step is two launches -- the forward-mode Jacobians of the K dynamics networks (K5, 20 us for 1024
// trajectories: 16 workgroups on 256 CUs) and predict / correct / fuse (K3, 5 us) -- with ~8 us of queue between dependent
// launches: ~40 us per step in which the chip is idle, 13 % of a 1024-trajectory step behind the image encoders and ALL of a
// 32-trajectory step (BASELINE config 1).  But the recursion couples nothing across trajectories: sub-filter k of
// trajectory n needs its own previous belief, its network, and -- only where the filter fuses AND feeds the fused belief
// back -- the other sub-filters' corrected beliefs of the SAME trajectory.  So a wave owns a tile of 8 trajectories (32
// Jacobian columns: primal + up to 3 tangents each) of ONE sub-filter for all T steps: the belief stays in registers,
// the network's weights in LDS, a step is the Jacobian tile + the d x d algebra (every lane of a trajectory's quad, both
// lane halves, runs the same statements on the same values -- no broadcast, no divergence).  With K > 1 the workgroups
// of the K roles meet once per step and trajectory through 8-byte {value, tag} granules in L2 (pf_persistent.inc's
// hand-off: the data is the flag), two slots by step parity: a role can be at most one step ahead of a role it waits for.
//
// Same bits as the loop of launches: jacobian_tile and particle_net_kernel<D, 3, kJacobian, 1, PREC, 2> call the same
// network pieces of particle_net_tiles.h (a column does not depend on what else sits in its tile), the algebra is
// ekf_algebra.h's functions, which ekf_step_kernel calls too (tests/test_gpu_models.py::test_persistent_ekf_loop_equals_loop_of_launches).

#include "ekf_algebra.h"

namespace {

constexpr int kEkfPersistThreads = 256;  // four waves, one per SIMD: the step is a latency chain
constexpr int kEkfPersistWaves = kEkfPersistThreads / MMF_WAVE;
constexpr int kEkfMaxRounds = 2;         // tiles per wave, each run for all T steps before the next (8192 x 2 sub-filters = 3
                                         // rounds: 2 % slower than the launches, profiles/r06/ekf_persistent_ab.txt)

struct EkfPersistArgs {
  int T, N, K, fusion, feedback, G;      // G: workgroups per role
  const float* dyn_packed[MMF_LOOP_MAX_MEAS];
  const float* dyn_bias[MMF_LOOP_MAX_MEAS];  // (T*N, 64)
  const float* q_tril;                   // (K, d, d)
  const float* z;                        // (T, K, N, d)
  const float* r_tril;                   // (T, K, N, d, d)
  const float* fuse_w;                   // (T, K, N, d) or null
  float* mu;                             // (K, N, d) in / out
  float* Sigma;                          // (K, N, d, d) in / out
  float* Sigma_f;                        // (N, d, d) out (fusion != 0)
  float* estimates;                      // (T, N, d)
  float* Sigma_steps;                    // (T, N, d, d) or null: every step's posterior covariance (fused, or sub-filter 0's)
  const int32_t* feedback_gate;          // (T) or null
  mmf::Granule* xg;                      // [2 slots][K][N][d + d*d] corrected beliefs on their way to the other roles
  unsigned* abort_word;
  int* range_flag;
};

template <int Q>
__device__ __forceinline__ float quad_lane(float x) {  // lane (l & ~3) + Q of every quad
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), Q * 0x55, 0xf, 0xf, true));
}

// One Jacobian tile: 32 columns = 8 trajectories x {primal, e_1 .. e_3}; x: the trajectory's mean, the same in every lane of
// its quad and in both lane halves.  Out, in every lane of the quad: x' = f(x) and A = d x' / d x.
// Built from particle_net_tiles.h's pieces, as particle_net_kernel<D, 3, kJacobian, 1, PREC, 2> is: first_layer,
// seed_nonfinite, net_unpipelined (join_init from this step's row), report_range, head, jacobian_outputs.  Its own: the
// first-layer operands come from the register mean, the outputs are broadcast across the quad into Mat<D>.
template <int D, int PREC>
__device__ __forceinline__ void jacobian_tile(const float* __restrict__ lds, const float* __restrict__ traj_bias_row,
                                              const float (&x)[D], int lane, float neg_one, int* range_flag,
                                              float (&xp)[D], mmf_ekf::Mat<D>& A) {
  constexpr int NRES = 3;
  constexpr bool F16 = PREC == MMF_PREC_F16X3;
  constexpr int NOUT = D + 1, KS0 = (D + 2) / 2;
  const int j = lane & 31, h = lane >> 5;
  const int role = j & 3;
  const bool primal = role == 0;
  float b0[KS0][1];
#pragma unroll
  for (int s = 0; s < KS0; ++s) {
    const int comp = 2 * s + h;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i) v = comp == i ? x[i] : v;
    const float prim = comp < D ? v : (comp == D ? 1.f : 0.f);
    b0[s][0] = primal ? prim : ((comp == role - 1) ? 1.f : 0.f);
  }
  Act<1> X, H;
  first_layer<1>(lds, b0, X, lane);
  half2v amax = {0, 0};
  if constexpr (F16) seed_nonfinite<1>(b0, amax);
  net_unpipelined<1, NRES, kJacobian, PREC>(lds, X, H, [&](Act<1>& acc) {
    join_init<1>(acc, 0, load_join_row(traj_bias_row, lane), primal);
  }, lane, neg_one, amax, primal);
  if constexpr (F16) report_range(range_flag, amax);
  float out[NOUT][1], mine[NOUT], own[D];
  head<NRES>(lds, H, lane, out);
#pragma unroll
  for (int o = 0; o < NOUT; ++o) mine[o] = out[o][0];
  // this lane's own output: role 0 -> x'_i, role c + 1 -> column c of the Jacobian
  jacobian_outputs<D>(mine, lds + off_bhead(NRES), x, role, own);
#pragma unroll
  for (int i = 0; i < D; ++i) {
    xp[i] = quad_lane<0>(own[i]);
    A.a[i][0] = quad_lane<1>(own[i]);
    if constexpr (D > 1) A.a[i][1] = quad_lane<2>(own[i]);
    if constexpr (D > 2) A.a[i][2] = quad_lane<3>(own[i]);
  }
}

template <int D, int PREC>
__global__ __launch_bounds__(kEkfPersistThreads, 1) void ekf_persistent_loop_kernel(EkfPersistArgs a) {
  using namespace mmf_ekf;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int kNres = 3, BEL = D + D * D;
  const int k = blockIdx.y, g = blockIdx.x;
  auto pick = [&](const float* const (&v)[MMF_LOOP_MAX_MEAS]) -> const float* {
    return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3];
  };
  const float* packed = pick(a.dyn_packed);
  const float* bias_all = pick(a.dyn_bias);
  mmf::stage_to_lds<blob_floats(kNres) / 4, kEkfPersistThreads>(reinterpret_cast<const float4*>(packed), reinterpret_cast<float4*>(lds), threadIdx.x);
  __syncthreads();
  float neg_one = -1.0f;
  asm volatile("" : "+s"(neg_one));
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31;
  const int ntiles = (a.N + 7) / 8;
  const size_t N = static_cast<size_t>(a.N);
  const Mat<D> L = load_mat<D>(a.q_tril + static_cast<size_t>(k) * D * D);

  for (int tile = g * kEkfPersistWaves + wave; tile < ntiles; tile += a.G * kEkfPersistWaves) {
    const int n_raw = 8 * tile + (j >> 2);
    const bool valid = n_raw < a.N;
    const size_t n = valid ? n_raw : a.N - 1;
    const bool writer = valid && (lane & 35) == 0;  // ONE lane per trajectory: role 0 of the lower lane half
    const size_t row = static_cast<size_t>(k) * N + n;
    float mu[D];
#pragma unroll
    for (int i = 0; i < D; ++i) mu[i] = a.mu[row * D + i];
    Mat<D> S = load_mat<D>(a.Sigma + row * D * D);
    Mat<D> Sf;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int jj = 0; jj < D; ++jj) Sf.a[i][jj] = 0.f;

    for (int t = 0; t < a.T; ++t) {
      // everything of this step that does not depend on the recursion is requested ahead of the tile
      const size_t trow = (static_cast<size_t>(t) * a.K + k) * N + n;
      float zk[D];
#pragma unroll
      for (int i = 0; i < D; ++i) zk[i] = a.z[trow * D + i];
      const Mat<D> Tk = load_mat<D>(a.r_tril + trow * D * D);
      float w[kMaxK][D];
      if (a.fusion == 1) {
#pragma unroll
        for (int kk = 0; kk < kMaxK; ++kk) {
          if (kk >= a.K) break;
#pragma unroll
          for (int i = 0; i < D; ++i) w[kk][i] = a.fuse_w[((static_cast<size_t>(t) * a.K + kk) * N + n) * D + i];
        }
      }
      int feedback = a.feedback;
      if (a.feedback_gate != nullptr && a.feedback_gate[t] == 0) feedback = 0;

      float xp[D];
      Mat<D> A;
      jacobian_tile<D, PREC>(lds, bias_all + (static_cast<size_t>(t) * N + n) * kUnits, mu, lane, neg_one, a.range_flag, xp, A);

      float mus[kMaxK][D];
      Mat<D> Ss[kMaxK];
      float mine_mu[D];
      Mat<D> mine_S;
      predict_correct<D>(A, S, L, Tk, xp, zk, mine_mu, mine_S);

      if (a.K > 1 && a.fusion != 0) {
        // publish this role's corrected belief, collect the others' (slot = step parity, tag = step + 1)
        mmf::Granule* slot = a.xg + static_cast<size_t>(t & 1) * a.K * N * BEL;
        const unsigned tag = static_cast<unsigned>(t + 1);
        if (writer) {
          mmf::Granule* p = slot + row * BEL;
#pragma unroll
          for (int i = 0; i < D; ++i) mmf::st_granule(p + i, mine_mu[i], tag);
#pragma unroll
          for (int i = 0; i < D; ++i)
#pragma unroll
            for (int jj = 0; jj < D; ++jj) mmf::st_granule(p + D + i * D + jj, mine_S.a[i][jj], tag);
        }
        bool gave_up = false;
#pragma unroll
        for (int kk = 0; kk < kMaxK; ++kk) {
          if (kk >= a.K) break;
          if (kk == k) {
#pragma unroll
            for (int i = 0; i < D; ++i) mus[kk][i] = mine_mu[i];
            Ss[kk] = mine_S;
            continue;
          }
          const mmf::Granule* p = slot + (static_cast<size_t>(kk) * N + n) * BEL;
          float v[BEL];
          unsigned spins = 0;
          for (;;) {
            bool ok = true;
#pragma unroll
            for (int e = 0; e < BEL; ++e) {
              const mmf::Granule gr = mmf::ld_granule(p + e);
              ok &= mmf::granule_tag(gr) == tag;
              v[e] = mmf::granule_value(gr);
            }
            if (__all(ok)) break;
            __builtin_amdgcn_s_sleep(1);
            if ((++spins & 63u) == 0) {  // wave-uniform; mirrors mmf::spin_stop (calling it here costs two more spilled SGPRs)
              int stop = 0;
              if (lane == 0) stop = (spins > mmf::kGranuleSpinLimit || __hip_atomic_load(a.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) ? 1 : 0;
              if (__builtin_amdgcn_readfirstlane(stop)) { gave_up = true; break; }
            }
          }
          if (gave_up) break;
#pragma unroll
          for (int i = 0; i < D; ++i) mus[kk][i] = v[i];
#pragma unroll
          for (int i = 0; i < D; ++i)
#pragma unroll
            for (int jj = 0; jj < D; ++jj) Ss[kk].a[i][jj] = v[D + i * D + jj];
        }
        if (gave_up) {  // wave-uniform: the host discards this loop and re-runs it as launches (engine.run_persistent, MMF_FLAG_GAVE_UP)
          if (lane == 0) mmf::give_up(a.abort_word, a.range_flag);
          return;
        }
      } else {
#pragma unroll
        for (int kk = 0; kk < kMaxK; ++kk)  // (constant indices: a run-time index sends the arrays to scratch)
          if (kk == k) {
#pragma unroll
            for (int i = 0; i < D; ++i) mus[kk][i] = mine_mu[i];
            Ss[kk] = mine_S;
          }
      }

      float mf[D];
#pragma unroll
      for (int i = 0; i < D; ++i) mf[i] = 0.f;
      if (a.fusion != 0) fuse<D>(a.K, a.fusion, w, mus, Ss, mf, Sf);
      const bool fb = a.fusion != 0 && feedback != 0;
#pragma unroll
      for (int i = 0; i < D; ++i) mu[i] = fb ? mf[i] : mine_mu[i];
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int jj = 0; jj < D; ++jj) S.a[i][jj] = fb ? Sf.a[i][jj] : mine_S.a[i][jj];
      if (writer && k == 0) {  // the fused mean, or (no fusion) sub-filter 0's corrected mean
#pragma unroll
        for (int i = 0; i < D; ++i) a.estimates[(static_cast<size_t>(t) * N + n) * D + i] = a.fusion != 0 ? mf[i] : mine_mu[i];
        // ... and the matrix that goes with it (gated-off feedback: still the fused posterior, as the estimate is)
        if (a.Sigma_steps != nullptr) store_mat<D>(a.Sigma_steps + (static_cast<size_t>(t) * N + n) * D * D, a.fusion != 0 ? Sf : mine_S);
      }
    }
    if (writer) {
#pragma unroll
      for (int i = 0; i < D; ++i) a.mu[row * D + i] = mu[i];
      store_mat<D>(a.Sigma + row * D * D, S);
      if (k == 0 && a.fusion != 0 && a.T > 0) store_mat<D>(a.Sigma_f + n * D * D, Sf);
    }
  }
}

// workgroups per role; 0 = not eligible (the loop of launches)
int ekf_persistent_plan(int N, int K, int* G_out) {
  if (N < 1 || K < 1 || K > MMF_LOOP_MAX_MEAS) return 0;
  static const int cus = [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return n;
  }();
  // the roles wait for each other (K > 1): every workgroup resident, one per CU (LDS), a sixteenth of the device left alone
  const int resident = cus - cus / 16 < 240 ? cus - cus / 16 : 240;
  const int per_role = resident / K;
  if (per_role < 1) return 0;
  const int ntiles = (N + 7) / 8;
  int G = (ntiles + kEkfPersistWaves - 1) / kEkfPersistWaves;
  if (G > per_role) G = per_role;
  if (ntiles > G * kEkfPersistWaves * kEkfMaxRounds) return 0;
  *G_out = G;
  return G * K;
}

template <int D, int PREC>
int launch_ekf_persistent(const EkfPersistArgs& pa, int blocks, hipStream_t s) {
  auto kfn = ekf_persistent_loop_kernel<D, PREC>;
  const size_t lds = static_cast<size_t>(blob_floats(3)) * sizeof(float);
  if (const int rc = mmf::resident(kfn, blocks, kEkfPersistThreads, lds)) return rc;
  return mmf::launch(kfn, dim3(pa.G, pa.K), kEkfPersistThreads, lds, s, pa);
}

}  // namespace

extern "C" int mmf_ekf_persistent_plan(int N, int K) {
  if (N < 1 || K < 1 || K > MMF_LOOP_MAX_MEAS) return MMF_EINVAL;
  int G = 0;
  return ekf_persistent_plan(N, K, &G);
}

// 4-byte words of the loop's device workspace: [abort word, padded to 16 B][2 slots][K][N][d + d*d] granules; zeroed by every call
extern "C" size_t mmf_ekf_persistent_sync_words(int N, int K, int d) {
  if (N < 1 || K < 1 || d < 1) return 0;
  return 4 + 2 * (2 * static_cast<size_t>(K) * N * (d + d * d));
}

int mmf_internal_ekf_persistent(const MmfEkfLoopArgs* a, float* Sigma_steps, void* stream) {
  if (!a || !a->sync_words) return MMF_EINVAL;
  if ((a->d != 2 && a->d != 3) || a->n_res_dyn != 3 || a->T < 1) return MMF_EINVAL;
  if (a->precision != MMF_PREC_F32 && a->precision != MMF_PREC_F16X3) return MMF_EINVAL;
  EkfPersistArgs pa{};
  const int blocks = ekf_persistent_plan(a->N, a->K, &pa.G);
  if (blocks <= 0) return MMF_INTERNAL_NOT_RESIDENT;
  const size_t words = mmf_ekf_persistent_sync_words(a->N, a->K, a->d);
  if (static_cast<size_t>(a->n_sync_words) < words) return MMF_EINVAL;
  pa.T = a->T; pa.N = a->N; pa.K = a->K; pa.fusion = a->fusion; pa.feedback = a->feedback;
  for (int k = 0; k < a->K; ++k) { pa.dyn_packed[k] = a->dyn_packed[k]; pa.dyn_bias[k] = a->dyn_bias[k]; }
  pa.q_tril = a->q_tril; pa.z = a->z; pa.r_tril = a->r_tril; pa.fuse_w = a->fuse_w;
  pa.mu = a->mu; pa.Sigma = a->Sigma; pa.Sigma_f = a->Sigma_f; pa.estimates = a->estimates; pa.Sigma_steps = Sigma_steps;
  pa.feedback_gate = a->feedback_gate;
  unsigned* w = reinterpret_cast<unsigned*>(a->sync_words);
  pa.abort_word = w;
  pa.xg = reinterpret_cast<mmf::Granule*>(w + 4);
  pa.range_flag = a->range_flag;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(a->sync_words, 0, words * sizeof(unsigned), hs);  // every tag 0: no step has delivered
  if (e != hipSuccess) return static_cast<int>(e);
  if (a->precision == MMF_PREC_F32) return a->d == 3 ? launch_ekf_persistent<3, MMF_PREC_F32>(pa, blocks, hs) : launch_ekf_persistent<2, MMF_PREC_F32>(pa, blocks, hs);
  return a->d == 3 ? launch_ekf_persistent<3, MMF_PREC_F16X3>(pa, blocks, hs) : launch_ekf_persistent<2, MMF_PREC_F16X3>(pa, blocks, hs);
}
