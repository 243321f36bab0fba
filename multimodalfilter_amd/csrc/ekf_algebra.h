// Every product-sum below is an EXPLICIT fused multiply-add and implicit contraction is off inside these functions: which
// a * b + c the compiler fuses otherwise depends on the kernel the function is inlined into, and the two callers
// (ekf_step_kernel, the persistent loop) must agree to the bit.
// The d x d algebra of K3 (one trajectory per lane, everything in registers) and the two halves of an EKF step -- predict +
// correct of ONE sub-filter, and the fusion of K sub-filters -- as device functions: ekf_step_kernel (ekf.hip) and the
// persistent EKF loop (ekf_persistent.inc) run the same statements in the same order, so their results are the same bits.
//   torchfilter ExtendedKalmanFilter._predict_step / _update_step with C = I (external dependency)
//   /root/reference/crossmodal/base_models/crossmodal_kf.py:153-167  (crossmodal fusion)
//   /root/reference/crossmodal/base_models/utility.py:4-11           (weighted_average)
//   /root/reference/crossmodal/base_models/unimodal_kf.py:204-242    (information-form fusion)
#pragma once
#include "mmf_common.h"
#include "../../include/mmf_detmath.h"

namespace mmf_ekf {

template <int D, typename F = float>
struct Mat {
  F a[D][D];
};

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float abs_(float a) { return __builtin_fabsf(a); }
__device__ __forceinline__ double abs_(double a) { return __builtin_fabs(a); }

template <int D>
__device__ __forceinline__ Mat<D> load_mat(const float* p) {
  Mat<D> m;
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) m.a[i][j] = p[i * D + j];
  return m;
}

template <int D>
__device__ __forceinline__ void store_mat(float* p, const Mat<D>& m) {
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) p[i * D + j] = m.a[i][j];
}

template <int D>
__device__ __forceinline__ Mat<D> matmul(const Mat<D>& x, const Mat<D>& y) {
#pragma clang fp contract(off)
  Mat<D> r;
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) s = __builtin_fmaf(x.a[i][k], y.a[k][j], s);
      r.a[i][j] = s;
    }
  return r;
}

template <int D>
__device__ __forceinline__ Mat<D> matmul_nt(const Mat<D>& x, const Mat<D>& y) {  // x y^T
#pragma clang fp contract(off)
  Mat<D> r;
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < D; ++k) s = __builtin_fmaf(x.a[i][k], y.a[j][k], s);
      r.a[i][j] = s;
    }
  return r;
}

// Gauss-Jordan with partial pivoting (the pivot order LU-based torch.inverse uses); row
// swaps are branch-free selects so every index stays compile-time and the matrix stays in
// registers.  F = float everywhere but in the information-form fusion (see fuse).
template <int D, typename F>
__device__ __forceinline__ Mat<D, F> inverse(Mat<D, F> m) {
#pragma clang fp contract(off)
  Mat<D, F> inv;
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) inv.a[i][j] = (i == j) ? F(1) : F(0);
#pragma unroll
  for (int c = 0; c < D; ++c) {
#pragma unroll
    for (int r = c + 1; r < D; ++r) {
      const bool sw = abs_(m.a[r][c]) > abs_(m.a[c][c]);
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const F t0 = m.a[c][j], t1 = m.a[r][j];
        m.a[c][j] = sw ? t1 : t0;
        m.a[r][j] = sw ? t0 : t1;
        const F u0 = inv.a[c][j], u1 = inv.a[r][j];
        inv.a[c][j] = sw ? u1 : u0;
        inv.a[r][j] = sw ? u0 : u1;
      }
    }
    const F piv = F(1) / m.a[c][c];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      m.a[c][j] *= piv;
      inv.a[c][j] *= piv;
    }
#pragma unroll
    for (int r = 0; r < D; ++r) {
      if (r == c) continue;
      const F f = m.a[r][c];
#pragma unroll
      for (int j = 0; j < D; ++j) {
        m.a[r][j] = fma_(-f, m.a[c][j], m.a[r][j]);
        inv.a[r][j] = fma_(-f, inv.a[c][j], inv.a[r][j]);
      }
    }
  }
  return inv;
}

constexpr int kMaxK = 4;

// predict + correct of one sub-filter (C = I):  S- = A S A^T + L L^T;  K = S- (S- + T T^T)^-1;
// mu = mu- + K (z - mu-);  S = (I - K) S-  with  I - K = T T^T (S- + T T^T)^-1
// The by-products a caller may keep: Sp = S- (the predicted covariance), Sinn = S- + T T^T (the innovation covariance),
// Si = Sinn^-1 and innov = z - mu-.  predict_correct below drops them; the statements that form mu_out / S_out are these, in
// this order, for either caller.
template <int D>
__device__ __forceinline__ void predict_correct_parts(const Mat<D>& Ak, const Mat<D>& S0, const Mat<D>& L, const Mat<D>& T,
                                                      const float (&mp)[D], const float (&z)[D], float (&mu_out)[D],
                                                      Mat<D>& S_out, Mat<D>& Sp, Mat<D>& Sinn, Mat<D>& Si, float (&innov)[D]) {
#pragma clang fp contract(off)
  const Mat<D> AS = matmul<D>(Ak, S0);
  Sp = matmul_nt<D>(AS, Ak);
  const Mat<D> Q = matmul_nt<D>(L, L);
  const Mat<D> Rm = matmul_nt<D>(T, T);
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      Sp.a[i][j] += Q.a[i][j];
      Sinn.a[i][j] = Sp.a[i][j] + Rm.a[i][j];
    }
  Si = inverse<D>(Sinn);
  const Mat<D> G = matmul<D>(Sp, Si);
  // I - G = (Sinn - S-) Sinn^-1 = T T^T Sinn^-1, formed as that product: where the sensor is sharp next to the prediction
  // G is close to I and "I - G" keeps only the rounding of G -- 7e-5 of S on its small directions, which the information
  // form (fuse, fusion 2) inverts: mu_f went 2e-4 .. 6e-4 off from that alone.  As a product, S is good to 1e-5.
  const Mat<D> ImG = matmul<D>(Rm, Si);
#pragma unroll
  for (int i = 0; i < D; ++i) innov[i] = z[i] - mp[i];
#pragma unroll
  for (int i = 0; i < D; ++i) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) s = __builtin_fmaf(G.a[i][j], innov[j], s);
    mu_out[i] = mp[i] + s;
  }
  S_out = matmul<D>(ImG, Sp);
}

template <int D>
__device__ __forceinline__ void predict_correct(const Mat<D>& Ak, const Mat<D>& S0, const Mat<D>& L, const Mat<D>& T,
                                                const float (&mp)[D], const float (&z)[D], float (&mu_out)[D], Mat<D>& S_out) {
  Mat<D> Sp, Sinn, Si;
  float innov[D];
  predict_correct_parts<D>(Ak, S0, L, T, mp, z, mu_out, S_out, Sp, Sinn, Si, innov);
}

// What the innovation says about the model (include/mmf.h, "innovation statistics"):  nis = innov^T Sinn^-1 innov as an
// explicit fma chain over Si innov, and log det Sinn from the Cholesky factorisation of Sinn in registers -- the sum of the
// logs of the squared pivots, with the deterministic log of mmf_detmath.h.  A pivot that is not positive (Sinn not positive
// definite, or not finite) makes log det NaN; the NIS is whatever the inverse gave.
template <int D>
__device__ __forceinline__ void innovation_stats(const Mat<D>& Sinn, const Mat<D>& Si, const float (&innov)[D], float& nis,
                                                 float& logdet) {
#pragma clang fp contract(off)
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    float y = 0.f;
#pragma unroll
    for (int j = 0; j < D; ++j) y = __builtin_fmaf(Si.a[i][j], innov[j], y);
    q = __builtin_fmaf(innov[i], y, q);
  }
  nis = q;
  Mat<D> C;  // lower triangle: Sinn = C C^T
  float ld = 0.f;
  bool pd = true;
#pragma unroll
  for (int j = 0; j < D; ++j) {
    float s = Sinn.a[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s = __builtin_fmaf(-C.a[j][k], C.a[j][k], s);
    pd = pd && s >= 1.17549435e-38f && s <= 3.40282347e+38f;  // mmf_det_log's domain: normal, finite (false for NaN too)
    ld += mmf_det_log(pd ? s : 1.f);
    const float dj = __builtin_sqrtf(s);
    C.a[j][j] = dj;
#pragma unroll
    for (int i = j + 1; i < D; ++i) {
      float t = Sinn.a[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) t = __builtin_fmaf(-C.a[i][k], C.a[j][k], t);
      C.a[i][j] = t / dj;
    }
  }
  logdet = pd ? ld : __builtin_nanf("");
}

// log N(innov; 0, Sinn) = -1/2 (nis + log det Sinn + d log 2 pi)
__device__ __forceinline__ float loglik_of(float nis, float logdet, int d) {
#pragma clang fp contract(off)
  const float c = static_cast<float>(d) * 1.8378770664093453f;
  return -0.5f * ((nis + logdet) + c);
}

// fusion of K corrected sub-filters: 1 = crossmodal weighted average (w: (K, D) weights of this trajectory),
// 2 = information form
template <int D>
__device__ __forceinline__ void fuse(int K, int fusion, const float (&w)[kMaxK][D], const float (&mus)[kMaxK][D],
                                     const Mat<D> (&Ss)[kMaxK], float (&mf)[D], Mat<D>& Sf) {
#pragma clang fp contract(off)
  if (fusion == 1) {
    // mu_f = sum_k (w_k / (sum_k w_k + 1e-9)) mu_k ; Sigma_f = sum_k (w_k w_k^T) (.) Sigma_k
    float wsum[D];
#pragma unroll
    for (int i = 0; i < D; ++i) wsum[i] = 0.f;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      if (k >= K) break;
#pragma unroll
      for (int i = 0; i < D; ++i) wsum[i] += w[k][i];
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
      mf[i] = 0.f;
#pragma unroll
      for (int j = 0; j < D; ++j) Sf.a[i][j] = 0.f;
    }
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      if (k >= K) break;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        mf[i] = __builtin_fmaf(w[k][i] / (wsum[i] + 1e-9f), mus[k][i], mf[i]);
#pragma unroll
        for (int j = 0; j < D; ++j) Sf.a[i][j] = __builtin_fmaf(w[k][i] * w[k][j], Ss[k].a[i][j], Sf.a[i][j]);
      }
    }
  } else if (fusion == 2) {
    // P_k = (Sigma_k + 1e-9)^-1 ; Sigma_f = (sum_k P_k + 1e-9)^-1 ; mu_f = Sigma_f sum_k P_k mu_k
    // In DOUBLE: the posteriors of a well-observed state are ill-conditioned (condition 1e2 .. 1e3 is common), their
    // precisions are summed and inverted again, and mu_f is a product of nearly cancelling factors.  In float32 the K + 1
    // inversions alone put mu_f up to 4e-3 off (four times what torch's fp32 LU form loses on the same rows).  What is left
    // in double is the rounding of the float32 posteriors themselves, amplified by their condition: under 4e-5 with
    // predict_correct's product form of I - G.  5 d x d inversions per trajectory: no time next to the launch.
    Mat<D, double> Psum;
    double info[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
      info[i] = 0.0;
#pragma unroll
      for (int j = 0; j < D; ++j) Psum.a[i][j] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
      if (k >= K) break;
      Mat<D, double> t;
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) t.a[i][j] = static_cast<double>(Ss[k].a[i][j]) + 1e-9;
      const Mat<D, double> P = inverse<D>(t);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
          s = fma_(P.a[i][j], static_cast<double>(mus[k][j]), s);
          Psum.a[i][j] += P.a[i][j];
        }
        info[i] += s;
      }
    }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) Psum.a[i][j] += 1e-9;
    const Mat<D, double> Sfd = inverse<D>(Psum);
#pragma unroll
    for (int i = 0; i < D; ++i) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        s = fma_(Sfd.a[i][j], info[j], s);
        Sf.a[i][j] = static_cast<float>(Sfd.a[i][j]);
      }
      mf[i] = static_cast<float>(s);
    }
  }
}

}  // namespace mmf_ekf
