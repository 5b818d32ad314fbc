// Small Hermitian linear algebra for MultichannelISNMF (csrc/assx_mnmf.hip), its covariance-domain form
// (csrc/assx_covnmf.hip) and IPSDTA (csrc/assx_ipsdta.hip), one thread per matrix, float64.
//
// Matrices are M x M complex, held as separate real and imaginary arrays (re[i][j], im[i][j]) with static indices, so
// they live in VGPRs.  Hermitian inputs are read from their lower triangle only.  Everything here is plain arithmetic
// (__host__ __device__): the same code can be compiled for the host and checked against NumPy.
//   herm_cholesky   A = L L^H, L lower with a real positive diagonal; false unless every pivot is > 0 and finite
//   tri_inverse     L^{-1} of a lower-triangular L
//   herm_jacobi     eigenvalues and eigenvectors of a Hermitian C by cyclic Jacobi rotations
//   herm_sqrt_psd   (C)^{1/2} of a Hermitian C through herm_jacobi, eigenvalues clamped at 0
//   herm_riccati    the positive-definite solution of H A H = B: the matrix geometric mean L^{-H} (L^H B L)^{1/2} L^{-1}
//   unpack_herm     a Hermitian matrix from its M^2 packed reals
#pragma once
#include <math.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

namespace assx {
namespace herm {

template <int M>
struct Mat {
  double re[M][M], im[M][M];
};

template <int M>
__host__ __device__ inline void set_zero(Mat<M>& A) {
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) A.re[i][j] = 0.0, A.im[i][j] = 0.0;
}

// fill the strict upper triangle from the lower one (A Hermitian)
template <int M>
__host__ __device__ inline void mirror_lower(Mat<M>& A) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    A.im[i][i] = 0.0;
#pragma unroll
    for (int j = i + 1; j < M; ++j) A.re[i][j] = A.re[j][i], A.im[i][j] = -A.im[j][i];
  }
}

// in place: the lower triangle of A becomes L (A = L L^H); the strict upper triangle is not read and is left as is
template <int M>
__host__ __device__ inline bool herm_cholesky(Mat<M>& A) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    double d = A.re[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= A.re[j][k] * A.re[j][k] + A.im[j][k] * A.im[j][k];
    ok = ok && d > 0.0 && d < INFINITY;
    const double l = sqrt(d > 0.0 ? d : 1.0);
    const double il = 1.0 / l;
    A.re[j][j] = l;
    A.im[j][j] = 0.0;
#pragma unroll
    for (int i = j + 1; i < M; ++i) {
      double sr = A.re[i][j], si = A.im[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) {  // - L_ik conj(L_jk)
        sr -= A.re[i][k] * A.re[j][k] + A.im[i][k] * A.im[j][k];
        si -= A.im[i][k] * A.re[j][k] - A.re[i][k] * A.im[j][k];
      }
      A.re[i][j] = sr * il;
      A.im[i][j] = si * il;
    }
  }
  return ok;
}

// Li = L^{-1} (lower triangular; the strict upper triangle of Li is set to 0)
template <int M>
__host__ __device__ inline void tri_inverse(const Mat<M>& L, Mat<M>& Li) {
#pragma unroll
  for (int j = 0; j < M; ++j) {
#pragma unroll
    for (int i = 0; i < j; ++i) Li.re[i][j] = 0.0, Li.im[i][j] = 0.0;
    Li.re[j][j] = 1.0 / L.re[j][j];
    Li.im[j][j] = 0.0;
#pragma unroll
    for (int i = j + 1; i < M; ++i) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) {  // sum L_ik Li_kj
        sr += L.re[i][k] * Li.re[k][j] - L.im[i][k] * Li.im[k][j];
        si += L.re[i][k] * Li.im[k][j] + L.im[i][k] * Li.re[k][j];
      }
      const double il = 1.0 / L.re[i][i];
      Li.re[i][j] = -sr * il;
      Li.im[i][j] = -si * il;
    }
  }
}

// C = A B (full)
template <int M>
__host__ __device__ inline void matmul(const Mat<M>& A, const Mat<M>& B, Mat<M>& C) {
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) {
        sr += A.re[i][k] * B.re[k][j] - A.im[i][k] * B.im[k][j];
        si += A.re[i][k] * B.im[k][j] + A.im[i][k] * B.re[k][j];
      }
      C.re[i][j] = sr, C.im[i][j] = si;
    }
}

// C = A^H B (full)
template <int M>
__host__ __device__ inline void matmul_ah(const Mat<M>& A, const Mat<M>& B, Mat<M>& C) {
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) {
        sr += A.re[k][i] * B.re[k][j] + A.im[k][i] * B.im[k][j];
        si += A.re[k][i] * B.im[k][j] - A.im[k][i] * B.re[k][j];
      }
      C.re[i][j] = sr, C.im[i][j] = si;
    }
}

// (A + A^H) / 2 in place
template <int M>
__host__ __device__ inline void hermitize(Mat<M>& A) {
#pragma unroll
  for (int i = 0; i < M; ++i) {
    A.im[i][i] = 0.0;
#pragma unroll
    for (int j = i + 1; j < M; ++j) {
      const double r = 0.5 * (A.re[i][j] + A.re[j][i]), m = 0.5 * (A.im[i][j] - A.im[j][i]);
      A.re[i][j] = r, A.im[i][j] = m, A.re[j][i] = r, A.im[j][i] = -m;
    }
  }
}

// The eigendecomposition C = U diag(w) U^H of a Hermitian C (full storage) by cyclic Jacobi: on return the diagonal of C
// holds w (in no particular order) and the columns of U the eigenvectors.  At most 12 sweeps; a sweep stops the iteration
// once the off-diagonal mass is below 1e-32 of the squared Frobenius norm.  Returns false when the sweeps ran out (or the
// mass is not a number).  Used by herm_sqrt_psd below and by the PCA basis of csrc/assx_beamform.hip.
template <int M>
__host__ __device__ inline bool herm_jacobi(Mat<M>& C, Mat<M>& U) {
  bool done = false;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) U.re[i][j] = i == j ? 1.0 : 0.0, U.im[i][j] = 0.0;
  for (int sweep = 0; sweep < 12; ++sweep) {
    double off = 0.0, tot = 0.0;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      tot += C.re[i][i] * C.re[i][i];
#pragma unroll
      for (int j = 0; j < i; ++j) off += C.re[i][j] * C.re[i][j] + C.im[i][j] * C.im[i][j];
    }
    if (!(off > 1e-32 * (tot + 2.0 * off))) {
      done = off == off;
      break;
    }
#pragma unroll
    for (int p = 0; p < M - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < M; ++q) {
        const double ar = C.re[p][q], ai = C.im[p][q];
        const double g = sqrt(ar * ar + ai * ai);
        if (g == 0.0) continue;
        const double er = ar / g, ei = ai / g;  // e = a_pq / |a_pq|
        const double theta = (C.re[q][q] - C.re[p][p]) / (2.0 * g);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        // J (columns p, q): J_pp = c, J_pq = s, J_qp = -s conj(e), J_qq = c conj(e).  C <- C J, U <- U J
#pragma unroll
        for (int k = 0; k < M; ++k) {
          const double pr = C.re[k][p], pi = C.im[k][p], qr = C.re[k][q], qi = C.im[k][q];
          // conj(e) a_kq
          const double wr = er * qr + ei * qi, wi = er * qi - ei * qr;
          C.re[k][p] = c * pr - s * wr, C.im[k][p] = c * pi - s * wi;
          C.re[k][q] = s * pr + c * wr, C.im[k][q] = s * pi + c * wi;
          const double upr = U.re[k][p], upi = U.im[k][p], uqr = U.re[k][q], uqi = U.im[k][q];
          const double vr = er * uqr + ei * uqi, vi = er * uqi - ei * uqr;
          U.re[k][p] = c * upr - s * vr, U.im[k][p] = c * upi - s * vi;
          U.re[k][q] = s * upr + c * vr, U.im[k][q] = s * upi + c * vi;
        }
        // C <- J^H C: row p = c row_p - s e row_q, row q = s row_p + c e row_q
#pragma unroll
        for (int k = 0; k < M; ++k) {
          const double pr = C.re[p][k], pi = C.im[p][k], qr = C.re[q][k], qi = C.im[q][k];
          const double wr = er * qr - ei * qi, wi = er * qi + ei * qr;  // e a_qk
          C.re[p][k] = c * pr - s * wr, C.im[p][k] = c * pi - s * wi;
          C.re[q][k] = s * pr + c * wr, C.im[q][k] = s * pi + c * wi;
        }
        C.re[p][q] = 0.0, C.im[p][q] = 0.0, C.re[q][p] = 0.0, C.im[q][p] = 0.0;
        C.im[p][p] = 0.0, C.im[q][q] = 0.0;
      }
  }
  return done;
}

// S = C^{1/2} for a Hermitian C (full storage): C = U diag(w) U^H by herm_jacobi, S = U diag(sqrt(max(w, 0))) U^H.
// C is destroyed.
template <int M>
__host__ __device__ inline void herm_sqrt_psd(Mat<M>& C, Mat<M>& S) {
  Mat<M>& U = S;  // eigenvectors first, then overwritten by the result
  herm_jacobi(C, U);
  double w[M];
#pragma unroll
  for (int i = 0; i < M; ++i) w[i] = C.re[i][i] > 0.0 ? sqrt(C.re[i][i]) : 0.0;
  // S = U diag(w) U^H, computed into C (free now), then copied into S (= U)
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int k = 0; k < M; ++k) {  // U_ik w_k conj(U_jk)
        sr += w[k] * (U.re[i][k] * U.re[j][k] + U.im[i][k] * U.im[j][k]);
        si += w[k] * (U.im[i][k] * U.re[j][k] - U.re[i][k] * U.im[j][k]);
      }
      C.re[i][j] = sr, C.im[i][j] = si;
    }
  S = C;
}

// H A H = B for Hermitian A (positive definite) and B (positive semi-definite), both in full storage: H = L^{-H}
// (L^H B L)^{1/2} L^{-1} with A = L L^H, then (H + H^H) / 2.  Returns 0, 1 when A is exactly zero (H = 0: the rule
// that reproduces the reference on a bin whose weights are all zero), or -1 when the Cholesky of A fails (H = 0).
// A and B are destroyed.
template <int M>
__host__ __device__ inline int herm_riccati(Mat<M>& A, Mat<M>& B, Mat<M>& H) {
  bool zero = true;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) zero = zero && A.re[i][j] == 0.0 && A.im[i][j] == 0.0;
  if (zero) {
    set_zero(H);
    return 1;
  }
  if (!herm_cholesky(A)) {
    set_zero(H);
    return -1;
  }
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = i + 1; j < M; ++j) A.re[i][j] = 0.0, A.im[i][j] = 0.0;  // A is L now
  matmul_ah(A, B, H);  // L^H B
  matmul(H, A, B);     // L^H B L
  hermitize(B);
  herm_sqrt_psd(B, H);  // S
  Mat<M> Li;
  tri_inverse(A, Li);
  matmul(H, Li, A);      // S L^{-1}
  matmul_ah(Li, A, H);   // L^{-H} S L^{-1}
  hermitize(H);
  return 0;
}

// A Hermitian matrix packed into M^2 reals (entry (i, j) holds Re A_ij for i >= j and Im A_ji for i < j), to full storage
template <int M>
__host__ __device__ inline void unpack_herm(const double* p, Mat<M>& A) {
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      A.re[i][j] = p[i * M + j];
      A.im[i][j] = i == j ? 0.0 : p[j * M + i];
    }
  mirror_lower(A);
}

}  // namespace herm
}  // namespace assx
