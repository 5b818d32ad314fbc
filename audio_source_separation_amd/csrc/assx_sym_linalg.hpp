// Workgroup-cooperative dense linear algebra for real symmetric n x n matrices, run-time 1 <= n <= 64, float64, the
// matrices in LDS.  The register-resident routines of assx_herm_linalg.hpp stop at M = 8; these are for the bins x bins
// matrices of PSDTF (and of IPSDTA later): one workgroup of 256 threads per matrix, every routine called by ALL threads
// of the workgroup with workgroup-uniform arguments.
//
// A matrix is a buffer of MAT doubles, element (i, j) at [i * LD + j] with LD = 65: a column walk (stride 65 doubles) hits
// every LDS bank once, like a row walk.  A 64 x 64 matrix is 33 KB; a CU has 160 KB of LDS, so a kernel may hold four.
//
//   chol        in-place lower Cholesky, left-looking, one thread per row; a pivot at or below the caller's floor is
//               replaced by 1 (the loop finishes without NaN) and reported
//   tri_inv     inverse of a lower triangle, one thread per column (forward substitution)
//   ata         Li^T Li, exactly symmetric (both halves sum the same products in the same order)
//   spd_inv     the three above: A^-1 of a positive definite A
//   matmul      op(A) op(B), op = identity or transpose, a strip of 4 rows per thread
//   jacobi      eigenvalues (and vectors) by Jacobi rotations in the parallel round-robin order: n / 2 disjoint pairs
//               rotate at once, n - 1 steps make a sweep.  A rotation is applied 2 x 2 block by 2 x 2 block, only the
//               blocks above the diagonal computed and mirrored, so the matrix stays exactly symmetric.  Before every
//               sweep the off-diagonal mass is tested by the rule of herm_sqrt_psd (stop at 1e-32 of the total); at most
//               SWEEPS sweeps, "not converged" is reported
//   to_psd      symmetrise, subtract min(lambda_min, 0) I, add eps trace I.  A Cholesky factorisation with every pivot
//               above 2^-40 of the largest diagonal entry proves lambda_min > 0, the shift is then the eigen path's
//               (delta = 0) without an eigen-solve; otherwise lambda_min comes from jacobi
//
// Every sum has a fixed order (a thread's own stride, a wave's butterfly, the waves in index order): the result of a
// routine depends on its input alone.
#pragma once
#include "assx_common.hpp"
#include "assx_factor_common.hpp"

namespace assx {
namespace sl {

constexpr int NMAX = 64;
constexpr int LD = NMAX + 1;
constexpr int MAT = NMAX * LD;
constexpr int BLK = 256;
constexpr int NW = BLK / WAVE;
constexpr int SWEEPS = 30;
constexpr int ST_SINGULAR = 1;       // a matrix that had to be positive definite was not (assx.h: ASSX_STATUS_SINGULAR)
constexpr int ST_NOT_CONVERGED = 4;  // jacobi ran out of sweeps

struct Scratch {
  double red[NW];
  double cs[NMAX / 2], sn[NMAX / 2];
  int pp[NMAX / 2], qq[NMAX / 2];
  double bc[2];
  int flag;
};

__device__ __forceinline__ void copy(const double* A, double* W, int n) {
  for (int e = threadIdx.x; e < n * n; e += BLK) W[(e / n) * LD + e % n] = A[(e / n) * LD + e % n];
  __syncthreads();
}

// n x n contiguous in global memory <-> LDS
__device__ __forceinline__ void load(const double* __restrict__ G, double* A, int n) {
  for (int e = threadIdx.x; e < n * n; e += BLK) A[(e / n) * LD + e % n] = G[e];
  __syncthreads();
}

__device__ __forceinline__ void store(const double* A, double* __restrict__ G, int n) {
  for (int e = threadIdx.x; e < n * n; e += BLK) G[e] = A[(e / n) * LD + e % n];
}

__device__ __forceinline__ void symmetrize(double* A, int n) {
  for (int e = threadIdx.x; e < n * n; e += BLK) {
    const int i = e / n, j = e % n;
    if (i < j) {
      const double v = (A[i * LD + j] + A[j * LD + i]) / 2;
      A[i * LD + j] = v;
      A[j * LD + i] = v;
    }
  }
  __syncthreads();
}

__device__ __forceinline__ bool chol(double* A, int n, double pivot_floor, Scratch& s) {
  const int i = threadIdx.x;
  __syncthreads();
  if (i == 0) s.flag = 0;
  for (int j = 0; j < n; ++j) {
    __syncthreads();
    if (i >= j && i < n) {
      double acc = A[i * LD + j];
      for (int k = 0; k < j; ++k) acc -= A[i * LD + k] * A[j * LD + k];
      A[i * LD + j] = acc;
    }
    __syncthreads();
    double d = A[j * LD + j];
    if (!(d > pivot_floor)) {  // also NaN
      d = 1.0;
      if (i == 0) s.flag = 1;
    }
    const double r = sqrt(d);
    __syncthreads();
    if (i == j)
      A[j * LD + j] = r;
    else if (i > j && i < n)
      A[i * LD + j] /= r;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n * n; e += BLK)
    if (e % n > e / n) A[(e / n) * LD + e % n] = 0;
  __syncthreads();
  return s.flag == 0;
}

// Li (all n x n entries written) = L^-1
__device__ __forceinline__ void tri_inv(const double* L, double* Li, int n) {
  const int j = threadIdx.x;
  if (j < n) {
    for (int i = 0; i < j; ++i) Li[i * LD + j] = 0;
    Li[j * LD + j] = 1.0 / L[j * LD + j];
    for (int i = j + 1; i < n; ++i) {
      double acc = 0;
      for (int k = j; k < i; ++k) acc += L[i * LD + k] * Li[k * LD + j];
      Li[i * LD + j] = -acc / L[i * LD + i];
    }
  }
  __syncthreads();
}

// Out = Li^T Li for a lower triangular Li
__device__ __forceinline__ void ata(const double* Li, double* Out, int n) {
  for (int e = threadIdx.x; e < n * n; e += BLK) {
    const int i = e / n, j = e % n;
    double acc = 0;
    for (int k = max(i, j); k < n; ++k) acc += Li[k * LD + i] * Li[k * LD + j];
    Out[i * LD + j] = acc;
  }
  __syncthreads();
}

// A <- A^-1 for a positive definite A; W, W2 scratch.  false: A was not positive definite (A is then meaningless but finite
// wherever its input was).
__device__ __forceinline__ bool spd_inv(double* A, double* W, double* W2, int n, Scratch& s) {
  copy(A, W, n);
  const bool ok = chol(W, n, 0.0, s);
  tri_inv(W, W2, n);
  ata(W2, A, n);
  return ok;
}

// C = op(A) op(B); C is neither A nor B
template <bool TA, bool TB>
__device__ __forceinline__ void matmul(const double* A, const double* B, double* C, int n) {
  const int groups = (n + 3) / 4;
  for (int w = threadIdx.x; w < groups * n; w += BLK) {
    const int j = w % n, i0 = (w / n) * 4;
    int r[4];
    double acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = 0, r[u] = min(i0 + u, n - 1);
    for (int k = 0; k < n; ++k) {
      const double b = TB ? B[j * LD + k] : B[k * LD + j];
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] += (TA ? A[k * LD + r[u]] : A[r[u] * LD + k]) * b;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + u < n) C[(i0 + u) * LD + j] = acc[u];
  }
  __syncthreads();
}

// sum_ij A[i][j] G[j][i], G n x n contiguous in global memory, one WAVE: every lane returns it
__device__ __forceinline__ double wave_trace_prod(const double* A, const double* __restrict__ G, int n) {
  double acc = 0;
  for (int e = threadIdx.x & (WAVE - 1); e < n * n; e += WAVE) acc += G[e] * A[(e % n) * LD + e / n];
  for (int o = WAVE / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  return acc;
}

// The eigenvalues of the symmetric A end on its diagonal (unsorted; the rest of A is destroyed); Vv != nullptr receives
// the eigenvectors as columns.  An odd n is padded with a zero row and column, which no rotation changes.  false: not
// converged after SWEEPS sweeps, or a NaN.
__device__ __forceinline__ bool jacobi(double* A, double* Vv, int n, Scratch& s) {
  const int tid = threadIdx.x;
  const int m = (n + 1) & ~1, np = m / 2;
  if (m > n) {
    for (int e = tid; e < m; e += BLK) A[n * LD + e] = 0, A[e * LD + n] = 0;
  }
  if (Vv)
    for (int e = tid; e < m * m; e += BLK) Vv[(e / m) * LD + e % m] = (e / m == e % m) ? 1.0 : 0.0;
  __syncthreads();
  bool conv = false;
  for (int sweep = 0; sweep <= SWEEPS; ++sweep) {
    double off = 0, dg = 0;
    for (int e = tid; e < n * n; e += BLK) {
      const int i = e / n, j = e % n;
      const double v = A[i * LD + j];
      if (j < i)
        off += v * v;
      else if (i == j)
        dg += v * v;
    }
    off = mf::block_sum_all(off, s.red);
    dg = mf::block_sum_all(dg, s.red);
    conv = off <= 1e-32 * (dg + 2.0 * off);
    if (conv || off != off || sweep == SWEEPS) break;
    for (int r = 0; r < m - 1; ++r) {
      if (tid < np) {
        const int a = tid == 0 ? r : (r + tid) % (m - 1), b = tid == 0 ? m - 1 : (r - tid + (m - 1)) % (m - 1);
        const int p = min(a, b), q = max(a, b);
        double c = 1, sn = 0;
        const double apq = A[p * LD + q];
        if (apq != 0.0) {
          const double app = A[p * LD + p], aqq = A[q * LD + q];
          const double th = (aqq - app) / (2 * apq);
          const double t = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1));
          c = 1 / sqrt(t * t + 1);
          sn = t * c;
          A[p * LD + p] = app - t * apq;
          A[q * LD + q] = aqq + t * apq;
          A[p * LD + q] = 0;
          A[q * LD + p] = 0;
        }
        s.pp[tid] = p, s.qq[tid] = q, s.cs[tid] = c, s.sn[tid] = sn;
      }
      __syncthreads();
      for (int w = tid; w < np * np; w += BLK) {
        const int P = w / np, Q = w % np;
        if (P >= Q) continue;
        const double c1 = s.cs[P], s1 = s.sn[P], c2 = s.cs[Q], s2 = s.sn[Q];
        if (s1 == 0.0 && s2 == 0.0) continue;
        const int p1 = s.pp[P], q1 = s.qq[P], p2 = s.pp[Q], q2 = s.qq[Q];
        const double a = A[p1 * LD + p2], b = A[p1 * LD + q2], c = A[q1 * LD + p2], d = A[q1 * LD + q2];
        // columns by the rotation of pair Q, then rows by that of pair P
        const double a1 = c2 * a - s2 * b, b1 = s2 * a + c2 * b, e1 = c2 * c - s2 * d, d1 = s2 * c + c2 * d;
        const double a2 = c1 * a1 - s1 * e1, e2 = s1 * a1 + c1 * e1, b2 = c1 * b1 - s1 * d1, d2 = s1 * b1 + c1 * d1;
        A[p1 * LD + p2] = a2, A[p2 * LD + p1] = a2;
        A[p1 * LD + q2] = b2, A[q2 * LD + p1] = b2;
        A[q1 * LD + p2] = e2, A[p2 * LD + q1] = e2;
        A[q1 * LD + q2] = d2, A[q2 * LD + q1] = d2;
      }
      if (Vv) {
        for (int w = tid; w < np * m; w += BLK) {
          const int P = w / m, i = w % m;
          const double c = s.cs[P], sn = s.sn[P];
          if (sn == 0.0) continue;
          const int p = s.pp[P], q = s.qq[P];
          const double x = Vv[i * LD + p], y = Vv[i * LD + q];
          Vv[i * LD + p] = c * x - sn * y;
          Vv[i * LD + q] = sn * x + c * y;
        }
      }
      __syncthreads();
    }
  }
  return conv;
}

// A <- (A + A^T) / 2 - min(lambda_min, 0) I + eps trace I; W scratch.  Returns 0 or ST_NOT_CONVERGED.
__device__ __forceinline__ int to_psd(double* A, double* W, int n, double eps, Scratch& s) {
  symmetrize(A, n);
  copy(A, W, n);
  if (threadIdx.x == 0) {
    double tr = 0, mx = 0;
    for (int i = 0; i < n; ++i) tr += A[i * LD + i], mx = fmax(mx, A[i * LD + i]);
    s.bc[0] = tr, s.bc[1] = mx;
  }
  __syncthreads();
  const double tr = s.bc[0], mx = s.bc[1];
  int st = 0;
  double delta = 0;
  if (!chol(W, n, ldexp(mx, -40), s)) {
    copy(A, W, n);
    if (!jacobi(W, nullptr, n, s)) st = ST_NOT_CONVERGED;
    if (threadIdx.x == 0) {
      double mn = 0;
      for (int i = 0; i < n; ++i) mn = fmin(mn, W[i * LD + i]);
      s.bc[0] = mn;
    }
    __syncthreads();
    delta = s.bc[0];
  }
  if (threadIdx.x < n) A[threadIdx.x * LD + threadIdx.x] = (A[threadIdx.x * LD + threadIdx.x] - delta) + eps * tr;
  __syncthreads();
  return st;
}

}  // namespace sl
}  // namespace assx
