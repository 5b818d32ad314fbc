// GaussIPSDTA, Kondo's block-diagonal independent positive semidefinite tensor analysis (src/bss/ipsdta.py:510-688,
// 820-1081) on MI355X: MM source model, vectorwise coordinate descent (VCD) spatial model, loss.  float64 / complex128.
//
// The n_bins bins are cut into n_blocks blocks: the first nlow = n_blocks - n_bins % n_blocks of nn = n_bins / n_blocks
// bins, the rest of nn + 1.  Block b has size nb, first bin f0 and packed offset off (the nb x nb matrices of all blocks
// laid end to end, P = sum nb^2 entries).  State: X (M,F,T) complex input, W (F,M,M) complex demixing filter,
// U (N,K,P) complex packed Hermitian bases, H (N,K,T) activation, N = M.  psd(A) = (A + A^H)/2 - min(lambda_min, 0) I +
// eps tr I follows every matrix the reference applies to_PSD to.  With y = W x the block's output,
//
//   ip_model_kernel<NB, MODE>  one thread per (source, block, frame), matrices in registers (assx_herm_linalg.hpp):
//                     R = psd(sum_k H U_k), Ri = psd(R^-1) (Cholesky); BASIS: Ri and Z = Ri (y y^H + eps I) Ri go to the
//                     workspace as (N,P,T), frames fastest; ACT: Ri and G = Ri psd(y y^H + eps I) Ri; SPATIAL: Ri;
//                     LOSS: y^H Ri y + sum log max(lambda(R), eps) per (source, block, frame)
//   ip_contract_kernel  S_k = sum_t H Z, T_k = sum_t H Ri: one wave per (source, entry), its lanes stride the frames, 8
//                     bases at a time, a butterfly adds the lanes
//   ip_basis_kernel<NB>  one thread per (source, basis, block): U <- psd(U S^1/2 psd(psd(psd(S^1/2 U T U S^1/2)^1/2)^-1)
//                     S^1/2 U), S^1/2 = psd of the Jacobi square root
//   ip_act_kernel     one thread per (source, basis, frame): num = sum_e Re(U_k[e] conj(G[e])), den likewise with Ri, in
//                     entry order; H <- H sqrt(max(num, 0) / max(den, eps))
//   ip_norm_kernel    one workgroup per (source, basis): U_k /= tr U_k, H[k,:] *= tr U_k
//   ip_q_kernel       Q[n,f] = mean_t (Ri)_ii(t) (x x^H + eps |x|^2 I), one wave per (source, bin), one lane per entry,
//                     the frames in index order; ip_qpsd_kernel<M> applies psd.  Q depends on neither W nor the sweep
//   ip_sweep_kernel   one workgroup per block, one VCD sweep: sources in order, positions of the block in order
//                     (Gauss-Seidel); gamma by all threads over the frames, the two M x M solves and the row update by
//                     thread 0; the block's rows of W live in LDS
//   ip_loss_kernel    one workgroup: the per-(source, block, frame) terms in index order and -2 T log|det W_f| (LU)
//
// The psd() of x x^H takes min(lambda_min, 0) as 0 (lambda_min of a rank-one matrix is rounding noise), and so does the one
// of y y^H + eps I.  A block that is not positive definite where the method inverts it, or a singular solve, sets
// ASSX_STATUS_SINGULAR; the kernels finish either way.  No float atomics, no partition that depends on anything but the
// shapes, every sum in a fixed order.
//
// tIPSDTA, the Student-t model of the same paper series (src/bss/ipsdta.py:1083-1762), shares the model, contraction, basis,
// activation and normalisation kernels (the template flag TD switches its weights in; the Gauss instantiations are
// unchanged) and adds ip_pi_kernel, ip_tq_kernel, ip_tstep_kernel and ip_tloss_kernel, described where they are defined.
// The host drivers are templates on the same flag and read one workspace layout (ip_layout: a field the model does not use
// has size 0); only the spatial updates, two different algorithms, are two functions.
#include "assx_common.hpp"
#include "assx_factor_common.hpp"
#include "assx_herm_linalg.hpp"

using namespace assx;
using herm::Mat;

namespace {

constexpr int BLK = 256;
constexpr int NW = BLK / WAVE;
constexpr int NBMAX = 8;
constexpr int MMAX = 8;
constexpr int KMAX = 64;
constexpr int KC = 8;
constexpr int ST_SINGULAR = 1;

typedef double2 cx;

struct IpGeo {
  int M, F, T, K, nblk, nn, nlow, P;
};

struct IpBlock {
  int nb, f0, off;
};

__host__ __device__ inline IpBlock ip_block(const IpGeo& g, int b) {
  IpBlock r;
  if (b < g.nlow) {
    r.nb = g.nn, r.f0 = b * g.nn, r.off = b * g.nn * g.nn;
  } else {
    const int h = b - g.nlow, n1 = g.nn + 1;
    r.nb = n1, r.f0 = g.nlow * g.nn + h * n1, r.off = g.nlow * g.nn * g.nn + h * n1 * n1;
  }
  return r;
}

// false outside the envelope of include/assx.h (f10)
inline bool ip_geo(int M, int F, int T, int K, int n_blocks, IpGeo& g) {
  if (M < 2 || M > MMAX || K < 1 || K > KMAX || T < 1 || F < 1 || n_blocks < 1 || n_blocks > F) return false;
  const int nn = F / n_blocks, rem = F % n_blocks;
  if (nn + (rem > 0) > NBMAX || F > (1 << 20) || T > (1 << 24)) return false;
  g.M = M, g.F = F, g.T = T, g.K = K, g.nblk = n_blocks, g.nn = nn, g.nlow = n_blocks - rem;
  g.P = g.nlow * nn * nn + rem * (nn + 1) * (nn + 1);
  // one thread per (source, block, frame): fewer than 2^31 of them
  return (long long)M * n_blocks * T < (1LL << 31) && (long long)M * g.P * T < (1LL << 40);
}

struct IpLayout {
  size_t ri, zz, part, q, qb, lossp, pi, total;
};

// ri, zz: (N,P,T) complex; part: S and T (N,2,K,P) complex; lossp: (N,n_blocks,T) double.  The Gauss model adds q
// (N,F,M,M) complex, the Student-t model (td) qb (N,n_blocks,T) and pi (N,T) double.  A field the model does not use has
// size 0
IpLayout ip_layout(const IpGeo& g, bool td) {
  const size_t c = sizeof(cx), N = g.M, terms = N * g.nblk * g.T * sizeof(double);
  mf::Carve cv(1);
  IpLayout L;
  L.ri = cv.take(N * g.P * g.T * c);
  L.zz = cv.take(N * g.P * g.T * c);
  L.part = cv.take(N * 2 * g.K * g.P * c);
  L.q = cv.take(td ? 0 : N * g.F * g.M * g.M * c);
  L.qb = cv.take(td ? terms : 0);
  L.lossp = cv.take(terms);
  L.pi = cv.take(td ? N * g.T * sizeof(double) : 0);
  L.total = cv.total();
  return L;
}

// Complex arithmetic on double2, not the Cx<double> helpers of assx_common.hpp: with arrays of the aligned struct the
// sweep, step and loss kernels reserve more scratch than with the native vector type.  cdiv (unscaled) and csqrt_ (half
// sums) have no counterpart there in any case.
__device__ __forceinline__ cx cmul(cx a, cx b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ cx cmulc(cx a, cx b) {  // a conj(b)
  return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y);
}
__device__ __forceinline__ cx cdiv(cx a, cx b) {
  const double d = b.x * b.x + b.y * b.y;
  return make_double2((a.x * b.x + a.y * b.y) / d, (a.y * b.x - a.x * b.y) / d);
}
// the principal square root
__device__ __forceinline__ cx csqrt_(cx z) {
  const double r = hypot(z.x, z.y);
  if (r == 0.0) return make_double2(0.0, 0.0);
  if (z.x >= 0.0) {
    const double re = sqrt(0.5 * (r + z.x));
    return make_double2(re, z.y / (2.0 * re));
  }
  const double im = copysign(sqrt(0.5 * (r - z.x)), z.y);
  return make_double2(z.y / (2.0 * im), im);
}

// the eigenvalues of the Hermitian C (full storage, destroyed) by the cyclic Jacobi rotations of herm::herm_sqrt_psd
template <int N>
__device__ inline void ip_eigvals(Mat<N>& C, double (&w)[N]) {
  for (int sweep = 0; sweep < 12; ++sweep) {
    double off = 0.0, tot = 0.0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      tot += C.re[i][i] * C.re[i][i];
#pragma unroll
      for (int j = 0; j < i; ++j) off += C.re[i][j] * C.re[i][j] + C.im[i][j] * C.im[i][j];
    }
    if (!(off > 1e-32 * (tot + 2.0 * off))) break;
#pragma unroll
    for (int p = 0; p < N - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double ar = C.re[p][q], ai = C.im[p][q];
        const double g = sqrt(ar * ar + ai * ai);
        if (g == 0.0) continue;
        const double er = ar / g, ei = ai / g;
        const double theta = (C.re[q][q] - C.re[p][p]) / (2.0 * g);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double pr = C.re[k][p], pi = C.im[k][p], qr = C.re[k][q], qi = C.im[k][q];
          const double wr = er * qr + ei * qi, wi = er * qi - ei * qr;
          C.re[k][p] = c * pr - s * wr, C.im[k][p] = c * pi - s * wi;
          C.re[k][q] = s * pr + c * wr, C.im[k][q] = s * pi + c * wi;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double pr = C.re[p][k], pi = C.im[p][k], qr = C.re[q][k], qi = C.im[q][k];
          const double wr = er * qr - ei * qi, wi = er * qi + ei * qr;
          C.re[p][k] = c * pr - s * wr, C.im[p][k] = c * pi - s * wi;
          C.re[q][k] = s * pr + c * wr, C.im[q][k] = s * pi + c * wi;
        }
        C.re[p][q] = 0.0, C.im[p][q] = 0.0, C.re[q][p] = 0.0, C.im[q][p] = 0.0;
        C.im[p][p] = 0.0, C.im[q][q] = 0.0;
      }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = C.re[i][i];
}

// A <- (A + A^H)/2 - min(lambda_min, 0) I + eps tr I.  A Cholesky factorisation with every pivot above 2^-40 of the
// largest diagonal entry proves lambda_min > 0 (the shortcut of sl::to_psd); otherwise lambda_min comes from Jacobi.
template <int N>
__device__ inline void ip_psd(Mat<N>& A, double eps) {
  herm::hermitize(A);
  double tr = 0.0, mx = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) tr += A.re[i][i], mx = fmax(mx, A.re[i][i]);
  Mat<N> L = A;
  bool ok = herm::herm_cholesky(L);
  const double fl = ldexp(mx, -40);
#pragma unroll
  for (int i = 0; i < N; ++i) ok = ok && L.re[i][i] * L.re[i][i] > fl;
  double delta = 0.0;
  if (!ok) {
    L = A;
    double w[N];
    ip_eigvals(L, w);
#pragma unroll
    for (int i = 0; i < N; ++i) delta = fmin(delta, w[i]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) A.re[i][i] = (A.re[i][i] - delta) + eps * tr;
}

// Ai = A^-1 of a Hermitian positive definite A (destroyed) by Cholesky; false when a pivot is not positive
template <int N>
__device__ inline bool ip_inv(Mat<N>& A, Mat<N>& Ai) {
  const bool ok = herm::herm_cholesky(A);
  Mat<N> Li;
  herm::tri_inverse(A, Li);
  herm::matmul_ah(Li, Li, Ai);
  return ok;
}

template <int N>
__device__ inline void ip_load(const cx* __restrict__ p, Mat<N>& A) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const cx v = p[i * N + j];
      A.re[i][j] = v.x, A.im[i][j] = v.y;
    }
}

template <int N>
__device__ inline void ip_store(const Mat<N>& A, cx* __restrict__ p) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) p[i * N + j] = make_double2(A.re[i][j], A.im[i][j]);
}

// entry e of a frame-fastest (N,P,T) array
template <int N>
__device__ inline void ip_store_t(const Mat<N>& A, cx* __restrict__ p, size_t T) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) p[(size_t)(i * N + j) * T] = make_double2(A.re[i][j], A.im[i][j]);
}

__device__ __forceinline__ void ip_flag(int32_t* status, bool bad) {
  if (bad && status) atomicOr(status, ST_SINGULAR);
}

enum { MODE_BASIS = 0, MODE_ACT = 1, MODE_SPATIAL = 2, MODE_LOSS = 3 };

// blocks b0 .. b0 + nbk - 1, all of size NB.  TD (the Student-t model): q = y^H Ri y goes to qb (N,n_blocks,T) in every
// mode but SPATIAL, and LOSS writes sum log max(lambda(R), eps) alone
template <int NB, int MODE, bool TD = false>
__global__ void __launch_bounds__(BLK) ip_model_kernel(const cx* __restrict__ X, const cx* __restrict__ W,
                                                       const cx* __restrict__ U, const double* __restrict__ H,
                                                       cx* __restrict__ ri, cx* __restrict__ zz,
                                                       double* __restrict__ lossp, int32_t* status, double eps, IpGeo g,
                                                       int b0, int nbk, double* __restrict__ qb = nullptr) {
  const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
  const size_t T = g.T;
  if (idx >= (size_t)g.M * nbk * T) return;
  const int t = (int)(idx % T), b = b0 + (int)((idx / T) % nbk), n = (int)(idx / (T * nbk));
  const IpBlock bk = ip_block(g, b);
  Mat<NB> R;
  herm::set_zero(R);
  for (int k = 0; k < g.K; ++k) {
    const double h = H[((size_t)n * g.K + k) * T + t];
    const cx* Uk = U + ((size_t)n * g.K + k) * g.P + bk.off;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        const cx u = Uk[i * NB + j];
        R.re[i][j] += h * u.x, R.im[i][j] += h * u.y;
      }
  }
  ip_psd(R, eps);
  double ld = 0.0;
  if (MODE == MODE_LOSS) {
    Mat<NB> E = R;
    double w[NB];
    ip_eigvals(E, w);
#pragma unroll
    for (int i = 0; i < NB; ++i) ld += log(fmax(w[i], eps));
  }
  Mat<NB> Ri;
  const bool ok = ip_inv(R, Ri);
  ip_psd(Ri, eps);
  ip_flag(status, !ok);
  // y = W x of the block's bins, v = Ri y
  double yr[NB], yi[NB], vr[NB], vi[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int f = bk.f0 + i;
    cx acc = make_double2(0.0, 0.0);
    for (int c = 0; c < g.M; ++c) {
      const cx p = cmul(W[((size_t)f * g.M + n) * g.M + c], X[((size_t)c * g.F + f) * T + t]);
      acc.x += p.x, acc.y += p.y;
    }
    yr[i] = acc.x, yi[i] = acc.y;
  }
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      sr += Ri.re[i][j] * yr[j] - Ri.im[i][j] * yi[j];
      si += Ri.re[i][j] * yi[j] + Ri.im[i][j] * yr[j];
    }
    vr[i] = sr, vi[i] = si;
  }
  if (TD && MODE != MODE_SPATIAL) {  // the spatial update forms q per sweep (ip_tq_kernel)
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < NB; ++i) q += yr[i] * vr[i] + yi[i] * vi[i];
    qb[((size_t)n * g.nblk + b) * T + t] = q;
    if (MODE == MODE_LOSS) {
      lossp[((size_t)n * g.nblk + b) * T + t] = ld;
      return;
    }
  } else if (MODE == MODE_LOSS) {
    double q = 0.0;
#pragma unroll
    for (int i = 0; i < NB; ++i) q += yr[i] * vr[i] + yi[i] * vi[i];
    lossp[((size_t)n * g.nblk + b) * T + t] = q + ld;
    return;
  }
  ip_store_t(Ri, ri + ((size_t)n * g.P + bk.off) * T + t, T);
  if (MODE == MODE_BASIS || MODE == MODE_ACT) {
    // Ri (y y^H + c I) Ri = v v^H + c Ri Ri for the Hermitian Ri; c = eps, and for ACT the eps-trace shift of psd on top
    double c = eps;
    if (MODE == MODE_ACT) {
      double tr = 0.0;
#pragma unroll
      for (int i = 0; i < NB; ++i) tr += (yr[i] * yr[i] + yi[i] * yi[i]) + eps;
      c = eps + eps * tr;
    }
    Mat<NB> Z;
    herm::matmul(Ri, Ri, Z);
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        Z.re[i][j] = c * Z.re[i][j] + (vr[i] * vr[j] + vi[i] * vi[j]);
        Z.im[i][j] = c * Z.im[i][j] + (vi[i] * vr[j] - vr[i] * vi[j]);
      }
    ip_store_t(Z, zz + ((size_t)n * g.P + bk.off) * T + t, T);
  }
}

// one wave per (source, entry): part[n][0][k][e] = sum_t H[n,k,t] zz[n,e,t], part[n][1][k][e] the same with ri.  TD: zz is
// weighted by pi[n,t] first
template <bool TD = false>
__global__ void __launch_bounds__(BLK) ip_contract_kernel(const double* __restrict__ H, const cx* __restrict__ ri,
                                                          const cx* __restrict__ zz, cx* __restrict__ part, IpGeo g,
                                                          const double* __restrict__ pi = nullptr) {
  const size_t wv = (size_t)blockIdx.x * NW + threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  if (wv >= (size_t)g.M * g.P) return;
  const size_t n = wv / g.P, e = wv % g.P, T = g.T;
  const cx *zrow = zz + wv * T, *rrow = ri + wv * T;
  for (int k0 = 0; k0 < g.K; k0 += KC) {
    double s[KC][2], r[KC][2];
#pragma unroll
    for (int c = 0; c < KC; ++c) s[c][0] = s[c][1] = r[c][0] = r[c][1] = 0.0;
    for (size_t t = lane; t < T; t += WAVE) {
      cx z = zrow[t];
      const cx q = rrow[t];
      if (TD) {
        const double p = pi[n * T + t];
        z.x = p * z.x, z.y = p * z.y;
      }
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const double h = H[(n * g.K + min(k0 + c, g.K - 1)) * T + t];
        s[c][0] += h * z.x, s[c][1] += h * z.y, r[c][0] += h * q.x, r[c][1] += h * q.y;
      }
    }
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      for (int o = WAVE / 2; o > 0; o >>= 1) {
        s[c][0] += __shfl_xor(s[c][0], o), s[c][1] += __shfl_xor(s[c][1], o);
        r[c][0] += __shfl_xor(r[c][0], o), r[c][1] += __shfl_xor(r[c][1], o);
      }
      if (lane == 0 && k0 + c < g.K) {
        part[((n * 2 + 0) * g.K + k0 + c) * g.P + e] = make_double2(s[c][0], s[c][1]);
        part[((n * 2 + 1) * g.K + k0 + c) * g.P + e] = make_double2(r[c][0], r[c][1]);
      }
    }
  }
}

template <int NB>
__global__ void __launch_bounds__(BLK) ip_basis_kernel(cx* __restrict__ U, const cx* __restrict__ part, int32_t* status,
                                                       double eps, IpGeo g, int b0, int nbk) {
  const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (idx >= (size_t)g.M * g.K * nbk) return;
  const int b = b0 + (int)(idx % nbk), k = (int)((idx / nbk) % g.K), n = (int)(idx / ((size_t)nbk * g.K));
  const IpBlock bk = ip_block(g, b);
  cx* Up = U + ((size_t)n * g.K + k) * g.P + bk.off;
  Mat<NB> A, Bm, C, Uk, sq;
  ip_load(part + (((size_t)n * 2 + 0) * g.K + k) * g.P + bk.off, A);  // S
  herm::hermitize(A);
  herm::herm_sqrt_psd(A, sq);
  ip_psd(sq, eps);
  ip_load(Up, Uk);
  ip_load(part + (((size_t)n * 2 + 1) * g.K + k) * g.P + bk.off, Bm);  // T
  herm::matmul(sq, Uk, A);
  herm::matmul(A, Bm, C);
  herm::matmul(C, Uk, A);
  herm::matmul(A, sq, C);  // S^1/2 U T U S^1/2
  ip_psd(C, eps);
  herm::herm_sqrt_psd(C, A);
  ip_psd(A, eps);
  const bool ok = ip_inv(A, Bm);
  ip_psd(Bm, eps);
  ip_flag(status, !ok);
  herm::matmul(Uk, sq, A);
  herm::matmul(A, Bm, C);
  herm::matmul(C, sq, A);
  herm::matmul(A, Uk, C);  // U S^1/2 (.)^-1 S^1/2 U
  ip_psd(C, eps);
  ip_store(C, Up);
}

// G in zz, Ri in ri (both from the new U).  TD: num is weighted by pi[n,t] before its floor
template <bool TD = false>
__global__ void __launch_bounds__(BLK) ip_act_kernel(const cx* __restrict__ U, double* __restrict__ H,
                                                     const cx* __restrict__ ri, const cx* __restrict__ zz, double eps,
                                                     IpGeo g, const double* __restrict__ pi = nullptr) {
  const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x, T = g.T;
  if (idx >= (size_t)g.M * g.K * T) return;
  const size_t t = idx % T, nk = idx / T, n = nk / g.K;
  const cx* Uk = U + nk * g.P;
  double num = 0.0, den = 0.0;
  for (int e = 0; e < g.P; ++e) {
    const cx u = Uk[e], z = zz[(n * g.P + e) * T + t], r = ri[(n * g.P + e) * T + t];
    num += u.x * z.x + u.y * z.y;
    den += u.x * r.x + u.y * r.y;
  }
  if (TD) num = pi[n * T + t] * num;
  H[idx] = H[idx] * sqrt(fmax(num, 0.0) / fmax(den, eps));
}

__global__ void __launch_bounds__(BLK) ip_norm_kernel(cx* __restrict__ U, double* __restrict__ H, IpGeo g) {
  __shared__ double red[NW];
  const size_t nk = blockIdx.x;
  cx* Uk = U + nk * g.P;
  double tr = 0.0;
  for (int b = threadIdx.x; b < g.nblk; b += BLK) {
    const IpBlock bk = ip_block(g, b);
    for (int i = 0; i < bk.nb; ++i) tr += Uk[bk.off + i * bk.nb + i].x;
  }
  tr = mf::block_sum_all(tr, red);
  for (int e = threadIdx.x; e < g.P; e += BLK) Uk[e] = make_double2(Uk[e].x / tr, Uk[e].y / tr);
  for (int t = threadIdx.x; t < g.T; t += BLK) H[nk * g.T + t] = H[nk * g.T + t] * tr;
}

// one wave per (source, bin), lane = entry (c, d)
__global__ void __launch_bounds__(WAVE) ip_q_kernel(const cx* __restrict__ X, const cx* __restrict__ ri, cx* __restrict__ Q,
                                                    double eps, IpGeo g) {
  const int n = blockIdx.x / g.F, f = blockIdx.x % g.F;
  const int c = threadIdx.x >> 3, d = threadIdx.x & 7;
  if (c >= g.M || d >= g.M) return;
  // the block and the position of bin f
  const int split = g.nlow * g.nn;
  const int b = f < split ? f / g.nn : g.nlow + (f - split) / (g.nn + 1);
  const IpBlock bk = ip_block(g, b);
  const int i = f - bk.f0;
  const size_t T = g.T;
  const cx* w = ri + ((size_t)n * g.P + bk.off + i * bk.nb + i) * T;
  const cx *xc = X + ((size_t)c * g.F + f) * T, *xd = X + ((size_t)d * g.F + f) * T;
  double re = 0.0, im = 0.0;
  for (size_t t = 0; t < T; ++t) {
    const double wt = w[t].x;
    const cx a = xc[t], bb = xd[t];
    double pr = a.x * bb.x + a.y * bb.y;
    const double pi = a.y * bb.x - a.x * bb.y;
    if (c == d) {
      double tr = 0.0;
      for (int m = 0; m < g.M; ++m) {
        const cx v = X[((size_t)m * g.F + f) * T + t];
        tr += v.x * v.x + v.y * v.y;
      }
      pr += eps * tr;
    }
    re += wt * pr, im += wt * pi;
  }
  Q[(((size_t)n * g.F + f) * g.M + c) * g.M + d] = make_double2(re / (double)g.T, im / (double)g.T);
}

template <int N>
__global__ void __launch_bounds__(BLK) ip_topsd_kernel(cx* __restrict__ A, size_t n_mat, double eps) {
  const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (idx >= n_mat) return;
  Mat<N> Am;
  ip_load(A + idx * N * N, Am);
  ip_psd(Am, eps);
  ip_store(Am, A + idx * N * N);
}

// a[M][M] x = b in place (b becomes x), LU with partial pivoting (pivot by |re| + |im|); false on a zero pivot
__device__ inline bool ip_solve(int M, cx (*a)[MMAX], cx* b) {
  bool ok = true;
  for (int j = 0; j < M; ++j) {
    int p = j;
    double best = fabs(a[j][j].x) + fabs(a[j][j].y);
    for (int i = j + 1; i < M; ++i) {
      const double v = fabs(a[i][j].x) + fabs(a[i][j].y);
      if (v > best) best = v, p = i;
    }
    if (!(best > 0.0)) ok = false;
    if (p != j) {
      for (int c = 0; c < M; ++c) {
        const cx tmp = a[j][c];
        a[j][c] = a[p][c], a[p][c] = tmp;
      }
      const cx tmp = b[j];
      b[j] = b[p], b[p] = tmp;
    }
    for (int i = j + 1; i < M; ++i) {
      const cx l = cdiv(a[i][j], a[j][j]);
      for (int c = j + 1; c < M; ++c) {
        const cx m = cmul(l, a[j][c]);
        a[i][c].x -= m.x, a[i][c].y -= m.y;
      }
      const cx m = cmul(l, b[j]);
      b[i].x -= m.x, b[i].y -= m.y;
    }
  }
  for (int i = M - 1; i >= 0; --i) {
    cx s = b[i];
    for (int c = i + 1; c < M; ++c) {
      const cx m = cmul(a[i][c], b[c]);
      s.x -= m.x, s.y -= m.y;
    }
    b[i] = cdiv(s, a[i][i]);
  }
  return ok;
}

// ipsdta.py:946-971 for source n, position i of one block: Wl[i][n][:] <- conj(weight zeta - zeta_hat)
__device__ inline bool ip_vcd_row(int M, int n, cx (*Wi)[MMAX], const cx* __restrict__ Qg, const cx* gam, double eps) {
  cx a[MMAX][MMAX], q[MMAX][MMAX], zeta[MMAX], zh[MMAX], u[MMAX];
  for (int c = 0; c < M; ++c)
    for (int d = 0; d < M; ++d) q[c][d] = Qg[c * M + d];
  for (int r = 0; r < M; ++r)
    for (int d = 0; d < M; ++d) {
      cx s = make_double2(0.0, 0.0);
      for (int c = 0; c < M; ++c) {
        const cx m = cmul(Wi[r][c], q[c][d]);
        s.x += m.x, s.y += m.y;
      }
      a[r][d] = s;
    }
  for (int c = 0; c < M; ++c) zeta[c] = make_double2(c == n ? 1.0 : 0.0, 0.0), zh[c] = gam[c];
  bool ok = ip_solve(M, a, zeta);
  for (int c = 0; c < M; ++c)
    for (int d = 0; d < M; ++d) a[c][d] = q[c][d];
  ok = ip_solve(M, a, zh) && ok;
  for (int d = 0; d < M; ++d) {  // u = zeta^H Q
    cx s = make_double2(0.0, 0.0);
    for (int c = 0; c < M; ++c) {
      const cx m = cmulc(q[c][d], zeta[c]);
      s.x += m.x, s.y += m.y;
    }
    u[d] = s;
  }
  cx eta = make_double2(0.0, 0.0), etah = make_double2(0.0, 0.0);
  for (int d = 0; d < M; ++d) {
    const cx m = cmul(u[d], zeta[d]), mh = cmul(u[d], zh[d]);
    eta.x += m.x, eta.y += m.y, etah.x += mh.x, etah.y += mh.y;
  }
  if (hypot(eta.x, eta.y) < eps) eta = make_double2(eps, 0.0);
  const double ah = hypot(etah.x, etah.y);
  cx wt;
  if (ah < eps) {
    wt = cdiv(make_double2(1.0, 0.0), csqrt_(eta));
  } else {
    const double a2 = ah * ah;
    const cx root = csqrt_(make_double2(1.0 + 4.0 * eta.x / a2, 4.0 * eta.y / a2));
    const cx lead = cdiv(etah, make_double2(2.0 * eta.x, 2.0 * eta.y));
    wt = cmul(lead, make_double2(1.0 - root.x, -root.y));
  }
  for (int c = 0; c < M; ++c) {
    const cx m = cmul(wt, zeta[c]);
    Wi[n][c] = make_double2(m.x - zh[c].x, -(m.y - zh[c].y));
  }
  return ok;
}

__global__ void __launch_bounds__(BLK) ip_sweep_kernel(const cx* __restrict__ X, cx* __restrict__ W,
                                                       const cx* __restrict__ ri, const cx* __restrict__ Q,
                                                       int32_t* status, double eps, IpGeo g) {
  __shared__ cx Wl[NBMAX][MMAX][MMAX];
  __shared__ cx red[NW][MMAX];
  __shared__ cx gam[MMAX];
  const int b = blockIdx.x, M = g.M, tid = threadIdx.x;
  const IpBlock bk = ip_block(g, b);
  const int nb = bk.nb;
  const size_t T = g.T;
  for (int e = tid; e < nb * M * M; e += BLK) Wl[e / (M * M)][(e / M) % M][e % M] = W[(size_t)bk.f0 * M * M + e];
  __syncthreads();
  for (int n = 0; n < M; ++n) {
    for (int i = 0; i < nb; ++i) {
      double ar[MMAX], ai[MMAX];
#pragma unroll
      for (int c = 0; c < MMAX; ++c) ar[c] = 0.0, ai[c] = 0.0;
      if (nb > 1) {
        for (size_t t = tid; t < T; t += BLK) {
          cx s = make_double2(0.0, 0.0);
          for (int j = 0; j < nb; ++j) {
            if (j == i) continue;
            cx y = make_double2(0.0, 0.0);
            for (int c = 0; c < M; ++c) {
              const cx p = cmul(Wl[j][n][c], X[((size_t)c * g.F + bk.f0 + j) * T + t]);
              y.x += p.x, y.y += p.y;
            }
            const cx p = cmulc(ri[((size_t)n * g.P + bk.off + j * nb + i) * T + t], y);
            s.x += p.x, s.y += p.y;
          }
#pragma unroll
          for (int c = 0; c < MMAX; ++c) {
            if (c < M) {
              const cx p = cmul(s, X[((size_t)c * g.F + bk.f0 + i) * T + t]);
              ar[c] += p.x, ai[c] += p.y;
            }
          }
        }
      }
#pragma unroll
      for (int c = 0; c < MMAX; ++c) {
        for (int o = WAVE / 2; o > 0; o >>= 1) ar[c] += __shfl_xor(ar[c], o), ai[c] += __shfl_xor(ai[c], o);
        if ((tid & (WAVE - 1)) == 0) red[tid / WAVE][c] = make_double2(ar[c], ai[c]);
      }
      __syncthreads();
      if (tid == 0) {
        for (int c = 0; c < M; ++c) {
          const double sr = ((red[0][c].x + red[1][c].x) + red[2][c].x) + red[3][c].x;
          const double si = ((red[0][c].y + red[1][c].y) + red[2][c].y) + red[3][c].y;
          gam[c] = make_double2(sr / (double)g.T, si / (double)g.T);
        }
        const bool ok = ip_vcd_row(M, n, Wl[i], Q + ((size_t)n * g.F + bk.f0 + i) * M * M, gam, eps);
        ip_flag(status, !ok);
      }
      __syncthreads();
    }
  }
  for (int e = tid; e < nb * M * M; e += BLK) W[(size_t)bk.f0 * M * M + e] = Wl[e / (M * M)][(e / M) % M][e % M];
}

// sum over the bins f = tid, tid + BLK, ... of log|det W_f| with |det| from an LU: sum_i log max(|u_ii|, eps)
__device__ inline double ip_logdet_w(const cx* __restrict__ W, double eps, const IpGeo& g) {
  double ldw = 0.0;
  const int M = g.M;
  for (int f = threadIdx.x; f < g.F; f += BLK) {
    cx a[MMAX][MMAX];
    for (int r = 0; r < M; ++r)
      for (int c = 0; c < M; ++c) a[r][c] = W[((size_t)f * M + r) * M + c];
    for (int j = 0; j < M; ++j) {
      int p = j;
      double best = fabs(a[j][j].x) + fabs(a[j][j].y);
      for (int i = j + 1; i < M; ++i) {
        const double s = fabs(a[i][j].x) + fabs(a[i][j].y);
        if (s > best) best = s, p = i;
      }
      if (p != j)
        for (int c = 0; c < M; ++c) {
          const cx tmp = a[j][c];
          a[j][c] = a[p][c], a[p][c] = tmp;
        }
      const double piv = hypot(a[j][j].x, a[j][j].y);
      ldw += log(fmax(piv, eps));
      if (piv > 0.0)
        for (int i = j + 1; i < M; ++i) {
          const cx l = cdiv(a[i][j], a[j][j]);
          for (int c = j + 1; c < M; ++c) {
            const cx m = cmul(l, a[j][c]);
            a[i][c].x -= m.x, a[i][c].y -= m.y;
          }
        }
    }
  }
  return ldw;
}

// loss = sum lossp - 2 T sum_f log max(|det W_f|, ...)
__global__ void __launch_bounds__(BLK) ip_loss_kernel(const cx* __restrict__ W, const double* __restrict__ lossp,
                                                      double* __restrict__ loss, double eps, IpGeo g) {
  __shared__ double red[NW];
  const size_t n_terms = (size_t)g.M * g.nblk * g.T;
  double v = 0.0;
  for (size_t e = threadIdx.x; e < n_terms; e += BLK) v += lossp[e];
  v = mf::block_sum_all(v, red);
  const double ldw = mf::block_sum_all(ip_logdet_w(W, eps, g), red);
  if (threadIdx.x == 0) loss[0] = v - 2.0 * (double)g.T * ldw;
}

// ---- the Student-t model (tIPSDTA, src/bss/ipsdta.py:1083-1762) --------------------------------------------------------
// Every update is weighted per (source, frame) by pi[n,t] = (nu + 2 F) / (nu + 2 sum_b q[n,b,t]), q = y_b^H Ri_b y_b.  The
// model pass writes q per block (TD above), ip_pi_kernel adds the blocks in index order.  The source model weights S_k and
// num by pi.  The spatial model cannot hoist Q (it holds pi, which holds W): a sweep is the sequence of steps (source n;
// the low blocks at position 0..nn-1, then the high blocks at position 0..nn), each step ip_pi_kernel for source n and then
// ip_tstep_kernel over the blocks of the group; stream order between the two is the only coupling between blocks.  A sweep
// starts with ip_tq_kernel, which forms q of all blocks from the current W.

// one thread per (source, frame) of the sources n0 .. n0 + cnt - 1, the blocks in index order
__global__ void __launch_bounds__(BLK) ip_pi_kernel(const double* __restrict__ qb, double* __restrict__ pi, double nu, IpGeo g,
                                                    int n0, int cnt) {
  const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x, T = g.T;
  if (idx >= (size_t)cnt * T) return;
  const size_t n = n0 + idx / T, t = idx % T;
  double s = 0.0;
  for (int b = 0; b < g.nblk; ++b) s += qb[(n * g.nblk + b) * T + t];
  pi[n * T + t] = (nu + 2.0 * (double)g.F) / (nu + 2.0 * s);
}

// q[n,b,t] = y_b^H Ri_b y_b from the Ri of the workspace and the current W, one thread per (source, block, frame).  Every
// sweep starts from this kernel's q, whether it is the first of its call or not: a call of n sweeps equals n calls of one
// bit for bit (the step kernel's own q serves the steps after it within the sweep).
__global__ void __launch_bounds__(BLK) ip_tq_kernel(const cx* __restrict__ X, const cx* __restrict__ W,
                                                    const cx* __restrict__ ri, double* __restrict__ qb, IpGeo g) {
  const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x, T = g.T;
  if (idx >= (size_t)g.M * g.nblk * T) return;
  const size_t t = idx % T;
  const int b = (int)((idx / T) % g.nblk), n = (int)(idx / (T * g.nblk));
  const IpBlock bk = ip_block(g, b);
  const int nb = bk.nb;
  const cx* rn = ri + ((size_t)n * g.P + bk.off) * T;
  double yr[NBMAX], yi[NBMAX];
#pragma unroll
  for (int j = 0; j < NBMAX; ++j) {
    cx y = make_double2(0.0, 0.0);
    if (j < nb) {
      for (int c = 0; c < g.M; ++c) {
        const cx m = cmul(W[((size_t)(bk.f0 + j) * g.M + n) * g.M + c], X[((size_t)c * g.F + bk.f0 + j) * T + t]);
        y.x += m.x, y.y += m.y;
      }
    }
    yr[j] = y.x, yi[j] = y.y;
  }
  double q = 0.0;
#pragma unroll
  for (int a = 0; a < NBMAX; ++a) {
    if (a < nb) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int j = 0; j < NBMAX; ++j) {
        if (j < nb) {
          const cx r = rn[(size_t)(a * nb + j) * T + t];
          sr += r.x * yr[j] - r.y * yi[j];
          si += r.x * yi[j] + r.y * yr[j];
        }
      }
      q += yr[a] * sr + yi[a] * si;
    }
  }
  qb[idx] = q;
}

// One VCD step of source n at position i of the blocks b0 + blockIdx.x (all of one size): over the frames, the Hermitian
// Q = mean_t pi (Ri)_ii (x x^H + eps |x|^2 I) (its diagonal and the entries below it, M^2 doubles) and gamma = mean_t pi
// sum_{j != i} (Ri)_ji x conj(y_j) (2 M doubles) per thread, a butterfly and LDS add them in a fixed order; thread 0 applies
// psd, solves and writes row n of W_f; then all threads recompute q[n,b,:] with the new row.
template <int M>
__global__ void __launch_bounds__(BLK) ip_tstep_kernel(const cx* __restrict__ X, cx* __restrict__ W, const cx* __restrict__ ri,
                                                       const double* __restrict__ pi, double* __restrict__ qb,
                                                       int32_t* status, double eps, IpGeo g, int n, int b0, int i) {
  constexpr int NQ = M * M, NA = NQ + 2 * M;
  static_assert(NW == 4, "the waves' partial sums are added as ((0 + 1) + 2) + 3");
  __shared__ cx Wf[MMAX][MMAX];
  __shared__ cx wn[NBMAX][MMAX];
  __shared__ double red[NW][NA];
  __shared__ cx Qs[M * M];
  __shared__ cx gam[MMAX];
  const int b = b0 + blockIdx.x, tid = threadIdx.x;
  const IpBlock bk = ip_block(g, b);
  const int nb = bk.nb, f = bk.f0 + i;
  const size_t T = g.T;
  for (int e = tid; e < M * M; e += BLK) Wf[e / M][e % M] = W[(size_t)f * M * M + e];
  for (int e = tid; e < nb * M; e += BLK) wn[e / M][e % M] = W[((size_t)(bk.f0 + e / M) * M + n) * M + e % M];
  __syncthreads();
  const double* pin = pi + (size_t)n * T;
  const cx* rn = ri + ((size_t)n * g.P + bk.off) * T;
  double acc[NA];
#pragma unroll
  for (int k = 0; k < NA; ++k) acc[k] = 0.0;
  for (size_t t = tid; t < T; t += BLK) {
    const double p = pin[t];
    cx x[M];
    double tr = 0.0;
#pragma unroll
    for (int c = 0; c < M; ++c) {
      x[c] = X[((size_t)c * g.F + f) * T + t];
      tr += x[c].x * x[c].x + x[c].y * x[c].y;
    }
    const double wt = p * rn[(size_t)(i * nb + i) * T + t].x;
    int k = 0;
#pragma unroll
    for (int c = 0; c < M; ++c)
#pragma unroll
      for (int d = 0; d <= c; ++d) {
        double pr = x[c].x * x[d].x + x[c].y * x[d].y;
        if (c == d) {
          pr += eps * tr;
          acc[k++] += wt * pr;
        } else {
          acc[k++] += wt * pr;
          acc[k++] += wt * (x[c].y * x[d].x - x[c].x * x[d].y);
        }
      }
    if (nb > 1) {
      cx s = make_double2(0.0, 0.0);
      for (int j = 0; j < nb; ++j) {
        if (j == i) continue;
        cx y = make_double2(0.0, 0.0);
#pragma unroll
        for (int c = 0; c < M; ++c) {
          const cx m = cmul(wn[j][c], X[((size_t)c * g.F + bk.f0 + j) * T + t]);
          y.x += m.x, y.y += m.y;
        }
        const cx m = cmulc(rn[(size_t)(j * nb + i) * T + t], y);
        s.x += m.x, s.y += m.y;
      }
      s.x = p * s.x, s.y = p * s.y;
#pragma unroll
      for (int c = 0; c < M; ++c) {
        const cx m = cmul(s, x[c]);
        acc[NQ + 2 * c] += m.x, acc[NQ + 2 * c + 1] += m.y;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < NA; ++k) {
    for (int o = WAVE / 2; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
    if ((tid & (WAVE - 1)) == 0) red[tid / WAVE][k] = acc[k];
  }
  __syncthreads();
  if (tid == 0) {
    double tot[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) tot[k] = (((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]) / (double)g.T;
    Mat<M> Q;
    int k = 0;
#pragma unroll
    for (int c = 0; c < M; ++c)
#pragma unroll
      for (int d = 0; d <= c; ++d) {
        if (c == d) {
          Q.re[c][c] = tot[k++], Q.im[c][c] = 0.0;
        } else {
          Q.re[c][d] = tot[k], Q.re[d][c] = tot[k++];
          Q.im[c][d] = tot[k], Q.im[d][c] = -tot[k++];
        }
      }
    ip_psd(Q, eps);
    ip_store(Q, Qs);
#pragma unroll
    for (int c = 0; c < M; ++c) gam[c] = make_double2(tot[NQ + 2 * c], tot[NQ + 2 * c + 1]);
    const bool ok = ip_vcd_row(M, n, Wf, Qs, gam, eps);
    ip_flag(status, !ok);
    for (int c = 0; c < M; ++c) {
      W[((size_t)f * M + n) * M + c] = Wf[n][c];
      wn[i][c] = Wf[n][c];
    }
  }
  __syncthreads();
  for (size_t t = tid; t < T; t += BLK) {
    double yr[NBMAX], yi[NBMAX];
#pragma unroll
    for (int j = 0; j < NBMAX; ++j) {
      cx y = make_double2(0.0, 0.0);
      if (j < nb) {
#pragma unroll
        for (int c = 0; c < M; ++c) {
          const cx m = cmul(wn[j][c], X[((size_t)c * g.F + bk.f0 + j) * T + t]);
          y.x += m.x, y.y += m.y;
        }
      }
      yr[j] = y.x, yi[j] = y.y;
    }
    double q = 0.0;
#pragma unroll
    for (int a = 0; a < NBMAX; ++a) {
      if (a < nb) {
        double sr = 0.0, si = 0.0;
#pragma unroll
        for (int j = 0; j < NBMAX; ++j) {
          if (j < nb) {
            const cx r = rn[(size_t)(a * nb + j) * T + t];
            sr += r.x * yr[j] - r.y * yi[j];
            si += r.x * yi[j] + r.y * yr[j];
          }
        }
        q += yr[a] * sr + yi[a] * si;
      }
    }
    qb[((size_t)n * g.nblk + b) * T + t] = q;
  }
}

// loss = sum ld + (nu + 2 F)/2 sum_{n,t} log(1 + (2/nu) sum_b q) - 2 T sum_f log|det W_f|, every sum in index order per thread
__global__ void __launch_bounds__(BLK) ip_tloss_kernel(const cx* __restrict__ W, const double* __restrict__ ld,
                                                       const double* __restrict__ qb, double* __restrict__ loss, double nu,
                                                       double eps, IpGeo g) {
  __shared__ double red[NW];
  const size_t n_terms = (size_t)g.M * g.nblk * g.T, T = g.T;
  double v = 0.0;
  for (size_t e = threadIdx.x; e < n_terms; e += BLK) v += ld[e];
  v = mf::block_sum_all(v, red);
  double u = 0.0;
  for (size_t e = threadIdx.x; e < (size_t)g.M * T; e += BLK) {
    const size_t n = e / T, t = e % T;
    double s = 0.0;
    for (int b = 0; b < g.nblk; ++b) s += qb[(n * g.nblk + b) * T + t];
    u += log(1.0 + (2.0 / nu) * s);
  }
  u = mf::block_sum_all(u, red);
  const double ldw = mf::block_sum_all(ip_logdet_w(W, eps, g), red);
  if (threadIdx.x == 0) loss[0] = (v + 0.5 * (nu + 2.0 * (double)g.F) * u) - 2.0 * (double)g.T * ldw;
}

#define IP_NB_SWITCH(nb, ...)                                   \
  switch (nb) {                                                 \
    case 1: { constexpr int NB = 1; __VA_ARGS__; } break;       \
    case 2: { constexpr int NB = 2; __VA_ARGS__; } break;       \
    case 3: { constexpr int NB = 3; __VA_ARGS__; } break;       \
    case 4: { constexpr int NB = 4; __VA_ARGS__; } break;       \
    case 5: { constexpr int NB = 5; __VA_ARGS__; } break;       \
    case 6: { constexpr int NB = 6; __VA_ARGS__; } break;       \
    case 7: { constexpr int NB = 7; __VA_ARGS__; } break;       \
    case 8: { constexpr int NB = 8; __VA_ARGS__; } break;       \
    default: break;                                             \
  }

struct IpArgs {
  const cx* X;
  cx* W;
  cx* U;
  double* H;
  double eps;
  int32_t* status;
  char* ws;
  IpGeo g;
  hipStream_t st;
  double nu;  // the Student-t entry points only
};

struct IpPtrs {
  cx *ri, *zz, *part, *q;
  double *qb, *lossp, *pi;
};

inline IpPtrs ip_ptrs(const IpArgs& a, bool td) {
  const IpLayout L = ip_layout(a.g, td);
  return {(cx*)(a.ws + L.ri), (cx*)(a.ws + L.zz), (cx*)(a.ws + L.part), (cx*)(a.ws + L.q),
          (double*)(a.ws + L.qb), (double*)(a.ws + L.lossp), (double*)(a.ws + L.pi)};
}

inline unsigned ip_grid(size_t n) { return (unsigned)((n + BLK - 1) / BLK); }

// f(b0, nbk, nb) for the low blocks (nbk blocks of nb bins from block b0 on), then for the high ones; a group without
// blocks is left out, the first non-zero return ends the walk
template <class Fn>
int ip_for_groups(const IpGeo& g, Fn f) {
  for (int h = 0; h < 2; ++h) {
    const int b0 = h ? g.nlow : 0, nbk = h ? g.nblk - g.nlow : g.nlow;
    if (nbk == 0) continue;
    const int rc = f(b0, nbk, g.nn + h);
    if (rc) return rc;
  }
  return 0;
}

template <int MODE, bool TD>
int ip_model(assx_ctx* ctx, const IpArgs& a, const IpPtrs& p) {
  const IpGeo& g = a.g;
  return ip_for_groups(g, [&](int b0, int nbk, int nb) -> int {
    IP_NB_SWITCH(nb, hipLaunchKernelGGL((ip_model_kernel<NB, MODE, TD>), dim3(ip_grid((size_t)g.M * nbk * g.T)), dim3(BLK),
                                        0, a.st, a.X, (const cx*)a.W, (const cx*)a.U, (const double*)a.H, p.ri, p.zz, p.lossp,
                                        a.status, a.eps, g, b0, nbk, TD ? p.qb : nullptr));
    ASSX_LAUNCH_CHECK(ctx, "ip_model_kernel");
    return 0;
  });
}

// pi of the sources n0 .. n0 + cnt - 1 from the q of the workspace (the Student-t model)
int ip_pi(assx_ctx* ctx, const IpArgs& a, const IpPtrs& p, int n0, int cnt) {
  hipLaunchKernelGGL(ip_pi_kernel, dim3(ip_grid((size_t)cnt * a.g.T)), dim3(BLK), 0, a.st, (const double*)p.qb, p.pi, a.nu,
                     a.g, n0, cnt);
  ASSX_LAUNCH_CHECK(ctx, "ip_pi_kernel");
  return 0;
}

// the model pass of MODE and, for the Student-t model, pi of all sources: what every source-model update starts with
template <int MODE, bool TD>
int ip_model_pi(assx_ctx* ctx, const IpArgs& a, const IpPtrs& p) {
  const int rc = ip_model<MODE, TD>(ctx, a, p);
  if (rc || !TD) return rc;
  return ip_pi(ctx, a, p, 0, a.g.M);
}

template <bool TD>
int ip_update_basis(assx_ctx* ctx, const IpArgs& a) {
  const IpGeo& g = a.g;
  const IpPtrs p = ip_ptrs(a, TD);
  const int rc = ip_model_pi<MODE_BASIS, TD>(ctx, a, p);
  if (rc) return rc;
  const size_t waves = (size_t)g.M * g.P;
  hipLaunchKernelGGL((ip_contract_kernel<TD>), dim3((unsigned)((waves + NW - 1) / NW)), dim3(BLK), 0, a.st,
                     (const double*)a.H, (const cx*)p.ri, (const cx*)p.zz, p.part, g, TD ? (const double*)p.pi : nullptr);
  ASSX_LAUNCH_CHECK(ctx, "ip_contract_kernel");
  return ip_for_groups(g, [&](int b0, int nbk, int nb) -> int {
    IP_NB_SWITCH(nb, hipLaunchKernelGGL((ip_basis_kernel<NB>), dim3(ip_grid((size_t)g.M * g.K * nbk)), dim3(BLK), 0, a.st,
                                        a.U, (const cx*)p.part, a.status, a.eps, g, b0, nbk));
    ASSX_LAUNCH_CHECK(ctx, "ip_basis_kernel");
    return 0;
  });
}

template <bool TD>
int ip_update_activation(assx_ctx* ctx, const IpArgs& a) {
  const IpGeo& g = a.g;
  const IpPtrs p = ip_ptrs(a, TD);
  const int rc = ip_model_pi<MODE_ACT, TD>(ctx, a, p);
  if (rc) return rc;
  hipLaunchKernelGGL((ip_act_kernel<TD>), dim3(ip_grid((size_t)g.M * g.K * g.T)), dim3(BLK), 0, a.st, (const cx*)a.U, a.H,
                     (const cx*)p.ri, (const cx*)p.zz, a.eps, g, TD ? (const double*)p.pi : nullptr);
  ASSX_LAUNCH_CHECK(ctx, "ip_act_kernel");
  return 0;
}

int ip_normalize(assx_ctx* ctx, const IpArgs& a) {
  hipLaunchKernelGGL(ip_norm_kernel, dim3((unsigned)(a.g.M * a.g.K)), dim3(BLK), 0, a.st, a.U, a.H, a.g);
  ASSX_LAUNCH_CHECK(ctx, "ip_norm_kernel");
  return 0;
}

template <bool TD>
int ip_update_source(assx_ctx* ctx, const IpArgs& a, int normalize) {
  int rc = ip_update_basis<TD>(ctx, a);
  if (rc) return rc;
  rc = ip_update_activation<TD>(ctx, a);
  if (rc) return rc;
  return normalize ? ip_normalize(ctx, a) : 0;
}

// the Gauss model: Q once, then the sweeps
int ip_update_spatial(assx_ctx* ctx, const IpArgs& a, int n_sweeps) {
  if (n_sweeps <= 0) return 0;
  const IpGeo& g = a.g;
  const IpPtrs p = ip_ptrs(a, false);
  int rc = ip_model<MODE_SPATIAL, false>(ctx, a, p);
  if (rc) return rc;
  hipLaunchKernelGGL(ip_q_kernel, dim3((unsigned)(g.M * g.F)), dim3(WAVE), 0, a.st, a.X, (const cx*)p.ri, p.q, a.eps, g);
  ASSX_LAUNCH_CHECK(ctx, "ip_q_kernel");
  const size_t nq = (size_t)g.M * g.F;
  IP_NB_SWITCH(g.M, hipLaunchKernelGGL((ip_topsd_kernel<NB>), dim3(ip_grid(nq)), dim3(BLK), 0, a.st, p.q, nq, a.eps));
  ASSX_LAUNCH_CHECK(ctx, "ip_topsd_kernel");
  for (int s = 0; s < n_sweeps; ++s) {
    hipLaunchKernelGGL(ip_sweep_kernel, dim3((unsigned)g.nblk), dim3(BLK), 0, a.st, a.X, a.W, (const cx*)p.ri, (const cx*)p.q,
                       a.status, a.eps, g);
    ASSX_LAUNCH_CHECK(ctx, "ip_sweep_kernel");
  }
  return 0;
}

// the Student-t model: 1 or 2 model launches, then per sweep the q pass and N (nn + (nn + 1 if there are high blocks))
// steps of 2 launches
int ip_tupdate_spatial(assx_ctx* ctx, const IpArgs& a, int n_sweeps) {
  if (n_sweeps <= 0) return 0;
  const IpGeo& g = a.g;
  const IpPtrs p = ip_ptrs(a, true);
  int rc = ip_model<MODE_SPATIAL, true>(ctx, a, p);
  if (rc) return rc;
  for (int s = 0; s < n_sweeps; ++s) {
    hipLaunchKernelGGL(ip_tq_kernel, dim3(ip_grid((size_t)g.M * g.nblk * g.T)), dim3(BLK), 0, a.st, a.X, (const cx*)a.W,
                       (const cx*)p.ri, p.qb, g);
    ASSX_LAUNCH_CHECK(ctx, "ip_tq_kernel");
    for (int n = 0; n < g.M; ++n) {
      rc = ip_for_groups(g, [&](int b0, int nbk, int nb) -> int {
        for (int i = 0; i < nb; ++i) {
          const int rp = ip_pi(ctx, a, p, n, 1);
          if (rp) return rp;
          IP_NB_SWITCH(g.M, hipLaunchKernelGGL((ip_tstep_kernel<NB>), dim3((unsigned)nbk), dim3(BLK), 0, a.st, a.X, a.W,
                                               (const cx*)p.ri, (const double*)p.pi, p.qb, a.status, a.eps, g, n, b0, i));
          ASSX_LAUNCH_CHECK(ctx, "ip_tstep_kernel");
        }
        return 0;
      });
      if (rc) return rc;
    }
  }
  return 0;
}

template <bool TD>
int ip_loss(assx_ctx* ctx, const IpArgs& a, double* loss) {
  const IpPtrs p = ip_ptrs(a, TD);
  const int rc = ip_model<MODE_LOSS, TD>(ctx, a, p);
  if (rc) return rc;
  if (TD) {
    hipLaunchKernelGGL(ip_tloss_kernel, dim3(1), dim3(BLK), 0, a.st, (const cx*)a.W, (const double*)p.lossp,
                       (const double*)p.qb, loss, a.nu, a.eps, a.g);
    ASSX_LAUNCH_CHECK(ctx, "ip_tloss_kernel");
  } else {
    hipLaunchKernelGGL(ip_loss_kernel, dim3(1), dim3(BLK), 0, a.st, (const cx*)a.W, (const double*)p.lossp, loss, a.eps, a.g);
    ASSX_LAUNCH_CHECK(ctx, "ip_loss_kernel");
  }
  return 0;
}

// n_iter x (source update, `spatial_iteration` sweeps, the loss if asked for)
template <bool TD>
int ip_iterate(assx_ctx* ctx, const IpArgs& a, int n_iter, int spatial_iteration, int normalize, double* loss) {
  for (int it = 0; it < n_iter; ++it) {
    int rc = ip_update_source<TD>(ctx, a, normalize);
    if (rc) return rc;
    rc = TD ? ip_tupdate_spatial(ctx, a, spatial_iteration) : ip_update_spatial(ctx, a, spatial_iteration);
    if (rc) return rc;
    if (loss) {
      rc = ip_loss<TD>(ctx, a, loss + it);
      if (rc) return rc;
    }
  }
  return 0;
}

inline bool ip_nu_ok(double nu) { return nu > 0.0 && nu <= 1.7976931348623157e308; }

// nu: the degree of freedom of the Student-t entry points, nullptr for the Gauss ones
int ip_args(assx_ctx* ctx, IpArgs& a, const void* X, void* W, void* U, void* H, double eps, int32_t* status, void* ws, int M,
            int F, int T, int K, int n_blocks, int dtype, void* stream, const double* nu = nullptr) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64 || dtype == ASSX_F32, ASSX_E_ARG, "bad dtype %d", dtype);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64, ASSX_E_UNSUPPORTED, "GaussIPSDTA: float64 only");
  ASSX_REQUIRE(ctx, ip_geo(M, F, T, K, n_blocks, a.g), ASSX_E_ARG,
               "GaussIPSDTA: M=%d F=%d T=%d K=%d n_blocks=%d outside the envelope (2 <= M <= 8, 1 <= K <= 64, 1 <= n_blocks "
               "<= F, largest block <= 8)",
               M, F, T, K, n_blocks);
  a.X = (const cx*)X, a.W = (cx*)W, a.U = (cx*)U, a.H = (double*)H, a.eps = eps, a.status = status, a.ws = (char*)ws;
  a.st = (hipStream_t)stream;
  if (nu) {
    ASSX_REQUIRE(ctx, ip_nu_ok(*nu), ASSX_E_ARG, "tIPSDTA: nu = %g (finite and > 0)", *nu);
    a.nu = *nu;
  }
  return 0;
}

}  // namespace

extern "C" {

size_t assx_ipsdta_workspace_bytes(int M, int F, int T, int K, int n_blocks, int dtype) {
  IpGeo g;
  if (dtype != ASSX_F64 || !ip_geo(M, F, T, K, n_blocks, g)) return 0;
  return ip_layout(g, false).total;
}

int assx_ipsdta_to_psd(assx_ctx* ctx, void* A, int n_mat, int nb, double eps, void* stream) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, n_mat >= 1 && nb >= 1 && nb <= NBMAX, ASSX_E_ARG,
               "assx_ipsdta_to_psd: n_mat=%d nb=%d (n_mat >= 1, nb in [1, 8])", n_mat, nb);
  ASSX_REQUIRE(ctx, A, ASSX_E_NULL, "assx_ipsdta_to_psd: NULL array");
  IP_NB_SWITCH(nb, hipLaunchKernelGGL((ip_topsd_kernel<NB>), dim3(ip_grid((size_t)n_mat)), dim3(BLK), 0,
                                      (hipStream_t)stream, (cx*)A, (size_t)n_mat, eps));
  ASSX_LAUNCH_CHECK(ctx, "ip_topsd_kernel");
  return 0;
}

int assx_ipsdta_update_basis(assx_ctx* ctx, const void* X, const void* W, void* U, const void* H, double eps, int32_t* status,
                             void* ws, int M, int F, int T, int K, int n_blocks, int dtype, void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, (void*)W, U, (void*)H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && U && H && ws, ASSX_E_NULL, "assx_ipsdta_update_basis: NULL array");
  return ip_update_basis<false>(ctx, a);
}

int assx_ipsdta_update_activation(assx_ctx* ctx, const void* X, const void* W, const void* U, void* H, double eps,
                                  int32_t* status, void* ws, int M, int F, int T, int K, int n_blocks, int dtype,
                                  void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, (void*)W, (void*)U, H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && U && H && ws, ASSX_E_NULL, "assx_ipsdta_update_activation: NULL array");
  return ip_update_activation<false>(ctx, a);
}

int assx_ipsdta_normalize(assx_ctx* ctx, void* U, void* H, int M, int F, int T, int K, int n_blocks, int dtype, void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, nullptr, nullptr, U, H, 0.0, nullptr, nullptr, M, F, T, K, n_blocks, dtype, stream);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, U && H, ASSX_E_NULL, "assx_ipsdta_normalize: NULL array");
  return ip_normalize(ctx, a);
}

int assx_ipsdta_update_source(assx_ctx* ctx, const void* X, const void* W, void* U, void* H, double eps, int normalize,
                              int32_t* status, void* ws, int M, int F, int T, int K, int n_blocks, int dtype, void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, (void*)W, U, H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && U && H && ws, ASSX_E_NULL, "assx_ipsdta_update_source: NULL array");
  return ip_update_source<false>(ctx, a, normalize);
}

int assx_ipsdta_update_spatial(assx_ctx* ctx, int n_sweeps, const void* X, void* W, const void* U, const void* H, double eps,
                               int32_t* status, void* ws, int M, int F, int T, int K, int n_blocks, int dtype, void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, W, (void*)U, (void*)H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, n_sweeps >= 0, ASSX_E_ARG, "assx_ipsdta_update_spatial: n_sweeps = %d", n_sweeps);
  ASSX_REQUIRE(ctx, X && W && U && H && ws, ASSX_E_NULL, "assx_ipsdta_update_spatial: NULL array");
  return ip_update_spatial(ctx, a, n_sweeps);
}

int assx_ipsdta_loss(assx_ctx* ctx, const void* X, const void* W, const void* U, const void* H, double eps, double* loss,
                     int32_t* status, void* ws, int M, int F, int T, int K, int n_blocks, int dtype, void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, (void*)W, (void*)U, (void*)H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && U && H && loss && ws, ASSX_E_NULL, "assx_ipsdta_loss: NULL array");
  return ip_loss<false>(ctx, a, loss);
}

int assx_ipsdta_iterate(assx_ctx* ctx, int n_iter, int spatial_iteration, const void* X, void* W, void* U, void* H, double eps,
                        int normalize, double* loss, int32_t* status, void* ws, int M, int F, int T, int K, int n_blocks,
                        int dtype, void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, W, U, H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, n_iter >= 0 && spatial_iteration >= 0, ASSX_E_ARG, "assx_ipsdta_iterate: n_iter = %d, spatial_iteration = %d",
               n_iter, spatial_iteration);
  ASSX_REQUIRE(ctx, X && W && U && H && ws, ASSX_E_NULL, "assx_ipsdta_iterate: NULL array");
  return ip_iterate<false>(ctx, a, n_iter, spatial_iteration, normalize, loss);
}

size_t assx_tipsdta_workspace_bytes(int M, int F, int T, int K, int n_blocks, int dtype, double nu) {
  IpGeo g;
  if (dtype != ASSX_F64 || !ip_nu_ok(nu) || !ip_geo(M, F, T, K, n_blocks, g)) return 0;
  return ip_layout(g, true).total;
}

int assx_tipsdta_update_basis(assx_ctx* ctx, const void* X, const void* W, void* U, const void* H, double eps, double nu,
                              int32_t* status, void* ws, int M, int F, int T, int K, int n_blocks, int dtype, void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, (void*)W, U, (void*)H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream, &nu);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && U && H && ws, ASSX_E_NULL, "assx_tipsdta_update_basis: NULL array");
  return ip_update_basis<true>(ctx, a);
}

int assx_tipsdta_update_activation(assx_ctx* ctx, const void* X, const void* W, const void* U, void* H, double eps, double nu,
                                   int32_t* status, void* ws, int M, int F, int T, int K, int n_blocks, int dtype,
                                   void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, (void*)W, (void*)U, H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream, &nu);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && U && H && ws, ASSX_E_NULL, "assx_tipsdta_update_activation: NULL array");
  return ip_update_activation<true>(ctx, a);
}

int assx_tipsdta_update_source(assx_ctx* ctx, const void* X, const void* W, void* U, void* H, double eps, double nu,
                               int normalize, int32_t* status, void* ws, int M, int F, int T, int K, int n_blocks, int dtype,
                               void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, (void*)W, U, H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream, &nu);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && U && H && ws, ASSX_E_NULL, "assx_tipsdta_update_source: NULL array");
  return ip_update_source<true>(ctx, a, normalize);
}

int assx_tipsdta_update_spatial(assx_ctx* ctx, int n_sweeps, const void* X, void* W, const void* U, const void* H, double eps,
                                double nu, int32_t* status, void* ws, int M, int F, int T, int K, int n_blocks, int dtype,
                                void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, W, (void*)U, (void*)H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream, &nu);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, n_sweeps >= 0, ASSX_E_ARG, "assx_tipsdta_update_spatial: n_sweeps = %d", n_sweeps);
  ASSX_REQUIRE(ctx, X && W && U && H && ws, ASSX_E_NULL, "assx_tipsdta_update_spatial: NULL array");
  return ip_tupdate_spatial(ctx, a, n_sweeps);
}

int assx_tipsdta_loss(assx_ctx* ctx, const void* X, const void* W, const void* U, const void* H, double eps, double nu,
                      double* loss, int32_t* status, void* ws, int M, int F, int T, int K, int n_blocks, int dtype,
                      void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, (void*)W, (void*)U, (void*)H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream, &nu);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && U && H && loss && ws, ASSX_E_NULL, "assx_tipsdta_loss: NULL array");
  return ip_loss<true>(ctx, a, loss);
}

int assx_tipsdta_iterate(assx_ctx* ctx, int n_iter, int spatial_iteration, const void* X, void* W, void* U, void* H, double eps,
                         double nu, int normalize, double* loss, int32_t* status, void* ws, int M, int F, int T, int K,
                         int n_blocks, int dtype, void* stream) {
  IpArgs a;
  int rc = ip_args(ctx, a, X, W, U, H, eps, status, ws, M, F, T, K, n_blocks, dtype, stream, &nu);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, n_iter >= 0 && spatial_iteration >= 0, ASSX_E_ARG,
               "assx_tipsdta_iterate: n_iter = %d, spatial_iteration = %d", n_iter, spatial_iteration);
  ASSX_REQUIRE(ctx, X && W && U && H && ws, ASSX_E_NULL, "assx_tipsdta_iterate: NULL array");
  return ip_iterate<true>(ctx, a, n_iter, spatial_iteration, normalize, loss);
}

}  // extern "C"
