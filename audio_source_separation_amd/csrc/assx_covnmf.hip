// MultichannelISNMF in the covariance domain (src/algorithm/nmf.py:116-148, 678-815) on MI355X: the whole iteration
// on the device.
//
// State (float64, one target): X (F,T,M,M) complex Hermitian, Tb (F,K) basis, V (K,T) activation, H (F,K,M,M) complex
// spatial.  With X^ = sum_k Tb[f,k] V[k,t] H_k, P = (X^ + eps I)^{-1} and Q = P X P (a full product: the target has full
// rank), one iteration is a fixed list of launches; every step re-forms X^ from the parameters as they stand:
//
//   basis       cv_eval_kernel<AB> -> a_k = tr(Q H_k), b_k = tr(P H_k) (2,K,F,T);  cv_basis_kernel per f, reduce over t
//   activation  cv_eval_kernel<AB>;  cv_act_partial_kernel (t block, f slice, k chunk);  act_apply_kernel
//   spatial     cv_eval_kernel<PQ> -> P and Q, Hermitian-packed, (F,T,2 M^2);  cv_spatial_sum_kernel (t slice, k group, f):
//               one thread per (k, packed entry) sums V[k,t] P and V[k,t] Q over its frames in order;
//               cv_riccati_kernel per (f, k): the slices in order, B = H C H, H A H = B by the closed form of
//               assx_herm_linalg.hpp (H = 0 where A is exactly 0), + eps I, / trace
//   loss        cv_eval_kernel<LOSS> (one partial per workgroup);  cv_loss_finalize_kernel
//   reconstruct cv_reconstruct_kernel, one thread per entry of X^
//
// One lane works on one (f, t) point for every M; a workgroup is one wave of 64 frames of one bin, with the bin's K
// spatial matrices Hermitian-packed in LDS (K M^2 reals, 32 KiB at the caps).  A Hermitian matrix is packed into M^2
// reals: entry (i, j) holds Re A_ij for i >= j and Im A_ji for i < j; a trace Re tr(A H) is then one dot product of two
// packed matrices with weight 2 off the diagonal.  Only lower triangles live in registers (P and Q: 2 M^2 doubles);
// Q = sum_c (column c of P) (row c of X) P is formed one row of X at a time, so the target is never held whole and is
// read exactly once per pass.  In PQ mode the wave's P and Q go through the LDS tile (the bin's H is dead by then), so
// that the 64 points leave as contiguous runs.
//
// The K reductions per point go through the two trace maps in the workspace, as MNMF's N do: the same evaluation pass
// serves the basis update (a sum over t) and the activation update (a sum over f), and both sums keep the fixed order
// of assx_factor_common.hpp (wave butterfly, waves in index order, slices in index order; no float atomics).  Two runs
// give the same bits, and iterate gives the bits of its steps called one by one.
#include "assx_common.hpp"
#include "assx_herm_linalg.hpp"
#include "assx_factor_common.hpp"

using namespace assx;
using namespace assx::mf;
using herm::Mat;

namespace {

constexpr int EBLK = WAVE;   // threads (frames) of an evaluation workgroup: one wave
constexpr int SBLK = 256;    // threads of a spatial-sum workgroup
constexpr int MODE_AB = 1, MODE_PQ = 2, MODE_LOSS = 3;

inline bool cv_in_envelope(int M, int F, int T, int K, int dtype) {
  if (dtype != ASSX_F64 || M < 2 || M > 8 || K < 1 || K > KMAX || F < 1 || T < 1) return false;
  if (F >= (1 << 28) || T >= (1 << 28)) return false;
  return (long long)M * M * F * T < (1LL << 28);  // the target stays below 4 GiB; no product below overflows
}

struct CvLayout {
  size_t ab, actp, pq, spp, lpart, total;
};

// ab: the trace maps (2,K,F,T); actp: activation slice partials (FS,2,K,T); pq: P and Q packed (F,T,2*M*M); spp: spatial
// slice partials (F,S,K,2*M*M); lpart: loss partials (F,nblocks(T, EBLK)).  All float64.
CvLayout cv_layout(int M, int F, int T, int K) {
  const size_t d = sizeof(double);
  Carve c(256);
  CvLayout L;
  L.ab = c.take((size_t)2 * K * F * T * d);
  L.actp = c.take((size_t)act_slices(F) * 2 * K * T * d);
  L.pq = c.take((size_t)F * T * 2 * M * M * d);
  L.spp = c.take((size_t)F * sp_slices(T) * K * 2 * M * M * d);
  L.lpart = c.take((size_t)F * nblocks(T, EBLK) * d);
  L.total = c.total();
  return L;
}

// entry (l, j) of a Hermitian matrix held as its lower triangle
template <int M>
__device__ __forceinline__ double lo_re(const Mat<M>& A, int l, int j) {
  return l >= j ? A.re[l][j] : A.re[j][l];
}
template <int M>
__device__ __forceinline__ double lo_im(const Mat<M>& A, int l, int j) {
  return l == j ? 0.0 : (l > j ? A.im[l][j] : -A.im[j][l]);
}

// A (lower triangle of X^) becomes the lower triangle of (X^ + eps I)^{-1}; ldet = sum_i ln L_ii of the Cholesky factor;
// false if the factorisation fails
template <int M>
__device__ __forceinline__ bool invert_point(Mat<M>& A, double eps, double& ldet) {
#pragma unroll
  for (int i = 0; i < M; ++i) A.re[i][i] += eps, A.im[i][i] = 0.0;
  const bool ok = herm::herm_cholesky(A);
  ldet = 0.0;
#pragma unroll
  for (int i = 0; i < M; ++i) ldet += log(A.re[i][i]);
  Mat<M> Li;
  herm::tri_inverse(A, Li);
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int k = i; k < M; ++k) {  // conj(Li_ki) Li_kj
        sr += Li.re[k][i] * Li.re[k][j] + Li.im[k][i] * Li.im[k][j];
        si += Li.re[k][i] * Li.im[k][j] - Li.im[k][i] * Li.re[k][j];
      }
      A.re[i][j] = sr, A.im[i][j] = i == j ? 0.0 : si;
    }
  return ok;
}

// one lane's packed matrix into its row of the LDS tile, then the wave's npts rows out as runs of MM reals, 2*MM apart
template <int M>
__device__ __forceinline__ void store_packed(const Mat<M>& A, bool active, double* tile, double* __restrict__ out,
                                             int npts) {
  constexpr int MM = M * M, LD = MM + 1;
  const int lane = threadIdx.x;
  if (active) {
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j < M; ++j) tile[lane * LD + i * M + j] = i >= j ? A.re[i][j] : A.im[j][i];
  }
  __syncthreads();
  for (int idx = lane; idx < npts * MM; idx += EBLK) {
    const int p = idx / MM, e = idx % MM;
    out[(size_t)p * 2 * MM + e] = tile[p * LD + e];
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------------------------
// The evaluation pass, one thread per (f, t), one wave per workgroup:
//   AB    a_k = Re tr(Q H_k) and b_k = Re tr(P H_k) into ab (2,K,F,T)
//   PQ    P and Q, packed, into pq (F,T,2*M*M)
//   LOSS  tr((X + eps I) P) - ln det(X + eps I) + ln det(X^ + eps I) - M, one partial per workgroup
// ---------------------------------------------------------------------------------------------------------------
template <int M, int MODE>
__global__ void __launch_bounds__(EBLK) cv_eval_kernel(const Cx<double>* __restrict__ X, const double* __restrict__ Tb,
                                                       const double* __restrict__ V, const Cx<double>* __restrict__ H,
                                                       double eps, double* __restrict__ ab, double* __restrict__ pq,
                                                       double* __restrict__ lpart, int32_t* __restrict__ status, int F,
                                                       int T, int K) {
  constexpr int MM = M * M, LD = MM + 1;
  __shared__ double sh[WAVE * LD];  // hp[k * MM + e]: the bin's H_k, packed; in PQ mode the wave's tile afterwards
  __shared__ double tv[KMAX];
  __shared__ double red[1];
  const int f = blockIdx.y, lane = threadIdx.x, t0 = blockIdx.x * EBLK, t = t0 + lane;
  const bool active = t < T;
  const Cx<double>* Hf = H + (size_t)f * K * MM;
  for (int i = lane; i < K * MM; i += EBLK) {
    const int k = i / MM, e = i % MM, r = e / M, c = e % M;
    const Cx<double> h = r >= c ? Hf[i] : Hf[k * MM + c * M + r];
    sh[i] = r >= c ? h.x : h.y;
  }
  for (int k = lane; k < K; k += EBLK) tv[k] = Tb[(size_t)f * K + k];
  __syncthreads();

  Mat<M> P, Q;
  double term = 0.0;
  bool ok = true;
  if (active) {
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) P.re[i][j] = 0.0, P.im[i][j] = 0.0;
    for (int k = 0; k < K; ++k) {
      const double w = tv[k] * V[(size_t)k * T + t];
      const double* h = sh + k * MM;
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          P.re[i][j] += w * h[i * M + j];
          if (j < i) P.im[i][j] += w * h[j * M + i];
        }
    }
    double ldh;
    ok = invert_point<M>(P, eps, ldh);
    const Cx<double>* Xp = X + ((size_t)f * T + t) * MM;
    if constexpr (MODE == MODE_LOSS) {
      Mat<M> Xm;
      double tr = 0.0;
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          const Cx<double> v = Xp[i * M + j];
          Xm.re[i][j] = v.x, Xm.im[i][j] = i == j ? 0.0 : v.y;
          if (i == j) {
            Xm.re[i][i] += eps;
            tr += Xm.re[i][i] * P.re[i][i];
          } else {
            tr += 2.0 * (Xm.re[i][j] * P.re[i][j] + Xm.im[i][j] * P.im[i][j]);
          }
        }
      ok = herm::herm_cholesky(Xm) && ok;
      double ldx = 0.0;
#pragma unroll
      for (int i = 0; i < M; ++i) ldx += log(Xm.re[i][i]);
      term = tr - 2.0 * ldx + 2.0 * ldh - (double)M;
    } else {
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) Q.re[i][j] = 0.0, Q.im[i][j] = 0.0;
#pragma unroll
      for (int c = 0; c < M; ++c) {
        double xr[M], xi[M], rr[M], ri[M];
#pragma unroll
        for (int l = 0; l < M; ++l) {
          const Cx<double> v = Xp[c * M + l];
          xr[l] = v.x, xi[l] = v.y;
        }
#pragma unroll
        for (int j = 0; j < M; ++j) {  // (row c of X) P
          double sr = 0.0, si = 0.0;
#pragma unroll
          for (int l = 0; l < M; ++l) {
            const double pr = lo_re<M>(P, l, j), pi = lo_im<M>(P, l, j);
            sr += xr[l] * pr - xi[l] * pi;
            si += xr[l] * pi + xi[l] * pr;
          }
          rr[j] = sr, ri[j] = si;
        }
#pragma unroll
        for (int i = 0; i < M; ++i) {  // Q_ij += P_ic r_j
          const double pr = lo_re<M>(P, i, c), pi = lo_im<M>(P, i, c);
#pragma unroll
          for (int j = 0; j <= i; ++j) {
            Q.re[i][j] += pr * rr[j] - pi * ri[j];
            if (j < i) Q.im[i][j] += pr * ri[j] + pi * rr[j];
          }
        }
      }
    }
    if (!ok && status) atomicOr(status, (int32_t)ASSX_STATUS_SINGULAR);
  }

  if constexpr (MODE == MODE_AB) {
    if (active) {
      const size_t plane = (size_t)K * F * T;
      for (int k = 0; k < K; ++k) {
        const double* h = sh + k * MM;
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int i = 0; i < M; ++i) {
          a += Q.re[i][i] * h[i * M + i];
          b += P.re[i][i] * h[i * M + i];
#pragma unroll
          for (int j = 0; j < i; ++j) {
            a += 2.0 * (Q.re[i][j] * h[i * M + j] + Q.im[i][j] * h[j * M + i]);
            b += 2.0 * (P.re[i][j] * h[i * M + j] + P.im[i][j] * h[j * M + i]);
          }
        }
        const size_t o = ((size_t)k * F + f) * T + t;
        ab[o] = a;
        ab[plane + o] = b;
      }
    }
  } else if constexpr (MODE == MODE_PQ) {
    __syncthreads();  // every lane is done with the bin's H
    const int npts = T - t0 < EBLK ? T - t0 : EBLK;
    double* out = pq + ((size_t)f * T + t0) * 2 * MM;
    store_packed<M>(P, active, sh, out, npts);
    store_packed<M>(Q, active, sh, out + MM, npts);
  } else {
    const double s = block_sum<double, 1>(term, red);
    if (lane == 0) lpart[(size_t)f * gridDim.x + blockIdx.x] = s;
  }
}

// the loss partials summed in a fixed order by one workgroup.  Not mf::batch_sum_kernel: with its int count the loop
// compiles to other code and assx_covnmf_loss measured 6 % slower (profiles/factor_common_refactor_bench.txt)
__global__ void __launch_bounds__(BLK) cv_loss_finalize_kernel(const double* __restrict__ lpart, double* __restrict__ loss,
                                                               size_t n) {
  __shared__ double red[BLK / WAVE];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (size_t i = tid; i < n; i += BLK) s += lpart[i];
  s = block_sum<double, BLK / WAVE>(s, red);
  if (tid == 0) loss[0] = s;
}

// ---------------------------------------------------------------------------------------------------------------
// basis (nmf.py:743-762): per f and k, num = sum_t V[k,t] a_k, den the same with b_k; Tb[f,k] *= sqrt(num / den) with
// den < eps -> eps.  The k are taken CH at a time.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLK) cv_basis_kernel(double* __restrict__ Tb, const double* __restrict__ V,
                                                       const double* __restrict__ ab, double eps, int F, int T, int K) {
  __shared__ double red[BLK / WAVE][2 * CH];
  const int f = blockIdx.x, tid = threadIdx.x;
  const size_t FT = (size_t)F * T, plane = (size_t)K * FT;
  const double* a = ab + (size_t)f * T;
  for (int k0 = 0; k0 < K; k0 += CH) {
    double num[CH], den[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) num[c] = 0.0, den[c] = 0.0;
    for (int t = tid; t < T; t += BLK) {
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int k = k0 + c;
        if (k < K) {
          const double v = V[(size_t)k * T + t];
          num[c] += v * a[k * FT + t];
          den[c] += v * a[plane + k * FT + t];
        }
      }
    }
    double sn, sd;
    block_pair_sums<double, BLK / WAVE>(num, den, red, sn, sd);
    if (tid < CH && k0 + tid < K) {
      if (sd < eps) sd = eps;
      double* tp = Tb + (size_t)f * K + k0 + tid;
      *tp = *tp * sqrt(sn / sd);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------
// activation (nmf.py:764-783): num[k,t] = sum_f Tb[f,k] a_k over an f slice per workgroup (partials (FS,2,K,T)); then
// act_apply_kernel adds the slices in ascending order and V *= sqrt(num / den), den < eps -> eps.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ABLK) cv_act_partial_kernel(const double* __restrict__ Tb, const double* __restrict__ ab,
                                                              double* __restrict__ part, int F, int T, int K, int FS) {
  const int t = blockIdx.x * ABLK + threadIdx.x, s = blockIdx.y, k0 = blockIdx.z * CH;
  if (t >= T) return;
  const int f0 = (int)((long long)F * s / FS), f1 = (int)((long long)F * (s + 1) / FS);
  const size_t FT = (size_t)F * T, plane = (size_t)K * FT;
  double num[CH], den[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) num[c] = 0.0, den[c] = 0.0;
  for (int f = f0; f < f1; ++f) {
    const double* tf = Tb + (size_t)f * K;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int k = k0 + c;
      if (k < K) {
        const size_t o = (size_t)k * FT + (size_t)f * T + t;
        const double tvk = tf[k];
        num[c] += tvk * ab[o];
        den[c] += tvk * ab[plane + o];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int k = k0 + c;
    if (k < K) {
      const size_t o = ((size_t)s * 2 * K + k) * T + t;
      part[o] = num[c];
      part[o + (size_t)K * T] = den[c];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// spatial (nmf.py:785-806), the sums: per (f, k), A = sum_t V[k,t] P and C = sum_t V[k,t] Q over a t slice, packed.
// A workgroup takes kpb = SBLK / (2 M^2) bases of one (slice, f); one thread per (k, packed entry) adds its frames in
// ascending order.  There is no Tb factor: the reference has none.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SBLK) cv_spatial_sum_kernel(const double* __restrict__ V, const double* __restrict__ pq,
                                                              double* __restrict__ part, int MM2, int T, int K, int S,
                                                              int kpb) {
  const int s = blockIdx.x, f = blockIdx.z, tid = threadIdx.x;
  const int kk = tid / MM2, e = tid % MM2, k = blockIdx.y * kpb + kk;
  if (kk >= kpb || k >= K) return;
  const int tiles = (T + WAVE - 1) / WAVE;
  const int t_lo = (int)((long long)tiles * s / S) * WAVE;
  int t_hi = (int)((long long)tiles * (s + 1) / S) * WAVE;
  if (t_hi > T) t_hi = T;
  const double* p = pq + (size_t)f * T * MM2 + e;
  const double* v = V + (size_t)k * T;
  double acc = 0.0;
  for (int t = t_lo; t < t_hi; ++t) acc += v[t] * p[(size_t)t * MM2];
  part[(((size_t)f * S + s) * K + k) * MM2 + e] = acc;
}

// spatial, second half: one thread per (f, k).  A, C summed over the slices in order; B = H C H; H A H = B solved in
// closed form (A exactly 0 -> H = 0; a failed Cholesky of A sets the singular status); + eps I; / trace.  The body up to
// "+ eps I" is mn_riccati_kernel's (assx_mnmf.hip) but for the indexing; see there why it is not one function.
template <int M>
__global__ void __launch_bounds__(WAVE) cv_riccati_kernel(Cx<double>* __restrict__ H, const double* __restrict__ part,
                                                          int normalize, double eps, int32_t* __restrict__ status,
                                                          int F, int K, int S) {
  constexpr int MM = M * M;
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i >= F * K) return;
  const int k = i % K, f = i / K;
  double pa[MM], pc[MM];
#pragma unroll
  for (int e = 0; e < MM; ++e) pa[e] = 0.0, pc[e] = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* p = part + (((size_t)f * S + s) * K + k) * 2 * MM;
#pragma unroll
    for (int e = 0; e < MM; ++e) pa[e] += p[e], pc[e] += p[MM + e];
  }
  Mat<M> A, C, Ho, Bm, T1;
  herm::unpack_herm<M>(pa, A);
  herm::unpack_herm<M>(pc, C);
  Cx<double>* Hp = H + (size_t)i * MM;
#pragma unroll
  for (int r = 0; r < M; ++r)
#pragma unroll
    for (int c = 0; c < M; ++c) {
      const Cx<double> h = Hp[r * M + c];
      Ho.re[r][c] = h.x, Ho.im[r][c] = h.y;
    }
  herm::matmul(Ho, C, T1);
  herm::matmul(T1, Ho, Bm);
  herm::hermitize(Bm);
  Mat<M>& Hn = C;
  const int rc = herm::herm_riccati(A, Bm, Hn);
  if (rc < 0 && status) atomicOr(status, (int32_t)ASSX_STATUS_SINGULAR);
#pragma unroll
  for (int m = 0; m < M; ++m) Hn.re[m][m] += eps;
  double sc = 1.0;
  if (normalize) {
    double tr = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) tr += Hn.re[m][m];
    sc = 1.0 / tr;
  }
#pragma unroll
  for (int r = 0; r < M; ++r)
#pragma unroll
    for (int c = 0; c < M; ++c) Hp[r * M + c] = Cx<double>{Hn.re[r][c] * sc, Hn.im[r][c] * sc};
}

// X^ (F,T,M,M) = sum_k (Tb[f,k] V[k,t]) H[f,k], one thread per entry, k ascending
__global__ void __launch_bounds__(BLK) cv_reconstruct_kernel(const double* __restrict__ Tb, const double* __restrict__ V,
                                                             const Cx<double>* __restrict__ H, Cx<double>* __restrict__ Xh,
                                                             int MM, int T, int K, size_t total) {
  const size_t idx = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (idx >= total) return;
  const int e = (int)(idx % MM);
  const size_t ft = idx / MM;
  const int t = (int)(ft % T);
  const size_t f = ft / T;
  double sr = 0.0, si = 0.0;
  for (int k = 0; k < K; ++k) {
    const double w = Tb[f * K + k] * V[(size_t)k * T + t];
    const Cx<double> h = H[(f * K + k) * MM + e];
    sr += w * h.x, si += w * h.y;
  }
  Xh[idx] = Cx<double>{sr, si};
}

// the context and the sizes of every entry point
int cv_check(assx_ctx* ctx, int M, int F, int T, int K, int dtype) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, F >= 1 && T >= 1, ASSX_E_ARG, "invalid sizes F=%d T=%d", F, T);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64 || dtype == ASSX_F32, ASSX_E_ARG, "bad dtype %d", dtype);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64, ASSX_E_UNSUPPORTED, "covariance-domain MNMF: float64 only");
  ASSX_REQUIRE(ctx, M >= 2 && M <= 8, ASSX_E_UNSUPPORTED, "covariance-domain MNMF: n_channels must be in [2, 8], got %d",
               M);
  ASSX_REQUIRE(ctx, K >= 1 && K <= KMAX, ASSX_E_UNSUPPORTED, "covariance-domain MNMF: n_basis must be in [1, 64], got %d",
               K);
  ASSX_REQUIRE(ctx, cv_in_envelope(M, F, T, K, dtype), ASSX_E_UNSUPPORTED,
               "covariance-domain MNMF: the target must stay below 4 GiB in complex128 (M*M*F*T < 2^28)");
  return 0;
}

// the evaluation pass in mode MODE over the whole target
template <int MODE>
int cv_eval(assx_ctx* ctx, const char* where, const void* X, const void* Tb, const void* V, const void* H, double eps,
            int32_t* status, void* ws, int M, int F, int T, int K, hipStream_t st) {
  const CvLayout L = cv_layout(M, F, T, K);
  return dispatch_channels(ctx, "covariance-domain MNMF", M, [&](auto mt) -> int {
    constexpr int MC = decltype(mt)::value;
    hipLaunchKernelGGL((cv_eval_kernel<MC, MODE>), dim3(nblocks(T, EBLK), F), dim3(EBLK), 0, st, (const Cx<double>*)X,
                       (const double*)Tb, (const double*)V, (const Cx<double>*)H, eps, (double*)((char*)ws + L.ab),
                       (double*)((char*)ws + L.pq), (double*)((char*)ws + L.lpart), status, F, T, K);
    ASSX_LAUNCH_CHECK(ctx, where);
    return 0;
  });
}

#define CV_ARGS_OK(name) ASSX_REQUIRE(ctx, X && Tb && V && H && ws, ASSX_E_NULL, name ": NULL array")

}  // namespace

extern "C" {

size_t assx_covnmf_workspace_bytes(int M, int F, int T, int K, int dtype) {
  if (!cv_in_envelope(M, F, T, K, dtype)) return 0;
  return cv_layout(M, F, T, K).total;
}

int assx_covnmf_update_basis(assx_ctx* ctx, const void* X, void* Tb, const void* V, const void* H, double eps,
                             int32_t* status, void* ws, int M, int F, int T, int K, int dtype, void* stream) {
  int rc = cv_check(ctx, M, F, T, K, dtype);
  if (rc) return rc;
  CV_ARGS_OK("assx_covnmf_update_basis");
  hipStream_t st = (hipStream_t)stream;
  rc = cv_eval<MODE_AB>(ctx, "cv_eval_kernel<ab>", X, Tb, V, H, eps, status, ws, M, F, T, K, st);
  if (rc) return rc;
  const CvLayout L = cv_layout(M, F, T, K);
  hipLaunchKernelGGL(cv_basis_kernel, dim3(F), dim3(BLK), 0, st, (double*)Tb, (const double*)V,
                     (const double*)((char*)ws + L.ab), eps, F, T, K);
  ASSX_LAUNCH_CHECK(ctx, "cv_basis_kernel");
  return 0;
}

int assx_covnmf_update_activation(assx_ctx* ctx, const void* X, const void* Tb, void* V, const void* H, double eps,
                                  int32_t* status, void* ws, int M, int F, int T, int K, int dtype, void* stream) {
  int rc = cv_check(ctx, M, F, T, K, dtype);
  if (rc) return rc;
  CV_ARGS_OK("assx_covnmf_update_activation");
  hipStream_t st = (hipStream_t)stream;
  rc = cv_eval<MODE_AB>(ctx, "cv_eval_kernel<ab>", X, Tb, V, H, eps, status, ws, M, F, T, K, st);
  if (rc) return rc;
  const CvLayout L = cv_layout(M, F, T, K);
  const int FS = act_slices(F), nchunk = (K + CH - 1) / CH;
  double* part = (double*)((char*)ws + L.actp);
  hipLaunchKernelGGL(cv_act_partial_kernel, dim3(nblocks(T, ABLK), FS, nchunk), dim3(ABLK), 0, st, (const double*)Tb,
                     (const double*)((char*)ws + L.ab), part, F, T, K, FS);
  ASSX_LAUNCH_CHECK(ctx, "cv_act_partial_kernel");
  const size_t total = (size_t)K * T;
  hipLaunchKernelGGL(act_apply_kernel<double>, dim3(nblocks(total, BLK)), dim3(BLK), 0, st, (double*)V,
                     (const double*)part, eps, K, T, FS, total);
  ASSX_LAUNCH_CHECK(ctx, "act_apply_kernel");
  return 0;
}

int assx_covnmf_update_spatial(assx_ctx* ctx, const void* X, const void* Tb, const void* V, void* H, int normalize,
                               double eps, int32_t* status, void* ws, int M, int F, int T, int K, int dtype,
                               void* stream) {
  int rc = cv_check(ctx, M, F, T, K, dtype);
  if (rc) return rc;
  CV_ARGS_OK("assx_covnmf_update_spatial");
  ASSX_REQUIRE(ctx, normalize == 0 || normalize == 1, ASSX_E_ARG, "normalize must be 0 or 1, got %d", normalize);
  hipStream_t st = (hipStream_t)stream;
  rc = cv_eval<MODE_PQ>(ctx, "cv_eval_kernel<pq>", X, Tb, V, H, eps, status, ws, M, F, T, K, st);
  if (rc) return rc;
  const CvLayout L = cv_layout(M, F, T, K);
  const int S = sp_slices(T), MM2 = 2 * M * M, kpb = SBLK / MM2;
  double* part = (double*)((char*)ws + L.spp);
  hipLaunchKernelGGL(cv_spatial_sum_kernel, dim3(S, (K + kpb - 1) / kpb, F), dim3(SBLK), 0, st, (const double*)V,
                     (const double*)((char*)ws + L.pq), part, MM2, T, K, S, kpb);
  ASSX_LAUNCH_CHECK(ctx, "cv_spatial_sum_kernel");
  return dispatch_channels(ctx, "covariance-domain MNMF", M, [&](auto mt) -> int {
    constexpr int MC = decltype(mt)::value;
    hipLaunchKernelGGL((cv_riccati_kernel<MC>), dim3(nblocks((size_t)F * K, WAVE)), dim3(WAVE), 0, st, (Cx<double>*)H,
                       (const double*)part, normalize, eps, status, F, K, S);
    ASSX_LAUNCH_CHECK(ctx, "cv_riccati_kernel");
    return 0;
  });
}

int assx_covnmf_reconstruct(assx_ctx* ctx, const void* Tb, const void* V, const void* H, void* Xh, int M, int F, int T,
                            int K, int dtype, void* stream) {
  int rc = cv_check(ctx, M, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, Tb && V && H && Xh, ASSX_E_NULL, "assx_covnmf_reconstruct: NULL array");
  const size_t total = (size_t)F * T * M * M;
  hipLaunchKernelGGL(cv_reconstruct_kernel, dim3(nblocks(total, BLK)), dim3(BLK), 0, (hipStream_t)stream,
                     (const double*)Tb, (const double*)V, (const Cx<double>*)H, (Cx<double>*)Xh, M * M, T, K, total);
  ASSX_LAUNCH_CHECK(ctx, "cv_reconstruct_kernel");
  return 0;
}

int assx_covnmf_loss(assx_ctx* ctx, const void* X, const void* Tb, const void* V, const void* H, double eps, double* loss,
                     int32_t* status, void* ws, int M, int F, int T, int K, int dtype, void* stream) {
  int rc = cv_check(ctx, M, F, T, K, dtype);
  if (rc) return rc;
  CV_ARGS_OK("assx_covnmf_loss");
  ASSX_REQUIRE(ctx, loss, ASSX_E_NULL, "assx_covnmf_loss: NULL loss");
  hipStream_t st = (hipStream_t)stream;
  rc = cv_eval<MODE_LOSS>(ctx, "cv_eval_kernel<loss>", X, Tb, V, H, eps, status, ws, M, F, T, K, st);
  if (rc) return rc;
  const CvLayout L = cv_layout(M, F, T, K);
  hipLaunchKernelGGL(cv_loss_finalize_kernel, dim3(1), dim3(BLK), 0, st, (const double*)((char*)ws + L.lpart), loss,
                     (size_t)F * nblocks(T, EBLK));
  ASSX_LAUNCH_CHECK(ctx, "cv_loss_finalize_kernel");
  return 0;
}

int assx_covnmf_iterate(assx_ctx* ctx, int n_iter, int normalize, const void* X, void* Tb, void* V, void* H, double eps,
                        double* loss, int32_t* status, void* ws, int M, int F, int T, int K, int dtype, void* stream) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, n_iter >= 0, ASSX_E_ARG, "n_iter must be >= 0, got %d", n_iter);
  // per iteration the three updates and loss[i]: the same entry points, in the same order, as the host loop
  int rc = cv_check(ctx, M, F, T, K, dtype);
  if (rc) return rc;
  CV_ARGS_OK("assx_covnmf_iterate");
  ASSX_REQUIRE(ctx, normalize == 0 || normalize == 1, ASSX_E_ARG, "normalize must be 0 or 1, got %d", normalize);
  for (int i = 0; i < n_iter; ++i) {
    rc = assx_covnmf_update_basis(ctx, X, Tb, V, H, eps, status, ws, M, F, T, K, dtype, stream);
    if (!rc) rc = assx_covnmf_update_activation(ctx, X, Tb, V, H, eps, status, ws, M, F, T, K, dtype, stream);
    if (!rc) rc = assx_covnmf_update_spatial(ctx, X, Tb, V, H, normalize, eps, status, ws, M, F, T, K, dtype, stream);
    if (!rc && loss) rc = assx_covnmf_loss(ctx, X, Tb, V, H, eps, loss + i, status, ws, M, F, T, K, dtype, stream);
    if (rc) return rc;
  }
  return 0;
}

}  // extern "C"
