// MultichannelISNMF (Sawada's full-rank MNMF, src/bss/mnmf.py:115-617) on MI355X: the whole iteration on the device.
//
// State (leading utterance axis B, float64):  X (B,M,F,T) complex, Tb (B,F,K) basis, V (B,K,T) activation, Z (B,N,K)
// latent, H (B,F,N,M,M) complex spatial.  With lam_n[f,t] = sum_k Z[n,k] Tb[f,k] V[k,t], X^ = sum_n lam_n H_n and
// P = (X^ + eps I)^{-1}, the reference's P x x^H P has rank one, so each of its traces is one of two reals per source:
// a_n = y^H H_n y (y = P x) and b_n = tr(P H_n).  One iteration (update_once_sawada) is a fixed list of launches; every
// step re-forms X^ from the parameters as they stand:
//
//   basis       mn_eval_kernel<AB> -> a, b (B,N,F,T);  mn_basis_kernel    one workgroup per (b, f), reduce over t
//   activation  mn_eval_kernel<AB>;  mn_act_partial_kernel (t block, f slice, b x k chunk);  act_apply_kernel
//   latent      mn_eval_kernel<AB>;  mn_latent_partial_kernel per (b, f);  mn_latent_sum_kernel per (b, n, k) (one wave
//               sums the bins in a fixed order);  mn_latent_apply_kernel per b (the update, then the normalisation over n)
//   spatial     mn_spatial_partial_kernel (t slice, f, b): one wave recomputes P, y, lam for 64 frames at a time and
//               sums lam P and lam y y^H per (f, n) through LDS;  mn_riccati_kernel per (b, f, n): B = H C H, H A H = B
//               by the closed form of assx_herm_linalg.hpp (H = 0 where A is exactly 0), + eps I, / trace
//   loss        mn_eval_kernel<LOSS> (per workgroup partials);  batch_sum_kernel per b
//   separate    mn_eval_kernel<SEP>: Y (B,N,F,T) = lam_n (H_n y)[ref]
//
// P is never materialised: it is recomputed in registers wherever it is needed.  Every reduction has a fixed order
// (wave butterflies, then the waves of a workgroup in index order, then slices in index order; no float atomics), and
// no partition depends on B: two runs give the same bits, a batch gives the bits of its single-utterance calls.
// One lane works on one (f, t) point for every M.  At M = 7, 8 the evaluation kernels hold part of their matrices in
// AGPRs; only the per-(f, n) Riccati kernels use scratch, from M = 6 on (profiles/mnmf_kernel_resource_usage.md).
#include "assx_common.hpp"
#include "assx_herm_linalg.hpp"
#include "assx_factor_common.hpp"

using namespace assx;
using namespace assx::mf;
using herm::Mat;

namespace {

constexpr int EBLK = 128;    // threads (frames) of an evaluation workgroup
constexpr int MODE_AB = 1, MODE_LOSS = 2, MODE_SEP = 3;

struct MnLayout {
  size_t ab, actp, latp, spp, lpart, total;
};

// ab: a and b (2,B,N,F,T); actp: activation slice partials (B,FS,2,K,T); latp: latent per-bin partials (B,F,2,N*K);
// spp: spatial slice partials (B,F,S,N,2*M*M); lpart: loss partials (B,F,nblocks(T, EBLK)).  All float64.
MnLayout mn_layout(int B, int M, int N, int F, int T, int K) {
  const size_t d = sizeof(double);
  Carve c(256);
  MnLayout L;
  L.ab = c.take((size_t)2 * B * N * F * T * d);
  L.actp = c.take((size_t)B * act_slices(F) * 2 * K * T * d);
  L.latp = c.take((size_t)B * F * 2 * N * K * d);
  L.spp = c.take((size_t)B * F * sp_slices(T) * N * 2 * M * M * d);
  L.lpart = c.take((size_t)B * F * nblocks(T, EBLK) * d);
  L.total = c.total();
  return L;
}

// the bin's model in LDS: zt[n*K + k] = Z[n,k] Tb[f,k]; hr/hi[(n*M + i)*M + j] = H[f,n,i,j]
template <int M>
__device__ __forceinline__ void load_bin(const double* __restrict__ Tb, const double* __restrict__ Z,
                                         const Cx<double>* __restrict__ H, int b, int f, int N, int F, int K, double* zt,
                                         double* hr, double* hi) {
  for (int i = threadIdx.x; i < N * K; i += blockDim.x)
    zt[i] = Z[(size_t)b * N * K + i] * Tb[((size_t)b * F + f) * K + i % K];
  const Cx<double>* Hf = H + ((size_t)b * F + f) * N * M * M;
  for (int i = threadIdx.x; i < N * M * M; i += blockDim.x) {
    const Cx<double> h = Hf[i];
    hr[i] = h.x, hi[i] = h.y;
  }
}

// lam_n at frame t and the lower triangle of X^ = sum_n lam_n H_n
template <int M>
__device__ __forceinline__ void model_point(const double* zt, const double* hr, const double* hi,
                                            const double* __restrict__ Vb, int N, int K, int T, int t,
                                            double (&lam)[NMAX], Mat<M>& Xh) {
#pragma unroll
  for (int n = 0; n < NMAX; ++n) lam[n] = 0.0;
  for (int k = 0; k < K; ++k) {
    const double v = Vb[(size_t)k * T + t];
#pragma unroll
    for (int n = 0; n < NMAX; ++n)
      if (n < N) lam[n] += zt[n * K + k] * v;
  }
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double sr = 0.0, si = 0.0;
#pragma unroll
      for (int n = 0; n < NMAX; ++n)
        if (n < N) {
          sr += lam[n] * hr[(n * M + i) * M + j];
          si += lam[n] * hi[(n * M + i) * M + j];
        }
      Xh.re[i][j] = sr, Xh.im[i][j] = si;
    }
}

// P = (X^ + eps I)^{-1} (lower triangle) and y = P x from the lower triangle of X^; false if the Cholesky fails
template <int M>
__device__ __forceinline__ bool solve_point(Mat<M>& Xh, double eps, const double (&xr)[M], const double (&xi)[M],
                                            Mat<M>& P, double (&yr)[M], double (&yi)[M]) {
#pragma unroll
  for (int i = 0; i < M; ++i) Xh.re[i][i] += eps;
  const bool ok = herm::herm_cholesky(Xh);
  Mat<M>& Li = P;  // L^{-1} first, then P = L^{-H} L^{-1} built from it in a second matrix
  herm::tri_inverse(Xh, Li);
  Mat<M>& Q = Xh;  // L is dead: Q = P, lower triangle
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
      Q.re[i][j] = sr, Q.im[i][j] = si;
    }
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) P.re[i][j] = Q.re[i][j], P.im[i][j] = Q.im[i][j];
  herm::mirror_lower(P);
#pragma unroll
  for (int i = 0; i < M; ++i) {
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      sr += P.re[i][j] * xr[j] - P.im[i][j] * xi[j];
      si += P.re[i][j] * xi[j] + P.im[i][j] * xr[j];
    }
    yr[i] = sr, yi[i] = si;
  }
  return ok;
}

// ---------------------------------------------------------------------------------------------------------------
// The evaluation pass, one thread per (b, f, t):
//   AB    a_n = y^H H_n y and b_n = tr(P H_n) into ab (2,B,N,F,T)
//   LOSS  the closed form of the reference's log-det divergence, one partial per workgroup
//   SEP   Y[b,n,f,t] = lam_n (H_n y)[ref]
// ---------------------------------------------------------------------------------------------------------------
template <int M, int MODE>
__global__ void __launch_bounds__(EBLK) mn_eval_kernel(const Cx<double>* __restrict__ X, const double* __restrict__ Tb,
                                                       const double* __restrict__ V, const double* __restrict__ Z,
                                                       const Cx<double>* __restrict__ H, double eps,
                                                       double* __restrict__ ab, double* __restrict__ lpart,
                                                       Cx<double>* __restrict__ Y, int ref, int32_t* __restrict__ status,
                                                       int B, int N, int F, int T, int K) {
  __shared__ double zt[NMAX * KMAX];
  __shared__ double hr[NMAX * M * M], hi[NMAX * M * M];
  __shared__ double red[EBLK / WAVE];
  const int f = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int t = blockIdx.x * EBLK + tid;
  load_bin<M>(Tb, Z, H, b, f, N, F, K, zt, hr, hi);
  __syncthreads();
  const size_t FT = (size_t)F * T;
  double term = 0.0;
  if (t < T) {
    double xr[M], xi[M];
    const Cx<double>* Xb = X + (size_t)b * M * FT + (size_t)f * T + t;
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const Cx<double> v = Xb[m * FT];
      xr[m] = v.x, xi[m] = v.y;
    }
    double lam[NMAX];
    Mat<M> Xh;
    model_point<M>(zt, hr, hi, V + (size_t)b * K * T, N, K, T, t, lam, Xh);
    if constexpr (MODE == MODE_LOSS) {
      // X' = X^ + (eps tr X^ + eps) I;  c = eps |x|^2 + eps
      double tr = 0.0, n2 = 0.0;
#pragma unroll
      for (int m = 0; m < M; ++m) tr += Xh.re[m][m], n2 += xr[m] * xr[m] + xi[m] * xi[m];
      const double shift = eps * tr + eps, c = eps * n2 + eps;
#pragma unroll
      for (int m = 0; m < M; ++m) Xh.re[m][m] += shift;
      if (!herm::herm_cholesky(Xh) && status) atomicOr(status + b, (int32_t)ASSX_STATUS_SINGULAR);
      Mat<M> Li;
      herm::tri_inverse(Xh, Li);
      double quad = 0.0, trinv = 0.0, ldet = 0.0;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        ldet += log(Xh.re[i][i]);
        double zr = 0.0, zi = 0.0;  // (L^{-1} x)_i
#pragma unroll
        for (int j = 0; j <= i; ++j) {
          zr += Li.re[i][j] * xr[j] - Li.im[i][j] * xi[j];
          zi += Li.re[i][j] * xi[j] + Li.im[i][j] * xr[j];
          trinv += Li.re[i][j] * Li.re[i][j] + Li.im[i][j] * Li.im[i][j];
        }
        quad += zr * zr + zi * zi;
      }
      term = quad + c * trinv - (double)(M - 1) * log(c) - log(n2 + c) + 2.0 * ldet - (double)M;
    } else {
      Mat<M> P;
      double yr[M], yi[M];
      if (!solve_point<M>(Xh, eps, xr, xi, P, yr, yi) && status) atomicOr(status + b, (int32_t)ASSX_STATUS_SINGULAR);
#pragma unroll
      for (int n = 0; n < NMAX; ++n) {
        if (n >= N) continue;
        const double* Hr = hr + n * M * M;
        const double* Hi = hi + n * M * M;
        if constexpr (MODE == MODE_AB) {
          double an = 0.0, bn = 0.0;
#pragma unroll
          for (int i = 0; i < M; ++i) {
            double ur = 0.0, ui = 0.0;  // (H_n y)_i
#pragma unroll
            for (int j = 0; j < M; ++j) {
              ur += Hr[i * M + j] * yr[j] - Hi[i * M + j] * yi[j];
              ui += Hr[i * M + j] * yi[j] + Hi[i * M + j] * yr[j];
            }
            an += yr[i] * ur + yi[i] * ui;
            bn += P.re[i][i] * Hr[i * M + i];
#pragma unroll
            for (int j = 0; j < i; ++j) bn += 2.0 * (P.re[i][j] * Hr[i * M + j] + P.im[i][j] * Hi[i * M + j]);
          }
          const size_t o = (((size_t)b * N + n) * F + f) * T + t;
          ab[o] = an;
          ab[(size_t)B * N * FT + o] = bn;
        } else {
          double ur = 0.0, ui = 0.0;
#pragma unroll
          for (int j = 0; j < M; ++j) {
            ur += Hr[ref * M + j] * yr[j] - Hi[ref * M + j] * yi[j];
            ui += Hr[ref * M + j] * yi[j] + Hi[ref * M + j] * yr[j];
          }
          Y[(((size_t)b * N + n) * F + f) * T + t] = Cx<double>{lam[n] * ur, lam[n] * ui};
        }
      }
    }
  }
  if constexpr (MODE == MODE_LOSS) {
    const double s = block_sum<double, EBLK / WAVE>(term, red);
    if (tid == 0) lpart[((size_t)b * F + f) * gridDim.x + blockIdx.x] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// basis (mnmf.py:431-451): per (b, f) and k, num = sum_t V[k,t] sum_n Z[n,k] a_n, den the same with b_n;
// Tb[f,k] *= sqrt(num / den) with den < eps -> eps.  The k are taken CH at a time.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLK) mn_basis_kernel(double* __restrict__ Tb, const double* __restrict__ V,
                                                       const double* __restrict__ Z, const double* __restrict__ ab,
                                                       double eps, int B, int N, int F, int T, int K) {
  __shared__ double zs[NMAX * KMAX];
  __shared__ double red[BLK / WAVE][2 * CH];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  for (int i = tid; i < N * K; i += BLK) zs[i] = Z[(size_t)b * N * K + i];
  __syncthreads();
  const size_t FT = (size_t)F * T, plane = (size_t)B * N * FT;
  const double* a = ab + (size_t)b * N * FT + (size_t)f * T;
  const double* bb = a + plane;
  const double* Vb = V + (size_t)b * K * T;
  for (int k0 = 0; k0 < K; k0 += CH) {
    double num[CH], den[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) num[c] = 0.0, den[c] = 0.0;
    for (int t = tid; t < T; t += BLK) {
      double an[NMAX], bn[NMAX];
#pragma unroll
      for (int n = 0; n < NMAX; ++n) {
        an[n] = n < N ? a[n * FT + t] : 0.0;
        bn[n] = n < N ? bb[n * FT + t] : 0.0;
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int k = k0 + c;
        if (k < K) {
          double sa = 0.0, sb = 0.0;
#pragma unroll
          for (int n = 0; n < NMAX; ++n)
            if (n < N) sa += zs[n * K + k] * an[n], sb += zs[n * K + k] * bn[n];
          const double v = Vb[(size_t)k * T + t];
          num[c] += v * sa;
          den[c] += v * sb;
        }
      }
    }
    double sn, sd;
    block_pair_sums<double, BLK / WAVE>(num, den, red, sn, sd);
    if (tid < CH && k0 + tid < K) {
      if (sd < eps) sd = eps;
      double* tp = Tb + ((size_t)b * F + f) * K + k0 + tid;
      *tp = *tp * sqrt(sn / sd);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------
// activation (mnmf.py:453-473): num[k,t] = sum_f Tb[f,k] sum_n Z[n,k] a_n over an f slice per workgroup (partials
// (B,FS,2,K,T)), then the slices summed in ascending order and V *= sqrt(num / den), den < eps -> eps.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(ABLK) mn_act_partial_kernel(const double* __restrict__ Tb, const double* __restrict__ Z,
                                                              const double* __restrict__ ab, double* __restrict__ part,
                                                              int B, int N, int F, int T, int K, int FS, int nchunk) {
  __shared__ double zs[NMAX * KMAX];
  const int t = blockIdx.x * ABLK + threadIdx.x, s = blockIdx.y;
  const int b = blockIdx.z / nchunk, k0 = (blockIdx.z % nchunk) * CH;
  for (int i = threadIdx.x; i < N * K; i += ABLK) zs[i] = Z[(size_t)b * N * K + i];
  __syncthreads();
  if (t >= T) return;
  const int f0 = (int)((long long)F * s / FS), f1 = (int)((long long)F * (s + 1) / FS);
  const size_t FT = (size_t)F * T, plane = (size_t)B * N * FT;
  double num[CH], den[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) num[c] = 0.0, den[c] = 0.0;
  for (int f = f0; f < f1; ++f) {
    double an[NMAX], bn[NMAX];
#pragma unroll
    for (int n = 0; n < NMAX; ++n) {
      const size_t o = (((size_t)b * N + n) * F + f) * T + t;
      an[n] = n < N ? ab[o] : 0.0;
      bn[n] = n < N ? ab[plane + o] : 0.0;
    }
    const double* tf = Tb + ((size_t)b * F + f) * K;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int k = k0 + c;
      if (k < K) {
        double sa = 0.0, sb = 0.0;
#pragma unroll
        for (int n = 0; n < NMAX; ++n)
          if (n < N) sa += zs[n * K + k] * an[n], sb += zs[n * K + k] * bn[n];
        const double tv = tf[k];
        num[c] += tv * sa;
        den[c] += tv * sb;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const int k = k0 + c;
    if (k < K) {
      const size_t o = (((size_t)b * FS + s) * 2 * K + k) * T + t;
      part[o] = num[c];
      part[o + (size_t)K * T] = den[c];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// latent (mnmf.py:475-497): per (b, f) and pair (n, k): sum_t Tb[f,k] V[k,t] a_n (and b_n) into (B,F,2,N*K); then per b
// the bins summed in ascending order, Z *= sqrt(num / den) (den < eps -> eps), Z /= sum_n Z (sum < eps -> eps).
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLK) mn_latent_partial_kernel(const double* __restrict__ Tb,
                                                                const double* __restrict__ V,
                                                                const double* __restrict__ ab, double* __restrict__ part,
                                                                int B, int N, int F, int T, int K) {
  __shared__ double red[BLK / WAVE][2 * CH];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const size_t FT = (size_t)F * T, plane = (size_t)B * N * FT;
  const double* tf = Tb + ((size_t)b * F + f) * K;
  const double* Vb = V + (size_t)b * K * T;
  const int NP = N * K;
  for (int p0 = 0; p0 < NP; p0 += CH) {
    double num[CH], den[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) num[c] = 0.0, den[c] = 0.0;
    for (int t = tid; t < T; t += BLK) {
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int p = p0 + c;
        if (p < NP) {
          const int n = p / K, k = p % K;
          const size_t o = (((size_t)b * N + n) * F + f) * T + t;
          const double tv = tf[k] * Vb[(size_t)k * T + t];
          num[c] += tv * ab[o];
          den[c] += tv * ab[plane + o];
        }
      }
    }
    double sn, sd;
    block_pair_sums<double, BLK / WAVE>(num, den, red, sn, sd);
    if (tid < CH && p0 + tid < NP) {
      const size_t o = ((size_t)b * F + f) * 2 * NP + p0 + tid;
      part[o] = sn;
      part[o + NP] = sd;
    }
    __syncthreads();
  }
}

// per (b, pair): the bins summed by one wave (lane l takes f = l, l + 64, ...; then a fixed butterfly) into the first
// F-row of the partials, which the apply kernel reads
__global__ void __launch_bounds__(WAVE) mn_latent_sum_kernel(double* __restrict__ part, int N, int F, int K) {
  const int p = blockIdx.x, b = blockIdx.y, lane = threadIdx.x, NP = N * K;
  double num = 0.0, den = 0.0;
  for (int f = lane; f < F; f += WAVE) {
    const size_t o = ((size_t)b * F + f) * 2 * NP + p;
    num += part[o];
    den += part[o + NP];
  }
  num = wave_sum_down(num);
  den = wave_sum_down(den);
  if (lane == 0) {  // row f = 0 of this pair was read by lane 0 itself
    const size_t o = (size_t)b * F * 2 * NP + p;
    part[o] = num;
    part[o + NP] = den;
  }
}

constexpr int LBLK = NMAX * KMAX;  // one thread per (n, k)

__global__ void __launch_bounds__(LBLK) mn_latent_apply_kernel(double* __restrict__ Z, const double* __restrict__ part,
                                                               double eps, int N, int F, int K) {
  __shared__ double zn[NMAX * KMAX];
  const int b = blockIdx.x, p = threadIdx.x, NP = N * K;
  if (p < NP) {
    const size_t o = (size_t)b * F * 2 * NP + p;
    const double num = part[o];
    double den = part[o + NP];
    if (den < eps) den = eps;
    zn[p] = Z[(size_t)b * NP + p] * sqrt(num / den);
  }
  __syncthreads();
  if (p < NP) {
    const int k = p % K;
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += zn[n * K + k];
    if (s < eps) s = eps;
    Z[(size_t)b * NP + p] = zn[p] / s;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// spatial (mnmf.py:499-525), first half: for each (f, n), A = sum_t lam_n P and C = sum_t lam_n y y^H over a t slice.
// One wave per (slice, f, b).  64 frames at a time: every lane evaluates its frame and leaves lam, P and y in LDS;
// then every lane sums its own targets (of N x 2 M^2) over the 64 frames in order.  A Hermitian matrix is packed into
// M^2 reals: entry (i, j) holds Re A_ij for i >= j and Im A_ji for i < j.
// ---------------------------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__(WAVE) mn_spatial_partial_kernel(const Cx<double>* __restrict__ X,
                                                                  const double* __restrict__ Tb,
                                                                  const double* __restrict__ V,
                                                                  const double* __restrict__ Z,
                                                                  const Cx<double>* __restrict__ H, double eps,
                                                                  double* __restrict__ part,
                                                                  int32_t* __restrict__ status, int N, int F, int T,
                                                                  int K, int S) {
  constexpr int MM = M * M;
  constexpr int NT = NMAX * 2 * MM;        // targets at N = NMAX
  constexpr int RT = (NT + WAVE - 1) / WAVE;  // targets per lane
  __shared__ double zt[NMAX * KMAX];
  __shared__ double hr[NMAX * MM], hi[NMAX * MM];
  __shared__ double lamL[NMAX][WAVE];
  __shared__ double pL[MM][WAVE];
  __shared__ double yL[2 * M][WAVE];
  const int s = blockIdx.x, f = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  load_bin<M>(Tb, Z, H, b, f, N, F, K, zt, hr, hi);
  const int tiles = (T + WAVE - 1) / WAVE;
  const int tile0 = (int)((long long)tiles * s / S), tile1 = (int)((long long)tiles * (s + 1) / S);
  const size_t FT = (size_t)F * T;
  const Cx<double>* Xb = X + (size_t)b * M * FT + (size_t)f * T;
  const double* Vb = V + (size_t)b * K * T;
  const int ntarget = N * 2 * MM;
  double acc[RT];
#pragma unroll
  for (int r = 0; r < RT; ++r) acc[r] = 0.0;
  __syncthreads();
  for (int tile = tile0; tile < tile1; ++tile) {
    const int t = tile * WAVE + lane;
    double lam[NMAX];
    Mat<M> P;
    double yr[M], yi[M];
    if (t < T) {
      double xr[M], xi[M];
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const Cx<double> v = Xb[m * FT + t];
        xr[m] = v.x, xi[m] = v.y;
      }
      Mat<M> Xh;
      model_point<M>(zt, hr, hi, Vb, N, K, T, t, lam, Xh);
      if (!solve_point<M>(Xh, eps, xr, xi, P, yr, yi) && status) atomicOr(status + b, (int32_t)ASSX_STATUS_SINGULAR);
    } else {
#pragma unroll
      for (int n = 0; n < NMAX; ++n) lam[n] = 0.0;
      herm::set_zero(P);
#pragma unroll
      for (int m = 0; m < M; ++m) yr[m] = 0.0, yi[m] = 0.0;
    }
#pragma unroll
    for (int n = 0; n < NMAX; ++n) lamL[n][lane] = lam[n];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j < M; ++j) pL[i * M + j][lane] = i >= j ? P.re[i][j] : P.im[j][i];
#pragma unroll
    for (int m = 0; m < M; ++m) yL[m][lane] = yr[m], yL[M + m][lane] = yi[m];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RT; ++r) {
      const int j = r * WAVE + lane;
      if (j < ntarget) {
        const int n = j / (2 * MM), e = j % (2 * MM);
        double sum = 0.0;
        if (e < MM) {
          for (int q = 0; q < WAVE; ++q) sum += lamL[n][q] * pL[e][q];
        } else {
          const int ee = e - MM, ii = ee / M, jj = ee % M;
          const int p = ii >= jj ? ii : jj, c = ii >= jj ? jj : ii;  // the lower entry (p, c) of y y^H
          for (int q = 0; q < WAVE; ++q) {
            const double pr = yL[p][q], pi = yL[M + p][q], cr = yL[c][q], ci = yL[M + c][q];
            // y_p conj(y_c)
            const double v = ii >= jj ? pr * cr + pi * ci : pi * cr - pr * ci;
            sum += lamL[n][q] * v;
          }
        }
        acc[r] += sum;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < RT; ++r) {
    const int j = r * WAVE + lane;
    if (j < ntarget) part[(((size_t)b * F + f) * S + s) * ntarget + j] = acc[r];
  }
}

// spatial, second half: one thread per (b, f, n).  A, C summed over the slices in order; B = H C H; H A H = B solved
// in closed form (A exactly 0 -> H = 0; a failed Cholesky of A sets the singular status); + eps I; / trace.  The body up
// to "+ eps I" is also cv_riccati_kernel's (assx_covnmf.hip), which indexes part and status differently: as one shared
// device function the M = 8 instance there spills more, so the two stay apart.
template <int M>
__global__ void __launch_bounds__(WAVE) mn_riccati_kernel(Cx<double>* __restrict__ H, const double* __restrict__ part,
                                                          int normalize, double eps, int32_t* __restrict__ status,
                                                          int B, int N, int F, int S) {
  constexpr int MM = M * M;
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i >= B * F * N) return;
  const int n = i % N, bf = i / N, b = bf / F;
  const int ntarget = N * 2 * MM;
  double pa[MM], pc[MM];
#pragma unroll
  for (int e = 0; e < MM; ++e) pa[e] = 0.0, pc[e] = 0.0;
  for (int s = 0; s < S; ++s) {
    const double* p = part + ((size_t)bf * S + s) * ntarget + (size_t)n * 2 * MM;
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
  if (rc < 0 && status) atomicOr(status + b, (int32_t)ASSX_STATUS_SINGULAR);
#pragma unroll
  for (int m = 0; m < M; ++m) Hn.re[m][m] += eps;
  double sr = 1.0, si = 0.0;
  if (normalize) {
    double tr = 0.0, ti = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m) tr += Hn.re[m][m], ti += Hn.im[m][m];
    const double d = tr * tr + ti * ti;  // 1 / trace
    sr = tr / d, si = -ti / d;
  }
#pragma unroll
  for (int r = 0; r < M; ++r)
#pragma unroll
    for (int c = 0; c < M; ++c)
      Hp[r * M + c] = Cx<double>{Hn.re[r][c] * sr - Hn.im[r][c] * si, Hn.re[r][c] * si + Hn.im[r][c] * sr};
}

// a batch of H A H = B (assx_hermitian_riccati), one thread per matrix
template <int M>
__global__ void __launch_bounds__(WAVE) mn_riccati_batch_kernel(const Cx<double>* __restrict__ A,
                                                                const Cx<double>* __restrict__ Bm,
                                                                Cx<double>* __restrict__ H, int32_t* __restrict__ status,
                                                                int n) {
  constexpr int MM = M * M;
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i >= n) return;
  Mat<M> a, bm, h;
#pragma unroll
  for (int r = 0; r < M; ++r)
#pragma unroll
    for (int c = 0; c < M; ++c) {
      const Cx<double> u = A[(size_t)i * MM + r * M + c], v = Bm[(size_t)i * MM + r * M + c];
      a.re[r][c] = u.x, a.im[r][c] = u.y, bm.re[r][c] = v.x, bm.im[r][c] = v.y;
    }
  const int rc = herm::herm_riccati(a, bm, h);
  if (status) status[i] = rc < 0 ? (int32_t)ASSX_STATUS_SINGULAR : 0;
#pragma unroll
  for (int r = 0; r < M; ++r)
#pragma unroll
    for (int c = 0; c < M; ++c) H[(size_t)i * MM + r * M + c] = Cx<double>{h.re[r][c], h.im[r][c]};
}

template <typename Fn>
int mn_dispatch(assx_ctx* ctx, int M, Fn&& fn) {
  return dispatch_channels(ctx, "MNMF", M, fn);
}

int mn_check(assx_ctx* ctx, int B, int M, int N, int F, int T, int K, int dtype) {
  return check_sizes(ctx, "MNMF", /*f64_only=*/true, B, M, N, F, T, K, dtype);
}

#define MN_ARGS_OK(name) \
  ASSX_REQUIRE(ctx, X && Tb && V && Z && H && ws, ASSX_E_NULL, name ": NULL array")

// the evaluation pass in AB mode: a, b of the current model into ws
int mn_eval_ab(assx_ctx* ctx, const void* X, const void* Tb, const void* V, const void* Z, const void* H, double eps,
               int32_t* status, void* ws, int B, int M, int N, int F, int T, int K, hipStream_t st) {
  const MnLayout L = mn_layout(B, M, N, F, T, K);
  return mn_dispatch(ctx, M, [&](auto mt) -> int {
    constexpr int MC = decltype(mt)::value;
    hipLaunchKernelGGL((mn_eval_kernel<MC, MODE_AB>), dim3(nblocks(T, EBLK), F, B), dim3(EBLK), 0, st,
                       (const Cx<double>*)X, (const double*)Tb, (const double*)V, (const double*)Z,
                       (const Cx<double>*)H, eps, (double*)((char*)ws + L.ab), nullptr, nullptr, 0, status, B, N, F,
                       T, K);
    ASSX_LAUNCH_CHECK(ctx, "mn_eval_kernel<ab>");
    return 0;
  });
}

}  // namespace

extern "C" {

size_t assx_mnmf_workspace_bytes(int B, int M, int N, int F, int T, int K, int dtype) {
  if (dtype != ASSX_F64 || B < 1 || M < 2 || M > 8 || N < 1 || N > NMAX || F < 1 || T < 1 || K < 1 || K > KMAX) return 0;
  return mn_layout(B, M, N, F, T, K).total;
}

int assx_mnmf_update_basis(assx_ctx* ctx, const void* X, void* Tb, const void* V, const void* Z, const void* H,
                           double eps, int32_t* status, void* ws, int B, int M, int N, int F, int T, int K, int dtype,
                           void* stream) {
  int rc = mn_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  MN_ARGS_OK("assx_mnmf_update_basis");
  hipStream_t st = (hipStream_t)stream;
  rc = mn_eval_ab(ctx, X, Tb, V, Z, H, eps, status, ws, B, M, N, F, T, K, st);
  if (rc) return rc;
  const MnLayout L = mn_layout(B, M, N, F, T, K);
  hipLaunchKernelGGL(mn_basis_kernel, dim3(F, B), dim3(BLK), 0, st, (double*)Tb, (const double*)V, (const double*)Z,
                     (const double*)((char*)ws + L.ab), eps, B, N, F, T, K);
  ASSX_LAUNCH_CHECK(ctx, "mn_basis_kernel");
  return 0;
}

int assx_mnmf_update_activation(assx_ctx* ctx, const void* X, const void* Tb, void* V, const void* Z, const void* H,
                                double eps, int32_t* status, void* ws, int B, int M, int N, int F, int T, int K,
                                int dtype, void* stream) {
  int rc = mn_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  MN_ARGS_OK("assx_mnmf_update_activation");
  hipStream_t st = (hipStream_t)stream;
  rc = mn_eval_ab(ctx, X, Tb, V, Z, H, eps, status, ws, B, M, N, F, T, K, st);
  if (rc) return rc;
  const MnLayout L = mn_layout(B, M, N, F, T, K);
  const int FS = act_slices(F), nchunk = (K + CH - 1) / CH;
  double* part = (double*)((char*)ws + L.actp);
  hipLaunchKernelGGL(mn_act_partial_kernel, dim3(nblocks(T, ABLK), FS, B * nchunk), dim3(ABLK), 0, st,
                     (const double*)Tb, (const double*)Z, (const double*)((char*)ws + L.ab), part, B, N, F, T, K, FS,
                     nchunk);
  ASSX_LAUNCH_CHECK(ctx, "mn_act_partial_kernel");
  const size_t total = (size_t)B * K * T;
  hipLaunchKernelGGL(act_apply_kernel<double>, dim3(nblocks(total, BLK)), dim3(BLK), 0, st, (double*)V,
                     (const double*)part, eps, K, T, FS, total);
  ASSX_LAUNCH_CHECK(ctx, "act_apply_kernel");
  return 0;
}

int assx_mnmf_update_latent(assx_ctx* ctx, const void* X, const void* Tb, const void* V, void* Z, const void* H,
                            double eps, int32_t* status, void* ws, int B, int M, int N, int F, int T, int K, int dtype,
                            void* stream) {
  int rc = mn_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  MN_ARGS_OK("assx_mnmf_update_latent");
  hipStream_t st = (hipStream_t)stream;
  rc = mn_eval_ab(ctx, X, Tb, V, Z, H, eps, status, ws, B, M, N, F, T, K, st);
  if (rc) return rc;
  const MnLayout L = mn_layout(B, M, N, F, T, K);
  double* part = (double*)((char*)ws + L.latp);
  hipLaunchKernelGGL(mn_latent_partial_kernel, dim3(F, B), dim3(BLK), 0, st, (const double*)Tb, (const double*)V,
                     (const double*)((char*)ws + L.ab), part, B, N, F, T, K);
  ASSX_LAUNCH_CHECK(ctx, "mn_latent_partial_kernel");
  hipLaunchKernelGGL(mn_latent_sum_kernel, dim3(N * K, B), dim3(WAVE), 0, st, part, N, F, K);
  ASSX_LAUNCH_CHECK(ctx, "mn_latent_sum_kernel");
  hipLaunchKernelGGL(mn_latent_apply_kernel, dim3(B), dim3(LBLK), 0, st, (double*)Z, (const double*)part, eps, N, F, K);
  ASSX_LAUNCH_CHECK(ctx, "mn_latent_apply_kernel");
  return 0;
}

int assx_mnmf_update_spatial(assx_ctx* ctx, const void* X, const void* Tb, const void* V, const void* Z, void* H,
                             int normalize, double eps, int32_t* status, void* ws, int B, int M, int N, int F, int T,
                             int K, int dtype, void* stream) {
  int rc = mn_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  MN_ARGS_OK("assx_mnmf_update_spatial");
  ASSX_REQUIRE(ctx, normalize == 0 || normalize == 1, ASSX_E_ARG, "normalize must be 0 or 1, got %d", normalize);
  hipStream_t st = (hipStream_t)stream;
  const MnLayout L = mn_layout(B, M, N, F, T, K);
  const int S = sp_slices(T);
  double* part = (double*)((char*)ws + L.spp);
  return mn_dispatch(ctx, M, [&](auto mt) -> int {
    constexpr int MC = decltype(mt)::value;
    hipLaunchKernelGGL((mn_spatial_partial_kernel<MC>), dim3(S, F, B), dim3(WAVE), 0, st, (const Cx<double>*)X,
                       (const double*)Tb, (const double*)V, (const double*)Z, (const Cx<double>*)H, eps, part, status,
                       N, F, T, K, S);
    ASSX_LAUNCH_CHECK(ctx, "mn_spatial_partial_kernel");
    hipLaunchKernelGGL((mn_riccati_kernel<MC>), dim3(nblocks((size_t)B * F * N, WAVE)), dim3(WAVE), 0, st,
                       (Cx<double>*)H, (const double*)part, normalize, eps, status, B, N, F, S);
    ASSX_LAUNCH_CHECK(ctx, "mn_riccati_kernel");
    return 0;
  });
}

int assx_mnmf_loss(assx_ctx* ctx, const void* X, const void* Tb, const void* V, const void* Z, const void* H,
                   double eps, double* loss, int32_t* status, void* ws, int B, int M, int N, int F, int T, int K,
                   int dtype, void* stream) {
  int rc = mn_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  MN_ARGS_OK("assx_mnmf_loss");
  ASSX_REQUIRE(ctx, loss, ASSX_E_NULL, "assx_mnmf_loss: NULL loss");
  hipStream_t st = (hipStream_t)stream;
  const MnLayout L = mn_layout(B, M, N, F, T, K);
  double* lpart = (double*)((char*)ws + L.lpart);
  const int tb = (int)nblocks(T, EBLK);
  return mn_dispatch(ctx, M, [&](auto mt) -> int {
    constexpr int MC = decltype(mt)::value;
    hipLaunchKernelGGL((mn_eval_kernel<MC, MODE_LOSS>), dim3(tb, F, B), dim3(EBLK), 0, st, (const Cx<double>*)X,
                       (const double*)Tb, (const double*)V, (const double*)Z, (const Cx<double>*)H, eps, nullptr, lpart,
                       nullptr, 0, status, B, N, F, T, K);
    ASSX_LAUNCH_CHECK(ctx, "mn_eval_kernel<loss>");
    hipLaunchKernelGGL(batch_sum_kernel<false>, dim3(B), dim3(BLK), 0, st, (const double*)lpart, loss, F * tb);
    ASSX_LAUNCH_CHECK(ctx, "batch_sum_kernel");
    return 0;
  });
}

int assx_mnmf_separate(assx_ctx* ctx, const void* X, const void* Tb, const void* V, const void* Z, const void* H,
                       int ref, double eps, void* Y, int32_t* status, int B, int M, int N, int F, int T, int K,
                       int dtype, void* stream) {
  int rc = mn_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && Tb && V && Z && H && Y, ASSX_E_NULL, "assx_mnmf_separate: NULL array");
  ASSX_REQUIRE(ctx, ref >= 0 && ref < M, ASSX_E_ARG, "reference_id must be in [0, %d), got %d", M, ref);
  hipStream_t st = (hipStream_t)stream;
  return mn_dispatch(ctx, M, [&](auto mt) -> int {
    constexpr int MC = decltype(mt)::value;
    hipLaunchKernelGGL((mn_eval_kernel<MC, MODE_SEP>), dim3(nblocks(T, EBLK), F, B), dim3(EBLK), 0, st,
                       (const Cx<double>*)X, (const double*)Tb, (const double*)V, (const double*)Z,
                       (const Cx<double>*)H, eps, nullptr, nullptr, (Cx<double>*)Y, ref, status, B, N, F, T, K);
    ASSX_LAUNCH_CHECK(ctx, "mn_eval_kernel<sep>");
    return 0;
  });
}

int assx_mnmf_iterate(assx_ctx* ctx, int n_iter, int normalize, const void* X, void* Tb, void* V, void* Z, void* H,
                      double eps, double* loss, int32_t* status, void* ws, int B, int M, int N, int F, int T, int K,
                      int dtype, void* stream) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, n_iter >= 0, ASSX_E_ARG, "n_iter must be >= 0, got %d", n_iter);
  // loss[0] of the entry model; then per iteration the four updates and loss[i + 1]: the same entry points, in the
  // same order, as the host loop
  int rc = 0;
  if (loss) rc = assx_mnmf_loss(ctx, X, Tb, V, Z, H, eps, loss, status, ws, B, M, N, F, T, K, dtype, stream);
  if (rc) return rc;
  for (int i = 0; i < n_iter; ++i) {
    rc = assx_mnmf_update_basis(ctx, X, Tb, V, Z, H, eps, status, ws, B, M, N, F, T, K, dtype, stream);
    if (!rc) rc = assx_mnmf_update_activation(ctx, X, Tb, V, Z, H, eps, status, ws, B, M, N, F, T, K, dtype, stream);
    if (!rc) rc = assx_mnmf_update_latent(ctx, X, Tb, V, Z, H, eps, status, ws, B, M, N, F, T, K, dtype, stream);
    if (!rc)
      rc = assx_mnmf_update_spatial(ctx, X, Tb, V, Z, H, normalize, eps, status, ws, B, M, N, F, T, K, dtype, stream);
    if (!rc && loss)
      rc = assx_mnmf_loss(ctx, X, Tb, V, Z, H, eps, loss + (size_t)(i + 1) * B, status, ws, B, M, N, F, T, K, dtype,
                          stream);
    if (rc) return rc;
  }
  return 0;
}

int assx_hermitian_riccati(assx_ctx* ctx, const void* A, const void* Bm, void* H, int32_t* status, int n, int M,
                           int dtype, void* stream) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, n >= 0, ASSX_E_ARG, "invalid batch n=%d", n);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64, ASSX_E_UNSUPPORTED, "assx_hermitian_riccati: float64 only");
  ASSX_REQUIRE(ctx, M >= 2 && M <= 8, ASSX_E_UNSUPPORTED, "assx_hermitian_riccati: M must be in [2, 8], got %d", M);
  if (n == 0) return 0;
  ASSX_REQUIRE(ctx, A && Bm && H, ASSX_E_NULL, "assx_hermitian_riccati: NULL array");
  hipStream_t st = (hipStream_t)stream;
  return mn_dispatch(ctx, M, [&](auto mt) -> int {
    constexpr int MC = decltype(mt)::value;
    hipLaunchKernelGGL((mn_riccati_batch_kernel<MC>), dim3(nblocks(n, WAVE)), dim3(WAVE), 0, st, (const Cx<double>*)A,
                       (const Cx<double>*)Bm, (Cx<double>*)H, status, n);
    ASSX_LAUNCH_CHECK(ctx, "mn_riccati_batch_kernel");
    return 0;
  });
}

}  // extern "C"
