// FastMultichannelISNMF (src/bss/mnmf.py:637-946) on MI355X: the whole iteration on the device.
//
// State (leading utterance axis B):  X (B,M,F,T) complex, Q (B,F,M,M) complex diagonalizer, W (B,N,F,K) basis,
// H (B,N,K,T) activation, g (B,N,F,M) spatial_covariance.  With  x~[f,t,m] = |(Q x)[m]|^2,  Lambda_n = W_n H_n  and
// R[f,t,m] = sum_n Lambda_n g[n,f,m], one iteration (update_once, mnmf.py:737-773) is a fixed list of launches:
//
//   P2  fm_bin_reduce_kernel<basis>   one workgroup per (b, f), reduce over t      W *= sqrt(num / max(den, eps))
//   P3  fm_act_partial_kernel          (t block, f slice, b x pair chunk), reduce over an f slice
//       act_apply_kernel               slices summed in ascending order             H *= sqrt(num / max(den, eps))
//   P4  fm_bin_reduce_kernel<scm>     one workgroup per (b, f), reduce over t      g *= sqrt(A / max(B, eps))
//   P5  fm_mix_kernel                  R (B,M,F,T) from W, H, g;  then the covariance pass + eps-floored IP sweep of
//                                      assx_fastmnmf_update_diagonalizer (fastmnmf_weighted_ip)
//   P6  fm_norm_bins_kernel            per (b, f): Q, g, W by the 'power' statistics
//       fm_norm_src_kernel             per (b, n, k): W normalised over f, H absorbs the sum
//   P1  fm_project_kernel              x~ (B,M,F,T) for the next iteration; the loss instantiation adds the data term
//       fm_logdet_kernel               (with the loss) ln|det Q_f|^2, one thread per (b, f)
//       fm_loss_finalize_kernel        (with the loss) per b: sum over bins in ascending order, - T sum_f ln|det Q_f|^2
//
// Lambda and R are recomputed in registers wherever they are needed (P1-P5); only x~ (written by P1, read by P2-P4)
// and the diagonaliser's weights R (P5) are materialised.  Every reduction has a fixed order (wave butterflies, then
// the waves of a workgroup in index order, then slices in index order; no float atomics), and no partition depends on
// B: two runs give the same bits, a batch gives the bits of its single-utterance calls.
#include "assx_common.hpp"
#include "assx_factor_common.hpp"
#include "assx_widem.hpp"

using namespace assx;
using namespace assx::mf;

namespace {

struct FmLayout {
  size_t xt, r2, lpart, dws, total;
};

// xt: x~ (B,M,F,T); r2: the diagonaliser's weights (B,M,F,T) or, earlier in the iteration, the activation half's slice
// partials (B,FS,2,N*K,T) -- never live at the same time; lpart: per-bin loss terms (2,B,F) float64; dws: the scratch of
// the covariance + IP pass (assx_workspace_bytes).
FmLayout fm_layout(int B, int M, int N, int F, int T, int K, int dtype) {
  const size_t es = dtype == ASSX_F64 ? 8 : 4;
  const size_t plane = (size_t)B * M * F * T * es;
  const size_t part = (size_t)B * act_slices(F) * 2 * N * K * T * es;
  Carve c(256);
  FmLayout L;
  L.xt = c.take(plane);
  L.r2 = c.take(plane > part ? plane : part);
  L.lpart = c.take((size_t)2 * B * F * sizeof(double));
  L.dws = c.take(assx_workspace_bytes(B, M, F, T, 1, dtype));
  L.total = c.total();
  return L;
}

template <typename R, int S>
__device__ __forceinline__ R pick(const R (&v)[S], int i) {  // v[i] for a run-time i without a scratch array
  R r = v[0];
#pragma unroll
  for (int q = 1; q < S; ++q) r = (i == q) ? v[q] : r;
  return r;
}

// Lambda_n at frame t and R_m = sum_n Lambda_n g[n,m] (mnmf.py:791-793).  Wf[n * wn + k], gf[n * gn + m]: the bin's
// basis and spatial covariance (LDS or global); Hb (N,K,T) the utterance's activation.
template <typename R, int M>
__device__ __forceinline__ void model_point(const R* Wf, size_t wn, const R* gf, size_t gn, const R* __restrict__ Hb,
                                            int N, int K, int T, int t, R (&lam)[NMAX], R (&Rm)[M]) {
#pragma unroll
  for (int n = 0; n < NMAX; ++n) {
    R acc = 0;
    if (n < N) {
      const R* h = Hb + (size_t)n * K * T + t;
      for (int k = 0; k < K; ++k) acc += Wf[n * wn + k] * h[(size_t)k * T];
    }
    lam[n] = acc;
  }
#pragma unroll
  for (int m = 0; m < M; ++m) {
    R acc = 0;
#pragma unroll
    for (int n = 0; n < NMAX; ++n)
      if (n < N) acc += lam[n] * gf[n * gn + m];
    Rm[m] = acc;
  }
}

// x~ / R^2 and 1 / R with R floored at eps (mnmf.py:794-795)
template <typename R, int M>
__device__ __forceinline__ void ratios(const R (&Rm)[M], const R (&x)[M], R eps, R (&a)[M], R (&c)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) {
    const R r = Rm[m] < eps ? eps : Rm[m];
    a[m] = x[m] / (r * r);
    c[m] = R(1) / r;
  }
}

// sum_m g[n,m] a_m and sum_m g[n,m] c_m for every source (mnmf.py:796-797)
template <typename R, int M>
__device__ __forceinline__ void source_sums(const R* gf, size_t gn, int N, const R (&a)[M], const R (&c)[M],
                                            R (&gx)[NMAX], R (&gr)[NMAX]) {
#pragma unroll
  for (int n = 0; n < NMAX; ++n) {
    R sx = 0, sr = 0;
    if (n < N) {
#pragma unroll
      for (int m = 0; m < M; ++m) {
        sx += gf[n * gn + m] * a[m];
        sr += gf[n * gn + m] * c[m];
      }
    }
    gx[n] = sx;
    gr[n] = sr;
  }
}

// ln |det A|^2 of a small complex matrix (LU with partial pivoting, in double); -inf for an exactly singular A
template <typename R, int M>
__device__ double log_abs_det2(const Cx<R>* A) {
  double re[M][M], im[M][M];
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < M; ++j) {
      re[i][j] = (double)A[i * M + j].x;
      im[i][j] = (double)A[i * M + j].y;
    }
  double acc = 0;
  for (int c = 0; c < M; ++c) {
    int p = c;
    double best = re[c][c] * re[c][c] + im[c][c] * im[c][c];
    for (int i = c + 1; i < M; ++i) {
      const double v = re[i][c] * re[i][c] + im[i][c] * im[i][c];
      if (v > best) best = v, p = i;
    }
    if (best == 0.0) return -INFINITY;
    if (p != c)
      for (int j = 0; j < M; ++j) {
        double tr = re[c][j], ti = im[c][j];
        re[c][j] = re[p][j], im[c][j] = im[p][j];
        re[p][j] = tr, im[p][j] = ti;
      }
    acc += log(best);
    const double ir = re[c][c] / best, ii = -im[c][c] / best;  // 1 / pivot
    for (int i = c + 1; i < M; ++i) {
      const double lr = re[i][c] * ir - im[i][c] * ii, li = re[i][c] * ii + im[i][c] * ir;
      for (int j = c + 1; j < M; ++j) {
        re[i][j] -= lr * re[c][j] - li * im[c][j];
        im[i][j] -= lr * im[c][j] + li * re[c][j];
      }
    }
  }
  return acc;
}

// row `ref` of A^{-1} (Gauss-Jordan with partial pivoting, in double); false for an exactly singular A
template <typename R, int M>
__device__ bool inverse_row(const Cx<R>* A, int ref, Cx<R>* out) {
  double re[M][2 * M], im[M][2 * M];
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < M; ++j) {
      re[i][j] = (double)A[i * M + j].x, im[i][j] = (double)A[i * M + j].y;
      re[i][M + j] = i == j ? 1.0 : 0.0, im[i][M + j] = 0.0;
    }
  for (int c = 0; c < M; ++c) {
    int p = c;
    double best = re[c][c] * re[c][c] + im[c][c] * im[c][c];
    for (int i = c + 1; i < M; ++i) {
      const double v = re[i][c] * re[i][c] + im[i][c] * im[i][c];
      if (v > best) best = v, p = i;
    }
    if (best == 0.0) return false;
    if (p != c)
      for (int j = 0; j < 2 * M; ++j) {
        double tr = re[c][j], ti = im[c][j];
        re[c][j] = re[p][j], im[c][j] = im[p][j];
        re[p][j] = tr, im[p][j] = ti;
      }
    const double ir = re[c][c] / best, ii = -im[c][c] / best;
    for (int j = 0; j < 2 * M; ++j) {
      const double a = re[c][j], b = im[c][j];
      re[c][j] = a * ir - b * ii, im[c][j] = a * ii + b * ir;
    }
    for (int i = 0; i < M; ++i) {
      if (i == c) continue;
      const double lr = re[i][c], li = im[i][c];
      for (int j = 0; j < 2 * M; ++j) {
        re[i][j] -= lr * re[c][j] - li * im[c][j];
        im[i][j] -= lr * im[c][j] + li * re[c][j];
      }
    }
  }
  for (int j = 0; j < M; ++j) out[j] = Cx<R>{(R)re[ref][M + j], (R)im[ref][M + j]};
  return true;
}

// the bin's model into LDS: Wf (N,K), gf (N,M), optionally Q_f
template <typename R, int M>
__device__ __forceinline__ void load_bin(const R* __restrict__ W, const R* __restrict__ g, const Cx<R>* __restrict__ Q,
                                         int b, int f, int N, int F, int K, R* Wf, R* gf, Cx<R>* Qs) {
  for (int i = threadIdx.x; i < N * K; i += blockDim.x)
    Wf[i] = W[(((size_t)b * N + i / K) * F + f) * K + i % K];
  for (int i = threadIdx.x; i < N * M; i += blockDim.x) gf[i] = g[(((size_t)b * N + i / M) * F + f) * M + i % M];
  if (Q)
    for (int i = threadIdx.x; i < M * M; i += blockDim.x) Qs[i] = Q[((size_t)b * F + f) * M * M + i];
}

// ---------------------------------------------------------------------------------------------------------------
// P1: x~ = |Q x|^2 (mnmf.py:785-786) and, in the LOSS instantiation, the per-bin data term of the loss
// (mnmf.py:890-917).  ln|det Q_f|^2 comes from fm_logdet_kernel: the pivoted LU stays out of this streaming kernel.
// ---------------------------------------------------------------------------------------------------------------
template <typename R, int M, bool LOSS>
__global__ void __launch_bounds__(BLK) fm_project_kernel(const Cx<R>* __restrict__ X, const Cx<R>* __restrict__ Q,
                                                         const R* __restrict__ W, const R* __restrict__ H,
                                                         const R* __restrict__ g, R* __restrict__ xt,
                                                         double* __restrict__ lpart, double eps, int N, int F, int T,
                                                         int K) {
  __shared__ Cx<R> Qs[M * M];
  __shared__ R Wf[NMAX * KMAX];
  __shared__ R gf[NMAX * M];
  __shared__ double red[BLK / WAVE];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if constexpr (LOSS)
    load_bin<R, M>(W, g, Q, b, f, N, F, K, Wf, gf, Qs);
  else
    for (int i = tid; i < M * M; i += BLK) Qs[i] = Q[((size_t)b * F + f) * M * M + i];
  __syncthreads();
  const size_t FT = (size_t)F * T;
  const Cx<R>* Xb = X + (size_t)b * M * FT + (size_t)f * T;
  R* xb = xt + (size_t)b * M * FT + (size_t)f * T;
  const R* Hb = H + (size_t)b * N * K * T;
  double acc = 0;
  for (int t = tid; t < T; t += BLK) {
    Cx<R> x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = Xb[m * FT + t];
    R xm[M];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      R yr = 0, yi = 0;
#pragma unroll
      for (int j = 0; j < M; ++j) {
        const Cx<R> q = Qs[m * M + j];
        yr += q.x * x[j].x - q.y * x[j].y;
        yi += q.x * x[j].y + q.y * x[j].x;
      }
      xm[m] = yr * yr + yi * yi;
      xb[m * FT + t] = xm[m];
    }
    if constexpr (LOSS) {
      R lam[NMAX], Rm[M];
      model_point<R, M>(Wf, K, gf, M, Hb, N, K, T, t, lam, Rm);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        const double xe = (double)xm[m] + eps, ye = (double)Rm[m] + eps;
        acc += xe / ye + log(ye);
      }
    }
  }
  if constexpr (!LOSS) return;
  acc = block_sum<double, BLK / WAVE>(acc, red);
  if (tid == 0) lpart[(size_t)b * F + f] = acc;
}

// ln|det(Q_f Q_f^T)| = ln|det Q_f|^2 per (b, f), one thread each, into the second half of lpart
template <typename R, int M>
__global__ void __launch_bounds__(WAVE) fm_logdet_kernel(const Cx<R>* __restrict__ Q, double* __restrict__ ldet,
                                                         int BF) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i >= BF) return;
  Cx<R> A[M * M];
#pragma unroll
  for (int j = 0; j < M * M; ++j) A[j] = Q[(size_t)i * M * M + j];
  ldet[i] = log_abs_det2<R, M>(A);
}

__global__ void __launch_bounds__(BLK) fm_loss_finalize_kernel(const double* __restrict__ lpart, double* __restrict__ loss,
                                                               int B, int F, int T) {
  __shared__ double red[2][BLK / WAVE];
  const int b = blockIdx.x, tid = threadIdx.x;
  double s = 0, d = 0;
  for (int f = tid; f < F; f += BLK) {
    s += lpart[(size_t)b * F + f];
    d += lpart[(size_t)B * F + (size_t)b * F + f];
  }
  s = block_sum<double, BLK / WAVE>(s, red[0]);
  d = block_sum<double, BLK / WAVE>(d, red[1]);
  if (tid == 0) loss[b] = s - (double)T * d;
}

// ---------------------------------------------------------------------------------------------------------------
// P2 / P4: reductions over t inside one bin.
//   basis (mnmf.py:788-801):  pair (n,k):  num = sum_t H[n,k,t] sum_m g[n,m] x~_m / R_m^2,  den = sum_t H[n,k,t] sum_m g[n,m] / R_m
//   SCM   (mnmf.py:829-844):  pair (n,m):  A   = sum_t Lambda_n x~_m / R_m^2,               B   = sum_t Lambda_n / R_m
// The pairs are taken CH at a time (registers); every chunk re-reads the bin's x~.  The model of the bin is updated
// only after the last chunk (every chunk reads the old one).
// ---------------------------------------------------------------------------------------------------------------
template <typename R, int M, bool SCM>
__global__ void __launch_bounds__(BLK) fm_bin_reduce_kernel(R* __restrict__ W, const R* __restrict__ H, R* __restrict__ g,
                                                            const R* __restrict__ xt, double eps_d, int N, int F, int T,
                                                            int K) {
  __shared__ R Wf[NMAX * KMAX];
  __shared__ R gf[NMAX * M];
  __shared__ R res[2 * NMAX * (SCM ? M : KMAX)];
  __shared__ R red[BLK / WAVE][2 * CH];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const R eps = (R)eps_d;
  load_bin<R, M>(W, g, nullptr, b, f, N, F, K, Wf, gf, nullptr);
  __syncthreads();
  const size_t FT = (size_t)F * T;
  const R* xb = xt + (size_t)b * M * FT + (size_t)f * T;
  const R* Hb = H + (size_t)b * N * K * T;
  const int Qd = SCM ? M : K;  // pair p = n * Qd + q
  const int NP = N * Qd;
  for (int p0 = 0; p0 < NP; p0 += CH) {
    int pn[CH], pq[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) pn[j] = (p0 + j) / Qd, pq[j] = (p0 + j) % Qd;
    R num[CH], den[CH];
#pragma unroll
    for (int j = 0; j < CH; ++j) num[j] = 0, den[j] = 0;
    for (int t = tid; t < T; t += BLK) {
      R x[M], lam[NMAX], Rm[M], a[M], c[M];
#pragma unroll
      for (int m = 0; m < M; ++m) x[m] = xb[m * FT + t];
      model_point<R, M>(Wf, K, gf, M, Hb, N, K, T, t, lam, Rm);
      ratios<R, M>(Rm, x, eps, a, c);
      if constexpr (!SCM) {
        R gx[NMAX], gr[NMAX];
        source_sums<R, M>(gf, M, N, a, c, gx, gr);
#pragma unroll
        for (int j = 0; j < CH; ++j)
          if (p0 + j < NP) {
            const R h = Hb[(size_t)(p0 + j) * T + t];
            num[j] += h * pick(gx, pn[j]);
            den[j] += h * pick(gr, pn[j]);
          }
      } else {
#pragma unroll
        for (int j = 0; j < CH; ++j)
          if (p0 + j < NP) {
            const R l = pick(lam, pn[j]);
            num[j] += l * pick(a, pq[j]);
            den[j] += l * pick(c, pq[j]);
          }
      }
    }
    R sn, sd;
    block_pair_sums<R, BLK / WAVE>(num, den, red, sn, sd);
    if (tid < CH && p0 + tid < NP) res[2 * (p0 + tid)] = sn, res[2 * (p0 + tid) + 1] = sd;
    __syncthreads();
  }
  for (int p = tid; p < NP; p += BLK) {
    const int n = p / Qd, q = p % Qd;
    R den = res[2 * p + 1];
    den = den < eps ? eps : den;
    const R s = sqrt(res[2 * p] / den);
    if constexpr (SCM)
      g[(((size_t)b * N + n) * F + f) * M + q] = gf[p] * s;
    else
      W[(((size_t)b * N + n) * F + f) * K + q] = Wf[p] * s;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// P3: activation half (mnmf.py:803-813), reduce over f.  Workgroup (frame block, f slice, utterance x pair chunk);
// the slice sums go to part (B,FS,2,N*K,T) and act_apply_kernel adds them in slice order.
// ---------------------------------------------------------------------------------------------------------------
template <typename R, int M>
__global__ void __launch_bounds__(ABLK) fm_act_partial_kernel(const R* __restrict__ W, const R* __restrict__ H,
                                                              const R* __restrict__ g, const R* __restrict__ xt,
                                                              R* __restrict__ part, double eps_d, int N, int F, int T,
                                                              int K, int FS, int nchunk) {
  const int t = blockIdx.x * ABLK + threadIdx.x, s = blockIdx.y;
  const int b = blockIdx.z / nchunk, p0 = (blockIdx.z % nchunk) * CH;
  if (t >= T) return;
  const R eps = (R)eps_d;
  const int NP = N * K;
  const int f0 = (int)((long long)s * F / FS), f1 = (int)((long long)(s + 1) * F / FS);
  const size_t FT = (size_t)F * T;
  const R* Hb = H + (size_t)b * N * K * T;
  int pn[CH], pk[CH];
#pragma unroll
  for (int j = 0; j < CH; ++j) pn[j] = (p0 + j) / K, pk[j] = (p0 + j) % K;
  R acc[2 * CH];
#pragma unroll
  for (int j = 0; j < 2 * CH; ++j) acc[j] = 0;
  for (int f = f0; f < f1; ++f) {
    const R* Wf = W + (size_t)b * N * F * K + (size_t)f * K;  // Wf[n * F * K + k]
    const R* gf = g + (size_t)b * N * F * M + (size_t)f * M;  // gf[n * F * M + m]
    const R* xb = xt + (size_t)b * M * FT + (size_t)f * T + t;
    R x[M], lam[NMAX], Rm[M], a[M], c[M], gx[NMAX], gr[NMAX];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = xb[m * FT];
    model_point<R, M>(Wf, (size_t)F * K, gf, (size_t)F * M, Hb, N, K, T, t, lam, Rm);
    ratios<R, M>(Rm, x, eps, a, c);
    source_sums<R, M>(gf, (size_t)F * M, N, a, c, gx, gr);
#pragma unroll
    for (int j = 0; j < CH; ++j)
      if (p0 + j < NP) {
        const R w = Wf[(size_t)pn[j] * F * K + pk[j]];
        acc[2 * j] += w * pick(gx, pn[j]);
        acc[2 * j + 1] += w * pick(gr, pn[j]);
      }
  }
#pragma unroll
  for (int j = 0; j < CH; ++j)
    if (p0 + j < NP) {
      R* o = part + (((size_t)b * FS + s) * 2 * NP + (p0 + j)) * T + t;
      o[0] = acc[2 * j];
      o[(size_t)NP * T] = acc[2 * j + 1];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// P5: the diagonaliser's weights R (mnmf.py:858-867) from the model
// ---------------------------------------------------------------------------------------------------------------
template <typename R, int M>
__global__ void __launch_bounds__(BLK) fm_mix_kernel(const R* __restrict__ W, const R* __restrict__ H,
                                                     const R* __restrict__ g, R* __restrict__ Rw, int N, int F, int T,
                                                     int K) {
  __shared__ R Wf[NMAX * KMAX];
  __shared__ R gf[NMAX * M];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  load_bin<R, M>(W, g, nullptr, b, f, N, F, K, Wf, gf, nullptr);
  __syncthreads();
  const size_t FT = (size_t)F * T;
  R* rb = Rw + (size_t)b * M * FT + (size_t)f * T;
  const R* Hb = H + (size_t)b * N * K * T;
  for (int t = tid; t < T; t += BLK) {
    R lam[NMAX], Rm[M];
    model_point<R, M>(Wf, K, gf, M, Hb, N, K, T, t, lam, Rm);
#pragma unroll
    for (int m = 0; m < M; ++m) rb[m * FT + t] = Rm[m];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// P6: normalize == 'power' (mnmf.py:748-769)
// ---------------------------------------------------------------------------------------------------------------
template <typename R, int M>
__global__ void __launch_bounds__(WAVE) fm_norm_bins_kernel(Cx<R>* __restrict__ Q, R* __restrict__ W,
                                                            R* __restrict__ g, double eps_d, int B, int N, int F,
                                                            int K) {
  const int i = blockIdx.x * WAVE + threadIdx.x;
  if (i >= B * F) return;
  const int b = i / F, f = i % F;
  const R eps = (R)eps_d;
  Cx<R>* Qf = Q + (size_t)i * M * M;
  R qq = 0;  // mean over rows of the row sums of |Q|^2
#pragma unroll
  for (int r = 0; r < M; ++r) {
    R row = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const Cx<R> q = Qf[r * M + j];
      row += q.x * q.x + q.y * q.y;
    }
    qq += row;
  }
  qq /= (R)M;
  qq = qq < eps ? eps : qq;
  const R sq = sqrt(qq);
#pragma unroll
  for (int j = 0; j < M * M; ++j) {
    Cx<R> q = Qf[j];
    Qf[j] = Cx<R>{q.x / sq, q.y / sq};
  }
  for (int n = 0; n < N; ++n) {
    R* gn = g + (((size_t)b * N + n) * F + f) * M;
    R gv[M], gs = 0;
#pragma unroll
    for (int m = 0; m < M; ++m) gv[m] = gn[m] / qq, gs += gv[m];
    gs = gs < eps ? eps : gs;
#pragma unroll
    for (int m = 0; m < M; ++m) gn[m] = gv[m] / gs;
    R* wn = W + (((size_t)b * N + n) * F + f) * K;
    for (int k = 0; k < K; ++k) wn[k] *= gs;
  }
}

template <typename R>
__global__ void __launch_bounds__(BLK) fm_norm_src_kernel(R* __restrict__ W, R* __restrict__ H, double eps_d, int N,
                                                          int F, int T, int K) {
  __shared__ R red[BLK / WAVE];
  __shared__ R tot;
  const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int n = p / K, k = p % K;
  R* Wc = W + ((size_t)b * N + n) * F * K + k;  // Wc[f * K]
  R s = 0;
  for (int f = tid; f < F; f += BLK) s += Wc[(size_t)f * K];
  s = block_sum<R, BLK / WAVE>(s, red);
  if (tid == 0) {
    const R eps = (R)eps_d;
    tot = s < eps ? eps : s;
  }
  __syncthreads();
  const R ws = tot;
  for (int f = tid; f < F; f += BLK) Wc[(size_t)f * K] = Wc[(size_t)f * K] / ws;
  R* Hr = H + ((size_t)b * N * K + p) * T;
  for (int t = tid; t < T; t += BLK) Hr[t] = Hr[t] * ws;
}

// ---------------------------------------------------------------------------------------------------------------
// separate (mnmf.py:919-946): Y[n] = sum_m (Q^{-1})[ref, m] (Q x)_m Lambda_n g[n,m] / max(R_m, eps)
// ---------------------------------------------------------------------------------------------------------------
template <typename R, int M>
__global__ void __launch_bounds__(BLK) fm_separate_kernel(const Cx<R>* __restrict__ X, const Cx<R>* __restrict__ Q,
                                                          const R* __restrict__ W, const R* __restrict__ H,
                                                          const R* __restrict__ g, int ref, double eps_d,
                                                          Cx<R>* __restrict__ Y, int32_t* __restrict__ status, int N,
                                                          int F, int T, int K) {
  __shared__ Cx<R> Qs[M * M];
  __shared__ Cx<R> qi[M];
  __shared__ R Wf[NMAX * KMAX];
  __shared__ R gf[NMAX * M];
  const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const R eps = (R)eps_d;
  load_bin<R, M>(W, g, Q, b, f, N, F, K, Wf, gf, Qs);
  __syncthreads();
  if (tid == 0) {
    if (!inverse_row<R, M>(Qs, ref, qi)) {
      for (int j = 0; j < M; ++j) qi[j] = Cx<R>{0, 0};
      if (status) atomicOr(status + b, (int32_t)ASSX_STATUS_SINGULAR);
    }
  }
  __syncthreads();
  const size_t FT = (size_t)F * T;
  const Cx<R>* Xb = X + (size_t)b * M * FT + (size_t)f * T;
  const R* Hb = H + (size_t)b * N * K * T;
  for (int t = tid; t < T; t += BLK) {
    Cx<R> x[M];
#pragma unroll
    for (int m = 0; m < M; ++m) x[m] = Xb[m * FT + t];
    R lam[NMAX], Rm[M];
    model_point<R, M>(Wf, K, gf, M, Hb, N, K, T, t, lam, Rm);
    Cx<R> u[M];  // (Q^{-1})[ref, m] (Q x)_m / max(R_m, eps)
#pragma unroll
    for (int m = 0; m < M; ++m) {
      R yr = 0, yi = 0;
#pragma unroll
      for (int j = 0; j < M; ++j) {
        const Cx<R> q = Qs[m * M + j];
        yr += q.x * x[j].x - q.y * x[j].y;
        yi += q.x * x[j].y + q.y * x[j].x;
      }
      const R r = Rm[m] < eps ? eps : Rm[m];
      const Cx<R> c = qi[m];
      u[m] = Cx<R>{(c.x * yr - c.y * yi) / r, (c.x * yi + c.y * yr) / r};
    }
#pragma unroll
    for (int n = 0; n < NMAX; ++n) {
      if (n < N) {
        R or_ = 0, oi = 0;
#pragma unroll
        for (int m = 0; m < M; ++m) {
          const R w = lam[n] * gf[n * M + m];
          or_ += w * u[m].x;
          oi += w * u[m].y;
        }
        Y[(((size_t)b * N + n) * F + f) * T + t] = Cx<R>{or_, oi};
      }
    }
  }
}

template <typename Fn>
int fm_dispatch(assx_ctx* ctx, int dtype, int M, Fn&& fn) {
  if (dtype != ASSX_F64 && dtype != ASSX_F32) return fail(ctx, ASSX_E_ARG, "bad dtype %d", dtype);
  auto go = [&](auto rt) -> int {
    return dispatch_channels(ctx, "FastMNMF", M, [&](auto mt) -> int { return fn(rt, mt); });
  };
  return dtype == ASSX_F64 ? go(double()) : go(float());
}

int fm_check(assx_ctx* ctx, int B, int M, int N, int F, int T, int K, int dtype) {
  return check_sizes(ctx, "FastMNMF", /*f64_only=*/false, B, M, N, F, T, K, dtype);
}

}  // namespace

extern "C" {

size_t assx_fastmnmf_workspace_bytes(int B, int M, int N, int F, int T, int K, int dtype) {
  if (B < 1 || M < 2 || M > 8 || N < 1 || N > NMAX || F < 1 || T < 1 || K < 1 || K > KMAX) return 0;
  return fm_layout(B, M, N, F, T, K, dtype).total;
}

int assx_fastmnmf_project(assx_ctx* ctx, const void* X, const void* Q, const void* W, const void* H, const void* g,
                          double eps, double* loss, void* ws, int B, int M, int N, int F, int T, int K, int dtype,
                          void* stream) {
  int rc = fm_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && Q && ws && (!loss || (W && H && g)), ASSX_E_NULL, "assx_fastmnmf_project: NULL array");
  const FmLayout L = fm_layout(B, M, N, F, T, K, dtype);
  hipStream_t st = (hipStream_t)stream;
  double* lpart = (double*)((char*)ws + L.lpart);
  return fm_dispatch(ctx, dtype, M, [&](auto rt, auto mt) -> int {
    using R = decltype(rt);
    constexpr int MM = decltype(mt)::value;
    R* xt = (R*)((char*)ws + L.xt);
    if (!loss) {
      hipLaunchKernelGGL((fm_project_kernel<R, MM, false>), dim3(F, B), dim3(BLK), 0, st, (const Cx<R>*)X,
                         (const Cx<R>*)Q, (const R*)W, (const R*)H, (const R*)g, xt, lpart, eps, N, F, T, K);
      ASSX_LAUNCH_CHECK(ctx, "fm_project_kernel");
      return 0;
    }
    hipLaunchKernelGGL((fm_project_kernel<R, MM, true>), dim3(F, B), dim3(BLK), 0, st, (const Cx<R>*)X,
                       (const Cx<R>*)Q, (const R*)W, (const R*)H, (const R*)g, xt, lpart, eps, N, F, T, K);
    ASSX_LAUNCH_CHECK(ctx, "fm_project_kernel<loss>");
    hipLaunchKernelGGL((fm_logdet_kernel<R, MM>), dim3(nblocks((size_t)B * F, WAVE)), dim3(WAVE), 0, st, (const Cx<R>*)Q,
                       lpart + (size_t)B * F, B * F);
    ASSX_LAUNCH_CHECK(ctx, "fm_logdet_kernel");
    hipLaunchKernelGGL(fm_loss_finalize_kernel, dim3(B), dim3(BLK), 0, st, (const double*)lpart, loss, B, F, T);
    ASSX_LAUNCH_CHECK(ctx, "fm_loss_finalize_kernel");
    return 0;
  });
}

int assx_fastmnmf_update_nmf(assx_ctx* ctx, void* W, void* H, const void* g, double eps, void* ws, int B, int M,
                             int N, int F, int T, int K, int dtype, void* stream) {
  int rc = fm_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, W && H && g && ws, ASSX_E_NULL, "assx_fastmnmf_update_nmf: NULL array");
  const FmLayout L = fm_layout(B, M, N, F, T, K, dtype);
  hipStream_t st = (hipStream_t)stream;
  const int FS = act_slices(F), NP = N * K, nchunk = (NP + CH - 1) / CH;
  return fm_dispatch(ctx, dtype, M, [&](auto rt, auto mt) -> int {
    using R = decltype(rt);
    constexpr int MM = decltype(mt)::value;
    const R* xt = (const R*)((const char*)ws + L.xt);
    R* part = (R*)((char*)ws + L.r2);
    hipLaunchKernelGGL((fm_bin_reduce_kernel<R, MM, false>), dim3(F, B), dim3(BLK), 0, st, (R*)W, (const R*)H, (R*)g,
                       xt, eps, N, F, T, K);
    ASSX_LAUNCH_CHECK(ctx, "fm_bin_reduce_kernel<basis>");
    hipLaunchKernelGGL((fm_act_partial_kernel<R, MM>), dim3(nblocks(T, ABLK), FS, B * nchunk), dim3(ABLK), 0, st,
                       (const R*)W, (const R*)H, (const R*)g, xt, part, eps, N, F, T, K, FS, nchunk);
    ASSX_LAUNCH_CHECK(ctx, "fm_act_partial_kernel");
    const size_t total = (size_t)B * NP * T;
    hipLaunchKernelGGL((act_apply_kernel<R>), dim3(nblocks(total, BLK)), dim3(BLK), 0, st, (R*)H, (const R*)part, eps,
                       NP, T, FS, total);
    ASSX_LAUNCH_CHECK(ctx, "act_apply_kernel");
    return 0;
  });
}

int assx_fastmnmf_update_scm(assx_ctx* ctx, const void* W, const void* H, void* g, double eps, void* ws, int B, int M,
                             int N, int F, int T, int K, int dtype, void* stream) {
  int rc = fm_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, W && H && g && ws, ASSX_E_NULL, "assx_fastmnmf_update_scm: NULL array");
  const FmLayout L = fm_layout(B, M, N, F, T, K, dtype);
  hipStream_t st = (hipStream_t)stream;
  return fm_dispatch(ctx, dtype, M, [&](auto rt, auto mt) -> int {
    using R = decltype(rt);
    constexpr int MM = decltype(mt)::value;
    hipLaunchKernelGGL((fm_bin_reduce_kernel<R, MM, true>), dim3(F, B), dim3(BLK), 0, st, (R*)W, (const R*)H, (R*)g,
                       (const R*)((const char*)ws + L.xt), eps, N, F, T, K);
    ASSX_LAUNCH_CHECK(ctx, "fm_bin_reduce_kernel<scm>");
    return 0;
  });
}

int assx_fastmnmf_update_diagonalizer_model(assx_ctx* ctx, const void* X, void* Q, const void* W, const void* H,
                                            const void* g, double eps, double threshold, int32_t* status, void* ws,
                                            int B, int M, int N, int F, int T, int K, int dtype, void* stream) {
  int rc = fm_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && Q && W && H && g && ws, ASSX_E_NULL, "assx_fastmnmf_update_diagonalizer_model: NULL array");
  const FmLayout L = fm_layout(B, M, N, F, T, K, dtype);
  hipStream_t st = (hipStream_t)stream;
  void* Rw = (char*)ws + L.r2;
  rc = fm_dispatch(ctx, dtype, M, [&](auto rt, auto mt) -> int {
    using R = decltype(rt);
    constexpr int MM = decltype(mt)::value;
    hipLaunchKernelGGL((fm_mix_kernel<R, MM>), dim3(F, B), dim3(BLK), 0, st, (const R*)W, (const R*)H, (const R*)g,
                       (R*)Rw, N, F, T, K);
    ASSX_LAUNCH_CHECK(ctx, "fm_mix_kernel");
    return 0;
  });
  if (rc) return rc;
  return fastmnmf_weighted_ip(ctx, X, Rw, Q, eps, threshold, status, (char*)ws + L.dws, B, M, F, T, dtype, st);
}

int assx_fastmnmf_normalize_power(assx_ctx* ctx, void* Q, void* W, void* H, void* g, double eps, int B, int M, int N,
                                  int F, int T, int K, int dtype, void* stream) {
  int rc = fm_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, Q && W && H && g, ASSX_E_NULL, "assx_fastmnmf_normalize_power: NULL array");
  hipStream_t st = (hipStream_t)stream;
  return fm_dispatch(ctx, dtype, M, [&](auto rt, auto mt) -> int {
    using R = decltype(rt);
    constexpr int MM = decltype(mt)::value;
    hipLaunchKernelGGL((fm_norm_bins_kernel<R, MM>), dim3(nblocks((size_t)B * F, WAVE)), dim3(WAVE), 0, st, (Cx<R>*)Q,
                       (R*)W, (R*)g, eps, B, N, F, K);
    ASSX_LAUNCH_CHECK(ctx, "fm_norm_bins_kernel");
    hipLaunchKernelGGL((fm_norm_src_kernel<R>), dim3(N * K, B), dim3(BLK), 0, st, (R*)W, (R*)H, eps, N, F, T, K);
    ASSX_LAUNCH_CHECK(ctx, "fm_norm_src_kernel");
    return 0;
  });
}

int assx_fastmnmf_separate(assx_ctx* ctx, const void* X, const void* Q, const void* W, const void* H, const void* g,
                           int ref, double eps, void* Y, int32_t* status, int B, int M, int N, int F, int T, int K,
                           int dtype, void* stream) {
  int rc = fm_check(ctx, B, M, N, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && Q && W && H && g && Y, ASSX_E_NULL, "assx_fastmnmf_separate: NULL array");
  ASSX_REQUIRE(ctx, ref >= 0 && ref < M, ASSX_E_ARG, "reference_id must be in [0, %d), got %d", M, ref);
  hipStream_t st = (hipStream_t)stream;
  return fm_dispatch(ctx, dtype, M, [&](auto rt, auto mt) -> int {
    using R = decltype(rt);
    constexpr int MM = decltype(mt)::value;
    hipLaunchKernelGGL((fm_separate_kernel<R, MM>), dim3(F, B), dim3(BLK), 0, st, (const Cx<R>*)X, (const Cx<R>*)Q,
                       (const R*)W, (const R*)H, (const R*)g, ref, eps, (Cx<R>*)Y, status, N, F, T, K);
    ASSX_LAUNCH_CHECK(ctx, "fm_separate_kernel");
    return 0;
  });
}

int assx_fastmnmf_iterate(assx_ctx* ctx, int n_iter, int normalize, const void* X, void* Q, void* W, void* H, void* g,
                          double eps, double threshold, double* loss, int32_t* status, void* ws, int B, int M, int N,
                          int F, int T, int K, int dtype, void* stream) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, n_iter >= 0, ASSX_E_ARG, "n_iter must be >= 0, got %d", n_iter);
  ASSX_REQUIRE(ctx, normalize == 0 || normalize == 1, ASSX_E_ARG, "normalize must be 0 or 1, got %d", normalize);
  // x~ of the entry model (and loss[0]); then per iteration the three updates, the normalisation and the x~ the next
  // iteration reads (loss[i + 1] in the same pass).  The same entry points, in the same order, as the host loop.
  int rc = assx_fastmnmf_project(ctx, X, Q, W, H, g, eps, loss, ws, B, M, N, F, T, K, dtype, stream);
  if (rc) return rc;
  for (int i = 0; i < n_iter; ++i) {
    if (i > 0 && !loss) {
      rc = assx_fastmnmf_project(ctx, X, Q, W, H, g, eps, nullptr, ws, B, M, N, F, T, K, dtype, stream);
      if (rc) return rc;
    }
    rc = assx_fastmnmf_update_nmf(ctx, W, H, g, eps, ws, B, M, N, F, T, K, dtype, stream);
    if (!rc) rc = assx_fastmnmf_update_scm(ctx, W, H, g, eps, ws, B, M, N, F, T, K, dtype, stream);
    if (!rc) rc = assx_fastmnmf_update_diagonalizer_model(ctx, X, Q, W, H, g, eps, threshold, status, ws, B, M, N, F, T, K,
                                                          dtype, stream);
    if (!rc && normalize) rc = assx_fastmnmf_normalize_power(ctx, Q, W, H, g, eps, B, M, N, F, T, K, dtype, stream);
    if (rc) return rc;
    if (loss) {
      rc = assx_fastmnmf_project(ctx, X, Q, W, H, g, eps, loss + (size_t)(i + 1) * B, ws, B, M, N, F, T, K, dtype, stream);
      if (rc) return rc;
    }
  }
  return 0;
}

}  // extern "C"
