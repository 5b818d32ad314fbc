// EUCNTF (non-negative tensor factorisation, src/algorithm/ntf.py:50-102) on MI355X: the whole update on the device.
//
// Model Xh[n,i,j] = sum_k Z[n,k] Tb[i,k] V[k,j].  State (leading batch axis B, float64, frames innermost): X (B,N,I,J)
// target, Z (B,N,K) partitioning, Tb (B,I,K) basis, V (B,K,J) activation.  With fl(a) = max(a, eps):
//
//   Tb' = Tb o fl(sum_{n,j} X Z V)    / fl(Tb G1)     G1 = (Z^T Z) o (V V^T)
//   V'  = V  o fl(sum_{n,i} X Z Tb')  / fl(G2 V)      G2 = (Z^T Z) o (Tb'^T Tb')
//   Z'  = Z  o fl(sum_{i,j} X Tb' V') / fl(Z G3)      G3 = (Tb'^T Tb') o (V' V'^T)
//
// The denominators are the reference's sums over Xh in Gram form: K x K matrices from the factors alone, so no pass
// forms Xh and X is read exactly three times per update, once per numerator.  Nothing with both a K and a J axis exists
// besides V, the slab partials of its numerator and its denominator.  One update is eight launches:
//
//   nt_gram_kernel        V V^T -> G1                  one workgroup per (b, k), lanes along j
//   nt_basis_kernel       one workgroup per (b, i), lanes along j, channels inside, n_basis in chunks of 16: with
//                         y_k(j) = sum_n Z[n,k] X[n,i,j] the numerator is sum_j y_k(j) V[k,j]; Tb' in place.  On request
//                         it first adds sum_{n,j} (X - Xh)^2 of its bin from the model at entry: the loss of the PREVIOUS
//                         update, by the code of nt_loss_kernel
//   nt_gram_kernel        Tb'^T Tb' -> G2; extra workgroups add the per-bin loss records in bin order
//   nt_act_kernel         64 frames x a slab of bins per workgroup, one wave per chunk of 16 bases, lanes on frames:
//                         the slab's partial of sum_i Tb'[i,k] y_k(i,j) into the workspace; slab 0 also G2 V
//   nt_act_apply_kernel   V' from the slab partials in slab order
//   nt_gram_kernel        V' V'^T -> G3
//   nt_part_kernel        one workgroup per (b, n, i), lanes along j: Tb'[i,k] sum_j X V'[k,j] into the workspace
//   nt_part_apply_kernel  one workgroup per (b, n): the bins in four strands of fixed order, Z' in place
//
// Every reduction has a fixed order (per-thread strides, a wave's butterfly, waves in index order, slabs or strands in
// index order; no float atomics) and no partition depends on B: two runs give the same bits, a batch gives the bits of
// its single calls, assx_ntf_iterate those of repeated assx_ntf_update.  Contraction is off for the whole file and every
// fused multiply-add is written out, so that the loss riding on the basis pass and assx_ntf_loss round alike.
#include "assx_common.hpp"
#include "assx_factor_common.hpp"

#pragma clang fp contract(off)

using namespace assx;
using mf::BLK;
using mf::CH;
using mf::KMAX;
using mf::block_sum;
using mf::nblocks;
using mf::strided_sum;

namespace {

constexpr int NW = BLK / WAVE;  // waves of a workgroup
constexpr int NCMAX = 32;       // channels
constexpr int NCH = 8;          // channels whose Xh a thread holds at once
constexpr int IS_MAX = 32;      // bin slabs of the activation pass, at least 8 bins each

struct NtLayout {
  size_t gv, gt, g, lossp, vnum, vden, zp, total;
};

// gv: V V^T (B,K,K); gt: Tb^T Tb (B,K,K); g: the Hadamard product the next denominator needs (B,K,K); lossp: sum_{n,j}
// (X - Xh)^2 (B,I); vnum: slab partials of V's numerator (B,IS,K,J); vden: G2 V (B,K,J); zp: Z's numerator per bin
// (B,N,I,K).  All float64, packed: the size grows with every one of B, N, I, J and K.
NtLayout nt_layout(int B, int N, int I, int J, int K) {
  const size_t d = sizeof(double), bkk = (size_t)B * K * K * d, bkj = (size_t)B * K * J * d;
  mf::Carve c(1);
  NtLayout L;
  L.gv = c.take(bkk);
  L.gt = c.take(bkk);
  L.g = c.take(bkk);
  L.lossp = c.take((size_t)B * I * d);
  L.vnum = c.take((size_t)mf::slabs8(I, IS_MAX) * bkj);
  L.vden = c.take(bkj);
  L.zp = c.take((size_t)B * N * I * K * d);
  L.total = c.total();
  return L;
}

// The workgroup's totals of CH per-thread values: a butterfly reduce-scatter in every wave, then the waves in index
// order.  Thread c < CH returns the total of value c, the others 0.  red is free again after the caller's next barrier.
__device__ __forceinline__ double nt_block_sums(double (&acc)[CH], double (*red)[CH]) {
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const double r = wave_reduce_scatter<double, CH>(acc);
  if (scatter_leader<CH>()) red[tid / WAVE][lane >> 2] = r;
  __syncthreads();
  double s = 0;
  if (tid < CH)
    for (int w = 0; w < NW; ++w) s += red[w][tid];
  return s;
}

// zt (N,K) = Z[n,k] Tb[i,k] of one bin, into LDS
__device__ __forceinline__ void nt_fill_zt(double* zt, const double* __restrict__ Zb, const double* __restrict__ Ti,
                                           int N, int K) {
  for (int e = threadIdx.x; e < N * K; e += BLK) zt[e] = Zb[e] * Ti[e % K];
  __syncthreads();
}

// Xh of frame j in channels n0 .. n0 + NCH - 1 (rows past N repeat the last channel and are ignored by the callers)
__device__ __forceinline__ void nt_xhat(const double* zt, const double* __restrict__ Vb, int N, size_t J, int K, int n0,
                                        int j, double (&xh)[NCH]) {
  int row[NCH];
#pragma unroll
  for (int u = 0; u < NCH; ++u) xh[u] = 0, row[u] = min(n0 + u, N - 1) * K;
  for (int k = 0; k < K; ++k) {
    const double v = Vb[(size_t)k * J + j];
#pragma unroll
    for (int u = 0; u < NCH; ++u) xh[u] = fma(zt[row[u] + k], v, xh[u]);
  }
}

// sum_{n,j} (X - Xh)^2 of one bin; Xi = X[b, 0, i, :]; thread 0 returns it
__device__ __forceinline__ double nt_row_loss(const double* __restrict__ Xi, const double* zt,
                                              const double* __restrict__ Vb, int N, int I, int J, int K, double* red) {
  double acc = 0;
  for (int j = threadIdx.x; j < J; j += BLK) {
    for (int n0 = 0; n0 < N; n0 += NCH) {
      double xh[NCH];
      nt_xhat(zt, Vb, N, (size_t)J, K, n0, j, xh);
#pragma unroll
      for (int u = 0; u < NCH; ++u) {
        if (n0 + u < N) {
          const double dlt = Xi[(size_t)(n0 + u) * I * J + j] - xh[u];
          acc = fma(dlt, dlt, acc);
        }
      }
    }
  }
  return block_sum<double, NW>(acc, red);
}

// Gram matrix of K vectors of length R: A[b*per + r*sr + k*sk].  raw (B,K,K) receives it, g (B,K,K) its Hadamard product
// with Z^T Z (Zm != NULL) or with `other`.  Blocks [0, B K): row k of utterance b; then B blocks for the loss (loss != NULL).
__global__ void __launch_bounds__(BLK) nt_gram_kernel(const double* __restrict__ A, size_t per, size_t sr, size_t sk, int R,
                                                      const double* __restrict__ Zm, const double* __restrict__ other,
                                                      double* __restrict__ raw, double* __restrict__ g,
                                                      const double* __restrict__ lossp, double* __restrict__ loss, int B,
                                                      int N, int I, int K) {
  __shared__ double red[NW][CH];
  __shared__ double redl[NW];
  if (blockIdx.x >= (unsigned)(B * K)) {
    const size_t b = blockIdx.x - (unsigned)(B * K);
    const double tot = strided_sum(lossp + b * I, I, 1, redl);
    if (threadIdx.x == 0) loss[b] = tot;
    return;
  }
  const size_t b = blockIdx.x / K;
  const int k = blockIdx.x % K;
  const double* Ab = A + b * per;
  for (int k0 = 0; k0 < K; k0 += CH) {
    double acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0;
    for (int r = threadIdx.x; r < R; r += BLK) {
      const double a = Ab[(size_t)r * sr + (size_t)k * sk];
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[c] = fma(a, Ab[(size_t)r * sr + (size_t)min(k0 + c, K - 1) * sk], acc[c]);
    }
    const double s = nt_block_sums(acc, red);
    const int kk = k0 + (int)threadIdx.x;
    if (threadIdx.x < CH && kk < K) {
      const size_t o = (b * K + k) * K + kk;
      double m;
      if (Zm) {
        m = 0;
        for (int n = 0; n < N; ++n) m = fma(Zm[(b * N + n) * K + k], Zm[(b * N + n) * K + kk], m);
      } else {
        m = other[o];
      }
      raw[o] = s;
      g[o] = s * m;
    }
    __syncthreads();
  }
}

template <bool LOSS>
__global__ void __launch_bounds__(BLK) nt_basis_kernel(const double* __restrict__ X, const double* __restrict__ Z,
                                                       double* Tb, const double* __restrict__ V,
                                                       const double* __restrict__ g, double* __restrict__ lossp,
                                                       double eps, int N, int I, int J, int K) {
  __shared__ double red[NW][CH];
  __shared__ double told[KMAX];
  __shared__ double zt[LOSS ? NCMAX * KMAX : 1];
  __shared__ double redl[NW];
  const size_t bi = blockIdx.x, b = bi / I, i = bi % I;
  const double* Xi = X + (b * N * I + i) * J;
  const double* Zb = Z + b * N * K;
  const double* Vb = V + b * K * J;
  if (threadIdx.x < K) told[threadIdx.x] = Tb[bi * K + threadIdx.x];
  if (LOSS) {
    nt_fill_zt(zt, Zb, Tb + bi * K, N, K);
    const double tot = nt_row_loss(Xi, zt, Vb, N, I, J, K, redl);
    if (threadIdx.x == 0) lossp[bi] = tot;
  }
  __syncthreads();
  for (int k0 = 0; k0 < K; k0 += CH) {
    double acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0;
    for (int j = threadIdx.x; j < J; j += BLK) {
      double y[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) y[c] = 0;
      for (int n = 0; n < N; ++n) {
        const double x = Xi[(size_t)n * I * J + j];
#pragma unroll
        for (int c = 0; c < CH; ++c) y[c] = fma(Zb[n * K + min(k0 + c, K - 1)], x, y[c]);
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[c] = fma(y[c], Vb[(size_t)min(k0 + c, K - 1) * J + j], acc[c]);
    }
    const double s = nt_block_sums(acc, red);
    const int k = k0 + (int)threadIdx.x;
    if (threadIdx.x < CH && k < K) {
      double den = 0;
      for (int kp = 0; kp < K; ++kp) den = fma(told[kp], g[(b * K + kp) * K + k], den);
      Tb[bi * K + k] = told[k] * (floor_eps(s, eps) / floor_eps(den, eps));
    }
    __syncthreads();
  }
}

// grid: x = b * jtiles + frame tile, y = slab; wave w of the workgroup owns bases 16 w .. 16 w + 15
__global__ void __launch_bounds__(BLK) nt_act_kernel(const double* __restrict__ X, const double* __restrict__ Z,
                                                     const double* __restrict__ Tb, const double* __restrict__ V,
                                                     const double* __restrict__ g, double* __restrict__ vnum,
                                                     double* __restrict__ vden, int N, int I, int J, int K, int IS,
                                                     int jtiles) {
  const int lane = threadIdx.x & (WAVE - 1), k0 = (threadIdx.x / WAVE) * CH;
  const size_t b = blockIdx.x / jtiles;
  const int tile = blockIdx.x % jtiles, slab = blockIdx.y;
  const int j = tile * WAVE + lane;
  if (j >= J || k0 >= K) return;
  const int i0 = (int)((size_t)slab * I / IS), i1 = (int)((size_t)(slab + 1) * I / IS);
  const double* Zb = Z + b * N * K;
  double acc[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) acc[c] = 0;
  for (int i = i0; i < i1; ++i) {
    const double* Xi = X + (b * N * I + i) * J + j;
    double y[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) y[c] = 0;
    for (int n = 0; n < N; ++n) {
      const double x = Xi[(size_t)n * I * J];
#pragma unroll
      for (int c = 0; c < CH; ++c) y[c] = fma(Zb[n * K + min(k0 + c, K - 1)], x, y[c]);
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = fma(y[c], Tb[(b * I + i) * K + min(k0 + c, K - 1)], acc[c]);
  }
  double* o = vnum + ((b * IS + slab) * K) * J + j;
#pragma unroll
  for (int c = 0; c < CH; ++c)
    if (k0 + c < K) o[(size_t)(k0 + c) * J] = acc[c];
  if (slab == 0) {
    double den[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) den[c] = 0;
    for (int kp = 0; kp < K; ++kp) {
      const double v = V[(b * K + kp) * J + j];
#pragma unroll
      for (int c = 0; c < CH; ++c) den[c] = fma(g[(b * K + min(k0 + c, K - 1)) * K + kp], v, den[c]);
    }
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (k0 + c < K) vden[(b * K + k0 + c) * J + j] = den[c];
  }
}

__global__ void __launch_bounds__(BLK) nt_act_apply_kernel(double* __restrict__ V, const double* __restrict__ vnum,
                                                           const double* __restrict__ vden, double eps, int J, int K,
                                                           int IS, size_t total) {
  const size_t e = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (e >= total) return;
  const size_t per = (size_t)K * J, b = e / per, r = e % per;
  double num = 0;
  for (int s = 0; s < IS; ++s) num += vnum[(b * IS + s) * per + r];
  V[e] = V[e] * (floor_eps(num, eps) / floor_eps(vden[e], eps));
}

// one workgroup per (b, n, i): zp[b,n,i,k] = Tb[i,k] sum_j X[n,i,j] V[k,j]
__global__ void __launch_bounds__(BLK) nt_part_kernel(const double* __restrict__ X, const double* __restrict__ Tb,
                                                      const double* __restrict__ V, double* __restrict__ zp, int N, int I,
                                                      int J, int K) {
  __shared__ double red[NW][CH];
  const size_t row = blockIdx.x, b = row / ((size_t)N * I), i = row % I;
  const double* Xr = X + row * J;
  const double* Vb = V + b * K * J;
  for (int k0 = 0; k0 < K; k0 += CH) {
    double acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0;
    for (int j = threadIdx.x; j < J; j += BLK) {
      const double x = Xr[j];
#pragma unroll
      for (int c = 0; c < CH; ++c) acc[c] = fma(x, Vb[(size_t)min(k0 + c, K - 1) * J + j], acc[c]);
    }
    const double s = nt_block_sums(acc, red);
    const int k = k0 + (int)threadIdx.x;
    if (threadIdx.x < CH && k < K) zp[row * K + k] = s * Tb[(b * I + i) * K + k];
    __syncthreads();
  }
}

// one workgroup per (b, n): thread (q, k) adds bins q, q + 4, ..; the four strands in index order
__global__ void __launch_bounds__(BLK) nt_part_apply_kernel(double* Z, const double* __restrict__ zp,
                                                            const double* __restrict__ g, double eps, int N, int I,
                                                            int K) {
  __shared__ double red[NW][KMAX];
  __shared__ double zold[KMAX];
  const size_t bn = blockIdx.x, b = bn / N;
  const int k = threadIdx.x & (KMAX - 1), q = threadIdx.x / KMAX;
  double s = 0;
  if (k < K)
    for (int i = q; i < I; i += NW) s += zp[(bn * I + i) * K + k];
  red[q][k] = s;
  if (threadIdx.x < K) zold[threadIdx.x] = Z[bn * K + threadIdx.x];
  __syncthreads();
  if (threadIdx.x < K) {
    const double num = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
    double den = 0;
    for (int kp = 0; kp < K; ++kp) den = fma(zold[kp], g[(b * K + kp) * K + k], den);
    Z[bn * K + k] = zold[k] * (floor_eps(num, eps) / floor_eps(den, eps));
  }
}

__global__ void __launch_bounds__(BLK) nt_loss_kernel(const double* __restrict__ X, const double* __restrict__ Z,
                                                      const double* __restrict__ Tb, const double* __restrict__ V,
                                                      double* __restrict__ lossp, int N, int I, int J, int K) {
  __shared__ double zt[NCMAX * KMAX];
  __shared__ double redl[NW];
  const size_t bi = blockIdx.x, b = bi / I, i = bi % I;
  nt_fill_zt(zt, Z + b * N * K, Tb + bi * K, N, K);
  const double tot = nt_row_loss(X + (b * N * I + i) * J, zt, V + b * K * J, N, I, J, K, redl);
  if (threadIdx.x == 0) lossp[bi] = tot;
}

__global__ void __launch_bounds__(BLK) nt_recon_kernel(const double* __restrict__ Z, const double* __restrict__ Tb,
                                                       const double* __restrict__ V, double* __restrict__ Xh, int N,
                                                       int I, int J, int K) {
  __shared__ double zt[NCMAX * KMAX];
  const size_t bi = blockIdx.x, b = bi / I, i = bi % I;
  nt_fill_zt(zt, Z + b * N * K, Tb + bi * K, N, K);
  double* Xi = Xh + (b * N * I + i) * J;
  for (int j = threadIdx.x; j < J; j += BLK) {
    for (int n0 = 0; n0 < N; n0 += NCH) {
      double xh[NCH];
      nt_xhat(zt, V + b * K * J, N, (size_t)J, K, n0, j, xh);
#pragma unroll
      for (int u = 0; u < NCH; ++u)
        if (n0 + u < N) Xi[(size_t)(n0 + u) * I * J + j] = xh[u];
    }
  }
}

int nt_check(assx_ctx* ctx, int B, int N, int I, int J, int K, int dtype) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, B >= 1 && I >= 1 && J >= 1, ASSX_E_ARG, "EUCNTF: invalid sizes B=%d I=%d J=%d", B, I, J);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64 || dtype == ASSX_F32, ASSX_E_ARG, "bad dtype %d", dtype);
  ASSX_REQUIRE(ctx, K >= 1 && K <= KMAX, ASSX_E_ARG, "EUCNTF: n_basis must be in [1, 64], got %d", K);
  ASSX_REQUIRE(ctx, N >= 1 && N <= NCMAX, ASSX_E_ARG, "EUCNTF: n_channels must be in [1, 32], got %d", N);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64, ASSX_E_UNSUPPORTED, "EUCNTF: float64 only");
  // one workgroup per (b, n, i), per (b, frame tile) and per 256 (b, k, j): the grids must fit 31 bits
  const long long lim = 1LL << 31;
  ASSX_REQUIRE(ctx, (long long)B * N * I < lim && (long long)B * nblocks((size_t)J, WAVE) < lim &&
                        ((long long)B * K * J + BLK - 1) / BLK < lim && (long long)B * (K + 1) < lim,
               ASSX_E_ARG, "EUCNTF: B=%d N=%d I=%d J=%d K=%d needs more workgroups than a launch can have", B, N, I, J, K);
  return 0;
}

struct NtDims {
  int B, N, I, J, K;
};

// which = 0: V V^T o Z^T Z;  1: Tb^T Tb o Z^T Z (and the loss records summed into loss_out);  2: V V^T o Tb^T Tb
int nt_gram(assx_ctx* ctx, int which, const double* Z, const double* Tb, const double* V, char* w, const NtLayout& L,
            double* loss_out, NtDims d, hipStream_t st) {
  const bool basis = which == 1;
  const double* A = basis ? Tb : V;
  const size_t per = basis ? (size_t)d.I * d.K : (size_t)d.K * d.J, sr = basis ? (size_t)d.K : 1,
               sk = basis ? 1 : (size_t)d.J;
  hipLaunchKernelGGL(nt_gram_kernel, dim3((unsigned)(d.B * d.K) + (loss_out ? (unsigned)d.B : 0u)), dim3(BLK), 0, st, A,
                     per, sr, sk, basis ? d.I : d.J, which == 2 ? (const double*)nullptr : Z,
                     which == 2 ? (const double*)(w + L.gt) : (const double*)nullptr,
                     (double*)(w + (basis ? L.gt : L.gv)), (double*)(w + L.g), (const double*)(w + L.lossp), loss_out,
                     d.B, d.N, d.I, d.K);
  ASSX_LAUNCH_CHECK(ctx, "nt_gram_kernel");
  return 0;
}

// one update_once; loss_prev (B,) or NULL receives the loss of the model at entry
int nt_update(assx_ctx* ctx, const double* X, double* Z, double* Tb, double* V, double eps, double* loss_prev, void* ws,
              NtDims d, hipStream_t st) {
  const int B = d.B, N = d.N, I = d.I, J = d.J, K = d.K;
  const NtLayout L = nt_layout(B, N, I, J, K);
  char* w = (char*)ws;
  const double* g = (const double*)(w + L.g);
  int rc = nt_gram(ctx, 0, Z, Tb, V, w, L, nullptr, d, st);
  if (rc) return rc;
  if (loss_prev)
    hipLaunchKernelGGL(nt_basis_kernel<true>, dim3((unsigned)(B * I)), dim3(BLK), 0, st, X, (const double*)Z, Tb,
                       (const double*)V, g, (double*)(w + L.lossp), eps, N, I, J, K);
  else
    hipLaunchKernelGGL(nt_basis_kernel<false>, dim3((unsigned)(B * I)), dim3(BLK), 0, st, X, (const double*)Z, Tb,
                       (const double*)V, g, (double*)nullptr, eps, N, I, J, K);
  ASSX_LAUNCH_CHECK(ctx, "nt_basis_kernel");
  rc = nt_gram(ctx, 1, Z, Tb, V, w, L, loss_prev, d, st);
  if (rc) return rc;
  const int IS = mf::slabs8(I, IS_MAX), nchunk = (K + CH - 1) / CH, jtiles = (int)nblocks((size_t)J, WAVE);
  hipLaunchKernelGGL(nt_act_kernel, dim3((unsigned)(B * jtiles), (unsigned)IS), dim3(WAVE * nchunk), 0, st, X,
                     (const double*)Z, (const double*)Tb, (const double*)V, g, (double*)(w + L.vnum),
                     (double*)(w + L.vden), N, I, J, K, IS, jtiles);
  ASSX_LAUNCH_CHECK(ctx, "nt_act_kernel");
  const size_t total = (size_t)B * K * J;
  hipLaunchKernelGGL(nt_act_apply_kernel, dim3(nblocks(total, BLK)), dim3(BLK), 0, st, V, (const double*)(w + L.vnum),
                     (const double*)(w + L.vden), eps, J, K, IS, total);
  ASSX_LAUNCH_CHECK(ctx, "nt_act_apply_kernel");
  rc = nt_gram(ctx, 2, Z, Tb, V, w, L, nullptr, d, st);
  if (rc) return rc;
  hipLaunchKernelGGL(nt_part_kernel, dim3((unsigned)(B * N * I)), dim3(BLK), 0, st, X, (const double*)Tb,
                     (const double*)V, (double*)(w + L.zp), N, I, J, K);
  ASSX_LAUNCH_CHECK(ctx, "nt_part_kernel");
  hipLaunchKernelGGL(nt_part_apply_kernel, dim3((unsigned)(B * N)), dim3(BLK), 0, st, Z, (const double*)(w + L.zp), g,
                     eps, N, I, K);
  ASSX_LAUNCH_CHECK(ctx, "nt_part_apply_kernel");
  return 0;
}

int nt_loss(assx_ctx* ctx, const double* X, const double* Z, const double* Tb, const double* V, double* loss, void* ws,
            NtDims d, hipStream_t st) {
  const NtLayout L = nt_layout(d.B, d.N, d.I, d.J, d.K);
  double* lossp = (double*)((char*)ws + L.lossp);
  hipLaunchKernelGGL(nt_loss_kernel, dim3((unsigned)(d.B * d.I)), dim3(BLK), 0, st, X, Z, Tb, V, lossp, d.N, d.I, d.J,
                     d.K);
  ASSX_LAUNCH_CHECK(ctx, "nt_loss_kernel");
  hipLaunchKernelGGL(mf::batch_sum_kernel<false>, dim3((unsigned)d.B), dim3(BLK), 0, st, (const double*)lossp, loss, d.I);
  ASSX_LAUNCH_CHECK(ctx, "batch_sum_kernel");
  return 0;
}

}  // namespace

extern "C" {

size_t assx_ntf_workspace_bytes(int B, int N, int I, int J, int K, int dtype) {
  if (dtype != ASSX_F64 || B < 1 || I < 1 || J < 1 || K < 1 || K > KMAX || N < 1 || N > NCMAX) return 0;
  return nt_layout(B, N, I, J, K).total;
}

int assx_ntf_update(assx_ctx* ctx, const void* X, void* Z, void* Tb, void* V, double eps, void* ws, int B, int N, int I,
                    int J, int K, int dtype, void* stream) {
  int rc = nt_check(ctx, B, N, I, J, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && Z && Tb && V && ws, ASSX_E_NULL, "assx_ntf_update: NULL array");
  return nt_update(ctx, (const double*)X, (double*)Z, (double*)Tb, (double*)V, eps, nullptr, ws, NtDims{B, N, I, J, K},
                   (hipStream_t)stream);
}

int assx_ntf_loss(assx_ctx* ctx, const void* X, const void* Z, const void* Tb, const void* V, double* loss, void* ws,
                  int B, int N, int I, int J, int K, int dtype, void* stream) {
  int rc = nt_check(ctx, B, N, I, J, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && Z && Tb && V && loss && ws, ASSX_E_NULL, "assx_ntf_loss: NULL array");
  return nt_loss(ctx, (const double*)X, (const double*)Z, (const double*)Tb, (const double*)V, loss, ws,
                 NtDims{B, N, I, J, K}, (hipStream_t)stream);
}

int assx_ntf_reconstruct(assx_ctx* ctx, const void* Z, const void* Tb, const void* V, void* Xh, int B, int N, int I, int J,
                         int K, int dtype, void* stream) {
  int rc = nt_check(ctx, B, N, I, J, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, Z && Tb && V && Xh, ASSX_E_NULL, "assx_ntf_reconstruct: NULL array");
  hipLaunchKernelGGL(nt_recon_kernel, dim3((unsigned)(B * I)), dim3(BLK), 0, (hipStream_t)stream, (const double*)Z,
                     (const double*)Tb, (const double*)V, (double*)Xh, N, I, J, K);
  ASSX_LAUNCH_CHECK(ctx, "nt_recon_kernel");
  return 0;
}

int assx_ntf_iterate(assx_ctx* ctx, int n_iter, const void* X, void* Z, void* Tb, void* V, double eps, double* loss,
                     void* ws, int B, int N, int I, int J, int K, int dtype, void* stream) {
  int rc = nt_check(ctx, B, N, I, J, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, n_iter >= 0, ASSX_E_ARG, "assx_ntf_iterate: n_iter = %d", n_iter);
  ASSX_REQUIRE(ctx, X && Z && Tb && V && ws, ASSX_E_NULL, "assx_ntf_iterate: NULL array");
  hipStream_t st = (hipStream_t)stream;
  const NtDims d{B, N, I, J, K};
  for (int it = 0; it < n_iter; ++it) {
    // the basis pass of update it + 1 reads X against the model update it left: its sum is loss[it - 1]
    double* prev = (loss && it > 0) ? loss + (size_t)(it - 1) * B : nullptr;
    rc = nt_update(ctx, (const double*)X, (double*)Z, (double*)Tb, (double*)V, eps, prev, ws, d, st);
    if (rc) return rc;
  }
  if (loss && n_iter > 0)
    return nt_loss(ctx, (const double*)X, (const double*)Z, (const double*)Tb, (const double*)V,
                   loss + (size_t)(n_iter - 1) * B, ws, d, st);
  return 0;
}

}  // extern "C"
