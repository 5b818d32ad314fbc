// ComplexEUCNMF (Kameoka's complex NMF, src/algorithm/nmf.py:58-114, 597-676) on MI355X: the whole update on the device.
//
// State (leading utterance axis B, float64):  X (B,F,T) complex, Tb (B,F,K) basis, V (B,K,T) activation, Phi (B,F,K,T)
// phase angles, frames innermost.  Beta is never stored: it is a function of Tb and V (nmf.py:669-676) and is re-formed
// where it is needed.  With E = exp(i Phi), a = Tb V (per f, k, t; V as it stands, unfloored), tv = max(sum_k a, eps):
//
//   ZX   = X - sum_k a E                       Beta = max(a / tv, eps)          Zbar = a E + Beta ZX
//   Re   = real(conj(Zbar) E)                  Vf   = max(V, eps)
//   Tb'  = sum_t (Vf / Beta) Re / max(sum_t Vf^2 / Beta, eps)
//   V'   = sum_f (Tb' / Beta) Re / max(sum_f Tb'^2 / Beta + regularizer p Vf^(p-2), eps)
//   Phi' = atan2(imag Zbar, real Zbar)         Tb'' = Tb' / sum_f Tb'
//
// One update is four launches; ZX and tv travel through the workspace (3 reals per (f, t) against K angles):
//
//   cn_resid_kernel     one workgroup per (b, f), lanes along t: ZX, tv into ws; sum_t |ZX|^2 per (b, f) -- the loss of
//                       the model as it stands, which is the loss of the PREVIOUS update
//   cn_basis_kernel     one workgroup per (b, f), lanes along t, n_basis in chunks of 16: the two t-sums, Tb' into ws
//                       (Tb itself stays: the activation pass still needs it)
//   cn_act_kernel       64 frames x a slab of bins x a chunk of 16 bases per workgroup; its four waves take the bins of
//                       the slab in turn.  Re-forms Zbar and Re from the old model, adds the two f-sums per (k, t) (waves
//                       in index order through LDS) into the slab's partial, writes Phi' over Phi: a lane owns its
//                       (f, k, t) entry
//   cn_finalize_kernel  V' from the slab partials in slab order; Tb'' = Tb' / column sum; the loss from the (b, f)
//                       partials of cn_resid_kernel
//
// Every reduction has a fixed order (a wave's butterfly, the waves of a workgroup in index order, then slabs or bins in
// index order; no float atomics) and no partition depends on B: two runs give the same bits, a batch gives the bits of
// its single-utterance calls, assx_cnmf_iterate those of repeated assx_cnmf_update.  Contraction into fused multiply-adds
// is off for the whole file: with one basis and a silent entry Zbar = a E + 1 (0 - a E) must come out exactly 0 (the
// reference's angle there is 0), which fma(a, E, -round(a E)) is not.
#include "assx_common.hpp"
#include "assx_factor_common.hpp"

#pragma clang fp contract(off)

using namespace assx;
using mf::BLK;
using mf::CH;
using mf::KMAX;
using mf::block_pair_sums;
using mf::block_sum;
using mf::nblocks;
using mf::strided_sum;

namespace {

constexpr int NW = BLK / WAVE;  // waves of a workgroup
constexpr int FS_MAX = 32;      // bin slabs of the activation pass, at least 8 bins each
enum { REG_RCP = 0, REG_ONE = 1, REG_POW = 2 };  // Vf^(p-2) for p = 1, p = 2, any other p

struct CnLayout {
  size_t zx, tvs, tnew, lossp, part, total;
};

// zx: ZX (B,F,T) complex; tvs: max(sum_k Tb V, eps) (B,F,T); tnew: Tb' (B,F,K); lossp: sum_t |ZX|^2 (B,F);
// part: slab partials of the activation sums (B,FS,2,K,T).  All float64.
CnLayout cn_layout(int B, int F, int T, int K) {
  const size_t d = sizeof(double), bft = (size_t)B * F * T;
  mf::Carve c(256);
  CnLayout L;
  L.zx = c.take(2 * bft * d);
  L.tvs = c.take(bft * d);
  L.tnew = c.take((size_t)B * F * K * d);
  L.lossp = c.take((size_t)B * F * d);
  L.part = c.take((size_t)B * mf::slabs8(F, FS_MAX) * 2 * K * T * d);
  L.total = c.total();
  return L;
}

// sum_k Tb V exp(i Phi) and sum_k Tb V at one (f, t): Tf = the bin's basis row, Vt / Pt = the frame's first entries of V
// and Phi (stride T between bases)
__device__ __forceinline__ void cn_point(const double* __restrict__ Tf, const double* __restrict__ Vt,
                                         const double* __restrict__ Pt, int K, size_t T, double& sr, double& si,
                                         double& tv) {
  sr = 0, si = 0, tv = 0;
  for (int k = 0; k < K; ++k) {
    double sn, cs;
    sincos(Pt[(size_t)k * T], &sn, &cs);
    const double a = Tf[k] * Vt[(size_t)k * T];
    sr += a * cs;
    si += a * sn;
    tv += a;
  }
}

// Zbar and Re of one (f, k, t) entry from the old model; returns Beta
__device__ __forceinline__ double cn_entry(double tk, double vu, double ph, Cx<double> z, double tv, double eps,
                                           double& zr, double& zi, double& re) {
  double sn, cs;
  sincos(ph, &sn, &cs);
  const double a = tk * vu;
  const double beta = floor_eps(a / tv, eps);
  zr = a * cs + beta * z.x;
  zi = a * sn + beta * z.y;
  re = zr * cs + zi * sn;
  return beta;
}

__global__ void __launch_bounds__(BLK) cn_resid_kernel(const Cx<double>* __restrict__ X, const double* __restrict__ Tb,
                                                       const double* __restrict__ V, const double* __restrict__ Phi,
                                                       Cx<double>* __restrict__ zx, double* __restrict__ tvs,
                                                       double* __restrict__ lossp, double eps, int F, int T, int K) {
  __shared__ double red[NW];
  const size_t bf = blockIdx.x, b = bf / F;
  const double* Tf = Tb + bf * K;
  double acc = 0;
  for (int t = threadIdx.x; t < T; t += BLK) {
    double sr, si, tv;
    cn_point(Tf, V + b * K * T + t, Phi + bf * K * T + t, K, (size_t)T, sr, si, tv);
    const Cx<double> x = X[bf * T + t];
    const double zr = x.x - sr, zi = x.y - si;
    zx[bf * T + t] = cmake<double>(zr, zi);
    tvs[bf * T + t] = floor_eps(tv, eps);
    acc += zr * zr + zi * zi;
  }
  const double tot = block_sum<double, NW>(acc, red);
  if (threadIdx.x == 0) lossp[bf] = tot;
}

// MODE 0: Y (B,F,T) complex = sum_k Tb V exp(i Phi);  MODE 1: Beta (B,F,K,T) = Tb V / max(sum_k Tb V, eps)
template <int MODE>
__global__ void __launch_bounds__(BLK) cn_model_kernel(const double* __restrict__ Tb, const double* __restrict__ V,
                                                       const double* __restrict__ Phi, void* __restrict__ out,
                                                       double eps, int F, int T, int K) {
  const size_t bf = blockIdx.x, b = bf / F;
  const double* Tf = Tb + bf * K;
  for (int t = threadIdx.x; t < T; t += BLK) {
    const double* Vt = V + b * K * T + t;
    if (MODE == 0) {
      double sr, si, tv;
      cn_point(Tf, Vt, Phi + bf * K * T + t, K, (size_t)T, sr, si, tv);
      ((Cx<double>*)out)[bf * T + t] = cmake<double>(sr, si);
    } else {
      double tv = 0;
      for (int k = 0; k < K; ++k) tv += Tf[k] * Vt[(size_t)k * T];
      tv = floor_eps(tv, eps);
      for (int k = 0; k < K; ++k) ((double*)out)[(bf * K + k) * T + t] = (Tf[k] * Vt[(size_t)k * T]) / tv;
    }
  }
}

__global__ void __launch_bounds__(BLK) cn_basis_kernel(const double* __restrict__ Tb, const double* __restrict__ V,
                                                       const double* __restrict__ Phi, const Cx<double>* __restrict__ zx,
                                                       const double* __restrict__ tvs, double* __restrict__ tnew,
                                                       double eps, int F, int T, int K) {
  __shared__ double red[NW][2 * CH];
  const size_t bf = blockIdx.x, b = bf / F;
  const double* Tf = Tb + bf * K;
  for (int k0 = 0; k0 < K; k0 += CH) {
    double num[CH], den[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) num[c] = 0, den[c] = 0;
    for (int t = threadIdx.x; t < T; t += BLK) {
      const Cx<double> z = zx[bf * T + t];
      const double tv = tvs[bf * T + t];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int k = k0 + c;
        if (k < K) {
          const double vu = V[(b * K + k) * T + t];
          double zr, zi, re;
          const double beta = cn_entry(Tf[k], vu, Phi[(bf * K + k) * T + t], z, tv, eps, zr, zi, re);
          const double vf = floor_eps(vu, eps);
          num[c] += (vf / beta) * re;
          den[c] += (vf * vf) / beta;
        }
      }
    }
    double sn, sd;
    block_pair_sums<double, NW>(num, den, red, sn, sd);
    if (threadIdx.x < CH && k0 + (int)threadIdx.x < K) tnew[bf * K + k0 + threadIdx.x] = sn / floor_eps(sd, eps);
    __syncthreads();
  }
}

// grid: x = b * ttiles + t tile, y = slab * nchunk + basis chunk
__global__ void __launch_bounds__(BLK) cn_act_kernel(const double* __restrict__ Tb, const double* __restrict__ tnew,
                                                     const double* __restrict__ V, double* Phi,
                                                     const Cx<double>* __restrict__ zx, const double* __restrict__ tvs,
                                                     double* __restrict__ part, double eps, int F, int T, int K, int FS,
                                                     int nchunk, int ttiles) {
  __shared__ double red[NW - 1][2 * CH][WAVE];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  const size_t b = blockIdx.x / ttiles;
  const int tile = blockIdx.x % ttiles, slab = blockIdx.y / nchunk, k0 = (blockIdx.y % nchunk) * CH;
  const int t = tile * WAVE + lane;
  const bool on = t < T;
  const int f0 = (int)((size_t)slab * F / FS), f1 = (int)((size_t)(slab + 1) * F / FS);
  double num[CH], den[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) num[c] = 0, den[c] = 0;
  if (on) {
    for (int f = f0 + w; f < f1; f += NW) {
      const size_t bf = b * F + f;
      const Cx<double> z = zx[bf * T + t];
      const double tv = tvs[bf * T + t];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int k = k0 + c;
        if (k < K) {
          double* ph = Phi + (bf * K + k) * T + t;
          double zr, zi, re;
          const double beta = cn_entry(Tb[bf * K + k], V[(b * K + k) * T + t], *ph, z, tv, eps, zr, zi, re);
          const double tn = tnew[bf * K + k];
          num[c] += (tn / beta) * re;
          den[c] += (tn * tn) / beta;
          *ph = atan2(zi, zr);
        }
      }
    }
  }
  if (w > 0) {
#pragma unroll
    for (int c = 0; c < CH; ++c) red[w - 1][2 * c][lane] = num[c], red[w - 1][2 * c + 1][lane] = den[c];
  }
  __syncthreads();
  if (w == 0 && on) {
    double* o = part + ((b * FS + slab) * 2) * K * T + t;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const int k = k0 + c;
      if (k < K) {
        double n = num[c], d = den[c];
        for (int v = 0; v < NW - 1; ++v) n += red[v][2 * c][lane], d += red[v][2 * c + 1][lane];
        o[(size_t)k * T] = n;
        o[((size_t)K + k) * T] = d;
      }
    }
  }
}

// blocks [0, nvb): V' of 256 (b, k, t) entries each; [nvb, nvb + B K): one basis column each; then B blocks for the
// loss when loss != NULL
__global__ void __launch_bounds__(BLK) cn_finalize_kernel(double* __restrict__ Tb, const double* __restrict__ tnew,
                                                          double* __restrict__ V, const double* __restrict__ part,
                                                          const double* __restrict__ lossp, double* __restrict__ loss,
                                                          double reg_p, double e, int mode, double eps, int B, int F,
                                                          int T, int K, int FS, unsigned nvb) {
  __shared__ double red[NW];
  __shared__ double total;
  if (blockIdx.x < nvb) {
    const size_t per = (size_t)K * T, i = (size_t)blockIdx.x * BLK + threadIdx.x;
    if (i >= (size_t)B * per) return;
    const size_t b = i / per, r = i % per;
    double num = 0, den = 0;
    for (int s = 0; s < FS; ++s) {
      const double* o = part + (b * FS + s) * 2 * per + r;
      num += o[0];
      den += o[per];
    }
    const double vf = floor_eps(V[i], eps);
    const double pw = mode == REG_RCP ? 1.0 / vf : mode == REG_ONE ? 1.0 : pow(vf, e);
    den = floor_eps(den + reg_p * pw, eps);
    V[i] = num / den;
  } else if (blockIdx.x < nvb + (unsigned)(B * K)) {
    const size_t idx = blockIdx.x - nvb, b = idx / K, k = idx % K;
    const double* src = tnew + b * F * K + k;
    const double tot = strided_sum(src, F, (size_t)K, red);
    if (threadIdx.x == 0) total = tot;
    __syncthreads();
    const double s = total;
    double* dst = Tb + b * F * K + k;
    for (int f = threadIdx.x; f < F; f += BLK) dst[(size_t)f * K] = src[(size_t)f * K] / s;
  } else {
    const size_t b = blockIdx.x - nvb - (unsigned)(B * K);
    const double tot = strided_sum(lossp + b * F, F, 1, red);
    if (threadIdx.x == 0) loss[b] = tot;
  }
}

int cn_check(assx_ctx* ctx, int B, int F, int T, int K, int dtype) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, B >= 1 && F >= 1 && T >= 1, ASSX_E_ARG, "ComplexEUCNMF: invalid sizes B=%d F=%d T=%d", B, F, T);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64 || dtype == ASSX_F32, ASSX_E_ARG, "bad dtype %d", dtype);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64, ASSX_E_UNSUPPORTED, "ComplexEUCNMF: float64 only");
  ASSX_REQUIRE(ctx, K >= 1 && K <= KMAX, ASSX_E_ARG, "ComplexEUCNMF: n_basis must be in [1, 64], got %d", K);
  // one workgroup per (b, f), per (b, t tile) and per 256 (b, k, t): the grids must fit 31 bits
  const long long lim = 1LL << 31;
  ASSX_REQUIRE(ctx, (long long)B * F < lim && (long long)B * nblocks((size_t)T, WAVE) < lim &&
                        ((long long)B * K * T + BLK - 1) / BLK + (long long)B * (K + 1) < lim,
               ASSX_E_ARG, "ComplexEUCNMF: B=%d F=%d T=%d K=%d needs more workgroups than a launch can have", B, F, T, K);
  return 0;
}

int cn_resid(assx_ctx* ctx, const void* X, const void* Tb, const void* V, const void* Phi, double eps, void* ws, int B,
             int F, int T, int K, hipStream_t st) {
  const CnLayout L = cn_layout(B, F, T, K);
  char* w = (char*)ws;
  hipLaunchKernelGGL(cn_resid_kernel, dim3((unsigned)(B * F)), dim3(BLK), 0, st, (const Cx<double>*)X, (const double*)Tb,
                     (const double*)V, (const double*)Phi, (Cx<double>*)(w + L.zx), (double*)(w + L.tvs),
                     (double*)(w + L.lossp), eps, F, T, K);
  ASSX_LAUNCH_CHECK(ctx, "cn_resid_kernel");
  return 0;
}

// one update_once; loss_prev (B,) or NULL receives the loss of the model at entry
int cn_update(assx_ctx* ctx, const void* X, void* Tb, void* V, void* Phi, double regularizer, double p, double eps,
              double* loss_prev, void* ws, int B, int F, int T, int K, hipStream_t st) {
  int rc = cn_resid(ctx, X, Tb, V, Phi, eps, ws, B, F, T, K, st);
  if (rc) return rc;
  const CnLayout L = cn_layout(B, F, T, K);
  char* w = (char*)ws;
  const Cx<double>* zx = (const Cx<double>*)(w + L.zx);
  const double* tvs = (const double*)(w + L.tvs);
  double* tnew = (double*)(w + L.tnew);
  double* part = (double*)(w + L.part);
  hipLaunchKernelGGL(cn_basis_kernel, dim3((unsigned)(B * F)), dim3(BLK), 0, st, (const double*)Tb, (const double*)V,
                     (const double*)Phi, zx, tvs, tnew, eps, F, T, K);
  ASSX_LAUNCH_CHECK(ctx, "cn_basis_kernel");
  const int FS = mf::slabs8(F, FS_MAX), nchunk = (K + CH - 1) / CH, ttiles = (int)nblocks((size_t)T, WAVE);
  hipLaunchKernelGGL(cn_act_kernel, dim3((unsigned)(B * ttiles), (unsigned)(FS * nchunk)), dim3(BLK), 0, st,
                     (const double*)Tb, (const double*)tnew, (const double*)V, (double*)Phi, zx, tvs, part, eps, F, T, K,
                     FS, nchunk, ttiles);
  ASSX_LAUNCH_CHECK(ctx, "cn_act_kernel");
  const unsigned nvb = nblocks((size_t)B * K * T, BLK);
  const int mode = p == 1.0 ? REG_RCP : p == 2.0 ? REG_ONE : REG_POW;
  hipLaunchKernelGGL(cn_finalize_kernel, dim3(nvb + (unsigned)(B * K) + (loss_prev ? (unsigned)B : 0u)), dim3(BLK), 0, st,
                     (double*)Tb, (const double*)tnew, (double*)V, (const double*)part, (const double*)(w + L.lossp),
                     loss_prev, regularizer * p, p - 2.0, mode, eps, B, F, T, K, FS, nvb);
  ASSX_LAUNCH_CHECK(ctx, "cn_finalize_kernel");
  return 0;
}

int cn_loss(assx_ctx* ctx, const void* X, const void* Tb, const void* V, const void* Phi, double eps, double* loss,
            void* ws, int B, int F, int T, int K, hipStream_t st) {
  int rc = cn_resid(ctx, X, Tb, V, Phi, eps, ws, B, F, T, K, st);
  if (rc) return rc;
  const CnLayout L = cn_layout(B, F, T, K);
  hipLaunchKernelGGL(mf::batch_sum_kernel<false>, dim3((unsigned)B), dim3(BLK), 0, st,
                     (const double*)((char*)ws + L.lossp), loss, F);
  ASSX_LAUNCH_CHECK(ctx, "batch_sum_kernel");
  return 0;
}

}  // namespace

extern "C" {

size_t assx_cnmf_workspace_bytes(int B, int F, int T, int K, int dtype) {
  if (dtype != ASSX_F64 || B < 1 || F < 1 || T < 1 || K < 1 || K > KMAX) return 0;
  return cn_layout(B, F, T, K).total;
}

int assx_cnmf_update(assx_ctx* ctx, const void* X, void* Tb, void* V, void* Phi, double regularizer, double p,
                     double eps, void* ws, int B, int F, int T, int K, int dtype, void* stream) {
  int rc = cn_check(ctx, B, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && Tb && V && Phi && ws, ASSX_E_NULL, "assx_cnmf_update: NULL array");
  return cn_update(ctx, X, Tb, V, Phi, regularizer, p, eps, nullptr, ws, B, F, T, K, (hipStream_t)stream);
}

int assx_cnmf_loss(assx_ctx* ctx, const void* X, const void* Tb, const void* V, const void* Phi, double eps,
                   double* loss, void* ws, int B, int F, int T, int K, int dtype, void* stream) {
  int rc = cn_check(ctx, B, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && Tb && V && Phi && loss && ws, ASSX_E_NULL, "assx_cnmf_loss: NULL array");
  return cn_loss(ctx, X, Tb, V, Phi, eps, loss, ws, B, F, T, K, (hipStream_t)stream);
}

int assx_cnmf_beta(assx_ctx* ctx, const void* Tb, const void* V, double eps, void* Beta, int B, int F, int T, int K,
                   int dtype, void* stream) {
  int rc = cn_check(ctx, B, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, Tb && V && Beta, ASSX_E_NULL, "assx_cnmf_beta: NULL array");
  hipLaunchKernelGGL(cn_model_kernel<1>, dim3((unsigned)(B * F)), dim3(BLK), 0, (hipStream_t)stream, (const double*)Tb,
                     (const double*)V, (const double*)nullptr, Beta, eps, F, T, K);
  ASSX_LAUNCH_CHECK(ctx, "cn_model_kernel<beta>");
  return 0;
}

int assx_cnmf_reconstruct(assx_ctx* ctx, const void* Tb, const void* V, const void* Phi, void* Y, int B, int F, int T,
                          int K, int dtype, void* stream) {
  int rc = cn_check(ctx, B, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, Tb && V && Phi && Y, ASSX_E_NULL, "assx_cnmf_reconstruct: NULL array");
  hipLaunchKernelGGL(cn_model_kernel<0>, dim3((unsigned)(B * F)), dim3(BLK), 0, (hipStream_t)stream, (const double*)Tb,
                     (const double*)V, (const double*)Phi, Y, 0.0, F, T, K);
  ASSX_LAUNCH_CHECK(ctx, "cn_model_kernel<reconstruct>");
  return 0;
}

int assx_cnmf_iterate(assx_ctx* ctx, int n_iter, const void* X, void* Tb, void* V, void* Phi, double regularizer,
                      double p, double eps, double* loss, void* ws, int B, int F, int T, int K, int dtype,
                      void* stream) {
  int rc = cn_check(ctx, B, F, T, K, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, n_iter >= 0, ASSX_E_ARG, "assx_cnmf_iterate: n_iter = %d", n_iter);
  ASSX_REQUIRE(ctx, X && Tb && V && Phi && ws, ASSX_E_NULL, "assx_cnmf_iterate: NULL array");
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < n_iter; ++i) {
    // the residual pass of update i + 1 reads the model update i left: its sum is loss[i - 1]
    double* prev = (loss && i > 0) ? loss + (size_t)(i - 1) * B : nullptr;
    rc = cn_update(ctx, X, Tb, V, Phi, regularizer, p, eps, prev, ws, B, F, T, K, st);
    if (rc) return rc;
  }
  if (loss && n_iter > 0) return cn_loss(ctx, X, Tb, V, Phi, eps, loss + (size_t)(n_iter - 1) * B, ws, B, F, T, K, st);
  return 0;
}

}  // extern "C"
