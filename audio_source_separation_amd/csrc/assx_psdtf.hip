// LDPSDTF (log-det positive semidefinite tensor factorisation, src/algorithm/psdtf.py:88-176) on MI355X: the whole update
// on the device, on the workgroup-cooperative routines of assx_sym_linalg.hpp.
//
// Model Y_t = sum_k H[k,t] V_k for a target of T symmetric M x M matrices.  State (leading batch axis B, float64, matrices
// contiguous): X (B,T,M,M) target, V (B,K,M,M) basis, H (B,K,T) activation.  psd(A) = to_PSD of the reference: symmetrise,
// subtract min(lambda_min, 0) I, add eps trace I; it follows every constructed matrix, as in the reference.  One update:
//
//   pt_prep_kernel      one workgroup per (b, t):  Y = psd(sum_k H V_k), Yi = psd(Y^-1), Z = psd(Yi X Yi); Yi and Z go to
//                       the workspace
//   pt_contract_kernel  sum_t H[k,t] Yi_t and sum_t H[k,t] Z_t: a (K x T)(T x M^2) product on the vector ALU, one thread
//                       per matrix entry, the frames of a slab in index order, 8 bases at a time; the slabs (at most 16, a
//                       function of T alone) are added in index order by the next kernel
//   pt_basis_kernel     one workgroup per (b, k):  P = psd(sum), Q = psd(sum), L = chol(Q), G = V L,
//                       C = psd(G^T P G), S = psd(C^1/2)^-1 (eigenvalues clamped at 0 before the root), V <- psd(G S G^T).
//                       G S G^T is the reference's V L S L^T V for the symmetric V the model keeps
//   pt_act_kernel       one workgroup per (b, t):  Y and Yi again from the new V, W = Yi X Yi (no psd), then one wave per
//                       basis: num = tr(V_k W), den = tr(V_k Yi), H <- H sqrt(max(num, 0) / max(den, eps))
//   pt_norm_kernel      one workgroup per (b, k):  V_k /= tr V_k, H[k,:] *= tr V_k
//
// The loss is sum_t tr(X Y^-1) - (logdet X - logdet Y) - M with Y = psd(sum_k H V_k) and both sets of eigenvalues (Jacobi)
// floored at eps; the log-determinants of X are computed by pt_ldx_kernel, once per assx_psdtf_iterate call.
//
// A matrix that is not positive definite where the method inverts or factors it sets ASSX_STATUS_SINGULAR in the batch
// entry's status word, a Jacobi solve that ran out of sweeps ASSX_STATUS_NOT_CONVERGED; the kernels finish either way.  No
// float atomics, no partition that depends on B, every sum in a fixed order: two runs give the same bits, a batch those
// of its single calls, assx_psdtf_iterate those of assx_psdtf_update + assx_psdtf_loss.
#include "assx_common.hpp"
#include "assx_sym_linalg.hpp"

using namespace assx;
using sl::BLK;
using sl::LD;
using sl::MAT;
using sl::NW;
using sl::Scratch;

namespace {

constexpr int MMAX = sl::NMAX;
using mf::KMAX;
constexpr int KC = 8;       // bases of one pass of the contraction
constexpr int S_MAX = 16;   // frame slabs of the contraction, at least 64 frames each

inline int pt_slabs(int T) {
  const int s = (T + 63) / 64;
  return s > S_MAX ? S_MAX : s;
}

struct PtLayout {
  size_t yinv, zz, part, ldx, lossp, total;
};

// yinv, zz: Yi_t and Z_t (B,T,M,M); part: slab partials of the two contractions (B,S,2,K,M,M); ldx: sum log max(lambda(X_t),
// eps) (B,T); lossp: the loss per frame (B,T)
PtLayout pt_layout(int B, int M, int T, int K) {
  const size_t d = sizeof(double), mm = (size_t)M * M;
  mf::Carve c(1);
  PtLayout L;
  L.yinv = c.take((size_t)B * T * mm * d);
  L.zz = c.take((size_t)B * T * mm * d);
  L.part = c.take((size_t)B * pt_slabs(T) * 2 * K * mm * d);
  L.ldx = c.take((size_t)B * T * d);
  L.lossp = c.take((size_t)B * T * d);
  L.total = c.total();
  return L;
}

__device__ __forceinline__ void pt_flag(int32_t* status, size_t b, int st) {
  if (st && status && threadIdx.x == 0) atomicOr(status + b, st);
}

// A = sum_k H[k,t] V_k
__device__ __forceinline__ void pt_build_y(double* A, const double* __restrict__ Vb, const double* __restrict__ Hb, int t,
                                           int M, int T, int K) {
  const int mm = M * M;
  for (int e = threadIdx.x; e < mm; e += BLK) {
    double acc = 0;
    for (int k = 0; k < K; ++k) acc += Hb[(size_t)k * T + t] * Vb[(size_t)k * mm + e];
    A[(e / M) * LD + e % M] = acc;
  }
  __syncthreads();
}

// A = psd(sum_k H V_k); with INV: A = psd(A^-1) after that.  Bm, C scratch.
template <bool INV>
__device__ __forceinline__ int pt_model(double* A, double* Bm, double* C, const double* __restrict__ Vb,
                                        const double* __restrict__ Hb, int t, int M, int T, int K, double eps,
                                        Scratch& s) {
  pt_build_y(A, Vb, Hb, t, M, T, K);
  int st = sl::to_psd(A, Bm, M, eps, s);
  if (INV) {
    if (!sl::spd_inv(A, Bm, C, M, s)) st |= sl::ST_SINGULAR;
    st |= sl::to_psd(A, Bm, M, eps, s);
  }
  return st;
}

__global__ void __launch_bounds__(BLK) pt_prep_kernel(const double* __restrict__ X, const double* __restrict__ V,
                                                      const double* __restrict__ H, double* __restrict__ yinv,
                                                      double* __restrict__ zz, int32_t* status, double eps, int M, int T,
                                                      int K) {
  __shared__ double buf[3 * MAT];
  __shared__ Scratch s;
  double *A = buf, *Bm = buf + MAT, *C = buf + 2 * MAT;
  const size_t bt = blockIdx.x, b = bt / T, mm = (size_t)M * M;
  const int t = (int)(bt % T);
  int st = pt_model<true>(A, Bm, C, V + b * K * mm, H + b * K * T, t, M, T, K, eps, s);
  sl::store(A, yinv + bt * mm, M);
  sl::load(X + bt * mm, Bm, M);
  sl::matmul<false, false>(A, Bm, C, M);
  sl::matmul<false, false>(C, A, Bm, M);
  st |= sl::to_psd(Bm, C, M, eps, s);
  sl::store(Bm, zz + bt * mm, M);
  pt_flag(status, b, st);
}

// grid: (b * S + slab) * eblocks + entry block
__global__ void __launch_bounds__(BLK) pt_contract_kernel(const double* __restrict__ H, const double* __restrict__ yinv,
                                                          const double* __restrict__ zz, double* __restrict__ part, int M,
                                                          int T, int K, int S, int eblocks) {
  const size_t mm = (size_t)M * M;
  const size_t bs = blockIdx.x / eblocks, b = bs / S;
  const int slab = (int)(bs % S);
  const size_t e = (size_t)(blockIdx.x % eblocks) * BLK + threadIdx.x;
  if (e >= mm) return;
  const int t0 = (int)((size_t)slab * T / S), t1 = (int)((size_t)(slab + 1) * T / S);
  const double* Hb = H + b * K * T;
  for (int k0 = 0; k0 < K; k0 += KC) {
    double p[KC], q[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) p[c] = 0, q[c] = 0;
    for (int t = t0; t < t1; ++t) {
      const double y = yinv[(b * T + t) * mm + e], z = zz[(b * T + t) * mm + e];
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const double h = Hb[(size_t)min(k0 + c, K - 1) * T + t];
        p[c] += h * y;
        q[c] += h * z;
      }
    }
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      if (k0 + c < K) {
        part[((bs * 2 + 0) * K + k0 + c) * mm + e] = p[c];
        part[((bs * 2 + 1) * K + k0 + c) * mm + e] = q[c];
      }
    }
  }
}

// A = the slab partials of contraction `which` for basis k, added in slab order
__device__ __forceinline__ void pt_sum_slabs(double* A, const double* __restrict__ part, size_t b, int k, int which, int M,
                                             int K, int S) {
  const size_t mm = (size_t)M * M;
  for (int e = threadIdx.x; e < (int)mm; e += BLK) {
    double acc = part[(((b * S + 0) * 2 + which) * K + k) * mm + e];
    for (int sl_ = 1; sl_ < S; ++sl_) acc += part[(((b * S + sl_) * 2 + which) * K + k) * mm + e];
    A[(e / M) * LD + e % M] = acc;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(BLK) pt_basis_kernel(double* V, const double* __restrict__ part, int32_t* status, double eps,
                                                       int M, int K, int S) {
  __shared__ double buf[4 * MAT];
  __shared__ Scratch s;
  double *A = buf, *Bm = buf + MAT, *C = buf + 2 * MAT, *D = buf + 3 * MAT;
  const size_t bk = blockIdx.x, b = bk / K, mm = (size_t)M * M;
  const int k = (int)(bk % K);
  pt_sum_slabs(Bm, part, b, k, 0, M, K, S);
  int st = sl::to_psd(Bm, C, M, eps, s);  // P
  pt_sum_slabs(A, part, b, k, 1, M, K, S);
  st |= sl::to_psd(A, C, M, eps, s);  // Q
  if (!sl::chol(A, M, 0.0, s)) st |= sl::ST_SINGULAR;  // L
  sl::load(V + bk * mm, C, M);
  sl::matmul<false, false>(C, A, D, M);   // G = V L
  sl::matmul<false, false>(Bm, D, C, M);  // P G
  sl::matmul<true, false>(D, C, Bm, M);   // G^T P G
  st |= sl::to_psd(Bm, C, M, eps, s);
  if (!sl::jacobi(Bm, C, M, s)) st |= sl::ST_NOT_CONVERGED;
  if (threadIdx.x < M) A[threadIdx.x] = sqrt(fmax(Bm[threadIdx.x * LD + threadIdx.x], 0.0));
  __syncthreads();
  for (int e = threadIdx.x; e < (int)mm; e += BLK) {
    const int i = e / M, j = e % M;
    double acc = 0;
    for (int q = 0; q < M; ++q) acc += C[i * LD + q] * A[q] * C[j * LD + q];
    Bm[i * LD + j] = acc;
  }
  __syncthreads();
  st |= sl::to_psd(Bm, A, M, eps, s);
  if (!sl::spd_inv(Bm, A, C, M, s)) st |= sl::ST_SINGULAR;  // S
  sl::matmul<false, false>(D, Bm, C, M);  // G S
  sl::matmul<false, true>(C, D, Bm, M);   // G S G^T
  st |= sl::to_psd(Bm, C, M, eps, s);
  sl::store(Bm, V + bk * mm, M);
  pt_flag(status, b, st);
}

__global__ void __launch_bounds__(BLK) pt_act_kernel(const double* __restrict__ X, const double* __restrict__ V, double* H,
                                                     int32_t* status, double eps, int M, int T, int K) {
  __shared__ double buf[3 * MAT];
  __shared__ Scratch s;
  double *A = buf, *Bm = buf + MAT, *C = buf + 2 * MAT;
  const size_t bt = blockIdx.x, b = bt / T, mm = (size_t)M * M;
  const int t = (int)(bt % T);
  double* Hb = H + b * K * T;
  const int st = pt_model<true>(A, Bm, C, V + b * K * mm, Hb, t, M, T, K, eps, s);
  sl::load(X + bt * mm, Bm, M);
  sl::matmul<false, false>(A, Bm, C, M);
  sl::matmul<false, false>(C, A, Bm, M);  // W = Yi X Yi
  for (int k = threadIdx.x / WAVE; k < K; k += NW) {
    const double* Vk = V + (b * K + k) * mm;
    const double num = sl::wave_trace_prod(Bm, Vk, M), den = sl::wave_trace_prod(A, Vk, M);
    if ((threadIdx.x & (WAVE - 1)) == 0) {
      const size_t o = (size_t)k * T + t;
      Hb[o] = Hb[o] * sqrt(fmax(num, 0.0) / fmax(den, eps));
    }
  }
  pt_flag(status, b, st);
}

__global__ void __launch_bounds__(BLK) pt_norm_kernel(double* V, double* H, int M, int T, int K) {
  __shared__ double tr_s;
  const size_t bk = blockIdx.x, mm = (size_t)M * M;
  double* Vk = V + bk * mm;
  if (threadIdx.x == 0) {
    double tr = 0;
    for (int i = 0; i < M; ++i) tr += Vk[(size_t)i * M + i];
    tr_s = tr;
  }
  __syncthreads();
  const double tr = tr_s;
  for (int e = threadIdx.x; e < (int)mm; e += BLK) Vk[e] = Vk[e] / tr;
  for (int t = threadIdx.x; t < T; t += BLK) H[bk * T + t] = H[bk * T + t] * tr;
}

// sum_i log max(lambda_i, eps) of the eigenvalues on the diagonal of A
__device__ __forceinline__ double pt_logdet(const double* A, int M, double eps, Scratch& s) {
  return mf::block_sum_all(threadIdx.x < M ? log(fmax(A[threadIdx.x * LD + threadIdx.x], eps)) : 0.0, s.red);
}

__global__ void __launch_bounds__(BLK) pt_ldx_kernel(const double* __restrict__ X, double* __restrict__ ldx, int32_t* status,
                                                     double eps, int M, int T) {
  __shared__ double buf[MAT];
  __shared__ Scratch s;
  const size_t bt = blockIdx.x;
  sl::load(X + bt * M * M, buf, M);
  sl::symmetrize(buf, M);
  const int st = sl::jacobi(buf, nullptr, M, s) ? 0 : sl::ST_NOT_CONVERGED;
  const double ld = pt_logdet(buf, M, eps, s);
  if (threadIdx.x == 0) ldx[bt] = ld;
  pt_flag(status, bt / T, st);
}

__global__ void __launch_bounds__(BLK) pt_loss_kernel(const double* __restrict__ X, const double* __restrict__ V,
                                                      const double* __restrict__ H, const double* __restrict__ ldx,
                                                      double* __restrict__ lossp, int32_t* status, double eps, int M, int T,
                                                      int K) {
  __shared__ double buf[3 * MAT];
  __shared__ Scratch s;
  double *A = buf, *Bm = buf + MAT, *C = buf + 2 * MAT;
  const size_t bt = blockIdx.x, b = bt / T, mm = (size_t)M * M;
  const int t = (int)(bt % T);
  int st = pt_model<false>(A, Bm, C, V + b * K * mm, H + b * K * T, t, M, T, K, eps, s);
  sl::copy(A, Bm, M);
  if (!sl::chol(Bm, M, 0.0, s)) st |= sl::ST_SINGULAR;
  sl::tri_inv(Bm, C, M);
  sl::ata(C, Bm, M);  // Y^-1
  double tr = 0;
  for (int e = threadIdx.x; e < (int)mm; e += BLK) tr += X[bt * mm + e] * Bm[(e % M) * LD + e / M];
  tr = mf::block_sum_all(tr, s.red);
  if (!sl::jacobi(A, nullptr, M, s)) st |= sl::ST_NOT_CONVERGED;
  const double ldy = pt_logdet(A, M, eps, s);
  if (threadIdx.x == 0) lossp[bt] = tr - (ldx[bt] - ldy) - M;
  pt_flag(status, b, st);
}

__global__ void __launch_bounds__(BLK) pt_recon_kernel(const double* __restrict__ V, const double* __restrict__ H,
                                                       double* __restrict__ Xh, int M, int T, int K) {
  const size_t bt = blockIdx.x, b = bt / T, mm = (size_t)M * M;
  const int t = (int)(bt % T);
  for (int e = threadIdx.x; e < (int)mm; e += BLK) {
    double acc = 0;
    for (int k = 0; k < K; ++k) acc += H[(b * K + k) * T + t] * V[(b * K + k) * mm + e];
    Xh[bt * mm + e] = acc;
  }
}

__global__ void __launch_bounds__(BLK) pt_topsd_kernel(double* Am, double eps, int M) {
  __shared__ double buf[2 * MAT];
  __shared__ Scratch s;
  double* G = Am + (size_t)blockIdx.x * M * M;
  sl::load(G, buf, M);
  sl::to_psd(buf, buf + MAT, M, eps, s);
  sl::store(buf, G, M);
}

struct PtDims {
  int B, M, T, K;
};

int pt_check(assx_ctx* ctx, PtDims d, int dtype) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, d.B >= 1 && d.T >= 1, ASSX_E_ARG, "LDPSDTF: invalid sizes B=%d T=%d", d.B, d.T);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64 || dtype == ASSX_F32, ASSX_E_ARG, "bad dtype %d", dtype);
  ASSX_REQUIRE(ctx, d.M >= 1 && d.M <= MMAX, ASSX_E_ARG, "LDPSDTF: n_bins must be in [1, 64], got %d", d.M);
  ASSX_REQUIRE(ctx, d.K >= 1 && d.K <= KMAX, ASSX_E_ARG, "LDPSDTF: n_basis must be in [1, 64], got %d", d.K);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64, ASSX_E_UNSUPPORTED, "LDPSDTF: float64 only");
  // one workgroup of 256 threads per (b, t), per (b, k) and per (b, slab, 256 entries), and a launch holds fewer than 2^32
  // threads: B T < 2^24 for the frames, B < 2^16 for the bases (K <= 64) and the contraction (16 slabs x 16 entry blocks)
  const long long lim = 1LL << 24;
  ASSX_REQUIRE(ctx, (long long)d.B * d.T < lim && (long long)d.B * S_MAX * 16 < lim, ASSX_E_ARG,
               "LDPSDTF: B=%d T=%d needs more workgroups than a launch can have (B T < 2^24, B < 2^16)", d.B, d.T);
  return 0;
}

int pt_update_basis(assx_ctx* ctx, const double* X, double* V, const double* H, double eps, int32_t* status, void* ws, PtDims d,
                    hipStream_t st) {
  const PtLayout L = pt_layout(d.B, d.M, d.T, d.K);
  char* w = (char*)ws;
  double *yinv = (double*)(w + L.yinv), *zz = (double*)(w + L.zz), *part = (double*)(w + L.part);
  hipLaunchKernelGGL(pt_prep_kernel, dim3((unsigned)(d.B * d.T)), dim3(BLK), 0, st, X, (const double*)V, H, yinv, zz,
                     status, eps, d.M, d.T, d.K);
  ASSX_LAUNCH_CHECK(ctx, "pt_prep_kernel");
  const int S = pt_slabs(d.T), eblocks = (d.M * d.M + BLK - 1) / BLK;
  hipLaunchKernelGGL(pt_contract_kernel, dim3((unsigned)(d.B * S * eblocks)), dim3(BLK), 0, st, H, (const double*)yinv,
                     (const double*)zz, part, d.M, d.T, d.K, S, eblocks);
  ASSX_LAUNCH_CHECK(ctx, "pt_contract_kernel");
  hipLaunchKernelGGL(pt_basis_kernel, dim3((unsigned)(d.B * d.K)), dim3(BLK), 0, st, V, (const double*)part, status, eps,
                     d.M, d.K, S);
  ASSX_LAUNCH_CHECK(ctx, "pt_basis_kernel");
  return 0;
}

int pt_update_activation(assx_ctx* ctx, const double* X, const double* V, double* H, double eps, int32_t* status, PtDims d,
                         hipStream_t st) {
  hipLaunchKernelGGL(pt_act_kernel, dim3((unsigned)(d.B * d.T)), dim3(BLK), 0, st, X, V, H, status, eps, d.M, d.T, d.K);
  ASSX_LAUNCH_CHECK(ctx, "pt_act_kernel");
  return 0;
}

int pt_normalize(assx_ctx* ctx, double* V, double* H, PtDims d, hipStream_t st) {
  hipLaunchKernelGGL(pt_norm_kernel, dim3((unsigned)(d.B * d.K)), dim3(BLK), 0, st, V, H, d.M, d.T, d.K);
  ASSX_LAUNCH_CHECK(ctx, "pt_norm_kernel");
  return 0;
}

int pt_update(assx_ctx* ctx, const double* X, double* V, double* H, double eps, int normalize, int32_t* status, void* ws,
              PtDims d, hipStream_t st) {
  int rc = pt_update_basis(ctx, X, V, H, eps, status, ws, d, st);
  if (rc) return rc;
  rc = pt_update_activation(ctx, X, V, H, eps, status, d, st);
  if (rc) return rc;
  return normalize ? pt_normalize(ctx, V, H, d, st) : 0;
}

int pt_ldx(assx_ctx* ctx, const double* X, double eps, int32_t* status, void* ws, PtDims d, hipStream_t st) {
  const PtLayout L = pt_layout(d.B, d.M, d.T, d.K);
  hipLaunchKernelGGL(pt_ldx_kernel, dim3((unsigned)(d.B * d.T)), dim3(BLK), 0, st, X, (double*)((char*)ws + L.ldx), status,
                     eps, d.M, d.T);
  ASSX_LAUNCH_CHECK(ctx, "pt_ldx_kernel");
  return 0;
}

// the log-determinants of X must be in the workspace (pt_ldx)
int pt_loss(assx_ctx* ctx, const double* X, const double* V, const double* H, double eps, double* loss, int32_t* status,
            void* ws, PtDims d, hipStream_t st) {
  const PtLayout L = pt_layout(d.B, d.M, d.T, d.K);
  double* lossp = (double*)((char*)ws + L.lossp);
  hipLaunchKernelGGL(pt_loss_kernel, dim3((unsigned)(d.B * d.T)), dim3(BLK), 0, st, X, V, H,
                     (const double*)((char*)ws + L.ldx), lossp, status, eps, d.M, d.T, d.K);
  ASSX_LAUNCH_CHECK(ctx, "pt_loss_kernel");
  hipLaunchKernelGGL(mf::batch_sum_kernel<true>, dim3((unsigned)d.B), dim3(BLK), 0, st, (const double*)lossp, loss, d.T);
  ASSX_LAUNCH_CHECK(ctx, "batch_sum_kernel");
  return 0;
}

}  // namespace

extern "C" {

size_t assx_psdtf_workspace_bytes(int B, int M, int T, int K, int dtype) {
  if (dtype != ASSX_F64 || B < 1 || T < 1 || M < 1 || M > MMAX || K < 1 || K > KMAX) return 0;
  return pt_layout(B, M, T, K).total;
}

int assx_psdtf_to_psd(assx_ctx* ctx, void* A, int n_mat, int M, double eps, void* stream) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, n_mat >= 1 && n_mat < (1 << 24) && M >= 1 && M <= MMAX, ASSX_E_ARG,
               "assx_psdtf_to_psd: n_mat=%d M=%d (n_mat in [1, 2^24), M in [1, 64])", n_mat, M);
  ASSX_REQUIRE(ctx, A, ASSX_E_NULL, "assx_psdtf_to_psd: NULL array");
  hipLaunchKernelGGL(pt_topsd_kernel, dim3((unsigned)n_mat), dim3(BLK), 0, (hipStream_t)stream, (double*)A, eps, M);
  ASSX_LAUNCH_CHECK(ctx, "pt_topsd_kernel");
  return 0;
}

int assx_psdtf_update_basis(assx_ctx* ctx, const void* X, void* V, const void* H, double eps, int32_t* status, void* ws, int B,
                            int M, int T, int K, int dtype, void* stream) {
  const PtDims d{B, M, T, K};
  int rc = pt_check(ctx, d, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && V && H && ws, ASSX_E_NULL, "assx_psdtf_update_basis: NULL array");
  return pt_update_basis(ctx, (const double*)X, (double*)V, (const double*)H, eps, status, ws, d, (hipStream_t)stream);
}

int assx_psdtf_update_activation(assx_ctx* ctx, const void* X, const void* V, void* H, double eps, int32_t* status, int B, int M,
                                 int T, int K, int dtype, void* stream) {
  const PtDims d{B, M, T, K};
  int rc = pt_check(ctx, d, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && V && H, ASSX_E_NULL, "assx_psdtf_update_activation: NULL array");
  return pt_update_activation(ctx, (const double*)X, (const double*)V, (double*)H, eps, status, d, (hipStream_t)stream);
}

int assx_psdtf_normalize(assx_ctx* ctx, void* V, void* H, int B, int M, int T, int K, int dtype, void* stream) {
  const PtDims d{B, M, T, K};
  int rc = pt_check(ctx, d, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, V && H, ASSX_E_NULL, "assx_psdtf_normalize: NULL array");
  return pt_normalize(ctx, (double*)V, (double*)H, d, (hipStream_t)stream);
}

int assx_psdtf_update(assx_ctx* ctx, const void* X, void* V, void* H, double eps, int normalize, int32_t* status, void* ws,
                      int B, int M, int T, int K, int dtype, void* stream) {
  const PtDims d{B, M, T, K};
  int rc = pt_check(ctx, d, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && V && H && ws, ASSX_E_NULL, "assx_psdtf_update: NULL array");
  return pt_update(ctx, (const double*)X, (double*)V, (double*)H, eps, normalize, status, ws, d, (hipStream_t)stream);
}

int assx_psdtf_loss(assx_ctx* ctx, const void* X, const void* V, const void* H, double eps, double* loss, int32_t* status,
                    void* ws, int B, int M, int T, int K, int dtype, void* stream) {
  const PtDims d{B, M, T, K};
  int rc = pt_check(ctx, d, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && V && H && loss && ws, ASSX_E_NULL, "assx_psdtf_loss: NULL array");
  rc = pt_ldx(ctx, (const double*)X, eps, status, ws, d, (hipStream_t)stream);
  if (rc) return rc;
  return pt_loss(ctx, (const double*)X, (const double*)V, (const double*)H, eps, loss, status, ws, d, (hipStream_t)stream);
}

int assx_psdtf_reconstruct(assx_ctx* ctx, const void* V, const void* H, void* Xh, int B, int M, int T, int K, int dtype,
                           void* stream) {
  const PtDims d{B, M, T, K};
  int rc = pt_check(ctx, d, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, V && H && Xh, ASSX_E_NULL, "assx_psdtf_reconstruct: NULL array");
  hipLaunchKernelGGL(pt_recon_kernel, dim3((unsigned)(B * T)), dim3(BLK), 0, (hipStream_t)stream, (const double*)V,
                     (const double*)H, (double*)Xh, M, T, K);
  ASSX_LAUNCH_CHECK(ctx, "pt_recon_kernel");
  return 0;
}

int assx_psdtf_iterate(assx_ctx* ctx, int n_iter, const void* X, void* V, void* H, double eps, int normalize, double* loss,
                       int32_t* status, void* ws, int B, int M, int T, int K, int dtype, void* stream) {
  const PtDims d{B, M, T, K};
  int rc = pt_check(ctx, d, dtype);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, n_iter >= 0, ASSX_E_ARG, "assx_psdtf_iterate: n_iter = %d", n_iter);
  ASSX_REQUIRE(ctx, X && V && H && ws, ASSX_E_NULL, "assx_psdtf_iterate: NULL array");
  hipStream_t st = (hipStream_t)stream;
  if (loss && n_iter > 0) {
    rc = pt_ldx(ctx, (const double*)X, eps, status, ws, d, st);
    if (rc) return rc;
  }
  for (int it = 0; it < n_iter; ++it) {
    rc = pt_update(ctx, (const double*)X, (double*)V, (double*)H, eps, normalize, status, ws, d, st);
    if (rc) return rc;
    if (loss) {
      rc = pt_loss(ctx, (const double*)X, (const double*)V, (const double*)H, eps, loss + (size_t)it * B, status, ws, d, st);
      if (rc) return rc;
    }
  }
  return 0;
}

}  // extern "C"
