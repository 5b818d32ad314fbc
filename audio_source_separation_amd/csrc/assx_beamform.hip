// The closed-form spatial filters of the reference on MI355X: the delay-and-sum, ML and MVDR beamformers
// (src/bss/beamform.py:5-58), the per-bin PCA front end (src/transform/pca.py:4-21) and the minimum distortion principle
// (src/algorithm/minimum_distortion_principle.py:3-31).  float64, one utterance, 2 <= M <= 8 channels, 1 <= N <= 8 sources,
// the two need not be equal.
//
// Arrays: X (M,F,T) complex128 with T fastest, the steering vectors A (F,M,N), a covariance R or C (F,M,M), a filter
// Wf (F,N,M) with an optional scale s (F,N), the output Y (N,F,T).
//
// Launches:
//   apply      bf_apply_kernel (bin x frame tile, a flat grid): lanes along t, the M samples of a frame in registers,
//              the bin's filter read through wave-uniform addresses; Y[n,f,t] = s[f,n] sum_m Wf[f,n,m] X[m,f,t].  The one
//              streaming pass that all three beamformers and PCA end in
//   weights    bf_ds_weights_kernel (an entry of Wf per thread), bf_ml_weights_kernel and pca_basis_kernel (a bin per
//              thread, the M x M matrix in registers): the inverse by elimination with partial pivoting (gj_inverse of
//              assx_small_linalg.hpp, LAPACK's pivot rule), the eigenvectors by cyclic Jacobi (herm_jacobi of
//              assx_herm_linalg.hpp, the routine herm_sqrt_psd runs on)
//   MDP        mdp_partial_kernel (bin x frame chunk x reference channel): sum_t conj(Y) X and sum_t |Y|^2 of one chunk,
//              a wave's butterfly, then the waves in index order; mdp_close_kernel: the chunks in index order, the division
// The plain covariance of MVDR and PCA is assx_cov_accumulate with ASSX_W_NONE; nothing here forms one.
//
// Every sum has a fixed order and there is no float atomic: two runs give the same bits.
#include "assx_herm_linalg.hpp"
#include "assx_perbin_common.hpp"

using namespace assx;
using namespace assx::mf;
using namespace assx::pb;

namespace {

constexpr int BF_CHUNK = ASSX_BF_FRAME_CHUNK;  // frames of one MDP workgroup

static_assert(BF_CHUNK % BLK == 0, "a chunk is whole trips of the workgroup");

// rows: the larger of the two channel counts of a call (X and Y, or Y and the reference)
inline bool bf_sizes_ok(int rows, int F, int T) {
  if (F < 1 || T < 1 || F >= (1 << 28) || T >= (1 << 28)) return false;
  return (long long)rows * F * T < (1LL << 28);  // every array stays below 4 GiB; no product below overflows
}

inline bool bf_in_envelope(int M, int N, int F, int T) {
  return M >= 2 && M <= 8 && N >= 1 && N <= NMAX && bf_sizes_ok(M > N ? M : N, F, T);
}

inline bool mdp_in_envelope(int C, int N, int F, int T) {
  return C >= 1 && C <= 8 && N >= 1 && N <= NMAX && bf_sizes_ok(C > N ? C : N, F, T);
}

inline int bf_chunks(int T) { return chunks(T, BF_CHUNK); }

// part (F, chunks, C, N, 3): Re and Im of sum_t conj(Y) X and sum_t |Y|^2 of one chunk
inline size_t mdp_ws_bytes(int C, int N, int F, int T) {
  Carve c(256);
  c.take((size_t)F * bf_chunks(T) * C * N * 3 * sizeof(double));
  return c.total();
}

// ---------------------------------------------------------------------------------------------------------------
// Y[n,f,t] = s[f,n] sum_m Wf[f,n,m] X[m,f,t]; s may be NULL.  Workgroup f NTILE + tile, one lane per frame.
// ---------------------------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__(BLK) bf_apply_kernel(const Cd* __restrict__ X, const Cd* __restrict__ Wf,
                                                       const Cd* __restrict__ s, Cd* __restrict__ Y, int N, int F, int T,
                                                       int NTILE) {
  const int f = blockIdx.x / NTILE, t = (blockIdx.x % NTILE) * BLK + threadIdx.x;
  if (t >= T) return;
  Cd x[M];
  load_frame<M>(X, f, t, F, T, x);
  const Cd* Wb = Wf + (size_t)f * N * M;
  for (int n = 0; n < N; ++n) {
    Cd y = cmake<double>(0.0, 0.0);
#pragma unroll
    for (int m = 0; m < M; ++m) cfma(y, Wb[n * M + m], x[m]);
    if (s) y = cmul(s[(size_t)f * N + n], y);
    Y[((size_t)n * F + f) * T + t] = y;
  }
}

// beamform.py:14-17: Wf[f,n,m] = conj(A[f,m,n]), s[f,n] = A[f,ref,n]
__global__ void __launch_bounds__(BLK) bf_ds_weights_kernel(const Cd* __restrict__ A, Cd* __restrict__ Wf,
                                                            Cd* __restrict__ s, int ref, int M, int N, size_t total) {
  const size_t i = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (i >= total) return;
  const int m = (int)(i % M), n = (int)(i / M % N);
  const size_t f = i / ((size_t)M * N);
  Wf[i] = cconj(A[(f * M + m) * N + n]);
  if (m == 0) s[f * N + n] = A[(f * M + ref) * N + n];
}

// beamform.py:32-42, one bin per thread: Num = R^-1 A, den[n] = sum_m conj(A[m,n]) Num[m,n], den = eps where den < eps in
// NumPy's order of complex numbers (the real parts, the imaginary parts on a tie; false where an imaginary part is not a
// number), Wf[f,n,m] = Num[m,n] / den[n] -- transposed, not conjugated, as the reference has it -- and s[f,n] = A[f,ref,n].
// An exactly zero pivot sets ASSX_STATUS_SINGULAR; the kernel finishes either way.
template <int M>
__global__ void __launch_bounds__(WAVE) bf_ml_weights_kernel(const Cd* __restrict__ A, const Cd* __restrict__ R,
                                                             Cd* __restrict__ Wf, Cd* __restrict__ s, int ref, double eps,
                                                             int N, int F, int32_t* __restrict__ status) {
  const int f = blockIdx.x * WAVE + threadIdx.x;
  if (f >= F) return;
  Cd Ri[M][M];
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) Ri[i][j] = R[((size_t)f * M + i) * M + j];
  if (!gj_inverse<M>(Ri, nullptr) && status) atomicOr(status, (int32_t)ASSX_STATUS_SINGULAR);
  const Cd* Af = A + (size_t)f * M * N;
  for (int n = 0; n < N; ++n) {
    Cd a[M], num[M];
#pragma unroll
    for (int m = 0; m < M; ++m) a[m] = Af[m * N + n];
    Cd den = cmake<double>(0.0, 0.0);
#pragma unroll
    for (int m = 0; m < M; ++m) {
      num[m] = cmake<double>(0.0, 0.0);
#pragma unroll
      for (int j = 0; j < M; ++j) cfma(num[m], Ri[m][j], a[j]);
      den.x = fma(a[m].x, num[m].x, den.x), den.x = fma(a[m].y, num[m].y, den.x);  // conj(a) num
      den.y = fma(a[m].x, num[m].y, den.y), den.y = fma(-a[m].y, num[m].x, den.y);
    }
    if ((den.x < eps && den.y == den.y) || (den.x == eps && den.y < 0.0)) den = cmake<double>(eps, 0.0);
#pragma unroll
    for (int m = 0; m < M; ++m) Wf[((size_t)f * N + n) * M + m] = cdiv(num[m], den);
    s[(size_t)f * N + n] = Af[ref * N + n];
  }
}

// pca.py:15-16, one bin per thread: C = V diag(w) V^H from the lower triangle of C (numpy.linalg.eigh reads the same one),
// w ascending, equal eigenvalues in the order of their Jacobi columns; every eigenvector times the unit phase that makes
// its first entry real and non-negative (left alone where that entry is zero); Wf[f,k,m] = conj(V[f,m,k]).
template <int M>
__global__ void __launch_bounds__(WAVE) pca_basis_kernel(const Cd* __restrict__ C, Cd* __restrict__ V, double* __restrict__ w,
                                                         Cd* __restrict__ Wf, int F, int32_t* __restrict__ status) {
  const int f = blockIdx.x * WAVE + threadIdx.x;
  if (f >= F) return;
  herm::Mat<M> Cm, U;
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      const Cd v = C[((size_t)f * M + i) * M + j];
      Cm.re[i][j] = v.x, Cm.im[i][j] = v.y;
    }
  herm::mirror_lower(Cm);
  if (!herm::herm_jacobi(Cm, U) && status) atomicOr(status, (int32_t)ASSX_STATUS_NOT_CONVERGED);
#pragma unroll
  for (int k = 0; k < M; ++k) {
    int rank = 0;
#pragma unroll
    for (int j = 0; j < M; ++j) rank += (Cm.re[j][j] < Cm.re[k][k] || (Cm.re[j][j] == Cm.re[k][k] && j < k)) ? 1 : 0;
    const double ar = U.re[0][k], ai = U.im[0][k], g = hypot(ar, ai);
    const double pr = g > 0.0 ? ar / g : 1.0, pi = g > 0.0 ? -ai / g : 0.0;  // conj(a) / |a|
    w[(size_t)f * M + rank] = Cm.re[k][k];
#pragma unroll
    for (int m = 0; m < M; ++m) {
      Cd v = cmake<double>(U.re[m][k] * pr - U.im[m][k] * pi, U.re[m][k] * pi + U.im[m][k] * pr);
      if (m == 0 && g > 0.0) v = cmake<double>(g, 0.0);
      V[((size_t)f * M + m) * M + rank] = v;
      Wf[((size_t)f * M + rank) * M + m] = cconj(v);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// MDP, minimum_distortion_principle.py:24-25.  Workgroup (f CH + ch) C + c takes chunk ch of bin f against reference
// channel c; the C workgroups of a chunk are neighbours in the grid and find Y in the cache after the first of them.
// part[.., n, 0..2] = Re, Im of sum_t conj(Y[n]) X[c] and sum_t |Y[n]|^2.
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLK) mdp_partial_kernel(const Cd* __restrict__ Y, const Cd* __restrict__ Xr,
                                                          double* __restrict__ part, int C, int N, int F, int T, int CH) {
  __shared__ double red[NW][NMAX * 3];
  const int c = blockIdx.x % C, ch = blockIdx.x / C % CH, f = blockIdx.x / C / CH;
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  double ar[NMAX], ai[NMAX], ap[NMAX];
#pragma unroll
  for (int n = 0; n < NMAX; ++n) ar[n] = 0.0, ai[n] = 0.0, ap[n] = 0.0;
  const int t_end = chunk_end(ch, BF_CHUNK, T);
  for (int t = ch * BF_CHUNK + tid; t < t_end; t += BLK) {
    const Cd x = tocx(ldv(Xr + ((size_t)c * F + f) * T + t));
#pragma unroll
    for (int n = 0; n < NMAX; ++n)
      if (n < N) {
        const Cd y = tocx(ldv(Y + ((size_t)n * F + f) * T + t));
        ar[n] = fma(y.x, x.x, ar[n]), ar[n] = fma(y.y, x.y, ar[n]);  // conj(y) x
        ai[n] = fma(y.x, x.y, ai[n]), ai[n] = fma(-y.y, x.x, ai[n]);
        ap[n] = fma(y.x, y.x, ap[n]), ap[n] = fma(y.y, y.y, ap[n]);
      }
  }
#pragma unroll
  for (int n = 0; n < NMAX; ++n)
    if (n < N) {
      const double vr = wave_sum_down(ar[n]), vi = wave_sum_down(ai[n]), vp = wave_sum_down(ap[n]);
      if (lane == 0) red[wave][n * 3] = vr, red[wave][n * 3 + 1] = vi, red[wave][n * 3 + 2] = vp;
    }
  __syncthreads();
  if (tid < N * 3) {  // the waves in index order
    double v = red[0][tid];
    for (int q = 1; q < NW; ++q) v += red[q][tid];
    part[(size_t)blockIdx.x * N * 3 + tid] = v;
  }
}

// scale[c,n,f] = (the chunks of sum conj(Y) X in index order) / (those of sum |Y|^2): plain IEEE, 0 / 0 is NaN
__global__ void __launch_bounds__(BLK) mdp_close_kernel(const double* __restrict__ part, Cd* __restrict__ scale, int C, int N,
                                                        int F, int CH, size_t total) {
  const size_t i = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (i >= total) return;
  const int f = (int)(i % F), n = (int)(i / F % N), c = (int)(i / F / N);
  double sr = 0.0, si = 0.0, sp = 0.0;
  for (int ch = 0; ch < CH; ++ch) {
    const double* p = part + ((((size_t)f * CH + ch) * C + c) * N + n) * 3;
    sr += p[0], si += p[1], sp += p[2];
  }
  scale[i] = cmake<double>(sr / sp, si / sp);
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
int bf_check(assx_ctx* ctx, const char* who, int M, int N, int F, int T) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, F >= 1 && T >= 1, ASSX_E_ARG, "%s: invalid sizes F=%d T=%d", who, F, T);
  ASSX_REQUIRE(ctx, M >= 2 && M <= 8, ASSX_E_UNSUPPORTED, "%s: n_channels must be in [2, 8], got %d", who, M);
  ASSX_REQUIRE(ctx, N >= 1 && N <= NMAX, ASSX_E_UNSUPPORTED, "%s: n_sources must be in [1, 8], got %d", who, N);
  ASSX_REQUIRE(ctx, bf_in_envelope(M, N, F, T), ASSX_E_UNSUPPORTED,
               "%s: every array must stay below 4 GiB in complex128 (max(M, N)*F*T < 2^28)", who);
  return 0;
}

}  // namespace

extern "C" {

size_t assx_bf_workspace_bytes(int C, int N, int F, int T) {
  if (!mdp_in_envelope(C, N, F, T)) return 0;
  return mdp_ws_bytes(C, N, F, T);
}

int assx_bf_apply(assx_ctx* ctx, const void* X, const void* Wf, const void* s, void* Y, int M, int N, int F, int T,
                  void* stream) {
  int rc = bf_check(ctx, "assx_bf_apply", M, N, F, T);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && Wf && Y, ASSX_E_NULL, "assx_bf_apply: NULL array");
  const int ntile = (int)nblocks(T, BLK);
  return launch_for_channels(ctx, "assx_bf_apply", "bf_apply_kernel", M, [&](auto mt) {
    hipLaunchKernelGGL((bf_apply_kernel<decltype(mt)::value>), dim3((unsigned)F * ntile), dim3(BLK), 0, (hipStream_t)stream,
                       (const Cd*)X, (const Cd*)Wf, (const Cd*)s, (Cd*)Y, N, F, T, ntile);
  });
}

int assx_bf_ds_weights(assx_ctx* ctx, const void* A, void* Wf, void* s, int ref, int M, int N, int F, void* stream) {
  int rc = bf_check(ctx, "assx_bf_ds_weights", M, N, F, 1);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, ref >= 0 && ref < M, ASSX_E_ARG, "reference_id must be in [0, %d), got %d", M, ref);
  ASSX_REQUIRE(ctx, A && Wf && s, ASSX_E_NULL, "assx_bf_ds_weights: NULL array");
  const size_t total = (size_t)F * N * M;
  hipLaunchKernelGGL(bf_ds_weights_kernel, dim3(nblocks(total, BLK)), dim3(BLK), 0, (hipStream_t)stream, (const Cd*)A,
                     (Cd*)Wf, (Cd*)s, ref, M, N, total);
  ASSX_LAUNCH_CHECK(ctx, "bf_ds_weights_kernel");
  return 0;
}

int assx_bf_ml_weights(assx_ctx* ctx, const void* A, const void* R, void* Wf, void* s, int ref, double eps, int M, int N,
                       int F, int32_t* status, void* stream) {
  int rc = bf_check(ctx, "assx_bf_ml_weights", M, N, F, 1);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, ref >= 0 && ref < M, ASSX_E_ARG, "reference_id must be in [0, %d), got %d", M, ref);
  ASSX_REQUIRE(ctx, A && R && Wf && s, ASSX_E_NULL, "assx_bf_ml_weights: NULL array");
  return launch_for_channels(ctx, "assx_bf_ml_weights", "bf_ml_weights_kernel", M, [&](auto mt) {
    hipLaunchKernelGGL((bf_ml_weights_kernel<decltype(mt)::value>), dim3(nblocks(F, WAVE)), dim3(WAVE), 0,
                       (hipStream_t)stream, (const Cd*)A, (const Cd*)R, (Cd*)Wf, (Cd*)s, ref, eps, N, F, status);
  });
}

int assx_pca_basis(assx_ctx* ctx, const void* C, void* V, double* w, void* Wf, int M, int F, int32_t* status, void* stream) {
  int rc = bf_check(ctx, "assx_pca_basis", M, M, F, 1);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, C && V && w && Wf, ASSX_E_NULL, "assx_pca_basis: NULL array");
  return launch_for_channels(ctx, "assx_pca_basis", "pca_basis_kernel", M, [&](auto mt) {
    hipLaunchKernelGGL((pca_basis_kernel<decltype(mt)::value>), dim3(nblocks(F, WAVE)), dim3(WAVE), 0, (hipStream_t)stream,
                       (const Cd*)C, (Cd*)V, w, (Cd*)Wf, F, status);
  });
}

int assx_mdp_scale(assx_ctx* ctx, const void* Y, const void* Xref, void* scale, void* ws, int C, int N, int F, int T,
                   void* stream) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, F >= 1 && T >= 1, ASSX_E_ARG, "assx_mdp_scale: invalid sizes F=%d T=%d", F, T);
  ASSX_REQUIRE(ctx, C >= 1 && C <= 8, ASSX_E_UNSUPPORTED, "assx_mdp_scale: the reference must have 1 to 8 channels, got %d", C);
  ASSX_REQUIRE(ctx, N >= 1 && N <= NMAX, ASSX_E_UNSUPPORTED, "assx_mdp_scale: n_sources must be in [1, 8], got %d", N);
  ASSX_REQUIRE(ctx, mdp_in_envelope(C, N, F, T), ASSX_E_UNSUPPORTED,
               "assx_mdp_scale: every array must stay below 4 GiB in complex128 (max(C, N)*F*T < 2^28)");
  ASSX_REQUIRE(ctx, Y && Xref && scale && ws, ASSX_E_NULL, "assx_mdp_scale: NULL array");
  const int CH = bf_chunks(T);
  hipLaunchKernelGGL(mdp_partial_kernel, dim3((unsigned)F * CH * C), dim3(BLK), 0, (hipStream_t)stream, (const Cd*)Y,
                     (const Cd*)Xref, (double*)ws, C, N, F, T, CH);
  ASSX_LAUNCH_CHECK(ctx, "mdp_partial_kernel");
  const size_t total = (size_t)C * N * F;
  hipLaunchKernelGGL(mdp_close_kernel, dim3(nblocks(total, BLK)), dim3(BLK), 0, (hipStream_t)stream, (const double*)ws,
                     (Cd*)scale, C, N, F, CH, total);
  ASSX_LAUNCH_CHECK(ctx, "mdp_close_kernel");
  return 0;
}

}  // extern "C"
