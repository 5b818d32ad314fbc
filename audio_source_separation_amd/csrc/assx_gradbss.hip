// Gradient and natural-gradient Laplace IVA (src/bss/iva.py:130-287) and FDICA (src/bss/fdica.py:8-301) on MI355X: the
// update loop and FDICA's permutation solver on the device.  float64, one utterance, N = M sources, 2 <= M <= 8.
//
// State: X (M,F,T) complex128 with T fastest, W (F,M,M) complex128.  With y = W x per (f, t):
//   score      IVA    phi[n] = y[n] / max(r[n,t], eps),  r[n,t] = sqrt(sum_f |y[n,f,t]|^2)
//              FDICA  phi[n] = y[n] / max(|y[n]|, eps)
//   moment     G = (1/T) sum_t phi z^H,  z = x (gradient form) or z = y (natural form)
//   step       gradient  W <- W - lr (G - W^-H)        natural  W <- W - lr (G - I) W
//   loss       IVA  (2/T) sum_{n,t} r[n,t] - 2 sum_f ln|det W_f|       FDICA  (2/T) sum_{n,f,t} |y| - 2 sum_f ln|det W_f|
//
// Launches:
//   weights    gb_weight_kernel (frame tile x bin slice): sum_f |y|^2 of a slice of bins per frame, in registers;
//              gb_weight_sum_kernel: the slices in index order, r = sqrt, and the partial sums of r for the IVA loss
//   moment     gb_moment_kernel (bin x frame chunk, a flat grid): lanes are frames, the M x M cross-moment in registers
//              (rows split over two wave pairs at M >= 7), wave butterfly, the waves in index order through LDS, one
//              partial per chunk;
//              FDICA's sum of |y| rides on it
//   finalize   gb_finalize_kernel, one wave per bin: the chunk partials in index order, / T, the step, W, ln|det W|; an
//              exactly zero pivot of the inverse sets ASSX_STATUS_SINGULAR.  mode 0 only takes ln|det W|
//   close      gb_loss_close_kernel: the data partials and the log-determinants in a fixed order
//   solver     gb_corr_kernel per bin, gb_order_kernel (rank counting), gb_perm_kernel (one persistent workgroup)
//
// Every sum has a fixed order (assx_perbin_common.hpp) and there is no float atomic: two runs give the same bits, and
// assx_gradbss_iterate enqueues the kernels of the single entry points, so it gives their bits.  Every value that both the
// loop and a single entry point produce comes out of the same kernel instantiation (the loss-only sweep is the moment
// kernel with its accumulation switched off by an argument; ln|det W| always comes from the tail of gb_finalize_kernel).
#include "assx_perbin_common.hpp"

using namespace assx;
using namespace assx::mf;
using namespace assx::pb;

namespace {

constexpr int GB_CHUNK = ASSX_GRADBSS_FRAME_CHUNK;   // frames of a moment workgroup
constexpr int GB_FS = 64;                            // bin slices of the IVA weight pass, at most
constexpr int MODE_LOGDET = 0, MODE_GRAD = 1, MODE_NAT = 2;
constexpr int GB_SOLVER_BINS = 1 << 16;              // the solver ranks the bins by counting, F^2 comparisons

static_assert(GB_CHUNK % BLK == 0, "a chunk is whole trips of the workgroup");

inline int gb_chunks(int T) { return chunks(T, GB_CHUNK); }
inline int gb_slices(int F) { return slices(F, GB_FS); }

struct GbLayout {
  size_t part, lpart, logdet, r, r2p, corr, crit, pbuf, total;
  size_t n_lpart_iva;
};

// part: moment partials (F,C,M,M) complex; lpart: data partials of the loss (FDICA: F*C, IVA: blocks of gb_weight_sum);
// logdet (F); r (M,T) and r2p (FS,M,T): the IVA weights and their slice partials; corr (F), crit (M,T), pbuf (M,T): solver
GbLayout gb_layout(int M, int F, int T) {
  const size_t d = sizeof(double);
  const size_t C = gb_chunks(T);
  Carve c(256);
  GbLayout L;
  L.n_lpart_iva = nblocks((size_t)M * T, BLK);
  const size_t nl = (size_t)F * C > L.n_lpart_iva ? (size_t)F * C : L.n_lpart_iva;
  L.part = c.take((size_t)F * C * M * M * 2 * d);
  L.lpart = c.take(nl * d);
  L.logdet = c.take((size_t)F * d);
  L.r = c.take((size_t)M * T * d);
  L.r2p = c.take((size_t)gb_slices(F) * M * T * d);
  L.corr = c.take((size_t)F * d);
  L.crit = c.take((size_t)M * T * d);
  L.pbuf = c.take((size_t)M * T * d);
  L.total = c.total();
  return L;
}

// ---------------------------------------------------------------------------------------------------------------
// IVA weights: r2p[s,n,t] = sum over the bins of slice s of |y[n,f,t]|^2, one lane per frame, bins in ascending order
// ---------------------------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__(WAVE) gb_weight_kernel(const Cd* __restrict__ X, const Cd* __restrict__ W,
                                                         double* __restrict__ r2p, int F, int T, int FS) {
  const int t = blockIdx.x * WAVE + threadIdx.x, s = blockIdx.y;
  if (t >= T) return;
  int f0, f1;
  slice_bounds(F, s, FS, f0, f1);
  double acc[M];
#pragma unroll
  for (int n = 0; n < M; ++n) acc[n] = 0.0;
  for (int f = f0; f < f1; ++f) {
    const Cd* Wf = W + (size_t)f * M * M;
    Cd x[M];
    load_frame<M>(X, f, t, F, T, x);
#pragma unroll
    for (int n = 0; n < M; ++n) {
      Cd y = cmake<double>(0.0, 0.0);
#pragma unroll
      for (int m = 0; m < M; ++m) cfma(y, Wf[n * M + m], x[m]);
      acc[n] += cabs2(y);
    }
  }
#pragma unroll
  for (int n = 0; n < M; ++n) r2p[((size_t)s * M + n) * T + t] = acc[n];
}

// r[n,t] = sqrt(sum_s r2p[s,n,t]), slices in index order; lpart[block] = the block's sum of r (the IVA loss's data term)
__global__ void __launch_bounds__(BLK) gb_weight_sum_kernel(const double* __restrict__ r2p, double* __restrict__ r,
                                                            double* __restrict__ lpart, size_t NT, int FS) {
  __shared__ double red[BLK / WAVE];
  const size_t i = (size_t)blockIdx.x * BLK + threadIdx.x;
  double v = 0.0;
  if (i < NT) {
    v = sqrt(slice_sum(r2p + i, NT, FS));
    r[i] = v;
  }
  const double tot = block_sum<double, BLK / WAVE>(v, red);
  if (threadIdx.x == 0) lpart[blockIdx.x] = tot;
}

// ---------------------------------------------------------------------------------------------------------------
// The moment pass: workgroup f C + c takes chunk c of bin f, lanes are frames.  part[f,c] = sum over the chunk's frames of phi z^H;
// FDICA: lpart[f,c] = sum of |y|.  do_moment = 0: only the data term (the loss-only sweep), same instructions up to it.
// ---------------------------------------------------------------------------------------------------------------
template <int M, int MODEL, bool NATURAL>
__global__ void __launch_bounds__(BLK) gb_moment_kernel(const Cd* __restrict__ X, const Cd* __restrict__ W,
                                                        const double* __restrict__ r, double eps, Cd* __restrict__ part,
                                                        double* __restrict__ lpart, int do_moment, int F, int T, int C) {
  using RS = RowSplit<M>;
  constexpr int RG = RS::RG, RPW = RS::RPW, NFG = RS::NFG;
  __shared__ Cd Ws[RS::ROWS * M];  // rows past M are zero: a wave's spare row accumulates nothing
  __shared__ double red[NW][RPW * M * 2];
  __shared__ double lred[NW];
  // a flat grid of F C workgroups: neither count fits a grid's y dimension at every size of the envelope
  const int f = blockIdx.x / C, c = blockIdx.x % C, tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const int rg = wave % RG, fg = wave / RG, r0 = rg * RPW;
  bin_matrix_to_lds<M>(Ws, W + (size_t)f * M * M);

  Cd acc[RPW][M];
#pragma unroll
  for (int i = 0; i < RPW; ++i)
#pragma unroll
    for (int m = 0; m < M; ++m) acc[i][m] = cmake<double>(0.0, 0.0);
  double lsum = 0.0;
  const int t_end = chunk_end(c, GB_CHUNK, T);
  for (int t = c * GB_CHUNK + fg * WAVE + lane; t < t_end; t += NFG * WAVE) {
    Cd x[M], z[M], yr[RPW];
    load_frame<M>(X, f, t, F, T, x);
    const Cd* Wl = Ws;
    if constexpr (RG > 1) Wl = Ws + lds_opaque();  // W stays in LDS: hoisted out of the loop it would take 256 VGPRs at M = 8
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      yr[i] = cmake<double>(0.0, 0.0);
#pragma unroll
      for (int m = 0; m < M; ++m) cfma(yr[i], Wl[(r0 + i) * M + m], x[m]);
    }
#pragma unroll
    for (int m = 0; m < M; ++m) {
      if constexpr (!NATURAL) {
        z[m] = x[m];
      } else if constexpr (RG == 1) {
        z[m] = yr[m];
      } else {  // every row of y, the wave's own rows as above
        z[m] = cmake<double>(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < M; ++k) cfma(z[m], Wl[m * M + k], x[k]);
      }
    }
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      double a;
      if constexpr (MODEL == ASSX_GRADBSS_IVA) {
        const int n = r0 + i < M ? r0 + i : M - 1;
        a = r[(size_t)n * T + t];
      } else {
        a = sqrt(cabs2(yr[i]));
        lsum += a;
      }
      const double den = floor_eps(a, eps);
      const double pr = yr[i].x / den, pi = yr[i].y / den;
      if (do_moment) {
#pragma unroll
        for (int m = 0; m < M; ++m) {  // phi conj(z)
          acc[i][m].x = fma(pr, z[m].x, acc[i][m].x);
          acc[i][m].x = fma(pi, z[m].y, acc[i][m].x);
          acc[i][m].y = fma(pi, z[m].x, acc[i][m].y);
          acc[i][m].y = fma(-pr, z[m].y, acc[i][m].y);
        }
      }
    }
  }

  if (do_moment) reduce_rows_store<M>(acc, red, part + ((size_t)f * C + c) * M * M);
  if constexpr (MODEL == ASSX_GRADBSS_FDICA) {
    const double tot = block_sum<double, NW>(lsum, lred);
    if (tid == 0 && lpart) lpart[(size_t)f * C + c] = tot;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Per bin, one wave, lane e = entry (n, m): G = (sum of the chunk partials in index order) / T, the step, W, ln|det W|.
// mode MODE_LOGDET leaves W alone.  The inverse and the determinant are lane 0's (assx_small_linalg.hpp).
// ---------------------------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__(WAVE) gb_finalize_kernel(Cd* __restrict__ W, const Cd* __restrict__ part,
                                                           double* __restrict__ logdet, int mode, double lr, int C, int T,
                                                           int32_t* __restrict__ status) {
  constexpr int MM = M * M;
  __shared__ Cd Ws[MM], Gs[MM], Vs[MM];
  const int f = blockIdx.x, e = threadIdx.x, n = e / M, m = e % M;
  const bool active = e < MM;
  if (active) {
    Ws[e] = W[(size_t)f * MM + e];
    if (mode != MODE_LOGDET) {
      const Cd g = chunk_sum<MM>(part, f, C, e);
      Gs[e] = cmake<double>(g.x / (double)T, g.y / (double)T);
    }
  }
  __syncthreads();
  Cd wn = cmake<double>(0.0, 0.0);
  if (mode == MODE_GRAD) {
    if (e == 0) {
      Cd A[M][M];
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) A[i][j] = Ws[i * M + j];
      const bool ok = gj_inverse<M>(A, nullptr);
      if (!ok && status) atomicOr(status, (int32_t)ASSX_STATUS_SINGULAR);
#pragma unroll
      for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) Vs[i * M + j] = A[i][j];
    }
    __syncthreads();
    if (active) {  // G - W^-H
      const Cd v = Vs[m * M + n], g = Gs[e], w = Ws[e];
      wn = cmake<double>(w.x - lr * (g.x - v.x), w.y - lr * (g.y + v.y));
    }
  } else if (mode == MODE_NAT) {
    if (active) {  // (G - I) W
      Cd d = cmake<double>(0.0, 0.0);
      for (int k = 0; k < M; ++k) {
        Cd g = Gs[n * M + k];
        if (k == n) g.x -= 1.0;
        cfma(d, g, Ws[k * M + m]);
      }
      const Cd w = Ws[e];
      wn = cmake<double>(w.x - lr * d.x, w.y - lr * d.y);
    }
  }
  __syncthreads();
  if (active && mode != MODE_LOGDET) {
    Ws[e] = wn;
    W[(size_t)f * MM + e] = wn;
  }
  __syncthreads();
  if (e == 0) {
    Cd A[M][M];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
      for (int j = 0; j < M; ++j) A[i][j] = Ws[i * M + j];
    const Cd det = lu_det<M>(A);
    logdet[f] = log(hypot(det.x, det.y));
  }
}

// loss[0] = (2 / T) (sum of the n data partials) - 2 (sum of the F log-determinants), each sum in a fixed order
__global__ void __launch_bounds__(BLK) gb_loss_close_kernel(const double* __restrict__ lpart, int n,
                                                            const double* __restrict__ logdet, int F, int T,
                                                            double* __restrict__ loss) {
  __shared__ double red[NW];
  double data, ld;
  loss_sums(lpart, n, logdet, F, red, data, ld);
  if (threadIdx.x == 0) loss[0] = 2.0 * data / (double)T - 2.0 * ld;
}

// ---------------------------------------------------------------------------------------------------------------
// FDICA's permutation solver (fdica.py:106-138).  P[n,t] = |y[n]| / max(sqrt(sum_n |y[n]|^2), eps) is re-formed from X and
// W wherever it is needed; it is never stored for more than the bin at hand.
// ---------------------------------------------------------------------------------------------------------------
template <int M>
__device__ __forceinline__ void gb_presence(const Cd* __restrict__ X, const Cd* Ws, int f, int t, int F, int T, double eps,
                                            double (&P)[M]) {
  Cd x[M];
  load_frame<M>(X, f, t, F, T, x);
  double tot = 0.0;
#pragma unroll
  for (int n = 0; n < M; ++n) {
    Cd y = cmake<double>(0.0, 0.0);
#pragma unroll
    for (int m = 0; m < M; ++m) cfma(y, Ws[n * M + m], x[m]);
    const double a2 = cabs2(y);
    tot += a2;
    P[n] = sqrt(a2);
  }
  const double nrm = floor_eps(sqrt(tot), eps);
#pragma unroll
  for (int n = 0; n < M; ++n) P[n] = P[n] / nrm;
}

// corr[f] = sum_t (sum_n P[n,t])^2
template <int M>
__global__ void __launch_bounds__(BLK) gb_corr_kernel(const Cd* __restrict__ X, const Cd* __restrict__ W, double eps,
                                                      double* __restrict__ corr, int F, int T) {
  __shared__ Cd Ws[M * M];
  __shared__ double red[NW];
  const int f = blockIdx.x, tid = threadIdx.x;
  if (tid < M * M) Ws[tid] = W[(size_t)f * M * M + tid];
  __syncthreads();
  double s = 0.0;
  for (int t = tid; t < T; t += BLK) {
    double P[M];
    gb_presence<M>(X, Ws, f, t, F, T, eps, P);
    double q = 0.0;
#pragma unroll
    for (int n = 0; n < M; ++n) q += P[n];
    s += q * q;
  }
  const double tot = block_sum<double, NW>(s, red);
  if (tid == 0) corr[f] = tot;
}

// a strict total order of the bins for ANY values: ascending correlation, equal values by index, NaN last by index
__device__ __forceinline__ bool gb_before(double ca, int a, double cb, int b) {
  const bool na = ca != ca, nb = cb != cb;
  if (na != nb) return nb;
  if (na) return a < b;
  return ca < cb || (ca == cb && a < b);
}

// order[rank of f] = f; the rank of a bin is the number of bins before it, so the ranks are a permutation of 0..F-1
__global__ void __launch_bounds__(BLK) gb_order_kernel(const double* __restrict__ corr, int32_t* __restrict__ order, int F) {
  const int f = blockIdx.x * BLK + threadIdx.x;
  if (f >= F) return;
  const double cf = corr[f];
  int rank = 0;
  for (int g = 0; g < F; ++g) rank += gb_before(corr[g], g, cf, f) ? 1 : 0;
  order[rank] = f;
}

// score of the permutation of lexicographic rank r (itertools.permutations order): sum_n C[n, pi(n)], n ascending;
// code holds pi(n) in nibble n.  Any r gives indices inside 0..N-1.
template <int N>
__device__ __forceinline__ double gb_perm_score(const double* Cs, int r, unsigned& code) {
  constexpr int FACT[9] = {1, 1, 2, 6, 24, 120, 720, 5040, 40320};
  unsigned mask = 0;
  double s = 0.0;
  code = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int fct = FACT[N - 1 - i];
    const int d = r / fct;
    r -= d * fct;
    int k = 0, cnt = 0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const bool free_ = !((mask >> j) & 1u);
      if (free_ && cnt == d) k = j;
      cnt += free_ ? 1 : 0;
    }
    mask |= 1u << k;
    s += Cs[i * N + k];
    code |= (unsigned)k << (4 * i);
  }
  return s;
}

// One persistent workgroup walks the bins in `order`.  crit (M,T) stays in the workspace (L2 at any realistic size); a
// thread owns the frames tid, tid + BLK, .. in every bin, so crit and pbuf need no ordering between threads.
template <int M>
__global__ void __launch_bounds__(BLK) gb_perm_kernel(const Cd* __restrict__ X, Cd* __restrict__ W, double eps,
                                                      const int32_t* __restrict__ order, int32_t* __restrict__ perm,
                                                      double* __restrict__ crit, double* __restrict__ pbuf, int F, int T) {
  constexpr int MM = M * M;
  constexpr int NPERM = M == 2 ? 2 : M == 3 ? 6 : M == 4 ? 24 : M == 5 ? 120 : M == 6 ? 720 : M == 7 ? 5040 : 40320;
  __shared__ Cd Ws[MM];
  __shared__ double red[NW][MM];
  __shared__ double Cs[MM];
  __shared__ double bs[BLK];
  __shared__ int br[BLK];
  __shared__ int pis[M];
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  for (int i = 0; i < F; ++i) {
    int f = order[i];
    f = f < 0 ? 0 : (f >= F ? F - 1 : f);
    __syncthreads();  // the previous bin is done with Ws, Cs and pis
    if (tid < MM) Ws[tid] = W[(size_t)f * MM + tid];
    __syncthreads();
    if (i == 0) {  // the criterion: not permuted
      for (int t = tid; t < T; t += BLK) {
        double P[M];
        gb_presence<M>(X, Ws, f, t, F, T, eps, P);
#pragma unroll
        for (int n = 0; n < M; ++n) crit[(size_t)n * T + t] = P[n];
      }
      if (tid < M) perm[(size_t)f * M + tid] = tid;
      continue;
    }
    double Ca[M][M];  // C[n][k] = sum_t crit[n,t] P[k,t]
#pragma unroll
    for (int n = 0; n < M; ++n)
#pragma unroll
      for (int k = 0; k < M; ++k) Ca[n][k] = 0.0;
    for (int t = tid; t < T; t += BLK) {
      double P[M];
      gb_presence<M>(X, Ws, f, t, F, T, eps, P);
#pragma unroll
      for (int k = 0; k < M; ++k) pbuf[(size_t)k * T + t] = P[k];
#pragma unroll
      for (int n = 0; n < M; ++n) {
        const double cr = crit[(size_t)n * T + t];
#pragma unroll
        for (int k = 0; k < M; ++k) Ca[n][k] = fma(cr, P[k], Ca[n][k]);
      }
    }
#pragma unroll
    for (int n = 0; n < M; ++n)
#pragma unroll
      for (int k = 0; k < M; ++k) {
        const double v = wave_sum_down(Ca[n][k]);
        if (lane == 0) red[wave][n * M + k] = v;
      }
    __syncthreads();
    if (tid < MM) Cs[tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
    __syncthreads();
    // the N! candidates across the lanes; the identity stands unless a later candidate is strictly greater
    unsigned code;
    double best = gb_perm_score<M>(Cs, 0, code);
    int best_r = 0;
    if (best == best) {
      for (int r = tid; r < NPERM; r += BLK) {
        const double s = gb_perm_score<M>(Cs, r, code);
        if (s > best) best = s, best_r = r;
      }
    }
    bs[tid] = best, br[tid] = best_r;
    __syncthreads();
    if (tid == 0) {  // the maximum, the lowest rank among equals
      for (int j = 1; j < BLK; ++j)
        if (bs[j] > best || (bs[j] == best && br[j] < best_r)) best = bs[j], best_r = br[j];
      gb_perm_score<M>(Cs, best_r, code);
#pragma unroll
      for (int n = 0; n < M; ++n) pis[n] = (int)((code >> (4 * n)) & 0xfu) % M;
    }
    __syncthreads();
    for (int t = tid; t < T; t += BLK) {
#pragma unroll
      for (int n = 0; n < M; ++n) crit[(size_t)n * T + t] += pbuf[(size_t)pis[n] * T + t];
    }
    if (tid < MM) W[(size_t)f * MM + tid] = Ws[pis[tid / M] * M + tid % M];
    if (tid < M) perm[(size_t)f * M + tid] = pis[tid];
  }
}

static_assert(NW == 4, "the solver adds four waves");

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
int gb_check(assx_ctx* ctx, int M, int F, int T) { return check_bin_sizes(ctx, "gradient IVA / FDICA", M, F, T); }

int gb_check_model(assx_ctx* ctx, int model, int natural) {
  ASSX_REQUIRE(ctx, model == ASSX_GRADBSS_IVA || model == ASSX_GRADBSS_FDICA, ASSX_E_ARG, "model must be 0 (IVA) or 1 (FDICA), got %d",
               model);
  ASSX_REQUIRE(ctx, natural == 0 || natural == 1, ASSX_E_ARG, "natural must be 0 or 1, got %d", natural);
  return 0;
}

struct GbRun : RunBase {
  assx_ctx* ctx;
  const Cd* X;
  Cd* W;
  int M, F, T;
  GbLayout L;
};

// IVA: r of the current W and the data partials of its loss
int gb_stage_weights(const GbRun& g) {
  const int FS = gb_slices(g.F);
  return dispatch_channels(g.ctx, "gradient IVA", g.M, [&](auto mt) -> int {
    constexpr int MC = decltype(mt)::value;
    hipLaunchKernelGGL((gb_weight_kernel<MC>), dim3(nblocks(g.T, WAVE), FS), dim3(WAVE), 0, g.st, g.X, (const Cd*)g.W,
                       g.at<double>(g.L.r2p), g.F, g.T, FS);
    ASSX_LAUNCH_CHECK(g.ctx, "gb_weight_kernel");
    hipLaunchKernelGGL(gb_weight_sum_kernel, dim3((unsigned)g.L.n_lpart_iva), dim3(BLK), 0, g.st,
                       (const double*)g.at<double>(g.L.r2p), g.at<double>(g.L.r), g.at<double>(g.L.lpart),
                       (size_t)g.M * g.T, FS);
    ASSX_LAUNCH_CHECK(g.ctx, "gb_weight_sum_kernel");
    return 0;
  });
}

template <int MODEL, bool NATURAL>
int gb_moment_launch(const GbRun& g, double eps, int do_moment) {
  return launch_for_channels(g.ctx, "gradient IVA / FDICA", "gb_moment_kernel", g.M, [&](auto mt) {
    hipLaunchKernelGGL((gb_moment_kernel<decltype(mt)::value, MODEL, NATURAL>), dim3((unsigned)g.F * gb_chunks(g.T)),
                       dim3(BLK), 0, g.st, g.X, (const Cd*)g.W, (const double*)g.at<double>(g.L.r), eps, g.at<Cd>(g.L.part),
                       MODEL == ASSX_GRADBSS_FDICA ? g.at<double>(g.L.lpart) : (double*)nullptr, do_moment, g.F, g.T,
                       gb_chunks(g.T));
  });
}

// the sweep that forms the moment (and, for FDICA, the data partials of the loss of the current W)
int gb_stage_moment(const GbRun& g, int model, int natural, double eps, int do_moment) {
  if (model == ASSX_GRADBSS_IVA)
    return natural ? gb_moment_launch<ASSX_GRADBSS_IVA, true>(g, eps, do_moment)
                   : gb_moment_launch<ASSX_GRADBSS_IVA, false>(g, eps, do_moment);
  return natural ? gb_moment_launch<ASSX_GRADBSS_FDICA, true>(g, eps, do_moment)
                 : gb_moment_launch<ASSX_GRADBSS_FDICA, false>(g, eps, do_moment);
}

int gb_stage_finalize(const GbRun& g, int mode, double lr, int32_t* status) {
  return launch_for_channels(g.ctx, "gradient IVA / FDICA", "gb_finalize_kernel", g.M, [&](auto mt) {
    hipLaunchKernelGGL((gb_finalize_kernel<decltype(mt)::value>), dim3(g.F), dim3(WAVE), 0, g.st, g.W,
                       (const Cd*)g.at<Cd>(g.L.part), g.at<double>(g.L.logdet), mode, lr, gb_chunks(g.T), g.T, status);
  });
}

int gb_stage_close(const GbRun& g, int model, double* loss) {
  const int n = model == ASSX_GRADBSS_IVA ? (int)g.L.n_lpart_iva : g.F * gb_chunks(g.T);
  hipLaunchKernelGGL(gb_loss_close_kernel, dim3(1), dim3(BLK), 0, g.st, (const double*)g.at<double>(g.L.lpart), n,
                     (const double*)g.at<double>(g.L.logdet), g.F, g.T, loss);
  ASSX_LAUNCH_CHECK(g.ctx, "gb_loss_close_kernel");
  return 0;
}

// the first sweep of an iteration: it leaves the data partials of the loss of the W it reads.  FDICA has one sweep, so
// its moment (do_moment) is formed here; IVA's moment sweep follows
int gb_first_sweep(const GbRun& g, int model, int natural, double eps, int do_moment) {
  if (model == ASSX_GRADBSS_IVA) return gb_stage_weights(g);
  return gb_stage_moment(g, model, natural, eps, do_moment);
}

GbRun gb_run(assx_ctx* ctx, const void* X, void* W, void* ws, int M, int F, int T, void* stream) {
  return GbRun{{(char*)ws, (hipStream_t)stream}, ctx, (const Cd*)X, (Cd*)W, M, F, T, gb_layout(M, F, T)};
}

}  // namespace

extern "C" {

size_t assx_gradbss_workspace_bytes(int M, int F, int T) {
  if (!in_envelope(M, F, T)) return 0;
  return gb_layout(M, F, T).total;
}

int assx_gradbss_update(assx_ctx* ctx, int model, int natural, const void* X, void* W, void* ws, double lr, double eps,
                        int M, int F, int T, int32_t* status, void* stream) {
  int rc = gb_check(ctx, M, F, T);
  if (!rc) rc = gb_check_model(ctx, model, natural);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && ws, ASSX_E_NULL, "assx_gradbss_update: NULL array");
  const GbRun g = gb_run(ctx, X, W, ws, M, F, T, stream);
  rc = gb_first_sweep(g, model, natural, eps, 1);
  if (!rc && model == ASSX_GRADBSS_IVA) rc = gb_stage_moment(g, model, natural, eps, 1);
  if (!rc) rc = gb_stage_finalize(g, natural ? MODE_NAT : MODE_GRAD, lr, status);
  return rc;
}

int assx_gradbss_loss(assx_ctx* ctx, int model, const void* X, const void* W, void* ws, double* loss, int M, int F, int T,
                      void* stream) {
  int rc = gb_check(ctx, M, F, T);
  if (!rc) rc = gb_check_model(ctx, model, 0);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && ws && loss, ASSX_E_NULL, "assx_gradbss_loss: NULL array");
  const GbRun g = gb_run(ctx, X, const_cast<void*>(W), ws, M, F, T, stream);
  rc = gb_first_sweep(g, model, 0, 0.0, 0);
  if (!rc) rc = gb_stage_finalize(g, MODE_LOGDET, 0.0, nullptr);
  if (!rc) rc = gb_stage_close(g, model, loss);
  return rc;
}

int assx_gradbss_iterate(assx_ctx* ctx, int n_iter, int model, int natural, const void* X, void* W, void* ws, double lr,
                         double eps, double* loss, int M, int F, int T, int32_t* status, void* stream) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, n_iter >= 0, ASSX_E_ARG, "n_iter must be >= 0, got %d", n_iter);
  int rc = gb_check(ctx, M, F, T);
  if (!rc) rc = gb_check_model(ctx, model, natural);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && ws, ASSX_E_NULL, "assx_gradbss_iterate: NULL array");
  const GbRun g = gb_run(ctx, X, W, ws, M, F, T, stream);
  // loss[i] belongs to the W that iteration i starts from: its data partials ride on that iteration's first sweep, its
  // log-determinants were left by the finalize before it.  One trailing sweep closes loss[n_iter].
  if (loss) rc = gb_stage_finalize(g, MODE_LOGDET, 0.0, nullptr);
  for (int i = 0; i < n_iter && !rc; ++i) {
    rc = gb_first_sweep(g, model, natural, eps, 1);
    if (!rc && loss) rc = gb_stage_close(g, model, loss + i);
    if (!rc && model == ASSX_GRADBSS_IVA) rc = gb_stage_moment(g, model, natural, eps, 1);
    if (!rc) rc = gb_stage_finalize(g, natural ? MODE_NAT : MODE_GRAD, lr, status);
  }
  if (!rc && loss) {
    rc = gb_first_sweep(g, model, 0, 0.0, 0);
    if (!rc) rc = gb_stage_close(g, model, loss + n_iter);
  }
  return rc;
}

int assx_fdica_solve_permutation(assx_ctx* ctx, const void* X, void* W, void* ws, int32_t* order, int32_t* perm, double eps,
                                 int M, int F, int T, void* stream) {
  int rc = gb_check(ctx, M, F, T);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, F <= GB_SOLVER_BINS, ASSX_E_UNSUPPORTED, "FDICA: the permutation solver takes at most %d bins, got %d",
               GB_SOLVER_BINS, F);
  ASSX_REQUIRE(ctx, X && W && ws && order && perm, ASSX_E_NULL, "assx_fdica_solve_permutation: NULL array");
  const GbRun g = gb_run(ctx, X, W, ws, M, F, T, stream);
  return dispatch_channels(ctx, "FDICA", M, [&](auto mt) -> int {
    constexpr int MC = decltype(mt)::value;
    hipLaunchKernelGGL((gb_corr_kernel<MC>), dim3(F), dim3(BLK), 0, g.st, g.X, (const Cd*)g.W, eps,
                       g.at<double>(g.L.corr), F, T);
    ASSX_LAUNCH_CHECK(ctx, "gb_corr_kernel");
    hipLaunchKernelGGL(gb_order_kernel, dim3(nblocks(F, BLK)), dim3(BLK), 0, g.st, (const double*)g.at<double>(g.L.corr),
                       order, F);
    ASSX_LAUNCH_CHECK(ctx, "gb_order_kernel");
    hipLaunchKernelGGL((gb_perm_kernel<MC>), dim3(1), dim3(BLK), 0, g.st, g.X, g.W, eps, (const int32_t*)order, perm,
                       g.at<double>(g.L.crit), g.at<double>(g.L.pbuf), F, T);
    ASSX_LAUNCH_CHECK(ctx, "gb_perm_kernel");
    return 0;
  });
}

}  // extern "C"
