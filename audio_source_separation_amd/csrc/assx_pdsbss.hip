// ProxLaplaceIVA (src/bss/iva.py:831-904) on PDSBSSbase (src/bss/prox.py:13-201) on MI355X: IVA by primal-dual splitting,
// the whole loop on the device.  float64, one utterance, N = M sources, 2 <= M <= 8.
//
// State: X (M,F,T) complex128 with T fastest, W (F,N,M), the dual y (F,N,T), norm (1,) in device memory.  The reference's
// block-diagonal sparse operator is dense per-bin algebra here; with rn = 1 / norm (one reciprocal per kernel, multiplied
// in AFTER the sum over channels or frames -- X itself is never scaled):
//   adjoint    G[f,n,m] = rn sum_t conj(X[m,f,t]) y[f,n,t]
//   prox       Wt = U h(S) V^H of the SVD of W - mu1 mu2 G,  h(s) = (s + sqrt(s^2 + 4 mu1)) / 2;  D = 2 Wt - W
//   forward    z[f,n,t] = y[f,n,t] + rn sum_m X[m,f,t] D[f,n,m]
//   shrink     den[n,t] = sqrt(sum_f |z|^2) (1 / mu2 where it is <= 0),  s = 1 - C max(0, 1 - (1 / mu2) / den)
//   step       y <- alpha s z + (1 - alpha) y,  W <- alpha Wt + (1 - alpha) W
//   loss       C sum_{n,t} sqrt(sum_f |(W x)[n,f,t]|^2) - sum_f ln|det W_f|
//
// Launches:
//   finalize   pd_finalize_kernel, one wave per bin: the chunk partials of G in index order, the prox argument, a one-sided
//              (Hestenes) Jacobi SVD in LDS with a cap on the sweeps, Wt, D, the new W and ln|det W|.  Its modes also serve
//              the single entry points (prox only, G only, ln|det W| only, the Gram matrix of the operator norm)
//   sweep 1    pd_group_kernel (frame tile x bin slice): z in registers, sum_f |z|^2 of a slice of bins per (n,t), bins
//              ascending, and beside it sum_f |W x|^2 for the loss; pd_shrink_kernel: the slices in index order, s, and
//              the block partials of the loss's data term
//   sweep 2    pd_dual_kernel (bin x frame chunk, a flat grid): z again, y written, and the partials of the NEXT
//              iteration's G from the y just formed (rows split over two wave pairs at M >= 7).  With its update switched
//              off by an argument it is the adjoint of a y as it stands, and on X in place of y the Gram matrix
//   close      pd_loss_close_kernel
//
// Every sum has a fixed order and there is no float atomic: two runs give the same bits.  Every value that both the loop
// and a single entry point produce comes out of the same kernel instantiation through explicit fused multiply-adds, so
// assx_pdsbss_iterate gives the bits of update + loss called in turn although it skips the adjoint sweep that
// assx_pdsbss_update has to begin with (the partials of the previous sweep 2 are those very numbers).
#include "assx_perbin_common.hpp"

using namespace assx;
using namespace assx::mf;
using namespace assx::pb;

namespace {

constexpr int PD_CHUNK = ASSX_PDSBSS_FRAME_CHUNK;  // frames of a sweep-2 workgroup
constexpr int PD_FS = 64;                          // bin slices of sweep 1, at most
constexpr int PD_SWEEPS = 40;                      // Jacobi sweeps, at most (a full-rank 8 x 8 takes 6 to 9)
constexpr double PD_RANK_TOL = 1e-13;              // a singular value below this x the largest: its left vector is completed
constexpr double PD_SKIP_TOL = 1e-14;              // a column below this x the Frobenius norm is not rotated any more
enum { FIN_LOGDET = 0, FIN_UPDATE = 1, FIN_PROX = 2, FIN_ADJOINT = 3, FIN_GRAM = 4 };
enum { SHRINK_NONE = 0, SHRINK_STEP = 1, SHRINK_PROX = 2 };

static_assert(PD_CHUNK % BLK == 0, "a chunk is whole trips of the workgroup");

inline int pd_chunks(int T) { return chunks(T, PD_CHUNK); }
inline int pd_slices(int F) { return slices(F, PD_FS); }

// part: partials of G (F,C,M,M) complex; D (F,M,M) complex; logdet (F), also the largest eigenvalue of a bin's Gram matrix;
// r2z, r2w (FS,M,T): slice partials of sum_f |z|^2 and sum_f |W x|^2; s (M,T): the shrink factor; lpart: block partials
// of the loss's data term
struct PdLayout {
  size_t part, D, logdet, r2z, r2w, s, lpart, total;
  size_t n_lpart;
};

PdLayout pd_layout(int M, int F, int T) {
  const size_t d = sizeof(double);
  const size_t C = pd_chunks(T);
  Carve c(256);
  PdLayout L;
  L.n_lpart = nblocks((size_t)M * T, BLK);
  L.part = c.take((size_t)F * C * M * M * 2 * d);
  L.D = c.take((size_t)F * M * M * 2 * d);
  L.logdet = c.take((size_t)F * d);
  L.r2z = c.take((size_t)pd_slices(F) * M * T * d);
  L.r2w = c.take((size_t)pd_slices(F) * M * T * d);
  L.s = c.take((size_t)M * T * d);
  L.lpart = c.take(L.n_lpart * d);
  L.total = c.total();
  return L;
}

// ---------------------------------------------------------------------------------------------------------------
// Sweep 1: r2z[sl,n,t] = sum over the bins of slice sl of |z[f,n,t]|^2 (do_z) and r2w the same of |(W x)[n]|^2 (do_w),
// one lane per frame, bins ascending.  D and W are read through wave-uniform addresses.
// ---------------------------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__(WAVE) pd_group_kernel(const Cd* __restrict__ X, const Cd* __restrict__ y,
                                                        const Cd* __restrict__ D, const Cd* __restrict__ W,
                                                        const double* __restrict__ norm, double* __restrict__ r2z,
                                                        double* __restrict__ r2w, int do_z, int do_w, int F, int T, int FS) {
  const int t = blockIdx.x * WAVE + threadIdx.x, sl = blockIdx.y;
  if (t >= T) return;
  int f0, f1;
  slice_bounds(F, sl, FS, f0, f1);
  const double rn = do_z ? 1.0 / norm[0] : 0.0;
  double az[M], aw[M];
#pragma unroll
  for (int n = 0; n < M; ++n) az[n] = 0.0, aw[n] = 0.0;
  for (int f = f0; f < f1; ++f) {
    Cd x[M];
    load_frame<M>(X, f, t, F, T, x);
    if (do_z) {
      const Cd* Df = D + (size_t)f * M * M;
#pragma unroll
      for (int n = 0; n < M; ++n) {
        const Cd yv = y[((size_t)f * M + n) * T + t];
        Cd dx = cmake<double>(0.0, 0.0);
#pragma unroll
        for (int m = 0; m < M; ++m) cfma(dx, Df[n * M + m], x[m]);
        const double zr = fma(dx.x, rn, yv.x), zi = fma(dx.y, rn, yv.y);
        az[n] = fma(zr, zr, az[n]);
        az[n] = fma(zi, zi, az[n]);
      }
    }
    if (do_w) {
      const Cd* Wf = W + (size_t)f * M * M;
#pragma unroll
      for (int n = 0; n < M; ++n) {
        Cd wx = cmake<double>(0.0, 0.0);
#pragma unroll
        for (int m = 0; m < M; ++m) cfma(wx, Wf[n * M + m], x[m]);
        aw[n] = fma(wx.x, wx.x, aw[n]);
        aw[n] = fma(wx.y, wx.y, aw[n]);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < M; ++n) {
    if (do_z) r2z[((size_t)sl * M + n) * T + t] = az[n];
    if (do_w) r2w[((size_t)sl * M + n) * T + t] = aw[n];
  }
}

// the same slice partials of a z (F, NT) that is given as an array (assx_pdsbss_prox_group)
__global__ void __launch_bounds__(BLK) pd_norm2_kernel(const Cd* __restrict__ z, double* __restrict__ r2z, int F, size_t NT,
                                                       int FS) {
  const size_t i = (size_t)blockIdx.x * BLK + threadIdx.x;
  const int sl = blockIdx.y;
  if (i >= NT) return;
  int f0, f1;
  slice_bounds(F, sl, FS, f0, f1);
  double a = 0.0;
  for (int f = f0; f < f1; ++f) {
    const Cd v = z[(size_t)f * NT + i];
    a = fma(v.x, v.x, a);
    a = fma(v.y, v.y, a);
  }
  r2z[(size_t)sl * NT + i] = a;
}

// The slices in index order.  do_z: den = sqrt(sum), 1 / mu where it is <= 0, p = C max(0, 1 - (1 / mu) / den) (imu = 1 / mu
// is the prox's own parameter, iva.py:883-885); s_out = 1 - p (SHRINK_STEP) or p (SHRINK_PROX).  do_w: lpart[block] = the
// block's sum of sqrt(sum of r2w), the data term of the loss.
__global__ void __launch_bounds__(BLK) pd_shrink_kernel(const double* __restrict__ r2z, const double* __restrict__ r2w,
                                                        double* __restrict__ s_out, double* __restrict__ lpart, size_t NT,
                                                        int FS, double Creg, double imu, int do_z, int do_w) {
  __shared__ double red[BLK / WAVE];
  const size_t i = (size_t)blockIdx.x * BLK + threadIdx.x;
  double v = 0.0;
  if (i < NT) {
    if (do_z != SHRINK_NONE) {
      double den = sqrt(slice_sum(r2z + i, NT, FS));
      if (den <= 0.0) den = imu;
      const double q = 1.0 - imu / den;
      const double p = Creg * (q > 0.0 ? q : 0.0);
      s_out[i] = do_z == SHRINK_STEP ? 1.0 - p : p;
    }
    if (do_w) v = sqrt(slice_sum(r2w + i, NT, FS));
  }
  if (do_w) {
    const double tot = block_sum<double, BLK / WAVE>(v, red);
    if (threadIdx.x == 0) lpart[blockIdx.x] = tot;
  }
}

// out[f,i] = p[i] z[f,i]
__global__ void __launch_bounds__(BLK) pd_apply_kernel(const Cd* __restrict__ z, const double* __restrict__ p,
                                                       Cd* __restrict__ out, size_t NT, size_t total) {
  const size_t i = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (i >= total) return;
  const double a = p[i % NT];
  const Cd v = z[i];
  out[i] = cmake<double>(a * v.x, a * v.y);
}

// z[f,n,t] = y[f,n,t] + rn sum_m X[m,f,t] D[f,n,m], written out (assx_pdsbss_forward); a flat grid of F x frame tiles
template <int M>
__global__ void __launch_bounds__(WAVE) pd_forward_kernel(const Cd* __restrict__ X, const Cd* __restrict__ y,
                                                          const Cd* __restrict__ D, const double* __restrict__ norm,
                                                          Cd* __restrict__ z, int F, int T, int NTILE) {
  const int f = blockIdx.x / NTILE, t = (blockIdx.x % NTILE) * WAVE + threadIdx.x;
  if (t >= T) return;
  const double rn = 1.0 / norm[0];
  const Cd* Df = D + (size_t)f * M * M;
  Cd x[M];
  load_frame<M>(X, f, t, F, T, x);
#pragma unroll
  for (int n = 0; n < M; ++n) {
    const Cd yv = y[((size_t)f * M + n) * T + t];
    Cd dx = cmake<double>(0.0, 0.0);
#pragma unroll
    for (int m = 0; m < M; ++m) cfma(dx, Df[n * M + m], x[m]);
    z[((size_t)f * M + n) * T + t] = cmake<double>(fma(dx.x, rn, yv.x), fma(dx.y, rn, yv.y));
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Sweep 2: workgroup f C + c takes chunk c of bin f, lanes are frames.  do_update: z = y + rn D x, y <- alpha s z +
// (1 - alpha) y is written.  Always: part[f,c,n,m] = sum over the chunk's frames of conj(X[m]) y[n] with the y the lane
// now holds.  y is addressed as y[f ysF + n ysN + t]: (F,N,T) for the dual, and X itself (ysF = T, ysN = F T, never
// written) for the Gram matrix of the operator norm.
// ---------------------------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__(BLK) pd_dual_kernel(const Cd* __restrict__ X, Cd* y, size_t ysF, size_t ysN,
                                                      const Cd* __restrict__ D, const double* __restrict__ s,
                                                      const double* __restrict__ norm, double alpha, Cd* __restrict__ part,
                                                      int do_update, int F, int T, int C) {
  using RS = RowSplit<M>;
  constexpr int RG = RS::RG, RPW = RS::RPW, NFG = RS::NFG;
  __shared__ Cd Ds[RS::ROWS * M];  // rows past M are zero and never used
  __shared__ double red[NW][RPW * M * 2];
  // a flat grid of F C workgroups: neither count fits a grid's y dimension at every size of the envelope
  const int f = blockIdx.x / C, c = blockIdx.x % C, tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const int rg = wave % RG, fg = wave / RG, r0 = rg * RPW;
  bin_matrix_to_lds<M>(Ds, D + (size_t)f * M * M, !do_update);
  const double rn = do_update ? 1.0 / norm[0] : 0.0;
  const double beta = 1.0 - alpha;

  Cd acc[RPW][M];
#pragma unroll
  for (int i = 0; i < RPW; ++i)
#pragma unroll
    for (int m = 0; m < M; ++m) acc[i][m] = cmake<double>(0.0, 0.0);
  const int t_end = chunk_end(c, PD_CHUNK, T);
  for (int t = c * PD_CHUNK + fg * WAVE + lane; t < t_end; t += NFG * WAVE) {
    Cd x[M];
    load_frame<M>(X, f, t, F, T, x);
    const Cd* Dl = Ds;
    if constexpr (RG > 1) Dl = Ds + lds_opaque();  // D stays in LDS: hoisted out of the loop it would take 128 VGPRs more
#pragma unroll
    for (int i = 0; i < RPW; ++i) {
      const int n = r0 + i;
      if (n < M) {
        Cd* yp = y + (size_t)f * ysF + (size_t)n * ysN + t;
        Cd yv = *yp;
        if (do_update) {
          Cd dx = cmake<double>(0.0, 0.0);
#pragma unroll
          for (int m = 0; m < M; ++m) cfma(dx, Dl[n * M + m], x[m]);
          const double zr = fma(dx.x, rn, yv.x), zi = fma(dx.y, rn, yv.y);
          const double a = alpha * s[(size_t)n * T + t];
          yv = cmake<double>(fma(a, zr, beta * yv.x), fma(a, zi, beta * yv.y));
          *yp = yv;
        }
#pragma unroll
        for (int m = 0; m < M; ++m) {  // conj(x) y
          acc[i][m].x = fma(x[m].x, yv.x, acc[i][m].x);
          acc[i][m].x = fma(x[m].y, yv.y, acc[i][m].x);
          acc[i][m].y = fma(x[m].x, yv.y, acc[i][m].y);
          acc[i][m].y = fma(-x[m].y, yv.x, acc[i][m].y);
        }
      }
    }
  }

  reduce_rows_store<M>(acc, red, part + ((size_t)f * C + c) * M * M);
}

// ---------------------------------------------------------------------------------------------------------------
// Per bin, one wave, lane e = entry (n, m).  The one-sided Jacobi works on A (M x M, row-major in LDS) and V = I: each
// pair of columns (p, q), p < q in cyclic order, is made orthogonal by a complex plane rotation applied to A and to V.
// Every lane forms the pair's three inner products itself, in the same order, so the decision is the wave's; lane r < M
// then rotates row r of A and lane M + r row r of V.  At the end the columns of A are U S.
//   FIN_UPDATE   A = W - mu12 G, G = rn (chunk partials in index order);  Wt;  D = 2 Wt - W;  W <- alpha Wt + (1 - alpha) W;
//                ln|det W|
//   FIN_PROX     A = in;  out = Wt
//   FIN_ADJOINT  out = G, nothing else
//   FIN_GRAM     A = the sum of the partials (a Hermitian Gram matrix);  logdet[f] = its largest singular value
//   FIN_LOGDET   ln|det W| of W as it stands
// A sweep cap that is reached, or a non-finite singular value, sets ASSX_STATUS_NOT_CONVERGED; the kernel always ends.
// ---------------------------------------------------------------------------------------------------------------
template <int M>
__global__ void __launch_bounds__(WAVE) pd_finalize_kernel(Cd* __restrict__ W, const Cd* __restrict__ in, Cd* __restrict__ out,
                                                           const Cd* __restrict__ part, Cd* __restrict__ D,
                                                           double* __restrict__ logdet, const double* __restrict__ norm,
                                                           int mode, double mu, double mu12, double alpha, int C,
                                                           int32_t* __restrict__ status) {
  constexpr int MM = M * M;
  __shared__ Cd As[MM], Vs[MM], Ws[MM];
  __shared__ double sg[M], hs[M];
  const int f = blockIdx.x, e = threadIdx.x, n = e / M, m = e % M;
  const bool active = e < MM;

  if (mode != FIN_LOGDET) {
    if (active) {
      Cd g = cmake<double>(0.0, 0.0);
      if (mode == FIN_UPDATE || mode == FIN_ADJOINT || mode == FIN_GRAM) {
        g = chunk_sum<MM>(part, f, C, e);
        if (mode != FIN_GRAM) {
          const double rn = 1.0 / norm[0];
          g = cmake<double>(g.x * rn, g.y * rn);
        }
      }
      if (mode == FIN_ADJOINT) out[(size_t)f * MM + e] = g;
      if (mode == FIN_UPDATE) {
        const Cd w = W[(size_t)f * MM + e];
        Ws[e] = w;
        As[e] = cmake<double>(fma(-mu12, g.x, w.x), fma(-mu12, g.y, w.y));
      } else if (mode == FIN_GRAM) {
        As[e] = g;
      } else if (mode == FIN_PROX) {
        As[e] = in[(size_t)f * MM + e];
      }
      Vs[e] = cmake<double>(n == m ? 1.0 : 0.0, 0.0);
    }
    if (mode == FIN_ADJOINT) return;
    __syncthreads();

    const double tol = 2.0 * M * 2.220446049250313e-16, tol2 = tol * tol;
    // A column below PD_SKIP_TOL x the Frobenius norm (which the rotations keep) is left alone: it lies below PD_RANK_TOL x
    // the largest singular value (>= the Frobenius norm / sqrt(M)), so its left vector is completed anyway, and rotating
    // it against rounding noise would shrink it sweep after sweep until the phase of a denormal inner product is no phase
    double fro2 = 0.0;
    for (int i = 0; i < MM; ++i) {
      const Cd a = As[i];
      fro2 = fma(a.x, a.x, fro2), fro2 = fma(a.y, a.y, fro2);
    }
    const double skip2 = PD_SKIP_TOL * PD_SKIP_TOL * fro2;
    bool rotated = true;
    for (int sweep = 0; sweep < PD_SWEEPS && rotated; ++sweep) {
      rotated = false;
      for (int p = 0; p < M - 1; ++p)
        for (int q = p + 1; q < M; ++q) {
          double al = 0.0, be = 0.0, gr = 0.0, gi = 0.0;
#pragma unroll
          for (int i = 0; i < M; ++i) {
            const Cd a = As[i * M + p], b = As[i * M + q];
            al = fma(a.x, a.x, al), al = fma(a.y, a.y, al);
            be = fma(b.x, b.x, be), be = fma(b.y, b.y, be);
            gr = fma(a.x, b.x, gr), gr = fma(a.y, b.y, gr);  // conj(a) b
            gi = fma(a.x, b.y, gi), gi = fma(-a.y, b.x, gi);
          }
          const double g2 = fma(gr, gr, gi * gi);
          const bool rot = g2 > tol2 * al * be && al > skip2 && be > skip2;  // false for a NaN: the bin is flagged below
          Cd ap = cmake<double>(0.0, 0.0), aq = ap;
          Cd* rowp = nullptr;
          if (rot && e < 2 * M) {
            rowp = e < M ? As + e * M : Vs + (e - M) * M;
            ap = rowp[p], aq = rowp[q];
          }
          __syncthreads();  // every lane has read the pair's columns
          if (rot) {
            rotated = true;
            if (rowp) {
              const double g = sqrt(g2), er = gr / g, ei = gi / g;
              const double zeta = (be - al) / (2.0 * g);
              const double tt = copysign(1.0, zeta) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
              const double cs = 1.0 / sqrt(fma(tt, tt, 1.0)), sn = cs * tt;
              const Cd bq = cmake<double>(aq.x * er + aq.y * ei, aq.y * er - aq.x * ei);  // aq conj(phase)
              rowp[p] = cmake<double>(cs * ap.x - sn * bq.x, cs * ap.y - sn * bq.y);
              rowp[q] = cmake<double>(sn * ap.x + cs * bq.x, sn * ap.y + cs * bq.y);
            }
          }
          __syncthreads();
        }
    }
    if (rotated && e == 0 && status) atomicOr(status, (int32_t)ASSX_STATUS_NOT_CONVERGED);

    if (e < M) {
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < M; ++i) {
        const Cd v = As[i * M + e];
        a = fma(v.x, v.x, a), a = fma(v.y, v.y, a);
      }
      sg[e] = sqrt(a);
    }
    __syncthreads();
    double smax = 0.0;
    bool bad = false;
#pragma unroll
    for (int j = 0; j < M; ++j) {
      const double v = sg[j];
      if (!(v <= 1.7976931348623157e308)) bad = true;
      smax = v > smax ? v : smax;
    }
    if (bad && e == 0 && status) atomicOr(status, (int32_t)ASSX_STATUS_NOT_CONVERGED);
    if (mode == FIN_GRAM) {
      if (e == 0) logdet[f] = bad ? __builtin_nan("") : smax;
      return;
    }

    // U: the columns of A over their norms; a column below PD_RANK_TOL x the largest is replaced by a unit vector
    // orthogonal to the others (any such choice is a valid prox of a rank-deficient argument)
    const double thr = smax * PD_RANK_TOL;
    if (e < M) {
      const double sv = sg[e];
      hs[e] = 0.5 * (sv + sqrt(fma(sv, sv, 4.0 * mu)));
      if (sv > thr) {
        const double r = 1.0 / sv;
#pragma unroll
        for (int i = 0; i < M; ++i) {
          const Cd v = As[i * M + e];
          As[i * M + e] = cmake<double>(v.x * r, v.y * r);
        }
      }
    }
    __syncthreads();
    if (e == 0 && !bad) {
      unsigned done = 0;
      for (int j = 0; j < M; ++j)
        if (sg[j] > thr) done |= 1u << j;
      for (int j = 0; j < M; ++j) {
        if (done & (1u << j)) continue;
        for (int k = 0; k < M; ++k) {  // e_k less its components along the columns in place, twice
          Cd v[M];
          for (int i = 0; i < M; ++i) v[i] = cmake<double>(i == k ? 1.0 : 0.0, 0.0);
          for (int pass = 0; pass < 2; ++pass)
            for (int c = 0; c < M; ++c) {
              if (!(done & (1u << c))) continue;
              Cd d = cmake<double>(0.0, 0.0);  // u_c^H v
              for (int i = 0; i < M; ++i) {
                const Cd u = As[i * M + c];
                d.x = fma(u.x, v[i].x, d.x), d.x = fma(u.y, v[i].y, d.x);
                d.y = fma(u.x, v[i].y, d.y), d.y = fma(-u.y, v[i].x, d.y);
              }
              for (int i = 0; i < M; ++i) {
                const Cd u = As[i * M + c];
                v[i].x -= u.x * d.x - u.y * d.y;
                v[i].y -= u.x * d.y + u.y * d.x;
              }
            }
          double nn = 0.0;
          for (int i = 0; i < M; ++i) nn = fma(v[i].x, v[i].x, nn), nn = fma(v[i].y, v[i].y, nn);
          if (nn * (2.0 * M) >= 1.0 || k == M - 1) {  // some e_k keeps at least 1 / M of its length
            const double r = nn > 0.0 ? 1.0 / sqrt(nn) : 0.0;
            for (int i = 0; i < M; ++i) As[i * M + j] = cmake<double>(v[i].x * r, v[i].y * r);
            done |= 1u << j;
            break;
          }
        }
      }
    }
    __syncthreads();

    Cd wt = cmake<double>(0.0, 0.0);
    if (active) {  // Wt[n][m] = sum_j U[n][j] h_j conj(V[m][j])
#pragma unroll
      for (int j = 0; j < M; ++j) {
        const Cd u = As[n * M + j], v = Vs[m * M + j];
        const double h = hs[j];
        const Cd uv = cmake<double>(u.x * v.x + u.y * v.y, u.y * v.x - u.x * v.y);
        wt.x = fma(h, uv.x, wt.x), wt.y = fma(h, uv.y, wt.y);
      }
    }
    if (mode == FIN_PROX) {
      if (active) out[(size_t)f * MM + e] = wt;
      return;
    }
    __syncthreads();
    if (active) {
      const Cd w = Ws[e];
      D[(size_t)f * MM + e] = cmake<double>(fma(2.0, wt.x, -w.x), fma(2.0, wt.y, -w.y));
      const double beta = 1.0 - alpha;
      const Cd wn = cmake<double>(fma(alpha, wt.x, beta * w.x), fma(alpha, wt.y, beta * w.y));
      Ws[e] = wn;
      W[(size_t)f * MM + e] = wn;
    }
  } else if (active) {
    Ws[e] = W[(size_t)f * MM + e];
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

// norm[0] = sqrt(max_f lam[f]); a NaN among them stays
__global__ void __launch_bounds__(BLK) pd_norm_max_kernel(const double* __restrict__ lam, int F, double* __restrict__ norm) {
  __shared__ double red[BLK];
  double best = 0.0;
  for (int f = threadIdx.x; f < F; f += BLK) {
    const double v = lam[f];
    if (best == best && (v > best || v != v)) best = v;
  }
  red[threadIdx.x] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 1; j < BLK; ++j) {
      const double v = red[j];
      if (best == best && (v > best || v != v)) best = v;
    }
    norm[0] = sqrt(best);
  }
}

// loss[0] = C (sum of the n data partials) - (sum of the F log-determinants), each sum in a fixed order; terms: the two
__global__ void __launch_bounds__(BLK) pd_loss_close_kernel(const double* __restrict__ lpart, int n,
                                                            const double* __restrict__ logdet, int F, double Creg,
                                                            double* __restrict__ loss, double* __restrict__ terms) {
  __shared__ double red[NW];
  double data, ld;
  loss_sums(lpart, n, logdet, F, red, data, ld);
  if (threadIdx.x == 0) {
    const double pen = Creg * data;
    loss[0] = pen - ld;
    if (terms) terms[0] = pen, terms[1] = -ld;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
int pd_check(assx_ctx* ctx, int M, int F, int T) { return check_bin_sizes(ctx, "ProxLaplaceIVA", M, F, T); }

int pd_check_penalty(assx_ctx* ctx, int penalty) {
  ASSX_REQUIRE(ctx, penalty == ASSX_PDSBSS_LAPLACE, ASSX_E_ARG, "penalty must be 0 (the Laplace group norm), got %d", penalty);
  return 0;
}

int pd_check_steps(assx_ctx* ctx, double Creg, double mu1, double mu2, double alpha) {
  ASSX_REQUIRE(ctx, std::isfinite(Creg) && std::isfinite(alpha), ASSX_E_ARG, "regularizer and step must be finite");
  ASSX_REQUIRE(ctx, std::isfinite(mu1) && mu1 > 0.0 && std::isfinite(mu2) && mu2 > 0.0, ASSX_E_ARG,
               "step_prox_logdet and step_prox_penalty must be finite and > 0, got %g and %g", mu1, mu2);
  return 0;
}

struct PdRun : RunBase {
  assx_ctx* ctx;
  const Cd* X;
  Cd* W;
  Cd* y;
  const double* norm;
  int M, F, T;
  PdLayout L;
};

// sweep 2, or with do_update = 0 the adjoint partials of y as it stands
int pd_stage_dual(const PdRun& g, Cd* y, size_t ysF, size_t ysN, double alpha, int do_update) {
  return launch_for_channels(g.ctx, "ProxLaplaceIVA", "pd_dual_kernel", g.M, [&](auto mt) {
    hipLaunchKernelGGL((pd_dual_kernel<decltype(mt)::value>), dim3((unsigned)g.F * pd_chunks(g.T)), dim3(BLK), 0, g.st, g.X,
                       y, ysF, ysN, (const Cd*)g.at<Cd>(g.L.D), (const double*)g.at<double>(g.L.s), g.norm, alpha,
                       g.at<Cd>(g.L.part), do_update, g.F, g.T, pd_chunks(g.T));
  });
}

int pd_stage_finalize(const PdRun& g, int F, int mode, const Cd* in, Cd* out, double mu, double mu12, double alpha,
                      int32_t* status) {
  return launch_for_channels(g.ctx, "ProxLaplaceIVA", "pd_finalize_kernel", g.M, [&](auto mt) {
    hipLaunchKernelGGL((pd_finalize_kernel<decltype(mt)::value>), dim3(F), dim3(WAVE), 0, g.st, g.W, in, out,
                       g.ws ? (const Cd*)g.at<Cd>(g.L.part) : (const Cd*)nullptr, g.ws ? g.at<Cd>(g.L.D) : (Cd*)nullptr,
                       g.ws ? g.at<double>(g.L.logdet) : (double*)nullptr, g.norm, mode, mu, mu12, alpha, pd_chunks(g.T),
                       status);
  });
}

// sweep 1 and the slice sums: s (do_z) and the data partials of the loss of W (do_w)
int pd_stage_group(const PdRun& g, double Creg, double mu2, int do_z, int do_w) {
  const int FS = pd_slices(g.F);
  return dispatch_channels(g.ctx, "ProxLaplaceIVA", g.M, [&](auto mt) -> int {
    constexpr int MC = decltype(mt)::value;
    hipLaunchKernelGGL((pd_group_kernel<MC>), dim3(nblocks(g.T, WAVE), FS), dim3(WAVE), 0, g.st, g.X, (const Cd*)g.y,
                       (const Cd*)g.at<Cd>(g.L.D), (const Cd*)g.W, g.norm, g.at<double>(g.L.r2z), g.at<double>(g.L.r2w),
                       do_z, do_w, g.F, g.T, FS);
    ASSX_LAUNCH_CHECK(g.ctx, "pd_group_kernel");
    hipLaunchKernelGGL(pd_shrink_kernel, dim3((unsigned)g.L.n_lpart), dim3(BLK), 0, g.st,
                       (const double*)g.at<double>(g.L.r2z), (const double*)g.at<double>(g.L.r2w), g.at<double>(g.L.s),
                       g.at<double>(g.L.lpart), (size_t)g.M * g.T, FS, Creg, 1.0 / mu2, do_z ? SHRINK_STEP : SHRINK_NONE,
                       do_w);
    ASSX_LAUNCH_CHECK(g.ctx, "pd_shrink_kernel");
    return 0;
  });
}

int pd_stage_close(const PdRun& g, double Creg, double* loss, double* terms) {
  hipLaunchKernelGGL(pd_loss_close_kernel, dim3(1), dim3(BLK), 0, g.st, (const double*)g.at<double>(g.L.lpart),
                     (int)g.L.n_lpart, (const double*)g.at<double>(g.L.logdet), g.F, Creg, loss, terms);
  ASSX_LAUNCH_CHECK(g.ctx, "pd_loss_close_kernel");
  return 0;
}

// the loss of W as it stands: a loss-only sweep 1, ln|det W| from the tail of the finalize kernel
int pd_loss_alone(const PdRun& g, double Creg, double* loss, double* terms) {
  int rc = pd_stage_group(g, Creg, 1.0, 0, 1);
  if (!rc) rc = pd_stage_finalize(g, g.F, FIN_LOGDET, nullptr, nullptr, 0.0, 0.0, 0.0, nullptr);
  if (!rc) rc = pd_stage_close(g, Creg, loss, terms);
  return rc;
}

// one iteration from valid partials of G: finalize, sweep 1 (the loss of the new W rides on it), sweep 2
int pd_iteration(const PdRun& g, double Creg, double mu1, double mu2, double alpha, int with_loss, int32_t* status) {
  int rc = pd_stage_finalize(g, g.F, FIN_UPDATE, nullptr, nullptr, mu1, mu1 * mu2, alpha, status);
  if (!rc) rc = pd_stage_group(g, Creg, mu2, 1, with_loss);
  if (!rc) rc = pd_stage_dual(g, g.y, (size_t)g.M * g.T, (size_t)g.T, alpha, 1);
  return rc;
}

PdRun pd_run(assx_ctx* ctx, const void* X, const void* norm, void* W, void* y, void* ws, int M, int F, int T, void* stream) {
  return PdRun{{(char*)ws, (hipStream_t)stream}, ctx, (const Cd*)X, (Cd*)W, (Cd*)y, (const double*)norm, M, F, T,
               pd_layout(M, F, T)};
}

}  // namespace

extern "C" {

size_t assx_pdsbss_workspace_bytes(int M, int F, int T) {
  if (!in_envelope(M, F, T)) return 0;
  return pd_layout(M, F, T).total;
}

int assx_pdsbss_operator_norm(assx_ctx* ctx, const void* X, void* ws, double* norm, int M, int F, int T, int32_t* status,
                              void* stream) {
  int rc = pd_check(ctx, M, F, T);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && ws && norm, ASSX_E_NULL, "assx_pdsbss_operator_norm: NULL array");
  const PdRun g = pd_run(ctx, X, norm, nullptr, nullptr, ws, M, F, T, stream);
  // the Gram matrix of a bin is the adjoint sweep with X in place of y; X is only read (do_update = 0)
  rc = pd_stage_dual(g, const_cast<Cd*>(g.X), (size_t)T, (size_t)F * T, 0.0, 0);
  if (!rc) rc = pd_stage_finalize(g, F, FIN_GRAM, nullptr, nullptr, 0.0, 0.0, 0.0, status);
  if (rc) return rc;
  hipLaunchKernelGGL(pd_norm_max_kernel, dim3(1), dim3(BLK), 0, g.st, (const double*)g.at<double>(g.L.logdet), F, norm);
  ASSX_LAUNCH_CHECK(ctx, "pd_norm_max_kernel");
  return 0;
}

int assx_pdsbss_adjoint(assx_ctx* ctx, const void* X, const double* norm, const void* y, void* G, void* ws, int M, int F,
                        int T, void* stream) {
  int rc = pd_check(ctx, M, F, T);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && norm && y && G && ws, ASSX_E_NULL, "assx_pdsbss_adjoint: NULL array");
  const PdRun g = pd_run(ctx, X, norm, nullptr, const_cast<void*>(y), ws, M, F, T, stream);
  rc = pd_stage_dual(g, g.y, (size_t)M * T, (size_t)T, 0.0, 0);
  if (!rc) rc = pd_stage_finalize(g, F, FIN_ADJOINT, nullptr, (Cd*)G, 0.0, 0.0, 0.0, nullptr);
  return rc;
}

int assx_pdsbss_prox_logdet(assx_ctx* ctx, const void* Win, void* Wout, double mu, int M, int F, int32_t* status,
                            void* stream) {
  int rc = pd_check(ctx, M, F, 1);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, std::isfinite(mu) && mu > 0.0, ASSX_E_ARG, "mu must be finite and > 0, got %g", mu);
  ASSX_REQUIRE(ctx, Win && Wout, ASSX_E_NULL, "assx_pdsbss_prox_logdet: NULL array");
  const PdRun g = pd_run(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, M, F, 1, stream);
  return pd_stage_finalize(g, F, FIN_PROX, (const Cd*)Win, (Cd*)Wout, mu, 0.0, 0.0, status);
}

int assx_pdsbss_forward(assx_ctx* ctx, const void* X, const double* norm, const void* y, const void* D, void* z, int M, int F,
                        int T, void* stream) {
  int rc = pd_check(ctx, M, F, T);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && norm && y && D && z, ASSX_E_NULL, "assx_pdsbss_forward: NULL array");
  const int ntile = (int)nblocks(T, WAVE);
  return launch_for_channels(ctx, "ProxLaplaceIVA", "pd_forward_kernel", M, [&](auto mt) {
    hipLaunchKernelGGL((pd_forward_kernel<decltype(mt)::value>), dim3((unsigned)F * ntile), dim3(WAVE), 0,
                       (hipStream_t)stream, (const Cd*)X, (const Cd*)y, (const Cd*)D, norm, (Cd*)z, F, T, ntile);
  });
}

int assx_pdsbss_prox_group(assx_ctx* ctx, int penalty, const void* z, void* out, void* ws, double C, double mu, int N, int F,
                           int T, void* stream) {
  int rc = pd_check(ctx, N, F, T);
  if (!rc) rc = pd_check_penalty(ctx, penalty);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, std::isfinite(C) && std::isfinite(mu) && mu > 0.0, ASSX_E_ARG,
               "regularizer must be finite and mu finite and > 0, got %g and %g", C, mu);
  ASSX_REQUIRE(ctx, z && out && ws, ASSX_E_NULL, "assx_pdsbss_prox_group: NULL array");
  const PdRun g = pd_run(ctx, nullptr, nullptr, nullptr, nullptr, ws, N, F, T, stream);
  const size_t NT = (size_t)N * T;
  const int FS = pd_slices(F);
  hipLaunchKernelGGL(pd_norm2_kernel, dim3(nblocks(NT, BLK), FS), dim3(BLK), 0, g.st, (const Cd*)z, g.at<double>(g.L.r2z), F,
                     NT, FS);
  ASSX_LAUNCH_CHECK(ctx, "pd_norm2_kernel");
  hipLaunchKernelGGL(pd_shrink_kernel, dim3(nblocks(NT, BLK)), dim3(BLK), 0, g.st, (const double*)g.at<double>(g.L.r2z),
                     (const double*)nullptr, g.at<double>(g.L.s), (double*)nullptr, NT, FS, C, mu, SHRINK_PROX, 0);
  ASSX_LAUNCH_CHECK(ctx, "pd_shrink_kernel");
  hipLaunchKernelGGL(pd_apply_kernel, dim3(nblocks(NT * F, BLK)), dim3(BLK), 0, g.st, (const Cd*)z,
                     (const double*)g.at<double>(g.L.s), (Cd*)out, NT, NT * F);
  ASSX_LAUNCH_CHECK(ctx, "pd_apply_kernel");
  return 0;
}

int assx_pdsbss_update(assx_ctx* ctx, int penalty, const void* X, const double* norm, void* W, void* y, void* ws, double C,
                       double mu1, double mu2, double alpha, int M, int F, int T, int32_t* status, void* stream) {
  int rc = pd_check(ctx, M, F, T);
  if (!rc) rc = pd_check_penalty(ctx, penalty);
  if (!rc) rc = pd_check_steps(ctx, C, mu1, mu2, alpha);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && norm && W && y && ws, ASSX_E_NULL, "assx_pdsbss_update: NULL array");
  const PdRun g = pd_run(ctx, X, norm, W, y, ws, M, F, T, stream);
  rc = pd_stage_dual(g, g.y, (size_t)M * T, (size_t)T, 0.0, 0);
  if (!rc) rc = pd_iteration(g, C, mu1, mu2, alpha, 0, status);
  return rc;
}

int assx_pdsbss_loss(assx_ctx* ctx, int penalty, const void* X, const void* W, void* ws, double C, double* loss,
                     double* terms, int M, int F, int T, void* stream) {
  int rc = pd_check(ctx, M, F, T);
  if (!rc) rc = pd_check_penalty(ctx, penalty);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, std::isfinite(C), ASSX_E_ARG, "regularizer must be finite");
  ASSX_REQUIRE(ctx, X && W && ws && loss, ASSX_E_NULL, "assx_pdsbss_loss: NULL array");
  const PdRun g = pd_run(ctx, X, nullptr, const_cast<void*>(W), nullptr, ws, M, F, T, stream);
  return pd_loss_alone(g, C, loss, terms);
}

int assx_pdsbss_iterate(assx_ctx* ctx, int n_iter, int record_loss, int penalty, const void* X, const double* norm, void* W,
                        void* y, void* ws, double C, double mu1, double mu2, double alpha, double* loss, int M, int F, int T,
                        int32_t* status, void* stream) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, n_iter >= 0, ASSX_E_ARG, "n_iter must be >= 0, got %d", n_iter);
  ASSX_REQUIRE(ctx, record_loss == 0 || record_loss == 1, ASSX_E_ARG, "record_loss must be 0 or 1, got %d", record_loss);
  int rc = pd_check(ctx, M, F, T);
  if (!rc) rc = pd_check_penalty(ctx, penalty);
  if (!rc) rc = pd_check_steps(ctx, C, mu1, mu2, alpha);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && norm && W && y && ws && (loss || !record_loss), ASSX_E_NULL, "assx_pdsbss_iterate: NULL array");
  const PdRun g = pd_run(ctx, X, norm, W, y, ws, M, F, T, stream);
  // loss[0] belongs to the W at entry; loss[i + 1] rides on sweep 1 of iteration i.  The adjoint sweep runs once: every
  // later iteration finds the partials of its G where the sweep 2 before it left them.
  if (record_loss) rc = pd_loss_alone(g, C, loss, nullptr);
  if (!rc && n_iter > 0) rc = pd_stage_dual(g, g.y, (size_t)M * T, (size_t)T, 0.0, 0);
  for (int i = 0; i < n_iter && !rc; ++i) {
    rc = pd_iteration(g, C, mu1, mu2, alpha, record_loss, status);
    if (!rc && record_loss) rc = pd_stage_close(g, C, loss + i + 1, nullptr);
  }
  return rc;
}

}  // extern "C"
