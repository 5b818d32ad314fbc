// What the per-bin BSS families share -- gradient IVA / FDICA (assx_gradbss.hip), ProxLaplaceIVA (assx_pdsbss.hip),
// GaussIDLMA (assx_idlma.hip) and the beamformers, PCA and MDP (assx_beamform.hip): kernels whose lanes are frames, one
// workgroup per (bin, frame chunk), one wave per bin to finish.  The row split of an M x M moment over the waves, the copy
// of a bin's matrix into LDS, the frame gather, the chunk, slice and envelope arithmetic, the sums below, and the host
// side's size check, workspace view and single-launch frame.
//
// Every family promises bit-reproducible results.  The order of every sum made here is part of that promise:
//   reduce_rows_store  a wave's butterfly (offsets 32, 16, .., 1) per accumulator; then, per entry, the frame groups of the
//                      entry's row group in index order, starting from the first group's value (r0 + r1 ..)
//   chunk_sum          the chunks of a bin in index order, from 0 (0 + p0 + p1 ..), real and imaginary part apart
//   slice_sum          the slices in index order, from 0
//   loss_sums          strided_sum of assx_factor_common.hpp (a stride of BLK per thread, the butterfly, the waves in index
//                      order), the data partials first, the log-determinants second
// No float atomics.  A loss's closing formula is NOT shared: a * data + b * ld in one form for all would round differently.
#pragma once
#include "assx_common.hpp"
#include "assx_small_linalg.hpp"
#include "assx_factor_common.hpp"

namespace assx {
namespace pb {

using namespace assx::mf;

constexpr int NW = BLK / WAVE;  // waves of a workgroup of BLK threads

// ---- host side.  The envelope: 2 <= M <= 8, at least min_frames frames, X below 4 GiB in complex128 (no product overflows)
inline bool in_envelope(int M, int F, int T, int min_frames = 1) {
  if (M < 2 || M > 8 || F < 1 || T < min_frames || F >= (1 << 28) || T >= (1 << 28)) return false;
  return (long long)M * F * T < (1LL << 28);
}
inline int chunks(int T, int chunk) { return (T + chunk - 1) / chunk; }  // frame chunks of a bin
inline int slices(int F, int cap) { return F < cap ? F : cap; }          // bin slices of a pass over all bins

// the context and the sizes of an entry point of gradient IVA / FDICA and of ProxLaplaceIVA; label: the model's name.  IDLMA
// and the beamformers put the entry point's name in front of the first message and check more: each keeps its check
inline int check_bin_sizes(assx_ctx* ctx, const char* label, int M, int F, int T) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, F >= 1 && T >= 1, ASSX_E_ARG, "invalid sizes F=%d T=%d", F, T);
  ASSX_REQUIRE(ctx, M >= 2 && M <= 8, ASSX_E_UNSUPPORTED, "%s: n_channels must be in [2, 8], got %d", label, M);
  ASSX_REQUIRE(ctx, in_envelope(M, F, T), ASSX_E_UNSUPPORTED,
               "%s: the input must stay below 4 GiB in complex128 (M*F*T < 2^28)", label);
  return 0;
}

// what every *Run struct begins with: the workspace, a view of one of its arrays, the stream
struct RunBase {
  char* ws;
  hipStream_t st;
  template <typename P>
  P* at(size_t off) const { return (P*)(ws + off); }
};

// one launch of a kernel instantiated per channel count: fn(IntC<M>()) enqueues it, `kernel` names it if the launch fails
template <typename Fn>
int launch_for_channels(assx_ctx* ctx, const char* label, const char* kernel, int M, Fn&& fn) {
  return dispatch_channels(ctx, label, M, [&](auto mt) -> int {
    fn(mt);
    ASSX_LAUNCH_CHECK(ctx, kernel);
    return 0;
  });
}

// ---- device side.  Rows of an M x M moment per wave: all M up to M = 6; at M = 7, 8 two wave pairs take half the rows
// each, so that a lane holds at most 4 x 8 complex accumulators (128 VGPRs) instead of 8 x 8
template <int M>
struct RowSplit {
  static_assert(NW == 4, "the row split pairs four waves");
  static constexpr int RG = M >= 7 ? 2 : 1;      // row groups
  static constexpr int RPW = (M + RG - 1) / RG;  // rows per wave
  static constexpr int NFG = NW / RG;            // frame groups (waves that share a row group)
  static constexpr int ROWS = RG * RPW;          // rows of the LDS copy: M, or M + 1 with a zero spare row
};

// a zero the optimiser cannot see through (no instruction is emitted): an LDS address formed with it is loop-variant
__device__ __forceinline__ unsigned lds_opaque() {
  unsigned v = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v));
#endif
  return v;
}

// the end of chunk c of `chunk` frames: the last chunk ends at T
__device__ __forceinline__ int chunk_end(int c, int chunk, int T) { return T - c * chunk < chunk ? T : (c + 1) * chunk; }

// the bins [f0, f1) of slice s of FS
__device__ __forceinline__ void slice_bounds(int F, int s, int FS, int& f0, int& f1) {
  f0 = (int)((long long)F * s / FS), f1 = (int)((long long)F * (s + 1) / FS);
}

// x[m] = X[m,f,t], X (M,F,T) with T fastest
template <int M>
__device__ __forceinline__ void load_frame(const Cd* __restrict__ X, int f, int t, int F, int T, Cd (&x)[M]) {
#pragma unroll
  for (int m = 0; m < M; ++m) x[m] = X[((size_t)m * F + f) * T + t];
}

// S (RowSplit<M>::ROWS x M in LDS) = the M x M matrix A of one bin, spare rows zero -- or all zero -- and the barrier
template <int M>
__device__ __forceinline__ void bin_matrix_to_lds(Cd* S, const Cd* __restrict__ A, bool all_zero = false) {
  for (int i = threadIdx.x; i < RowSplit<M>::ROWS * M; i += BLK)
    S[i] = (!all_zero && i < M * M) ? A[i] : cmake<double>(0.0, 0.0);
  __syncthreads();
}

// out[n,m] = the workgroup's sum of acc, the wave of row group g and frame group q holding rows g RPW .. of it
template <int M>
__device__ __forceinline__ void reduce_rows_store(const Cd (&acc)[RowSplit<M>::RPW][M],
                                                  double (*red)[RowSplit<M>::RPW * M * 2], Cd* __restrict__ out) {
  using RS = RowSplit<M>;
  constexpr int RG = RS::RG, RPW = RS::RPW, NFG = RS::NFG;
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
#pragma unroll
  for (int i = 0; i < RPW; ++i)
#pragma unroll
    for (int m = 0; m < M; ++m) {
      const double vr = wave_sum_down(acc[i][m].x), vi = wave_sum_down(acc[i][m].y);
      if (lane == 0) red[wave][(i * M + m) * 2] = vr, red[wave][(i * M + m) * 2 + 1] = vi;
    }
  __syncthreads();
  if (tid < M * M) {  // the frame groups of the entry's row group, in index order
    const int n = tid / M, m = tid % M, g = n / RPW, i = n % RPW;
    double sr = red[g][(i * M + m) * 2], si = red[g][(i * M + m) * 2 + 1];
    for (int q = 1; q < NFG; ++q) sr += red[q * RG + g][(i * M + m) * 2], si += red[q * RG + g][(i * M + m) * 2 + 1];
    out[tid] = cmake<double>(sr, si);
  }
}

// the sum of the C chunk partials part[f, 0 .. C, e] of one entry of part (F, C, MM), in index order
template <int MM>
__device__ __forceinline__ Cd chunk_sum(const Cd* __restrict__ part, int f, int C, int e) {
  double sr = 0.0, si = 0.0;
  for (int c = 0; c < C; ++c) {
    const Cd p = part[((size_t)f * C + c) * MM + e];
    sr += p.x, si += p.y;
  }
  return cmake<double>(sr, si);
}

// the sum of the FS slice partials p[0], p[stride], .., in index order
__device__ __forceinline__ double slice_sum(const double* __restrict__ p, size_t stride, int FS) {
  double s = 0.0;
  for (int k = 0; k < FS; ++k) s += p[(size_t)k * stride];
  return s;
}

// the two sums a loss closes with, each in a fixed order: thread 0 gets the n data partials and the F log-determinants
__device__ __forceinline__ void loss_sums(const double* __restrict__ lpart, int n, const double* __restrict__ logdet, int F,
                                          double* red, double& data, double& ld) {
  data = strided_sum(lpart, n, 1, red);
  __syncthreads();
  ld = strided_sum(logdet, F, 1, red);
}

}  // namespace pb
}  // namespace assx
