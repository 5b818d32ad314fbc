// What the seven factorisation families share -- FastMNMF (assx_fastmnmf.hip), MNMF (assx_mnmf.hip), covariance-domain
// MNMF (assx_covnmf.hip), ComplexEUCNMF (assx_cnmf.hip), EUCNTF (assx_ntf.hip), LDPSDTF (assx_psdtf.hip, through
// assx_sym_linalg.hpp) and the two IPSDTA models (assx_ipsdta.hip): the limits and tile sizes, the fixed-order
// reductions of a workgroup, the per-utterance sum of partials, the slice sum of the activation update, the slab and
// slice counts, the carving of a workspace, and the channel dispatch and size check of the two MNMFs' entry points.
//
// Every family promises bit-reproducible, batch-independent results.  The order of every sum made here is part of that
// promise: a wave's butterfly (offsets 32, 16, .., 1); then the waves of a workgroup in index order; then slices in
// index order.  No float atomics.  The two block sums differ in their arithmetic (0 + r0 + r1 .. against
// ((r0 + r1) + r2) + r3) and a family keeps the one it was written with.
#pragma once
#include "assx_common.hpp"

namespace assx {
namespace mf {

constexpr int NMAX = 8;     // sources
constexpr int KMAX = 64;    // n_basis
constexpr int CH = 16;      // (numerator, denominator) pairs a thread accumulates per chunk
constexpr int FS_ACT = 16;  // f slices of the activation update
constexpr int BLK = 256;    // threads of the per-bin kernels
constexpr int ABLK = 64;    // threads (frames) of an activation workgroup
constexpr int SP_SLICES = 8;  // t slices of the spatial sums of the two MNMFs

inline unsigned nblocks(size_t n, int b) { return (unsigned)((n + b - 1) / b); }
inline int act_slices(int F) { return F < FS_ACT ? F : FS_ACT; }
// slabs of at least 8 bins, at most cap of them
inline int slabs8(int n, int cap) {
  const int s = (n + 7) / 8;
  return s > cap ? cap : s;
}
// t slices of the spatial sums: whole wave tiles of frames, at most SP_SLICES
inline int sp_slices(int T) {
  const int tiles = (T + WAVE - 1) / WAVE;
  return tiles < SP_SLICES ? tiles : SP_SLICES;
}

// Offsets of the arrays of a workspace, handed out front to back: take(bytes) returns the current offset and advances
// to the next multiple of align.  A workspace size is a public number: align is 256 or 1 (packed) as the family had it.
class Carve {
 public:
  explicit Carve(size_t align) : align_(align) {}
  size_t take(size_t bytes) {
    const size_t at = off_;
    off_ = align_up(off_ + bytes, align_);
    return at;
  }
  size_t total() const { return off_; }

 private:
  size_t align_, off_ = 0;
};

template <typename R>
__device__ __forceinline__ R wave_sum_down(R v) {  // fixed butterfly; the total lands in lane 0
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, WAVE);
  return v;
}

// The sum of v over a workgroup of NW waves: the butterfly, lane 0 of every wave leaves its total in red[w], a barrier,
// thread 0 adds the waves in index order.  Only thread 0 returns the total (the others 0).  red is free again after the
// caller's next barrier.
template <typename R, int NW>
__device__ __forceinline__ R block_sum(R v, R* red) {
  const int tid = threadIdx.x;
  v = wave_sum_down(v);
  if ((tid & (WAVE - 1)) == 0) red[tid / WAVE] = v;
  __syncthreads();
  R s = 0;
  if (tid == 0)
    for (int w = 0; w < NW; ++w) s += red[w];
  return s;
}

// The sum of v over a workgroup of four waves, returned to every thread: an xor butterfly, then the waves in index
// order.  red (four doubles) may still be read by a straggler of the previous call, hence the first barrier.
__device__ __forceinline__ double block_sum_all(double v, double* red) {
  for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// The same for the CH (numerator, denominator) pairs of a chunk: every thread brings its partial sums num[c], den[c];
// thread c < CH returns the workgroup's totals of pair c in (sn, sd), the others (0, 0).  red is free again after the
// caller's next barrier.
template <typename R, int NW>
__device__ __forceinline__ void block_pair_sums(const R (&num)[CH], const R (&den)[CH], R (*red)[2 * CH], R& sn, R& sd) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    const R vn = wave_sum_down(num[c]), vd = wave_sum_down(den[c]);
    if ((tid & (WAVE - 1)) == 0) red[tid / WAVE][2 * c] = vn, red[tid / WAVE][2 * c + 1] = vd;
  }
  __syncthreads();
  sn = 0, sd = 0;
  if (tid < CH)
    for (int w = 0; w < NW; ++w) sn += red[w][2 * tid], sd += red[w][2 * tid + 1];
}

// The sum of n values, stride apart, by a workgroup of BLK threads in a fixed order: every thread its own stride of
// BLK, then the workgroup by block_sum (thread 0 returns the total) or, with ALL, by block_sum_all (every thread does).
template <bool ALL = false>
__device__ __forceinline__ double strided_sum(const double* __restrict__ p, int n, size_t stride, double* red) {
  double v = 0;
  for (int i = threadIdx.x; i < n; i += BLK) v += p[(size_t)i * stride];
  if constexpr (ALL) return block_sum_all(v, red);
  return block_sum<double, BLK / WAVE>(v, red);
}

// out[b] = the sum of partials[b, 0 .. n_per_b) in that order, one workgroup per b: the last step of a loss (covnmf
// keeps a kernel of its own)
template <bool ALL = false>
__global__ void __launch_bounds__(BLK) batch_sum_kernel(const double* __restrict__ partials, double* __restrict__ out,
                                                        int n_per_b) {
  __shared__ double red[BLK / WAVE];
  const double tot = strided_sum<ALL>(partials + (size_t)blockIdx.x * n_per_b, n_per_b, 1, red);
  if (threadIdx.x == 0) out[blockIdx.x] = tot;
}

// Second half of both activation updates: V (B, NP, T) *= sqrt(num / max(den, eps)) with num and den the FS slice
// partials of part (B, FS, 2, NP, T) added in slice order.
template <typename R>
__global__ void __launch_bounds__(BLK) act_apply_kernel(R* __restrict__ V, const R* __restrict__ part, double eps_d,
                                                        int NP, int T, int FS, size_t total) {
  const size_t i = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (i >= total) return;
  const R eps = (R)eps_d;
  const size_t per = (size_t)NP * T, b = i / per, r = i % per;
  R num = 0, den = 0;
  for (int s = 0; s < FS; ++s) {
    const R* o = part + ((size_t)b * FS + s) * 2 * per + r;
    num += o[0];
    den += o[per];
  }
  den = den < eps ? eps : den;
  V[i] = V[i] * sqrt(num / den);
}

// fn(IntC<M>()) for the M = 2..8 the kernels are instantiated for
template <typename Fn>
int dispatch_channels(assx_ctx* ctx, const char* label, int M, Fn&& fn) {
  switch (M) {
    case 2: return fn(IntC<2>());
    case 3: return fn(IntC<3>());
    case 4: return fn(IntC<4>());
    case 5: return fn(IntC<5>());
    case 6: return fn(IntC<6>());
    case 7: return fn(IntC<7>());
    case 8: return fn(IntC<8>());
  }
  return fail(ctx, ASSX_E_UNSUPPORTED, "%s: n_channels must be in [2, 8], got %d", label, M);
}

// the context and the sizes of every MNMF and FastMNMF entry point; label: the model's name in the messages.  The other
// families check in an order of their own, which decides the code and the text when two arguments are wrong at once, so
// each keeps its check
inline int check_sizes(assx_ctx* ctx, const char* label, bool f64_only, int B, int M, int N, int F, int T, int K,
                       int dtype) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, B >= 1 && F >= 1 && T >= 1, ASSX_E_ARG, "invalid sizes B=%d F=%d T=%d", B, F, T);
  ASSX_REQUIRE(ctx, dtype == ASSX_F64 || dtype == ASSX_F32, ASSX_E_ARG, "bad dtype %d", dtype);
  ASSX_REQUIRE(ctx, !f64_only || dtype == ASSX_F64, ASSX_E_UNSUPPORTED, "%s: float64 only", label);
  ASSX_REQUIRE(ctx, M >= 2 && M <= 8, ASSX_E_UNSUPPORTED, "%s: n_channels must be in [2, 8], got %d", label, M);
  ASSX_REQUIRE(ctx, N >= 1 && N <= NMAX, ASSX_E_UNSUPPORTED, "%s: n_sources must be in [1, 8], got %d", label, N);
  ASSX_REQUIRE(ctx, K >= 1 && K <= KMAX, ASSX_E_UNSUPPORTED, "%s: n_basis must be in [1, 64], got %d", label, K);
  ASSX_REQUIRE(ctx, (long long)M * F * T < (1LL << 28), ASSX_E_UNSUPPORTED,
               "%s: one utterance must stay below 4 GiB in complex128 (M*F*T < 2^28)", label);
  return 0;
}

}  // namespace mf
}  // namespace assx
