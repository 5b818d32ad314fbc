// GaussIDLMA (src/sss/idlma.py:89-246) around its network on MI355X: everything of an iteration that is not the DNN's
// forward pass.  float64 state, one utterance, 2 <= M <= 8 channels, N = M sources, F >= 1 bins, T >= M frames.
//
// Arrays: X (M,F,T) complex128 with T fastest, W (F,N,M) complex128, the network's input and output and dnn_output
// (N,F,T) float32, the variance R (N,F,T) float64 (every value a widened float32), scale (N,F) complex128.
//
// Launches:
//   input, loss   idlma_tail_kernel<M, LOSS, INPUT> (bin x chunk of ID_CHUNK frames, a flat grid): a thread takes ID_VEC
//                 consecutive frames, the M samples of a frame in registers, the bin's filter through wave-uniform
//                 addresses; y = W_f x once, p = |y|^2.  INPUT: (float)p^(domain/2) into the network's input, one 16-byte
//                 store per source where the rows allow it.  LOSS: sum p / R + log R of the thread's frames and sources in
//                 index order, a wave's butterfly, the waves in index order, one partial per workgroup.  The three
//                 instantiations run the same arithmetic on the same partition: the fused one gives the bits of the two
//   loss close    idlma_logdet_kernel (a bin per thread, LU with partial pivoting) and idlma_loss_close_kernel (one
//                 workgroup: the partials, then the bins, each in a fixed order)
//   variance      idlma_variance_kernel, element-wise in float32 as NumPy runs it on the network's float32 output
//                 (idlma.py:223, 230, 183/242, 189/243), four elements per thread
//   normalise     idlma_normalize_pb_kernel: W[f,n,:] *= scale[n,f]
// The spatial update is assx_idlma_space_update on R with domain 2, the scale assx_projection_back_scale.
//
// Every sum has a fixed order and there is no float atomic: two runs give the same bits.
#include "assx_perbin_common.hpp"

using namespace assx;
using namespace assx::mf;
using namespace assx::pb;

namespace {

constexpr int ID_VEC = 4;                         // frames of one thread: one 16-byte store of float32
constexpr int ID_CHUNK = ASSX_IDLMA_FRAME_CHUNK;  // frames of one workgroup

static_assert(ID_CHUNK == BLK * ID_VEC, "a chunk is one trip of the workgroup");

inline bool id_in_envelope(int M, int F, int T) { return in_envelope(M, F, T, M); }  // at least M frames
inline int id_chunks(int T) { return chunks(T, ID_CHUNK); }

// part (F, chunks) loss partials, ldet (F), scale (N,F) complex, R (N,F,T), then the scratch of the spatial update and
// the projection-back scale (assx_workspace_bytes)
struct IdLayout {
  size_t part, ldet, scale, R, inner, total;
};

inline IdLayout id_layout(int M, int F, int T) {
  IdLayout L;
  Carve c(256);
  L.part = c.take((size_t)F * id_chunks(T) * sizeof(double));
  L.ldet = c.take((size_t)F * sizeof(double));
  L.scale = c.take((size_t)M * F * sizeof(Cd));
  L.R = c.take((size_t)M * F * T * sizeof(double));
  L.inner = c.take(assx_workspace_bytes(1, M, F, T, 1, ASSX_F64));
  L.total = c.total();
  return L;
}

// x**e of a float32 array and a Python float in NumPy: the identity for 1, a multiply for 2, powf otherwise
enum { IDP_ID = 0, IDP_SQUARE = 1, IDP_POW = 2 };

struct PowF {
  float e;
  int mode;
};

inline PowF make_powf(double e) {
  PowF p;
  p.e = (float)e;
  p.mode = e == 1.0 ? IDP_ID : e == 2.0 ? IDP_SQUARE : IDP_POW;
  return p;
}

__device__ __forceinline__ float powf_spec(float x, PowF p) {
  if (p.mode == IDP_ID) return x;
  if (p.mode == IDP_SQUARE) return x * x;
  return powf(x, p.e);
}

// ---------------------------------------------------------------------------------------------------------------
// Workgroup f CH + ch takes chunk ch of bin f; thread tid the frames ch ID_CHUNK + tid ID_VEC + 0 .. ID_VEC - 1.
// vec: T is a multiple of ID_VEC and inp is 16-byte aligned, so every row of inp starts on a 16-byte boundary and a
// thread's frames are all inside T or all outside.
// ---------------------------------------------------------------------------------------------------------------
template <int M, bool LOSS, bool INPUT>
__global__ void __launch_bounds__(BLK) idlma_tail_kernel(const Cd* __restrict__ X, const Cd* __restrict__ W,
                                                         const double* __restrict__ R, float* __restrict__ inp,
                                                         double* __restrict__ part, PowSpec ps, int F, int T, int CH,
                                                         int vec) {
  __shared__ double red[NW];
  const int f = blockIdx.x / CH, ch = blockIdx.x % CH;
  const int t0 = ch * ID_CHUNK + (int)threadIdx.x * ID_VEC;
  const Cd* Wb = W + (size_t)f * M * M;
  double acc = 0.0;
  float q[M][ID_VEC];
#pragma unroll
  for (int k = 0; k < ID_VEC; ++k) {
    const int t = t0 + k;
    if (t < T) {
      Cd x[M];  // not load_frame of assx_perbin_common.hpp: inside this unrolled loop it moves the registers of every instance
#pragma unroll
      for (int m = 0; m < M; ++m) x[m] = tocx(ldv(X + ((size_t)m * F + f) * T + t));
#pragma unroll
      for (int n = 0; n < M; ++n) {
        Cd y = cmake<double>(0.0, 0.0);
#pragma unroll
        for (int m = 0; m < M; ++m) cfma(y, Wb[n * M + m], x[m]);
        const double p = cabs2(y);
        if constexpr (INPUT) q[n][k] = (float)powspec(p, ps);
        if constexpr (LOSS) {
          const double r = R[((size_t)n * F + f) * T + t];
          const double lr = (double)(float)log(r);
          acc += p / r + lr;
        }
      }
    }
  }
  if constexpr (INPUT) {
    if (t0 < T) {
#pragma unroll
      for (int n = 0; n < M; ++n) {
        float* o = inp + ((size_t)n * F + f) * T + t0;
        if (vec) {
          *reinterpret_cast<float4*>(o) = make_float4(q[n][0], q[n][1], q[n][2], q[n][3]);
        } else {
#pragma unroll
          for (int k = 0; k < ID_VEC; ++k)
            if (t0 + k < T) o[k] = q[n][k];
        }
      }
    }
  }
  if constexpr (LOSS) {
    const double tot = block_sum<double, NW>(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
  }
}

// ldet[f] = log|det W_f| (idlma.py:244)
template <int M>
__global__ void __launch_bounds__(WAVE) idlma_logdet_kernel(const Cd* __restrict__ W, double* __restrict__ ldet, int F) {
  const int f = blockIdx.x * WAVE + threadIdx.x;
  if (f >= F) return;
  Cd A[M][M];
#pragma unroll
  for (int i = 0; i < M; ++i)
#pragma unroll
    for (int j = 0; j < M; ++j) A[i][j] = W[((size_t)f * M + i) * M + j];
  const Cd det = lu_det<M>(A);
  ldet[f] = log(hypot(det.x, det.y));
}

// loss[0] = (the n data partials) - 2 T (the F log-determinants), each sum in a fixed order
__global__ void __launch_bounds__(BLK) idlma_loss_close_kernel(const double* __restrict__ part, int n,
                                                               const double* __restrict__ ldet, int F, int T,
                                                               double* __restrict__ loss) {
  __shared__ double red[NW];
  double data, ld;
  loss_sums(part, n, ldet, F, red, data, ld);
  if (threadIdx.x == 0) loss[0] = data - 2.0 * (double)T * ld;
}

// raw: src is the network's output: d = src^(2/domain) in float32, floored at (float)dnn_flooring when that is set, and
// written to dnn_output.  Otherwise src is a dnn_output as it stands.  R = d^(2/domain) in float32, floored at (float)eps,
// widened.  A NaN passes both floors, as numpy.maximum and the mask assignment pass it.
__global__ void __launch_bounds__(BLK) idlma_variance_kernel(const float* src, float* dnn_output, double* __restrict__ R,
                                                             PowF pw, int raw, int do_floor, float flooring, float eps,
                                                             size_t total, int vec) {
  const size_t i0 = ((size_t)blockIdx.x * BLK + threadIdx.x) * ID_VEC;
  if (i0 >= total) return;
  const bool whole = vec && i0 + ID_VEC <= total;
  float v[ID_VEC];
  if (whole) {
    const float4 s = *reinterpret_cast<const float4*>(src + i0);
    v[0] = s.x, v[1] = s.y, v[2] = s.z, v[3] = s.w;
  } else {
#pragma unroll
    for (int k = 0; k < ID_VEC; ++k) v[k] = i0 + k < total ? src[i0 + k] : 1.0f;
  }
  double r[ID_VEC];
#pragma unroll
  for (int k = 0; k < ID_VEC; ++k) {
    float d = v[k];
    if (raw) {
      d = powf_spec(d, pw);
      if (do_floor) d = (d < flooring || flooring != flooring) ? flooring : d;
      v[k] = d;
    }
    float rr = powf_spec(d, pw);
    rr = rr < eps ? eps : rr;
    r[k] = (double)rr;
  }
  if (whole) {
    if (raw) *reinterpret_cast<float4*>(dnn_output + i0) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<double2*>(R + i0) = make_double2(r[0], r[1]);
    *reinterpret_cast<double2*>(R + i0 + 2) = make_double2(r[2], r[3]);
  } else {
#pragma unroll
    for (int k = 0; k < ID_VEC; ++k)
      if (i0 + k < total) {
        if (raw) dnn_output[i0 + k] = v[k];
        R[i0 + k] = r[k];
      }
  }
}

// W[f,n,m] *= scale[n,f]
__global__ void __launch_bounds__(BLK) idlma_normalize_pb_kernel(Cd* __restrict__ W, const Cd* __restrict__ scale, int M,
                                                                 int F, size_t total) {
  const size_t i = (size_t)blockIdx.x * BLK + threadIdx.x;
  if (i >= total) return;
  const int n = (int)(i / M % M);
  const size_t f = i / ((size_t)M * M);
  W[i] = cmul(W[i], scale[(size_t)n * F + f]);
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
int id_check(assx_ctx* ctx, const char* who, int M, int F, int T) {
  ASSX_REQUIRE_CTX(ctx);
  ASSX_REQUIRE(ctx, F >= 1 && T >= 1, ASSX_E_ARG, "%s: invalid sizes F=%d T=%d", who, F, T);
  ASSX_REQUIRE(ctx, M >= 2 && M <= 8, ASSX_E_UNSUPPORTED, "%s: n_channels must be in [2, 8], got %d", who, M);
  ASSX_REQUIRE(ctx, T >= M, ASSX_E_UNSUPPORTED, "%s: n_frames must be at least n_channels (%d), got %d", who, M, T);
  ASSX_REQUIRE(ctx, id_in_envelope(M, F, T), ASSX_E_UNSUPPORTED,
               "%s: one utterance must stay below 4 GiB in complex128 (M*F*T < 2^28)", who);
  return 0;
}

int id_check_domain(assx_ctx* ctx, const char* who, double domain) {
  ASSX_REQUIRE(ctx, domain >= 1.0 && domain <= 2.0, ASSX_E_ARG, "%s: domain must be in [1, 2], got %g", who, domain);
  return 0;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the pass over X: the loss of (W, R) into loss[0] when loss != NULL, the network's input when inp != NULL
int id_tail(assx_ctx* ctx, const void* X, const void* W, const double* R, double domain, float* inp, double* loss,
            double* part, double* ldet, int M, int F, int T, hipStream_t st) {
  const int CH = id_chunks(T);
  const int vec = inp && T % ID_VEC == 0 && aligned16(inp) ? 1 : 0;
  const PowSpec ps = make_pow(domain / 2.0);
  return dispatch_channels(ctx, "assx_idlma", M, [&](auto mt) -> int {
    constexpr int MC = decltype(mt)::value;
    const dim3 grid((unsigned)F * CH), blk(BLK);
    if (loss && inp)
      hipLaunchKernelGGL((idlma_tail_kernel<MC, true, true>), grid, blk, 0, st, (const Cd*)X, (const Cd*)W, R, inp, part, ps,
                         F, T, CH, vec);
    else if (loss)
      hipLaunchKernelGGL((idlma_tail_kernel<MC, true, false>), grid, blk, 0, st, (const Cd*)X, (const Cd*)W, R, inp, part,
                         ps, F, T, CH, vec);
    else
      hipLaunchKernelGGL((idlma_tail_kernel<MC, false, true>), grid, blk, 0, st, (const Cd*)X, (const Cd*)W, R, inp, part,
                         ps, F, T, CH, vec);
    ASSX_LAUNCH_CHECK(ctx, "idlma_tail_kernel");
    if (loss) {
      hipLaunchKernelGGL((idlma_logdet_kernel<MC>), dim3(nblocks(F, WAVE)), dim3(WAVE), 0, st, (const Cd*)W, ldet, F);
      ASSX_LAUNCH_CHECK(ctx, "idlma_logdet_kernel");
      hipLaunchKernelGGL(idlma_loss_close_kernel, dim3(1), blk, 0, st, (const double*)part, F * CH, (const double*)ldet, F,
                         T, loss);
      ASSX_LAUNCH_CHECK(ctx, "idlma_loss_close_kernel");
    }
    return 0;
  });
}

int id_variance(assx_ctx* ctx, const float* src, int raw, double domain, double dnn_flooring, double eps,
                float* dnn_output, double* R, int M, int F, int T, hipStream_t st) {
  const size_t total = (size_t)M * F * T;
  const int vec = aligned16(src) && aligned16(dnn_output) && aligned16(R) ? 1 : 0;
  hipLaunchKernelGGL(idlma_variance_kernel, dim3(nblocks(nblocks(total, ID_VEC), BLK)), dim3(BLK), 0, st, src, dnn_output, R,
                     make_powf(2.0 / domain), raw, dnn_flooring != 0.0 ? 1 : 0, (float)dnn_flooring, (float)eps, total, vec);
  ASSX_LAUNCH_CHECK(ctx, "idlma_variance_kernel");
  return 0;
}

int id_normalize_pb(assx_ctx* ctx, void* W, const void* scale, int M, int F, hipStream_t st) {
  const size_t total = (size_t)F * M * M;
  hipLaunchKernelGGL(idlma_normalize_pb_kernel, dim3(nblocks(total, BLK)), dim3(BLK), 0, st, (Cd*)W, (const Cd*)scale, M, F,
                     total);
  ASSX_LAUNCH_CHECK(ctx, "idlma_normalize_pb_kernel");
  return 0;
}

}  // namespace

extern "C" {

size_t assx_idlma_workspace_bytes(int M, int F, int T) {
  if (!id_in_envelope(M, F, T)) return 0;
  return id_layout(M, F, T).total;
}

int assx_idlma_dnn_input(assx_ctx* ctx, const void* X, const void* W, double domain, float* input, int M, int F, int T,
                         void* stream) {
  int rc = id_check(ctx, "assx_idlma_dnn_input", M, F, T);
  if (rc) return rc;
  if ((rc = id_check_domain(ctx, "assx_idlma_dnn_input", domain))) return rc;
  ASSX_REQUIRE(ctx, X && W && input, ASSX_E_NULL, "assx_idlma_dnn_input: NULL array");
  return id_tail(ctx, X, W, nullptr, domain, input, nullptr, nullptr, nullptr, M, F, T, (hipStream_t)stream);
}

int assx_idlma_variance(assx_ctx* ctx, const float* network_output, double domain, double dnn_flooring, double eps,
                        float* dnn_output, double* R, int M, int F, int T, void* stream) {
  int rc = id_check(ctx, "assx_idlma_variance", M, F, T);
  if (rc) return rc;
  if ((rc = id_check_domain(ctx, "assx_idlma_variance", domain))) return rc;
  ASSX_REQUIRE(ctx, dnn_output && R, ASSX_E_NULL, "assx_idlma_variance: NULL array");
  return id_variance(ctx, network_output ? network_output : dnn_output, network_output ? 1 : 0, domain, dnn_flooring, eps,
                     dnn_output, R, M, F, T, (hipStream_t)stream);
}

int assx_idlma_normalize_pb(assx_ctx* ctx, void* W, const void* scale, int M, int F, void* stream) {
  int rc = id_check(ctx, "assx_idlma_normalize_pb", M, F, M);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, W && scale, ASSX_E_NULL, "assx_idlma_normalize_pb: NULL array");
  return id_normalize_pb(ctx, W, scale, M, F, (hipStream_t)stream);
}

int assx_idlma_loss(assx_ctx* ctx, const void* X, const void* W, const double* R, double* loss, void* ws, int M, int F,
                    int T, void* stream) {
  int rc = id_check(ctx, "assx_idlma_loss", M, F, T);
  if (rc) return rc;
  ASSX_REQUIRE(ctx, X && W && R && loss && ws, ASSX_E_NULL, "assx_idlma_loss: NULL array");
  const IdLayout L = id_layout(M, F, T);
  char* base = (char*)ws;
  return id_tail(ctx, X, W, R, 2.0, nullptr, loss, (double*)(base + L.part), (double*)(base + L.ldet), M, F, T,
                 (hipStream_t)stream);
}

int assx_idlma_step(assx_ctx* ctx, const void* X, void* W, const float* network_output, double domain, double dnn_flooring,
                    double eps, double threshold, int ref, float* dnn_output, double* loss, float* next_input,
                    int32_t* status, void* ws, int M, int F, int T, void* stream) {
  int rc = id_check(ctx, "assx_idlma_step", M, F, T);
  if (rc) return rc;
  if ((rc = id_check_domain(ctx, "assx_idlma_step", domain))) return rc;
  ASSX_REQUIRE(ctx, ref >= 0 && ref < M, ASSX_E_ARG, "reference_id must be in [0, %d), got %d", M, ref);
  ASSX_REQUIRE(ctx, X && W && dnn_output && ws, ASSX_E_NULL, "assx_idlma_step: NULL array");
  hipStream_t st = (hipStream_t)stream;
  const IdLayout L = id_layout(M, F, T);
  char* base = (char*)ws;
  double* R = (double*)(base + L.R);
  void* scale = base + L.scale;
  void* inner = base + L.inner;
  if ((rc = id_variance(ctx, network_output ? network_output : dnn_output, network_output ? 1 : 0, domain, dnn_flooring,
                        eps, dnn_output, R, M, F, T, st)))
    return rc;
  // R is floored at (float)eps already: with that very number as the floor the spatial update changes nothing in it
  if ((rc = assx_idlma_space_update(ctx, X, W, R, 2.0, (double)(float)eps, threshold, nullptr, status, inner, 1, M, F, T,
                                    ASSX_F64, stream)))
    return rc;
  if ((rc = assx_projection_back_scale(ctx, X, W, ref, scale, status, inner, 1, M, F, T, ASSX_F64, stream))) return rc;
  if ((rc = id_normalize_pb(ctx, W, scale, M, F, st))) return rc;
  if (!loss && !next_input) return 0;
  return id_tail(ctx, X, W, R, domain, next_input, loss, (double*)(base + L.part), (double*)(base + L.ldet), M, F, T, st);
}

}  // extern "C"
