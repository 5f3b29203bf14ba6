// Elementwise / reduction CDNA4 kernels: GELU (tanh) fwd+bwd, column-sum.
//
// The reference leaves GELU to torch autograd (/root/reference/example/
// model.py:94) and the linear bias grad to dY.sum(0) (ops/linear.py:70-75);
// here both are single-pass HBM-bound kernels (bf16x8 vectorized loads,
// Guideline 13; grid-stride with a capped grid, Guideline 11).
#include "common.h"
#include "launchers.h"

namespace tdsa {

constexpr float GC0 = 0.7978845608028654f;  // sqrt(2/pi)
constexpr float GC1 = 0.044715f;
constexpr float TWO_LOG2E = 2.8853900817779268f;  // 2*log2(e)

// tanh via raw v_exp/v_rcp: tanh(t) = 1 - 2/(exp(2t)+1). Saturates cleanly
// (exp2(+inf)=inf -> 1, exp2(-inf)=0 -> -1); ~2-3 ulp, inside bf16/fp32
// tolerance for GELU. libm tanhf is a long polynomial/branch chain and made
// the elementwise kernels VALU-bound.
DEV_INLINE float fast_tanh(float t) {
  float e = __builtin_amdgcn_exp2f(TWO_LOG2E * t);
  return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

DEV_INLINE float gelu_f(float x) {
  return 0.5f * x * (1.0f + fast_tanh(GC0 * (x + GC1 * x * x * x)));
}
DEV_INLINE float gelu_df(float x) {
  float t = fast_tanh(GC0 * (x + GC1 * x * x * x));
  float dt = (1.0f - t * t) * GC0 * (1.0f + 3.0f * GC1 * x * x);
  return 0.5f * (1.0f + t) + 0.5f * x * dt;
}

// One 16-byte vector per thread and step; the n % W elements past the last
// whole vector go one each to the first threads of the grid, in the same
// launch (training's sizes have none).
template <typename T>
__global__ void gelu_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                long long n) {
  using VT = Vec<T>;
  constexpr int W = VT::W;
  const long long nvec = n / W;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = global_tid(); i < nvec; i += stride) {
    typename VT::V v = VT::load(x + i * W);
    typename VT::V o;
#pragma unroll
    for (int k = 0; k < W; ++k) VT::set(o, k, gelu_f(VT::get(v, k)));
    VT::store(y + i * W, o);
  }
  const long long t = nvec * W + global_tid();
  if (t < n) y[t] = (T)gelu_f((float)x[t]);
}

template <typename T>
__global__ void gelu_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                T* __restrict__ dx, long long n) {
  using VT = Vec<T>;
  constexpr int W = VT::W;
  const long long nvec = n / W;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = global_tid(); i < nvec; i += stride) {
    typename VT::V dv = VT::load(dy + i * W);
    typename VT::V xv = VT::load(x + i * W);
    typename VT::V o;
#pragma unroll
    for (int k = 0; k < W; ++k)
      VT::set(o, k, VT::get(dv, k) * gelu_df(VT::get(xv, k)));
    VT::store(dx + i * W, o);
  }
  const long long t = nvec * W + global_tid();
  if (t < n) dx[t] = (T)((float)dy[t] * gelu_df((float)x[t]));
}

// db[N] = sum over M rows of dy[M,N]. Row-chunked: grid.y blocks each reduce
// a chunk of rows for one 256-column slab, then one fp32 atomicAdd per
// (chunk, column) — per-block partials first, Guideline 12.
template <typename T>
__global__ void colsum_kernel(const T* __restrict__ dy, float* __restrict__ out32,
                              int M, int N, int rows_per_chunk) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= N) return;
  const int r0 = blockIdx.y * rows_per_chunk;
  const int r1 = min(M, r0 + rows_per_chunk);
  float acc = 0.f;
  for (int r = r0; r < r1; ++r) acc += (float)dy[(long long)r * N + c];
  atomicAdd(&out32[c], acc);
}

template <typename T>
__global__ void cast_from_f32(const float* __restrict__ in, T* __restrict__ out,
                              long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = global_tid(); i < n; i += stride) out[i] = (T)in[i];
}

}  // namespace tdsa

using namespace tdsa;

extern "C" {

hipError_t tdsa_gelu_fwd(const void* x, void* y, long long n, int is_bf16,
                         hipStream_t stream) {
  const int block = 256;
  dispatch_dtype(is_bf16, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(gelu_fwd_kernel<T>,
                       dim3(capped_grid(n / Vec<T>::W, block)), dim3(block), 0,
                       stream, (const T*)x, (T*)y, n);
  });
  return hipGetLastError();
}

hipError_t tdsa_gelu_bwd(const void* dy, const void* x, void* dx, long long n,
                         int is_bf16, hipStream_t stream) {
  const int block = 256;
  dispatch_dtype(is_bf16, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(gelu_bwd_kernel<T>,
                       dim3(capped_grid(n / Vec<T>::W, block)), dim3(block), 0,
                       stream, (const T*)dy, (const T*)x, (T*)dx, n);
  });
  return hipGetLastError();
}

// out32 must be zero-filled fp32[N]; out (same dtype as dy) receives the cast.
hipError_t tdsa_column_sum(const void* dy, float* out32, void* out, int M, int N,
                           int is_bf16, hipStream_t stream) {
  const int block = 256;
  // size row chunks so total blocks ~ fill the chip
  int chunks = 1;
  long long col_blocks = (N + block - 1) / block;
  while (col_blocks * chunks < 1024 && chunks * 128 < M) chunks *= 2;
  int rows_per_chunk = (M + chunks - 1) / chunks;
  dim3 grid(col_blocks, chunks);
  dispatch_dtype(is_bf16, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(colsum_kernel<T>, grid, dim3(block), 0, stream,
                       (const T*)dy, out32, M, N, rows_per_chunk);
    hipLaunchKernelGGL(cast_from_f32<T>, dim3(capped_grid(N, block)), dim3(block),
                       0, stream, out32, (T*)out, (long long)N);
  });
  return hipGetLastError();
}

}  // extern "C"
