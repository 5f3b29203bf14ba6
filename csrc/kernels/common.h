// Common device helpers for the tiny_deepspeed_amd CDNA4 (gfx950) kernels.
//
// MI355X facts used throughout (see /opt/skills/guides/MI355X_MICROARCH.md):
//   wavefront = 64 lanes; 256 CUs in 8 XCDs; 160 KiB LDS/CU; HBM3E ~8 TB/s.
// All kernels accumulate in fp32 (acc-dtype policy of SURVEY.md 2.10D) and
// vectorize bf16 global traffic as short4/short8 reinterprets (Guideline 13).
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include <cstdlib>

#define WAVE 64
#define DEV_INLINE __device__ __forceinline__

typedef __hip_bfloat16 bf16;

// ---- vector types ---------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) short short4v;
typedef __attribute__((ext_vector_type(8))) short short8v;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

DEV_INLINE float bf2f(bf16 x) { return __bfloat162float(x); }
DEV_INLINE bf16 f2bf(float x) { return __float2bfloat16(x); }

// Load/store 8 bf16 (16 B) per lane — the coalescing sweet spot.
DEV_INLINE short8v load8(const bf16* p) {
  return *reinterpret_cast<const short8v*>(p);
}
DEV_INLINE void store8(bf16* p, short8v v) {
  *reinterpret_cast<short8v*>(p) = v;
}
template <typename V>  // short4v or short8v
DEV_INLINE float bf_elem(V v, int i) {
  union { short s; bf16 b; } u; u.s = v[i]; return bf2f(u.b);
}
DEV_INLINE short bf_pack(float x) {
  union { short s; bf16 b; } u; u.b = f2bf(x); return u.s;
}

// ---- Vec<T, W>: W elements of T moved as one access, read/written as fp32 ---
// The default width is 16 bytes per lane (4 float, 8 bf16); bf16 also comes
// 4 wide (8 bytes, next to an fp32 vector of 4), and W = 1 is the plain
// element, so a scalar path instantiates the same template as a vector one.
template <typename T> constexpr int kVecWidth = 16 / sizeof(T);
template <typename T, int W_ = kVecWidth<T>> struct Vec;
template <> struct Vec<float, 4> {
  static constexpr int W = 4;
  typedef f32x4 V;
  static DEV_INLINE V load(const float* p) { return *reinterpret_cast<const V*>(p); }
  static DEV_INLINE void store(float* p, V v) { *reinterpret_cast<V*>(p) = v; }
  static DEV_INLINE float get(V v, int i) { return v[i]; }
  static DEV_INLINE void set(V& v, int i, float x) { v[i] = x; }
};
template <int W_> struct BfVec {  // bf16 x 4 or 8, carried as shorts
  static constexpr int W = W_;
  typedef __attribute__((ext_vector_type(W_))) short V;
  static DEV_INLINE V load(const bf16* p) { return *reinterpret_cast<const V*>(p); }
  static DEV_INLINE void store(bf16* p, V v) { *reinterpret_cast<V*>(p) = v; }
  static DEV_INLINE float get(V v, int i) { return bf_elem(v, i); }
  static DEV_INLINE void set(V& v, int i, float x) { v[i] = bf_pack(x); }
};
template <> struct Vec<bf16, 8> : BfVec<8> {};
template <> struct Vec<bf16, 4> : BfVec<4> {};
template <typename T> struct Vec<T, 1> {
  static constexpr int W = 1;
  typedef T V;
  static DEV_INLINE V load(const T* p) { return *p; }
  static DEV_INLINE void store(T* p, V v) { *p = v; }
  static DEV_INLINE float get(V v, int) { return (float)v; }
  static DEV_INLINE void set(V& v, int, float x) { v = (T)x; }
};

// ---- wave reductions ------------------------------------------------------
DEV_INLINE float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}
DEV_INLINE float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, WAVE));
  return v;
}

// Block-level reductions through LDS (blockDim.x threads, <=1024).
// `scratch` must hold blockDim.x/WAVE floats.
DEV_INLINE float block_sum(float v, float* scratch) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int nw = blockDim.x / WAVE;
  v = wave_sum(v);
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  float r = (lane < nw) ? scratch[lane] : 0.0f;
  r = wave_sum(r);
  // every wave now computed the same value in lane set; broadcast via lane 0
  r = __shfl(r, 0, WAVE);
  __syncthreads();
  return r;
}
// Paired reduction: one barrier round for two sums (layernorm's sum/sumsq
// and c1/c2 pairs — halves the barrier count of two block_sum calls).
DEV_INLINE void block_sum2(float& a, float& b, float* scratch) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int nw = blockDim.x / WAVE;
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane == 0) {
    scratch[wid] = a;
    scratch[nw + wid] = b;
  }
  __syncthreads();
  float ra = (lane < nw) ? scratch[lane] : 0.0f;
  float rb = (lane < nw) ? scratch[nw + lane] : 0.0f;
  ra = wave_sum(ra);
  rb = wave_sum(rb);
  a = __shfl(ra, 0, WAVE);
  b = __shfl(rb, 0, WAVE);
  __syncthreads();
}

DEV_INLINE float block_max(float v, float* scratch) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  const int nw = blockDim.x / WAVE;
  v = wave_max(v);
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  float r = (lane < nw) ? scratch[lane] : -INFINITY;
  r = wave_max(r);
  r = __shfl(r, 0, WAVE);
  __syncthreads();
  return r;
}

#define HIP_CHECK(cmd)                                                     \
  do {                                                                     \
    hipError_t e_ = (cmd);                                                 \
    if (e_ != hipSuccess) {                                                \
      return e_;                                                           \
    }                                                                      \
  } while (0)

// Integer launch knob from the environment: `dflt` when unset, otherwise
// atoll() of the value, whatever it holds.
inline long long env_int(const char* name, long long dflt) {
  const char* v = getenv(name);
  return v ? atoll(v) : dflt;
}

// A launcher's is_bf16 flag becomes a type: calls f with TypeTag<bf16> or
// TypeTag<float> and returns what f returns.
//   dispatch_dtype(is_bf16, [&](auto tag) {
//     using T = typename decltype(tag)::type; ... kernel<T> ... });
template <typename T> struct TypeTag { typedef T type; };
template <typename F>
inline auto dispatch_dtype(int is_bf16, F f) {
  if (is_bf16) return f(TypeTag<bf16>{});
  return f(TypeTag<float>{});
}

DEV_INLINE int global_tid() { return blockIdx.x * blockDim.x + threadIdx.x; }
DEV_INLINE int global_nthreads() { return gridDim.x * blockDim.x; }

// Grid sizing for memory-bound grid-stride kernels (Guideline 11):
// cap at ~8 blocks per CU and stride the rest.
inline int capped_grid(long long work, int block) {
  long long g = (work + block - 1) / block;
  const long long cap = 2048;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return static_cast<int>(g);
}
