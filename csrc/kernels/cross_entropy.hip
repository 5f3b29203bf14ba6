// Fused softmax cross-entropy CDNA4 kernels.
//
// The reference calls F.cross_entropy on (B*T, 50304) logits
// (/root/reference/example/model.py:156). Here the forward is ONE HBM pass
// per row: an online logsumexp (running max + rescaled sum, the same merge
// rule as flash attention) plus the picked-logit lookup; backward is one
// pass writing (softmax - onehot) * scale. fp32 accumulation throughout.
#include "common.h"
#include "launchers.h"

namespace tdsa {

// Scales a, b that bring two logsumexp states with maxima m, m2 to their
// common maximum, which replaces m (raw v_exp: exp(-inf) == 0, and the
// branchless form keeps both scales well-defined for m == m2 == -inf).
DEV_INLINE void lse_scales(float& m, float m2, float& a, float& b) {
  const float mn = fmaxf(m, m2);
  a = (m == -INFINITY) ? 0.f
      : __builtin_amdgcn_exp2f(1.4426950408889634f * (m - mn));
  b = (m2 == -INFINITY) ? 0.f
      : __builtin_amdgcn_exp2f(1.4426950408889634f * (m2 - mn));
  m = mn;
}

// merge two (m, s) logsumexp states: the incoming product is rounded, then
// one fma adds the scaled own sum. Written out because the compiler, left to
// contract s*a + s2*b itself, picks the product to round by the code around
// it; this is the form it had picked in all but one merge step (see
// lse_wave_merge).
DEV_INLINE void lse_merge(float& m, float& s, float m2, float s2) {
  float a, b;
  lse_scales(m, m2, a, b);
  s = fmaf(s, a, s2 * b);
}

// The same merge for the per-chunk loop, with both products rounded before
// the add. Left to the optimizer, whether s*a + s2*b becomes an FMA depends
// on the code around it, so lse would move in the last bit with an
// unrelated edit of the loop; here the form is fixed.
DEV_INLINE void lse_merge_chunk(float& m, float& s, float m2, float s2) {
#pragma clang fp contract(off)
  float a, b;
  lse_scales(m, m2, a, b);
  s = s * a + s2 * b;
}

// Merges the (m, s) states of a wave's 64 lanes; every lane ends with the
// result. Used on the threads of a wave and again on the per-wave results.
// ROUND_LAST: the last step rounds both products (lse_merge_chunk's form).
// That is how the step was compiled at the thread level before the forms
// were written out, and lse keeps those bits.
template <bool ROUND_LAST>
DEV_INLINE void lse_wave_merge(float& m, float& s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float m2 = __shfl_xor(m, off, WAVE);
    const float s2 = __shfl_xor(s, off, WAVE);
    if (ROUND_LAST && off == 1)
      lse_merge_chunk(m, s, m2, s2);
    else
      lse_merge(m, s, m2, s2);
  }
}

// One workgroup per row (grid-strided). Writes lse[row] and the row's loss
// row_loss[row] (fp32, 0 for ignored rows; the caller sums them in a fixed
// order) and atomically counts n_valid (int32, order-independent).
// Precondition, enforced by the launcher: V % W == 0, so a row is whole
// vectors and every row base is 16-byte aligned.
template <typename T, int W>
__global__ void ce_fwd_kernel(const T* __restrict__ logits,
                              const long long* __restrict__ targets,
                              float* __restrict__ lse, float* __restrict__ row_loss,
                              int* __restrict__ n_valid, long long R, int V,
                              long long ignore_index) {
  using RV = Vec<T, W>;
  __shared__ float sm[1024 / WAVE];
  __shared__ float ssum[1024 / WAVE];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  const int nw = blockDim.x / WAVE;
  // block-local count: one atomicAdd per BLOCK at the end (a per-row
  // atomicAdd on a single scalar serialized 32k blocks — measured 4x the
  // kernel's HBM floor)
  int valid_acc = 0;
  for (long long row = blockIdx.x; row < R; row += gridDim.x) {
    const T* lr = logits + row * V;
    float m = -INFINITY, s = 0.f;
    // per-CHUNK online merge: a per-element data-dependent branch diverges
    // and serializes; instead reduce the chunk max, sum exps against it,
    // and merge (m, s) once per chunk.
    for (int i = tid * W; i + W <= V; i += blockDim.x * W) {
      typename RV::V v = RV::load(lr + i);
      float cm = RV::get(v, 0);
#pragma unroll
      for (int k = 1; k < W; ++k) cm = fmaxf(cm, RV::get(v, k));
      // a chunk that is all -inf (masked vocabulary padding) must contribute
      // (-inf, 0): subtracting its own max would give -inf - -inf = NaN.
      // One select per chunk, on the subtrahend only: every element then
      // gives exp2(-inf) = 0, and any other chunk subtracts cm as before.
      const float sub = (cm == -INFINITY) ? 0.f : cm;
      float cs = 0.f;
#pragma unroll
      for (int k = 0; k < W; ++k)
        cs += __builtin_amdgcn_exp2f(1.4426950408889634f
                                     * (RV::get(v, k) - sub));
      lse_merge_chunk(m, s, cm, cs);
    }
    lse_wave_merge<true>(m, s);
    if (lane == 0) { sm[wid] = m; ssum[wid] = s; }
    __syncthreads();
    if (wid == 0) {
      float mm = (lane < nw) ? sm[lane] : -INFINITY;
      float ss2 = (lane < nw) ? ssum[lane] : 0.f;
      lse_wave_merge<false>(mm, ss2);
      if (lane == 0) {
        float l = mm + __logf(ss2);
        lse[row] = l;
        const long long t = targets[row];
        float row_l = 0.f;
        if (t != ignore_index) {
          row_l = l - (float)lr[t];
          valid_acc += 1;
        }
        row_loss[row] = row_l;
      }
    }
    __syncthreads();
  }
  if (tid == 0 && valid_acc > 0) atomicAdd(n_valid, valid_acc);
}

// dlogits = valid ? (exp(logit - lse) - onehot) * scale : 0
// Precondition, enforced by the launcher: V % W == 0 (see ce_fwd_kernel).
template <typename T, int W>
__global__ void ce_bwd_kernel(const T* __restrict__ logits,
                              const long long* __restrict__ targets,
                              const float* __restrict__ lse, T* __restrict__ dlogits,
                              long long R, int V, float scale,
                              long long ignore_index) {
  using RV = Vec<T, W>;
  for (long long row = blockIdx.x; row < R; row += gridDim.x) {
    const T* lr = logits + row * V;
    T* dr = dlogits + row * V;
    const long long t = targets[row];
    const bool valid = (t != ignore_index);
    const float l = lse[row];
    for (int i = threadIdx.x * W; i + W <= V; i += blockDim.x * W) {
      typename RV::V v = RV::load(lr + i);
      typename RV::V out;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        float g = 0.f;
        if (valid) {
          g = __expf(RV::get(v, k) - l);
          if ((long long)(i + k) == t) g -= 1.0f;
          g *= scale;
        }
        RV::set(out, k, g);
      }
      RV::store(dr + i, out);
    }
  }
}

// What both launchers share. The kernels take whole 16-byte vectors only
// and row bases logits + row * V must stay 16-byte aligned, so V % W != 0 is
// refused (as the layernorm launchers do; the python op routes such shapes
// to the composite). Otherwise calls launch(type tag, grid, block) with one
// workgroup per row up to the TDSA_CE_GRID cap.
template <typename Launch>
static hipError_t ce_launch(long long R, int V, int is_bf16, Launch launch) {
  if (V % (is_bf16 ? Vec<bf16>::W : Vec<float>::W)) return hipErrorInvalidValue;
  const long long cap = env_int("TDSA_CE_GRID", 32768);
  const int grid = (int)((R < cap) ? R : cap);
  dispatch_dtype(is_bf16, [&](auto tag) { launch(tag, dim3(grid), dim3(256)); });
  return hipGetLastError();
}

}  // namespace tdsa

using namespace tdsa;

extern "C" {

hipError_t tdsa_ce_fwd(const void* logits, const long long* targets, float* lse,
                       float* row_loss, int* n_valid, long long R, int V,
                       long long ignore_index, int is_bf16, hipStream_t stream) {
  return ce_launch(R, V, is_bf16, [&](auto tag, dim3 grid, dim3 block) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((ce_fwd_kernel<T, Vec<T>::W>), grid, block, 0, stream,
                       (const T*)logits, targets, lse, row_loss, n_valid, R, V,
                       ignore_index);
  });
}

hipError_t tdsa_ce_bwd(const void* logits, const long long* targets,
                       const float* lse, void* dlogits, long long R, int V,
                       float scale, long long ignore_index, int is_bf16,
                       hipStream_t stream) {
  return ce_launch(R, V, is_bf16, [&](auto tag, dim3 grid, dim3 block) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((ce_bwd_kernel<T, Vec<T>::W>), grid, block, 0, stream,
                       (const T*)logits, targets, lse, (T*)dlogits, R, V, scale,
                       ignore_index);
  });
}

}  // extern "C"
