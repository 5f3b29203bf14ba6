// Multi-tensor sum of squares: the global gradient norm of a clipped
// optimizer step in one launch over every gradient (bf16 and fp32 mixed).
//
// Same blob as the optimizer launch (optim_desc.h): [GradNormDesc][ChunkRef],
// one workgroup per chunk of kOptimChunkElems elements, grid-stride over the
// chunks. A chunk's sum depends on the chunk alone: each lane squares a fixed
// set of elements into four fp32 accumulators, the workgroup adds its lanes
// in block_sum's fixed order and stores one partial at partials[cid]. A
// second kernel of one workgroup adds the partials in fp64, again in an order
// fixed by nchunks. No atomics: neither the grid size nor which workgroup
// took which chunk can change a bit of the result.
#include "common.h"
#include "launchers.h"
#include "optim_desc.h"

#include <cstdint>

namespace tdsa {

constexpr int kNormThreads = 256;
constexpr int kNormUnroll = 4;  // independent 16-byte loads per lane

template <typename T>
DEV_INLINE float square_of(T x) {
  const float f = (float)x;
  return f * f;
}

// Sum of squares of g[0, n) over the workgroup's lanes (not yet reduced).
// g need not be 16-byte aligned (a view at an odd element offset): up to
// 16/sizeof(T) - 1 head elements are taken one per lane, the vector body
// starts at the next 16-byte boundary, and the ragged end gets a scalar tail.
template <typename T>
DEV_INLINE float chunk_sumsq(const T* g, long long n) {
  typedef Vec<T> VT;
  constexpr int W = VT::W;
  const int tid = threadIdx.x;
  long long head = ((16 - ((uintptr_t)g & 15)) & 15) / sizeof(T);
  if (head > n) head = n;
  float acc[kNormUnroll] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (tid < head) acc[0] += square_of(g[tid]);
  const T* body = g + head;
  const long long nv = (n - head) / W;
  long long q = tid;
  for (; q + (kNormUnroll - 1) * kNormThreads < nv;
       q += kNormUnroll * kNormThreads) {
    typename VT::V v[kNormUnroll];
#pragma unroll
    for (int u = 0; u < kNormUnroll; ++u)
      v[u] = VT::load(body + (q + u * kNormThreads) * W);
#pragma unroll
    for (int u = 0; u < kNormUnroll; ++u)
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const float f = VT::get(v[u], k);
        acc[u] = fmaf(f, f, acc[u]);
      }
  }
  for (; q < nv; q += kNormThreads) {
    const typename VT::V v = VT::load(body + q * W);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float f = VT::get(v, k);
      acc[0] = fmaf(f, f, acc[0]);
    }
  }
  for (long long i = head + nv * W + tid; i < n; i += kNormThreads)
    acc[1] += square_of(g[i]);
  return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

__global__ void __launch_bounds__(kNormThreads)
grad_sumsq_kernel(const GradNormDesc* __restrict__ descs,
                  const ChunkRef* __restrict__ chunks, int nchunks,
                  int chunk_elems, float* __restrict__ partials) {
  __shared__ float scratch[kNormThreads / WAVE];
  for (int cid = blockIdx.x; cid < nchunks; cid += gridDim.x) {
    const ChunkRef ch = chunks[cid];
    const GradNormDesc d = descs[ch.tensor];
    const long long start = (long long)ch.chunk * chunk_elems;
    const long long n = min(d.numel - start, (long long)chunk_elems);
    float s = d.bf16 ? chunk_sumsq((const bf16*)d.g + start, n)
                     : chunk_sumsq((const float*)d.g + start, n);
    s = block_sum(s, scratch);
    if (threadIdx.x == 0) partials[cid] = s;
  }
}

// One workgroup: lane t adds partials[t], [t + 256], ... in fp64, the lanes
// are added by xor-shuffles and the four waves in wave order.
__global__ void __launch_bounds__(kNormThreads)
grad_sumsq_finalize_kernel(const float* __restrict__ partials, int nchunks,
                           float* __restrict__ out) {
  __shared__ double wsum[kNormThreads / WAVE];
  double s = 0.0;
  for (int i = threadIdx.x; i < nchunks; i += kNormThreads)
    s += (double)partials[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = wsum[0];
    for (int w = 1; w < kNormThreads / WAVE; ++w) r += wsum[w];
    *out = (float)r;
  }
}

}  // namespace tdsa

using namespace tdsa;

extern "C" {

hipError_t tdsa_grad_sumsq_multi(const void* blob, int ndescs, int nchunks,
                                 float* partials, float* out,
                                 hipStream_t stream) {
  const GradNormDesc* descs = (const GradNormDesc*)blob;
  const ChunkRef* chunks = (const ChunkRef*)(descs + ndescs);
  if (nchunks > 0) {
    const int grid = nchunks < 2048 ? nchunks : 2048;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(kNormThreads), 0,
                       stream, descs, chunks, nchunks, kOptimChunkElems,
                       partials);
    HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(grad_sumsq_finalize_kernel, dim3(1), dim3(kNormThreads),
                     0, stream, partials, nchunks, out);
  return hipGetLastError();
}

}  // extern "C"
