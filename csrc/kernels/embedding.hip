// Embedding gather / scatter-add CDNA4 kernels.
//
// Parity with /root/reference/tiny_deepspeed/core/module/ops/embedding.py:
// forward = row gather (index_select :57), backward = scatter-add into the
// (vocab, E) table (:60-65). MI355X design: vectorized 16B-per-lane gather;
// backward sums each table row's contributions in fp32 in sorted-index order
// (no atomics: the result is the same from run to run).
#include "common.h"
#include "launchers.h"

namespace tdsa {

// Row gather, W elements per thread and step: the full 16-byte vector when
// D is a whole number of them, else W = 1 (the launcher picks).
template <typename T, int W>
__global__ void emb_fwd_kernel(const T* __restrict__ weight,
                               const long long* __restrict__ idx,
                               T* __restrict__ out, long long R, int D) {
  using VT = Vec<T, W>;
  const int chunks = D / W;
  const long long total = R * chunks;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = global_tid(); i < total; i += stride) {
    const long long r = i / chunks;
    const int c = (int)(i % chunks) * W;
    VT::store(out + r * (long long)D + c,
              VT::load(weight + idx[r] * (long long)D + c));
  }
}

// idx is sorted ascending and perm[j] is the dy row that sorted entry j came
// from (stable sort). The sorted list is cut into pieces at every change of
// index and at every multiple of EMB_PIECE, so no thread sums more than
// EMB_PIECE rows however often one index occurs. The thread at the start of
// a piece sums it in sorted order. A run of equal indices that is one piece
// is stored straight into dw32; otherwise the piece sum goes to part[start]
// and emb_bwd_join adds the run's pieces in order. Every sum has a fixed
// order, so the result does not depend on scheduling (an fp32 atomicAdd
// scatter summed rows hit three or more times in a different order from run
// to run).
constexpr int EMB_PIECE = 32;

template <typename T>
__global__ void emb_bwd_kernel(const T* __restrict__ dy,
                               const long long* __restrict__ idx,
                               const long long* __restrict__ perm,
                               float* __restrict__ dw32,
                               float* __restrict__ part, long long R, int D,
                               long long padding_idx) {
  const long long total = R * D;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = global_tid(); i < total; i += stride) {
    const long long r = i / D;
    const int c = (int)(i % D);
    const long long t = idx[r];
    if (t == padding_idx) continue;
    const bool head = r == 0 || idx[r - 1] != t;
    if (!head && r % EMB_PIECE != 0) continue;
    const long long end = (r / EMB_PIECE + 1) * EMB_PIECE;
    float acc = 0.f;
    long long k = r;
    for (; k < R && k < end && idx[k] == t; ++k)
      acc += (float)dy[perm[k] * (long long)D + c];
    if (head && (k == R || idx[k] != t))
      dw32[t * (long long)D + c] = acc;
    else
      part[r * (long long)D + c] = acc;
  }
}

// One thread per (piece boundary e = b * EMB_PIECE, column). Where a run of
// equal indices crosses e for the first time, add its pieces in order: the
// one from the run's head (within EMB_PIECE before e), then those starting
// at e, e + EMB_PIECE, ... while the run lasts.
__global__ void emb_bwd_join(const long long* __restrict__ idx,
                             const float* __restrict__ part,
                             float* __restrict__ dw32, long long R, int D,
                             long long padding_idx) {
  const long long nb = (R - 1) / EMB_PIECE;  // boundaries at e = 32 .. < R
  const long long total = nb * D;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = global_tid(); i < total; i += stride) {
    const long long e = (i / D + 1) * EMB_PIECE;
    const int c = (int)(i % D);
    const long long t = idx[e];
    if (t == padding_idx || idx[e - 1] != t) continue;
    long long h = e - 1;                       // run head, in [e - 32, e)
    while (h > e - EMB_PIECE && idx[h - 1] == t) --h;
    if (h == e - EMB_PIECE && h > 0 && idx[h - 1] == t)
      continue;                                // crossed an earlier boundary
    float acc = part[h * (long long)D + c];
    for (long long p = e; p < R && idx[p] == t; p += EMB_PIECE)
      acc += part[p * (long long)D + c];
    dw32[t * (long long)D + c] = acc;
  }
}

}  // namespace tdsa

using namespace tdsa;

extern "C" {

hipError_t tdsa_embedding_fwd(const void* weight, const long long* idx, void* out,
                              long long R, int D, int is_bf16, hipStream_t stream) {
  const int block = 256;
  dispatch_dtype(is_bf16, [&](auto tag) {
    using T = typename decltype(tag)::type;
    constexpr int W = Vec<T>::W;
    if (D % W == 0)
      hipLaunchKernelGGL((emb_fwd_kernel<T, W>),
                         dim3(capped_grid(R * (D / W), block)), dim3(block), 0,
                         stream, (const T*)weight, idx, (T*)out, R, D);
    else
      hipLaunchKernelGGL((emb_fwd_kernel<T, 1>),
                         dim3(capped_grid(R * D, block)), dim3(block), 0,
                         stream, (const T*)weight, idx, (T*)out, R, D);
  });
  return hipGetLastError();
}

// dw32 must be zero-filled fp32 [V, D]; padding_idx = -1 for "none". idx is
// the sorted index list and perm the source row of each sorted entry; part
// is an fp32 [R, D] scratch buffer (need not be initialised).
hipError_t tdsa_embedding_bwd(const void* dy, const long long* idx,
                              const long long* perm, float* dw32, float* part,
                              long long R, int D, long long padding_idx,
                              int is_bf16, hipStream_t stream) {
  const int block = 256;
  dispatch_dtype(is_bf16, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(emb_bwd_kernel<T>, dim3(capped_grid(R * D, block)),
                       dim3(block), 0, stream, (const T*)dy, idx, perm, dw32,
                       part, R, D, padding_idx);
  });
  if (R > EMB_PIECE)
    hipLaunchKernelGGL(emb_bwd_join,
                       dim3(capped_grid(((R - 1) / EMB_PIECE) * D, block)),
                       dim3(block), 0, stream, idx, part, dw32, R, D,
                       padding_idx);
  return hipGetLastError();
}

}  // extern "C"
