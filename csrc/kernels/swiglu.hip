// SwiGLU on the packed gate/up projection: y = silu(gate) * up, fwd + bwd.
//
// gu is contiguous (M, 2F): gate = gu[:, :F], up = gu[:, F:], the two halves
// of one c_fc GEMM. The forward writes y (M, F); the backward reads dy (M, F)
// and gu again (nothing else is saved) and writes both halves of the packed
// dgu (M, 2F) in one pass, so dX and dW of c_fc stay one GEMM each.
//
// Work split. The index is two-dimensional (a row, and a column that is read
// at two places F apart), so there is no flat grid-stride loop: a thread owns
// vector (row, cv) of the vpr = F / W vectors of a row and walks the (M, vpr)
// grid by the launch's thread count. The launcher passes that count already
// split as dr = nthreads / vpr and dc = nthreads % vpr; a step is two adds
// and one conditional carry, and the only division is the one that places
// the thread at its start. row and cv are 32-bit (unsigned, so the step past
// the last row cannot wrap); element offsets are 64-bit, row * 2F passes 2^31
// at training sizes.
//
// Per step a thread issues every load of its kSwigluDepth vectors (2 each
// forward, 3 backward) before the first arithmetic instruction. No LDS, no
// atomics: a pure stream, 6F bytes per row forward and 10F backward in bf16.
#include "common.h"
#include "launchers.h"

#include <type_traits>

namespace tdsa {

constexpr float LOG2E = 1.4426950408889634f;

// sigmoid via raw v_exp/v_rcp: 1 / (1 + exp2(-g * log2e)). Saturates cleanly:
// exp2 overflows to inf for g < -88 and rcp(inf) = 0; exp2 underflows to 0 for
// large g and rcp(1) = 1. libm expf and an IEEE divide would make the stream
// VALU-bound.
DEV_INLINE float fast_sigmoid(float g) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E * g));
}

// Independent vectors a thread has in flight per step: its own (row, cv) and
// the one a grid stride further on. Measured at (32768, 2816 / 4096) bf16
// against depth 1: forward level to 4 % faster, backward level to 5 % faster
// (docs/kernels.md).
constexpr int kSwigluDepth = 2;

// A thread's position in the (M, vpr) grid of vectors, its step, and the
// element offsets of where it stands: of y/dy (M, F) and of the gate vector
// in gu/dgu (M, 2F), whose up vector lies F further on.
struct SwigluWalk {
  unsigned row, cv;
  DEV_INLINE SwigluWalk(unsigned vpr) {
    const unsigned tid = (unsigned)global_tid();
    row = tid / vpr;
    cv = tid - row * vpr;
  }
  DEV_INLINE void step(unsigned vpr, unsigned dr, unsigned dc) {
    row += dr;
    cv += dc;
    if (cv >= vpr) {
      cv -= vpr;
      ++row;
    }
  }
  DEV_INLINE long long y_offset(unsigned F, int W) const {
    return (long long)row * F + (long long)cv * W;
  }
  DEV_INLINE long long gate_offset(unsigned F, int W) const {
    return (long long)row * F * 2 + (long long)cv * W;
  }
};

template <typename T, int W>
__global__ void swiglu_fwd_kernel(const T* __restrict__ gu, T* __restrict__ y,
                                  unsigned M, unsigned F, unsigned vpr,
                                  unsigned dr, unsigned dc) {
  using VT = Vec<T, W>;
  typedef typename VT::V V;
  SwigluWalk at(vpr);
  while (at.row < M) {
    bool live[kSwigluDepth];
    long long oy[kSwigluDepth];
    V g[kSwigluDepth], u[kSwigluDepth];
#pragma unroll
    for (int d = 0; d < kSwigluDepth; ++d) {
      live[d] = at.row < M;
      oy[d] = at.y_offset(F, W);
      if (live[d]) {
        const T* p = gu + at.gate_offset(F, W);
        g[d] = VT::load(p);
        u[d] = VT::load(p + F);
      }
      at.step(vpr, dr, dc);
    }
#pragma unroll
    for (int d = 0; d < kSwigluDepth; ++d) {
      if (!live[d]) continue;
      V o;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const float gk = VT::get(g[d], k);
        VT::set(o, k, gk * fast_sigmoid(gk) * VT::get(u[d], k));
      }
      VT::store(y + oy[d], o);
    }
  }
}

// s = sigmoid(g): dup = dy * g * s, dgate = dy * u * s * (1 + g * (1 - s)).
template <typename T, int W>
__global__ void swiglu_bwd_kernel(const T* __restrict__ dy,
                                  const T* __restrict__ gu,
                                  T* __restrict__ dgu, unsigned M, unsigned F,
                                  unsigned vpr, unsigned dr, unsigned dc) {
  using VT = Vec<T, W>;
  typedef typename VT::V V;
  SwigluWalk at(vpr);
  while (at.row < M) {
    bool live[kSwigluDepth];
    long long og[kSwigluDepth];
    V g[kSwigluDepth], u[kSwigluDepth], dv[kSwigluDepth];
#pragma unroll
    for (int d = 0; d < kSwigluDepth; ++d) {
      live[d] = at.row < M;
      og[d] = at.gate_offset(F, W);
      if (live[d]) {
        dv[d] = VT::load(dy + at.y_offset(F, W));
        g[d] = VT::load(gu + og[d]);
        u[d] = VT::load(gu + og[d] + F);
      }
      at.step(vpr, dr, dc);
    }
#pragma unroll
    for (int d = 0; d < kSwigluDepth; ++d) {
      if (!live[d]) continue;
      V dgate, dup;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const float gk = VT::get(g[d], k);
        const float s = fast_sigmoid(gk);
        const float ds = VT::get(dv[d], k) * s;
        VT::set(dup, k, ds * gk);
        VT::set(dgate, k, ds * VT::get(u[d], k) * (1.0f + gk * (1.0f - s)));
      }
      VT::store(dgu + og[d], dgate);
      VT::store(dgu + og[d] + F, dup);
    }
  }
}

// Launch geometry of an (M, F) problem at vector width W: a persistent grid
// of 256-thread blocks under the TDSA_SWIGLU_GRID cap (read per launch;
// default 1024, four blocks per CU: 3-8 % ahead of capped_grid's 2048 at
// training sizes), and its thread count split by vpr.
struct SwigluGeom {
  unsigned grid, vpr, dr, dc;
};
inline SwigluGeom swiglu_geom(int M, int F, int W) {
  const int block = 256;
  SwigluGeom g;
  g.vpr = (unsigned)(F / W);
  long long cap = env_int("TDSA_SWIGLU_GRID", 1024);
  cap = cap < 1 ? 1 : (cap > 65535 ? 65535 : cap);
  long long blocks = ((long long)M * g.vpr + block - 1) / block;
  g.grid = (unsigned)(blocks < cap ? blocks : cap);
  const unsigned nthreads = g.grid * block;
  g.dr = nthreads / g.vpr;
  g.dc = nthreads % g.vpr;
  return g;
}

// Calls f with the width as a type: the 16-byte vector where it divides F
// (both halves of every row then start on a 16-byte boundary), else 1.
template <typename T, typename Fn>
inline void swiglu_width(int F, Fn f) {
  if (F % kVecWidth<T> == 0)
    f(std::integral_constant<int, kVecWidth<T>>{});
  else
    f(std::integral_constant<int, 1>{});
}

}  // namespace tdsa

using namespace tdsa;

extern "C" {

hipError_t tdsa_swiglu_fwd(const void* gu, void* y, int M, int F, int is_bf16,
                           hipStream_t stream) {
  if (M < 1 || F < 1) return hipErrorInvalidValue;
  dispatch_dtype(is_bf16, [&](auto tag) {
    using T = typename decltype(tag)::type;
    swiglu_width<T>(F, [&](auto width) {
      constexpr int W = decltype(width)::value;
      const SwigluGeom g = swiglu_geom(M, F, W);
      hipLaunchKernelGGL((swiglu_fwd_kernel<T, W>), dim3(g.grid), dim3(256), 0,
                         stream, (const T*)gu, (T*)y, (unsigned)M, (unsigned)F,
                         g.vpr, g.dr, g.dc);
    });
  });
  return hipGetLastError();
}

hipError_t tdsa_swiglu_bwd(const void* dy, const void* gu, void* dgu, int M,
                           int F, int is_bf16, hipStream_t stream) {
  if (M < 1 || F < 1) return hipErrorInvalidValue;
  dispatch_dtype(is_bf16, [&](auto tag) {
    using T = typename decltype(tag)::type;
    swiglu_width<T>(F, [&](auto width) {
      constexpr int W = decltype(width)::value;
      const SwigluGeom g = swiglu_geom(M, F, W);
      hipLaunchKernelGGL((swiglu_bwd_kernel<T, W>), dim3(g.grid), dim3(256), 0,
                         stream, (const T*)dy, (const T*)gu, (T*)dgu,
                         (unsigned)M, (unsigned)F, g.vpr, g.dr, g.dc);
    });
  });
  return hipGetLastError();
}

}  // extern "C"
