// RMSNorm forward / backward CDNA4 kernels (last dim, weight only, bf16
// storage, fp32 arithmetic), with the residual add fused as in layernorm.hip.
//
//   forward : h = x (+ res, rounded to bf16 once and stored);
//             rstd = rsqrt(mean(h^2) + eps);  y = h * rstd * w
//   backward: g = w * dy;  c = mean(g * h) * rstd^2;
//             dx = (g - h * c) * rstd (+ dh);  dw = sum_rows dy * h * rstd
//
// Each direction has ONE row reduction (LayerNorm has two) and there is no
// mean and no bias: one fp32 per row saved, one stripe buffer for dw. The
// single reduction is what makes a row spread over a whole workgroup viable
// (SPAN = 4): the cross-wave exchange of a batch of R rows costs one barrier,
// not two per row.
#include "common.h"
#include "launchers.h"

#include <type_traits>

namespace tdsa {

#define RMS_BLOCK 256
#define RMS_WAVES (RMS_BLOCK / WAVE)
#define RMS_MAXVEC 4
// Batch depths: rows whose loads are in flight per unit. Bounded by
// registers: the forward holds R * NVEC vectors of x (and as many of res
// until h is formed), the backward 2 * R * NVEC plus NVEC * 8 fp32 dw
// accumulators (docs/kernels.md "RMSNorm" has the counts).
#define RMS_FWD_DEPTH(NVEC) ((NVEC) <= 2 ? 4 : 2)
#define RMS_BWD_DEPTH(NVEC) 2

// No packed fp32 math: the results do not depend on how the compiler pairs
// the elements of a vector (as in the dropout LayerNorm kernels).
#if defined(__HIP_DEVICE_COMPILE__)
#define RMS_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define RMS_NO_PK_F32
#endif

// ---- the two spans ------------------------------------------------------------
// A "unit" owns whole rows: unit u of the U units of the persistent grid
// takes rows u, u+U, ... and works on them in batches of R (rows u + r*U).
//   SPAN = 1: a unit is a wave (four units per workgroup). Lane l holds
//             vectors l, l+64, ... of the row; the row sum is a wave_sum.
//   SPAN = 4: a unit is the workgroup. Thread t holds vectors t, t+256, ...;
//             every wave reduces its part with wave_sum and the four partial
//             sums of each of the batch's R rows meet in LDS under one
//             barrier per batch.
// In both, a thread holds NVEC <= 4 16-byte vectors of a row, only the last
// one predicated, and every global load of a batch is issued before the
// batch's reduction.
//
// LDS exchange: batch b uses slot b & 1 of red[2][R][4]. A wave writes slot s
// for batch b+2 only after the barrier of batch b+1, which no wave passes
// before it has read slot s of batch b: two slots, one barrier per batch.
// The partials are combined as (p0 + p1) + (p2 + p3) by every thread, so all
// four waves hold the same bits.
template <int R, int SPAN>
DEV_INLINE void rms_exchange(float (&p)[R], float* red, int& slot, int lane,
                             int wave) {
  if constexpr (SPAN > 1) {
    float* s = red + slot * (R * RMS_WAVES);
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) s[r * RMS_WAVES + wave] = p[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r)
      p[r] = (s[r * RMS_WAVES + 0] + s[r * RMS_WAVES + 1]) +
             (s[r * RMS_WAVES + 2] + s[r * RMS_WAVES + 3]);
    slot ^= 1;
  }
}

template <bool HAS_RES, int NVEC, int R, int SPAN>
__global__ __launch_bounds__(RMS_BLOCK) RMS_NO_PK_F32 void rms_fwd_kernel(
    const bf16* __restrict__ x, const bf16* __restrict__ res,
    bf16* __restrict__ h, const bf16* __restrict__ w, bf16* __restrict__ y,
    float* __restrict__ rstd, int M, int N, float eps) {
  using VT = Vec<bf16>;
  typedef typename VT::V V;
  constexpr int W = VT::W;
  constexpr int VS = WAVE * SPAN;  // vectors between a thread's slots
  __shared__ float red[SPAN > 1 ? 2 * R * RMS_WAVES : 1];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const int tu = SPAN == 1 ? lane : (int)threadIdx.x;  // thread of the unit
  const int u = SPAN == 1 ? (int)blockIdx.x * RMS_WAVES + wave : (int)blockIdx.x;
  const long long U = (long long)gridDim.x * (RMS_WAVES / SPAN);
  const bool last_ok = (tu + (NVEC - 1) * VS) * W < N;
  // 32-bit per-thread element offset of vector 0; row bases stay uniform
  const unsigned voff = tu * W;
  const V zero = {};
  V wv[NVEC];
#pragma unroll
  for (int j = 0; j < NVEC; ++j) {
    wv[j] = zero;
    if (j < NVEC - 1 || last_ok) wv[j] = VT::load(w + voff + j * VS * W);
  }
  int slot = 0;
  for (long long row0 = u; row0 < M; row0 += U * R) {
    V xc[R][NVEC], rc[R][NVEC];
    // every load of the batch is issued before its reduction
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = row0 + r * U;
#pragma unroll
      for (int j = 0; j < NVEC; ++j) xc[r][j] = rc[r][j] = zero;
      if (row < M) {
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
          if (j < NVEC - 1 || last_ok) {
            xc[r][j] = VT::load(x + row * N + voff + j * VS * W);
            if (HAS_RES) rc[r][j] = VT::load(res + row * N + voff + j * VS * W);
          }
        }
      }
    }
    float p[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = row0 + r * U;
      p[r] = 0.f;
      if (row < M) {
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
          if (HAS_RES) {
            V hv;
#pragma unroll
            for (int k = 0; k < W; ++k)
              VT::set(hv, k, VT::get(xc[r][j], k) + VT::get(rc[r][j], k));
            if (j < NVEC - 1 || last_ok)
              VT::store(h + row * N + voff + j * VS * W, hv);
            xc[r][j] = hv;
          }
#pragma unroll
          for (int k = 0; k < W; ++k) {
            const float f = VT::get(xc[r][j], k);
            p[r] += f * f;
          }
        }
        p[r] = wave_sum(p[r]);
      }
    }
    rms_exchange<R, SPAN>(p, red, slot, lane, wave);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = row0 + r * U;
      if (row < M) {
        const float rs = rsqrtf(p[r] / N + eps);
        if (tu == 0) rstd[row] = rs;
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
          V ov;
#pragma unroll
          for (int k = 0; k < W; ++k)
            VT::set(ov, k, VT::get(xc[r][j], k) * rs * VT::get(wv[j], k));
          if (j < NVEC - 1 || last_ok)
            VT::store(y + row * N + voff + j * VS * W, ov);
        }
      }
    }
  }
}

// Backward dx (+dh) with the dw partials kept in per-thread fp32 registers
// across all of the unit's rows; at the end unit u writes stripe row u of
// pdw [U, N] (coalesced). A unit that owns no row writes zeros, so the
// at::empty stripe buffer is fully defined: no atomics, no zero-fill launch.
// `x` is the tensor the forward normalised (h in the residual form).
// dh is only added at the very end: its loads go out per row after the
// partial sums are formed and land behind the batch's one reduction.
template <bool HAS_DH, int NVEC, int R, int SPAN>
__global__ __launch_bounds__(RMS_BLOCK) RMS_NO_PK_F32 void rms_bwd_kernel(
    const bf16* __restrict__ dy, const bf16* __restrict__ dh,
    const bf16* __restrict__ x, const bf16* __restrict__ w,
    const float* __restrict__ rstd, bf16* __restrict__ dx,
    float* __restrict__ pdw, int M, int N) {
  using VT = Vec<bf16>;
  typedef typename VT::V V;
  constexpr int W = VT::W;
  constexpr int VS = WAVE * SPAN;
  __shared__ float red[SPAN > 1 ? 2 * R * RMS_WAVES : 1];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / WAVE));
  const int tu = SPAN == 1 ? lane : (int)threadIdx.x;
  const int u = SPAN == 1 ? (int)blockIdx.x * RMS_WAVES + wave : (int)blockIdx.x;
  const long long U = (long long)gridDim.x * (RMS_WAVES / SPAN);
  const bool last_ok = (tu + (NVEC - 1) * VS) * W < N;
  const unsigned voff = tu * W;
  const V zero = {};
  V wv[NVEC];
  float accdw[NVEC][W];
#pragma unroll
  for (int j = 0; j < NVEC; ++j) {
    wv[j] = zero;
    if (j < NVEC - 1 || last_ok) wv[j] = VT::load(w + voff + j * VS * W);
#pragma unroll
    for (int k = 0; k < W; ++k) accdw[j][k] = 0.f;
  }
  int slot = 0;
  for (long long row0 = u; row0 < M; row0 += U * R) {
    V dyc[R][NVEC], xc[R][NVEC], hc[R][NVEC];
    float rs[R], p[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = row0 + r * U;
      rs[r] = 0.f;
#pragma unroll
      for (int j = 0; j < NVEC; ++j) dyc[r][j] = xc[r][j] = zero;
      if (row < M) {
        rs[r] = rstd[row];
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
          if (j < NVEC - 1 || last_ok) {
            dyc[r][j] = VT::load(dy + row * N + voff + j * VS * W);
            xc[r][j] = VT::load(x + row * N + voff + j * VS * W);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = row0 + r * U;
      p[r] = 0.f;
      if (row < M) {
        // a thread without the last vector holds zeros there: it adds 0 to
        // the row sum and to its (never written) accumulators
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
#pragma unroll
          for (int k = 0; k < W; ++k) {
            const float d = VT::get(dyc[r][j], k);
            const float hx = VT::get(xc[r][j], k);
            p[r] += VT::get(wv[j], k) * d * hx;
            accdw[j][k] += d * hx * rs[r];
          }
        }
        // keep the row packed across the reduction instead of carrying its
        // unpacked fp32 products over it (2x the registers)
#pragma unroll
        for (int j = 0; j < NVEC; ++j)
          asm volatile("" : "+v"(dyc[r][j]), "+v"(xc[r][j]));
        if (HAS_DH) {
#pragma unroll
          for (int j = 0; j < NVEC; ++j) {
            hc[r][j] = zero;
            if (j < NVEC - 1 || last_ok)
              hc[r][j] = VT::load(dh + row * N + voff + j * VS * W);
          }
        }
        p[r] = wave_sum(p[r]);
      }
    }
    rms_exchange<R, SPAN>(p, red, slot, lane, wave);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = row0 + r * U;
      if (row < M) {
        const float c = p[r] / N * rs[r] * rs[r];
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
          V ov;
#pragma unroll
          for (int k = 0; k < W; ++k) {
            const float g = VT::get(wv[j], k) * VT::get(dyc[r][j], k);
            float gx = (g - VT::get(xc[r][j], k) * c) * rs[r];
            if (HAS_DH) gx += VT::get(hc[r][j], k);
            VT::set(ov, k, gx);
          }
          if (j < NVEC - 1 || last_ok)
            VT::store(dx + row * N + voff + j * VS * W, ov);
        }
      }
    }
  }
  float* sdw = pdw + (long long)u * N;
#pragma unroll
  for (int j = 0; j < NVEC; ++j) {
    if (j < NVEC - 1 || last_ok) {
      const unsigned col = voff + j * VS * W;
#pragma unroll
      for (int k = 0; k < W; k += 4) {
        f32x4 vw = {accdw[j][k], accdw[j][k + 1], accdw[j][k + 2],
                    accdw[j][k + 3]};
        *reinterpret_cast<f32x4*>(sdw + col + k) = vw;
      }
    }
  }
}

// Column-reduce the stripe buffer -> dw[N], written directly in the requested
// dtype (fp32, or bf16 with the round-to-nearest-even of a .to(bfloat16) of
// the fp32 sum). A workgroup takes 32 adjacent columns; consecutive lanes
// read consecutive columns of one stripe row. 64 partials per column, partial
// l summing stripes l, l+64, ... in ascending order; thread (s, c) holds
// partials s and s+32 of column c, adds them in registers, and the remaining
// five levels go through LDS at distances 16, 8, 4, 2, 1: a fixed tree.
#define RMS_DW_BLOCK 1024
#define RMS_DW_SLAB 32
#define RMS_DW_SUB (RMS_DW_BLOCK / RMS_DW_SLAB)
static_assert(RMS_DW_SUB == WAVE / 2, "tree below assumes 64 partials");
DEV_INLINE void rms_store_out(float* p, float v) { *p = v; }
DEV_INLINE void rms_store_out(bf16* p, float v) { *p = f2bf(v); }

template <typename OutT>
__global__ __launch_bounds__(RMS_DW_BLOCK) void rms_dw_reduce_kernel(
    const float* __restrict__ pdw, OutT* __restrict__ dw, int G, int N) {
  __shared__ float red[RMS_DW_SUB][RMS_DW_SLAB];
  const int c = threadIdx.x % RMS_DW_SLAB;
  const int sub = threadIdx.x / RMS_DW_SLAB;
  const int col = blockIdx.x * RMS_DW_SLAB + c;
  float sa = 0.f, sb = 0.f;
  if (col < N) {
#pragma unroll 4
    for (int g = sub; g < G; g += WAVE) {
      sa += pdw[(long long)g * N + col];
      if (g + RMS_DW_SUB < G) sb += pdw[(long long)(g + RMS_DW_SUB) * N + col];
    }
  }
  red[sub][c] = sa + sb;
#pragma unroll
  for (int off = RMS_DW_SUB / 2; off > 0; off >>= 1) {
    __syncthreads();
    if (sub < off) red[sub][c] += red[sub + off][c];
  }
  if (sub == 0 && col < N) rms_store_out(dw + col, red[0][c]);
}

}  // namespace tdsa

using namespace tdsa;

// ---- launch geometry ------------------------------------------------------------
// Routing: bf16, N % 8 == 0, 8 <= N <= 8192; a wave per row up to 2048, the
// workgroup per row above. Returns the span, 0 when the shape is not routed.
#define RMS_SPAN1_MAX (RMS_MAXVEC * WAVE * 8)
#define RMS_BOUND (RMS_MAXVEC * RMS_BLOCK * 8)
static int rms_span(int N, int is_bf16) {
  if (!is_bf16 || N < 8 || N % 8 || N > RMS_BOUND) return 0;
  return N <= RMS_SPAN1_MAX ? 1 : RMS_WAVES;
}

static int rms_nvec(int N, int span) {
  return (N / 8 + WAVE * span - 1) / (WAVE * span);
}

// Units of a grid: whole workgroups, at most `cap` waves' worth, no more
// than the rows need. The caps are the LayerNorm row-per-wave knobs, counted
// in waves: with SPAN = 4 a unit is a workgroup, so cap / 4 units.
static int rms_units(int M, long long cap, int span) {
  const int per_wg = RMS_WAVES / span;
  long long wgs = ((long long)(M < 1 ? 1 : M) + per_wg - 1) / per_wg;
  long long cap_wgs = cap / RMS_WAVES;
  if (cap_wgs < 1) cap_wgs = 1;
  if (wgs > cap_wgs) wgs = cap_wgs;
  return (int)(wgs * per_wg);
}
static int rms_fwd_units(int M, int span) {
  return rms_units(M, env_int("TDSA_LN_RW_WAVES", 4096), span);
}
static int rms_bwd_units(int M, int span) {
  return rms_units(M, env_int("TDSA_LN_STRIPES", 2048), span);
}

// (span, nvec) become template arguments: SPAN = 1 has NVEC 1..4, SPAN = 4
// has NVEC 2..4 (N > 2048 is more than 256 vectors).
template <typename F>
static void rms_with_shape(int span, int nvec, F f) {
  static_assert(RMS_MAXVEC == 4, "one case per routed vector count");
  using S1 = std::integral_constant<int, 1>;
  using S4 = std::integral_constant<int, RMS_WAVES>;
  if (span == 1) {
    switch (nvec) {
      case 1: f(S1{}, std::integral_constant<int, 1>{}); break;
      case 2: f(S1{}, std::integral_constant<int, 2>{}); break;
      case 3: f(S1{}, std::integral_constant<int, 3>{}); break;
      default: f(S1{}, std::integral_constant<int, 4>{}); break;
    }
  } else {
    switch (nvec) {
      case 2: f(S4{}, std::integral_constant<int, 2>{}); break;
      case 3: f(S4{}, std::integral_constant<int, 3>{}); break;
      default: f(S4{}, std::integral_constant<int, 4>{}); break;
    }
  }
}
template <typename F>
static void rms_with_flag(bool flag, F f) {
  if (flag) f(std::true_type{}); else f(std::false_type{});
}

extern "C" {

void tdsa_rms_geometry(int M, int N, int is_bf16, int* stripes, int* fwd_units,
                       int* fwd_depth, int* bwd_depth, int* span, int* bound) {
  const int sp = rms_span(N, is_bf16);
  const int nvec = sp ? rms_nvec(N, sp) : 0;
  *span = sp;
  *stripes = sp ? rms_bwd_units(M, sp) : 0;
  *fwd_units = sp ? rms_fwd_units(M, sp) : 0;
  *fwd_depth = sp ? RMS_FWD_DEPTH(nvec) : 0;
  *bwd_depth = sp ? RMS_BWD_DEPTH(nvec) : 0;
  *bound = sp ? RMS_BOUND : 0;
}

hipError_t tdsa_rms_fwd(const void* x, const void* res, void* h, const void* w,
                        void* y, float* rstd, int M, int N, float eps,
                        int is_bf16, hipStream_t stream) {
  const int span = rms_span(N, is_bf16);
  if (!span || M < 0 || (res != nullptr) != (h != nullptr))
    return hipErrorInvalidValue;
  if (M == 0) return hipSuccess;
  const int grid = rms_fwd_units(M, span) / (RMS_WAVES / span);
  rms_with_shape(span, rms_nvec(N, span), [&](auto sp, auto nv) {
    rms_with_flag(res != nullptr, [&](auto has_res) {
      constexpr int SP = decltype(sp)::value;
      constexpr int NV = decltype(nv)::value;
      hipLaunchKernelGGL(
          (rms_fwd_kernel<decltype(has_res)::value, NV, RMS_FWD_DEPTH(NV), SP>),
          dim3(grid), dim3(RMS_BLOCK), 0, stream, (const bf16*)x,
          (const bf16*)res, (bf16*)h, (const bf16*)w, (bf16*)y, rstd, M, N,
          eps);
    });
  });
  return hipGetLastError();
}

hipError_t tdsa_rms_bwd_dx(const void* dy, const void* dh, const void* x,
                           const void* w, const float* rstd, void* dx,
                           float* pdw, int M, int N, int is_bf16,
                           hipStream_t stream) {
  const int span = rms_span(N, is_bf16);
  if (!span || M < 0) return hipErrorInvalidValue;
  // M == 0 still launches: the one unit writes its zero stripe row
  const int grid = rms_bwd_units(M, span) / (RMS_WAVES / span);
  rms_with_shape(span, rms_nvec(N, span), [&](auto sp, auto nv) {
    rms_with_flag(dh != nullptr, [&](auto has_dh) {
      constexpr int SP = decltype(sp)::value;
      constexpr int NV = decltype(nv)::value;
      hipLaunchKernelGGL(
          (rms_bwd_kernel<decltype(has_dh)::value, NV, RMS_BWD_DEPTH(NV), SP>),
          dim3(grid), dim3(RMS_BLOCK), 0, stream, (const bf16*)dy,
          (const bf16*)dh, (const bf16*)x, (const bf16*)w, rstd, (bf16*)dx,
          pdw, M, N);
    });
  });
  return hipGetLastError();
}

hipError_t tdsa_rms_dw_reduce(const float* pdw, void* dw, int G, int N,
                              int out_bf16, hipStream_t stream) {
  if (G < 1 || N < 1) return hipErrorInvalidValue;
  const int grid = (N + RMS_DW_SLAB - 1) / RMS_DW_SLAB;
  dispatch_dtype(out_bf16, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(rms_dw_reduce_kernel<T>, dim3(grid), dim3(RMS_DW_BLOCK),
                       0, stream, pdw, (T*)dw, G, N);
  });
  return hipGetLastError();
}

}  // extern "C"
