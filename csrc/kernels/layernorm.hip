// LayerNorm forward / backward CDNA4 kernels (last-dim, affine+bias).
//
// Replaces the reference's three Triton kernels
// (/root/reference/tiny_deepspeed/core/module/ops/layernorm.py:158-298) with
// an MI355X-native design: fp32 accumulation, bf16x8 / float4 vectorized
// global traffic, and a conflict-free two-pass dw/db reduction through fp32
// stripe buffers instead of the reference's spin-lock atomic_cas scheme
// (SURVEY.md 2.10A). bf16 rows up to N=2048 run on the row-per-wave kernels
// (one wave per row, dw/db partials in registers); fp32 and wider rows on
// the workgroup-per-row and wide kernels.
#include "common.h"
#include "launchers.h"

#include <type_traits>

namespace tdsa {

// ---- workgroup-per-row kernels (fp32, and bf16 with TDSA_LN_ROWWAVE=0) ------
// Register-cache depth: a thread keeps up to LN_WG_MAXITER vectors of its row
// between the statistics pass and the apply pass. The kernels' MAXITER
// argument and the launchers' wide-row test both take it from here; a row
// with more than LN_WG_MAXITER * blockDim.x vectors would index past the
// cache.
constexpr int LN_WG_MAXITER = 2;

// HAS_RES: fused residual add — h = x + res is computed in-kernel, written
// out (the residual stream) and normalized, saving the separate elementwise
// add pass + launch per LayerNorm site (2 per transformer block).
// MAXITER = 0 is the wide-row form: nothing is cached and the apply pass
// reads the row a second time (L2-resident at practical widths), so any N
// fits.
// There is no one-wave-per-workgroup form: at one row per 64-thread
// workgroup it measured 2-3x slower (docs/kernels.md).
template <typename T, bool HAS_RES, int MAXITER>
__global__ void ln_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                              T* __restrict__ h, const T* __restrict__ w,
                              const T* __restrict__ b, T* __restrict__ y,
                              float* __restrict__ mean, float* __restrict__ rstd,
                              int M, int N, float eps) {
  using VT = Vec<T>;
  constexpr int W = VT::W;
  constexpr bool CACHED = MAXITER > 0;
  __shared__ float scratch[2 * 1024 / WAVE];
  const int tid = threadIdx.x;
  const int nth = blockDim.x;
  for (int row = blockIdx.x; row < M; row += gridDim.x) {
    const T* xr = x + (long long)row * N;
    const T* rr = HAS_RES ? res + (long long)row * N : nullptr;
    T* hr = HAS_RES ? h + (long long)row * N : nullptr;
    typename VT::V xc[CACHED ? MAXITER : 1];
    float s = 0.f, ss = 0.f;
    {
      int it = 0;
      for (int i = tid * W; i < N; i += nth * W, ++it) {
        typename VT::V v = VT::load(xr + i);
        if (HAS_RES) {
          typename VT::V rv = VT::load(rr + i);
          typename VT::V hv;
#pragma unroll
          for (int k = 0; k < W; ++k)
            VT::set(hv, k, VT::get(v, k) + VT::get(rv, k));
          VT::store(hr + i, hv);
          v = hv;
        }
        if (CACHED) xc[it] = v;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          float f = VT::get(v, k);
          s += f;
          ss += f * f;
        }
      }
    }
    block_sum2(s, ss, scratch);
    const float mu = s / N;
    const float var = fmaxf(ss / N - mu * mu, 0.0f);
    const float rs = rsqrtf(var + eps);
    if (tid == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
    // uncached: re-read the (already residual-fused) row
    const T* src = HAS_RES ? hr : xr;
    T* yr = y + (long long)row * N;
    {
      int it = 0;
      for (int i = tid * W; i < N; i += nth * W, ++it) {
        typename VT::V xv = CACHED ? xc[it] : VT::load(src + i);
        typename VT::V wv = VT::load(w + i);
        typename VT::V bv = VT::load(b + i);
        typename VT::V ov;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          float xh = (VT::get(xv, k) - mu) * rs;
          VT::set(ov, k, xh * VT::get(wv, k) + VT::get(bv, k));
        }
        VT::store(yr + i, ov);
      }
    }
  }
}

// Backward dx, launched at one row per workgroup; the dw/db stripes come from
// ln_dwdb_accum_kernel below. A fused form that also accumulated the stripes
// here chained a workgroup's rows through two block-wide reduction barriers
// each and measured 9 % slower than the pair, although the pair reads dy and
// x once more (docs/kernels.md).
// HAS_DH: dx += dh (gradient of the residual-stream output h), fusing the
// backward-side elementwise add of the residual connection.
template <typename T, int MAXITER, bool HAS_DH>
__global__ void ln_bwd_dx_kernel(const T* __restrict__ dy, const T* __restrict__ dh,
                                 const T* __restrict__ x,
                                 const T* __restrict__ w, const float* __restrict__ mean,
                                 const float* __restrict__ rstd, T* __restrict__ dx,
                                 int M, int N) {
  using VT = Vec<T>;
  constexpr int W = VT::W;
  __shared__ float scratch[2 * 1024 / WAVE];
  const int tid = threadIdx.x;
  const int nth = blockDim.x;
  for (int row = blockIdx.x; row < M; row += gridDim.x) {
    const T* dyr = dy + (long long)row * N;
    const T* xr = x + (long long)row * N;
    const float mu = mean[row];
    const float rs = rstd[row];
    typename VT::V dyc[MAXITER], xc[MAXITER];
    float c1 = 0.f, c2 = 0.f;
    {
      int it = 0;
      for (int i = tid * W; i < N; i += nth * W, ++it) {
        typename VT::V dv = VT::load(dyr + i);
        typename VT::V xv = VT::load(xr + i);
        typename VT::V wv = VT::load(w + i);
        dyc[it] = dv;
        xc[it] = xv;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          float d = VT::get(dv, k);
          float xh = (VT::get(xv, k) - mu) * rs;
          float wdy = VT::get(wv, k) * d;
          c1 += xh * wdy;
          c2 += wdy;
        }
      }
    }
    block_sum2(c1, c2, scratch);
    c1 /= N;
    c2 /= N;
    T* dxr = dx + (long long)row * N;
    const T* dhr = HAS_DH ? dh + (long long)row * N : nullptr;
    {
      int it = 0;
      for (int i = tid * W; i < N; i += nth * W, ++it) {
        typename VT::V dv = dyc[it];
        typename VT::V xv = xc[it];
        typename VT::V wv = VT::load(w + i);
        typename VT::V hv;
        if (HAS_DH) hv = VT::load(dhr + i);
        typename VT::V ov;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          float d = VT::get(dv, k);
          float xh = (VT::get(xv, k) - mu) * rs;
          float wdy = VT::get(wv, k) * d;
          float g = (wdy - (xh * c1 + c2)) * rs;
          if (HAS_DH) g += VT::get(hv, k);
          VT::set(ov, k, g);
        }
        VT::store(dxr + i, ov);
      }
    }
  }
}

// Streaming dw/db stripe accumulation (no barriers: the per-column sums
// need no cross-thread reduction). Block g chains rows g, g+G, ... into
// stripe row g of pdw/pdb (no atomics); with nothing serializing the row
// loop it runs at the HBM read floor.
template <typename T, int MAXITER>
__global__ void ln_dwdb_accum_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     float* __restrict__ pdw,
                                     float* __restrict__ pdb, int M, int N) {
  using VT = Vec<T>;
  constexpr int W = VT::W;
  const int tid = threadIdx.x;
  const int nth = blockDim.x;
  float accdw[MAXITER][W];
  float accdb[MAXITER][W];
#pragma unroll
  for (int it = 0; it < MAXITER; ++it)
#pragma unroll
    for (int k = 0; k < W; ++k) accdw[it][k] = accdb[it][k] = 0.f;
  for (int row = blockIdx.x; row < M; row += gridDim.x) {
    const T* dyr = dy + (long long)row * N;
    const T* xr = x + (long long)row * N;
    const float mu = mean[row];
    const float rs = rstd[row];
    int it = 0;
    for (int i = tid * W; i < N; i += nth * W, ++it) {
      typename VT::V dv = VT::load(dyr + i);
      typename VT::V xv = VT::load(xr + i);
#pragma unroll
      for (int k = 0; k < W; ++k) {
        float d = VT::get(dv, k);
        accdw[it][k] += d * (VT::get(xv, k) - mu) * rs;
        accdb[it][k] += d;
      }
    }
  }
  float* sdw = pdw + (long long)blockIdx.x * N;
  float* sdb = pdb + (long long)blockIdx.x * N;
  int it = 0;
  for (int i = tid * W; i < N; i += nth * W, ++it) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      sdw[i + k] = accdw[it][k];
      sdb[i + k] = accdb[it][k];
    }
  }
}

// ---- row-per-wave kernels --------------------------------------------------
// 256-thread workgroups, four waves, each wave owning whole rows: wave g of
// the G waves in the (persistent) grid takes rows g, g+G, ... Lane l holds
// NVEC 16-byte vectors of the row (vectors l, l+64, ...; only the last one
// is predicated), so both per-row sums are pure wave_sum shuffles: no
// __shared__, no __syncthreads, nothing chaining one row to the next.
// Memory-level parallelism is explicit instead of left to however many
// tiny workgroups a CU holds: a wave issues every global load of a batch of
// R rows before the first reduction of that batch, and several such waves
// share a SIMD. (An earlier one-wave attempt with one row per 64-thread
// workgroup had 32768 tiny workgroups and one row of loads in flight per
// wave; that, not the missing barrier, made it 2-3x slower.)
#define LN_RW_BLOCK 256
#define LN_RW_WAVES (LN_RW_BLOCK / WAVE)
#define LN_RW_MAXVEC 4
// Batch depths (rows whose loads are in flight per wave). Bounded by
// registers: the backward keeps 2*NVEC*W fp32 dw/db accumulators live.
#ifndef LN_RW_FWD_DEPTH
#define LN_RW_FWD_DEPTH(NVEC) ((NVEC) <= 2 ? 4 : 2)
#endif
#ifndef LN_RW_BWD_DEPTH
#define LN_RW_BWD_DEPTH(NVEC) 2
#endif

// Row sums are reduced per vector slot (one wave_sum each) and the slots
// combined as (s0 + s2) + (s1 + s3): vector slot j of a row is exactly what
// wave j of the workgroup-per-row kernel holds, and this is the order its
// block_sum2 adds the waves in. The row statistics, and with them y and dx,
// therefore keep the bits of that path.
template <int NVEC>
DEV_INLINE float ln_rw_row_sum(float (&p)[NVEC]) {
#pragma unroll
  for (int j = 0; j < NVEC; ++j) p[j] = wave_sum(p[j]);
  if (NVEC == 1) return p[0];
  if (NVEC == 2) return p[0] + p[1];
  if (NVEC == 3) return (p[0] + p[2]) + p[1];
  return (p[0] + p[2]) + (p[1] + p[NVEC - 1]);
}

template <typename T, bool HAS_RES, int NVEC, int R>
__global__ __launch_bounds__(LN_RW_BLOCK) void ln_fwd_rowwave_kernel(
    const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ h,
    const T* __restrict__ w, const T* __restrict__ b, T* __restrict__ y,
    float* __restrict__ mean, float* __restrict__ rstd, int M, int N,
    float eps) {
  using VT = Vec<T>;
  typedef typename VT::V V;
  constexpr int W = VT::W;
  const int lane = threadIdx.x & (WAVE - 1);
  const int g = __builtin_amdgcn_readfirstlane(
      (int)(blockIdx.x * LN_RW_WAVES + threadIdx.x / WAVE));
  const long long G = (long long)gridDim.x * LN_RW_WAVES;
  const bool last_ok = (lane + (NVEC - 1) * WAVE) * W < N;
  // 32-bit per-lane element offset of vector 0; row bases stay wave-uniform
  // (scalar base + lane offset addressing, no 64-bit per-lane pointers)
  const unsigned voff = lane * W;
  const V zero = {};
  V wv[NVEC], bv[NVEC];
#pragma unroll
  for (int j = 0; j < NVEC; ++j) {
    wv[j] = bv[j] = zero;
    if (j < NVEC - 1 || last_ok) {
      wv[j] = VT::load(w + voff + j * WAVE * W);
      bv[j] = VT::load(b + voff + j * WAVE * W);
    }
  }
  for (long long row0 = g; row0 < M; row0 += G * R) {
    V xc[R][NVEC], rc[R][NVEC];
    // every load of the batch is issued before the first reduction
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = row0 + r * G;
#pragma unroll
      for (int j = 0; j < NVEC; ++j) xc[r][j] = rc[r][j] = zero;
      if (row < M) {
        const T* xr = x + row * N;
        const T* rr = HAS_RES ? res + row * N : nullptr;
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
          if (j < NVEC - 1 || last_ok) {
            xc[r][j] = VT::load(xr + voff + j * WAVE * W);
            if (HAS_RES) rc[r][j] = VT::load(rr + voff + j * WAVE * W);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = row0 + r * G;
      if (row < M) {
        float ps[NVEC], pss[NVEC];
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
          ps[j] = pss[j] = 0.f;
          V v = xc[r][j];
          if (HAS_RES) {
            V hv;
#pragma unroll
            for (int k = 0; k < W; ++k)
              VT::set(hv, k, VT::get(v, k) + VT::get(rc[r][j], k));
            if (j < NVEC - 1 || last_ok)
              VT::store(h + row * N + voff + j * WAVE * W, hv);
            v = hv;
            xc[r][j] = hv;
          }
#pragma unroll
          for (int k = 0; k < W; ++k) {
            float f = VT::get(v, k);
            ps[j] += f;
            pss[j] += f * f;
          }
        }
        const float s = ln_rw_row_sum<NVEC>(ps);
        const float ss = ln_rw_row_sum<NVEC>(pss);
        const float mu = s / N;
        const float var = fmaxf(ss / N - mu * mu, 0.0f);
        const float rs = rsqrtf(var + eps);
        if (lane == 0) {
          mean[row] = mu;
          rstd[row] = rs;
        }
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
          V ov;
#pragma unroll
          for (int k = 0; k < W; ++k) {
            float xh = (VT::get(xc[r][j], k) - mu) * rs;
            VT::set(ov, k, xh * VT::get(wv[j], k) + VT::get(bv[j], k));
          }
          if (j < NVEC - 1 || last_ok)
            VT::store(y + row * N + voff + j * WAVE * W, ov);
        }
      }
    }
  }
}

// Backward dx (+dh) with the dw/db partials kept in per-lane fp32 registers
// across all of the wave's rows: with no barrier in the row loop the
// chaining that forced the r2 split does not exist, so dy and x are read
// once. At the end wave g writes stripe row g of pdw/pdb (coalesced); a wave
// that owns no row writes zeros, so the at::empty stripes are fully defined.
template <typename T, bool HAS_DH, int NVEC, int R>
__global__ __launch_bounds__(LN_RW_BLOCK) void ln_bwd_rowwave_kernel(
    const T* __restrict__ dy, const T* __restrict__ dh, const T* __restrict__ x,
    const T* __restrict__ w, const float* __restrict__ mean,
    const float* __restrict__ rstd, T* __restrict__ dx,
    float* __restrict__ pdw, float* __restrict__ pdb, int M, int N) {
  using VT = Vec<T>;
  typedef typename VT::V V;
  constexpr int W = VT::W;
  const int lane = threadIdx.x & (WAVE - 1);
  const int g = __builtin_amdgcn_readfirstlane(
      (int)(blockIdx.x * LN_RW_WAVES + threadIdx.x / WAVE));
  const long long G = (long long)gridDim.x * LN_RW_WAVES;
  const bool last_ok = (lane + (NVEC - 1) * WAVE) * W < N;
  // 32-bit per-lane element offset of vector 0; row bases stay wave-uniform
  // (scalar base + lane offset addressing, no 64-bit per-lane pointers)
  const unsigned voff = lane * W;
  const V zero = {};
  V wv[NVEC];
  float accdw[NVEC][W], accdb[NVEC][W];
#pragma unroll
  for (int j = 0; j < NVEC; ++j) {
    wv[j] = zero;
    if (j < NVEC - 1 || last_ok) wv[j] = VT::load(w + voff + j * WAVE * W);
#pragma unroll
    for (int k = 0; k < W; ++k) accdw[j][k] = accdb[j][k] = 0.f;
  }
  for (long long row0 = g; row0 < M; row0 += G * R) {
    V dyc[R][NVEC], xc[R][NVEC];
    float mu[R], rs[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = row0 + r * G;
      mu[r] = rs[r] = 0.f;
#pragma unroll
      for (int j = 0; j < NVEC; ++j) dyc[r][j] = xc[r][j] = zero;
      if (row < M) {
        mu[r] = mean[row];
        rs[r] = rstd[row];
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
          if (j < NVEC - 1 || last_ok) {
            dyc[r][j] = VT::load(dy + row * N + voff + j * WAVE * W);
            xc[r][j] = VT::load(x + row * N + voff + j * WAVE * W);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const long long row = row0 + r * G;
      if (row < M) {
        float p1[NVEC], p2[NVEC];
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
          p1[j] = p2[j] = 0.f;
          // a lane without the last vector must not fold -mu*rs into dw
          if (j < NVEC - 1 || last_ok) {
#pragma unroll
            for (int k = 0; k < W; ++k) {
              float d = VT::get(dyc[r][j], k);
              float xh = (VT::get(xc[r][j], k) - mu[r]) * rs[r];
              float wdy = VT::get(wv[j], k) * d;
              p1[j] += xh * wdy;
              p2[j] += wdy;
              // same expression, row order and stripe mapping as
              // ln_dwdb_accum_kernel: the stripes keep its bits
              accdw[j][k] += d * (VT::get(xc[r][j], k) - mu[r]) * rs[r];
              accdb[j][k] += d;
            }
          }
        }
        // keep the row packed across the reduction: without this the
        // compiler carries the unpacked fp32 xh/wdy of the whole row over
        // the wave_sum (2x the registers) instead of re-deriving them
#pragma unroll
        for (int j = 0; j < NVEC; ++j)
          asm volatile("" : "+v"(dyc[r][j]), "+v"(xc[r][j]));
        // dh is only added at the very end: its loads go out here, one row
        // at a time, and land behind the c1/c2 reduction instead of holding
        // registers for the whole batch
        V hc[NVEC];
        if (HAS_DH) {
#pragma unroll
          for (int j = 0; j < NVEC; ++j) {
            hc[j] = zero;
            if (j < NVEC - 1 || last_ok)
              hc[j] = VT::load(dh + row * N + voff + j * WAVE * W);
          }
        }
        const float c1 = ln_rw_row_sum<NVEC>(p1) / N;
        const float c2 = ln_rw_row_sum<NVEC>(p2) / N;
#pragma unroll
        for (int j = 0; j < NVEC; ++j) {
          V ov;
#pragma unroll
          for (int k = 0; k < W; ++k) {
            float d = VT::get(dyc[r][j], k);
            float xh = (VT::get(xc[r][j], k) - mu[r]) * rs[r];
            float wdy = VT::get(wv[j], k) * d;
            float gx = (wdy - (xh * c1 + c2)) * rs[r];
            if (HAS_DH) gx += VT::get(hc[j], k);
            VT::set(ov, k, gx);
          }
          if (j < NVEC - 1 || last_ok)
            VT::store(dx + row * N + voff + j * WAVE * W, ov);
        }
      }
    }
  }
  float* sdw = pdw + (long long)g * N;
  float* sdb = pdb + (long long)g * N;
#pragma unroll
  for (int j = 0; j < NVEC; ++j) {
    if (j < NVEC - 1 || last_ok) {
      const unsigned col = voff + j * WAVE * W;
#pragma unroll
      for (int k = 0; k < W; k += 4) {
        f32x4 vw = {accdw[j][k], accdw[j][k + 1], accdw[j][k + 2],
                      accdw[j][k + 3]};
        f32x4 vb = {accdb[j][k], accdb[j][k + 1], accdb[j][k + 2],
                      accdb[j][k + 3]};
        *reinterpret_cast<f32x4*>(sdw + col + k) = vw;
        *reinterpret_cast<f32x4*>(sdb + col + k) = vb;
      }
    }
  }
}

// ---- wide-row backward -----------------------------------------------------
// Rows beyond the register-cache bound (N > LN_WG_MAXITER * block * W) are a
// correctness fallback for non-GPT widths; the forward is ln_fwd_kernel with
// MAXITER = 0. Both passes read dy and x from global (L2-resident at
// practical widths), and the stripe partials accumulate straight into the
// block-owned global stripe rows (read-modify-write, no atomics needed)
// after a zero-init sweep — registers cannot hold a whole wide row.
template <typename T, bool HAS_DH>
__global__ void ln_bwd_dx_wide_kernel(const T* __restrict__ dy,
                                      const T* __restrict__ dh,
                                      const T* __restrict__ x,
                                      const T* __restrict__ w,
                                      const float* __restrict__ mean,
                                      const float* __restrict__ rstd,
                                      T* __restrict__ dx, float* __restrict__ pdw,
                                      float* __restrict__ pdb, int M, int N) {
  using VT = Vec<T>;
  constexpr int W = VT::W;
  __shared__ float scratch[2 * 1024 / WAVE];
  const int tid = threadIdx.x;
  const int nth = blockDim.x;
  float* sdw = pdw + (long long)blockIdx.x * N;
  float* sdb = pdb + (long long)blockIdx.x * N;
  for (int i = tid; i < N; i += nth) {
    sdw[i] = 0.f;
    sdb[i] = 0.f;
  }
  for (int row = blockIdx.x; row < M; row += gridDim.x) {
    const T* dyr = dy + (long long)row * N;
    const T* xr = x + (long long)row * N;
    const float mu = mean[row];
    const float rs = rstd[row];
    float c1 = 0.f, c2 = 0.f;
    for (int i = tid * W; i < N; i += nth * W) {
      typename VT::V dv = VT::load(dyr + i);
      typename VT::V xv = VT::load(xr + i);
      typename VT::V wv = VT::load(w + i);
#pragma unroll
      for (int k = 0; k < W; ++k) {
        float d = VT::get(dv, k);
        float xh = (VT::get(xv, k) - mu) * rs;
        float wdy = VT::get(wv, k) * d;
        c1 += xh * wdy;
        c2 += wdy;
      }
    }
    block_sum2(c1, c2, scratch);
    c1 /= N;
    c2 /= N;
    T* dxr = dx + (long long)row * N;
    const T* dhr = HAS_DH ? dh + (long long)row * N : nullptr;
    for (int i = tid * W; i < N; i += nth * W) {
      typename VT::V dv = VT::load(dyr + i);
      typename VT::V xv = VT::load(xr + i);
      typename VT::V wv = VT::load(w + i);
      typename VT::V hv;
      if (HAS_DH) hv = VT::load(dhr + i);
      typename VT::V ov;
#pragma unroll
      for (int k = 0; k < W; ++k) {
        float d = VT::get(dv, k);
        float xh = (VT::get(xv, k) - mu) * rs;
        float wdy = VT::get(wv, k) * d;
        float g = (wdy - (xh * c1 + c2)) * rs;
        if (HAS_DH) g += VT::get(hv, k);
        VT::set(ov, k, g);
        sdw[i + k] += d * xh;
        sdb[i + k] += d;
      }
      VT::store(dxr + i, ov);
    }
  }
}

// Column-reduce the stripe buffers -> dw[N], db[N], written directly in the
// requested dtype (fp32, or bf16 with the same round-to-nearest-even as a
// .to(bfloat16) of the fp32 sum).
// A workgroup takes a slab of LN_DWDB_SLAB adjacent columns; consecutive
// lanes read consecutive columns of one stripe row (each half-wave one
// contiguous 128-B segment). The summation tree is the one the previous
// column-per-wave kernel used, so dw/db keep their bits: 64 partials per
// column, partial l summing stripes l, l+64, ... in ascending order, then
// combined pairwise at distances 32, 16, 8, 4, 2, 1 (what its wave_sum
// butterfly computed). Thread (s, c) holds partials s and s+32 of column c
// and adds them in registers; the remaining five levels go through LDS in
// that fixed order. No atomics, no zero-init launch. (The previous form's
// 64 lanes read 64 stripe rows N*4 bytes apart per instruction, the worst
// access shape there is; an earlier 2-D atomicAdd version needed two
// at::zeros fills per call.)
#define LN_DWDB_BLOCK 1024
#define LN_DWDB_SLAB 32
#define LN_DWDB_SUB (LN_DWDB_BLOCK / LN_DWDB_SLAB)
static_assert(LN_DWDB_SUB == WAVE / 2, "tree below assumes 64 partials");
DEV_INLINE void ln_store_out(float* p, float v) { *p = v; }
DEV_INLINE void ln_store_out(bf16* p, float v) { *p = f2bf(v); }

template <typename OutT>
__global__ __launch_bounds__(LN_DWDB_BLOCK) void ln_bwd_dwdb_kernel(
    const float* __restrict__ pdw, const float* __restrict__ pdb,
    OutT* __restrict__ dw, OutT* __restrict__ db, int G, int N) {
  __shared__ float red[2][LN_DWDB_SUB][LN_DWDB_SLAB];
  const int c = threadIdx.x % LN_DWDB_SLAB;
  const int sub = threadIdx.x / LN_DWDB_SLAB;
  const int col = blockIdx.x * LN_DWDB_SLAB + c;
  float swa = 0.f, swb = 0.f, sba = 0.f, sbb = 0.f;
  if (col < N) {
#pragma unroll 4
    for (int g = sub; g < G; g += WAVE) {
      swa += pdw[(long long)g * N + col];
      sba += pdb[(long long)g * N + col];
      if (g + LN_DWDB_SUB < G) {
        swb += pdw[(long long)(g + LN_DWDB_SUB) * N + col];
        sbb += pdb[(long long)(g + LN_DWDB_SUB) * N + col];
      }
    }
  }
  red[0][sub][c] = swa + swb;
  red[1][sub][c] = sba + sbb;
#pragma unroll
  for (int off = LN_DWDB_SUB / 2; off > 0; off >>= 1) {
    __syncthreads();
    if (sub < off) {
      red[0][sub][c] += red[0][sub + off][c];
      red[1][sub][c] += red[1][sub + off][c];
    }
  }
  if (sub == 0 && col < N) {
    ln_store_out(dw + col, red[0][0][c]);
    ln_store_out(db + col, red[1][0][c]);
  }
}

}  // namespace tdsa

using namespace tdsa;

// ---- launch geometry --------------------------------------------------------
// Row-per-wave routing: bf16, N % 8 == 0, at most LN_RW_MAXVEC 16-byte
// vectors per lane (N <= 2048). TDSA_LN_ROWWAVE=0 gives the workgroup-per-row
// path back. Returns the vectors per lane, or 0 when the shape is not routed.
static int ln_rw_nvec(int N, int is_bf16) {
  const int on = (int)env_int("TDSA_LN_ROWWAVE", 1);
  if (!on || !is_bf16 || N < 8 || N % 8) return 0;
  const int nvec = (N / 8 + WAVE - 1) / WAVE;
  return nvec <= LN_RW_MAXVEC ? nvec : 0;
}

// Waves in a row-per-wave grid: whole workgroups, at most `cap` waves, no
// more than the rows need.
static int ln_rw_waves(int M, int cap) {
  long long g = ((long long)(M < 1 ? 1 : M) + LN_RW_WAVES - 1) / LN_RW_WAVES *
                LN_RW_WAVES;
  cap = cap / LN_RW_WAVES * LN_RW_WAVES;
  if (cap < LN_RW_WAVES) cap = LN_RW_WAVES;
  return (int)(g < cap ? g : cap);
}

// Waves of the row-per-wave forward grid. 4096 = 16 per CU, all resident.
static int ln_rw_fwd_waves(int M) {
  return ln_rw_waves(M, (int)env_int("TDSA_LN_RW_WAVES", 4096));
}

// Stripe count G for `nvec` vectors per lane (0: not row-per-wave). On the
// row-per-wave path G is the number of waves in the grid (every wave writes
// its stripe row).
static int ln_stripe_count(int M, int nvec) {
  // within-box sweep: 2048 stripes beat 4096 (dwdb reduce pays per stripe)
  const int cap = (int)env_int("TDSA_LN_STRIPES", 2048);
  if (nvec) return ln_rw_waves(M, cap);
  const int g = M < cap ? M : cap;
  return g < 1 ? 1 : g;
}

// Workgroup-per-row block size, matched to the row width: at 256 threads and
// N=1024 bf16 only 128 lanes have work (tid*W < N) — half the block idled
// (profiled 2x).
static int ln_block(int N, int W) {
  int need = (N + W - 1) / W;
  int blk = ((need + 63) / 64) * 64;
  if (blk > 256) blk = 256;
  if (blk < 64) blk = 64;
  return blk;
}

// Workgroup-per-row grid, one row per block up to the cap: chaining rows
// serializes the per-row reduction barriers; resident blocks overlap freely
// instead.
static int ln_wg_grid(int M) {
  const int cap = (int)env_int("TDSA_LN_GRID", 32768);
  return M < cap ? M : cap;
}

// ---- launchers ---------------------------------------------------------------
// A runtime flag or vector count becomes a template argument by calling `f`
// with the matching std::integral_constant.
template <typename F>
static void ln_with_flag(bool flag, F f) {
  if (flag) f(std::true_type{}); else f(std::false_type{});
}
template <typename F>
static void ln_rw_with_nvec(int nvec, F f) {
  static_assert(LN_RW_MAXVEC == 4, "one case per routed vector count");
  switch (nvec) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

// Workgroup-per-row forward; rows past the register cache take the re-reading
// form at full block size.
template <typename T>
static hipError_t ln_fwd_wg(const T* x, const T* res, T* h, const T* w,
                            const T* b, T* y, float* mean, float* rstd, int M,
                            int N, float eps, hipStream_t stream) {
  constexpr int W = Vec<T>::W;
  if (N % W) return hipErrorInvalidValue;  // 16B row-base alignment
  const int block = ln_block(N, W);
  const int grid = ln_wg_grid(M);
  ln_with_flag(res != nullptr, [&](auto has_res) {
    constexpr bool HAS_RES = decltype(has_res)::value;
    if (N > LN_WG_MAXITER * block * W)
      hipLaunchKernelGGL((ln_fwd_kernel<T, HAS_RES, 0>), dim3(grid), dim3(1024),
                         0, stream, x, res, h, w, b, y, mean, rstd, M, N, eps);
    else
      hipLaunchKernelGGL((ln_fwd_kernel<T, HAS_RES, LN_WG_MAXITER>), dim3(grid),
                         dim3(block), 0, stream, x, res, h, w, b, y, mean, rstd,
                         M, N, eps);
  });
  return hipGetLastError();
}

// Workgroup-per-row backward: dx at one row per block, then the streaming
// stripe accumulation at the stripe grid; past the register cache the wide
// kernel does both at the stripe grid.
template <typename T>
static hipError_t ln_bwd_dx_wg(const T* dy, const T* dh, const T* x, const T* w,
                               const float* mean, const float* rstd, T* dx,
                               float* pdw, float* pdb, int M, int N,
                               hipStream_t stream) {
  constexpr int W = Vec<T>::W;
  if (N % W) return hipErrorInvalidValue;  // 16B row-base alignment
  const int block = ln_block(N, W);
  const int stripes = ln_stripe_count(M, 0);
  const bool wide = N > LN_WG_MAXITER * block * W;
  const int dx_grid = wide ? stripes : ln_wg_grid(M);
  ln_with_flag(dh != nullptr, [&](auto has_dh) {
    constexpr bool HAS_DH = decltype(has_dh)::value;
    if (wide)
      hipLaunchKernelGGL((ln_bwd_dx_wide_kernel<T, HAS_DH>), dim3(dx_grid),
                         dim3(1024), 0, stream, dy, dh, x, w, mean, rstd, dx,
                         pdw, pdb, M, N);
    else
      hipLaunchKernelGGL((ln_bwd_dx_kernel<T, LN_WG_MAXITER, HAS_DH>),
                         dim3(dx_grid), dim3(block), 0, stream, dy, dh, x, w,
                         mean, rstd, dx, M, N);
  });
  if (!wide)
    hipLaunchKernelGGL((ln_dwdb_accum_kernel<T, LN_WG_MAXITER>), dim3(stripes),
                       dim3(block), 0, stream, dy, x, mean, rstd, pdw, pdb, M,
                       N);
  return hipGetLastError();
}

extern "C" {

// Geometry of the row-per-wave path for the tests and tools: forward waves
// and batch depths for this shape (0 when it is not routed) and the last
// routed bf16 N.
void tdsa_ln_rowwave_info(int M, int N, int is_bf16, int* fwd_waves,
                          int* fwd_depth, int* bwd_depth, int* bound) {
  const int nvec = ln_rw_nvec(N, is_bf16);
  *fwd_waves = nvec ? ln_rw_fwd_waves(M) : 0;
  *fwd_depth = nvec ? LN_RW_FWD_DEPTH(nvec) : 0;
  *bwd_depth = nvec ? LN_RW_BWD_DEPTH(nvec) : 0;
  *bound = LN_RW_MAXVEC * WAVE * 8;
}

// res/h: optional fused residual (pass nullptr for the plain form).
hipError_t tdsa_ln_fwd(const void* x, const void* res, void* h, const void* w,
                       const void* b, void* y, float* mean, float* rstd,
                       int M, int N, float eps, int is_bf16,
                       hipStream_t stream) {
  if (const int nvec = ln_rw_nvec(N, is_bf16)) {
    const int grid = ln_rw_fwd_waves(M) / LN_RW_WAVES;
    ln_rw_with_nvec(nvec, [&](auto nv) {
      ln_with_flag(res != nullptr, [&](auto has_res) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL(
            (ln_fwd_rowwave_kernel<bf16, decltype(has_res)::value, NV,
                                   LN_RW_FWD_DEPTH(NV)>),
            dim3(grid), dim3(LN_RW_BLOCK), 0, stream, (const bf16*)x,
            (const bf16*)res, (bf16*)h, (const bf16*)w, (const bf16*)b,
            (bf16*)y, mean, rstd, M, N, eps);
      });
    });
    return hipGetLastError();
  }
  return dispatch_dtype(is_bf16, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return ln_fwd_wg((const T*)x, (const T*)res, (T*)h, (const T*)w,
                     (const T*)b, (T*)y, mean, rstd, M, N, eps, stream);
  });
}

// G (stripe count), reported to the caller so it can size pdw/pdb. This and
// the launcher below both take it from ln_stripe_count, the single place that
// decides it.
int tdsa_ln_bwd_dx_stripes(int M, int N, int is_bf16) {
  return ln_stripe_count(M, ln_rw_nvec(N, is_bf16));
}

// dh: optional residual-stream gradient added into dx (nullptr for plain).
// Routed shapes run ln_bwd_rowwave_kernel (one pass, no accum kernel).
hipError_t tdsa_ln_bwd_dx(const void* dy, const void* dh, const void* x,
                          const void* w, const float* mean, const float* rstd,
                          void* dx, float* pdw, float* pdb, int M, int N,
                          int is_bf16, hipStream_t stream) {
  if (const int nvec = ln_rw_nvec(N, is_bf16)) {
    const int grid = ln_stripe_count(M, nvec) / LN_RW_WAVES;
    ln_rw_with_nvec(nvec, [&](auto nv) {
      ln_with_flag(dh != nullptr, [&](auto has_dh) {
        constexpr int NV = decltype(nv)::value;
        hipLaunchKernelGGL(
            (ln_bwd_rowwave_kernel<bf16, decltype(has_dh)::value, NV,
                                   LN_RW_BWD_DEPTH(NV)>),
            dim3(grid), dim3(LN_RW_BLOCK), 0, stream, (const bf16*)dy,
            (const bf16*)dh, (const bf16*)x, (const bf16*)w, mean, rstd,
            (bf16*)dx, pdw, pdb, M, N);
      });
    });
    return hipGetLastError();
  }
  return dispatch_dtype(is_bf16, [&](auto tag) {
    using T = typename decltype(tag)::type;
    return ln_bwd_dx_wg((const T*)dy, (const T*)dh, (const T*)x, (const T*)w,
                        mean, rstd, (T*)dx, pdw, pdb, M, N, stream);
  });
}

// out_bf16: write dw/db as bf16 (rounded once from the fp32 sums) instead
// of fp32.
hipError_t tdsa_ln_bwd_dwdb(const float* pdw, const float* pdb, void* dw,
                            void* db, int G, int N, int out_bf16,
                            hipStream_t stream) {
  const int grid = (N + LN_DWDB_SLAB - 1) / LN_DWDB_SLAB;
  dispatch_dtype(out_bf16, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(ln_bwd_dwdb_kernel<T>, dim3(grid), dim3(LN_DWDB_BLOCK),
                       0, stream, pdw, pdb, (T*)dw, (T*)db, G, N);
  });
  return hipGetLastError();
}

}  // extern "C"
