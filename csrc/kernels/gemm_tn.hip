// Hand-written CDNA4 TN GEMM for the Linear weight gradient:
//
//   dw[N,K] = dy[M,N]^T @ x[M,K]     (bf16 in, fp32 accumulate)
//
// The ONE GEMM shape family where the reduction dim (M = B*T, 32k typical)
// is the ROW dim of BOTH row-major operands. That makes both MFMA operands
// reachable through the same ds_read_tr16_b64 hardware-transpose read of
// row-major staged [64][64] LDS images (mfma.h: the A and B fragment
// layouts of v_mfma_f32_32x32x16_bf16 share one lane->(k-elem, 32-axis)
// map) — no transposed staging, no bank conflicts, no strided global reads.
// hipBLASLt's weakest library shape per profiles/gemm_shapes_hipblaslt.txt;
// registered as the autotuner's first candidate for linear_dw
// (ops/linear.py), so the library wins any shape where it is faster.
//
// Geometry: 4 waves / workgroup, 128(N) x 128(K) output tile; wave w owns
// the 32-row n-band [32w, 32w+32) x 128 k. Per 64-row m-chunk each wave
// issues 4 A tr-reads + 16 B tr-reads + 16 MFMAs from four 16 KB swizzled
// LDS images (dy 64x128, x 64x128), with the next chunk's global loads
// issued before the compute (fetch/put split — they fly under the MFMAs).
// The output is tiny (N*K vs M*K inputs), so workgroups additionally
// split the M reduction (grid.y); each split stores its 128x128 fp32
// partials into its own [N, K] slab of a [splits, N, K] buffer, and the
// caller sums the slabs in a fixed order and converts to bf16 (an fp32
// atomicAdd combine gave run-to-run different sums at 3+ splits).
//
//
// Contract: bf16, contiguous, any M >= 1, N % 64 == 0, K % 64 == 0. Shapes
// with M % 64 == 0, N % 128 == 0 and K % 128 == 0 run gemm_tn_kernel, whose
// code knows no edge; every other shape runs the EDGE instantiations (see
// the kernel).
//
// Reference hot path being replaced:
// /root/reference/tiny_deepspeed/core/module/ops/linear.py:59-68.
#include "common.h"
#include "launchers.h"
#include "mfma.h"

#include <cstdlib>

namespace tdsa {

// XCD-group remap: the dispatcher places linear block b on XCD b % 8 with
// x varying fastest, so the tiles_k workgroups that share one (tn, split)
// — and therefore stream the SAME dy column-slice — would land on 8
// different XCDs' L2s and fetch it 8x from HBM. Remap so they share an
// XCD. Bijective when tiles_n * splits % 8 == 0; identity otherwise.
DEV_INLINE void tn_remap(int gx, int gy, int& tile, int& split, int tiles_k) {
  const int groups = (gx / tiles_k) * gy;  // (tn, split) pairs
  if (groups % 8) return;
  const long long id = (long long)split * gx + tile;
  const long long window = 8LL * tiles_k;
  const int g = (int)((id / window) * 8 + (id % 8));
  const int tk = (int)((id % window) / 8);
  const int tn = g / gy;
  split = g % gy;
  tile = tn * tiles_k + tk;
}

// Supertile remap (mode 2): group tiles into 2(tn) x 4(tk) rectangles and
// place each rectangle's 8 tiles on ONE XCD (ids congruent mod 8 within a
// 64-id window) — the XCD's L2 then re-serves both dy slices (2) and x
// slices (4) instead of streaming 8 distinct slice pairs. Needs
// tiles_n % 2 == 0, tiles_k % 4 == 0 and (supertiles * splits) % 8 == 0.
DEV_INLINE void tn_remap2(int gx, int gy, int& tile, int& split,
                          int tiles_k) {
  const int tiles_n = gx / tiles_k;
  if (tiles_n % 2 || tiles_k % 4) return;
  const int sn = tiles_n >> 1, sk = tiles_k >> 2;
  if ((sn * sk * gy) % 8) return;
  const long long id = (long long)split * gx + tile;
  const long long w = id >> 6;        // 64-id window
  const int s_local = (int)(id & 7);  // supertile within window (XCD)
  const int t_local = (int)((id & 63) >> 3);  // tile within supertile
  const long long sup = w * 8 + s_local;
  const int per_split = sn * sk;
  split = (int)(sup / per_split);
  const int ss = (int)(sup % per_split);
  const int tn = (ss / sk) * 2 + (t_local >> 2);
  const int tk = (ss % sk) * 4 + (t_local & 3);
  tile = tn * tiles_k + tk;
}

// EDGE, 4 waves: image i of {dy lo, dy hi, x lo, x hi} exists.
DEV_INLINE bool tn_has(int i, bool dy_hi, bool x_hi) {
  return (i != 1 || dy_hi) && (i != 3 || x_hi);
}

// NW waves; output tile (NW*32) x 128. Wave w owns n-band [32w, 32w+32) x
// 128 k. NW=8 halves the staged bytes per FLOP vs NW=4 (the dy slice is
// amortized over twice the MFMA work) — used when N % 256 == 0.
//
// EDGE (NW = 4 only): M % 64, N % 128 or K % 128 is not zero. N and K are
// still multiples of 64, the granule of one LDS image, so an edge is a whole
// missing image and every guard below is a block- or wave-uniform scalar:
//   - tile counts are rounded up; a workgroup on the last tile row (column)
//     may have ONE dy (x) image. The operands are contiguous, so "columns
//     N .. N+63 of row r" would be the start of row r+1 and, past the last
//     row, not memory: a missing image is neither fetched nor put nor read
//     from LDS. Waves 2 and 3 (its n-bands) skip the MFMA loop and keep both
//     barriers; all waves skip dt = 2, 3 without the second x image;
//   - splits stay multiples of 64 rows, so only the last chunk of the split
//     that owns row M-1 has left < 64 rows. It is fetched by
//     Stage::fetch_rows: rows >= left are not read and are zeros in the
//     registers and so in LDS, in BOTH operands, and the MFMAs add 0 * 0
//     (a zero times a NaN from memory the caller does not own would be NaN).
//     Every output element therefore sums the products of the aligned kernel
//     on the zero-padded problem, in its order, plus exact zeros;
//   - stores are guarded per (wave, dt): nothing outside [N, K] of a slab is
//     written; a split that starts at or beyond M stores zeros, as always.
// tn_remap / tn_remap2 run on the rounded-up tile counts: their conditions
// (groups % 8; tiles_n % 2, tiles_k % 4, supertiles * splits % 8) are
// conditions on tiles_n, tiles_k and gridDim.y alone, and the grid is
// exactly tiles_n * tiles_k x splits, so the maps stay bijections.
template <int NW, bool SPLIT, bool EDGE = false>
__launch_bounds__(NW * WAVE)
__global__ void gemm_tn_kernel(const bf16* __restrict__ dy,
                               const bf16* __restrict__ x,
                               float* __restrict__ dw, long long M, int N,
                               int K, long long m_per_split, int remap) {
  static_assert(!EDGE || NW == 4, "edge shapes take the 4-wave tile");
  const int tiles_k = EDGE ? (K + 127) >> 7 : K >> 7;
  int tile = blockIdx.x;
  int split = blockIdx.y;
  if (remap == 2)
    tn_remap2(gridDim.x, gridDim.y, tile, split, tiles_k);
  else if (remap)
    tn_remap(gridDim.x, gridDim.y, tile, split, tiles_k);
  const int tn = tile / tiles_k;
  const int tk = tile % tiles_k;
  const int n0 = tn * (NW * 32);
  const int k0 = tk << 7;
  const long long m_begin = (long long)split * m_per_split;
  long long m_end = m_begin + m_per_split;
  if (m_end > M) m_end = M;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid >> 6;
  const int h32 = lane >> 5;

  constexpr int NT = NW * WAVE;
  constexpr int NIMG = NW / 2 + 2;         // dy images + 2 x images
  constexpr int IMG = 64 * 128;            // one swizzled [64][64] tile, 8 KB
  __shared__ char lds[NIMG * IMG];

  // images 0..NW/2-1: dy 64-col slices; images NW/2, NW/2+1: x lo/hi
  Stage<NT> st[NIMG];
#pragma unroll
  for (int i = 0; i < NW / 2; ++i)
    st[i].init(dy + m_begin * N + n0 + 64 * i, tid, N);
  st[NW / 2].init(x + m_begin * K + k0, tid, K);
  st[NW / 2 + 1].init(x + m_begin * K + k0 + 64, tid, K);
  // EDGE: the second dy / x image exists (block-uniform); tn_has: image i
  // does. The Stage of a missing image holds addresses that are never used.
  bool dy_hi = true, x_hi = true;
  if constexpr (EDGE) {
    dy_hi = n0 + 64 < N;
    x_hi = k0 + 64 < K;
  }

  int trb[2][2];
  tr_bases(lane, trb);
  const char* a_img = lds + (wave >> 1) * IMG;
  const int dta = wave & 1;

  f32x16 acc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[dt][r] = 0.f;

  int nchunks = m_end > m_begin ? (int)((m_end - m_begin) >> 6) : 0;
  long long rows = 0;  // EDGE: rows of this split (<= 0: none), last chunk
  if constexpr (EDGE) {  // may be ragged
    rows = m_end - m_begin;
    nchunks = rows > 0 ? (int)((rows + 63) >> 6) : 0;
  }
  // EDGE: this wave's n-band lies inside N (wave-uniform, made scalar)
  bool band = true;
  if constexpr (EDGE)
    band = dy_hi || __builtin_amdgcn_readfirstlane(wave) < 2;
  if (nchunks > 0) {
    if (!EDGE || rows >= 64) {
#pragma unroll
      for (int i = 0; i < NIMG; ++i) {
        if (EDGE && !tn_has(i, dy_hi, x_hi)) continue;
        st[i].run(lds + i * IMG);
        st[i].advance();
      }
    } else {  // the only chunk of the split is the ragged one
#pragma unroll
      for (int i = 0; i < NIMG; ++i) {
        if (EDGE && !tn_has(i, dy_hi, x_hi)) continue;
        short8v first[Stage<NT>::REPS];
        st[i].fetch_rows(first, tid, (int)rows);
        st[i].put(lds + i * IMG, first);
      }
    }
  }
  for (int c = 0; c < nchunks; ++c) {
    __syncthreads();
    short8v pend[NIMG][Stage<NT>::REPS];
    const bool more = c + 1 < nchunks;
    if (more) {
      if constexpr (EDGE) {
        // rows of the next chunk; < 64 only for the chunk that holds row M-1
        const long long left = rows - ((long long)(c + 1) << 6);
        if (left >= 64) {
#pragma unroll
          for (int i = 0; i < NIMG; ++i)
            if (tn_has(i, dy_hi, x_hi)) st[i].fetch(pend[i]);
        } else {
#pragma unroll
          for (int i = 0; i < NIMG; ++i)
            if (tn_has(i, dy_hi, x_hi))
              st[i].fetch_rows(pend[i], tid, (int)left);
        }
      } else {
#pragma unroll
        for (int i = 0; i < NIMG; ++i) st[i].fetch(pend[i]);
      }
    }
    if (!EDGE || band) {
#pragma unroll
      for (int S = 0; S < 4; ++S) {
        const bfrag a = tr_bfrag(a_img, trb[dta][0] + S * 2048,
                                 trb[dta][1] + S * 2048);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          if (EDGE && dt == 2 && !x_hi) break;
          const bfrag b = tr_bfrag(lds + (NW / 2 + (dt >> 1)) * IMG,
                                   trb[dt & 1][0] + S * 2048,
                                   trb[dt & 1][1] + S * 2048);
          acc[dt] = MFMA32(a, b, acc[dt]);
        }
      }
    }
    __syncthreads();
    if (more) {
#pragma unroll
      for (int i = 0; i < NIMG; ++i) {
        if (EDGE && !tn_has(i, dy_hi, x_hi)) continue;
        st[i].put(lds + i * IMG, pend[i]);
        st[i].advance();
      }
    }
  }

  // epilogue: C[32x32] lane l reg r -> row crow(r,h32), col l%32
  // SPLIT: this M-split's partial goes to its own [N, K] slab of the
  // [splits, N, K] buffer; the caller adds the slabs in a fixed order
  // EDGE: per (wave, dt) only what lies inside [N, K]
  const int col = k0 + (lane & 31);
  if (SPLIT) dw += (long long)split * N * K;
  if (EDGE && !band) return;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    if (EDGE && dt == 2 && !x_hi) break;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long idx =
          (long long)(n0 + wave * 32 + crow(r, h32)) * K + col + dt * 32;
      dw[idx] = acc[dt][r];
    }
  }
}

}  // namespace tdsa

using namespace tdsa;

extern "C" {

// Shapes that the aligned kernels do not take: one of the three dims ends
// inside a tile or chunk.
static bool tn_edge(long long M, int N, int K) {
  return (M & 63) || (N & 127) || (K & 127);
}

// Tile height: 4 waves / 128 rows measured BEST (the 8-wave 256-row tile
// variant lost 10-20% on every shape despite doubled staging intensity —
// gemm_tn v2 against v1 sweeps); 8 kept behind the env for re-testing, for
// aligned shapes only: edge shapes always take 4 waves.
static int tn_nw(int N, bool edge) {
  int nw = 4;
  if (edge) return nw;
  if (const char* v = getenv("TDSA_GEMM_TN_NW")) {
    int e = atoi(v);
    if ((e == 4 || e == 8) && N % (e * 32) == 0) nw = e;
  }
  return nw;
}

// Output tiles along N (rounded up: the last may be half a tile).
static int tn_tiles_n(int N, int nw) { return (N + nw * 32 - 1) / (nw * 32); }

// Returns the split count the launcher will use (the caller sizes the fp32
// buffer as [splits, N, K]); <=0 means shape unsupported: the contract is
// M >= 1, N % 64 == 0, K % 64 == 0.
int tdsa_gemm_tn_splits(long long M, int N, int K) {
  if (M < 1 || N < 64 || K < 64 || (N & 63) || (K & 63)) return 0;
  const int nw = tn_nw(N, tn_edge(M, N, K));
  const long long tiles = (long long)tn_tiles_n(N, nw) * ((K + 127) >> 7);
  // ~512 total workgroups (2 per CU): the splits sweep measured 8 splits
  // at 64 tiles (512 wgs) 25% faster than 32 splits — more splits just
  // multiply the fp32 partial traffic once every CU has work. (That sweep
  // combined partials with atomicAdd; with one slab per split the heuristic
  // is kept and each extra split costs one more [N, K] fp32 slab to store
  // and sum.)
  long long want = (512 + tiles - 1) / tiles;
  long long maxs = (M + 63) >> 6;  // at least one 64-chunk per split
  if (want > maxs) want = maxs;
  if (const char* v = getenv("TDSA_GEMM_TN_SPLITS")) want = atoll(v);
  // the caller allocates splits * N * K fp32: cap the workspace at 1 GiB
  // (heuristic shapes need at most 64 slabs of 128x128; this bounds the
  // override)
  const long long slab = (long long)N * K * 4;
  if (want * slab > (1ll << 30)) want = (1ll << 30) / slab;
  if (want < 1) want = 1;
  return (int)want;
}

hipError_t tdsa_gemm_tn(const void* dy, const void* x, float* dw, long long M,
                        int N, int K, hipStream_t stream) {
  const int splits = tdsa_gemm_tn_splits(M, N, K);
  if (splits <= 0) return hipErrorInvalidValue;
  const bool edge = tn_edge(M, N, K);
  const int nw = tn_nw(N, edge);
  // splits are whole 64-row chunks; the last chunk of M may be ragged
  const long long chunks_per_split = (((M + 63) >> 6) + splits - 1) / splits;
  const long long m_per_split = chunks_per_split << 6;
  // mode 2 (supertile) measured +1-5% across shapes; mode 1 (tn-group)
  // neutral — the chip-wide Infinity Cache already serves shared slices,
  // so XCD placement only trims the L2-miss tail
  int remap = 2;
  if (const char* v = getenv("TDSA_GEMM_TN_REMAP")) remap = atoi(v);
  dim3 grid(tn_tiles_n(N, nw) * ((K + 127) >> 7), splits);
#define TN_LAUNCH(KERNEL, NWV)                                              \
  hipLaunchKernelGGL(KERNEL, grid, dim3(NWV * WAVE), 0, stream,             \
                     (const bf16*)dy, (const bf16*)x, dw, M, N, K,          \
                     m_per_split, remap)
  if (edge) {
    if (splits == 1) TN_LAUNCH((gemm_tn_kernel<4, false, true>), 4);
    else TN_LAUNCH((gemm_tn_kernel<4, true, true>), 4);
  } else if (nw == 8) {
    if (splits == 1) TN_LAUNCH((gemm_tn_kernel<8, false>), 8);
    else TN_LAUNCH((gemm_tn_kernel<8, true>), 8);
  } else {
    if (splits == 1) TN_LAUNCH((gemm_tn_kernel<4, false>), 4);
    else TN_LAUNCH((gemm_tn_kernel<4, true>), 4);
  }
#undef TN_LAUNCH
  return hipGetLastError();
}

}  // extern "C"
