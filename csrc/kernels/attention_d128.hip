// Fused causal attention for head dim 128 (bf16, any T >= 1).
// T % 64 == 0 runs the kernels described here; any other T their tail
// variants ("Ragged T" above the first tail kernel), which handle the partial
// last tile and read or write no row >= T. With dropout either runs as its
// DROP instantiation ("Dropout" above the first of those kernels).
// k and v with fewer heads than q run the grouped-query kernels
// ("Grouped-query" above them; no dropout).
//
// Same scheme and number formats as attention.hip (head dim 64): forward with
// online softmax in exp2 space and a natural-log lse; backward in two kernels
// without atomics, dq first (it publishes delta = rowsum(dO*O)), then dk/dv.
// The three conventions are kept, so the same error model holds: swapped
// S^T = mfma(K, Q) (a softmax row lives in one lane pair), P and dS from C
// layout to A fragments through v_permlane32_swap, Q (K in dk/dv) prescaled by
// scale*log2e and rounded to bf16. scale is 2^-3.5 here: the prescale is NOT
// exact, which the error model already covers (it rounds q*scale*log2e).
// The skeleton (BlockCtx, tile_map, TilePipe, RowPipe, FragOff, PackedC) is
// attn_common.h, shared with attention.hip.
//
// Operand tiles: a 64-row K, V, Q or dO tile is 64 x 128 bf16 = TWO swizzled
// [64][64] images of mfma.h side by side in LDS (columns 0-63, then 64-127,
// IMG bytes apart). One TilePipe stages the two images of one tensor: its
// "pair" is (left half, right half) of the same 64 rows. A fragment or a
// transpose read of d-slice s / column tile dt picks the image by s >> 2 /
// dt >> 1 and uses the unchanged [64][64] offsets inside it.
//
// Geometry: what does not carry over from head dim 64 is the register budget.
// A wave keeps 32 rows as before, and per wave the live state is
//   fwd : O 64 fp32 + Q fragments 32 + S^T 32 + staging
//   dq  : dQ 64 + Q, dO fragments 64 + S^T, dP^T 32 + dS 16 + staging
//   dkv : dK, dV 128 + K, V fragments 64 + S, dP 32 + P, dS 32 + staging
// An 8-wave block (2 waves per SIMD) caps a lane at 256 registers, which dkv
// exceeds before staging. So every kernel here runs 4-WAVE blocks (128 rows;
// 2-wave blocks where T % 128 != 0): one wave per SIMD and block, up to 512
// registers with the AGPR half, K and V (Q, dO) fragments stay pinned in
// registers and the staging cost of a tile is shared by 4 waves instead of 8.
// The price is occupancy: a CU holds as many blocks as 512 / registers allows
// (docs/kernels.md, "Head dim 128" has the counts); dkv is left with one wave
// per SIMD and hides its softmax behind nothing but its own MFMA queue.
//
// MFMA per 64-row tile and wave: fwd 16 (S^T: 8 d-slices x 2 key halves) + 16
// (O: 4 key slices x 4 column tiles); dq 32 + 16; dkv 32 + 32.
//
// LDS: two 64 x 128 tiles (32 KB) per block, plus lse/delta of a Q tile in
// dkv. The epilogue images (one [32][128] bf16 image per wave, whole 256-byte
// rows out) reuse the tile space after a block barrier: every wave of a block
// runs the same number of loop iterations, so the barrier costs no waiting
// that the loop's own barriers had not already imposed.
#include "common.h"
#include "launchers.h"
#include "attn_common.h"
#include "mfma.h"

#include <type_traits>

namespace tdsa {

// The kernels are compiled without packed fp32 math, the project's choice for
// attention kernels since the tail kernels of attention.hip, whose packed
// build measured slower (profiles/attn_ragged.txt: fwd 139 against 127 us).
// A packed build of these kernels has not been measured.
#if defined(__HIP_DEVICE_COMPILE__)
#define NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define NO_PK_F32
#endif

constexpr int IMG = KVB * 64 * 2;    // bytes of one swizzled [64][64] image
constexpr int TILE128 = 2 * IMG;     // a 64 x 128 tile: two images
constexpr int STAGE128 = 32 * 128 * 2;   // a wave's [32][128] epilogue image
constexpr int HALF = 64;             // elements from a row's left to right half

// Stages one tensor's 64 x 128 tiles: image 0 <- columns 0-63, 1 <- 64-127.
// TAIL: `left` rows of the first tile exist. The pipe's two stages are the
// halves of the SAME 64 rows, so its one row count serves both.
template <int NT, bool TAIL = false>
DEV_INLINE TilePipe<NT, TAIL> tile128_pipe(const bf16* g, int st, int tid,
                                           int left = 0) {
  return TilePipe<NT, TAIL>(g, st, g + HALF, st, tid, left);
}

// TilePipe::next for the two tensors of a loop at once, under ONE barrier
// (each pipe's own next() would bring its own): barrier (the previous tiles
// are consumed), pending registers -> LDS, and with `more` the loads of the
// following tiles. `rows` rides along as in TilePipe::next. The caller places
// the barrier that publishes the tiles. TAIL: this takes TilePipe::next's
// place, so it steps each pipe's row count before the fetch as next() does.
template <int NT, bool TAIL,
          typename Rows = typename TilePipe<NT, TAIL>::NoRows>
DEV_INLINE void next_tiles128(TilePipe<NT, TAIL>& x, char* lds_x,
                              TilePipe<NT, TAIL>& y, char* lds_y, bool more,
                              Rows&& rows = Rows{}) {
  __syncthreads();
  x.a.put(lds_x, x.pend_a);
  x.b.put(lds_x + IMG, x.pend_b);
  y.a.put(lds_y, y.pend_a);
  y.b.put(lds_y + IMG, y.pend_b);
  rows.put();
  if (more) {
    x.a.advance();
    x.b.advance();
    y.a.advance();
    y.b.advance();
    if constexpr (TAIL) {
      x.left -= KVB;
      y.left -= KVB;
    }
    x.fetch();
    y.fetch();
    rows.advance();
    rows.fetch();
  }
}

// Pinned B operands of one row: d-slices 0..7, optionally prescaled.
// TAIL: a row that does not exist (`ok` false) is not read and is all zeros.
template <bool TAIL = false>
DEV_INLINE void load_row_frags(bfrag (&f)[8], const bf16* p, int row, int h32,
                               int st, bool ok = true) {
#pragma unroll
  for (int s = 0; s < 8; ++s)
    f[s] = load_frag<TAIL>(p, row, s * 16 + 8 * h32, st, ok);
}

template <bool TAIL = false>
DEV_INLINE void load_row_frags_scaled(bfrag (&f)[8], const bf16* p, int row,
                                      int h32, int st, float mul,
                                      bool ok = true) {
#pragma unroll
  for (int s = 0; s < 8; ++s)
    f[s] = load_frag_scaled<TAIL>(p, row, s * 16 + 8 * h32, st, mul, ok);
}

// acc = A(32-row half t2 of the tile at `lds`) x B(pinned row fragments),
// reduced over all 128 columns: 8 MFMA.
DEV_INLINE f32x16 mfma_rows_d128(const char* lds, const FragOff& fo, int t2,
                                 const bfrag (&b)[8], const f32x16& zero) {
  f32x16 acc = MFMA32(lds_read16(lds, fo(t2, 0)), b[0], zero);
#pragma unroll
  for (int s = 1; s < 8; ++s)
    acc = MFMA32(lds_read16(lds + (s >> 2) * IMG, fo(t2, s & 3)), b[s], acc);
  return acc;
}

// The same with the B rows read from LDS as well: 32-row band tb of the
// TILES (prescaled) tiles at `lds_b`, one after the other (the 2-wave dkv
// kernel, whose staging registers leave no room for pinned fragments: one
// tile, band = half; the 4-wave DROP dkv kernel: two tiles, four bands).
template <int TILES = 1>
DEV_INLINE f32x16 mfma_rows_d128(const char* lds, const FragOff& fo, int t2,
                                 const char* lds_b, int tb,
                                 const f32x16& zero) {
  // tb is a run-time value (the wave index): half tb is 32 rows of 128 bytes
  // past half 0. Indexing FragOff's row[] with it made the compiler move
  // the struct to LDS (2 KB per block).
  if constexpr (TILES > 1) {
    lds_b += (tb >> 1) * TILE128;
    tb &= 1;
  }
  lds_b += tb * (32 * 128);
  f32x16 acc = MFMA32(lds_read16(lds, fo(t2, 0)), lds_read16(lds_b, fo(0, 0)),
                      zero);
#pragma unroll
  for (int s = 1; s < 8; ++s)
    acc = MFMA32(lds_read16(lds + (s >> 2) * IMG, fo(t2, s & 3)),
                 lds_read16(lds_b + (s >> 2) * IMG, fo(0, s & 3)), acc);
  return acc;
}

// One-shot staging of the 64 x 128 tile at g (row stride st) times mul,
// rounded to bf16, as two swizzled images at lds: 1024 chunks over NT threads.
// TAIL: the tile has only its first `rows` rows (>= 1); a chunk of a later
// row is not read and is zeros in LDS.
template <int NT, bool TAIL = false>
DEV_INLINE void stage_tile128_scaled(char* lds, const bf16* g, int st, int tid,
                                     float mul, int rows = KVB) {
#pragma unroll
  for (int rep = 0; rep < 1024 / NT; ++rep) {
    const int chunk = tid + rep * NT;
    const int row = chunk >> 4, piece = chunk & 15;
    const bf16* src = g + (long long)row * st + piece * 8;
    short8v v = {};
    if constexpr (TAIL) {
      if (row < rows) v = load8(src);
    } else {
      v = load8(src);
    }
    short8v w;
#pragma unroll
    for (int e = 0; e < 8; ++e) w[e] = bf_pack(bf_elem(v, e) * mul);
    *reinterpret_cast<short8v*>(lds + (piece >> 3) * IMG +
                                swz(row, (piece & 7) * 16)) = w;
  }
}

// acc[dt] += A-fragment `a` (k = rows 16s..16s+15 of the tile) x the tile's
// 32-column tile dt, read transposed: 4 MFMA.
DEV_INLINE void mfma_cols_d128(f32x16 (&acc)[4], const bfrag& a,
                               const char* lds, const int (&trb)[2][2], int s) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    acc[dt] = MFMA32(a, tr_bfrag(lds + (dt >> 1) * IMG,
                                 trb[dt & 1][0] + s * 2048,
                                 trb[dt & 1][1] + s * 2048),
                     acc[dt]);
}

// Epilogue of one wave's 32 x 128 result (four C tiles): element
// (crow(r,h32), 32*dt + x32) = acc[dt][r] * mul(r) as bf16, through the
// wave's own [32][128] LDS image and out as whole 256-byte rows (16 lanes x
// 16 bytes, 4 rows per store instruction, 8 instructions).
// TAIL: only the wave's first `rows` rows (any value; <= 0: none) exist and
// are stored.
template <bool TAIL = false, typename F>
DEV_INLINE void store_ctiles128(bf16* p, int st, const BlockCtx& c,
                                const f32x16 (&acc)[4], F mul, char* stage,
                                int rows = 32) {
  bf16* img = reinterpret_cast<bf16*>(stage);
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      img[crow(r, c.h32) * 128 + dt * 32 + c.x32] = f2bf(acc[dt][r] * mul(r));
  wave_lds_fence();
  const int piece = c.lane & 15;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int row = 4 * i + (c.lane >> 4);
    if constexpr (TAIL) {
      if (row >= rows) continue;
    }
    store8(p + row * st + piece * 8,
           *reinterpret_cast<const short8v*>(stage + row * 256 + piece * 16));
  }
  wave_lds_fence();   // the image is free for this wave's next result
}

// The tile functions below take the Dropout as a parameter pack, `drop_arg`:
// empty in the kernels without dropout, one Dropout in the DROP kernels. A
// plain parameter, even one that nothing reads, changed the register
// allocation of the forward and dkv kernels without dropout.
DEV_INLINE const Dropout& the_dropout(const Dropout& d) { return d; }

// Grouped-query attention ("Grouped-query" above the GQA kernels) rides in
// the same pack: one KvHeads in the GQA kernels, which have no DROP form.
// G = H / Hkv query heads share K/V head h / G, so the K/V head of query
// (batch, head) bh is bh / G of B * Hkv, addressed through k's and v's own
// strides sk.
struct KvHeads {
  int G, Hkv;
  GStride sk;
};
DEV_INLINE const KvHeads& the_kv_heads(const KvHeads& h) { return h; }
template <typename T, typename... Pack>
constexpr bool pack_has = (std::is_same_v<T, Pack> || ...);

// Waves per SIMD that the forward and dq kernels are compiled for. 2 holds
// the 4-wave kernels to 256 registers (left alone the compiler takes 316 and
// 344 of the 512 a lone wave may have, and a CU then holds one block, not
// two). The 2-wave kernels stage twice as much per thread and spill under
// that cap, so they keep the full file (363 and 392).
constexpr int fwd_dq_waves_per_simd(int nw) { return nw == 4 ? 2 : 1; }

// ---------------------------------------------------------------------------
// Forward: one workgroup per (NW*32)-row Q block; wave w owns 32 rows.
// ---------------------------------------------------------------------------
// TAIL: ragged T, see "Ragged T" above the tail kernels.
// DROP: fused dropout, see "Dropout" above the DROP kernels.
template <int NW, bool TAIL, typename... Drop>
DEV_INLINE void d128_fwd_tile(const BlockCtx& c, char* smem,
                              const bf16* __restrict__ q,
                              const bf16* __restrict__ k,
                              const bf16* __restrict__ v,
                              bf16* __restrict__ o, float* __restrict__ lse,
                              int T, int H, float scale, const GStride& sq,
                              const GStride& so, const Drop&... drop_arg) {
  constexpr bool DROP = pack_has<Dropout, Drop...>;
  constexpr bool GQA = pack_has<KvHeads, Drop...>;
  constexpr int BM = NW * 32;
  constexpr int NT = NW * WAVE;
  char* lds_k = smem;
  char* lds_v = smem + TILE128;

  const long long boff = c.base(sq, H);
  const int row_lo = c.tile * BM + c.w * 32;
  const int row_me = row_lo + c.x32;
  // dropout index base of this pass's row: idx = base + key
  unsigned long long drop_base = 0;
  if constexpr (DROP) drop_base = ((unsigned long long)c.bh * T + row_me) * T;

  // K and V of this block's head; GQA: of K/V head bh / G, through sk
  long long koff = boff;
  int kst = sq.t;
  if constexpr (GQA) {
    const KvHeads& kvh = the_kv_heads(drop_arg...);
    const int kvbh = (int)c.bh / kvh.G;   // B * H fits an int: grid y
    koff = (long long)(kvbh / kvh.Hkv) * kvh.sk.b +
           (long long)(kvbh % kvh.Hkv) * kvh.sk.h;
    kst = kvh.sk.t;
  }
  auto pipe_k = tile128_pipe<NT, TAIL>(k + koff, kst, c.tid, T);
  auto pipe_v = tile128_pipe<NT, TAIL>(v + koff, kst, c.tid, T);
  const FragOff kf(c);
  int trb[2][2];
  tr_bases(c.lane, trb);
  bfrag q_frag[8];
  load_row_frags_scaled<TAIL>(q_frag, q + boff, row_me, c.h32, sq.t,
                              scale * LOG2E, row_me < T);

  const f32x16 kzero = {};
  f32x16 o_acc[4] = {};
  float m_run = -INFINITY;
  float l_run = 0.f;

  const int n_kv = (c.tile + 1) * BM / KVB;
  pipe_k.prime();
  pipe_v.prime();
  for (int j = 0; j < n_kv; ++j) {
    next_tiles128(pipe_k, lds_k, pipe_v, lds_v, j + 1 < n_kv);
    __syncthreads();

    const int key0 = j * KVB;
    if (key0 > row_lo + 31) continue;
    if constexpr (TAIL) {
      if (row_lo >= T) continue;   // a wave of padded rows only
    }

    // S^T tiles: C[key = 32*t2 + crow(r,h32)][qrow = x32], log2-scaled
    f32x16 st[2];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
      st[t2] = mfma_rows_d128(lds_k, kf, t2, q_frag, kzero);
    __builtin_amdgcn_s_setprio(0);

    const bool diag = key0 + KVB - 1 > row_lo;
    float mt = -INFINITY;
    if (diag) {
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = key0 + t2 * 32 + crow(r, c.h32);
          float s = (key <= row_me) ? st[t2][r] : -INFINITY;
          st[t2][r] = s;
          mt = fmaxf(mt, s);
        }
    } else {
#pragma unroll
      for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int r = 0; r < 16; ++r) mt = fmaxf(mt, st[t2][r]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32, WAVE));
    const float m_new = fmaxf(m_run, mt);
    const float alpha = fast_exp2(m_run - m_new);
    float psum = 0.f;
    PackedC P;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
      for (int r1 = 0; r1 < 4; ++r1) {
        float p[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          p[e] = fast_exp2(st[t2][4 * r1 + e] - m_new);
          psum += p[e];   // the row sum is the undropped one: lse as without
          if constexpr (DROP) {
            const Dropout& drop = the_dropout(drop_arg...);
            const int key = key0 + t2 * 32 + crow(4 * r1 + e, c.h32);
            p[e] = pin(drop.keep(drop_base + key) ? p[e] * drop.inv_keep : 0.f);
          }
        }
        P.wA[t2][r1] = pack2(p[0], p[1]);
        P.wB[t2][r1] = pack2(p[2], p[3]);
      }
    psum += __shfl_xor(psum, 32, WAVE);
    l_run = l_run * alpha + psum;
    m_run = m_new;

    if (__any(alpha != 1.0f)) {
      float a_row[16];
#pragma unroll
      for (int r = 0; r < 16; ++r)
        a_row[r] = __shfl(alpha, crow(r, c.h32), WAVE);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[dt][r] *= a_row[r];
    }

    // O[qrow][d] += P V  (A-frag k = key)
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 4; ++s)
      mfma_cols_d128(o_acc, frag_from_packed(P, s), lds_v, trb, s);
    __builtin_amdgcn_s_setprio(0);
  }

  __syncthreads();   // K/V tiles are consumed: their space holds the images
  const BlockCtx e = c.fresh_lane();
  float linv_row[16];
#pragma unroll
  for (int r = 0; r < 16; ++r)
    linv_row[r] = fast_rcp(__shfl(l_run, crow(r, e.h32), WAVE));
  const int erow_lo = e.tile * BM + e.w * 32;
  store_ctiles128<TAIL>(o + e.base(so, H) + (long long)erow_lo * so.t, so.t,
                        e, o_acc, [&](int r) { return linv_row[r]; },
                        smem + e.w * STAGE128, T - erow_lo);
  if (e.lane < 32 && (!TAIL || erow_lo + e.x32 < T))
    lse[e.bh * T + erow_lo + e.x32] = (m_run + log2f(l_run)) * LN2;
}

template <int NW>
__launch_bounds__(NW * WAVE, fwd_dq_waves_per_simd(NW))
NO_PK_F32
__global__ void attn_d128_fwd_kernel(const bf16* __restrict__ q,
                                     const bf16* __restrict__ k,
                                     const bf16* __restrict__ v,
                                     bf16* __restrict__ o,
                                     float* __restrict__ lse, int T, int H,
                                     float scale, GStride sq, GStride so,
                                     int balance) {
  static_assert(NW * STAGE128 <= 2 * TILE128, "epilogue images reuse the tiles");
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE128];
  BlockCtx c(T / (NW * 32), balance, true);
  do {
    d128_fwd_tile<NW, false>(c, smem, q, k, v, o, lse, T, H, scale, sq, so);
  } while (c.next_pass());
}

// Ragged T (T % 64 != 0): the tail kernels. They are the kernels of this file
// with TAIL set in their tile functions, on ceil(T / (NW*32)) blocks along T,
// NW chosen for T rounded up to 64 (so NW*32 divides that, every K/V or Q/dO
// loop ends at ceil(T/64) tiles and its last tile is the one that holds row
// T-1). Rows >= T of a (batch, head) do not exist: in the packed layout "row
// T" is row 0 of the next batch, and past the last batch it is not memory. So
//   - no global read touches a row >= T: streamed chunks (TilePipe<NT, true>,
//     whose row count next_tiles128 steps), pinned fragments
//     (load_row_frags*<true>), the 2-wave dkv's own K and V
//     (stage_tile128_scaled<NT, true>) and lse/delta (RowPipe<true>, the dq
//     prologue) are predicated and arrive as zeros (lse: +inf);
//   - nothing is stored to a row >= T (store_ctiles128<true>, lse, delta);
//   - a wave whose 32 rows (keys in dkv) are all >= T skips its compute and
//     keeps every barrier, like a wave above the diagonal.
// A padded key is above the diagonal of every row < T, and a padded row adds
// P = exp2(0 - inf) = 0 and dS = 0 * (0 - 0) = 0 times Q = 0, dO = 0 to dK/dV
// of the keys < T: exact zeros, so rows < T carry the bits of the aligned
// kernels on the problem zero-padded to ceil64(T) (same NW by construction).
// Separate __global__ functions, so that they can take launch bounds of
// their own; they fit the aligned kernels' (docs/kernels.md has the table).
template <int NW>
__launch_bounds__(NW * WAVE, fwd_dq_waves_per_simd(NW))
NO_PK_F32
__global__ void attn_d128_fwd_tail_kernel(const bf16* __restrict__ q,
                                          const bf16* __restrict__ k,
                                          const bf16* __restrict__ v,
                                          bf16* __restrict__ o,
                                          float* __restrict__ lse, int T,
                                          int H, float scale, GStride sq,
                                          GStride so, int balance) {
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE128];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, true);
  do {
    d128_fwd_tile<NW, true>(c, smem, q, k, v, o, lse, T, H, scale, sq, so);
  } while (c.next_pass());
}

// ---------------------------------------------------------------------------
// Backward dQ: one workgroup per (NW*32)-row Q block; wave w owns 32 rows.
// Computes and publishes delta for the dkv kernel, which runs after it.
// ---------------------------------------------------------------------------
template <int NW, bool TAIL, typename... Drop>
DEV_INLINE void d128_bwd_dq_tile(const BlockCtx& c, char* smem,
                                 const bf16* __restrict__ q,
                                 const bf16* __restrict__ k,
                                 const bf16* __restrict__ v,
                                 const bf16* __restrict__ o,
                                 const bf16* __restrict__ dout,
                                 const float* __restrict__ lse,
                                 float* __restrict__ delta,
                                 bf16* __restrict__ dq, int T, int H,
                                 float scale, const GStride& sq,
                                 const GStride& so, const GStride& sd,
                                 const Drop&... drop_arg) {
  constexpr bool DROP = pack_has<Dropout, Drop...>;
  constexpr bool GQA = pack_has<KvHeads, Drop...>;
  constexpr int BM = NW * 32;
  constexpr int NT = NW * WAVE;
  char* lds_k = smem;
  char* lds_v = smem + TILE128;

  const long long boff = c.base(sq, H);
  const long long ooff = c.base(so, H);
  const int row_lo = c.tile * BM + c.w * 32;
  const int row_me = row_lo + c.x32;

  // TAIL: this lane's row exists
  const bool row_ok = !TAIL || row_me < T;
  // dropout index base of this pass's row: idx = base + key
  unsigned long long drop_base = 0;
  if constexpr (DROP) drop_base = ((unsigned long long)c.bh * T + row_me) * T;

  // K and V of this block's head; GQA: of K/V head bh / G, through sk
  long long koff = boff;
  int kst = sq.t;
  if constexpr (GQA) {
    const KvHeads& kvh = the_kv_heads(drop_arg...);
    const int kvbh = (int)c.bh / kvh.G;   // B * H fits an int: grid y
    koff = (long long)(kvbh / kvh.Hkv) * kvh.sk.b +
           (long long)(kvbh % kvh.Hkv) * kvh.sk.h;
    kst = kvh.sk.t;
  }
  auto pipe_k = tile128_pipe<NT, TAIL>(k + koff, kst, c.tid, T);
  auto pipe_v = tile128_pipe<NT, TAIL>(v + koff, kst, c.tid, T);
  const FragOff fo(c);
  int trb[2][2];
  tr_bases(c.lane, trb);
  bfrag q_frag[8], do_frag[8];
  load_row_frags_scaled<TAIL>(q_frag, q + boff, row_me, c.h32, sq.t,
                              scale * LOG2E, row_ok);
  load_row_frags<TAIL>(do_frag, dout + ooff, row_me, c.h32, so.t, row_ok);
  // a padded row: lse = +inf, so that P = exp2(s - inf) is exactly 0
  float lse2_me = INFINITY;
  if (row_ok) lse2_me = lse[c.bh * T + row_me] * LOG2E;
  // delta = rowsum(dO*O) from the dO fragments already here plus one O load
  float dlt_me = 0.f;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    union { bfrag f; short8v v8; } ov, dv;
    ov.f = load_frag<TAIL>(o + ooff, row_me, s * 16 + 8 * c.h32, so.t, row_ok);
    dv.f = do_frag[s];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      dlt_me += bf_elem(ov.v8, e) * bf_elem(dv.v8, e);
  }
  dlt_me += __shfl_xor(dlt_me, 32, WAVE);
  if (c.lane < 32 && row_ok) delta[c.bh * T + row_me] = dlt_me;

  const f32x16 kzero = {};
  f32x16 dq_acc[4] = {};

  const int n_kv = (c.tile + 1) * BM / KVB;
  pipe_k.prime();
  pipe_v.prime();
  for (int j = 0; j < n_kv; ++j) {
    next_tiles128(pipe_k, lds_k, pipe_v, lds_v, j + 1 < n_kv);
    __syncthreads();

    const int key0 = j * KVB;
    if (key0 > row_lo + 31) continue;
    if constexpr (TAIL) {
      if (row_lo >= T) continue;   // a wave of padded rows only
    }

    const bool diag = key0 + KVB - 1 > row_lo;
    PackedC dS;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      // S^T, dP^T tiles: C[key = 32*t2 + crow(r,h32)][qrow = x32]
      __builtin_amdgcn_s_setprio(1);
      const f32x16 s_acc = mfma_rows_d128(lds_k, fo, t2, q_frag, kzero);
      const f32x16 dp_acc = mfma_rows_d128(lds_v, fo, t2, do_frag, kzero);
      __builtin_amdgcn_s_setprio(0);
      float dsv[16];
      // the mask as a compile-time split on a wave-uniform condition
      auto consume = [&](auto MASK) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float pp = fast_exp2(s_acc[r] - lse2_me);
          if (MASK.value) {
            const int key = key0 + t2 * 32 + crow(r, c.h32);
            pp = (key <= row_me) ? pp : 0.f;
          }
          float dpv = dp_acc[r];   // DROP: masked and rescaled before dS
          if constexpr (DROP) {
            const Dropout& drop = the_dropout(drop_arg...);
            const int key = key0 + t2 * 32 + crow(r, c.h32);
            dpv = drop.keep(drop_base + key) ? dpv * drop.inv_keep : 0.f;
          }
          dsv[r] = pp * (dpv - dlt_me);   // scale in the epilogue
        }
      };
      if (diag)
        consume(std::true_type{});
      else
        consume(std::false_type{});
#pragma unroll
      for (int r1 = 0; r1 < 4; ++r1) {
        dS.wA[t2][r1] = pack2(dsv[4 * r1], dsv[4 * r1 + 1]);
        dS.wB[t2][r1] = pack2(dsv[4 * r1 + 2], dsv[4 * r1 + 3]);
      }
      // dQ[qrow][d] += dS K over this half's keys (A-frag k = key): the two
      // k-slices of half t2 need no value of the other half
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s = 2 * t2; s < 2 * t2 + 2; ++s)
        mfma_cols_d128(dq_acc, frag_from_packed(dS, s), lds_k, trb, s);
      __builtin_amdgcn_s_setprio(0);
    }
  }

  __syncthreads();   // K/V tiles are consumed: their space holds the images
  const BlockCtx e = c.fresh_lane();
  const int erow_lo = e.tile * BM + e.w * 32;
  store_ctiles128<TAIL>(dq + e.base(sd, H) + (long long)erow_lo * sd.t, sd.t,
                        e, dq_acc, [&](int) { return scale; },
                        smem + e.w * STAGE128, T - erow_lo);
}

template <int NW>
__launch_bounds__(NW * WAVE, fwd_dq_waves_per_simd(NW))
NO_PK_F32
__global__ void attn_d128_bwd_dq_kernel(const bf16* __restrict__ q,
                                        const bf16* __restrict__ k,
                                        const bf16* __restrict__ v,
                                        const bf16* __restrict__ o,
                                        const bf16* __restrict__ dout,
                                        const float* __restrict__ lse,
                                        float* __restrict__ delta,
                                        bf16* __restrict__ dq, int T, int H,
                                        float scale, GStride sq, GStride so,
                                        GStride sd, int balance) {
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE128];
  BlockCtx c(T / (NW * 32), balance, true);
  do {
    d128_bwd_dq_tile<NW, false>(c, smem, q, k, v, o, dout, lse, delta, dq, T,
                                H, scale, sq, so, sd);
  } while (c.next_pass());
}

template <int NW>
__launch_bounds__(NW * WAVE, fwd_dq_waves_per_simd(NW))
NO_PK_F32
__global__ void attn_d128_bwd_dq_tail_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ o,
    const bf16* __restrict__ dout, const float* __restrict__ lse,
    float* __restrict__ delta, bf16* __restrict__ dq, int T, int H,
    float scale, GStride sq, GStride so, GStride sd, int balance) {
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE128];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, true);
  do {
    d128_bwd_dq_tile<NW, true>(c, smem, q, k, v, o, dout, lse, delta, dq, T,
                               H, scale, sq, so, sd);
  } while (c.next_pass());
}

// ---------------------------------------------------------------------------
// Backward dK/dV: one workgroup per (NW*32)-key block; wave w owns 32 keys
// and streams 64-row Q/dO tiles from the diagonal to the end.
// ---------------------------------------------------------------------------
template <int NW, bool TAIL, typename... Drop>
DEV_INLINE void d128_bwd_dkv_tile(const BlockCtx& c, char* smem,
                                  const bf16* __restrict__ q,
                                  const bf16* __restrict__ k,
                                  const bf16* __restrict__ v,
                                  const bf16* __restrict__ dout,
                                  const float* __restrict__ lse,
                                  const float* __restrict__ delta,
                                  bf16* __restrict__ dk, bf16* __restrict__ dv,
                                  int T, int H, float scale, const GStride& sq,
                                  const GStride& so, const GStride& sd,
                                  const Drop&... drop_arg) {
  constexpr bool DROP = sizeof...(Drop) != 0;
  constexpr int BK = NW * 32;
  constexpr int NT = NW * WAVE;
  char* lds_q = smem;
  char* lds_do = smem + TILE128;
  float* lds_lse = reinterpret_cast<float*>(smem + 2 * TILE128);
  float* lds_dlt = lds_lse + KVB;

  const long long boff = c.base(sq, H);
  const int i0 = c.tile * BK / KVB;   // first Q tile that sees these keys
  const int n_q = TAIL ? (T + KVB - 1) / KVB : T / KVB;   // Q tiles in all

  auto pipe_q = tile128_pipe<NT, TAIL>(
      q + boff + (long long)(i0 * KVB) * sq.t, sq.t, c.tid, T - i0 * KVB);
  auto pipe_do = tile128_pipe<NT, TAIL>(
      dout + c.base(so, H) + (long long)(i0 * KVB) * so.t, so.t, c.tid,
      T - i0 * KVB);
  const FragOff af(c);
  int trb[2][2];
  tr_bases(c.lane, trb);
  const int key_lo = c.tile * BK + c.w * 32;
  const int key_me = key_lo + c.x32;
  // B operands (col = key x32, d-slices): pinned in registers by the 4-wave
  // kernel. The 2-wave kernel stages twice as much per thread (112 registers
  // of pointers and pending chunks) and would spill, so its block's K and V,
  // one 64 x 128 tile each, stay in LDS and wave w reads half w per use.
  // DROP: the 4-wave kernel does the same with two tiles each (128 keys;
  // wave w reads 32-key band w), which frees the 64 registers of the pinned
  // fragments for the mask ("Dropout" above the DROP kernels).
  constexpr bool PINNED = (NW != 2) && !DROP;
  constexpr int OWN = BK / KVB;   // tiles of the block's own K (and V)
  char* lds_kown = smem + 2 * TILE128 + 2 * KVB * 4;
  char* lds_vown = lds_kown + OWN * TILE128;
  // dropout index: idx = bhTT + qrow * T + key_me (qrow * T fits 32 bits)
  unsigned long long drop_bhTT = 0;
  if constexpr (DROP) drop_bhTT = (unsigned long long)c.bh * T * T;
  bfrag k_frag[8], v_frag[8];
  if constexpr (PINNED) {
    load_row_frags_scaled<TAIL>(k_frag, k + boff, key_me, c.h32, sq.t,
                                scale * LOG2E, key_me < T);
    load_row_frags<TAIL>(v_frag, v + boff, key_me, c.h32, sq.t, key_me < T);
  } else {
    const long long koff = boff + (long long)(c.tile * BK) * sq.t;
    __syncthreads();   // BAL_PAIRS: the previous pass has read its K and V
    // TAIL: BK = 64 here, so the block's tile has T - tile * 64 >= 1 rows
    stage_tile128_scaled<NT, TAIL>(lds_kown, k + koff, sq.t, c.tid,
                                   scale * LOG2E, T - c.tile * BK);
    stage_tile128_scaled<NT, TAIL>(lds_vown, v + koff, sq.t, c.tid, 1.0f,
                                   T - c.tile * BK);
    if constexpr (OWN > 1) {
      // keys 64-127 of a 4-wave block; TAIL: T rounded up to 64 is a multiple
      // of 128, so this tile too has T - tile * 128 - 64 >= 1 rows
      const long long koff1 = koff + (long long)KVB * sq.t;
      stage_tile128_scaled<NT, TAIL>(lds_kown + TILE128, k + koff1, sq.t,
                                     c.tid, scale * LOG2E,
                                     T - c.tile * BK - KVB);
      stage_tile128_scaled<NT, TAIL>(lds_vown + TILE128, v + koff1, sq.t,
                                     c.tid, 1.0f, T - c.tile * BK - KVB);
    }
    // published by the barriers of the first loop iteration
  }

  const f32x16 kzero = {};
  f32x16 dk_acc[4] = {};
  f32x16 dv_acc[4] = {};

  // lse (to log2 space) and delta of a Q tile travel with the tile
  const long long row0 = c.bh * T + i0 * KVB;
  RowPipe<TAIL> rows(lse + row0, delta + row0, lds_lse, lds_dlt, LOG2E, c.tid,
                     T - i0 * KVB);
  pipe_q.prime();
  pipe_do.prime();
  rows.fetch();
  for (int i = i0; i < n_q; ++i) {
    next_tiles128(pipe_q, lds_q, pipe_do, lds_do, i + 1 < n_q, rows);
    __syncthreads();

    const int q0 = i * KVB;
    if (q0 + KVB - 1 < key_lo) continue;
    if constexpr (TAIL) {
      if (key_lo >= T) continue;   // a wave of padded keys only
    }

    const bool diag = q0 < key_lo + 32;
    const int mask_lo = key_me - q0 - 4 * c.h32;   // diagonal tiles only
    // (q0 + lrow) * T, split like the mask: lane part here, literal at use
    unsigned drop_rowT = 0;
    if constexpr (DROP) drop_rowT = pin((unsigned)((q0 + 4 * c.h32) * T));
    PackedC P, dS;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      // S, dP tiles: C[qrow = 32*t2 + crow(r,h32)][key = x32]
      __builtin_amdgcn_s_setprio(1);
      f32x16 s_acc, dp_acc;
      if constexpr (PINNED) {
        s_acc = mfma_rows_d128(lds_q, af, t2, k_frag, kzero);
        dp_acc = mfma_rows_d128(lds_do, af, t2, v_frag, kzero);
      } else {
        s_acc = mfma_rows_d128<OWN>(lds_q, af, t2, lds_kown, c.w, kzero);
        dp_acc = mfma_rows_d128<OWN>(lds_do, af, t2, lds_vown, c.w, kzero);
      }
      __builtin_amdgcn_s_setprio(0);
      auto consume = [&](auto MASK) {
#pragma unroll
        for (int r1 = 0; r1 < 4; ++r1) {
          float p[4], dsv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * r1 + e;
            const int lrow = t2 * 32 + crow(r, c.h32);
            float pp = fast_exp2(s_acc[r] - lds_lse[lrow]);
            // key_me <= q0 + lrow, the lane's part of lrow moved to mask_lo
            if (MASK.value) pp = (t2 * 32 + crow(r, 0) >= mask_lo) ? pp : 0.f;
            float pv = pp;             // DROP: dropped P feeds dV,
            float dpv = dp_acc[r];     // masked and rescaled dP feeds dS
            if constexpr (DROP) {
              const Dropout& drop = the_dropout(drop_arg...);
              const bool keep = drop.keep(
                  drop_bhTT +
                  (drop_rowT + (unsigned)((t2 * 32 + crow(r, 0)) * T)) +
                  key_me);
              pv = keep ? pp * drop.inv_keep : 0.f;
              dpv = keep ? dpv * drop.inv_keep : 0.f;
            }
            p[e] = pv;
            dsv[e] = pp * (dpv - lds_dlt[lrow]);   // scale in epilogue
          }
          P.wA[t2][r1] = pack2(p[0], p[1]);
          P.wB[t2][r1] = pack2(p[2], p[3]);
          dS.wA[t2][r1] = pack2(dsv[0], dsv[1]);
          dS.wB[t2][r1] = pack2(dsv[2], dsv[3]);
        }
      };
      if (diag)
        consume(std::true_type{});
      else
        consume(std::false_type{});
      // dV[key][d] += P^T dO ; dK[key][d] += dS^T Q over this half's rows
      // (A-frag k = qrow): P and dS of one half are live at a time
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s = 2 * t2; s < 2 * t2 + 2; ++s) {
        mfma_cols_d128(dv_acc, frag_from_packed(P, s), lds_do, trb, s);
        mfma_cols_d128(dk_acc, frag_from_packed(dS, s), lds_q, trb, s);
      }
      __builtin_amdgcn_s_setprio(0);
    }
  }

  __syncthreads();   // Q/dO tiles are consumed: their space holds the images
  const BlockCtx e = c.fresh_lane();
  const int ekey_lo = e.tile * BK + e.w * 32;
  const long long doff = e.base(sd, H) + (long long)ekey_lo * sd.t;
  char* stage = smem + e.w * STAGE128;
  store_ctiles128<TAIL>(dk + doff, sd.t, e, dk_acc,
                        [&](int) { return scale; }, stage, T - ekey_lo);
  store_ctiles128<TAIL>(dv + doff, sd.t, e, dv_acc,
                        [&](int) { return 1.0f; }, stage, T - ekey_lo);
}

// Q and dO tiles, lse and delta of a Q tile, and in the 2-wave kernel and
// under DROP the block's own K and V (nw / 2 tiles each).
constexpr int dkv_lds_bytes(int nw, bool drop = false) {
  return 2 * TILE128 + 2 * KVB * 4 + (nw == 2 || drop ? nw * TILE128 : 0);
}

template <int NW>
__launch_bounds__(NW * WAVE)
NO_PK_F32
__global__ void attn_d128_bwd_dkv_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    bf16* __restrict__ dk, bf16* __restrict__ dv, int T, int H, float scale,
    GStride sq, GStride so, GStride sd, int balance) {
  __shared__ __attribute__((aligned(16)))
  char smem[dkv_lds_bytes(NW)];
  BlockCtx c(T / (NW * 32), balance, false);
  do {
    d128_bwd_dkv_tile<NW, false>(c, smem, q, k, v, dout, lse, delta, dk, dv,
                                 T, H, scale, sq, so, sd);
  } while (c.next_pass());
}

template <int NW>
__launch_bounds__(NW * WAVE)
NO_PK_F32
__global__ void attn_d128_bwd_dkv_tail_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    bf16* __restrict__ dk, bf16* __restrict__ dv, int T, int H, float scale,
    GStride sq, GStride so, GStride sd, int balance) {
  __shared__ __attribute__((aligned(16)))
  char smem[dkv_lds_bytes(NW)];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, false);
  do {
    d128_bwd_dkv_tile<NW, true>(c, smem, q, k, v, dout, lse, delta, dk, dv, T,
                                H, scale, sq, so, sd);
  } while (c.next_pass());
}

// ---------------------------------------------------------------------------
// Dropout: the kernels above with DROP set in their tile functions, aligned
// and tail, as __global__ functions of their own (their own launch bounds and
// LDS; the kernels above keep their code). The contract is the one of
// attention.hip, and so is the mask: score (bh, row, key) is kept where
// Dropout::keep((bh * T + row) * T + key) holds, on the real T, whatever the
// head dim, NW, TAIL or tile mapping. Nothing is stored: dq and dkv make the
// forward's mask again from the seed. Every index term comes from c.tile, c.bh
// and the lane inside the tile function, so a tile pair's second pass makes
// its own.
//   fwd: the row sum takes the undropped exponentials, so lse is the lse
//        without dropout; only the packed P of P V is keep ? p / (1-p) : 0.
//   dq : dP is masked and rescaled before dS = P (dP - delta).
//   dkv: dV takes the dropped P; dS the undropped P and the masked dP.
// A padded row or key (TAIL) has P = 0 before the mask and stays 0; dropout
// reads and writes no memory.
//
// Registers (docs/kernels.md, "Dropout", has the table). The 4-wave forward
// and dq sit at 238 and 250 of the 256 that two waves per SIMD allow; under
// that cap their DROP forms keep 40-60 and 32-44 bytes of scratch per lane,
// so they are compiled for one wave per SIMD like the 2-wave kernels (360 and
// 360-378 registers, no scratch; a CU then holds one block of them).
// The 4-wave dkv (486 of 512 with K and V fragments pinned) gives up the
// pinned fragments instead: its block's K (prescaled) and V, 128 keys x 128
// columns = two tiles each, stay in LDS after the lse/delta rows and wave w
// reads 32-key band w per use, as the 2-wave kernel does with one tile each
// (436-444 registers). That is 64 KB more LDS (96.5 KB per block) on a kernel
// that ran one block per CU already.
// ---------------------------------------------------------------------------
constexpr int drop_waves_per_simd(int) { return 1; }

template <int NW, bool TAIL>
__launch_bounds__(NW * WAVE, drop_waves_per_simd(NW))
NO_PK_F32
__global__ void attn_d128_fwd_drop_kernel(const bf16* __restrict__ q,
                                          const bf16* __restrict__ k,
                                          const bf16* __restrict__ v,
                                          bf16* __restrict__ o,
                                          float* __restrict__ lse, int T,
                                          int H, float scale, GStride sq,
                                          GStride so, Dropout drop,
                                          int balance) {
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE128];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, true);
  do {
    d128_fwd_tile<NW, TAIL>(c, smem, q, k, v, o, lse, T, H, scale, sq,
                                  so, drop);
  } while (c.next_pass());
}

template <int NW, bool TAIL>
__launch_bounds__(NW * WAVE, drop_waves_per_simd(NW))
NO_PK_F32
__global__ void attn_d128_bwd_dq_drop_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ o,
    const bf16* __restrict__ dout, const float* __restrict__ lse,
    float* __restrict__ delta, bf16* __restrict__ dq, int T, int H,
    float scale, GStride sq, GStride so, GStride sd, Dropout drop,
    int balance) {
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE128];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, true);
  do {
    d128_bwd_dq_tile<NW, TAIL>(c, smem, q, k, v, o, dout, lse, delta,
                                     dq, T, H, scale, sq, so, sd, drop);
  } while (c.next_pass());
}

template <int NW, bool TAIL>
__launch_bounds__(NW * WAVE)
NO_PK_F32
__global__ void attn_d128_bwd_dkv_drop_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    bf16* __restrict__ dk, bf16* __restrict__ dv, int T, int H, float scale,
    GStride sq, GStride so, GStride sd, Dropout drop, int balance) {
  __shared__ __attribute__((aligned(16)))
  char smem[dkv_lds_bytes(NW, true)];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, false);
  do {
    d128_bwd_dkv_tile<NW, TAIL>(c, smem, q, k, v, dout, lse, delta, dk,
                                      dv, T, H, scale, sq, so, sd, drop);
  } while (c.next_pass());
}

// ---------------------------------------------------------------------------
// Grouped-query: q, o, dout, dq, lse and delta have H heads, k, v, dk and dv
// Hkv of them (H % Hkv == 0, G = H / Hkv), and query head h attends K/V head
// h / G. k and v share the strides sk, dk and dv sdk. No DROP form.
//   fwd, dq: the kernels above with a KvHeads in the pack: grid (tile, B*H),
//        the same arithmetic per query head in the same order, only the K/V
//        tiles come from head bh / G. o, lse, dq and delta carry the bits of
//        the multi-head kernels on K/V expanded G-fold.
//        The G heads of a group stream the same K/V, so the remapped y index
//        is decoded group-minor (gqa_query_head): where B*Hkv % 8 == 0 they
//        then share an XCD and its L2, as one head's blocks do.
//   dkv: grid (tile or pair, B*Hkv); a workgroup owns NW*32 keys of a K/V
//        head, loads them once and keeps dK/dV in registers while it walks
//        the Q/dO tiles i0..n_q-1 of all G query heads of the group in ONE
//        loop of G*(n_q-i0) iterations: the step from a head's last tile to
//        the next head's first is an advance() by another uniform amount, so
//        the pipeline never drains. One epilogue and one rounding per group:
//        the group's sum is fp32 in the accumulators, in head order.
// TAIL: the rules of "Ragged T" hold per query head: every head's last tile
// takes the predicated fetch, and the pipes' row counts start over with each
// head.
// ---------------------------------------------------------------------------
// The query (batch, head) of remapped y index y: group-minor with xcd_group,
// so that y % 8, the XCD under xcd_remap, is the group's where B*Hkv % 8 == 0;
// else y itself. Both are bijections of [0, B*H).
DEV_INLINE int gqa_query_head(int y, int BH, int G, int xcd_group) {
  if (!xcd_group) return y;
  const int groups = BH / G;   // B * Hkv
  return (y % groups) * G + y / groups;
}

template <int NW, bool TAIL>
__launch_bounds__(NW * WAVE, fwd_dq_waves_per_simd(NW))
NO_PK_F32
__global__ void attn_d128_gqa_fwd_kernel(const bf16* __restrict__ q,
                                         const bf16* __restrict__ k,
                                         const bf16* __restrict__ v,
                                         bf16* __restrict__ o,
                                         float* __restrict__ lse, int T, int H,
                                         int Hkv, float scale, GStride sq,
                                         GStride sk, GStride so,
                                         int xcd_group, int balance) {
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE128];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, true);
  const KvHeads kvh = {H / Hkv, Hkv, sk};
  c.bh = gqa_query_head((int)c.bh, gridDim.y, kvh.G, xcd_group);
  do {
    d128_fwd_tile<NW, TAIL>(c, smem, q, k, v, o, lse, T, H, scale, sq, so,
                            kvh);
  } while (c.next_pass());
}

template <int NW, bool TAIL>
__launch_bounds__(NW * WAVE, fwd_dq_waves_per_simd(NW))
NO_PK_F32
__global__ void attn_d128_gqa_bwd_dq_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ o,
    const bf16* __restrict__ dout, const float* __restrict__ lse,
    float* __restrict__ delta, bf16* __restrict__ dq, int T, int H, int Hkv,
    float scale, GStride sq, GStride sk, GStride so, GStride sd,
    int xcd_group, int balance) {
  __shared__ __attribute__((aligned(16))) char smem[2 * TILE128];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, true);
  const KvHeads kvh = {H / Hkv, Hkv, sk};
  c.bh = gqa_query_head((int)c.bh, gridDim.y, kvh.G, xcd_group);
  do {
    d128_bwd_dq_tile<NW, TAIL>(c, smem, q, k, v, o, dout, lse, delta, dq, T,
                               H, scale, sq, so, sd, kvh);
  } while (c.next_pass());
}

// next_tiles128 for the dkv loop over the heads of a group. With `wrap` the
// pending tiles were a head's last, and the following ones are the first of
// the next head: the pipes move by jump_x / jump_y elements and the rows by
// row_jump instead of one tile, and every row count (TAIL) starts over at
// left0. `wrap` is block-uniform.
template <int NT, bool TAIL>
DEV_INLINE void next_tiles128_heads(TilePipe<NT, TAIL>& x, char* lds_x,
                                    TilePipe<NT, TAIL>& y, char* lds_y,
                                    RowPipe<TAIL>& rows, bool more, bool wrap,
                                    long long jump_x, long long jump_y,
                                    long long row_jump, int left0) {
  __syncthreads();
  x.a.put(lds_x, x.pend_a);
  x.b.put(lds_x + IMG, x.pend_b);
  y.a.put(lds_y, y.pend_a);
  y.b.put(lds_y + IMG, y.pend_b);
  rows.put();
  if (more) {
    if (wrap) {
#pragma unroll
      for (int rep = 0; rep < Stage<NT>::REPS; ++rep) {
        x.a.src[rep] += jump_x;
        x.b.src[rep] += jump_x;
        y.a.src[rep] += jump_y;
        y.b.src[rep] += jump_y;
      }
      rows.ga += row_jump;
      rows.gb += row_jump;
      if constexpr (TAIL) {
        x.left = left0;
        y.left = left0;
        rows.left = left0;
      }
    } else {
      x.a.advance();
      x.b.advance();
      y.a.advance();
      y.b.advance();
      rows.advance();
      if constexpr (TAIL) {
        x.left -= KVB;
        y.left -= KVB;
      }
    }
    x.fetch();
    y.fetch();
    rows.fetch();
  }
}

// K and V of the block's keys in LDS (the 2-wave kernel always; the 4-wave
// kernel where GQA_DKV4_PINNED is false), as in d128_bwd_dkv_tile.
constexpr bool GQA_DKV4_PINNED = true;

template <int NW, bool TAIL>
DEV_INLINE void d128_gqa_bwd_dkv_tile(
    const BlockCtx& c, char* smem, const bf16* __restrict__ q,
    const bf16* __restrict__ k, const bf16* __restrict__ v,
    const bf16* __restrict__ dout, const float* __restrict__ lse,
    const float* __restrict__ delta, bf16* __restrict__ dk,
    bf16* __restrict__ dv, int T, int H, int Hkv, float scale,
    const GStride& sq, const GStride& sk, const GStride& so,
    const GStride& sdk) {
  constexpr int BK = NW * 32;
  constexpr int NT = NW * WAVE;
  char* lds_q = smem;
  char* lds_do = smem + TILE128;
  float* lds_lse = reinterpret_cast<float*>(smem + 2 * TILE128);
  float* lds_dlt = lds_lse + KVB;

  // c.bh is the K/V head; its query heads are qbh .. qbh + G - 1, all of
  // one batch, a head stride apart in q and dout and T apart in lse and delta
  // (B * H fits an int, the grid's y: 32-bit divisions)
  const int G = H / Hkv;
  const int qbh = (int)c.bh * G;
  auto head_off = [](int bh, int heads, const GStride& s) {
    return (long long)(bh / heads) * s.b + (long long)(bh % heads) * s.h;
  };
  const long long koff = head_off((int)c.bh, Hkv, sk);
  const int i0 = c.tile * BK / KVB;   // first Q tile that sees these keys
  const int n_q = TAIL ? (T + KVB - 1) / KVB : T / KVB;   // Q tiles per head
  const int left0 = T - i0 * KVB;
  // from a head's last tile to the next head's tile i0
  const long long back = (long long)(n_q - 1 - i0) * KVB;
  const long long jump_q = sq.h - back * sq.t;
  const long long jump_do = so.h - back * so.t;
  const long long jump_row = T - back;

  auto pipe_q = tile128_pipe<NT, TAIL>(
      q + head_off(qbh, H, sq) + (long long)(i0 * KVB) * sq.t, sq.t, c.tid,
      left0);
  auto pipe_do = tile128_pipe<NT, TAIL>(
      dout + head_off(qbh, H, so) + (long long)(i0 * KVB) * so.t, so.t, c.tid,
      left0);
  const FragOff af(c);
  int trb[2][2];
  tr_bases(c.lane, trb);
  const int key_lo = c.tile * BK + c.w * 32;
  const int key_me = key_lo + c.x32;
  constexpr bool PINNED = (NW != 2) && GQA_DKV4_PINNED;
  constexpr int OWN = BK / KVB;   // tiles of the block's own K (and V)
  char* lds_kown = smem + 2 * TILE128 + 2 * KVB * 4;
  char* lds_vown = lds_kown + OWN * TILE128;
  bfrag k_frag[8], v_frag[8];
  if constexpr (PINNED) {
    load_row_frags_scaled<TAIL>(k_frag, k + koff, key_me, c.h32, sk.t,
                                scale * LOG2E, key_me < T);
    load_row_frags<TAIL>(v_frag, v + koff, key_me, c.h32, sk.t, key_me < T);
  } else {
    const long long kown = koff + (long long)(c.tile * BK) * sk.t;
    __syncthreads();   // BAL_PAIRS: the previous pass has read its K and V
#pragma unroll
    for (int t = 0; t < OWN; ++t) {
      // TAIL: T rounded up to 64 is a multiple of BK, so every tile of the
      // block has at least one row
      const long long kt = kown + (long long)(t * KVB) * sk.t;
      stage_tile128_scaled<NT, TAIL>(lds_kown + t * TILE128, k + kt, sk.t,
                                     c.tid, scale * LOG2E,
                                     T - c.tile * BK - t * KVB);
      stage_tile128_scaled<NT, TAIL>(lds_vown + t * TILE128, v + kt, sk.t,
                                     c.tid, 1.0f, T - c.tile * BK - t * KVB);
    }
    // published by the barriers of the first loop iteration
  }

  const f32x16 kzero = {};
  f32x16 dk_acc[4] = {};
  f32x16 dv_acc[4] = {};

  const long long row0 = (long long)qbh * T + i0 * KVB;
  RowPipe<TAIL> rows(lse + row0, delta + row0, lds_lse, lds_dlt, LOG2E, c.tid,
                     left0);
  pipe_q.prime();
  pipe_do.prime();
  rows.fetch();
  const int n_iter = G * (n_q - i0);
  int i = i0;   // the Q tile of this iteration, i0..n_q-1 in every head
  for (int it = 0; it < n_iter; ++it) {
    const bool wrap = i + 1 == n_q;
    next_tiles128_heads(pipe_q, lds_q, pipe_do, lds_do, rows,
                        it + 1 < n_iter, wrap, jump_q, jump_do, jump_row,
                        left0);
    __syncthreads();

    const int q0 = i * KVB;
    i = wrap ? i0 : i + 1;
    if (q0 + KVB - 1 < key_lo) continue;
    if constexpr (TAIL) {
      if (key_lo >= T) continue;   // a wave of padded keys only
    }

    const bool diag = q0 < key_lo + 32;
    const int mask_lo = key_me - q0 - 4 * c.h32;   // diagonal tiles only
    PackedC P, dS;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      // S, dP tiles: C[qrow = 32*t2 + crow(r,h32)][key = x32]
      __builtin_amdgcn_s_setprio(1);
      f32x16 s_acc, dp_acc;
      if constexpr (PINNED) {
        s_acc = mfma_rows_d128(lds_q, af, t2, k_frag, kzero);
        dp_acc = mfma_rows_d128(lds_do, af, t2, v_frag, kzero);
      } else {
        s_acc = mfma_rows_d128<OWN>(lds_q, af, t2, lds_kown, c.w, kzero);
        dp_acc = mfma_rows_d128<OWN>(lds_do, af, t2, lds_vown, c.w, kzero);
      }
      __builtin_amdgcn_s_setprio(0);
      auto consume = [&](auto MASK) {
#pragma unroll
        for (int r1 = 0; r1 < 4; ++r1) {
          float p[4], dsv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * r1 + e;
            const int lrow = t2 * 32 + crow(r, c.h32);
            float pp = fast_exp2(s_acc[r] - lds_lse[lrow]);
            // key_me <= q0 + lrow, the lane's part of lrow moved to mask_lo
            if (MASK.value) pp = (t2 * 32 + crow(r, 0) >= mask_lo) ? pp : 0.f;
            p[e] = pp;
            dsv[e] = pp * (dp_acc[r] - lds_dlt[lrow]);   // scale in epilogue
          }
          P.wA[t2][r1] = pack2(p[0], p[1]);
          P.wB[t2][r1] = pack2(p[2], p[3]);
          dS.wA[t2][r1] = pack2(dsv[0], dsv[1]);
          dS.wB[t2][r1] = pack2(dsv[2], dsv[3]);
        }
      };
      if (diag)
        consume(std::true_type{});
      else
        consume(std::false_type{});
      // dV[key][d] += P^T dO ; dK[key][d] += dS^T Q over this half's rows
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int s = 2 * t2; s < 2 * t2 + 2; ++s) {
        mfma_cols_d128(dv_acc, frag_from_packed(P, s), lds_do, trb, s);
        mfma_cols_d128(dk_acc, frag_from_packed(dS, s), lds_q, trb, s);
      }
      __builtin_amdgcn_s_setprio(0);
    }
  }

  __syncthreads();   // Q/dO tiles are consumed: their space holds the images
  const BlockCtx e = c.fresh_lane();
  const int ekey_lo = e.tile * BK + e.w * 32;
  const long long doff =
      head_off((int)e.bh, Hkv, sdk) + (long long)ekey_lo * sdk.t;
  char* stage = smem + e.w * STAGE128;
  store_ctiles128<TAIL>(dk + doff, sdk.t, e, dk_acc,
                        [&](int) { return scale; }, stage, T - ekey_lo);
  store_ctiles128<TAIL>(dv + doff, sdk.t, e, dv_acc,
                        [&](int) { return 1.0f; }, stage, T - ekey_lo);
}

template <int NW, bool TAIL>
__launch_bounds__(NW * WAVE)
NO_PK_F32
__global__ void attn_d128_gqa_bwd_dkv_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    bf16* __restrict__ dk, bf16* __restrict__ dv, int T, int H, int Hkv,
    float scale, GStride sq, GStride sk, GStride so, GStride sdk,
    int balance) {
  __shared__ __attribute__((aligned(16)))
  char smem[dkv_lds_bytes(NW, !GQA_DKV4_PINNED)];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, false);
  do {
    d128_gqa_bwd_dkv_tile<NW, TAIL>(c, smem, q, k, v, dout, lse, delta, dk,
                                    dv, T, H, Hkv, scale, sq, sk, so, sdk);
  } while (c.next_pass());
}

// Calls f(NW, TAIL, DROP) as std::integral_constants. TAIL: T % 64 != 0.
// 4-wave blocks where 128 divides T rounded up to 64, else 2-wave blocks.
template <typename F>
static void d128_dispatch(int T, bool drop, F f) {
  const int T64 = (T + KVB - 1) / KVB * KVB;
  auto with_nw = [&](auto TAIL, auto DROP) {
    if (T64 % 128 == 0)
      f(std::integral_constant<int, 4>{}, TAIL, DROP);
    else
      f(std::integral_constant<int, 2>{}, TAIL, DROP);
  };
  auto with_drop = [&](auto TAIL) {
    if (drop) with_nw(TAIL, std::true_type{});
    else with_nw(TAIL, std::false_type{});
  };
  if (T % KVB) with_drop(std::true_type{}); else with_drop(std::false_type{});
}

// The three kernels of one (NW, TAIL, DROP), under one signature: the
// kernels without dropout take no Dropout argument.
template <int NW, bool TAIL, bool DROP>
struct D128Kernels {
  static constexpr auto fwd =
      TAIL ? attn_d128_fwd_tail_kernel<NW> : attn_d128_fwd_kernel<NW>;
  static constexpr auto dq =
      TAIL ? attn_d128_bwd_dq_tail_kernel<NW> : attn_d128_bwd_dq_kernel<NW>;
  static constexpr auto dkv =
      TAIL ? attn_d128_bwd_dkv_tail_kernel<NW> : attn_d128_bwd_dkv_kernel<NW>;
};
template <int NW, bool TAIL>
struct D128Kernels<NW, TAIL, true> {
  static constexpr auto fwd = attn_d128_fwd_drop_kernel<NW, TAIL>;
  static constexpr auto dq = attn_d128_bwd_dq_drop_kernel<NW, TAIL>;
  static constexpr auto dkv = attn_d128_bwd_dkv_drop_kernel<NW, TAIL>;
};

// Launches a kernel of either kind: `drop` goes before `balance`, the last
// argument, where the kernel takes it.
template <bool DROP, auto Kernel, typename... A>
static void d128_launch(dim3 grid, int threads, hipStream_t stream,
                        const Dropout& drop, int balance, A... a) {
  if constexpr (DROP)
    hipLaunchKernelGGL(Kernel, grid, dim3(threads), 0, stream, a..., drop,
                       balance);
  else
    hipLaunchKernelGGL(Kernel, grid, dim3(threads), 0, stream, a..., balance);
}

// Any T >= 1; the entry points below check T against their own contract.
// dropout_p > 0 selects the DROP instantiations and the mask of `seed`.
static hipError_t d128_launch_fwd(const void* q, const void* k, const void* v,
                                  void* o, float* lse, long long B,
                                  long long H, int T, float scale,
                                  const long long* sq_in,
                                  const long long* so_in, float dropout_p,
                                  unsigned long long seed,
                                  hipStream_t stream) {
  const GStride sq = gstride(sq_in), so = gstride(so_in);
  const Dropout drop = make_dropout(dropout_p, seed);
  d128_dispatch(T, dropout_p > 0.0f, [&](auto nw, auto tl, auto dr) {
    constexpr int NW = decltype(nw)::value;
    constexpr bool DROP = decltype(dr)::value;
    constexpr auto fwd = D128Kernels<NW, decltype(tl)::value, DROP>::fwd;
    const int n_tiles = (T + NW * 32 - 1) / (NW * 32);
    const TileMap m = tile_map<fwd>(n_tiles, B * H, NW * WAVE);
    d128_launch<DROP, fwd>(m.grid, NW * WAVE, stream, drop, m.balance,
                           (const bf16*)q, (const bf16*)k, (const bf16*)v,
                           (bf16*)o, lse, T, (int)H, scale, sq, so);
  });
  return hipGetLastError();
}

static hipError_t d128_launch_bwd(const void* q, const void* k, const void* v,
                                  const void* o, const float* lse,
                                  const void* dout, void* dq, void* dk,
                                  void* dv, float* delta, long long B,
                                  long long H, int T, float scale,
                                  const long long* sq_in,
                                  const long long* so_in,
                                  const long long* sd_in, float dropout_p,
                                  unsigned long long seed,
                                  hipStream_t stream) {
  const GStride sq = gstride(sq_in), so = gstride(so_in), sd = gstride(sd_in);
  const Dropout drop = make_dropout(dropout_p, seed);
  // dq runs FIRST: it publishes delta, which dkv (same stream) consumes
  d128_dispatch(T, dropout_p > 0.0f, [&](auto nw, auto tl, auto dr) {
    constexpr int NW = decltype(nw)::value;
    constexpr bool DROP = decltype(dr)::value;
    using K = D128Kernels<NW, decltype(tl)::value, DROP>;
    constexpr auto dq_k = K::dq;
    constexpr auto dkv_k = K::dkv;
    const int n_tiles = (T + NW * 32 - 1) / (NW * 32);
    // the two kernels differ in residency, so each gets its own mapping
    const TileMap mq = tile_map<dq_k>(n_tiles, B * H, NW * WAVE);
    const TileMap mkv = tile_map<dkv_k>(n_tiles, B * H, NW * WAVE);
    d128_launch<DROP, dq_k>(mq.grid, NW * WAVE, stream, drop, mq.balance,
                            (const bf16*)q, (const bf16*)k, (const bf16*)v,
                            (const bf16*)o, (const bf16*)dout, lse, delta,
                            (bf16*)dq, T, (int)H, scale, sq, so, sd);
    d128_launch<DROP, dkv_k>(mkv.grid, NW * WAVE, stream, drop, mkv.balance,
                             (const bf16*)q, (const bf16*)k, (const bf16*)v,
                             (const bf16*)dout, lse, (const float*)delta,
                             (bf16*)dk, (bf16*)dv, T, (int)H, scale, sq, so,
                             sd);
  });
  return hipGetLastError();
}

// TDSA_ATTN_GQA_XCD, read at every launch: 1 (default) decodes the forward's
// and dq's y index group-minor (gqa_query_head), 0 leaves it as it is
// (profiles/attn_d128_gqa.txt has both timed).
static int gqa_xcd_group() { return env_int("TDSA_ATTN_GQA_XCD", 1) != 0; }

static bool gqa_heads_ok(long long H, long long Hkv) {
  return Hkv >= 1 && H >= Hkv && H % Hkv == 0;
}

}  // namespace tdsa

using namespace tdsa;

extern "C" {

hipError_t tdsa_attn_d128_fwd(const void* q, const void* k, const void* v,
                              void* o, float* lse, long long B, long long H,
                              int T, float scale, const long long* sq,
                              const long long* so, float dropout_p,
                              unsigned long long seed, hipStream_t stream) {
  if (T < KVB || T % KVB) return hipErrorInvalidValue;
  return d128_launch_fwd(q, k, v, o, lse, B, H, T, scale, sq, so, dropout_p,
                         seed, stream);
}

hipError_t tdsa_attn_d128_bwd(const void* q, const void* k, const void* v,
                              const void* o, const float* lse,
                              const void* dout, void* dq, void* dk, void* dv,
                              float* delta, long long B, long long H, int T,
                              float scale, const long long* sq,
                              const long long* so, const long long* sd,
                              float dropout_p, unsigned long long seed,
                              hipStream_t stream) {
  if (T < KVB || T % KVB) return hipErrorInvalidValue;
  return d128_launch_bwd(q, k, v, o, lse, dout, dq, dk, dv, delta, B, H, T,
                         scale, sq, so, sd, dropout_p, seed, stream);
}

hipError_t tdsa_attn_d128_ragged_fwd(const void* q, const void* k,
                                     const void* v, void* o, float* lse,
                                     long long B, long long H, int T,
                                     float scale, const long long* sq,
                                     const long long* so, float dropout_p,
                                     unsigned long long seed,
                                     hipStream_t stream) {
  if (T < 1) return hipErrorInvalidValue;
  return d128_launch_fwd(q, k, v, o, lse, B, H, T, scale, sq, so, dropout_p,
                         seed, stream);
}

hipError_t tdsa_attn_d128_ragged_bwd(const void* q, const void* k,
                                     const void* v, const void* o,
                                     const float* lse, const void* dout,
                                     void* dq, void* dk, void* dv,
                                     float* delta, long long B, long long H,
                                     int T, float scale, const long long* sq,
                                     const long long* so, const long long* sd,
                                     float dropout_p, unsigned long long seed,
                                     hipStream_t stream) {
  if (T < 1) return hipErrorInvalidValue;
  return d128_launch_bwd(q, k, v, o, lse, dout, dq, dk, dv, delta, B, H, T,
                         scale, sq, so, sd, dropout_p, seed, stream);
}

hipError_t tdsa_attn_d128_gqa_fwd(const void* q, const void* k, const void* v,
                                  void* o, float* lse, long long B,
                                  long long H, long long Hkv, int T,
                                  float scale, const long long* sq_in,
                                  const long long* sk_in,
                                  const long long* so_in,
                                  hipStream_t stream) {
  if (T < 1 || !gqa_heads_ok(H, Hkv)) return hipErrorInvalidValue;
  const GStride sq = gstride(sq_in), sk = gstride(sk_in), so = gstride(so_in);
  d128_dispatch(T, false, [&](auto nw, auto tl, auto) {
    constexpr int NW = decltype(nw)::value;
    constexpr auto fwd = attn_d128_gqa_fwd_kernel<NW, decltype(tl)::value>;
    const int n_tiles = (T + NW * 32 - 1) / (NW * 32);
    const TileMap m = tile_map<fwd>(n_tiles, B * H, NW * WAVE);
    hipLaunchKernelGGL(fwd, m.grid, dim3(NW * WAVE), 0, stream,
                       (const bf16*)q, (const bf16*)k, (const bf16*)v,
                       (bf16*)o, lse, T, (int)H, (int)Hkv, scale, sq, sk, so,
                       gqa_xcd_group(), m.balance);
  });
  return hipGetLastError();
}

hipError_t tdsa_attn_d128_gqa_bwd(const void* q, const void* k, const void* v,
                                  const void* o, const float* lse,
                                  const void* dout, void* dq, void* dk,
                                  void* dv, float* delta, long long B,
                                  long long H, long long Hkv, int T,
                                  float scale, const long long* sq_in,
                                  const long long* sk_in,
                                  const long long* so_in,
                                  const long long* sd_in,
                                  const long long* sdk_in,
                                  hipStream_t stream) {
  if (T < 1 || !gqa_heads_ok(H, Hkv)) return hipErrorInvalidValue;
  const GStride sq = gstride(sq_in), sk = gstride(sk_in), so = gstride(so_in),
                sd = gstride(sd_in), sdk = gstride(sdk_in);
  // dq runs FIRST: it publishes delta, which dkv (same stream) consumes
  d128_dispatch(T, false, [&](auto nw, auto tl, auto) {
    constexpr int NW = decltype(nw)::value;
    constexpr bool TAIL = decltype(tl)::value;
    constexpr auto dq_k = attn_d128_gqa_bwd_dq_kernel<NW, TAIL>;
    constexpr auto dkv_k = attn_d128_gqa_bwd_dkv_kernel<NW, TAIL>;
    const int n_tiles = (T + NW * 32 - 1) / (NW * 32);
    // dq maps the B*H query heads, dkv the B*Hkv K/V heads, whose workgroups
    // cost G times as much: each mapping from its own grid and residency
    const TileMap mq = tile_map<dq_k>(n_tiles, B * H, NW * WAVE);
    const TileMap mkv = tile_map<dkv_k>(n_tiles, B * Hkv, NW * WAVE);
    hipLaunchKernelGGL(dq_k, mq.grid, dim3(NW * WAVE), 0, stream,
                       (const bf16*)q, (const bf16*)k, (const bf16*)v,
                       (const bf16*)o, (const bf16*)dout, lse, delta,
                       (bf16*)dq, T, (int)H, (int)Hkv, scale, sq, sk, so, sd,
                       gqa_xcd_group(), mq.balance);
    hipLaunchKernelGGL(dkv_k, mkv.grid, dim3(NW * WAVE), 0, stream,
                       (const bf16*)q, (const bf16*)k, (const bf16*)v,
                       (const bf16*)dout, lse, (const float*)delta,
                       (bf16*)dk, (bf16*)dv, T, (int)H, (int)Hkv, scale, sq,
                       sk, so, sdk, mkv.balance);
  });
  return hipGetLastError();
}

}  // extern "C"
