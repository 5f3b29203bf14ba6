// Fused causal attention (flash-style) on CDNA4 MFMA matrix cores.
//
// Replaces the reference's materialized (B,H,T,T) score path
// (/root/reference/example/model.py:29-51) with an MI355X-native design
// built around v_mfma_f32_32x32x16_bf16 (fp32 accumulate):
//
//   forward : per Q block (NW waves x 32 rows), stream 64-key K/V tiles
//             through XOR-swizzled LDS. S^T = mfma(K, Q) puts the whole
//             softmax row in one lane pair (one shfl_xor(32) per reduce);
//             online softmax runs in exp2 space (log2e folded into the Q
//             prescale); P is repacked into MFMA A-fragments with TWO
//             v_permlane32_swap per k-slice (no LDS round trip); O = P V
//             with V consumed via ds_read_tr16_b64 hardware transpose
//             reads from the row-major image. Saves per-row natural-log lse.
//   backward: recompute-based two-kernel scheme (no atomics):
//             the dq kernel (launched first) owns a (NW*32)-row Q block,
//             computes delta = rowsum(dO*O) from its own fragments and
//             publishes it; the dkv kernel owns a (NW*32)-key block and
//             accumulates dK/dV over 64-row Q tiles, consuming delta.
//             The 1/sqrt(D) on dS is folded into the dK/dQ epilogue.
//
// The three kernels share one skeleton: BlockCtx (block prologue), TilePipe
// (two-tile LDS pipeline; in the dkv kernel its companion RowPipe carries
// lse and delta of the next Q tile along), FragOff (fragment read offsets),
// frag_from_packed (C -> A repack) and store_ctiles (epilogue). Each kernel
// is a pass loop around its attn_*_tile function.
//
// Workgroup -> tile mapping (tile_map, TDSA_ATTN_BALANCE): under the causal
// mask tile t of n costs t+1 tiles of K/V (fwd, dq) or n-t tiles of Q (dkv).
// A workgroup runs the pair (t, n-1-t) of one (batch, head), n+1 tiles
// whichever pair; where the halved grid would not fill the device, one tile
// as before, the heaviest tiles of the whole grid dispatched first. H=16,
// T=1024, B=32: forward 167-171 -> 138-145 us, backward 538-547 -> 394-400 us
// (profiles/attn_balance.txt).
//
// Epilogues: a lane holds one column of its wave's result, so o, dq, dk and
// dv go through a per-wave LDS image and leave as whole 128-byte rows (16
// bytes per lane, 4 store instructions per 32x64 tile instead of 32).
//
// All global accesses are stride-parameterized so the kernels consume the
// packed qkv projection layout (B,T,3,H,D) and write O/dQKV into (B,T,H,D)
// buffers directly — no transpose-copies on the hot path.
//
// VALU discipline (first profile measured 22:1 VALU:MFMA on a naive
// version): every LDS offset is precomputed before the K/V loop; causal
// masking runs only on diagonal tiles (wave-uniform branch); waves whose
// rows lie entirely outside a tile skip its compute. Two bf16 results that
// share a word are packed by ONE v_cvt_pk_bf16_f32 (pack2, mfma.h). Per
// off-diagonal tile and wave the 8-wave loops issue about 155 (fwd, 16
// MFMA; 19 more when the running max moves), 125 (dq, 24 MFMA) and 150
// (dkv, 32 MFMA) vector instructions (profiles/attn_valu.txt);
// what is left is the softmax itself (sub, exp2, max/sum, the P*(dP-delta)
// products), the permlane repack and LDS addressing.
//
// Waits: each loop waits for global memory once per tile, at its head, for
// loads issued a whole tile earlier. The dkv kernel fetches lse/delta of
// tile i+1 together with tile i+1's Q/dO (RowPipe) for that reason: loads
// retire in order, and a load-and-use between the prefetch and the barrier
// would wait for the prefetch as well.
//
// 32x32x16 fragment layouts (hardware-verified slot-pairing rule: A and B
// must agree on the slot->k map, C is fixed; see scripts/debug_mfma.py):
//   A[32x16]: lane l, elem e(0..7) -> A[l%32][(l/32)*8 + e]
//   B[16x32]: lane l, elem e      -> B[(l/32)*8 + e][l%32]
//   C[32x32]: lane l, reg r(0..15)-> C[(r&3) + 8*(r>>2) + 4*(l/32)][l%32]
//
// Contract: bf16, head_dim 64, T % 64 == 0 (the Python op falls back to a
// composite rocBLAS path otherwise, ops/attention.py).
#include "common.h"
#include "launchers.h"
#include "mfma.h"

#include <type_traits>

namespace tdsa {

constexpr int KVB = 64;   // keys / rows per LDS tile
constexpr int D = 64;     // head dim (all GPT-2 sizes)
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

// Raw v_exp_f32: libm exp2f wraps every call in an ldexp+select sequence for
// |x| > 126 handling; our arguments are always <= 0 (score - running max /
// lse), where the bare instruction is exact-enough (1 ulp) and handles -inf
// -> 0. Measured 1:1 v_ldexp_f32 per exp in the softmax hot loop without it.
DEV_INLINE float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }
// Raw v_rcp_f32 for the epilogue 1/l (IEEE div emits ~10-inst div_scale
// chains; the result feeds a bf16 store).
DEV_INLINE float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
// Value barrier (emits nothing): the compiler may not look through x. Used
// where it otherwise rewrites the dropout code into something costlier:
// a select moved across the bf16 pack (then done per half and re-joined with
// v_perm_b32), or a per-tile index term folded into 32 hoisted registers.
DEV_INLINE float pin(float x) { asm("" : "+v"(x)); return x; }
DEV_INLINE unsigned pin(unsigned x) { asm("" : "+v"(x)); return x; }

// XCD-aware block remap (T1): the dispatcher places linear block b on XCD
// b % 8, and the x-dimension varies fastest, so the gridDim.x blocks that
// share one (batch, head) — and its K/V tiles — land on different XCDs'
// L2s. Remap so they share an XCD: within each window of 8*gridX linear
// ids, ids congruent mod 8 form one bh. Bijective when gridY % 8 == 0.
DEV_INLINE void xcd_remap(int gx, long long gy, int& tile, long long& bh) {
  if (gy % 8 == 0) {
    const long long id = bh * gx + tile;   // linear dispatch id
    tile = (int)((id % (8 * gx)) / 8);
    bh = (id / (8 * gx)) * 8 + (id % 8);
  }
}

// Per-tensor global strides in ELEMENTS (last dim contiguous).
struct GStride {
  long long b;
  long long h;
  int t;
};

// Workgroup -> tile mapping (TDSA_ATTN_BALANCE). Under the causal mask tile t
// of n costs t+1 units in fwd/dq and n-t in dkv, so BAL_OFF hands out
// workgroups of 1..n units. BAL_PAIRS gives one workgroup the tiles t and
// n-1-t of one (batch, head), one after the other: every workgroup then
// costs n+1 units (the middle tile of an odd n runs alone).
constexpr int BAL_OFF = 0;    // one tile per workgroup, x = tile
constexpr int BAL_PAIRS = 1;  // two tiles per workgroup, x = pair
constexpr int BAL_HEAVY = 2;  // one tile, heaviest tiles of the GRID first

// Block prologue of all three kernels: the remapped (tile, batch*head) this
// block owns and the lane's place in its wave's 32x32 MFMA tiles.
struct BlockCtx {
  int tile;        // block index along T after the XCD remap
  int tile2;       // BAL_PAIRS: the tile of the second pass, else -1
  long long bh;    // batch * H + head
  int tid, lane, w;
  int x32, h32;    // lane % 32 (index on the 32-axis), lane / 32

  // n_tiles: blocks along T; heavy_last: the cost grows with the tile index
  DEV_INLINE BlockCtx(int n_tiles, int balance, bool heavy_last) {
    tile = blockIdx.x;
    tile2 = -1;
    bh = blockIdx.y;
    if (balance == BAL_HEAVY) {
      const long long id = bh * gridDim.x + tile;   // linear dispatch id
      const int rank = (int)(id / gridDim.y);
      bh = id % gridDim.y;   // gridY % 8 == 0: a head stays on one XCD
      tile = heavy_last ? n_tiles - 1 - rank : rank;
    } else {
      xcd_remap(gridDim.x, gridDim.y, tile, bh);
      if (balance == BAL_PAIRS) {
        // heavier tile first: the lighter one then finds its K/V (Q/dO) in L2
        const int far = n_tiles - 1 - tile;
        if (far != tile) tile2 = heavy_last ? tile : far;
        if (heavy_last) tile = far;
      }
    }
    place_lane();
  }

  // BAL_PAIRS: moves on to the second tile; false when there is none
  DEV_INLINE bool next_pass() {
    if (tile2 < 0) return false;
    tile = tile2;
    tile2 = -1;
    place_lane();
    return true;
  }

  // The lane's place, as values made anew for every pass and for every
  // epilogue (fresh_lane): they are the same each time, and so is every
  // fragment, staging and store offset derived from them. Left visible, the
  // compiler computes all of those before the first pass and keeps them in
  // registers through both (the 32 two-byte store offsets of the old
  // epilogue alone were 64 VGPRs; the forward spilled 432 B).
  DEV_INLINE BlockCtx fresh_lane() const {
    BlockCtx e = *this;
    e.place_lane();
    return e;
  }

  DEV_INLINE void place_lane() {
    tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    lane = tid & (WAVE - 1);
    w = tid / WAVE;
    x32 = lane & 31;
    h32 = lane >> 5;
  }

  // element offset of this block's (batch, head) in a tensor with strides s
  DEV_INLINE long long base(const GStride& s, int H) const {
    return (bh / H) * s.b + (bh % H) * s.h;
  }
};

// Byte offset of this lane's A/B fragment for k-slice s in 32-row half t2 of
// a swizzled [64][64] image: swz(32*t2 + x32, 2*(16*s + 8*h32)). The s/h
// term and the swizzle XOR live in the same byte bits 4-6, so XOR composes
// and the offset is cheap enough to compute at each use: the forward and dkv
// kernels do, which keeps 8 VGPRs free for their staging split.
struct FragOff {
  int row[2];
  int xk;
  int h16;

  DEV_INLINE FragOff(const BlockCtx& c)
      : row{c.x32 * 128, (32 + c.x32) * 128}, xk((c.x32 & 7) << 4),
        h16(16 * c.h32) {}

  DEV_INLINE int operator()(int t2, int s) const {
    return row[t2] + ((s * 32 + h16) ^ xk);
  }
};

// Two-tile LDS pipeline: a pair of [64][64] tiles is staged per iteration,
// with the next pair's global loads in flight under this pair's compute.
//   prime();
//   for (...) { next(lds_a, lds_b, more); __syncthreads();
//               <compute on lds_a / lds_b> }
// Per-tile side inputs ride along as a companion (RowPipe, below), so that
// no load-and-use sits between next() and the barrier.
template <int NT>
struct TilePipe {
  Stage<NT> a, b;
  short8v pend_a[Stage<NT>::REPS], pend_b[Stage<NT>::REPS];

  DEV_INLINE TilePipe(const bf16* ga, int st_a, const bf16* gb, int st_b,
                      int tid)
      : a(ga, tid, st_a), b(gb, tid, st_b) {}

  DEV_INLINE void prime() {
    a.fetch(pend_a);
    b.fetch(pend_b);
  }

  // Barrier (the previous pair is consumed), pending registers -> LDS, and
  // with `more` the loads of the following pair. The caller places the
  // barrier that publishes the tiles.
  DEV_INLINE void next(char* lds_a, char* lds_b, bool more) {
    next(lds_a, lds_b, more, NoRows{});
  }

  // The same with a companion (RowPipe) that rides along: its pending
  // registers go to LDS after the tiles', its loads are issued after the
  // tiles'. Every wait in here is for loads issued a whole iteration
  // earlier; nothing waits between the new loads and the caller's barrier.
  template <typename Rows>
  DEV_INLINE void next(char* lds_a, char* lds_b, bool more, Rows&& rows) {
    __syncthreads();
    a.put(lds_a, pend_a);
    b.put(lds_b, pend_b);
    rows.put();
    if (more) {
      a.advance();
      b.advance();
      a.fetch(pend_a);
      b.fetch(pend_b);
      rows.advance();
      rows.fetch();
    }
  }

  struct NoRows {
    DEV_INLINE void put() {}
    DEV_INLINE void advance() {}
    DEV_INLINE void fetch() {}
  };
};

// TilePipe companion for two fp32 values per tile row (lse and delta in the
// dkv kernel), KVB rows per tile: thread r < KVB (wave 0) carries row r one
// tile ahead in two registers and publishes a[r] * mul_a and b[r] to LDS.
//   pipe.prime(); rows.fetch();
//   for (...) { pipe.next(lds_a, lds_b, more, rows); __syncthreads(); ... }
struct RowPipe {
  const float* ga;   // the pending tile's first row (block-uniform)
  const float* gb;
  float* lds_a;
  float* lds_b;
  float mul_a;
  int tid;
  float pend_a, pend_b;

  DEV_INLINE RowPipe(const float* ga, const float* gb, float* lds_a,
                     float* lds_b, float mul_a, int tid)
      : ga(ga), gb(gb), lds_a(lds_a), lds_b(lds_b), mul_a(mul_a), tid(tid) {}

  DEV_INLINE void fetch() {
    if (tid < KVB) {
      pend_a = ga[tid];
      pend_b = gb[tid];
    }
  }

  DEV_INLINE void put() {
    if (tid < KVB) {
      lds_a[tid] = pend_a * mul_a;
      lds_b[tid] = pend_b;
    }
  }

  DEV_INLINE void advance() {
    ga += KVB;
    gb += KVB;
  }
};

// Counter-based dropout RNG: keyed by (bh, qrow, key) so the backward
// kernels REGENERATE the forward's mask from (seed, indices) — nothing is
// stored, matching the recompute design. 32-bit fold + murmur3 fmix32
// finalizer: the first splitmix64 version kept 64-bit temporaries live
// across the softmax loop and pushed the DROP template into a 312 B/lane
// spill — the avalanche quality of fmix32 is ample for dropout.
// keep <=> rng < keep_thr, keep_thr = (1-p) * 2^32.
struct Dropout {
  unsigned long long seed;
  unsigned keep_thr;
  float inv_keep;   // 1 / (1-p)

  DEV_INLINE bool keep(unsigned long long idx) const {
    unsigned h = (unsigned)(idx ^ (idx >> 32));
    h += (unsigned)seed;
    h ^= (unsigned)(seed >> 32);
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h < keep_thr;
  }
};

// C-layout -> A-fragment repack. Values live per lane as 16 C registers per
// 32-wide tile (packed to bf16 word pairs wA[r1]=(r0=0,1), wB[r1]=(r0=2,3)).
// A-frag slice s (k = 16s + 8*h32 + e at this lane's own 32-axis index)
// takes word pairs from C registers r1 = 2(s&1)+h of BOTH halves: one
// permlane32_swap per word pair delivers own-half and partner-half at once.
struct PackedC {
  unsigned wA[2][4];  // [32-tile][r1]
  unsigned wB[2][4];
};

// `s` is a constant once the caller's slice loop is unrolled.
DEV_INLINE bfrag frag_from_packed(const PackedC& p, int s) {
  const unsigned uA = p.wA[s >> 1][2 * (s & 1)];
  const unsigned vA = p.wA[s >> 1][2 * (s & 1) + 1];
  const unsigned uB = p.wB[s >> 1][2 * (s & 1)];
  const unsigned vB = p.wB[s >> 1][2 * (s & 1) + 1];
  auto rA = __builtin_amdgcn_permlane32_swap(uA, vA, false, false);
  auto rB = __builtin_amdgcn_permlane32_swap(uB, vB, false, false);
  union { bfrag f; unsigned w[4]; } r;
  r.w[0] = rA[0];
  r.w[1] = rB[0];
  r.w[2] = rA[1];
  r.w[3] = rB[1];
  return r.f;
}

DEV_INLINE bfrag load_frag_scaled(const bf16* p, int row, int col, int st,
                                  float s) {
  short8v v = load8(p + (long long)row * st + col);
  union { bfrag f; short w[8]; } r;
#pragma unroll
  for (int e = 0; e < 8; ++e) r.w[e] = bf_pack(bf_elem(v, e) * s);
  return r.f;
}

DEV_INLINE bfrag load_frag(const bf16* p, int row, int col, int st) {
  union { bfrag f; short8v v; } r;
  r.v = load8(p + (long long)row * st + col);
  return r.f;
}

// Epilogue of one wave's 32x64 result, held as two C tiles: element
// (crow(r,h32), 32*dt + x32) = acc[dt][r] * mul(r), stored as bf16 at row
// stride st from p (the wave's first row).
//
// A lane holds one column of the tile, so a direct store is 32 two-byte
// stores per lane. The values go through the wave's own [32][64] bf16 LDS
// image instead (`stage`, STAGE_BYTES, touched by no other wave: no block
// barrier) and leave as whole 128-byte rows: 8 lanes x 16 bytes per row, 4
// store instructions. Same f2bf(acc * mul) values, same bytes in memory.
// Banks: a ds_write_b16 group is one half-wave = 64 contiguous bytes of one
// row; a ds_read_b128 group of 16 lanes covers four 64-byte half rows whose
// offsets mod 256 are all different. Neither needs padding or a swizzle.
constexpr int STAGE_BYTES = 32 * D * 2;

// Orders a wave's LDS writes before its own later LDS reads (and the other
// way round) where the two go through differently typed pointers. The LDS
// runs one wave's accesses in program order; this is for the compiler.
DEV_INLINE void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename F>
DEV_INLINE void store_ctiles(bf16* p, int st, const BlockCtx& c,
                             const f32x16 (&acc)[2], F mul, char* stage) {
  bf16* img = reinterpret_cast<bf16*>(stage);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      img[crow(r, c.h32) * D + dt * 32 + c.x32] = f2bf(acc[dt][r] * mul(r));
  wave_lds_fence();
  const int piece = c.lane & 7;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 8 * i + (c.lane >> 3);
    store8(p + row * st + piece * 8,
           *reinterpret_cast<const short8v*>(stage + row * (D * 2) +
                                             piece * 16));
  }
  wave_lds_fence();   // the image is free for this wave's next result
}

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
// NW=8: cap at 128 VGPR so two 8-wave blocks are resident per CU (at 132
// VGPR the 8-wave granularity rounds occupancy down to ONE block). With
// DROP the no-drop kernel's 128 registers are already full and the cap
// spills 316 B/lane, so dropout takes the relaxed cap (168 VGPR, 1 block/CU),
// which measured faster for it.
constexpr int fwd_min_blocks(int nw, bool drop) {
  return nw == 8 ? (drop ? 3 : 4) : 2;
}

// One Q block (c.tile) of the forward; the kernel below calls it once per
// pass. Everything but `c` and the LDS is re-created per pass; the first
// pipe.next() of a pass holds the barrier that ends the previous pass's reads.
template <int NW, bool DROP>
// DROP: fused attention dropout — the row sum l_run uses the UNMASKED
// exponentials (normalization is the true softmax sum) while the PV
// accumulation consumes masked/rescaled P.
DEV_INLINE void attn_fwd_tile(const BlockCtx& c, char* smem,
                              const bf16* __restrict__ q,
                              const bf16* __restrict__ k,
                              const bf16* __restrict__ v,
                              bf16* __restrict__ o, float* __restrict__ lse,
                              int T, int H, float scale, const GStride& sq,
                              const GStride& so, const Dropout& drop) {
  constexpr int BM = NW * 32;
  constexpr int NT = NW * WAVE;
  char* lds_k = smem;                 // [64][64] keys row-major
  char* lds_v = smem + KVB * D * 2;   // [64][64] values row-major

  const long long boff = c.base(sq, H);
  const bf16* qp = q + boff + (long long)(c.tile * BM) * sq.t;

  TilePipe<NT> pipe(k + boff, sq.t, v + boff, sq.t, c.tid);
  const FragOff kf(c);
  int trb[2][2];
  tr_bases(c.lane, trb);
  const float qscale = scale * LOG2E;
  bfrag q_frag[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    q_frag[s] = load_frag_scaled(qp, c.w * 32 + c.x32, s * 16 + 8 * c.h32,
                                 sq.t, qscale);

  const f32x16 kzero = {};
  f32x16 o_acc[2] = {};
  float m_run = -INFINITY;
  float l_run = 0.f;

  const int row_lo = c.tile * BM + c.w * 32;
  const int row_me = row_lo + c.x32;
  // dropout index base (loop-invariant): idx = base + key
  const unsigned long long drop_base =
      DROP ? ((unsigned long long)c.bh * T + row_me) * T : 0;
  const int n_kv = (c.tile + 1) * BM / KVB;
  pipe.prime();
  for (int j = 0; j < n_kv; ++j) {
    pipe.next(lds_k, lds_v, j + 1 < n_kv);
    __syncthreads();

    const int key0 = j * KVB;
    if (key0 > row_lo + 31) continue;

    // S^T tiles: C[key = 32*t2 + crow(r,h32)][qrow = x32], log2-scaled
    f32x16 st[2];
    __builtin_amdgcn_s_setprio(1);  // favor MFMA-issuing waves (T5)
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      // seed from the loop-invariant zero vector: a per-tile `= {}` init
      // re-emits 16 v_mov per accumulator per tile
      f32x16 acc = MFMA32(lds_read16(lds_k, kf(t2, 0)), q_frag[0], kzero);
#pragma unroll
      for (int s = 1; s < 4; ++s)
        acc = MFMA32(lds_read16(lds_k, kf(t2, s)), q_frag[s], acc);
      st[t2] = acc;
    }
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
          float pe = fast_exp2(st[t2][4 * r1 + e] - m_new);
          psum += pe;
          if (DROP) {
            const int key = key0 + t2 * 32 + crow(4 * r1 + e, c.h32);
            pe = pin(drop.keep(drop_base + key) ? pe * drop.inv_keep : 0.f);
          }
          p[e] = pe;
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
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o_acc[dt][r] *= a_row[r];
    }

    // PV
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bfrag pa = frag_from_packed(P, s);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        o_acc[dt] = MFMA32(pa, tr_bfrag(lds_v, trb[dt][0] + s * 2048,
                                        trb[dt][1] + s * 2048),
                           o_acc[dt]);
    }
    __builtin_amdgcn_s_setprio(0);
  }

  const BlockCtx e = c.fresh_lane();
  float linv_row[16];
#pragma unroll
  for (int r = 0; r < 16; ++r)
    linv_row[r] = fast_rcp(__shfl(l_run, crow(r, e.h32), WAVE));
  const int erow_lo = e.tile * BM + e.w * 32;
  store_ctiles(o + e.base(so, H) + (long long)erow_lo * so.t, so.t, e, o_acc,
               [&](int r) { return linv_row[r]; },
               smem + 2 * KVB * D * 2 + e.w * STAGE_BYTES);
  if (e.lane < 32) {
    lse[e.bh * T + erow_lo + e.x32] = (m_run + log2f(l_run)) * LN2;
  }
}

// LDS of the forward and dq kernels: the K and V tiles, then one staging
// image per wave for the epilogue.
constexpr int attn_lds_bytes(int nw) {
  return 2 * KVB * D * 2 + nw * STAGE_BYTES;
}

template <int NW, bool DROP = false>
__launch_bounds__(NW * WAVE, fwd_min_blocks(NW, DROP))
__global__ void attn_fwd_kernel(const bf16* __restrict__ q,
                                const bf16* __restrict__ k,
                                const bf16* __restrict__ v,
                                bf16* __restrict__ o, float* __restrict__ lse,
                                int T, int H, float scale, GStride sq,
                                GStride so, Dropout drop, int balance) {
  __shared__ __attribute__((aligned(16))) char smem[attn_lds_bytes(NW)];
  BlockCtx c(T / (NW * 32), balance, true);
  do {
    attn_fwd_tile<NW, DROP>(c, smem, q, k, v, o, lse, T, H, scale, sq, so,
                            drop);
  } while (c.next_pass());
}

// ---------------------------------------------------------------------------
// Backward dK/dV: one workgroup per (NW*32)-key block; wave w owns 32 keys.
// ---------------------------------------------------------------------------
// One key block (c.tile, c.x32: key in wave) of dK/dV, called once per pass.
template <int NW, bool DROP>
DEV_INLINE void attn_bwd_dkv_tile(const BlockCtx& c, char* smem,
                                  const bf16* __restrict__ q,
                                  const bf16* __restrict__ k,
                                  const bf16* __restrict__ v,
                                  const bf16* __restrict__ dout,
                                  const float* __restrict__ lse,
                                  const float* __restrict__ delta,
                                  bf16* __restrict__ dk, bf16* __restrict__ dv,
                                  int T, int H, float scale, const GStride& sq,
                                  const GStride& so, const GStride& sd,
                                  const Dropout& drop) {
  constexpr int BK = NW * 32;
  constexpr int NT = NW * WAVE;
  char* lds_q = smem;
  char* lds_do = smem + KVB * D * 2;
  char* stage = smem + 2 * KVB * D * 2 + c.w * STAGE_BYTES;
  float* lds_lse =
      reinterpret_cast<float*>(smem + 2 * KVB * D * 2 + NW * STAGE_BYTES);
  float* lds_dlt = lds_lse + KVB;

  const long long boff = c.base(sq, H);
  const int i0 = c.tile * BK / KVB;   // first Q tile that sees these keys

  TilePipe<NT> pipe(q + boff + (long long)(i0 * KVB) * sq.t, sq.t,
                    dout + c.base(so, H) + (long long)(i0 * KVB) * so.t, so.t,
                    c.tid);
  const FragOff af(c);
  int trb[2][2];
  tr_bases(c.lane, trb);
  const float kscale = scale * LOG2E;
  const int key_lo = c.tile * BK + c.w * 32;
  const int key_me = key_lo + c.x32;
  // dropout index base: idx = base + qrow*T + key_me (qrow*T fits 32 bits)
  const unsigned long long drop_bhTT =
      DROP ? (unsigned long long)c.bh * T * T : 0;
  bfrag k_frag[4], v_frag[4];  // B operands: col = x32, k-slices over D
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    k_frag[s] = load_frag_scaled(k + boff, key_me, s * 16 + 8 * c.h32, sq.t,
                                 kscale);
    v_frag[s] = load_frag(v + boff, key_me, s * 16 + 8 * c.h32, sq.t);
  }

  const f32x16 kzero = {};
  f32x16 dk_acc[2] = {};
  f32x16 dv_acc[2] = {};

  // lse (to log2 space) and delta of each Q tile travel one tile ahead,
  // next to the tile itself
  const long long row0 = c.bh * T + i0 * KVB;
  RowPipe rows(lse + row0, delta + row0, lds_lse, lds_dlt, LOG2E, c.tid);
  pipe.prime();
  rows.fetch();
  for (int i = i0; i < T / KVB; ++i) {
    pipe.next(lds_q, lds_do, i + 1 < T / KVB, rows);
    __syncthreads();

    const int q0 = i * KVB;
    if (q0 + KVB - 1 < key_lo) continue;

    const bool diag = q0 < key_lo + 32;
    const int mask_lo = key_me - q0 - 4 * c.h32;  // diagonal tiles only
    const unsigned drop_rowT =
        DROP ? pin((unsigned)((q0 + 4 * c.h32) * T)) : 0;
    PackedC P, dS;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      // S, dP tiles: C[qrow = 32*t2 + crow(r,h32)][key = x32]
      __builtin_amdgcn_s_setprio(1);
      f32x16 s_acc = MFMA32(lds_read16(lds_q, af(t2, 0)), k_frag[0], kzero);
      f32x16 dp_acc = MFMA32(lds_read16(lds_do, af(t2, 0)), v_frag[0], kzero);
#pragma unroll
      for (int s = 1; s < 4; ++s) {
        s_acc = MFMA32(lds_read16(lds_q, af(t2, s)), k_frag[s], s_acc);
        dp_acc = MFMA32(lds_read16(lds_do, af(t2, s)), v_frag[s], dp_acc);
      }
      __builtin_amdgcn_s_setprio(0);
      // MASK as a compile-time split: `diag` is wave-uniform but inside the
      // unrolled loop the single-version ternary was if-converted into
      // cmp+cndmask+add on EVERY tile (~96 VALU/tile measured in the .s);
      // only ~1 of 16 tiles is diagonal.
      auto consume = [&](auto MASK) {
#pragma unroll
        for (int r1 = 0; r1 < 4; ++r1) {
          float p[4], dsv[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = 4 * r1 + e;
            const int lrow = t2 * 32 + crow(r, c.h32);
            float pp = fast_exp2(s_acc[r] - lds_lse[lrow]);
            // key_me <= q0 + lrow, with the lane's part of lrow moved into
            // mask_lo: the compare is against a literal, where the first
            // form kept one hoisted register per r live across the loop
            if (MASK.value) pp = (t2 * 32 + crow(r, 0) >= mask_lo) ? pp : 0.f;
            float pv = pp;                 // masked/rescaled P feeds dV
            float dpv = dp_acc[r];         // masked/rescaled dP feeds dS
            if (DROP) {
              // (q0 + lrow) * T, split like the mask: lane part + uniform
              const bool keep = drop.keep(
                  drop_bhTT +
                  (drop_rowT + (unsigned)((t2 * 32 + crow(r, 0)) * T)) +
                  key_me);
              pv = keep ? pp * drop.inv_keep : 0.f;
              dpv = keep ? dpv * drop.inv_keep : 0.f;
            }
            p[e] = pv;
            dsv[e] = pp * (dpv - lds_dlt[lrow]);  // scale in epilogue
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
    }

    // dV[key][d] += P^T dO ; dK[key][d] += dS^T Q  (A-frag k = qrow)
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bfrag ap = frag_from_packed(P, s);
      const bfrag as = frag_from_packed(dS, s);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dv_acc[dt] = MFMA32(ap, tr_bfrag(lds_do, trb[dt][0] + s * 2048,
                                         trb[dt][1] + s * 2048),
                            dv_acc[dt]);
        dk_acc[dt] = MFMA32(as, tr_bfrag(lds_q, trb[dt][0] + s * 2048,
                                         trb[dt][1] + s * 2048),
                            dk_acc[dt]);
      }
    }
    __builtin_amdgcn_s_setprio(0);
  }

  // dk, then dv, through the same staging image
  const long long doff = c.base(sd, H) + (long long)(key_lo) * sd.t;
  bf16* dkp = dk + doff;
  bf16* dvp = dv + doff;
  store_ctiles(dkp, sd.t, c, dk_acc, [&](int) { return scale; }, stage);
  store_ctiles(dvp, sd.t, c, dv_acc, [&](int) { return 1.0f; }, stage);
}

template <int NW, bool DROP = false>
// unconstrained VGPRs: the compiler takes ~256 (2 waves/SIMD) — capping to
// 128 (MINW 4) spills 800 B/lane and 170 (MINW 3) still 288 B/lane, and the
// measured time at 256 equals the kernel's best (169.8 us at B8)
__launch_bounds__(NW * WAVE)
__global__ void attn_bwd_dkv_kernel(const bf16* __restrict__ q,
                                    const bf16* __restrict__ k,
                                    const bf16* __restrict__ v,
                                    const bf16* __restrict__ dout,
                                    const float* __restrict__ lse,
                                    const float* __restrict__ delta,
                                    bf16* __restrict__ dk, bf16* __restrict__ dv,
                                    int T, int H, float scale, GStride sq,
                                    GStride so, GStride sd, Dropout drop,
                                    int balance) {
  __shared__ __attribute__((aligned(16)))
  char smem[attn_lds_bytes(NW) + 2 * KVB * 4];   // + lse and delta of a tile
  BlockCtx c(T / (NW * 32), balance, false);
  do {
    attn_bwd_dkv_tile<NW, DROP>(c, smem, q, k, v, dout, lse, delta, dk, dv, T,
                                H, scale, sq, so, sd, drop);
  } while (c.next_pass());
}

// ---------------------------------------------------------------------------
// Backward dQ: one workgroup per (NW*32)-row Q block; wave w owns 32 rows.
// ---------------------------------------------------------------------------
// One Q block (c.tile) of dQ, called once per pass.
template <int NW, bool DROP>
DEV_INLINE void attn_bwd_dq_tile(const BlockCtx& c, char* smem,
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
                                 const Dropout& drop) {
  constexpr int BM = NW * 32;
  constexpr int NT = NW * WAVE;
  char* lds_k = smem;                     // K row-major
  char* lds_v = smem + KVB * D * 2;       // V row-major
  char* stage = smem + 2 * KVB * D * 2 + c.w * STAGE_BYTES;

  const long long boff = c.base(sq, H);
  const long long ooff = c.base(so, H) + (long long)(c.tile * BM) * so.t;
  const bf16* qp = q + boff + (long long)(c.tile * BM) * sq.t;

  TilePipe<NT> pipe(k + boff, sq.t, v + boff, sq.t, c.tid);
  const FragOff fo(c);
  int f_off[2][4];   // kept in registers here: this kernel has them to spare
#pragma unroll
  for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
    for (int s = 0; s < 4; ++s) f_off[t2][s] = fo(t2, s);
  int trb[2][2];
  tr_bases(c.lane, trb);
  const float qscale = scale * LOG2E;
  bfrag q_frag[4], do_frag[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    q_frag[s] = load_frag_scaled(qp, c.w * 32 + c.x32, s * 16 + 8 * c.h32,
                                 sq.t, qscale);
    do_frag[s] = load_frag(dout + ooff, c.w * 32 + c.x32, s * 16 + 8 * c.h32,
                           so.t);
  }
  const int row_lo = c.tile * BM + c.w * 32;
  const int row_me = row_lo + c.x32;
  const unsigned long long drop_base =
      DROP ? ((unsigned long long)c.bh * T + row_me) * T : 0;
  const float lse2_me = lse[c.bh * T + row_me] * LOG2E;
  // delta = rowsum(dO*O) computed here from the fragments already in
  // registers (+ one O load) and PUBLISHED for the dkv kernel, which is
  // launched after this one — replaces a separate full-pass delta kernel.
  float dlt_me = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    union { bfrag f; short8v v8; } ov;
    ov.f = load_frag(o + ooff, c.w * 32 + c.x32, s * 16 + 8 * c.h32, so.t);
    union { bfrag f; short8v v8; } dv;
    dv.f = do_frag[s];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      dlt_me += bf_elem(ov.v8, e) * bf_elem(dv.v8, e);
  }
  dlt_me += __shfl_xor(dlt_me, 32, WAVE);
  if (c.lane < 32) delta[c.bh * T + row_me] = dlt_me;

  const f32x16 kzero = {};
  f32x16 dq_acc[2] = {};

  const int n_kv = (c.tile + 1) * BM / KVB;
  pipe.prime();
  for (int j = 0; j < n_kv; ++j) {
    pipe.next(lds_k, lds_v, j + 1 < n_kv);
    __syncthreads();

    const int key0 = j * KVB;
    if (key0 > row_lo + 31) continue;

    const bool diag = key0 + KVB - 1 > row_lo;
    PackedC dS;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
      // S^T, dP^T tiles: C[key = 32*t2 + crow(r,h32)][qrow = x32]
      __builtin_amdgcn_s_setprio(1);
      f32x16 s_acc = MFMA32(lds_read16(lds_k, f_off[t2][0]), q_frag[0], kzero);
      f32x16 dp_acc = MFMA32(lds_read16(lds_v, f_off[t2][0]), do_frag[0], kzero);
#pragma unroll
      for (int s = 1; s < 4; ++s) {
        s_acc = MFMA32(lds_read16(lds_k, f_off[t2][s]), q_frag[s], s_acc);
        dp_acc = MFMA32(lds_read16(lds_v, f_off[t2][s]), do_frag[s], dp_acc);
      }
      __builtin_amdgcn_s_setprio(0);
      float dsv[16];
      // wave-uniform mask split (same rationale as the dkv kernel)
      auto consume = [&](auto MASK) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float pp = fast_exp2(s_acc[r] - lse2_me);
          if (MASK.value) {
            const int key = key0 + t2 * 32 + crow(r, c.h32);
            pp = (key <= row_me) ? pp : 0.f;
          }
          float dpv = dp_acc[r];
          if (DROP) {
            const int key = key0 + t2 * 32 + crow(r, c.h32);
            dpv = drop.keep(drop_base + key) ? dpv * drop.inv_keep : 0.f;
          }
          dsv[r] = pp * (dpv - dlt_me);
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
    }

    // dQ[qrow][d] += dS K  (A-frag k = key)
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const bfrag as = frag_from_packed(dS, s);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        dq_acc[dt] = MFMA32(as, tr_bfrag(lds_k, trb[dt][0] + s * 2048,
                                         trb[dt][1] + s * 2048),
                            dq_acc[dt]);
    }
    __builtin_amdgcn_s_setprio(0);
  }

  store_ctiles(dq + c.base(sd, H) + (long long)row_lo * sd.t, sd.t, c, dq_acc,
               [&](int) { return scale; }, stage);
}

template <int NW, bool DROP = false>
__launch_bounds__(NW * WAVE)  // capping at 128 VGPR spills 164 B/lane here
__global__ void attn_bwd_dq_kernel(const bf16* __restrict__ q,
                                   const bf16* __restrict__ k,
                                   const bf16* __restrict__ v,
                                   const bf16* __restrict__ o,
                                   const bf16* __restrict__ dout,
                                   const float* __restrict__ lse,
                                   float* __restrict__ delta,
                                   bf16* __restrict__ dq, int T, int H,
                                   float scale, GStride sq, GStride so,
                                   GStride sd, Dropout drop, int balance) {
  __shared__ __attribute__((aligned(16))) char smem[attn_lds_bytes(NW)];
  BlockCtx c(T / (NW * 32), balance, true);
  do {
    attn_bwd_dq_tile<NW, DROP>(c, smem, q, k, v, o, dout, lse, delta, dq, T, H,
                               scale, sq, so, sd, drop);
  } while (c.next_pass());
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
static GStride gstride(const long long* s) { return {s[0], s[1], (int)s[2]}; }

static Dropout make_dropout(float p, unsigned long long seed) {
  const double keepd = 1.0 - (double)p;
  // clamp: for p -> 0, keepd*2^32 == 2^32 overflows (unsigned) to 0 and
  // would drop EVERYTHING instead of nothing
  const double thr_d = keepd * 4294967296.0;
  const unsigned keep_thr =
      thr_d >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)thr_d;
  return {seed, keep_thr, (float)(1.0 / keepd)};
}

// Calls f(NW, DROP) as std::integral_constants. NW is the widest block that
// divides T, capped by the knob `nw_env` (2, 4 or 8, anything else counts as
// the default 8; read at every launch — within-box A/B, because box-to-box
// wall-clock noise is ~3%). 8-wave blocks are the measured best: backward
// 285us vs 332us for 4-wave at B8/H16/T1024 (pre-tr16), staging
// amortization across 8 waves beat block overlap.
template <typename F>
static void attn_dispatch(int T, const char* nw_env, bool drop, F f) {
  const long long knob = env_int(nw_env, 8);
  const int nw_max = (knob == 2 || knob == 4) ? (int)knob : 8;
  auto with_nw = [&](auto DROP) {
    if (T % 256 == 0 && nw_max == 8) f(std::integral_constant<int, 8>{}, DROP);
    else if (T % 128 == 0 && nw_max >= 4) f(std::integral_constant<int, 4>{}, DROP);
    else f(std::integral_constant<int, 2>{}, DROP);
  };
  if (drop) with_nw(std::true_type{}); else with_nw(std::false_type{});
}

// Workgroups of `Kernel` that the device holds at once (CUs x resident
// blocks per CU, as the runtime computes it from the kernel's registers and
// LDS); asked once per kernel.
template <auto Kernel>
static long long resident_blocks(int threads) {
  static const long long n = [&]() -> long long {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, Kernel, threads,
                                                     0) != hipSuccess) {
      (void)hipGetLastError();
      return 0;
    }
    return (long long)cus * per_cu;
  }();
  return n;
}

// The tile mapping and the grid of one launch. TDSA_ATTN_BALANCE, read at
// every launch:
//   0  one tile per workgroup, in windows of 8 heads (the mapping up to here)
//   1  (default) tile pairs where the halved grid still fills every resident
//      slot of the device, otherwise 2
//   2  one tile per workgroup, the heaviest tiles of the whole grid first
//  -1  tile pairs whatever the grid (small grids in tests)
// Measured at H=16, T=1024 (profiles/attn_balance.txt): at B=32 pairs take
// the forward from 161 to 129 us and the backward from 536 to 381 us, 2 is
// level in the forward and 2 % behind in the backward; at B=8 the forward's
// 256 pairs would fill half of its 512 slots, and 2 takes it from 47 to 38 us.
struct TileMap {
  int balance;
  dim3 grid;
};

template <auto Kernel>
static TileMap tile_map(int n_tiles, long long bh, int threads) {
  int balance = (int)env_int("TDSA_ATTN_BALANCE", BAL_PAIRS);
  const bool forced = balance == -1;
  if (balance < BAL_OFF || balance > BAL_HEAVY) balance = BAL_PAIRS;
  const int n_pairs = (n_tiles + 1) / 2;
  if (balance == BAL_PAIRS && !forced &&
      n_pairs * bh < resident_blocks<Kernel>(threads))
    balance = BAL_HEAVY;
  return {balance, dim3(balance == BAL_PAIRS ? n_pairs : n_tiles, bh)};
}

}  // namespace tdsa

using namespace tdsa;

extern "C" {

// strides arrays: {b, h, t} in elements, per tensor group:
// sq = q/k/v, so = o (and dO in bwd), sd = dq/dk/dv.
// dropout_p > 0 enables the fused-dropout template (seed regenerates the
// identical mask in the backward kernels).
hipError_t tdsa_attn_fwd(const void* q, const void* k, const void* v, void* o,
                         float* lse, long long B, long long H, int T,
                         float scale, const long long* sq_in,
                         const long long* so_in, float dropout_p,
                         unsigned long long seed, hipStream_t stream) {
  if (T % KVB) return hipErrorInvalidValue;
  const GStride sq = gstride(sq_in), so = gstride(so_in);
  const Dropout drop = make_dropout(dropout_p, seed);
  attn_dispatch(T, "TDSA_ATTN_FWD_NW", dropout_p > 0.0f, [&](auto nw, auto dr) {
    constexpr int NW = decltype(nw)::value;
    constexpr auto fwd = attn_fwd_kernel<NW, decltype(dr)::value>;
    const TileMap m = tile_map<fwd>(T / (NW * 32), B * H, NW * WAVE);
    hipLaunchKernelGGL(fwd, m.grid, dim3(NW * WAVE), 0, stream,
                       (const bf16*)q, (const bf16*)k, (const bf16*)v,
                       (bf16*)o, lse, T, (int)H, scale, sq, so, drop,
                       m.balance);
  });
  return hipGetLastError();
}

hipError_t tdsa_attn_bwd(const void* q, const void* k, const void* v,
                         const void* o, const float* lse, const void* dout,
                         void* dq, void* dk, void* dv, float* delta,
                         long long B, long long H, int T, float scale,
                         const long long* sq_in, const long long* so_in,
                         const long long* sd_in, float dropout_p,
                         unsigned long long seed, hipStream_t stream) {
  if (T % KVB) return hipErrorInvalidValue;
  const GStride sq = gstride(sq_in), so = gstride(so_in), sd = gstride(sd_in);
  const Dropout drop = make_dropout(dropout_p, seed);
  // dq runs FIRST: it computes and publishes delta = rowsum(dO*O) from
  // fragments it loads anyway; dkv (same stream) consumes it.
  attn_dispatch(T, "TDSA_ATTN_BWD_NW", dropout_p > 0.0f, [&](auto nw, auto dr) {
    constexpr int NW = decltype(nw)::value;
    constexpr bool DROP = decltype(dr)::value;
    constexpr auto dq_k = attn_bwd_dq_kernel<NW, DROP>;
    constexpr auto dkv_k = attn_bwd_dkv_kernel<NW, DROP>;
    const dim3 block(NW * WAVE);
    // the two kernels differ in residency, so each gets its own mapping
    const TileMap mq = tile_map<dq_k>(T / (NW * 32), B * H, NW * WAVE);
    const TileMap mkv = tile_map<dkv_k>(T / (NW * 32), B * H, NW * WAVE);
    hipLaunchKernelGGL(dq_k, mq.grid, block, 0, stream,
                       (const bf16*)q, (const bf16*)k, (const bf16*)v,
                       (const bf16*)o, (const bf16*)dout, lse, delta,
                       (bf16*)dq, T, (int)H, scale, sq, so, sd, drop,
                       mq.balance);
    hipLaunchKernelGGL(dkv_k, mkv.grid, block, 0, stream,
                       (const bf16*)q, (const bf16*)k, (const bf16*)v,
                       (const bf16*)dout, lse, delta, (bf16*)dk, (bf16*)dv, T,
                       (int)H, scale, sq, so, sd, drop, mkv.balance);
  });
  return hipGetLastError();
}

}  // extern "C"
