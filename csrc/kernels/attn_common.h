// Skeleton shared by the fused attention kernel files (attention.hip: head
// dim 64; attention_d128.hip: head dim 128): the workgroup -> tile mapping
// (xcd_remap, BlockCtx, tile_map), the two-tile LDS pipeline with its row
// companion (TilePipe, RowPipe), fragment offsets and loads (FragOff,
// load_frag*), the C-layout -> A-fragment repack (PackedC,
// frag_from_packed) and the dropout RNG (Dropout, make_dropout), one copy so
// that both head dims realise one mask. Everything here works on 64-row tiles of swizzled
// [64][64] bf16 images (mfma.h); nothing depends on the head dim.
#pragma once

#include "common.h"
#include "mfma.h"

namespace tdsa {

constexpr int KVB = 64;   // keys / rows per LDS tile

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

// Counter-based dropout RNG: keyed by (bh, qrow, key) so the backward
// kernels REGENERATE the forward's mask from (seed, indices) — nothing is
// stored, matching the recompute design. 32-bit fold + murmur3 fmix32
// finalizer: the first splitmix64 version kept 64-bit temporaries live
// across the softmax loop and pushed the DROP template into a 312 B/lane
// spill — the avalanche quality of fmix32 is ample for dropout.
// keep <=> rng < keep_thr, keep_thr = (1-p) * 2^32.
// The index of score (bh, qrow, key) is (bh * T + qrow) * T + key on the real
// T at every head dim, block geometry and tile mapping: one (B, H, T, p,
// seed) is one mask.
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

static Dropout make_dropout(float p, unsigned long long seed) {
  const double keepd = 1.0 - (double)p;
  // clamp: for p -> 0, keepd*2^32 == 2^32 overflows (unsigned) to 0 and
  // would drop EVERYTHING instead of nothing
  const double thr_d = keepd * 4294967296.0;
  const unsigned keep_thr =
      thr_d >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)thr_d;
  return {seed, keep_thr, (float)(1.0 / keepd)};
}


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
//
// TAIL (ragged T): `left` is the number of rows that the pending pair has in
// memory, counted from its first row; the constructor takes it for the first
// pair. A pair with left >= KVB is fetched as in the aligned kernels; the one
// pair that holds row T-1 takes the predicated fetch (a block-uniform
// branch, so whole tiles pay one scalar compare), reads no row >= T and puts
// zeros in their place. The tail's state is an empty base in the aligned
// kernels: as plain members that they never read it still changed the
// register allocation of the 4-wave dkv kernel.
template <bool TAIL>
struct TailRows {
  DEV_INLINE TailRows(int, int) {}
};
template <>
struct TailRows<true> {
  int tid, left;
  DEV_INLINE TailRows(int tid, int left) : tid(tid), left(left) {}
};

template <int NT, bool TAIL = false>
struct TilePipe : TailRows<TAIL> {
  Stage<NT> a, b;
  short8v pend_a[Stage<NT>::REPS], pend_b[Stage<NT>::REPS];

  DEV_INLINE TilePipe(const bf16* ga, int st_a, const bf16* gb, int st_b,
                      int tid, int left = 0)
      : TailRows<TAIL>(tid, left), a(ga, tid, st_a), b(gb, tid, st_b) {}

  DEV_INLINE void fetch() {
    if constexpr (TAIL) {
      if (this->left < KVB) {
        a.fetch_rows(pend_a, this->tid, this->left);
        b.fetch_rows(pend_b, this->tid, this->left);
        return;
      }
    }
    a.fetch(pend_a);
    b.fetch(pend_b);
  }

  DEV_INLINE void prime() { fetch(); }

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
      if constexpr (TAIL) this->left -= KVB;
      fetch();
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
// TAIL (ragged T): `left` rows of the pending tile exist; a later row is not
// read and carries a = +inf (lse: P = exp2(s - inf) is exactly 0) and b = 0.
template <bool TAIL = false>
struct RowPipe {
  const float* ga;   // the pending tile's first row (block-uniform)
  const float* gb;
  float* lds_a;
  float* lds_b;
  float mul_a;
  int tid;
  int left;   // TAIL only
  float pend_a, pend_b;

  DEV_INLINE RowPipe(const float* ga, const float* gb, float* lds_a,
                     float* lds_b, float mul_a, int tid, int left = 0)
      : ga(ga), gb(gb), lds_a(lds_a), lds_b(lds_b), mul_a(mul_a), tid(tid),
        left(left) {}

  DEV_INLINE void fetch() {
    if constexpr (TAIL) {
      if (tid < KVB) {
        pend_a = INFINITY;
        pend_b = 0.f;
        if (tid < left) {
          pend_a = ga[tid];
          pend_b = gb[tid];
        }
      }
    } else if (tid < KVB) {
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
    if constexpr (TAIL) left -= KVB;
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

// TAIL (ragged T): the fragment of a row that does not exist (`ok` false) is
// not read and is all zeros; a zero row scaled is a zero row.
template <bool TAIL>
DEV_INLINE bfrag load_frag_scaled(const bf16* p, int row, int col, int st,
                                  float s, bool ok) {
  if constexpr (TAIL) {
    if (!ok) return bfrag{};
  }
  return load_frag_scaled(p, row, col, st, s);
}

template <bool TAIL>
DEV_INLINE bfrag load_frag(const bf16* p, int row, int col, int st, bool ok) {
  if constexpr (TAIL) {
    if (!ok) return bfrag{};
  }
  return load_frag(p, row, col, st);
}


// Orders a wave's LDS writes before its own later LDS reads (and the other
// way round) where the two go through differently typed pointers. The LDS
// runs one wave's accesses in program order; this is for the compiler.
DEV_INLINE void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

static GStride gstride(const long long* s) { return {s[0], s[1], (int)s[2]}; }


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
