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
// The three kernels share one skeleton (attn_common.h, used by the head-dim-128
// kernels of attention_d128.hip as well): BlockCtx (block prologue), TilePipe
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
// Contract: bf16, head_dim 64, any T >= 1. T % 64 == 0 runs the kernels as
// described above; any other T their tail variants ("Ragged T" below), which
// handle the partial last tile and read or write no row >= T.
#include "common.h"
#include "launchers.h"
#include "attn_common.h"
#include "mfma.h"

#include <type_traits>

namespace tdsa {

constexpr int D = 64;     // head dim (all GPT-2 sizes)

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
// TAIL (ragged T): only the wave's first `rows` rows (any value; <= 0: none)
// exist and are stored.
constexpr int STAGE_BYTES = 32 * D * 2;

template <bool TAIL = false, typename F>
DEV_INLINE void store_ctiles(bf16* p, int st, const BlockCtx& c,
                             const f32x16 (&acc)[2], F mul, char* stage,
                             int rows = 32) {
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
    if constexpr (TAIL) {
      if (row >= rows) continue;
    }
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
template <int NW, bool DROP, bool TAIL>
// DROP: fused attention dropout — the row sum l_run uses the UNMASKED
// exponentials (normalization is the true softmax sum) while the PV
// accumulation consumes masked/rescaled P.
// TAIL: ragged T, see "Ragged T" above the tail kernels.
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

  const int row_lo = c.tile * BM + c.w * 32;
  const int row_me = row_lo + c.x32;

  TilePipe<NT, TAIL> pipe(k + boff, sq.t, v + boff, sq.t, c.tid, T);
  const FragOff kf(c);
  int trb[2][2];
  tr_bases(c.lane, trb);
  const float qscale = scale * LOG2E;
  bfrag q_frag[4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
    q_frag[s] = load_frag_scaled<TAIL>(qp, c.w * 32 + c.x32,
                                       s * 16 + 8 * c.h32, sq.t, qscale,
                                       row_me < T);

  const f32x16 kzero = {};
  f32x16 o_acc[2] = {};
  float m_run = -INFINITY;
  float l_run = 0.f;

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
    if constexpr (TAIL) {
      if (row_lo >= T) continue;   // a wave of padded rows only
    }

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
  store_ctiles<TAIL>(o + e.base(so, H) + (long long)erow_lo * so.t, so.t, e,
                     o_acc, [&](int r) { return linv_row[r]; },
                     smem + 2 * KVB * D * 2 + e.w * STAGE_BYTES, T - erow_lo);
  if (e.lane < 32 && (!TAIL || erow_lo + e.x32 < T)) {
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
    attn_fwd_tile<NW, DROP, false>(c, smem, q, k, v, o, lse, T, H, scale, sq,
                                   so, drop);
  } while (c.next_pass());
}

// Ragged T (T % 64 != 0): the tail kernels. They are the kernels above with
// TAIL set in their tile functions, on ceil(T / (NW*32)) blocks along T, NW
// chosen for T rounded up to 64 (so NW*32 divides that, and the last K/V or
// Q/dO tile of every loop is the one tile that holds row T-1). Rows >= T of a
// (batch, head) do not exist: in the packed layout "row T" is row 0 of the
// next batch. So
//   - no global read touches a row >= T: staged chunks (TilePipe), pinned
//     fragments (load_frag*<TAIL>) and lse/delta (RowPipe<TAIL>, dq prologue)
//     are predicated and arrive as zeros (lse: +inf);
//   - nothing is stored to a row >= T (store_ctiles<TAIL>, lse, delta);
//   - a wave whose 32 rows (keys in dkv) are all >= T skips its compute and
//     keeps its barriers, like a wave above the diagonal.
// A padded key is above the diagonal of every row < T, and a padded row adds
// P = 0, dS = 0 times Q = 0, dO = 0 to dK/dV of the keys < T: exact zeros,
// so rows < T carry the bits of the aligned kernels on the zero-padded
// problem. Separate __global__ functions: they take their own launch bounds
// and are compiled without packed fp32 math (TAIL_TARGET).
#if defined(__HIP_DEVICE_COMPILE__)
#define TAIL_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define TAIL_TARGET
#endif

template <int NW, bool DROP = false>
__launch_bounds__(NW * WAVE, fwd_min_blocks(NW, DROP))
TAIL_TARGET
__global__ void attn_fwd_tail_kernel(const bf16* __restrict__ q,
                                     const bf16* __restrict__ k,
                                     const bf16* __restrict__ v,
                                     bf16* __restrict__ o,
                                     float* __restrict__ lse, int T, int H,
                                     float scale, GStride sq, GStride so,
                                     Dropout drop, int balance) {
  __shared__ __attribute__((aligned(16))) char smem[attn_lds_bytes(NW)];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, true);
  do {
    attn_fwd_tile<NW, DROP, true>(c, smem, q, k, v, o, lse, T, H, scale, sq,
                                  so, drop);
  } while (c.next_pass());
}

// ---------------------------------------------------------------------------
// Backward dK/dV: one workgroup per (NW*32)-key block; wave w owns 32 keys.
// ---------------------------------------------------------------------------
// One key block (c.tile, c.x32: key in wave) of dK/dV, called once per pass.
template <int NW, bool DROP, bool TAIL>
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

  TilePipe<NT, TAIL> pipe(q + boff + (long long)(i0 * KVB) * sq.t, sq.t,
                          dout + c.base(so, H) + (long long)(i0 * KVB) * so.t,
                          so.t, c.tid, T - i0 * KVB);
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
    k_frag[s] = load_frag_scaled<TAIL>(k + boff, key_me, s * 16 + 8 * c.h32,
                                       sq.t, kscale, key_me < T);
    v_frag[s] = load_frag<TAIL>(v + boff, key_me, s * 16 + 8 * c.h32, sq.t,
                                key_me < T);
  }

  const f32x16 kzero = {};
  f32x16 dk_acc[2] = {};
  f32x16 dv_acc[2] = {};

  // lse (to log2 space) and delta of each Q tile travel one tile ahead,
  // next to the tile itself
  const long long row0 = c.bh * T + i0 * KVB;
  RowPipe<TAIL> rows(lse + row0, delta + row0, lds_lse, lds_dlt, LOG2E, c.tid,
                     T - i0 * KVB);
  pipe.prime();
  rows.fetch();
  // Q tiles in all (a name for what the loop reads per iteration)
  auto n_q = [&]() { return TAIL ? (T + KVB - 1) / KVB : T / KVB; };
  for (int i = i0; i < n_q(); ++i) {
    pipe.next(lds_q, lds_do, i + 1 < n_q(), rows);
    __syncthreads();

    const int q0 = i * KVB;
    if (q0 + KVB - 1 < key_lo) continue;
    if constexpr (TAIL) {
      if (key_lo >= T) continue;   // a wave of padded keys only
    }

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
  store_ctiles<TAIL>(dkp, sd.t, c, dk_acc, [&](int) { return scale; }, stage,
                     T - key_lo);
  store_ctiles<TAIL>(dvp, sd.t, c, dv_acc, [&](int) { return 1.0f; }, stage,
                     T - key_lo);
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
    attn_bwd_dkv_tile<NW, DROP, false>(c, smem, q, k, v, dout, lse, delta, dk,
                                       dv, T, H, scale, sq, so, sd, drop);
  } while (c.next_pass());
}

template <int NW, bool DROP = false>
__launch_bounds__(NW * WAVE)
TAIL_TARGET
__global__ void attn_bwd_dkv_tail_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    bf16* __restrict__ dk, bf16* __restrict__ dv, int T, int H, float scale,
    GStride sq, GStride so, GStride sd, Dropout drop, int balance) {
  __shared__ __attribute__((aligned(16)))
  char smem[attn_lds_bytes(NW) + 2 * KVB * 4];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, false);
  do {
    attn_bwd_dkv_tile<NW, DROP, true>(c, smem, q, k, v, dout, lse, delta, dk,
                                      dv, T, H, scale, sq, so, sd, drop);
  } while (c.next_pass());
}

// ---------------------------------------------------------------------------
// Backward dQ: one workgroup per (NW*32)-row Q block; wave w owns 32 rows.
// ---------------------------------------------------------------------------
// One Q block (c.tile) of dQ, called once per pass.
template <int NW, bool DROP, bool TAIL>
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

  // TAIL: this lane's row exists
  const bool row_ok = !TAIL || c.tile * BM + c.w * 32 + c.x32 < T;

  TilePipe<NT, TAIL> pipe(k + boff, sq.t, v + boff, sq.t, c.tid, T);
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
    q_frag[s] = load_frag_scaled<TAIL>(qp, c.w * 32 + c.x32,
                                       s * 16 + 8 * c.h32, sq.t, qscale,
                                       row_ok);
    do_frag[s] = load_frag<TAIL>(dout + ooff, c.w * 32 + c.x32,
                                 s * 16 + 8 * c.h32, so.t, row_ok);
  }
  const int row_lo = c.tile * BM + c.w * 32;
  const int row_me = row_lo + c.x32;
  const unsigned long long drop_base =
      DROP ? ((unsigned long long)c.bh * T + row_me) * T : 0;
  // a padded row: lse = +inf, so that P = exp2(s - inf) is exactly 0
  float lse2_me = INFINITY;
  if (row_ok) lse2_me = lse[c.bh * T + row_me] * LOG2E;
  // delta = rowsum(dO*O) computed here from the fragments already in
  // registers (+ one O load) and PUBLISHED for the dkv kernel, which is
  // launched after this one — replaces a separate full-pass delta kernel.
  float dlt_me = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    union { bfrag f; short8v v8; } ov;
    ov.f = load_frag<TAIL>(o + ooff, c.w * 32 + c.x32, s * 16 + 8 * c.h32,
                           so.t, row_ok);
    union { bfrag f; short8v v8; } dv;
    dv.f = do_frag[s];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      dlt_me += bf_elem(ov.v8, e) * bf_elem(dv.v8, e);
  }
  dlt_me += __shfl_xor(dlt_me, 32, WAVE);
  if (c.lane < 32 && row_ok) delta[c.bh * T + row_me] = dlt_me;

  const f32x16 kzero = {};
  f32x16 dq_acc[2] = {};

  const int n_kv = (c.tile + 1) * BM / KVB;
  pipe.prime();
  for (int j = 0; j < n_kv; ++j) {
    pipe.next(lds_k, lds_v, j + 1 < n_kv);
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

  store_ctiles<TAIL>(dq + c.base(sd, H) + (long long)row_lo * sd.t, sd.t, c,
                     dq_acc, [&](int) { return scale; }, stage, T - row_lo);
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
    attn_bwd_dq_tile<NW, DROP, false>(c, smem, q, k, v, o, dout, lse, delta,
                                      dq, T, H, scale, sq, so, sd, drop);
  } while (c.next_pass());
}

template <int NW, bool DROP = false>
__launch_bounds__(NW * WAVE)
TAIL_TARGET
__global__ void attn_bwd_dq_tail_kernel(
    const bf16* __restrict__ q, const bf16* __restrict__ k,
    const bf16* __restrict__ v, const bf16* __restrict__ o,
    const bf16* __restrict__ dout, const float* __restrict__ lse,
    float* __restrict__ delta, bf16* __restrict__ dq, int T, int H,
    float scale, GStride sq, GStride so, GStride sd, Dropout drop,
    int balance) {
  __shared__ __attribute__((aligned(16))) char smem[attn_lds_bytes(NW)];
  BlockCtx c((T + NW * 32 - 1) / (NW * 32), balance, true);
  do {
    attn_bwd_dq_tile<NW, DROP, true>(c, smem, q, k, v, o, dout, lse, delta, dq,
                                     T, H, scale, sq, so, sd, drop);
  } while (c.next_pass());
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

// Calls f(NW, DROP, TAIL) as std::integral_constants. TAIL: T % 64 != 0.
// NW is the widest block that divides T rounded up to 64, capped by the knob
// `nw_env` (2, 4 or 8, anything else counts as the default 8; read at every
// launch — within-box A/B, because box-to-box wall-clock noise is ~3%).
// 8-wave blocks are the measured best: backward 285us vs 332us for 4-wave at
// B8/H16/T1024 (pre-tr16), staging amortization across 8 waves beat block
// overlap.
template <typename F>
static void attn_dispatch(int T, const char* nw_env, bool drop, F f) {
  const long long knob = env_int(nw_env, 8);
  const int nw_max = (knob == 2 || knob == 4) ? (int)knob : 8;
  const int T64 = (T + KVB - 1) / KVB * KVB;
  auto with_nw = [&](auto DROP, auto TAIL) {
    if (T64 % 256 == 0 && nw_max == 8)
      f(std::integral_constant<int, 8>{}, DROP, TAIL);
    else if (T64 % 128 == 0 && nw_max >= 4)
      f(std::integral_constant<int, 4>{}, DROP, TAIL);
    else
      f(std::integral_constant<int, 2>{}, DROP, TAIL);
  };
  auto with_drop = [&](auto TAIL) {
    if (drop) with_nw(std::true_type{}, TAIL);
    else with_nw(std::false_type{}, TAIL);
  };
  if (T % KVB) with_drop(std::true_type{}); else with_drop(std::false_type{});
}

// The three kernels of one (NW, DROP, TAIL).
template <int NW, bool DROP, bool TAIL>
struct AttnKernels {
  static constexpr auto fwd =
      TAIL ? attn_fwd_tail_kernel<NW, DROP> : attn_fwd_kernel<NW, DROP>;
  static constexpr auto dq =
      TAIL ? attn_bwd_dq_tail_kernel<NW, DROP> : attn_bwd_dq_kernel<NW, DROP>;
  static constexpr auto dkv = TAIL ? attn_bwd_dkv_tail_kernel<NW, DROP>
                                   : attn_bwd_dkv_kernel<NW, DROP>;
};

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
  if (T < 1) return hipErrorInvalidValue;
  const GStride sq = gstride(sq_in), so = gstride(so_in);
  const Dropout drop = make_dropout(dropout_p, seed);
  attn_dispatch(T, "TDSA_ATTN_FWD_NW", dropout_p > 0.0f,
                [&](auto nw, auto dr, auto tl) {
    constexpr int NW = decltype(nw)::value;
    constexpr auto fwd =
        AttnKernels<NW, decltype(dr)::value, decltype(tl)::value>::fwd;
    const int n_tiles = (T + NW * 32 - 1) / (NW * 32);
    const TileMap m = tile_map<fwd>(n_tiles, B * H, NW * WAVE);
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
  if (T < 1) return hipErrorInvalidValue;
  const GStride sq = gstride(sq_in), so = gstride(so_in), sd = gstride(sd_in);
  const Dropout drop = make_dropout(dropout_p, seed);
  // dq runs FIRST: it computes and publishes delta = rowsum(dO*O) from
  // fragments it loads anyway; dkv (same stream) consumes it.
  attn_dispatch(T, "TDSA_ATTN_BWD_NW", dropout_p > 0.0f,
                [&](auto nw, auto dr, auto tl) {
    constexpr int NW = decltype(nw)::value;
    using K = AttnKernels<NW, decltype(dr)::value, decltype(tl)::value>;
    constexpr auto dq_k = K::dq;
    constexpr auto dkv_k = K::dkv;
    const dim3 block(NW * WAVE);
    const int n_tiles = (T + NW * 32 - 1) / (NW * 32);
    // the two kernels differ in residency, so each gets its own mapping
    const TileMap mq = tile_map<dq_k>(n_tiles, B * H, NW * WAVE);
    const TileMap mkv = tile_map<dkv_k>(n_tiles, B * H, NW * WAVE);
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
