// bf16 2-D transpose out[K, N] = in[N, K]^T for the linear layers' input
// gradient: with W^T held row-major, dx = dy @ W is the forward's GEMM layout
// (both operands contiguous along the contraction), see ops/linear.py.
//
// One 64x64 tile per wave, kWaves waves per workgroup, no loop: the tile is
// read with 8 x 16-byte global loads per lane along K (8 lanes = one 128-byte
// row), written to the wave's own 8 KiB LDS image as 16-byte chunks, read
// back with the gfx950 hardware-transposed read (ds_read_tr16_b64, two per
// 16-byte result) and written with 8 x 16-byte global stores per lane along
// N. One store instruction covers 16 output rows x 64 contiguous bytes; the
// next one completes those rows' 128-byte lines.
//
// LDS image: the swizzled image with the transposed read, not the padded one
// (a padded image has no conflict-free 16-byte-per-lane column read: it
// needs eight 2-byte reads per result). The swizzle is NOT mfma.h's swz():
// that one is built for the attention fragments, whose 32-lane half reads 4
// rows x 64 bytes; here a half reads 8 rows x 32 bytes (rows R..R+3 and
// R+8..R+11, one 16-column block), and under swz() rows R and R+8 land on
// the same banks (2-way). Rows are 128 bytes, so rows r and r+1 already
// split the 64 banks; tr_off() moves the 32-byte slot of a row by
// slot(r) = bit1(r) | bit3(r) << 1, which sends the four even (and the four
// odd) rows of such a read to four different slots: every
// transposed read touches each bank once. The 16-byte writes stay whole (the
// XOR moves 32-byte slots) and a group of 8 lanes writes one full row, so
// they are conflict-free as well.
#include "common.h"
#include "launchers.h"
#include "mfma.h"

#include <climits>

namespace tdsa {

constexpr int kTrWaves = 4;               // tiles per workgroup
constexpr int kTrTileBytes = 64 * 64 * 2;

// Byte offset of (row, byte_in_row) in the [64][64] bf16 image.
DEV_INLINE int tr_off(int row, int byte_in_row) {
  const int slot = ((row >> 1) & 1) | (((row >> 3) & 1) << 1);
  return row * 128 + (byte_in_row ^ (slot << 5));
}

__global__ __launch_bounds__(kTrWaves * WAVE) void transpose_bf16_kernel(
    const bf16* __restrict__ in, bf16* __restrict__ out, int N, int K,
    long long tiles) {
  __shared__ __attribute__((aligned(16))) char image[kTrWaves * kTrTileBytes];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  char* lds = image + wave * kTrTileBytes;
  // consecutive waves take consecutive tiles along K: the same 64 input rows
  const long long tile = (long long)blockIdx.x * kTrWaves + wave;
  const bool active = tile < tiles;  // wave-uniform: EXEC stays all ones
  const int ktiles = K >> 6;
  const long long n0 = (tile / ktiles) * 64;
  const long long k0 = (tile % ktiles) * 64;

  if (active) {
    const int row = lane >> 3;       // + 8 per rep
    const int chunk = lane & 7;      // 16-byte chunk of the 128-byte row
    const bf16* src = in + (n0 + row) * K + k0 + chunk * 8;
    short8v buf[8];
#pragma unroll
    for (int rep = 0; rep < 8; ++rep) buf[rep] = load8(src + (long long)rep * 8 * K);
#pragma unroll
    for (int rep = 0; rep < 8; ++rep)
      *reinterpret_cast<short8v*>(lds + tr_off(row + 8 * rep, chunk * 16)) =
          buf[rep];
  }
  __syncthreads();
  if (active) {
    // 16-lane group g reads, for column block cb, the image rows
    // R..R+7 (R = 32*s + 8*g) at columns 16*cb..16*cb+15; lane i of the group
    // supplies row q = i >> 2, columns 4*(i & 3).. and receives column i.
    const int g = lane >> 4;
    const int i = lane & 15;
    const int q = i >> 2;
    const int colbyte = 8 * (i & 3);
    bf16* dst = out + (k0 + i) * N + n0 + 8 * g;
#pragma unroll
    for (int cb = 0; cb < 4; ++cb)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int R = 32 * s + 8 * g + q;
        const bfrag v = tr_bfrag(lds, tr_off(R, 32 * cb + colbyte),
                                 tr_off(R + 4, 32 * cb + colbyte));
        store8(dst + (long long)(16 * cb) * N + 32 * s, v);
      }
  }
}

}  // namespace tdsa

using namespace tdsa;

extern "C" hipError_t tdsa_transpose_bf16(const void* in, void* out,
                                          long long N, long long K,
                                          hipStream_t stream) {
  if (N <= 0 || K <= 0 || N % 64 != 0 || K % 64 != 0 || N > INT_MAX ||
      K > INT_MAX)
    return hipErrorInvalidValue;
  const long long tiles = (N / 64) * (K / 64);
  const long long grid = (tiles + kTrWaves - 1) / kTrWaves;
  if (grid > INT_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(transpose_bf16_kernel, dim3((unsigned)grid),
                     dim3(kTrWaves * WAVE), 0, stream, (const bf16*)in,
                     (bf16*)out, (int)N, (int)K, tiles);
  return hipGetLastError();
}
