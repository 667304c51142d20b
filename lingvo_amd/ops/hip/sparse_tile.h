// What the list-walking attention kernels (block_sparse_attn.hip,
// routing_attn.hip) share on top of attn_tile.h: the 64-token tile geometry,
// a 64 x H tile held in registers between global memory and LDS, and a
// wave's fp32 strip going to LDS as MFMA A operands. How the registers are
// filled (contiguous rows, gathered rows) stays with each kernel file.
//
// Included inside the target-attribute region of its translation unit, like
// attn_tile.h.
#pragma once

#include "attn_tile.h"

namespace {

constexpr int BT = 64;                  // tile edge, queries and keys
constexpr int BNW = 4;                  // waves per block
constexpr int BBLOCK = BNW * WAVE_SIZE;
constexpr int TP = BT * 2;              // byte pitch of a [.][64] bf16 tile
constexpr int NF = BT / 16;             // 16-wide fragments across a tile

// A 64 x H tile in flight between global memory and LDS: H/8 threads per
// row, 16 bytes each, H/32 passes of 2048/H rows.
template <int H>
struct TileRegs {
  ushortx8 v[H / 32];
};

// -> LDS row-major [64][H], swizzled.
template <int H>
__device__ __forceinline__ void tile_put_rows(const TileRegs<H>& t,
                                              char* dst) {
  constexpr int TPR = H / 8, RPP = BBLOCK / TPR;
  const int r0 = threadIdx.x / TPR;
  const int h0 = (threadIdx.x % TPR) * 8;
#pragma unroll
  for (int rp = 0; rp < H / 32; ++rp) {
    const int row = r0 + rp * RPP;
    *reinterpret_cast<ushortx8*>(dst + row * (H * 2) + swz(row, h0 * 2)) =
        t.v[rp];
  }
}

// -> LDS transposed [H][64], swizzled per h-row.
template <int H>
__device__ __forceinline__ void tile_put_transposed(const TileRegs<H>& t,
                                                    char* dst) {
  constexpr int TPR = H / 8, RPP = BBLOCK / TPR;
  const int r0 = threadIdx.x / TPR;
  const int h0 = (threadIdx.x % TPR) * 8;
#pragma unroll
  for (int rp = 0; rp < H / 32; ++rp) {
    const int row = r0 + rp * RPP;
#pragma unroll
    for (int j = 0; j < 8; ++j) lds_put(dst, h0 + j, TP, row, t.v[rp][j]);
  }
}

// One wave's [16][64] fp32 strip in C layout (row g*4+r, col nf*16+cl) into
// its LDS strip as bf16 MFMA A operands.
__device__ __forceinline__ void strip_to_lds(const float (&s)[NF][4],
                                             float mul, char* pw) {
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cl = lane & 15;
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      lds_put(pw, g * 4 + r, TP, nf * 16 + cl,
              float_to_bf16_bits(s[nf][r] * mul));
  }
}

}  // namespace
