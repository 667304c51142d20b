// K loop shared by the latency-bound small-M MFMA kernels (lstm_scan.hip,
// las_decoder.hip, las_step.hip).
//
// A wave accumulates MT 16x16 output tiles over a K range. The caller
// splits every fragment address into a per-lane BASE pointer (the lane's
// row, with whatever row stride the operand has, plus its k-group offset
// g*8) and the running k offset the loop adds, so contiguous rows, rows of
// a strided view and a second A source all go through the same loop.
//
// A step kernel is latency-bound (the next launch depends on it), so the
// loop is written for loads in flight, not for occupancy: it has no
// per-row branches (callers clamp rows beyond M to row M-1: output row r
// of an MFMA depends on A row r alone, and those rows are never stored)
// and KU k-steps of fragments are loaded ahead of their MFMAs.
#pragma once

#include "common.h"
#include "mfma.h"

// acc[mt] += A_mt[16, k_len] @ B[16, k_len]^T with per-lane fragment
// pointers (arow[mt] / brow already include the lane's row and k-group
// offset). k_len % 32 == 0; k_len <= 0 does nothing.
template <int MT>
__device__ __forceinline__ void tile_gemm(
    const unsigned short* const (&arow)[MT], const unsigned short* brow,
    int k_len, f32x4 (&acc)[MT]) {
  constexpr int KU = MT == 1 ? 8 : (MT == 2 ? 4 : 2);  // k-steps in flight
  int k0 = 0;
  for (; k0 + 32 * KU <= k_len; k0 += 32 * KU) {
    bf16x8 bf[KU];
    bf16x8 af[KU][MT];
#pragma unroll
    for (int u = 0; u < KU; ++u) {
      bf[u] = load_bf16x8_bits(brow + k0 + u * 32);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        af[u][mt] = load_bf16x8_bits(arow[mt] + k0 + u * 32);
      }
    }
#pragma unroll
    for (int u = 0; u < KU; ++u) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        acc[mt] = mfma16x16x32_bf16(af[u][mt], bf[u], acc[mt]);
      }
    }
  }
  for (; k0 < k_len; k0 += 32) {
    const bf16x8 bf = load_bf16x8_bits(brow + k0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      acc[mt] = mfma16x16x32_bf16(load_bf16x8_bits(arow[mt] + k0), bf,
                                  acc[mt]);
    }
  }
}

// Two-source A against one transposed weight row: K range [0, k1) comes
// from a1row, [k1, k1 + k2) from a2row. Either range may be empty; its
// pointers are then never dereferenced.
template <int MT>
__device__ __forceinline__ void tile_gemm2(
    const unsigned short* const (&a1row)[MT], int k1,
    const unsigned short* const (&a2row)[MT], int k2,
    const unsigned short* brow, f32x4 (&acc)[MT]) {
  tile_gemm<MT>(a1row, brow, k1, acc);
  tile_gemm<MT>(a2row, brow + k1, k2, acc);
}
