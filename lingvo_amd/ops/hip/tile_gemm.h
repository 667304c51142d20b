// What the latency-bound small-M MFMA kernels share (lstm_scan.hip,
// las_step.hip, smallm_gemm in las_decoder.hip): the K loop and the
// skeleton of a step kernel around it.
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
//
// Around it a step kernel (block 256 = 4 waves, a 16*MT x 16 state tile)
// loads its pointwise operands as raw bits BEFORE the GEMM, parks the
// accumulators in a [4][16*MT][16] LDS tile and, after one barrier, runs the
// pointwise part on all 256 threads.
#pragma once

#include <c10/util/Exception.h>

#include <cstdint>
#include <type_traits>

#include "common.h"
#include "mfma.h"

// MFMA view: wave wid, k-group g, row / column cl of the fragment. Pointwise
// view: element e is tile row e*16 + lr, column lc. lr stays unsigned like
// threadIdx.x: the prologue clamps min(m0 + e*16 + lr, b - 1) compile as
// they always have (docs/KERNEL_NOTES.md).
struct StepThread {
  int wid, g, cl;
  unsigned lr;
  int lc;
};

__device__ __forceinline__ StepThread step_thread() {
  const int lane = threadIdx.x & 63;
  return {(int)(threadIdx.x / WAVE_SIZE), lane >> 4, lane & 15,
          threadIdx.x >> 4, (int)(threadIdx.x & 15)};
}

// A wave's accumulators into its plane of the LDS tile (C layout: row
// mt*16 + g*4 + r, column cl).
template <int MT>
__device__ __forceinline__ void park_acc(float (&plane)[16 * MT][16], int g,
                                         int cl, const f32x4 (&acc)[MT]) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) plane[mt * 16 + g * 4 + r][cl] = acc[mt][r];
  }
}

// Sum of the four waves' K-split partials of one tile element.
template <int ROWS>
__device__ __forceinline__ float sum_partials(
    const float (&tile)[4][ROWS][16], int lrow, int lc) {
  return tile[0][lrow][lc] + tile[1][lrow][lc] + tile[2][lrow][lc] +
         tile[3][lrow][lc];
}

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

// ---- host side ------------------------------------------------------------

// Rows per workgroup of a step kernel, as MT = rows / 16. rows == 0 picks
// the default: 32 rows were the fastest for every stage measured
// (docs/KERNEL_NOTES.md). The scan also compiles MT = 1 (min_mt = 1), the
// decoder stages start at MT = 2.
inline int step_mt(int64_t rows, int min_mt) {
  if (rows == 0) rows = 32;
  TORCH_CHECK((rows == 16 && min_mt == 1) || rows == 32 || rows == 64 ||
                  rows == 128,
              "rows_per_block must be 0, ", min_mt == 1 ? "16, " : "",
              "32, 64 or 128");
  return (int)rows / 16;
}

// Calls f(std::integral_constant<int, MT>) for the runtime mt of step_mt.
template <int MIN_MT, typename F>
void dispatch_mt(int mt, F&& f) {
  if constexpr (MIN_MT == 1) {
    if (mt == 1) return f(std::integral_constant<int, 1>{});
  }
  switch (mt) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}
