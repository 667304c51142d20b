// What the MFMA attention kernels (flash_attn.hip, xl_attn.hip) share, on top
// of mfma.h: access to swizzled LDS tiles, the masked-logit constant and the
// delta kernel of the backward passes.
//
// Nothing here knows which kernel calls it. A translation unit that builds
// its device code under a target attribute includes this file inside that
// region, so the helpers it instantiates carry the attribute too.
//
// The staging loops, the strip MFMA loops and the online softmax stay
// spelled out in their kernels: moved into shared helpers they computed the
// same bits, but register allocation and scheduling moved with them and
// several kernels measured slower (docs/KERNEL_NOTES.md).
#pragma once

#include "mfma.h"

// Internal linkage: the kernel template below gets its own host stub in each
// translation unit that launches it.
namespace {

constexpr float NEG_INF = -1e30f;

// ---------------------------------------------------------------------------
// LDS tiles. Row-major tiles are stored with a per-row XOR swizzle on 16B
// granules (mfma.h swz) so B-fragment ds_read_b128 at row-stride >= 128B
// doesn't bank-conflict (guide §6 G4).
// ---------------------------------------------------------------------------

// ds_read a fragment (8 bf16) from a swizzled row-major LDS tile.
__device__ __forceinline__ bf16x8 lds_frag(const char* tile, int row,
                                           int rowb, int byte_in_row) {
  union {
    ushortx8 u;
    bf16x8 h;
  } cv;
  cv.u = *reinterpret_cast<const ushortx8*>(tile + row * rowb +
                                            swz(row, byte_in_row));
  return cv.h;
}

__device__ __forceinline__ void lds_put(char* tile, int row, int rowb,
                                        int col, unsigned short bits) {
  *reinterpret_cast<unsigned short*>(tile + row * rowb + swz(row, col * 2)) =
      bits;
}

// ---------------------------------------------------------------------------
// delta[b,n,t] = sum_h dO * O of the backward passes, dO and O [B,T,N,H].
// ---------------------------------------------------------------------------
constexpr int DELTA_BLOCK = 256;

template <int H>
__global__ __launch_bounds__(DELTA_BLOCK) void attn_delta_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ o, float* __restrict__ delta, int B,
    int T, int N) {
  // H/8 neighbouring lanes per (b, t, n) row, one 16-byte load of dO and
  // of O each; rows enumerate [B,T,N,H] in memory order.
  constexpr int LPR = H / 8;                 // lanes per row
  constexpr int RPB = DELTA_BLOCK / LPR;     // rows per block
  const long nrows = (long)B * T * N;
  const long row = (long)blockIdx.x * RPB + threadIdx.x / LPR;
  const int c = threadIdx.x % LPR;
  // Clamped row: whole waves stay in the shuffles below.
  const long lrow = row < nrows ? row : nrows - 1;
  const ushortx8 dv8 =
      *reinterpret_cast<const ushortx8*>(dout + lrow * H + c * 8);
  const ushortx8 ov8 = *reinterpret_cast<const ushortx8*>(o + lrow * H + c * 8);
  float sum = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    sum += bf16_bits_to_float(dv8[j]) * bf16_bits_to_float(ov8[j]);
#pragma unroll
  for (int off = 1; off < LPR; off <<= 1) sum += __shfl_xor(sum, off);
  if (c == 0 && row < nrows) {
    long b = row / ((long)T * N);
    long tn = row % ((long)T * N);
    long t = tn / N, n = tn % N;
    delta[(b * N + n) * T + t] = sum;
  }
}

}  // namespace
