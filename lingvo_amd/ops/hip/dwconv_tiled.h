// Host entry points of the LDS-tiled depthwise convolution kernels
// (dwconv_tiled.hip).
// Pointers are device bf16 bit patterns; shapes are validated by callers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

// Time rows per tile of the default configuration.
int64_t dwconv_tile_len();
// Rows of the [groups, 2D] column-sum partials glu_dwconv_tiled_dx writes.
int64_t dwconv_tiled_groups(int64_t B, int64_t T);
// True if the tiled kernels can run the shape on this device (LDS request
// of every kernel, the weight gradient included, within the per-block
// limit; grid within range).
bool dwconv_tiled_supported(int64_t B, int64_t T, int64_t D, int64_t K);

// Partial groups of the tiled weight gradient for this shape.
int64_t dwconv_tiled_dw_groups(int64_t B, int64_t T, int64_t D);
// dw_part [ngroups, K, D] and db_part [ngroups, D] fp32, every entry
// written; x is the conv input u, or h [B,T,2D] (+ padm) with glu.
void dwconv_tiled_dw(bool glu, const unsigned short* dy,
                     const unsigned short* x, const unsigned short* padm,
                     float* dw_part, float* db_part, int B, int T, int D,
                     int K, int pad, int ngroups, hipStream_t stream);
void dwconv_tiled_fwd(const unsigned short* x, const unsigned short* w,
                      const unsigned short* bias, unsigned short* y, int B,
                      int T, int D, int K, int pad,
                      hipStream_t stream);
void dwconv_tiled_dx(const unsigned short* dy, const unsigned short* w,
                     unsigned short* dx, int B, int T, int D, int K, int pad,
                     hipStream_t stream);
void glu_dwconv_tiled_fwd(const unsigned short* h, const unsigned short* padm,
                          const unsigned short* w, const unsigned short* bias,
                          unsigned short* y, int B, int T, int D, int K,
                          int pad, hipStream_t stream);
void glu_dwconv_tiled_dx(const unsigned short* dy, const unsigned short* h,
                         const unsigned short* padm, const unsigned short* w,
                         unsigned short* dh, float* cs_part, int B, int T,
                         int D, int K, int pad, hipStream_t stream);
