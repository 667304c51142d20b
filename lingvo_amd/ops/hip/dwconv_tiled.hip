// LDS-tiled depthwise 1-D time convolution for gfx950, with the GLU and the
// padding mask of the Conformer LConv front optionally folded in.
//
// A workgroup owns one tile: utterance b, TT consecutive time rows and CB
// channels. It stages the TT + KT - 1 input rows once into LDS with
// 16-byte loads (rows outside [0, T) and channels >= D are staged as
// zeros, so the tap loop has no bounds test), then each thread slides a
// window over R consecutive outputs of one channel pair with its KT taps
// held as fp32 pairs in registers. Taps j >= K are zero, so any K <= KT
// runs the same code. Results go back through LDS as fp32 so the epilogue
// stores 16 bytes per lane.
//
// Modes:
//   kPlainFwd  y  = conv(x, w) + bias
//   kPlainDx   dx = conv(dy, flip(w)) with pad' = K - 1 - pad
//   kGluFwd    y  = conv(mask * bf16(a * sigmoid(g)), w) + bias, h = [a|g]
//   kGluDx     du = conv(dy, flip(w)); dh = mask * GLU'(h) * du, plus the
//              fp32 column sums of the stored dh as per-tile partials.
// dwconv_tiled_dw_kernel is the weight gradient on the same tile, from u or
// from h (GLU recomputed while staging).

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <algorithm>

#include "common.h"
#include "dwconv_tiled.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float floatx2;

enum { kPlainFwd = 0, kPlainDx = 1, kGluFwd = 2, kGluDx = 3 };

template <int KT_, int R_, int CB_, int NT_>
struct TileCfg {
  static constexpr int KT = KT_;    // taps held per thread (zero-padded)
  static constexpr int R = R_;      // consecutive outputs per thread
  static constexpr int CB = CB_;    // channels per tile
  static constexpr int NT = NT_;    // threads
  static constexpr int NP = CB / 2;       // channel pairs
  static constexpr int NRG = NT / NP;     // row groups
  static constexpr int TT = R * NRG;      // time rows per tile
  static constexpr int OCT = CB / 8;      // 16-byte vectors per row
  static constexpr int NRL = NT / OCT;    // row lanes of the epilogue
  static constexpr int IN_ROWS = TT + KT - 1;
  static constexpr int IN_BYTES = IN_ROWS * CB * 2;
  static constexpr int OUT_BYTES = TT * CB * 4;
  static constexpr int RED_BYTES = NRL * 2 * CB * 4;
  static constexpr int LDS_BYTES =
      IN_BYTES > OUT_BYTES ? (IN_BYTES > RED_BYTES ? IN_BYTES : RED_BYTES)
                           : (OUT_BYTES > RED_BYTES ? OUT_BYTES : RED_BYTES);
  // dwconv_tiled_dw_kernel: input tile + dy tile + fp32 combine buffer.
  static constexpr int DW_LDS_BYTES =
      IN_BYTES + TT * CB * 2 + (KT + 1) * CB * 4;
  static_assert(NT % NP == 0 && NT % OCT == 0 && CB % 8 == 0, "tile shape");
  static_assert(LDS_BYTES <= 64 * 1024 && DW_LDS_BYTES <= 64 * 1024,
                "static LDS limit");
};

__device__ __forceinline__ float sigmoidf_(float g) {
  return 1.f / (1.f + expf(-g));
}

// bf16(1 - p) for a bf16 padding value p, as a float (what ApplyPadding
// multiplies by).
__device__ __forceinline__ float keep_of(unsigned short p) {
  return bf16_bits_to_float(float_to_bf16_bits(1.f - bf16_bits_to_float(p)));
}

// Stages ROWS x CB of `in` (row stride in_stride) starting at time t_first
// of utterance b into in_s. Addresses are clamped into the tensor, so
// every load is unconditional and the zeroing of rows outside [0, T) and
// of channels >= D is a select. GLU: `in` is h = [a|g] and the staged value
// is mask * bf16(a * sigmoid(g)).
template <bool GLU, int ROWS, class C>
__device__ __forceinline__ void stage_rows(
    const unsigned short* __restrict__ in, long in_stride,
    const unsigned short* __restrict__ padm, unsigned short* in_s, long b,
    int T, int D, int t_first, int d0, int tid) {
  constexpr int CB = C::CB, NT = C::NT;
  constexpr int kStage = (ROWS * C::OCT + NT - 1) / NT;
#pragma unroll
  for (int it = 0; it < kStage; ++it) {
    const int idx = tid + it * NT;
    const int row = idx / C::OCT;
    const int o = idx % C::OCT;
    const int t = t_first + row;
    const int gd = d0 + o * 8;
    const bool ok = t >= 0 && t < T && gd < D;
    const long grow = b * T + (ok ? t : 0);
    const int gdc = ok ? gd : 0;
    ushortx8 v = *reinterpret_cast<const ushortx8*>(in + grow * in_stride + gdc);
    if (GLU) {
      const ushortx8 gv = *reinterpret_cast<const ushortx8*>(
          in + grow * in_stride + D + gdc);
      const float keep = padm ? keep_of(padm[grow]) : 1.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const unsigned short u = float_to_bf16_bits(
            bf16_bits_to_float(v[e]) * sigmoidf_(bf16_bits_to_float(gv[e])));
        v[e] = padm ? float_to_bf16_bits(bf16_bits_to_float(u) * keep) : u;
      }
    }
    if (!ok) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = 0;
    }
    if (idx < ROWS * C::OCT)
      *reinterpret_cast<ushortx8*>(in_s + row * CB + o * 8) = v;
  }
}

template <int MODE, class C>
__global__ __launch_bounds__(C::NT) void dwconv_tiled_kernel(
    const unsigned short* __restrict__ in,    // x | dy | h | dy
    const unsigned short* __restrict__ h,     // kGluDx only
    const unsigned short* __restrict__ padm,  // [B, T] bf16 or null
    const unsigned short* __restrict__ w,     // [K, D]
    const unsigned short* __restrict__ bias,  // [D] or null (fwd modes)
    unsigned short* __restrict__ out,         // y | dx | y | dh
    float* __restrict__ cs_part,              // [B * ntt, 2D] (kGluDx)
    int T, int D, int K, int pad, int ntt, int ndb) {
  constexpr int KT = C::KT, R = C::R, CB = C::CB, NT = C::NT;
  constexpr bool kFlip = MODE == kPlainDx || MODE == kGluDx;
  __shared__ __attribute__((aligned(16))) unsigned char lds[C::LDS_BYTES];
  unsigned short* in_s = reinterpret_cast<unsigned short*>(lds);
  float* out_s = reinterpret_cast<float*>(lds);

  const int tid = threadIdx.x;
  const int db = blockIdx.x % ndb;
  const int tile = blockIdx.x / ndb;  // b * ntt + tt
  const int tt = tile % ntt;
  const long b = tile / ntt;
  const int t0 = tt * C::TT;
  const int d0 = db * CB;
  const int epad = kFlip ? K - 1 - pad : pad;
  const long in_stride = MODE == kGluFwd ? 2L * D : D;

  // Taps of this thread's channel pair, fp32, zero beyond K and D.
  const int p = tid % C::NP;
  const int rg = tid / C::NP;
  const int dp = d0 + 2 * p;
  floatx2 wt[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) {
    const int jj = kFlip ? K - 1 - j : j;
    const bool ok = j < K && dp < D;
    const unsigned int v = *reinterpret_cast<const unsigned int*>(
        w + (ok ? (long)jj * D + dp : 0L));
    wt[j][0] = ok ? __uint_as_float(v << 16) : 0.f;
    wt[j][1] = ok ? __uint_as_float(v & 0xffff0000u) : 0.f;
  }

  stage_rows<MODE == kGluFwd, C::IN_ROWS, C>(in, in_stride, padm, in_s, b, T,
                                             D, t0 - epad, d0, tid);
  __syncthreads();

  // Sliding window: input row i feeds output r through tap i - r.
  floatx2 acc[R];
  {
    floatx2 b2 = {0.f, 0.f};
    if (!kFlip && bias && dp < D) {
      const unsigned int v = *reinterpret_cast<const unsigned int*>(bias + dp);
      b2[0] = __uint_as_float(v << 16);
      b2[1] = __uint_as_float(v & 0xffff0000u);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = b2;
  }
  const unsigned short* base = in_s + (rg * R) * CB + 2 * p;
#pragma unroll
  for (int i = 0; i < R + KT - 1; ++i) {
    const unsigned int v = *reinterpret_cast<const unsigned int*>(base + i * CB);
    floatx2 xv;
    xv[0] = __uint_as_float(v << 16);
    xv[1] = __uint_as_float(v & 0xffff0000u);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = i - r;
      if (j >= 0 && j < KT) acc[r] += xv * wt[j];
    }
  }
  __syncthreads();  // every window read is done; the tile is reused
#pragma unroll
  for (int r = 0; r < R; ++r)
    *reinterpret_cast<floatx2*>(out_s + (rg * R + r) * CB + 2 * p) = acc[r];
  __syncthreads();

  // Epilogue: thread = (row lane, channel octet), 16-byte stores.
  const int o = tid % C::OCT;
  const int rl = tid / C::OCT;
  const int gd = d0 + o * 8;
  float csa[8], csg[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) csa[e] = csg[e] = 0.f;
  for (int row = rl; row < C::TT; row += C::NRL) {
    const int t = t0 + row;
    if (t >= T || gd >= D) break;
    const floatx4 lo = *reinterpret_cast<const floatx4*>(out_s + row * CB + o * 8);
    const floatx4 hi =
        *reinterpret_cast<const floatx4*>(out_s + row * CB + o * 8 + 4);
    const float r8[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    const long grow = b * T + t;
    if (MODE != kGluDx) {
      ushortx8 ov;
#pragma unroll
      for (int e = 0; e < 8; ++e) ov[e] = float_to_bf16_bits(r8[e]);
      *reinterpret_cast<ushortx8*>(out + grow * D + gd) = ov;
    } else {
      const ushortx8 av =
          *reinterpret_cast<const ushortx8*>(h + grow * 2L * D + gd);
      const ushortx8 gv =
          *reinterpret_cast<const ushortx8*>(h + grow * 2L * D + D + gd);
      const float keep = padm ? keep_of(padm[grow]) : 1.f;
      ushortx8 oa, og;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float s = sigmoidf_(bf16_bits_to_float(gv[e]));
        const float du = keep == 0.f ? 0.f : r8[e] * keep;
        oa[e] = float_to_bf16_bits(du * s);
        og[e] = float_to_bf16_bits(du * bf16_bits_to_float(av[e]) * s *
                                   (1.f - s));
        csa[e] += bf16_bits_to_float(oa[e]);
        csg[e] += bf16_bits_to_float(og[e]);
      }
      *reinterpret_cast<ushortx8*>(out + grow * 2L * D + gd) = oa;
      *reinterpret_cast<ushortx8*>(out + grow * 2L * D + D + gd) = og;
    }
  }
  if (MODE == kGluDx) {
    // Column sums of this tile: row lanes summed in fixed order.
    __syncthreads();
    float* red = reinterpret_cast<float*>(lds);  // [NRL][2][CB]
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      red[(rl * 2 + 0) * CB + o * 8 + e] = csa[e];
      red[(rl * 2 + 1) * CB + o * 8 + e] = csg[e];
    }
    __syncthreads();
    for (int c = tid; c < 2 * CB; c += NT) {
      const int half = c / CB, cc = c % CB;
      if (d0 + cc < D) {
        float s = 0.f;
        for (int q = 0; q < C::NRL; ++q) s += red[(q * 2 + half) * CB + cc];
        cs_part[(long)tile * 2 * D + (long)half * D + d0 + cc] = s;
      }
    }
  }
}

// Weight gradient: dw[j,d] = sum_{b,t} dy[b,t,d] u[b,t+j-pad,d], db = sum dy.
// Same tile and the same sliding window with the roles swapped: the R dy
// values of a thread's rows sit in registers, the taps are the
// accumulators. A workgroup walks tiles grp, grp + ngroups, ... of its
// channel block with the accumulators in registers, combines its row
// groups through LDS one at a time (fixed order) and stores one
// [K, CB] slice of dw_part [ngroups, K, D] (and db_part [ngroups, D]);
// dwconv_bwd_dw_reduce sums the groups in order. No atomics.
template <bool GLU, class C>
__global__ __launch_bounds__(C::NT) void dwconv_tiled_dw_kernel(
    const unsigned short* __restrict__ dy,
    const unsigned short* __restrict__ x,     // u [B,T,D], or h if GLU
    const unsigned short* __restrict__ padm,  // [B, T] bf16 or null (GLU)
    float* __restrict__ dw_part, float* __restrict__ db_part, int T, int D,
    int K, int pad, int ntt, int ndb, int ntiles, int ngroups) {
  constexpr int KT = C::KT, R = C::R, CB = C::CB, NT = C::NT;
  __shared__ __attribute__((aligned(16))) unsigned short in_s[C::IN_ROWS * CB];
  __shared__ __attribute__((aligned(16))) unsigned short dy_s[C::TT * CB];
  __shared__ float red[(KT + 1) * CB];
  const int tid = threadIdx.x;
  const int db = blockIdx.x % ndb;
  const int grp = blockIdx.x / ndb;
  const int d0 = db * CB;
  const int p = tid % C::NP;
  const int rg = tid / C::NP;
  const long in_stride = GLU ? 2L * D : D;

  floatx2 acc[KT];
#pragma unroll
  for (int j = 0; j < KT; ++j) acc[j] = floatx2{0.f, 0.f};
  floatx2 dbacc = {0.f, 0.f};

  for (int tile = grp; tile < ntiles; tile += ngroups) {
    const int tt = tile % ntt;
    const long b = tile / ntt;
    const int t0 = tt * C::TT;
    stage_rows<GLU, C::IN_ROWS, C>(x, in_stride, padm, in_s, b, T, D,
                                   t0 - pad, d0, tid);
    stage_rows<false, C::TT, C>(dy, D, nullptr, dy_s, b, T, D, t0, d0, tid);
    __syncthreads();
    floatx2 g[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const unsigned int v = *reinterpret_cast<const unsigned int*>(
          dy_s + (rg * R + r) * CB + 2 * p);
      g[r][0] = __uint_as_float(v << 16);
      g[r][1] = __uint_as_float(v & 0xffff0000u);
      dbacc += g[r];
    }
    const unsigned short* base = in_s + (rg * R) * CB + 2 * p;
#pragma unroll
    for (int i = 0; i < R + KT - 1; ++i) {
      const unsigned int v =
          *reinterpret_cast<const unsigned int*>(base + i * CB);
      floatx2 xv;
      xv[0] = __uint_as_float(v << 16);
      xv[1] = __uint_as_float(v & 0xffff0000u);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int j = i - r;
        if (j >= 0 && j < KT) acc[j] += g[r] * xv;
      }
    }
    __syncthreads();  // the tiles are restaged
  }

  for (int q = 0; q < C::NRG; ++q) {
    if (rg == q) {
#pragma unroll
      for (int j = 0; j < KT; ++j) {
        floatx2* dst = reinterpret_cast<floatx2*>(red + j * CB + 2 * p);
        *dst = q == 0 ? acc[j] : *dst + acc[j];
      }
      floatx2* dst = reinterpret_cast<floatx2*>(red + KT * CB + 2 * p);
      *dst = q == 0 ? dbacc : *dst + dbacc;
    }
    __syncthreads();
  }
  for (int i = tid; i < K * CB; i += NT) {
    const int j = i / CB, c = i % CB;
    if (d0 + c < D)
      dw_part[((long)grp * K + j) * D + d0 + c] = red[j * CB + c];
  }
  for (int c = tid; c < CB; c += NT) {
    if (d0 + c < D) db_part[(long)grp * D + d0 + c] = red[KT * CB + c];
  }
}

// The tile: fastest of the shapes measured at B=512, T=300, D=512, K=32
// (table in docs/KERNEL_NOTES.md). The K16/K8 forms hold fewer taps.
using Cfg0 = TileCfg<32, 20, 64, 256>;  // TT = 160
using Cfg0K16 = TileCfg<16, 20, 64, 256>;
using Cfg0K8 = TileCfg<8, 20, 64, 256>;

int lds_limit() {
  static const int limit = []() {
    int dev = 0, v = 0;
    LV_CHECK_HIP(hipGetDevice(&dev));
    LV_CHECK_HIP(hipDeviceGetAttribute(
        &v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    return v;
  }();
  return limit;
}

template <int MODE, class C>
void launch(const unsigned short* in, const unsigned short* h,
            const unsigned short* padm, const unsigned short* w,
            const unsigned short* bias, unsigned short* out, float* cs_part,
            int B, int T, int D, int K, int pad, hipStream_t stream) {
  const int ntt = (T + C::TT - 1) / C::TT;
  const int ndb = (D + C::CB - 1) / C::CB;
  hipLaunchKernelGGL((dwconv_tiled_kernel<MODE, C>),
                     dim3((unsigned)((long)B * ntt * ndb)), dim3(C::NT), 0,
                     stream, in, h, padm, w, bias, out, cs_part, T, D, K, pad,
                     ntt, ndb);
}

template <int MODE>
void dispatch(const unsigned short* in, const unsigned short* h,
              const unsigned short* padm, const unsigned short* w,
              const unsigned short* bias, unsigned short* out, float* cs_part,
              int B, int T, int D, int K, int pad, hipStream_t stream) {
#define LV_GO(C) \
  launch<MODE, C>(in, h, padm, w, bias, out, cs_part, B, T, D, K, pad, stream)
  if (K <= 8) {
    LV_GO(Cfg0K8);
  } else if (K <= 16) {
    LV_GO(Cfg0K16);
  } else {
    LV_GO(Cfg0);
  }
#undef LV_GO
}

}  // namespace

int64_t dwconv_tile_len() { return Cfg0::TT; }

int64_t dwconv_tiled_groups(int64_t B, int64_t T) {
  const int tt = Cfg0::TT;
  return B * ((T + tt - 1) / tt);
}

bool dwconv_tiled_supported(int64_t B, int64_t T, int64_t D, int64_t K) {
  if (B < 1 || T < 1 || D < 8 || D % 8 != 0 || K < 1 || K > 32) return false;
  // One workgroup per tile in a 1-D grid.
  const long tiles = B * ((T + Cfg0::TT - 1) / Cfg0::TT) *
                     ((D + Cfg0::CB - 1) / Cfg0::CB);
  if (tiles >= (1L << 31)) return false;
  // The largest static LDS request of the set (the K=32 forms), the
  // weight-gradient kernel included.
  return Cfg0::LDS_BYTES <= lds_limit() && Cfg0::DW_LDS_BYTES <= lds_limit();
}

int64_t dwconv_tiled_dw_groups(int64_t B, int64_t T, int64_t D) {
  const long ntiles = B * ((T + Cfg0::TT - 1) / Cfg0::TT);
  const long ndb = (D + Cfg0::CB - 1) / Cfg0::CB;
  // ~1536 workgroups: two rounds of the three that fit a CU's LDS.
  return std::min<long>(ntiles, std::max<long>(1, 1536 / ndb));
}

void dwconv_tiled_dw(bool glu, const unsigned short* dy,
                     const unsigned short* x, const unsigned short* padm,
                     float* dw_part, float* db_part, int B, int T, int D,
                     int K, int pad, int ngroups, hipStream_t stream) {
  const int ntt = (T + Cfg0::TT - 1) / Cfg0::TT;
  const int ndb = (D + Cfg0::CB - 1) / Cfg0::CB;
#define LV_DW(GLU, C)                                                        \
  hipLaunchKernelGGL((dwconv_tiled_dw_kernel<GLU, C>),                       \
                     dim3((unsigned)((long)ngroups * ndb)), dim3(C::NT), 0,  \
                     stream, dy, x, padm, dw_part, db_part, T, D, K, pad,    \
                     ntt, ndb, B * ntt, ngroups)
  if (K <= 8) {
    if (glu) LV_DW(true, Cfg0K8); else LV_DW(false, Cfg0K8);
  } else if (K <= 16) {
    if (glu) LV_DW(true, Cfg0K16); else LV_DW(false, Cfg0K16);
  } else {
    if (glu) LV_DW(true, Cfg0); else LV_DW(false, Cfg0);
  }
#undef LV_DW
}

void dwconv_tiled_fwd(const unsigned short* x, const unsigned short* w,
                      const unsigned short* bias, unsigned short* y, int B,
                      int T, int D, int K, int pad,
                      hipStream_t stream) {
  dispatch<kPlainFwd>(x, nullptr, nullptr, w, bias, y, nullptr, B, T, D,
                      K, pad, stream);
}

void dwconv_tiled_dx(const unsigned short* dy, const unsigned short* w,
                     unsigned short* dx, int B, int T, int D, int K, int pad,
                     hipStream_t stream) {
  dispatch<kPlainDx>(dy, nullptr, nullptr, w, nullptr, dx, nullptr, B, T,
                     D, K, pad, stream);
}

void glu_dwconv_tiled_fwd(const unsigned short* h, const unsigned short* padm,
                          const unsigned short* w, const unsigned short* bias,
                          unsigned short* y, int B, int T, int D, int K,
                          int pad, hipStream_t stream) {
  dispatch<kGluFwd>(h, nullptr, padm, w, bias, y, nullptr, B, T, D, K,
                    pad, stream);
}

void glu_dwconv_tiled_dx(const unsigned short* dy, const unsigned short* h,
                         const unsigned short* padm, const unsigned short* w,
                         unsigned short* dh, float* cs_part, int B, int T,
                         int D, int K, int pad, hipStream_t stream) {
  dispatch<kGluDx>(dy, h, padm, w, nullptr, dh, cs_part, B, T, D, K, pad,
                   stream);
}
