// Fused padded-aware GroupNorm fwd+bwd for gfx950
// (reference op: lingvo/core/bn_layers.py:747 GroupNormLayer).
//
// x: [B, T, D] bf16, G groups over the channel dim; moments are per
// (b, g) over (valid T) x (D/G); padded frames are excluded from the
// moments and zeroed in the output. y = xhat * (1+gamma) + beta.
//
// Scalar and vec kernels: one block (256 threads) per (b, g): block-reduce
// moments, then a second pass over global memory normalizes; dgamma/dbeta
// accumulate via fp32 atomics (small: D columns).
//
// Tile kernels (route 'tile', cg % 8 == 0 and 64 % cg == 0): one workgroup
// per (b, 64-channel slab) stages all T rows of the slab into dynamic LDS
// in whole 128-byte lines, reduces per group in a fixed order and produces
// the output from LDS, so x (and dy) are read from memory once. dgamma /
// dbeta go to a [B, 2D] partial buffer with plain stores and colsum_reduce
// sums it: no atomics, no fills, same bits on every run.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <string>

#include "common.h"
#include "host_checks.h"

namespace {

constexpr int GN_BLOCK = 256;
constexpr int GN_WAVES = GN_BLOCK / WAVE_SIZE;

__global__ __launch_bounds__(GN_BLOCK) void gn_fwd_kernel(
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ paddings,  // [B,T] bf16 or null
    unsigned short* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int B, int T, int D, int G, float eps,
    int act) {
  __shared__ float scratch[GN_WAVES];
  const int b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int cg = D / G;
  const int tid = threadIdx.x;

  float sum = 0.f, sumsq = 0.f, count = 0.f;
  for (int i = tid; i < T * cg; i += GN_BLOCK) {
    int t = i / cg;
    int c = g * cg + i % cg;
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    if (pad < 0.5f) {
      float v = bf16_bits_to_float(x[((long)b * T + t) * D + c]);
      sum += v;
      sumsq += v * v;
      count += 1.f;
    }
  }
  sum = block_reduce_sum<GN_WAVES>(sum, scratch);
  sumsq = block_reduce_sum<GN_WAVES>(sumsq, scratch);
  count = block_reduce_sum<GN_WAVES>(count, scratch);
  count = fmaxf(count, 1.f);
  float mu = sum / count;
  float var = sumsq / count - mu * mu;
  float rstd = rsqrtf(var + eps);
  if (tid == 0) {
    mean_out[(long)b * G + g] = mu;
    rstd_out[(long)b * G + g] = rstd;
  }

  for (int i = tid; i < T * cg; i += GN_BLOCK) {
    int t = i / cg;
    int c = g * cg + i % cg;
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    float v = bf16_bits_to_float(x[((long)b * T + t) * D + c]);
    float w = 1.f + bf16_bits_to_float(gamma[c]);
    float bb = bf16_bits_to_float(beta[c]);
    float out = (v - mu) * rstd * w + bb;
    if (act == 1) out = out / (1.f + __expf(-out));  // fused SiLU
    out *= (1.f - pad);
    y[((long)b * T + t) * D + c] = float_to_bf16_bits(out);
  }
}

// Vectorized fwd for cg % 8 == 0, laid out like gn_bwd_vec_kernel: each
// thread owns one 8-channel octet and strides over rows, so all traffic
// is ushortx8, the padding is read once per row and there is no divide
// or modulo per element. Moments stay fp32; they differ from the scalar
// kernel only through summation order.
__global__ __launch_bounds__(GN_BLOCK) void gn_fwd_vec_kernel(
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ paddings,  // [B,T] bf16 or null
    unsigned short* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int B, int T, int D, int G, float eps,
    int act) {
  __shared__ float scratch[GN_WAVES];
  const int b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int cg = D / G;
  const int noct = cg / 8;
  const int tid = threadIdx.x;
  const int oct = tid % noct;
  const int rt = tid / noct;
  const int rstep = GN_BLOCK / noct;
  // Threads past the last whole row lane idle (noct need not divide 256).
  const int t_first = rt < rstep ? rt : T;
  const long col0 = (long)g * cg + (rt < rstep ? oct : 0) * 8;

  float sum = 0.f, sumsq = 0.f, count = 0.f;
  for (int t = t_first; t < T; t += rstep) {
    const float pad =
        paddings ? bf16_bits_to_float(paddings[(long)b * T + t]) : 0.f;
    if (pad >= 0.5f) continue;
    const ushortx8 xv = *reinterpret_cast<const ushortx8*>(
        x + ((long)b * T + t) * D + col0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = bf16_bits_to_float(xv[e]);
      sum += v;
      sumsq += v * v;
    }
    count += 8.f;
  }
  sum = block_reduce_sum<GN_WAVES>(sum, scratch);
  sumsq = block_reduce_sum<GN_WAVES>(sumsq, scratch);
  count = block_reduce_sum<GN_WAVES>(count, scratch);
  count = fmaxf(count, 1.f);
  const float mu = sum / count;
  const float var = sumsq / count - mu * mu;
  const float rstd = rsqrtf(var + eps);
  if (tid == 0) {
    mean_out[(long)b * G + g] = mu;
    rstd_out[(long)b * G + g] = rstd;
  }

  float w[8], bb[8];
  {
    const ushortx8 gv = *reinterpret_cast<const ushortx8*>(gamma + col0);
    const ushortx8 bv = *reinterpret_cast<const ushortx8*>(beta + col0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      w[e] = 1.f + bf16_bits_to_float(gv[e]);
      bb[e] = bf16_bits_to_float(bv[e]);
    }
  }
  for (int t = t_first; t < T; t += rstep) {
    const float pad =
        paddings ? bf16_bits_to_float(paddings[(long)b * T + t]) : 0.f;
    const long base = ((long)b * T + t) * D + col0;
    const ushortx8 xv = *reinterpret_cast<const ushortx8*>(x + base);
    ushortx8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float out = (bf16_bits_to_float(xv[e]) - mu) * rstd * w[e] + bb[e];
      if (act == 1) out = out / (1.f + __expf(-out));  // fused SiLU
      out *= (1.f - pad);
      o[e] = float_to_bf16_bits(out);
    }
    *reinterpret_cast<ushortx8*>(y + base) = o;
  }
}

__global__ __launch_bounds__(GN_BLOCK) void gn_bwd_kernel(
    const unsigned short* __restrict__ dy,
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ paddings,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    unsigned short* __restrict__ dx, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int B, int T, int D, int G, int act) {
  __shared__ float scratch[GN_WAVES];
  const int b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int cg = D / G;
  const int tid = threadIdx.x;
  const float mu = mean[(long)b * G + g];
  const float rs = rstd[(long)b * G + g];

  // Pass 1: reductions over the group: s1=sum(dyw), s2=sum(dyw*xhat),
  // count; and per-channel dgamma/dbeta partials via LDS.
  __shared__ float dg_s[64];  // cg <= 64 supported
  __shared__ float db_s[64];
  for (int i = tid; i < cg; i += GN_BLOCK) {
    dg_s[i] = 0.f;
    db_s[i] = 0.f;
  }
  __syncthreads();
  float s1 = 0.f, s2 = 0.f, count = 0.f;
  for (int i = tid; i < T * cg; i += GN_BLOCK) {
    int t = i / cg;
    int ci = i % cg;
    int c = g * cg + ci;
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    if (pad < 0.5f) {
      float xv = bf16_bits_to_float(x[((long)b * T + t) * D + c]);
      float dyv = bf16_bits_to_float(dy[((long)b * T + t) * D + c]);
      float w = 1.f + bf16_bits_to_float(gamma[c]);
      float xhat = (xv - mu) * rs;
      float dxhat = dyv * w;
      s1 += dxhat;
      s2 += dxhat * xhat;
      count += 1.f;
      atomicAdd(&dg_s[ci], dyv * xhat);
      atomicAdd(&db_s[ci], dyv);
    }
  }
  s1 = block_reduce_sum<GN_WAVES>(s1, scratch);
  s2 = block_reduce_sum<GN_WAVES>(s2, scratch);
  count = block_reduce_sum<GN_WAVES>(count, scratch);
  count = fmaxf(count, 1.f);
  const float inv_n = 1.f / count;

  for (int i = tid; i < cg; i += GN_BLOCK) {
    int c = g * cg + i;
    if (dg_s[i] != 0.f) atomicAdd(dgamma + c, dg_s[i]);
    if (db_s[i] != 0.f) atomicAdd(dbeta + c, db_s[i]);
  }

  for (int i = tid; i < T * cg; i += GN_BLOCK) {
    int t = i / cg;
    int c = g * cg + i % cg;
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    float xv = bf16_bits_to_float(x[((long)b * T + t) * D + c]);
    float dyv = bf16_bits_to_float(dy[((long)b * T + t) * D + c]);
    float w = 1.f + bf16_bits_to_float(gamma[c]);
    float xhat = (xv - mu) * rs;
    float dxhat = dyv * w;
    float val = rs * (dxhat - inv_n * (s1 + xhat * s2)) * (1.f - pad);
    dx[((long)b * T + t) * D + c] = float_to_bf16_bits(val);
  }
}

// Vectorized bwd for cg % 8 == 0 (the production config: D=512, G=32,
// cg=16). Each thread owns one 8-channel octet and strides over rows:
// all x/dy traffic is ushortx8, and dgamma/dbeta partials accumulate
// in REGISTERS (the scalar kernel above pays two LDS atomics per
// element in its hot loop, which dominates its runtime).
// act == 1: the forward emitted silu(y_pre); incoming dy is w.r.t.
// silu's output, so fold silu'(y_pre) in (y_pre recomputed from the
// saved moments + beta — nothing extra stored).
__global__ __launch_bounds__(GN_BLOCK) void gn_bwd_vec_kernel(
    const unsigned short* __restrict__ dy,
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ paddings,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    unsigned short* __restrict__ dx, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int B, int T, int D, int G, int act) {
  __shared__ float scratch[GN_WAVES];
  __shared__ float dg_s[64];
  __shared__ float db_s[64];
  const int b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int cg = D / G;
  const int noct = cg / 8;
  const int tid = threadIdx.x;
  const int oct = tid % noct;
  const int rt = tid / noct;
  const int rstep = GN_BLOCK / noct;
  const float mu = mean[(long)b * G + g];
  const float rs = rstd[(long)b * G + g];
  const long col0 = (long)g * cg + oct * 8;

  float w[8], bb[8];
  {
    ushortx8 gv = *reinterpret_cast<const ushortx8*>(gamma + col0);
    ushortx8 bv = *reinterpret_cast<const ushortx8*>(beta + col0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      w[e] = 1.f + bf16_bits_to_float(gv[e]);
      bb[e] = bf16_bits_to_float(bv[e]);
    }
  }
  for (int i = tid; i < cg; i += GN_BLOCK) {
    dg_s[i] = 0.f;
    db_s[i] = 0.f;
  }

  float s1 = 0.f, s2 = 0.f, count = 0.f;
  float dg8[8], db8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    dg8[e] = 0.f;
    db8[e] = 0.f;
  }
  for (int t = rt; t < T; t += rstep) {
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    if (pad >= 0.5f) continue;
    const long base = ((long)b * T + t) * D + col0;
    ushortx8 xv = *reinterpret_cast<const ushortx8*>(x + base);
    ushortx8 dyv = *reinterpret_cast<const ushortx8*>(dy + base);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float xf = bf16_bits_to_float(xv[e]);
      float df = bf16_bits_to_float(dyv[e]);
      float xhat = (xf - mu) * rs;
      if (act == 1) {
        const float ypre = xhat * w[e] + bb[e];
        const float sg = 1.f / (1.f + __expf(-ypre));
        df *= sg * (1.f + ypre * (1.f - sg));
      }
      float dxhat = df * w[e];
      s1 += dxhat;
      s2 += dxhat * xhat;
      dg8[e] += df * xhat;
      db8[e] += df;
    }
    count += 8.f;
  }
  __syncthreads();  // dg_s/db_s zero-init visible
  s1 = block_reduce_sum<GN_WAVES>(s1, scratch);
  s2 = block_reduce_sum<GN_WAVES>(s2, scratch);
  count = block_reduce_sum<GN_WAVES>(count, scratch);
  count = fmaxf(count, 1.f);
  const float inv_n = 1.f / count;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (dg8[e] != 0.f) atomicAdd(&dg_s[oct * 8 + e], dg8[e]);
    if (db8[e] != 0.f) atomicAdd(&db_s[oct * 8 + e], db8[e]);
  }
  __syncthreads();
  for (int i = tid; i < cg; i += GN_BLOCK) {
    int c = g * cg + i;
    if (dg_s[i] != 0.f) atomicAdd(dgamma + c, dg_s[i]);
    if (db_s[i] != 0.f) atomicAdd(dbeta + c, db_s[i]);
  }

  for (int t = rt; t < T; t += rstep) {
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    const long base = ((long)b * T + t) * D + col0;
    ushortx8 xv = *reinterpret_cast<const ushortx8*>(x + base);
    ushortx8 dyv = *reinterpret_cast<const ushortx8*>(dy + base);
    ushortx8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float xf = bf16_bits_to_float(xv[e]);
      float df = bf16_bits_to_float(dyv[e]);
      float xhat = (xf - mu) * rs;
      if (act == 1) {
        const float ypre = xhat * w[e] + bb[e];
        const float sg = 1.f / (1.f + __expf(-ypre));
        df *= sg * (1.f + ypre * (1.f - sg));
      }
      float dxhat = df * w[e];
      float val = rs * (dxhat - inv_n * (s1 + xhat * s2)) * (1.f - pad);
      o[e] = float_to_bf16_bits(val);
    }
    *reinterpret_cast<ushortx8*>(dx + base) = o;
  }
}

// ---- tile-resident kernels ------------------------------------------------
// The new device code is built without the packed-fp32 VALU forms.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

// Tile geometry. A thread is (row lane rl, octet o): OCT lanes cover one
// row of the slab, a wave instruction covers 64 / OCT whole rows.
template <int CB_, int NT_, int U_>
struct GnTile {
  static constexpr int CB = CB_;         // channels per slab
  static constexpr int NT = NT_;         // threads
  static constexpr int OCT = CB / 8;     // 16-byte vectors per row
  static constexpr int NRL = NT / OCT;   // rows per pass of the workgroup
  static constexpr int NW = NT / WAVE_SIZE;
  static constexpr int U = U_;           // rows a thread has in flight
  // red[NW][OCT][3] group sums, then (backward) redc[NW][2][CB].
  static constexpr int RED_BYTES = NW * OCT * 3 * 4;
  static constexpr int REDC_BYTES = NW * 2 * CB * 4;
  static size_t lds_bytes(long T, bool backward) {
    const size_t pads = ((size_t)T * 2 + 15) / 16 * 16;
    return (size_t)T * CB * 2 * (backward ? 2 : 1) + pads + RED_BYTES +
           (backward ? REDC_BYTES : 0);
  }
};

// Sum over the lanes of a wave that hold the same group: all row lanes
// (xor >= OCT) and the opg octets of the group (xor < opg; groups are
// aligned to opg octets). A fixed butterfly, the same on every run.
template <int OCT>
__device__ __forceinline__ float gn_wave_group_sum(float v, int opg) {
#pragma unroll
  for (int off = 32; off >= OCT; off >>= 1) v += __shfl_xor(v, off, WAVE_SIZE);
#pragma unroll
  for (int off = OCT / 2; off >= 1; off >>= 1)
    if (off < opg) v += __shfl_xor(v, off, WAVE_SIZE);
  return v;
}

// Group totals of three per-thread partials: waves summed in order through
// red [NW][OCT][3]. Ends with every thread holding its group's totals.
template <class C>
__device__ __forceinline__ void gn_group_totals(float& a, float& b, float& c,
                                                int opg, int o, float* red) {
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wid = threadIdx.x / WAVE_SIZE;
  a = gn_wave_group_sum<C::OCT>(a, opg);
  b = gn_wave_group_sum<C::OCT>(b, opg);
  c = gn_wave_group_sum<C::OCT>(c, opg);
  if (lane < C::OCT) {
    red[(wid * C::OCT + o) * 3 + 0] = a;
    red[(wid * C::OCT + o) * 3 + 1] = b;
    red[(wid * C::OCT + o) * 3 + 2] = c;
  }
  __syncthreads();
  a = b = c = 0.f;
#pragma unroll
  for (int w = 0; w < C::NW; ++w) {
    a += red[(w * C::OCT + o) * 3 + 0];
    b += red[(w * C::OCT + o) * 3 + 1];
    c += red[(w * C::OCT + o) * 3 + 2];
  }
}

template <class C>
__global__ __launch_bounds__(C::NT) void gn_fwd_tile_kernel(
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ paddings,  // [B,T] bf16 or null
    unsigned short* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int T, int D, int G, int nslab, float eps,
    int act) {
  constexpr int CB = C::CB, NRL = C::NRL, U = C::U;
  extern __shared__ __attribute__((aligned(16))) unsigned char gn_lds[];
  unsigned short* xs = reinterpret_cast<unsigned short*>(gn_lds);  // [T][CB]
  unsigned short* pad_s = xs + (long)T * CB;                       // [T]
  float* red = reinterpret_cast<float*>(gn_lds + (long)T * CB * 2 +
                                        ((long)T * 2 + 15) / 16 * 16);
  const int tid = threadIdx.x;
  const int o = tid % C::OCT;
  const int rl = tid / C::OCT;
  const long b = blockIdx.x / nslab;
  const int d0 = (blockIdx.x % nslab) * CB;
  const int cg = D / G;
  const int opg = cg / 8;
  const bool col_ok = d0 + o * 8 < D;
  const int gd = col_ok ? d0 + o * 8 : d0;  // clamped into the slab
  const int t_first = col_ok ? rl : T;      // lanes past a narrow slab idle
  const unsigned short* xb = x + b * T * D + gd;
  const unsigned short* pb = paddings ? paddings + b * T : nullptr;

  // The paddings of the utterance first, so that no row load waits on a
  // global read of its padding value.
  for (int t = tid; t < T; t += C::NT) pad_s[t] = pb ? pb[t] : (unsigned short)0;
  __syncthreads();

  float sum = 0.f, sumsq = 0.f, count = 0.f;
  for (int tb = t_first; tb < T; tb += U * NRL) {
    ushortx8 v[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = tb + u * NRL;
      live[u] = t < T && bf16_bits_to_float(pad_s[t < T ? t : T - 1]) < 0.5f;
      if (live[u]) v[u] = *reinterpret_cast<const ushortx8*>(xb + (long)t * D);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!live[u]) continue;
      const int t = tb + u * NRL;
      *reinterpret_cast<ushortx8*>(xs + (long)t * CB + o * 8) = v[u];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float f = bf16_bits_to_float(v[u][e]);
        sum += f;
        sumsq += f * f;
      }
      count += 8.f;
    }
  }
  gn_group_totals<C>(sum, sumsq, count, opg, o, red);
  count = fmaxf(count, 1.f);
  const float mu = sum / count;
  const float var = sumsq / count - mu * mu;
  const float rstd = rsqrtf(var + eps);
  if (rl == 0 && col_ok && o % opg == 0) {
    mean_out[b * G + gd / cg] = mu;
    rstd_out[b * G + gd / cg] = rstd;
  }

  float w[8], bb[8];
  {
    const ushortx8 gv = *reinterpret_cast<const ushortx8*>(gamma + gd);
    const ushortx8 bv = *reinterpret_cast<const ushortx8*>(beta + gd);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      w[e] = 1.f + bf16_bits_to_float(gv[e]);
      bb[e] = bf16_bits_to_float(bv[e]);
    }
  }
  unsigned short* yb = y + b * T * D + gd;
  for (int t = t_first; t < T; t += NRL) {
    const float pad = bf16_bits_to_float(pad_s[t]);
    ushortx8 ov = {0, 0, 0, 0, 0, 0, 0, 0};
    if (pad < 0.5f) {
      const ushortx8 xv =
          *reinterpret_cast<const ushortx8*>(xs + (long)t * CB + o * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float out = (bf16_bits_to_float(xv[e]) - mu) * rstd * w[e] + bb[e];
        if (act == 1) out = out / (1.f + __expf(-out));  // fused SiLU
        out *= (1.f - pad);
        ov[e] = float_to_bf16_bits(out);
      }
    }
    *reinterpret_cast<ushortx8*>(yb + (long)t * D) = ov;
  }
}

// Backward on the same tile: x and dy staged raw, silu'(y_pre) recomputed
// in both passes (as the vec kernel does), so LDS holds 256 B per row. The
// kernel is bound by its VALU work, so the sigmoid takes the hardware
// reciprocal (1 ulp) where the vec kernel divides.
// part: [B, 2D] fp32, dgamma columns then dbeta columns; this workgroup is
// the only writer of its slab's columns of row b.
template <class C>
__global__ __launch_bounds__(C::NT) void gn_bwd_tile_kernel(
    const unsigned short* __restrict__ dy,
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ paddings,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    unsigned short* __restrict__ dx, float* __restrict__ part, int T, int D,
    int G, int nslab, int act) {
  constexpr int CB = C::CB, NRL = C::NRL, U = C::U;
  extern __shared__ __attribute__((aligned(16))) unsigned char gn_lds[];
  unsigned short* xs = reinterpret_cast<unsigned short*>(gn_lds);  // [T][CB]
  unsigned short* dys = xs + (long)T * CB;                         // [T][CB]
  unsigned short* pad_s = dys + (long)T * CB;                      // [T]
  float* red = reinterpret_cast<float*>(gn_lds + (long)T * CB * 4 +
                                        ((long)T * 2 + 15) / 16 * 16);
  float* redc = red + C::NW * C::OCT * 3;                     // [NW][2][CB]
  const int tid = threadIdx.x;
  const int o = tid % C::OCT;
  const int rl = tid / C::OCT;
  const long b = blockIdx.x / nslab;
  const int d0 = (blockIdx.x % nslab) * CB;
  const int cg = D / G;
  const int opg = cg / 8;
  const bool col_ok = d0 + o * 8 < D;
  const int gd = col_ok ? d0 + o * 8 : d0;
  const int t_first = col_ok ? rl : T;
  const unsigned short* xb = x + b * T * D + gd;
  const unsigned short* dyb = dy + b * T * D + gd;
  const unsigned short* pb = paddings ? paddings + b * T : nullptr;
  const float mu = mean[b * G + gd / cg];
  const float rs = rstd[b * G + gd / cg];

  float w[8], bb[8];
  {
    const ushortx8 gv = *reinterpret_cast<const ushortx8*>(gamma + gd);
    const ushortx8 bv = *reinterpret_cast<const ushortx8*>(beta + gd);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      w[e] = 1.f + bf16_bits_to_float(gv[e]);
      bb[e] = bf16_bits_to_float(bv[e]);
    }
  }

  float s1 = 0.f, s2 = 0.f, count = 0.f;
  float dg8[8], db8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    dg8[e] = 0.f;
    db8[e] = 0.f;
  }
  for (int t = tid; t < T; t += C::NT) pad_s[t] = pb ? pb[t] : (unsigned short)0;
  __syncthreads();
  for (int tb = t_first; tb < T; tb += U * NRL) {
    ushortx8 xv[U], dv[U];
    bool live[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = tb + u * NRL;
      live[u] = t < T && bf16_bits_to_float(pad_s[t < T ? t : T - 1]) < 0.5f;
      if (live[u]) {
        xv[u] = *reinterpret_cast<const ushortx8*>(xb + (long)t * D);
        dv[u] = *reinterpret_cast<const ushortx8*>(dyb + (long)t * D);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!live[u]) continue;
      const int t = tb + u * NRL;
      *reinterpret_cast<ushortx8*>(xs + (long)t * CB + o * 8) = xv[u];
      *reinterpret_cast<ushortx8*>(dys + (long)t * CB + o * 8) = dv[u];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xf = bf16_bits_to_float(xv[u][e]);
        float df = bf16_bits_to_float(dv[u][e]);
        const float xhat = (xf - mu) * rs;
        if (act == 1) {
          const float ypre = xhat * w[e] + bb[e];
          const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-ypre));
          df *= sg * (1.f + ypre * (1.f - sg));
        }
        const float dxhat = df * w[e];
        s1 += dxhat;
        s2 += dxhat * xhat;
        dg8[e] += df * xhat;
        db8[e] += df;
      }
      count += 8.f;
    }
  }

  // Per-channel sums: row lanes of a wave by butterfly, waves in order.
  {
    const int lane = tid & (WAVE_SIZE - 1);
    const int wid = tid / WAVE_SIZE;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      dg8[e] = gn_wave_group_sum<C::OCT>(dg8[e], 1);
      db8[e] = gn_wave_group_sum<C::OCT>(db8[e], 1);
    }
    if (lane < C::OCT) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        redc[(wid * 2 + 0) * CB + o * 8 + e] = dg8[e];
        redc[(wid * 2 + 1) * CB + o * 8 + e] = db8[e];
      }
    }
  }
  gn_group_totals<C>(s1, s2, count, opg, o, red);  // syncs: redc visible too
  count = fmaxf(count, 1.f);
  const float inv_n = 1.f / count;
  for (int c = tid; c < 2 * CB; c += C::NT) {
    const int half = c / CB, cc = c % CB;
    if (d0 + cc < D) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < C::NW; ++q) s += redc[(q * 2 + half) * CB + cc];
      part[b * 2 * D + (long)half * D + d0 + cc] = s;
    }
  }

  unsigned short* dxb = dx + b * T * D + gd;
  for (int t = t_first; t < T; t += NRL) {
    const float pad = bf16_bits_to_float(pad_s[t]);
    ushortx8 ov = {0, 0, 0, 0, 0, 0, 0, 0};
    if (pad < 0.5f) {
      const ushortx8 xv =
          *reinterpret_cast<const ushortx8*>(xs + (long)t * CB + o * 8);
      const ushortx8 dv =
          *reinterpret_cast<const ushortx8*>(dys + (long)t * CB + o * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float xf = bf16_bits_to_float(xv[e]);
        float df = bf16_bits_to_float(dv[e]);
        const float xhat = (xf - mu) * rs;
        if (act == 1) {
          const float ypre = xhat * w[e] + bb[e];
          const float sg = __builtin_amdgcn_rcpf(1.f + __expf(-ypre));
          df *= sg * (1.f + ypre * (1.f - sg));
        }
        const float dxhat = df * w[e];
        const float val =
            rs * (dxhat - inv_n * (s1 + xhat * s2)) * (1.f - pad);
        ov[e] = float_to_bf16_bits(val);
      }
    }
    *reinterpret_cast<ushortx8*>(dxb + (long)t * D) = ov;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// The tiles: fastest of the shapes measured at B=512, T=300, D=512, G=32
// (table in docs/KERNEL_NOTES.md). The backward's 77 KB tile leaves room
// for two workgroups of 256 threads per CU; 512 threads need a larger
// reduce buffer and fit once.
constexpr int GN_TILE_CB = 64;
using GnFwdTile = GnTile<GN_TILE_CB, 512, 2>;
using GnBwdTile = GnTile<GN_TILE_CB, 256, 4>;

size_t gn_tile_lds_bytes(long T, bool backward) {
  return backward ? GnBwdTile::lds_bytes(T, true)
                  : GnFwdTile::lds_bytes(T, false);
}

size_t gn_lds_limit() {
  static const int limit = []() {
    int dev = 0, v = 0;
    LV_CHECK_HIP(hipGetDevice(&dev));
    LV_CHECK_HIP(hipDeviceGetAttribute(
        &v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    return v;
  }();
  return (size_t)limit;
}

bool gn_tile_width_ok(int D, int G) {
  const int cg = D / G;
  return cg % 8 == 0 && GN_TILE_CB % cg == 0;
}

// Everything the tile route requires, checked before anything is allocated.
// Returns the dynamic LDS request.
size_t gn_tile_check(const torch::Tensor& x, const torch::Tensor& gamma,
                     const torch::Tensor& beta,
                     const c10::optional<torch::Tensor>& pad, int G,
                     bool backward) {
  check_contig(x, torch::kBFloat16, "group_norm: x");
  check_contig(gamma, torch::kBFloat16, "group_norm: gamma");
  check_contig(beta, torch::kBFloat16, "group_norm: beta");
  TORCH_CHECK(x.dim() == 3 && x.numel() > 0 && aligned16(x),
              "group_norm: x must be a non-empty 16-byte aligned [B,T,D]");
  const long B = x.size(0), T = x.size(1), D = x.size(2);
  TORCH_CHECK(G >= 1 && D % G == 0 && gn_tile_width_ok((int)D, G),
              "group_norm: route='tile' needs cg % 8 == 0 and 64 % cg == 0");
  TORCH_CHECK(gamma.numel() == D && beta.numel() == D && aligned16(gamma) &&
                  aligned16(beta),
              "group_norm: gamma and beta must be 16-byte aligned [D]");
  if (pad.has_value()) {
    check_contig(*pad, torch::kBFloat16, "group_norm: paddings");
    TORCH_CHECK(pad->numel() == B * T, "group_norm: paddings must be [B,T]");
  }
  const long nslab = (D + GN_TILE_CB - 1) / GN_TILE_CB;
  TORCH_CHECK(B * nslab < (1L << 31) && T < (1L << 24),
              "group_norm: grid too large for route='tile'");
  const size_t lds = gn_tile_lds_bytes(T, backward);
  TORCH_CHECK(lds <= gn_lds_limit(), "group_norm: route='tile' needs ", lds,
              " bytes of LDS per workgroup for T=", T, ", the device allows ",
              gn_lds_limit());
  return lds;
}

}  // namespace

int64_t group_norm_tile_max_rows(bool backward) {
  const size_t limit = gn_lds_limit();
  long t = (long)(limit / (GN_TILE_CB * 2 * (backward ? 2 : 1)));
  while (t > 0 && gn_tile_lds_bytes(t, backward) > limit) --t;
  return t;
}

bool group_norm_tile_supported(int64_t T, int64_t D, int64_t groups) {
  return T >= 1 && groups >= 1 && D % groups == 0 &&
         gn_tile_width_ok((int)D, (int)groups) &&
         T <= group_norm_tile_max_rows(false) &&
         T <= group_norm_tile_max_rows(true);
}

std::vector<torch::Tensor> group_norm_fwd(torch::Tensor x,
                                          torch::Tensor gamma,
                                          torch::Tensor beta,
                                          c10::optional<torch::Tensor> pad,
                                          int64_t groups, double eps,
                                          int64_t act,
                                          const std::string& route) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 3 &&
              x.scalar_type() == torch::kBFloat16);
  const int B = x.size(0), T = x.size(1), D = x.size(2);
  const int G = (int)groups;
  TORCH_CHECK(D % G == 0 && D / G <= 64, "cg must be <= 64");
  // 'auto' takes the vector kernel for cg % 8 == 0; 'scalar' forces the
  // per-element kernel (the tests' yardstick); 'tile' the tile-resident
  // kernel, which callers choose (ops/group_norm.py).
  TORCH_CHECK(route == "auto" || route == "scalar" || route == "vec" ||
                  route == "tile",
              "route must be 'auto', 'scalar', 'vec' or 'tile'");
  auto opts = x.options().dtype(torch::kFloat32);
  auto stream = at::cuda::getCurrentCUDAStream();
  const unsigned short* padp = pad.has_value() ? u16(*pad) : nullptr;
  if (route == "tile") {
    const size_t lds = gn_tile_check(x, gamma, beta, pad, G, false);
    auto y = torch::empty_like(x);
    auto mean = torch::empty({(long)B * G}, opts);
    auto rstd = torch::empty({(long)B * G}, opts);
    const int nslab = cdiv(D, GN_TILE_CB);
    hipLaunchKernelGGL((gn_fwd_tile_kernel<GnFwdTile>),
                       dim3((unsigned)(B * nslab)), dim3(GnFwdTile::NT), lds,
                       stream, u16(x), u16(gamma), u16(beta), padp, u16(y),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(), T, D,
                       G, nslab, (float)eps, (int)act);
    return {y, mean, rstd};
  }
  const bool can_vec = (D / G) % 8 == 0;
  TORCH_CHECK(route != "vec" || can_vec, "route='vec' needs cg % 8 == 0");
  const bool vec = can_vec && route != "scalar";
  auto y = torch::empty_like(x);
  auto mean = torch::empty({(long)B * G}, opts);
  auto rstd = torch::empty({(long)B * G}, opts);
  TORCH_CHECK(act == 0 || (D / G) % 8 == 0,
              "fused activation needs cg % 8 == 0");
  hipLaunchKernelGGL(vec ? gn_fwd_vec_kernel : gn_fwd_kernel, dim3(B * G),
                     dim3(GN_BLOCK), 0, stream, u16(x), u16(gamma), u16(beta),
                     padp, u16(y), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(), B, T, D, G, (float)eps,
                     (int)act);
  return {y, mean, rstd};
}

std::vector<torch::Tensor> group_norm_bwd(torch::Tensor dy, torch::Tensor x,
                                          torch::Tensor gamma,
                                          torch::Tensor beta,
                                          c10::optional<torch::Tensor> pad,
                                          torch::Tensor mean,
                                          torch::Tensor rstd,
                                          int64_t groups, int64_t act,
                                          const std::string& route) {
  TORCH_CHECK(route == "auto" || route == "vec" || route == "tile",
              "route must be 'auto', 'vec' or 'tile'");
  const int B = x.size(0), T = x.size(1), D = x.size(2);
  const int G = (int)groups;
  auto opts = x.options().dtype(torch::kFloat32);
  auto stream = at::cuda::getCurrentCUDAStream();
  const unsigned short* padp = pad.has_value() ? u16(*pad) : nullptr;
  if (route == "tile") {
    const size_t lds = gn_tile_check(x, gamma, beta, pad, G, true);
    check_contig(dy, torch::kBFloat16, "group_norm: dy");
    check_contig(mean, torch::kFloat32, "group_norm: mean");
    check_contig(rstd, torch::kFloat32, "group_norm: rstd");
    TORCH_CHECK(dy.sizes() == x.sizes() && aligned16(dy) &&
                    mean.numel() == (long)B * G && rstd.numel() == (long)B * G,
                "group_norm: dy must match x, mean and rstd must be [B*G]");
    auto dx = torch::empty_like(x);
    // Every column of every row is written by exactly one workgroup.
    auto part = torch::empty({B, 2L * D}, opts);
    auto dgb = torch::empty({2L * D}, opts);
    const int nslab = cdiv(D, GN_TILE_CB);
    hipLaunchKernelGGL((gn_bwd_tile_kernel<GnBwdTile>),
                       dim3((unsigned)(B * nslab)), dim3(GnBwdTile::NT), lds,
                       stream, u16(dy), u16(x), u16(gamma), u16(beta), padp,
                       mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       u16(dx), part.data_ptr<float>(), T, D, G, nslab,
                       (int)act);
    colsum_reduce(part.data_ptr<float>(), dgb.data_ptr<float>(), B, 2L * D,
                  stream);
    return {dx, dgb.slice(0, 0, D), dgb.slice(0, D, 2L * D)};
  }
  auto dx = torch::empty_like(x);
  auto dgamma = torch::zeros({D}, opts);
  auto dbeta = torch::zeros({D}, opts);
  const int cg = D / G;
  const bool vec = cg % 8 == 0 && GN_BLOCK % (cg / 8) == 0;
  TORCH_CHECK(route != "vec" || vec, "route='vec' needs cg % 8 == 0");
  TORCH_CHECK(act == 0 || vec, "fused activation needs cg % 8 == 0");
  auto kern = vec ? gn_bwd_vec_kernel : gn_bwd_kernel;
  hipLaunchKernelGGL(kern, dim3(B * G), dim3(GN_BLOCK), 0, stream, u16(dy),
                     u16(x), u16(gamma), u16(beta), padp,
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), u16(dx),
                     dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), B,
                     T, D, G, (int)act);
  return {dx, dgamma, dbeta};
}
