// Performer / FAVOR+ linear attention for gfx950, forward and backward
// (layers/attention_sparse.py PerformerAttention; Choromanski et al. 2021).
//
// Per batch b and head n, q, k, v [T,64] bf16, proj [M,64] fp32, M % 32 == 0,
// M <= 128, xs = x * 64^(-1/4):
//   z(x)  = xs.proj^T - |xs|^2/2
//   phi_q = exp(z(q) - rowmax)/sqrt(M) + 1e-6
//   phi_k = exp(z(k) - max over all T and M)/sqrt(M) + 1e-6, 0 at s >= klen
//   o_t   = sum_s (phi_q[t].phi_k[s]) v_s / max(sum_s phi_q[t].phi_k[s], 1e-6)
// over all s, or s <= t when causal.
//
// One workgroup of 4 waves per (b, n) walks time in chunks of 64 rows; wave w
// owns rows 16w..16w+15 of a chunk. The feature map runs in-kernel: proj is
// scaled by 64^(-1/4) in fp32, split into bf16 hi + lo tiles resident in LDS,
// and z is two MFMAs per fragment with |xs|^2/2 on the VALU. Features exist
// only as bf16 [64,M] chunk tiles in LDS. The carried state S = sum Kp^T V
// [M,64] stays in fp32 accumulators (wave w owns h columns 16w..16w+15) and
// is rounded to bf16 into LDS only as an MFMA operand; z = sum Kp [M] is fp32
// in LDS, double-buffered across chunks.
//
//  - favor_fwd_kernel: a first loop reduces the key stabiliser, then the
//    scan. Causal: per chunk A = tril(Qp Kp^T), num = A V + Qp S,
//    den = rowsum(A) + Qp.z, then S += Kp^T V, z += colsum(Kp). Non-causal:
//    the same loop twice, accumulate then emit. Emits o, the unclamped den
//    [B,N,T] and the stabiliser [B,N].
//  - favor_bwd_q_kernel: the same forward scan; dQp = dnum S^T + dden z +
//    tril(dA) Kp with dA = dnum V^T + dden, then dq through the feature map.
//  - favor_bwd_kv_kernel: the reverse scan over R = sum Qp^T dnum [M,64] and
//    r = sum Qp dden [M]; dKp = V R^T + r + tril(dA)^T Qp, dV = Kp R +
//    tril(A)^T dnum, then dk through the feature map.
// Every output is written once; there are no atomics.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include "host_checks.h"
#include "mfma.h"

// Device code of this file is built without the packed-fp32 VALU forms; the
// tile helpers are included inside the region so that theirs is too.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "attn_tile.h"

namespace {

constexpr int FH = 64;               // head dim
constexpr int FC = 64;               // rows per chunk
constexpr int FNW = 4;               // waves per block
constexpr int FBLOCK = FNW * WAVE_SIZE;
constexpr int FMAX = 128;            // most features
constexpr int HB = FH * 2;           // pitch of a [.][64] bf16 tile
constexpr int MB = FMAX * 2;         // pitch of a [.][features] bf16 tile
constexpr int K16 = 16 * 1024;
constexpr int K8 = 8 * 1024;
constexpr float PHI_EPS = 1e-6f;
constexpr float DEN_MIN = 1e-6f;

__device__ __forceinline__ bf16x8 as_bf(ushortx8 u) {
  union {
    ushortx8 u;
    bf16x8 h;
  } cv;
  cv.u = u;
  return cv.h;
}

__device__ __forceinline__ float group16_sum(float x) {
#pragma unroll
  for (int off = 1; off < 16; off <<= 1) x += __shfl_xor(x, off);
  return x;
}

// A-operand fragments of 16 rows of x [.,64]: lane (g, cl) holds row cl,
// elements kk*32 + g*8 .. +8. Rows >= valid are zeros and are not read.
__device__ __forceinline__ void load_a2(const unsigned short* x, long stride,
                                        int row, int valid, int g,
                                        ushortx8* out) {
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    ushortx8 u;
#pragma unroll
    for (int j = 0; j < 8; ++j) u[j] = 0;
    if (row < valid)
      u = *reinterpret_cast<const ushortx8*>(x + (long)row * stride + kk * 32 +
                                             g * 8);
    out[kk] = u;
  }
}

// 64 rows x 64 h from global into LDS, row-major [row][h] (ROWMAJOR) or
// transposed [h][row]; rows >= valid are zeros.
template <bool ROWMAJOR>
__device__ void stage64(const unsigned short* src, long stride, int valid,
                        char* dst) {
  const int r0 = threadIdx.x >> 3;
  const int h0 = (threadIdx.x & 7) * 8;
#pragma unroll
  for (int rp = 0; rp < FC / (FBLOCK / 8); ++rp) {
    const int row = r0 + rp * (FBLOCK / 8);
    ushortx8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0;
    if (row < valid)
      v = *reinterpret_cast<const ushortx8*>(src + (long)row * stride + h0);
    if (ROWMAJOR) {
      *reinterpret_cast<ushortx8*>(dst + row * HB + swz(row, h0 * 2)) = v;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) lds_put(dst, h0 + j, HB, row, v[j]);
    }
  }
}

// proj [M,64] fp32 times 64^(-1/4), split into bf16 hi and lo tiles [M][64].
__device__ void stage_proj(const float* proj, int M, char* ph, char* pl) {
  const float s = 0.35355339059327373f;  // 64^(-1/4)
  for (int i = threadIdx.x; i < M * FH; i += FBLOCK) {
    const int f = i / FH, h = i % FH;
    const float x = proj[i] * s;
    const unsigned short hi = float_to_bf16_bits(x);
    lds_put(ph, f, HB, h, hi);
    lds_put(pl, f, HB, h, float_to_bf16_bits(x - bf16_bits_to_float(hi)));
  }
}

// z of the wave's 16 rows, C layout: z[mt][r] is row g*4 + r, feature
// mt*16 + cl.
template <int MT>
__device__ __forceinline__ void feat_z(const ushortx8* xf, const char* ph,
                                       const char* pl, int g, int cl,
                                       float z[MT][4]) {
  float ss = 0.f;
#pragma unroll
  for (int kk = 0; kk < 2; ++kk)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = bf16_bits_to_float(xf[kk][j]);
      ss += f * f;
    }
  ss += __shfl_xor(ss, 16);
  ss += __shfl_xor(ss, 32);  // |x|^2 of row cl
  float nr[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) nr[r] = __shfl(ss, g * 4 + r) * 0.0625f;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int kb = (kk * 32 + g * 8) * 2;
      acc = mfma16x16x32_bf16(as_bf(xf[kk]),
                              lds_frag(ph, mt * 16 + cl, HB, kb), acc);
      acc = mfma16x16x32_bf16(as_bf(xf[kk]),
                              lds_frag(pl, mt * 16 + cl, HB, kb), acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) z[mt][r] = acc[r] - nr[r];
  }
}

// z -> exp(z - rowmax)/sqrt(M) in place (phi_q minus its 1e-6).
template <int MT>
__device__ __forceinline__ void exp_q(float z[MT][4]) {
  const float inv = rsqrtf((float)(MT * 16));
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float mx = z[0][r];
#pragma unroll
    for (int mt = 1; mt < MT; ++mt) mx = fmaxf(mx, z[mt][r]);
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) z[mt][r] = __expf(z[mt][r] - mx) * inv;
  }
}

// z -> exp(z - stab)/sqrt(M) in place (phi_k minus its 1e-6); rows at or past
// `live` give 0.
template <int MT>
__device__ __forceinline__ void exp_k(float z[MT][4], float stab, int row0,
                                      int live) {
  const float inv = rsqrtf((float)(MT * 16));
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      z[mt][r] = row0 + r < live ? __expf(z[mt][r] - stab) * inv : 0.f;
}

// The wave's share of state += X^T Y: xt [M][64 rows] as A, yt [64][64 rows]
// as B, columns 16*wid.. of the state.
template <int MT>
__device__ __forceinline__ void state_update(const char* xt, const char* yt,
                                             int wid, int g, int cl,
                                             f32x4* acc) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int kb = (kk * 32 + g * 8) * 2;
      acc[mt] = mfma16x16x32_bf16(lds_frag(xt, mt * 16 + cl, HB, kb),
                                  lds_frag(yt, wid * 16 + cl, HB, kb), acc[mt]);
    }
}

// vec_out[f] = vec_in[f] + sum_t xt[f][t] * w[t] (w == nullptr: ones), for
// the [M][64] tile xt; one thread per feature.
__device__ __forceinline__ void vec_update(const char* xt, int M,
                                           const float* w, const float* vin,
                                           float* vout) {
  const int f = threadIdx.x;
  if (f >= M) return;
  float sum = 0.f;
#pragma unroll
  for (int c8 = 0; c8 < 8; ++c8) {
    const ushortx8 u =
        *reinterpret_cast<const ushortx8*>(xt + f * HB + swz(f, c8 * 16));
#pragma unroll
    for (int j = 0; j < 8; ++j)
      sum += bf16_bits_to_float(u[j]) * (w ? w[c8 * 8 + j] : 1.f);
  }
  vout[f] = vin[f] + sum;
}

// The state as MFMA operands: sm [M][64] (features by h) and/or st [64][M].
template <int MT>
__device__ __forceinline__ void put_state(const f32x4* acc, int wid, int g,
                                          int cl, char* sm, char* st) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const unsigned short bits = float_to_bf16_bits(acc[mt][r]);
      const int f = mt * 16 + g * 4 + r;
      if (sm) lds_put(sm, f, HB, wid * 16 + cl, bits);
      if (st) lds_put(st, wid * 16 + cl, MB, f, bits);
    }
}

// dnum = dout/max(den, 1e-6) as bf16 A fragments of the wave's 16 rows, and
// dden = -(dnum.o) (0 under the clamp) in C layout: dd[r] is row g*4 + r.
// dden is the diagonal of the MFMA product dnum.O^T, so that it carries the
// rounding of dnum and dA = dnum.V^T + dden cancels exactly where v == o.
__device__ __forceinline__ void load_dnum(const unsigned short* dout,
                                          const unsigned short* o,
                                          const float* den, long stride,
                                          int valid, int g, int cl,
                                          ushortx8* dnf, float* dd) {
  ushortx8 df[2], of[2];
  load_a2(dout, stride, cl, valid, g, df);
  load_a2(o, stride, cl, valid, g, of);
  const float dn = cl < valid ? den[cl] : 1.f;
  const float inv = 1.f / fmaxf(dn, DEN_MIN);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      dnf[kk][j] = float_to_bf16_bits(bf16_bits_to_float(df[kk][j]) * inv);
    acc = mfma16x16x32_bf16(as_bf(dnf[kk]), as_bf(of[kk]), acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = g * 4 + r;
    const float diag = __shfl(acc[r], g * 16 + row);
    dd[r] = __shfl(dn, row) >= DEN_MIN ? -diag : 0.f;
  }
}

// dx of the wave's 16 rows from dz (bf16 [16][M] in dzw, local rows):
// dx = dz.proj' - (sum_m dz) x / 8, proj' the hi tile [M][64] read as a B
// operand element by element.
template <int MT>
__device__ __forceinline__ void store_dx(const char* dzw, const char* ph,
                                         const float* sdz,
                                         const unsigned short* x,
                                         unsigned short* dx, long stride,
                                         int valid, int g, int cl) {
#pragma unroll
  for (int hf = 0; hf < FH / 16; ++hf) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < MT / 2; ++kk) {
      ushortx8 pb;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int f = kk * 32 + g * 8 + j;
        pb[j] = *reinterpret_cast<const unsigned short*>(
            ph + f * HB + swz(f, (hf * 16 + cl) * 2));
      }
      acc = mfma16x16x32_bf16(lds_frag(dzw, cl, MB, (kk * 32 + g * 8) * 2),
                              as_bf(pb), acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = g * 4 + r;
      if (row >= valid) continue;
      const long off = (long)row * stride + hf * 16 + cl;
      dx[off] = float_to_bf16_bits(
          acc[r] - sdz[r] * bf16_bits_to_float(x[off]) * 0.125f);
    }
  }
}

__device__ __forceinline__ int live_keys(const int* klen_ptr, int b, int T) {
  return klen_ptr ? max(0, min(klen_ptr[b], T)) : T;
}

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
constexpr size_t kFwdLds = 6 * K16 + 2 * K8 + (2 * FMAX + FNW) * 4;

template <int MT>
__global__ __launch_bounds__(FBLOCK) void favor_fwd_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const float* __restrict__ proj,
    const int* __restrict__ klen_ptr, unsigned short* __restrict__ o,
    float* __restrict__ den_out, float* __restrict__ kstab_out, int T, int N,
    int causal) {
  constexpr int M = MT * 16;
  extern __shared__ char smem[];
  char* ph = smem;                 // [M][64]  proj hi
  char* pl = ph + K16;             // [M][64]  proj lo
  char* kp = pl + K16;             // [s][M]   B of Qp.Kp^T
  char* kpt = kp + K16;            // [M][s]   A of Kp^T.V
  char* st = kpt + K16;            // [h][M]   B of Qp.S
  char* qp_w = st + K16;           // [wave][16][M]  A: Qp
  char* vt = qp_w + K16;           // [h][s]   B of A.V and of Kp^T.V
  char* a_w = vt + K8;             // [wave][16][s]  A: tril(Qp.Kp^T)
  float* zs = reinterpret_cast<float*>(a_w + K8);  // [2][FMAX]
  float* red = zs + 2 * FMAX;                      // [FNW]

  const int n = blockIdx.x, b = blockIdx.y;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cl = lane & 15;
  const int row0 = wid * 16;
  const long stride = (long)N * FH;
  const long base = (long)b * T * stride + n * FH;
  const int live = live_keys(klen_ptr, b, T);
  const int nchunks = (T + FC - 1) / FC;
  char* qpw = qp_w + wid * 16 * MB;
  char* aw = a_w + wid * 16 * HB;

  stage_proj(proj, M, ph, pl);
  if (threadIdx.x < FMAX) zs[threadIdx.x] = 0.f;
  __syncthreads();

  // Key stabiliser: max of z(k) over every row < T and every feature.
  float stab = -3.0e38f;
  for (int c = 0; c < nchunks; ++c) {
    const int t1 = c * FC + row0;
    ushortx8 xf[2];
    float z[MT][4];
    load_a2(k + base + t1 * stride, stride, cl, T - t1, g, xf);
    feat_z<MT>(xf, ph, pl, g, cl, z);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (t1 + g * 4 + r < T)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) stab = fmaxf(stab, z[mt][r]);
  }
  stab = wave_reduce_max(stab);
  if (lane == 0) red[wid] = stab;
  __syncthreads();
  stab = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  if (threadIdx.x == 0) kstab_out[b * N + n] = stab;

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
  int zcur = 0;

  for (int pass = causal ? 1 : 0; pass < 2; ++pass) {
    const bool accum = causal || pass == 0, emit = pass == 1;
    for (int c = 0; c < nchunks; ++c) {
      const int t0 = c * FC, t1 = t0 + row0;
      float qv[MT][4];
      if (accum) {
        ushortx8 xf[2];
        float z[MT][4];
        load_a2(k + base + t1 * stride, stride, cl, T - t1, g, xf);
        feat_z<MT>(xf, ph, pl, g, cl, z);
        exp_k<MT>(z, stab, t1 + g * 4, live);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const unsigned short bits = float_to_bf16_bits(
                t1 + g * 4 + r < live ? z[mt][r] + PHI_EPS : 0.f);
            lds_put(kp, row0 + g * 4 + r, MB, mt * 16 + cl, bits);
            lds_put(kpt, mt * 16 + cl, HB, row0 + g * 4 + r, bits);
          }
        stage64<false>(v + base + t0 * stride, stride, T - t0, vt);
      }
      if (emit) {
        ushortx8 xf[2];
        load_a2(q + base + t1 * stride, stride, cl, T - t1, g, xf);
        feat_z<MT>(xf, ph, pl, g, cl, qv);
        exp_q<MT>(qv);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const unsigned short bits =
                float_to_bf16_bits(qv[mt][r] + PHI_EPS);
            qv[mt][r] = bf16_bits_to_float(bits);
            lds_put(qpw, g * 4 + r, MB, mt * 16 + cl, bits);
          }
        put_state<MT>(acc, wid, g, cl, nullptr, st);
      }
      __syncthreads();

      if (emit) {
        const float* zc = zs + zcur * FMAX;
        float den[4] = {0.f, 0.f, 0.f, 0.f};
        f32x4 on[FH / 16];
#pragma unroll
        for (int hf = 0; hf < FH / 16; ++hf) on[hf] = {0.f, 0.f, 0.f, 0.f};
        if (causal) {
#pragma unroll
          for (int nf = 0; nf < FC / 16; ++nf) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (nf <= wid) {
#pragma unroll
              for (int kk = 0; kk < MT / 2; ++kk) {
                const int kb = (kk * 32 + g * 8) * 2;
                a = mfma16x16x32_bf16(lds_frag(qpw, cl, MB, kb),
                                      lds_frag(kp, nf * 16 + cl, MB, kb), a);
              }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const bool keep = nf * 16 + cl <= row0 + g * 4 + r;
              const unsigned short bits =
                  float_to_bf16_bits(keep ? a[r] : 0.f);
              den[r] += bf16_bits_to_float(bits);
              lds_put(aw, g * 4 + r, HB, nf * 16 + cl, bits);
            }
          }
#pragma unroll
          for (int kk = 0; kk < FC / 32; ++kk) {
            const int kb = (kk * 32 + g * 8) * 2;
            const bf16x8 af = lds_frag(aw, cl, HB, kb);
#pragma unroll
            for (int hf = 0; hf < FH / 16; ++hf)
              on[hf] = mfma16x16x32_bf16(
                  af, lds_frag(vt, hf * 16 + cl, HB, kb), on[hf]);
          }
        }
#pragma unroll
        for (int kk = 0; kk < MT / 2; ++kk) {
          const int kb = (kk * 32 + g * 8) * 2;
          const bf16x8 qf = lds_frag(qpw, cl, MB, kb);
#pragma unroll
          for (int hf = 0; hf < FH / 16; ++hf)
            on[hf] = mfma16x16x32_bf16(
                qf, lds_frag(st, hf * 16 + cl, MB, kb), on[hf]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            den[r] += qv[mt][r] * zc[mt * 16 + cl];
          den[r] = group16_sum(den[r]);
          const int t = t1 + g * 4 + r;
          if (t >= T) continue;
          const float inv = 1.f / fmaxf(den[r], DEN_MIN);
          unsigned short* orow = o + base + t * stride;
#pragma unroll
          for (int hf = 0; hf < FH / 16; ++hf)
            orow[hf * 16 + cl] = float_to_bf16_bits(on[hf][r] * inv);
          if (cl == 0) den_out[((long)b * N + n) * T + t] = den[r];
        }
      }
      if (accum) {
        state_update<MT>(kpt, vt, wid, g, cl, acc);
        vec_update(kpt, M, nullptr, zs + zcur * FMAX,
                   zs + (zcur ^ 1) * FMAX);
      }
      __syncthreads();
      if (accum) zcur ^= 1;
    }
  }
}

// ---------------------------------------------------------------------------
// Backward, dq: the forward scan again.
// ---------------------------------------------------------------------------
constexpr size_t kBwdQLds = 5 * K16 + 3 * K8 + 2 * FMAX * 4;

template <int MT>
__global__ __launch_bounds__(FBLOCK) void favor_bwd_q_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const float* __restrict__ proj,
    const unsigned short* __restrict__ o, const float* __restrict__ den,
    const float* __restrict__ kstab, const int* __restrict__ klen_ptr,
    unsigned short* __restrict__ dq, int T, int N, int causal) {
  constexpr int M = MT * 16;
  extern __shared__ char smem[];
  char* ph = smem;                 // [M][64]
  char* pl = ph + K16;             // [M][64]
  char* kpt = pl + K16;            // [M][s]   B of dA.Kp, A of Kp^T.V
  char* sm = kpt + K16;            // [M][h]   B of dnum.S^T
  char* dz_w = sm + K16;           // [wave][16][M]  A: dz
  char* vr = dz_w + K16;           // [s][h]   B of dnum.V^T
  char* vt = vr + K8;              // [h][s]   B of Kp^T.V
  char* da_w = vt + K8;            // [wave][16][s]  A: tril(dA)
  float* zs = reinterpret_cast<float*>(da_w + K8);  // [2][FMAX]

  const int n = blockIdx.x, b = blockIdx.y;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cl = lane & 15;
  const int row0 = wid * 16;
  const long stride = (long)N * FH;
  const long base = (long)b * T * stride + n * FH;
  const int live = live_keys(klen_ptr, b, T);
  const int nchunks = (T + FC - 1) / FC;
  const float stab = kstab[b * N + n];
  char* dzw = dz_w + wid * 16 * MB;
  char* daw = da_w + wid * 16 * HB;

  stage_proj(proj, M, ph, pl);
  if (threadIdx.x < FMAX) zs[threadIdx.x] = 0.f;
  __syncthreads();

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
  int zcur = 0;

  for (int pass = causal ? 1 : 0; pass < 2; ++pass) {
    const bool accum = causal || pass == 0, emit = pass == 1;
    for (int c = 0; c < nchunks; ++c) {
      const int t0 = c * FC, t1 = t0 + row0;
      float e[MT][4];
      ushortx8 dnf[2];
      float dd[4];
      if (accum) {
        ushortx8 xf[2];
        float z[MT][4];
        load_a2(k + base + t1 * stride, stride, cl, T - t1, g, xf);
        feat_z<MT>(xf, ph, pl, g, cl, z);
        exp_k<MT>(z, stab, t1 + g * 4, live);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            lds_put(kpt, mt * 16 + cl, HB, row0 + g * 4 + r,
                    float_to_bf16_bits(
                        t1 + g * 4 + r < live ? z[mt][r] + PHI_EPS : 0.f));
        stage64<true>(v + base + t0 * stride, stride, T - t0, vr);
        stage64<false>(v + base + t0 * stride, stride, T - t0, vt);
      }
      if (emit) {
        ushortx8 xf[2];
        load_a2(q + base + t1 * stride, stride, cl, T - t1, g, xf);
        feat_z<MT>(xf, ph, pl, g, cl, e);
        exp_q<MT>(e);
        load_dnum(dout + base + t1 * stride, o + base + t1 * stride,
                  den + ((long)b * N + n) * T + t1, stride, T - t1, g, cl,
                  dnf, dd);
        put_state<MT>(acc, wid, g, cl, sm, nullptr);
      }
      __syncthreads();

      if (emit) {
        const float* zc = zs + zcur * FMAX;
        f32x4 dqp[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) dqp[mt] = {0.f, 0.f, 0.f, 0.f};
        if (causal) {
#pragma unroll
          for (int nf = 0; nf < FC / 16; ++nf) {
            f32x4 da = {0.f, 0.f, 0.f, 0.f};
            if (nf <= wid) {
#pragma unroll
              for (int kk = 0; kk < 2; ++kk)
                da = mfma16x16x32_bf16(
                    as_bf(dnf[kk]),
                    lds_frag(vr, nf * 16 + cl, HB, (kk * 32 + g * 8) * 2), da);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const bool keep = nf * 16 + cl <= row0 + g * 4 + r;
              lds_put(daw, g * 4 + r, HB, nf * 16 + cl,
                      float_to_bf16_bits(keep ? da[r] + dd[r] : 0.f));
            }
          }
#pragma unroll
          for (int kk = 0; kk < FC / 32; ++kk) {
            const int kb = (kk * 32 + g * 8) * 2;
            const bf16x8 af = lds_frag(daw, cl, HB, kb);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
              dqp[mt] = mfma16x16x32_bf16(
                  af, lds_frag(kpt, mt * 16 + cl, HB, kb), dqp[mt]);
          }
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int kb = (kk * 32 + g * 8) * 2;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            dqp[mt] = mfma16x16x32_bf16(
                as_bf(dnf[kk]), lds_frag(sm, mt * 16 + cl, HB, kb), dqp[mt]);
        }
        float sdz[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const unsigned short bits = float_to_bf16_bits(
                (dqp[mt][r] + dd[r] * zc[mt * 16 + cl]) * e[mt][r]);
            sdz[r] += bf16_bits_to_float(bits);
            lds_put(dzw, g * 4 + r, MB, mt * 16 + cl, bits);
          }
#pragma unroll
        for (int r = 0; r < 4; ++r) sdz[r] = group16_sum(sdz[r]);
        store_dx<MT>(dzw, ph, sdz, q + base + t1 * stride,
                     dq + base + t1 * stride, stride, T - t1, g, cl);
      }
      if (accum) {
        state_update<MT>(kpt, vt, wid, g, cl, acc);
        vec_update(kpt, M, nullptr, zs + zcur * FMAX,
                   zs + (zcur ^ 1) * FMAX);
      }
      __syncthreads();
      if (accum) zcur ^= 1;
    }
  }
}

// ---------------------------------------------------------------------------
// Backward, dk and dv: the reverse scan.
// ---------------------------------------------------------------------------
constexpr size_t kBwdKvLds = 7 * K16 + 4 * K8 + (2 * FMAX + FC) * 4;

template <int MT>
__global__ __launch_bounds__(FBLOCK) void favor_bwd_kv_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const float* __restrict__ proj,
    const unsigned short* __restrict__ o, const float* __restrict__ den,
    const float* __restrict__ kstab, const int* __restrict__ klen_ptr,
    unsigned short* __restrict__ dk, unsigned short* __restrict__ dv, int T,
    int N, int causal) {
  constexpr int M = MT * 16;
  extern __shared__ char smem[];
  char* ph = smem;                 // [M][64]
  char* pl = ph + K16;             // [M][64]
  char* kp = pl + K16;             // [s][M]   B of Qp.Kp^T, A of Kp.R; then dz
  char* qpt = kp + K16;            // [M][t]   B of dA^T.Qp, A of Qp^T.dnum
  char* rm = qpt + K16;            // [M][h]   B of V.R^T
  char* rt = rm + K16;             // [h][M]   B of Kp.R
  char* qp_w = rt + K16;           // [wave][16][M]  A: Qp
  char* vr = qp_w + K16;           // [s][h]   B of dnum.V^T
  char* dnt = vr + K8;             // [h][t]   B of A^T.dnum and of Qp^T.dnum
  char* at = dnt + K8;             // [s][t]   A: tril(A)^T
  char* dat = at + K8;             // [s][t]   A: tril(dA)^T
  float* rs = reinterpret_cast<float*>(dat + K8);  // [2][FMAX]
  float* ddl = rs + 2 * FMAX;                      // [FC] dden of the chunk

  const int n = blockIdx.x, b = blockIdx.y;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cl = lane & 15;
  const int row0 = wid * 16;
  const long stride = (long)N * FH;
  const long base = (long)b * T * stride + n * FH;
  const int live = live_keys(klen_ptr, b, T);
  const int nchunks = (T + FC - 1) / FC;
  const float stab = kstab[b * N + n];
  char* qpw = qp_w + wid * 16 * MB;
  char* dzw = kp + row0 * MB;  // the wave's own key rows, once they are spent

  stage_proj(proj, M, ph, pl);
  if (threadIdx.x < FMAX) rs[threadIdx.x] = 0.f;
  __syncthreads();

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
  int rcur = 0;

  for (int pass = causal ? 1 : 0; pass < 2; ++pass) {
    const bool accum = causal || pass == 0, emit = pass == 1;
    for (int c = nchunks - 1; c >= 0; --c) {
      const int t0 = c * FC, t1 = t0 + row0;
      float e[MT][4];
      ushortx8 dnf[2], vf[2];
      float dd[4];
      if (accum) {
        ushortx8 xf[2];
        float z[MT][4];
        load_a2(q + base + t1 * stride, stride, cl, T - t1, g, xf);
        feat_z<MT>(xf, ph, pl, g, cl, z);
        exp_q<MT>(z);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const unsigned short bits = float_to_bf16_bits(z[mt][r] + PHI_EPS);
            lds_put(qpt, mt * 16 + cl, HB, row0 + g * 4 + r, bits);
            if (causal) lds_put(qpw, g * 4 + r, MB, mt * 16 + cl, bits);
          }
        load_dnum(dout + base + t1 * stride, o + base + t1 * stride,
                  den + ((long)b * N + n) * T + t1, stride, T - t1, g, cl,
                  dnf, dd);
        if (cl == 0) {
#pragma unroll
          for (int r = 0; r < 4; ++r) ddl[row0 + g * 4 + r] = dd[r];
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
          for (int j = 0; j < 8; ++j)
            lds_put(dnt, kk * 32 + g * 8 + j, HB, row0 + cl, dnf[kk][j]);
      }
      if (emit) {
        ushortx8 xf[2];
        load_a2(k + base + t1 * stride, stride, cl, T - t1, g, xf);
        feat_z<MT>(xf, ph, pl, g, cl, e);
        exp_k<MT>(e, stab, t1 + g * 4, live);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            lds_put(kp, row0 + g * 4 + r, MB, mt * 16 + cl,
                    float_to_bf16_bits(
                        t1 + g * 4 + r < live ? e[mt][r] + PHI_EPS : 0.f));
        load_a2(v + base + t1 * stride, stride, cl, T - t1, g, vf);
        if (causal) stage64<true>(v + base + t0 * stride, stride, T - t0, vr);
        put_state<MT>(acc, wid, g, cl, rm, rt);
      }
      __syncthreads();

      if (causal) {
        // The wave's 16 query rows against the chunk's keys, stored
        // transposed for the key-major products below.
#pragma unroll
        for (int nf = 0; nf < FC / 16; ++nf) {
          f32x4 a = {0.f, 0.f, 0.f, 0.f}, da = {0.f, 0.f, 0.f, 0.f};
          if (nf <= wid) {
#pragma unroll
            for (int kk = 0; kk < MT / 2; ++kk) {
              const int kb = (kk * 32 + g * 8) * 2;
              a = mfma16x16x32_bf16(lds_frag(qpw, cl, MB, kb),
                                    lds_frag(kp, nf * 16 + cl, MB, kb), a);
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
              da = mfma16x16x32_bf16(
                  as_bf(dnf[kk]),
                  lds_frag(vr, nf * 16 + cl, HB, (kk * 32 + g * 8) * 2), da);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const bool keep = nf * 16 + cl <= row0 + g * 4 + r;
            lds_put(at, nf * 16 + cl, HB, row0 + g * 4 + r,
                    float_to_bf16_bits(keep ? a[r] : 0.f));
            lds_put(dat, nf * 16 + cl, HB, row0 + g * 4 + r,
                    float_to_bf16_bits(keep ? da[r] + dd[r] : 0.f));
          }
        }
        __syncthreads();
      }

      if (emit) {
        const float* rc = rs + rcur * FMAX;
        f32x4 dkp[MT], dvo[FH / 16];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) dkp[mt] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int hf = 0; hf < FH / 16; ++hf) dvo[hf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const int kb = (kk * 32 + g * 8) * 2;
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
            dkp[mt] = mfma16x16x32_bf16(
                as_bf(vf[kk]), lds_frag(rm, mt * 16 + cl, HB, kb), dkp[mt]);
        }
#pragma unroll
        for (int kk = 0; kk < MT / 2; ++kk) {
          const int kb = (kk * 32 + g * 8) * 2;
          const bf16x8 kf = lds_frag(kp, row0 + cl, MB, kb);
#pragma unroll
          for (int hf = 0; hf < FH / 16; ++hf)
            dvo[hf] = mfma16x16x32_bf16(
                kf, lds_frag(rt, hf * 16 + cl, MB, kb), dvo[hf]);
        }
        if (causal) {
#pragma unroll
          for (int kk = 0; kk < FC / 32; ++kk) {
            const int kb = (kk * 32 + g * 8) * 2;
            const bf16x8 daf = lds_frag(dat, row0 + cl, HB, kb);
            const bf16x8 af = lds_frag(at, row0 + cl, HB, kb);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
              dkp[mt] = mfma16x16x32_bf16(
                  daf, lds_frag(qpt, mt * 16 + cl, HB, kb), dkp[mt]);
#pragma unroll
            for (int hf = 0; hf < FH / 16; ++hf)
              dvo[hf] = mfma16x16x32_bf16(
                  af, lds_frag(dnt, hf * 16 + cl, HB, kb), dvo[hf]);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = t1 + g * 4 + r;
          if (t >= T) continue;
          unsigned short* drow = dv + base + t * stride;
#pragma unroll
          for (int hf = 0; hf < FH / 16; ++hf)
            drow[hf * 16 + cl] =
                float_to_bf16_bits(t < live ? dvo[hf][r] : 0.f);
        }
        // dz over the wave's own key rows: every read of them is done.
        float sdz[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const unsigned short bits = float_to_bf16_bits(
                (dkp[mt][r] + rc[mt * 16 + cl]) * e[mt][r]);
            sdz[r] += bf16_bits_to_float(bits);
            lds_put(dzw, g * 4 + r, MB, mt * 16 + cl, bits);
          }
#pragma unroll
        for (int r = 0; r < 4; ++r) sdz[r] = group16_sum(sdz[r]);
        store_dx<MT>(dzw, ph, sdz, k + base + t1 * stride,
                     dk + base + t1 * stride, stride, T - t1, g, cl);
      }
      if (accum) {
        state_update<MT>(qpt, dnt, wid, g, cl, acc);
        vec_update(qpt, M, ddl, rs + rcur * FMAX, rs + (rcur ^ 1) * FMAX);
      }
      __syncthreads();
      if (accum) rcur ^= 1;
    }
  }
}

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------
struct FavorShape {
  int B, T, N, M;
};

FavorShape favor_check(const torch::Tensor& q, const torch::Tensor& k,
                       const torch::Tensor& v, const torch::Tensor& proj,
                       const c10::optional<torch::Tensor>& klen,
                       size_t lds) {
  check_contig(q, torch::kBFloat16, "q");
  check_contig(k, torch::kBFloat16, "k");
  check_contig(v, torch::kBFloat16, "v");
  check_contig(proj, torch::kFloat32, "proj");
  TORCH_CHECK(q.dim() == 4 && proj.dim() == 2,
              "favor_attn: q [B,T,N,H], proj [m,H]");
  const int B = q.size(0), T = q.size(1), N = q.size(2), H = q.size(3);
  const int M = proj.size(0);
  TORCH_CHECK(H == FH, "favor_attn: the kernels support H == 64 only, got ",
              H);
  TORCH_CHECK(M >= 32 && M % 32 == 0 && M <= FMAX && proj.size(1) == H,
              "favor_attn: proj must be [m,64] with m % 32 == 0 and m <= ",
              FMAX);
  TORCH_CHECK(B >= 1 && T >= 1 && N >= 1, "favor_attn: B, T, N >= 1");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(),
              "favor_attn: k and v must have the shape of q");
  TORCH_CHECK(aligned16(q) && aligned16(k) && aligned16(v),
              "favor_attn: operands must be 16-byte aligned");
  TORCH_CHECK(B <= 65535, "favor_attn: B is a grid dim");
  if (klen.has_value())
    TORCH_CHECK(cuda_contig(*klen, torch::kInt32) && klen->dim() == 1 &&
                    klen->size(0) == B,
                "favor_attn: klen must be int32 [B]");
  int dev = 0, limit = 0;
  LV_CHECK_HIP(hipGetDevice(&dev));
  LV_CHECK_HIP(hipDeviceGetAttribute(
      &limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  TORCH_CHECK(lds <= (size_t)limit, "favor_attn: needs ", lds,
              " bytes of LDS per workgroup");
  return {B, T, N, M};
}

// Launches KERNEL<M/16> on a (N, B) grid.
#define FAVOR_LAUNCH(KERNEL, M, lds, N, B, ...)                            \
  do {                                                                     \
    auto stream_ = at::cuda::getCurrentCUDAStream();                       \
    switch ((M) / 16) {                                                    \
      case 2:                                                              \
        hipLaunchKernelGGL(KERNEL<2>, dim3(N, B), dim3(FBLOCK), lds,       \
                           stream_, __VA_ARGS__);                          \
        break;                                                             \
      case 4:                                                              \
        hipLaunchKernelGGL(KERNEL<4>, dim3(N, B), dim3(FBLOCK), lds,       \
                           stream_, __VA_ARGS__);                          \
        break;                                                             \
      case 6:                                                              \
        hipLaunchKernelGGL(KERNEL<6>, dim3(N, B), dim3(FBLOCK), lds,       \
                           stream_, __VA_ARGS__);                          \
        break;                                                             \
      default:                                                             \
        hipLaunchKernelGGL(KERNEL<8>, dim3(N, B), dim3(FBLOCK), lds,       \
                           stream_, __VA_ARGS__);                          \
    }                                                                      \
  } while (0)

}  // namespace

// -> o (bf16 [B,T,N,H]), den (fp32 [B,N,T], unclamped), kstab (fp32 [B,N]).
std::vector<torch::Tensor> favor_attn_fwd(torch::Tensor q, torch::Tensor k,
                                          torch::Tensor v, torch::Tensor proj,
                                          c10::optional<torch::Tensor> klen,
                                          bool causal) {
  const FavorShape s = favor_check(q, k, v, proj, klen, kFwdLds);
  auto fopts = q.options().dtype(torch::kFloat32);
  auto o = torch::empty_like(q);
  auto den = torch::empty({s.B, s.N, s.T}, fopts);
  auto kstab = torch::empty({s.B, s.N}, fopts);
  FAVOR_LAUNCH(favor_fwd_kernel, s.M, kFwdLds, s.N, s.B, u16(q), u16(k),
               u16(v), proj.data_ptr<float>(),
               klen.has_value() ? klen->data_ptr<int>() : nullptr, u16(o),
               den.data_ptr<float>(), kstab.data_ptr<float>(), s.T, s.N,
               (int)causal);
  return {o, den, kstab};
}

// -> dq, dk, dv (bf16 [B,T,N,H]).
std::vector<torch::Tensor> favor_attn_bwd(torch::Tensor dout, torch::Tensor q,
                                          torch::Tensor k, torch::Tensor v,
                                          torch::Tensor proj, torch::Tensor o,
                                          torch::Tensor den,
                                          torch::Tensor kstab,
                                          c10::optional<torch::Tensor> klen,
                                          bool causal) {
  const FavorShape s = favor_check(q, k, v, proj, klen, kBwdKvLds);
  check_contig(dout, torch::kBFloat16, "dout");
  check_contig(o, torch::kBFloat16, "o");
  check_contig(den, torch::kFloat32, "den");
  check_contig(kstab, torch::kFloat32, "kstab");
  TORCH_CHECK(dout.sizes() == q.sizes() && o.sizes() == q.sizes() &&
                  den.numel() == (long)s.B * s.N * s.T &&
                  kstab.numel() == (long)s.B * s.N,
              "favor_attn_bwd: dout/o must match q, den must be [B,N,T] and "
              "kstab [B,N]");
  TORCH_CHECK(aligned16(dout) && aligned16(o),
              "favor_attn_bwd: operands must be 16-byte aligned");
  const int* kl = klen.has_value() ? klen->data_ptr<int>() : nullptr;
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  FAVOR_LAUNCH(favor_bwd_q_kernel, s.M, kBwdQLds, s.N, s.B, u16(dout), u16(q),
               u16(k), u16(v), proj.data_ptr<float>(), u16(o),
               den.data_ptr<float>(), kstab.data_ptr<float>(), kl, u16(dq),
               s.T, s.N, (int)causal);
  FAVOR_LAUNCH(favor_bwd_kv_kernel, s.M, kBwdKvLds, s.N, s.B, u16(dout),
               u16(q), u16(k), u16(v), proj.data_ptr<float>(), u16(o),
               den.data_ptr<float>(), kstab.data_ptr<float>(), kl, u16(dk),
               u16(dv), s.T, s.N, (int)causal);
  return {dq, dk, dv};
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
