// Transformer-XL relative attention for gfx950, forward and backward
// (layers/attention.py TransformerXLAttention; Dai et al. 2019).
//
// Per batch b and head n, S = M + T keys (M = memory length):
//   logit[i,j] = scale * ((q_i + u_n).k_j + (q_i + w_n).r[(M+i) - j + (S-1)])
//   visible(i,j) = j < klen[b] and (not causal or j <= M + i)
//   o_i = softmax_j(logit[i,.]) . v
// q [B,T,N,64], k/v [B,S,N,64], r [2S-1,N,64] bf16; u, w [N,64].
//
// The position term never exists at [T,S] or [T,2S-1]. A block of XQ = 64
// query rows and a tile of XK = 64 keys touch 127 distances: the block stages
// those rows of r, reversed, as a 128-row window in LDS (window row c holds
// distance (M + qb + 63 - j0) - c; rows outside [-(S-1), S-1] are zeros). A
// wave's strip of 16 rows needs the 80 window rows from 48 - 16*wave on:
// G[16,80] = (q+w) . Rwin^T is five MFMA column fragments, and the value of
// (row ii, key jj) sits at column jj + 15 - ii, a per-row rotation inside the
// 16-lane C-layout group, done with a cross-lane shuffle (no LDS, no barrier).
//
//  - xl_fwd_kernel: grid (ceil(T/64), N, B), 4 waves, online softmax as in
//    fa_fwd_kernel; K, V^T and the r window staged per key tile; emits o, lse.
//  - xl_bwd_kernel: grid (ceil(S/64), N, B), 4 waves; the block owns a key
//    tile, walks the q tiles and recomputes P from lse. Phase 1 (a wave owns
//    16 query rows): P, dS, then dQc = dS.K and dQp = skew(dS).Rwin go out as
//    fp32 atomics into two [B,T,N,H] accumulators. Phase 2 (a wave owns 16
//    keys, after a barrier): dV += P^T dO and dK += dS^T (q+u) in registers,
//    written once; dRwin = skew(dS)^T (q+w) for 32 window rows per wave, as
//    fp32 atomics into one [2S-1,N,H] accumulator. skew(dS) is the inverse
//    of the forward rotation, written into LDS as MFMA operands.
//  - xl_finish_kernel: dq = dQc + dQp (bf16) and per-slab column sums that
//    colsum_reduce turns into du = sum dQc, dw = sum dQp; xl_cast_kernel
//    rounds dr.

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

constexpr int XH = 64;              // head dim
constexpr int XQ = 64;              // q rows per block / per inner tile
constexpr int XK = 64;              // keys per tile
constexpr int XNW = 4;              // waves per block
constexpr int XBLOCK = XNW * WAVE_SIZE;
constexpr int XWIN = 128;           // staged window rows (127 used)
constexpr int ROWB = XH * 2;        // bytes of a 64-element bf16 row
constexpr int WINB = XWIN * 2;      // pitch of a [.][window] tile

// 8 elements of row `row` (rows >= valid are zeros), plus add[0..8) if given:
// the fp32 add first, then one rounding to bf16.
__device__ __forceinline__ ushortx8 load_row8(const unsigned short* src,
                                              long stride, int row, int valid,
                                              int h0,
                                              const unsigned short* add) {
  ushortx8 v;
  if (row < valid) {
    v = *reinterpret_cast<const ushortx8*>(src + (long)row * stride + h0);
    if (add) {
      const ushortx8 a = *reinterpret_cast<const ushortx8*>(add + h0);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = float_to_bf16_bits(bf16_bits_to_float(v[j]) +
                                  bf16_bits_to_float(a[j]));
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0;
  }
  return v;
}

// 64 rows x 64 h from global into LDS, row-major [row][h] (ROWMAJOR) or
// transposed [h][row], both swizzled with a 128-byte pitch.
template <bool ROWMAJOR>
__device__ void stage64(const unsigned short* src, long stride, int valid,
                        const unsigned short* add, char* dst) {
  const int r0 = threadIdx.x >> 3;
  const int h0 = (threadIdx.x & 7) * 8;
#pragma unroll
  for (int rp = 0; rp < 64 / (XBLOCK / 8); ++rp) {
    const int row = r0 + rp * (XBLOCK / 8);
    const ushortx8 v = load_row8(src, stride, row, valid, h0, add);
    if (ROWMAJOR) {
      *reinterpret_cast<ushortx8*>(dst + row * ROWB + swz(row, h0 * 2)) = v;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) lds_put(dst, h0 + j, ROWB, row, v[j]);
    }
  }
}

// The block's window of r: row c holds r[dtop - c + (S-1)] of head n, zeros
// where that index is outside [0, 2S-2]. win is [XWIN][64] row-major; wint,
// when given, is the transpose [64][XWIN].
__device__ void stage_window(const unsigned short* r, int n, int N, int S,
                             int dtop, char* win, char* wint) {
  const int r0 = threadIdx.x >> 3;
  const int h0 = (threadIdx.x & 7) * 8;
#pragma unroll
  for (int rp = 0; rp < XWIN / (XBLOCK / 8); ++rp) {
    const int c = r0 + rp * (XBLOCK / 8);
    const int idx = dtop - c + (S - 1);
    ushortx8 v;
    if (idx >= 0 && idx <= 2 * S - 2) {
      v = *reinterpret_cast<const ushortx8*>(r + ((long)idx * N + n) * XH +
                                             h0);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0;
    }
    *reinterpret_cast<ushortx8*>(win + c * ROWB + swz(c, h0 * 2)) = v;
    if (wint) {
#pragma unroll
      for (int j = 0; j < 8; ++j) lds_put(wint, h0 + j, WINB, c, v[j]);
    }
  }
}

// A-operand fragments (row = lane & 15) of one 16-row strip of x [.,64] with
// an optional per-head row vector added in fp32 before the rounding.
__device__ __forceinline__ void load_a_frags(const unsigned short* x,
                                             long stride, int row, int valid,
                                             const unsigned short* add, int g,
                                             bf16x8* out) {
#pragma unroll
  for (int kk = 0; kk < XH / 32; ++kk) {
    union {
      ushortx8 u;
      bf16x8 h;
    } cv;
    cv.u = load_row8(x, stride, row, valid, kk * 32 + g * 8, add);
    out[kk] = cv.h;
  }
}

// logits of one wave's strip against the staged key tile and window:
// s[nf][r] = (q+u).k + rel-shifted (q+w).r, unscaled, C layout (row g*4+r,
// key nf*16+cl).
__device__ __forceinline__ void strip_logits(const bf16x8* qu,
                                             const bf16x8* qw,
                                             const char* k_lds,
                                             const char* win, int wid, int g,
                                             int cl, float s[XK / 16][4]) {
  constexpr int KH = XH / 32;
  constexpr int NF = XK / 16;
  const int woff = 48 - 16 * wid;
  float gm[NF + 1][4];
#pragma unroll
  for (int nf = 0; nf < NF + 1; ++nf) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KH; ++kk)
      acc = mfma16x16x32_bf16(
          qw[kk],
          lds_frag(win, woff + nf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2),
          acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) gm[nf][r] = acc[r];
  }
#pragma unroll
  for (int nf = 0; nf < NF; ++nf) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KH; ++kk)
      acc = mfma16x16x32_bf16(
          qu[kk], lds_frag(k_lds, nf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2),
          acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) s[nf][r] = acc[r];
  }
  // Rel-shift: (row, key jj) reads G column jj + 15 - row, i.e. lane
  // (cl + 15 - row) & 15 of the same 16-lane group, one fragment further on
  // when that sum carries.
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int sh = cl + 15 - (g * 4 + r);
    const int src = (g << 4) | (sh & 15);
    // A bit mask, not a ternary on t[]: the latter becomes an indexed load
    // from a private-memory copy of t.
    const int carry = -(sh >> 4);
    int t[NF + 1];
#pragma unroll
    for (int nf = 0; nf < NF + 1; ++nf)
      t[nf] = __shfl(__float_as_int(gm[nf][r]), src);
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
      s[nf][r] += __int_as_float((t[nf + 1] & carry) | (t[nf] & ~carry));
  }
}

__device__ __forceinline__ int clamp_klen(const int* klen_ptr, int b, int S) {
  return klen_ptr ? max(0, min(klen_ptr[b], S)) : S;
}

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(XBLOCK) void xl_fwd_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const unsigned short* __restrict__ rr,
    const unsigned short* __restrict__ u, const unsigned short* __restrict__ w,
    const int* __restrict__ klen_ptr, unsigned short* __restrict__ o,
    float* __restrict__ lse, int T, int S, int N, int causal, float scale) {
  constexpr int HF = XH / 16;
  constexpr int NF = XK / 16;
  extern __shared__ char smem[];
  char* k_lds = smem;                     // [XK][64]
  char* vt_lds = k_lds + XK * ROWB;       // [64][XK]
  char* win = vt_lds + XH * ROWB;         // [XWIN][64]
  char* p_lds = win + XWIN * ROWB;        // [XNW][16][XK]

  const int qb = blockIdx.x * XQ;
  const int n = blockIdx.y;
  const int b = blockIdx.z;
  const int M = S - T;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int cl = lane & 15;
  const int klen = clamp_klen(klen_ptr, b, S);
  const int q0 = qb + wid * 16;
  const long row_stride = (long)N * XH;

  bf16x8 qu[XH / 32], qw[XH / 32];
  {
    const unsigned short* qs = q + ((long)b * T + q0) * row_stride + n * XH;
    load_a_frags(qs, row_stride, cl, T - q0, u + n * XH, g, qu);
    load_a_frags(qs, row_stride, cl, T - q0, w + n * XH, g, qw);
  }

  f32x4 acc_o[HF];
#pragma unroll
  for (int hf = 0; hf < HF; ++hf) acc_o[hf] = {0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = NEG_INF;
    l_run[r] = 0.f;
  }

  const int kmax_excl = min(klen, causal ? min(S, M + qb + XQ) : S);
  const int kt_hi = (max(kmax_excl, 1) - 1) / XK;
  for (int kt = 0; kt <= kt_hi; ++kt) {
    const int j0 = kt * XK;
    stage64<true>(k + ((long)b * S + j0) * row_stride + n * XH, row_stride,
                  klen - j0, nullptr, k_lds);
    stage64<false>(v + ((long)b * S + j0) * row_stride + n * XH, row_stride,
                   klen - j0, nullptr, vt_lds);
    stage_window(rr, n, N, S, M + qb + XQ - 1 - j0, win, nullptr);
    __syncthreads();

    float s[NF][4];
    strip_logits(qu, qw, k_lds, win, wid, g, cl, s);
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const int key = j0 + nf * 16 + cl;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = q0 + g * 4 + r;
        const bool vis =
            qrow < T && key < klen && (!causal || key <= M + qrow);
        s[nf][r] = vis ? s[nf][r] * scale : NEG_INF;
      }
    }

    // Online softmax; row r lives across the 16 lanes of this lane's group.
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = s[0][r];
#pragma unroll
      for (int nf = 1; nf < NF; ++nf) mx = fmaxf(mx, s[nf][r]);
#pragma unroll
      for (int off = 1; off < 16; off <<= 1)
        mx = fmaxf(mx, __shfl_xor(mx, off));
      const float m_new = fmaxf(m_run[r], mx);
      const float alpha =
          (m_run[r] == NEG_INF) ? 0.f : __expf(m_run[r] - m_new);
      m_run[r] = m_new;
      float sum = 0.f;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        const float p =
            (s[nf][r] <= NEG_INF * 0.5f) ? 0.f : __expf(s[nf][r] - m_new);
        s[nf][r] = p;
        sum += p;
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) sum += __shfl_xor(sum, off);
      l_run[r] = l_run[r] * alpha + sum;
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) acc_o[hf][r] *= alpha;
    }

    // P -> per-wave LDS as the A operand of P.V; same-wave DS ordering
    // makes the reads safe without a barrier.
    char* pw = p_lds + wid * 16 * ROWB;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        lds_put(pw, g * 4 + r, ROWB, nf * 16 + cl,
                float_to_bf16_bits(s[nf][r]));
#pragma unroll
    for (int kk = 0; kk < XK / 32; ++kk) {
      const bf16x8 pa = lds_frag(pw, cl, ROWB, (kk * 32 + g * 8) * 2);
#pragma unroll
      for (int hf = 0; hf < HF; ++hf)
        acc_o[hf] = mfma16x16x32_bf16(
            pa, lds_frag(vt_lds, hf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2),
            acc_o[hf]);
    }
    __syncthreads();
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + g * 4 + r;
    if (qrow >= T) continue;
    const float inv_l = l_run[r] > 0.f ? 1.f / l_run[r] : 0.f;
    unsigned short* orow = o + (((long)b * T + qrow) * N + n) * XH;
#pragma unroll
    for (int hf = 0; hf < HF; ++hf)
      orow[hf * 16 + cl] = float_to_bf16_bits(acc_o[hf][r] * inv_l);
    if (cl == 0)
      lse[((long)b * N + n) * T + qrow] =
          l_run[r] > 0.f ? m_run[r] + __logf(l_run[r]) : NEG_INF;
  }
}

// ---------------------------------------------------------------------------
// Backward
// ---------------------------------------------------------------------------
constexpr size_t kBwdLds =
    3 * XK * ROWB              // k_lds, kt_lds, v_lds
    + 2 * XWIN * ROWB          // win, wint
    + 3 * XH * ROWB            // qut, qwt, dot
    + 2 * XK * ROWB            // pt, dst
    + XWIN * ROWB              // dskt
    + XNW * 16 * (ROWB + WINB);  // per wave: ds, dsk

__global__ __launch_bounds__(XBLOCK) void xl_bwd_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const unsigned short* __restrict__ rr,
    const unsigned short* __restrict__ u, const unsigned short* __restrict__ w,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const int* __restrict__ klen_ptr, float* __restrict__ dqc_acc,
    float* __restrict__ dqp_acc, float* __restrict__ dr_acc,
    unsigned short* __restrict__ dk, unsigned short* __restrict__ dv, int T,
    int S, int N, int causal, float scale) {
  constexpr int HF = XH / 16;
  constexpr int NF = XK / 16;
  extern __shared__ char smem[];
  char* k_lds = smem;                      // [key][h]   B of (q+u).K^T
  char* kt_lds = k_lds + XK * ROWB;        // [h][key]   B of dS.K
  char* v_lds = kt_lds + XH * ROWB;        // [key][h]   B of dO.V^T
  char* win = v_lds + XK * ROWB;           // [c][h]     B of (q+w).Rwin^T
  char* wint = win + XWIN * ROWB;          // [h][c]     B of skew(dS).Rwin
  char* qut = wint + XH * WINB;            // [h][ii]    B of dS^T.(q+u)
  char* qwt = qut + XH * ROWB;             // [h][ii]    B of skew(dS)^T.(q+w)
  char* dot = qwt + XH * ROWB;             // [h][ii]    B of P^T.dO
  char* pt = dot + XH * ROWB;              // [key][ii]  A: P^T
  char* dst = pt + XK * ROWB;              // [key][ii]  A: dS^T
  char* dskt = dst + XK * ROWB;            // [c][ii]    A: skew(dS)^T
  char* ds_w = dskt + XWIN * ROWB;         // [wave][16][key]  A: dS
  char* dsk_w = ds_w + XNW * 16 * ROWB;    // [wave][16][c]    A: skew(dS)

  const int j0 = blockIdx.x * XK;
  const int n = blockIdx.y;
  const int b = blockIdx.z;
  const int M = S - T;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int cl = lane & 15;
  const int klen = clamp_klen(klen_ptr, b, S);
  const long row_stride = (long)N * XH;

  f32x4 acc_dk[HF], acc_dv[HF];
#pragma unroll
  for (int hf = 0; hf < HF; ++hf) {
    acc_dk[hf] = {0.f, 0.f, 0.f, 0.f};
    acc_dv[hf] = {0.f, 0.f, 0.f, 0.f};
  }

  // q tiles with a visible (i, j): j <= M + i needs qb + 63 >= j0 - M. A
  // key tile at or past klen has none.
  const int qt_lo = causal ? max(0, j0 - M) / XQ : 0;
  const int qt_hi = j0 < klen ? (T - 1) / XQ : -1;

  if (qt_lo <= qt_hi) {
    const unsigned short* ks = k + ((long)b * S + j0) * row_stride + n * XH;
    stage64<true>(ks, row_stride, klen - j0, nullptr, k_lds);
    stage64<false>(ks, row_stride, klen - j0, nullptr, kt_lds);
    stage64<true>(v + ((long)b * S + j0) * row_stride + n * XH, row_stride,
                  klen - j0, nullptr, v_lds);
  }

  for (int qt = qt_lo; qt <= qt_hi; ++qt) {
    const int qb = qt * XQ;
    const int dtop = M + qb + XQ - 1 - j0;
    const unsigned short* qs = q + ((long)b * T + qb) * row_stride + n * XH;
    const unsigned short* dos =
        dout + ((long)b * T + qb) * row_stride + n * XH;
    __syncthreads();  // phase 2 of the previous tile is done with the tiles
    stage_window(rr, n, N, S, dtop, win, wint);
    stage64<false>(qs, row_stride, T - qb, u + n * XH, qut);
    stage64<false>(qs, row_stride, T - qb, w + n * XH, qwt);
    stage64<false>(dos, row_stride, T - qb, nullptr, dot);
    __syncthreads();

    // ---- phase 1: this wave's 16 query rows against the 64 keys ----------
    const int ib = wid * 16;  // strip's first row inside the q tile
    bf16x8 qu[XH / 32], qw[XH / 32], dof[XH / 32];
    load_a_frags(qs + ib * row_stride, row_stride, cl, T - qb - ib,
                 u + n * XH, g, qu);
    load_a_frags(qs + ib * row_stride, row_stride, cl, T - qb - ib,
                 w + n * XH, g, qw);
    load_a_frags(dos + ib * row_stride, row_stride, cl, T - qb - ib, nullptr,
                 g, dof);
    float lse_r[4], delta_r[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = qb + ib + g * 4 + r;
      const bool ok = qrow < T;
      lse_r[r] = ok ? lse[((long)b * N + n) * T + qrow] : NEG_INF;
      delta_r[r] = ok ? delta[((long)b * N + n) * T + qrow] : 0.f;
    }

    float s[NF][4];
    strip_logits(qu, qw, k_lds, win, wid, g, cl, s);

    char* dsw = ds_w + wid * 16 * ROWB;
    char* dskw = dsk_w + wid * 16 * WINB;
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < XH / 32; ++kk)
        dp = mfma16x16x32_bf16(
            dof[kk],
            lds_frag(v_lds, nf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2), dp);
      const int jj = nf * 16 + cl;
      const int key = j0 + jj;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = g * 4 + r;
        const int ii = ib + row;
        const int qrow = qb + ii;
        const bool vis = qrow < T && key < klen &&
                         (!causal || key <= M + qrow) &&
                         lse_r[r] > NEG_INF * 0.5f;
        const float p = vis ? __expf(s[nf][r] * scale - lse_r[r]) : 0.f;
        const unsigned short pb = float_to_bf16_bits(p);
        const unsigned short dsb =
            float_to_bf16_bits(p * (dp[r] - delta_r[r]) * scale);
        lds_put(pt, jj, ROWB, ii, pb);
        lds_put(dst, jj, ROWB, ii, dsb);
        lds_put(dsw, row, ROWB, jj, dsb);
        // Inverse rel-shift: (ii, jj) lands at window row jj + 63 - ii.
        const int c = jj + 63 - ii;
        lds_put(dskw, row, WINB, c, dsb);
        lds_put(dskt, c, ROWB, ii, dsb);
        // Row ii's band is [63 - ii, 126 - ii]; the 64 window rows outside
        // it are zeros, one per (nf, cl).
        const int cz = jj < 63 - ii ? jj : jj + 64;
        lds_put(dskw, row, WINB, cz, 0);
        lds_put(dskt, cz, ROWB, ii, 0);
      }
    }

    // dQc = dS.K and dQp = skew(dS).Rwin for this strip.
    {
      f32x4 acc_c[HF], acc_p[HF];
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) {
        acc_c[hf] = {0.f, 0.f, 0.f, 0.f};
        acc_p[hf] = {0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int kk = 0; kk < XK / 32; ++kk) {
        const bf16x8 a = lds_frag(dsw, cl, ROWB, (kk * 32 + g * 8) * 2);
#pragma unroll
        for (int hf = 0; hf < HF; ++hf)
          acc_c[hf] = mfma16x16x32_bf16(
              a, lds_frag(kt_lds, hf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2),
              acc_c[hf]);
      }
#pragma unroll
      for (int kk = 0; kk < XWIN / 32; ++kk) {
        const bf16x8 a = lds_frag(dskw, cl, WINB, (kk * 32 + g * 8) * 2);
#pragma unroll
        for (int hf = 0; hf < HF; ++hf)
          acc_p[hf] = mfma16x16x32_bf16(
              a, lds_frag(wint, hf * 16 + cl, WINB, (kk * 32 + g * 8) * 2),
              acc_p[hf]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = qb + ib + g * 4 + r;
        if (qrow >= T) continue;
        const long off = (((long)b * T + qrow) * N + n) * XH + cl;
#pragma unroll
        for (int hf = 0; hf < HF; ++hf) {
          if (acc_c[hf][r] != 0.f)
            atomicAdd(dqc_acc + off + hf * 16, acc_c[hf][r]);
          if (acc_p[hf][r] != 0.f)
            atomicAdd(dqp_acc + off + hf * 16, acc_p[hf][r]);
        }
      }
    }
    __syncthreads();

    // ---- phase 2: this wave's 16 keys / 32 window rows, all 64 queries ---
#pragma unroll
    for (int kk = 0; kk < XQ / 32; ++kk) {
      const bf16x8 pa =
          lds_frag(pt, wid * 16 + cl, ROWB, (kk * 32 + g * 8) * 2);
      const bf16x8 da =
          lds_frag(dst, wid * 16 + cl, ROWB, (kk * 32 + g * 8) * 2);
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) {
        acc_dv[hf] = mfma16x16x32_bf16(
            pa, lds_frag(dot, hf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2),
            acc_dv[hf]);
        acc_dk[hf] = mfma16x16x32_bf16(
            da, lds_frag(qut, hf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2),
            acc_dk[hf]);
      }
    }
#pragma unroll
    for (int rf = 0; rf < 2; ++rf) {
      const int c0 = wid * 32 + rf * 16;
      f32x4 acc_r[HF];
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) acc_r[hf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < XQ / 32; ++kk) {
        const bf16x8 a = lds_frag(dskt, c0 + cl, ROWB, (kk * 32 + g * 8) * 2);
#pragma unroll
        for (int hf = 0; hf < HF; ++hf)
          acc_r[hf] = mfma16x16x32_bf16(
              a, lds_frag(qwt, hf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2),
              acc_r[hf]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int idx = dtop - (c0 + g * 4 + r) + (S - 1);
        if (idx < 0 || idx > 2 * S - 2) continue;
        float* drow = dr_acc + ((long)idx * N + n) * XH + cl;
#pragma unroll
        for (int hf = 0; hf < HF; ++hf)
          if (acc_r[hf][r] != 0.f) atomicAdd(drow + hf * 16, acc_r[hf][r]);
      }
    }
  }

  // dK, dV of this wave's 16 keys, written once (zeros past klen).
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = j0 + wid * 16 + g * 4 + r;
    if (key >= S) continue;
    const long off = (((long)b * S + key) * N + n) * XH + cl;
#pragma unroll
    for (int hf = 0; hf < HF; ++hf) {
      dk[off + hf * 16] = float_to_bf16_bits(acc_dk[hf][r]);
      dv[off + hf * 16] = float_to_bf16_bits(acc_dv[hf][r]);
    }
  }
}

// dq = bf16(dQc + dQp) over rows [B*T] x D = N*64 columns, and this slab's
// column sums of dQc and dQp into partials[slab][2][D].
__global__ __launch_bounds__(XBLOCK) void xl_finish_kernel(
    const float* __restrict__ dqc, const float* __restrict__ dqp,
    unsigned short* __restrict__ dq, float* __restrict__ partials, long rows,
    int D) {
  for (int c = threadIdx.x; c < D; c += XBLOCK) {
    float sc = 0.f, sp = 0.f;
    for (long row = blockIdx.x; row < rows; row += gridDim.x) {
      const float a = dqc[row * D + c], p = dqp[row * D + c];
      dq[row * D + c] = float_to_bf16_bits(a + p);
      sc += a;
      sp += p;
    }
    partials[((long)blockIdx.x * 2) * D + c] = sc;
    partials[((long)blockIdx.x * 2 + 1) * D + c] = sp;
  }
}

__global__ void xl_cast_kernel(const float* __restrict__ src,
                               unsigned short* __restrict__ dst, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    dst[i] = float_to_bf16_bits(src[i]);
}

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------
struct XlShape {
  int B, T, S, N;
};

XlShape xl_check(const torch::Tensor& q, const torch::Tensor& k,
                 const torch::Tensor& v, const torch::Tensor& r,
                 const torch::Tensor& u, const torch::Tensor& w,
                 const c10::optional<torch::Tensor>& klen) {
  check_contig(q, torch::kBFloat16, "q");
  check_contig(k, torch::kBFloat16, "k");
  check_contig(v, torch::kBFloat16, "v");
  check_contig(r, torch::kBFloat16, "r");
  check_contig(u, torch::kBFloat16, "u");
  check_contig(w, torch::kBFloat16, "w");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4, "xl_attn: q [B,T,N,H], k [B,S,N,H]");
  const int B = q.size(0), T = q.size(1), N = q.size(2), H = q.size(3);
  const int S = k.size(1);
  TORCH_CHECK(H == XH, "xl_attn: the kernels support H == 64 only, got ", H);
  TORCH_CHECK(B >= 1 && T >= 1 && N >= 1 && S >= T, "xl_attn: S >= T >= 1");
  TORCH_CHECK(k.size(0) == B && k.size(2) == N && k.size(3) == H &&
                  v.sizes() == k.sizes(),
              "xl_attn: k and v must be [B,S,N,H] with N == q heads");
  TORCH_CHECK(r.dim() == 3 && r.size(0) == 2 * (long)S - 1 && r.size(1) == N &&
                  r.size(2) == H,
              "xl_attn: r must be [2S-1,N,H]");
  TORCH_CHECK(u.dim() == 2 && u.size(0) == N && u.size(1) == H &&
                  w.sizes() == u.sizes(),
              "xl_attn: u and w must be [N,H]");
  TORCH_CHECK(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(r) &&
                  aligned16(u) && aligned16(w),
              "xl_attn: operands must be 16-byte aligned");
  TORCH_CHECK(N <= 65535 && B <= 65535, "xl_attn: N and B are grid dims");
  if (klen.has_value())
    TORCH_CHECK(cuda_contig(*klen, torch::kInt32) && klen->dim() == 1 &&
                    klen->size(0) == B,
                "xl_attn: klen must be int32 [B]");
  return {B, T, S, N};
}

size_t xl_lds_limit() {
  int dev = 0, limit = 0;
  LV_CHECK_HIP(hipGetDevice(&dev));
  LV_CHECK_HIP(hipDeviceGetAttribute(
      &limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  return (size_t)limit;
}

}  // namespace

std::vector<torch::Tensor> xl_attn_fwd(torch::Tensor q, torch::Tensor k,
                                       torch::Tensor v, torch::Tensor r,
                                       torch::Tensor u, torch::Tensor w,
                                       c10::optional<torch::Tensor> klen,
                                       bool causal, double scale) {
  const XlShape s = xl_check(q, k, v, r, u, w, klen);
  auto o = torch::empty_like(q);
  auto lse =
      torch::empty({s.B, s.N, s.T}, q.options().dtype(torch::kFloat32));
  const size_t lds = 2 * XK * ROWB + XWIN * ROWB + XNW * 16 * ROWB;
  hipLaunchKernelGGL(xl_fwd_kernel, dim3(cdiv(s.T, XQ), s.N, s.B),
                     dim3(XBLOCK), lds, at::cuda::getCurrentCUDAStream(),
                     u16(q), u16(k), u16(v), u16(r), u16(u), u16(w),
                     klen.has_value() ? klen->data_ptr<int>() : nullptr,
                     u16(o), lse.data_ptr<float>(), s.T, s.S, s.N,
                     (int)causal, (float)scale);
  return {o, lse};
}

// -> dq, dk, dv (bf16), dr (bf16 [2S-1,N,H]), du, dw (fp32 [N,H]).
std::vector<torch::Tensor> xl_attn_bwd(torch::Tensor dout, torch::Tensor q,
                                       torch::Tensor k, torch::Tensor v,
                                       torch::Tensor r, torch::Tensor u,
                                       torch::Tensor w, torch::Tensor o,
                                       torch::Tensor lse,
                                       c10::optional<torch::Tensor> klen,
                                       bool causal, double scale) {
  const XlShape s = xl_check(q, k, v, r, u, w, klen);
  check_contig(dout, torch::kBFloat16, "dout");
  check_contig(o, torch::kBFloat16, "o");
  check_contig(lse, torch::kFloat32, "lse");
  TORCH_CHECK(dout.sizes() == q.sizes() && o.sizes() == q.sizes() &&
                  lse.numel() == (long)s.B * s.N * s.T,
              "xl_attn_bwd: dout/o must match q, lse must be [B,N,T]");
  TORCH_CHECK(kBwdLds <= xl_lds_limit(), "xl_attn_bwd: needs ", kBwdLds,
              " bytes of LDS per workgroup");
  auto stream = at::cuda::getCurrentCUDAStream();
  auto fopts = q.options().dtype(torch::kFloat32);
  const long rows = (long)s.B * s.T;
  const int D = s.N * XH;

  auto delta = torch::empty({s.B, s.N, s.T}, fopts);
  hipLaunchKernelGGL(attn_delta_kernel<XH>,
                     dim3(cdiv(rows * s.N, DELTA_BLOCK / (XH / 8))),
                     dim3(DELTA_BLOCK), 0, stream, u16(dout), u16(o),
                     delta.data_ptr<float>(), s.B, s.T, s.N);

  auto dqc = torch::zeros({s.B, s.T, s.N, XH}, fopts);
  auto dqp = torch::zeros({s.B, s.T, s.N, XH}, fopts);
  auto dr_acc = torch::zeros({2 * s.S - 1, s.N, XH}, fopts);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  hipLaunchKernelGGL(xl_bwd_kernel, dim3(cdiv(s.S, XK), s.N, s.B),
                     dim3(XBLOCK), kBwdLds, stream, u16(dout), u16(q), u16(k),
                     u16(v), u16(r), u16(u), u16(w), lse.data_ptr<float>(),
                     delta.data_ptr<float>(),
                     klen.has_value() ? klen->data_ptr<int>() : nullptr,
                     dqc.data_ptr<float>(), dqp.data_ptr<float>(),
                     dr_acc.data_ptr<float>(), u16(dk), u16(dv), s.T, s.S,
                     s.N, (int)causal, (float)scale);

  auto dq = torch::empty_like(q);
  const int nslab = (int)std::min<long>(rows, 64);
  auto partials = torch::empty({nslab, 2, D}, fopts);
  auto duw = torch::empty({2, s.N, XH}, fopts);
  hipLaunchKernelGGL(xl_finish_kernel, dim3(nslab), dim3(XBLOCK), 0, stream,
                     dqc.data_ptr<float>(), dqp.data_ptr<float>(), u16(dq),
                     partials.data_ptr<float>(), rows, D);
  colsum_reduce(partials.data_ptr<float>(), duw.data_ptr<float>(), nslab,
                2L * D, stream);
  auto dr = torch::empty_like(r);
  hipLaunchKernelGGL(xl_cast_kernel,
                     dim3(memory_bound_grid(dr.numel(), 256)), dim3(256), 0,
                     stream, dr_acc.data_ptr<float>(), u16(dr), dr.numel());
  return {dq, dk, dv, dr, duw[0], duw[1]};
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
