// Block-sparse attention for gfx950, forward and backward
// (layers/attention_sparse.py BlockSparseAttention; ops/block_sparse_attn.py).
//
// q, k, v [B,T,N,H] bf16, self-attention (one length, N == NKV), H 64 or 128.
// The visibility pattern is static and shared over batch and heads; the host
// turns it into lists of 64x64 tiles (CSR, int32, on the device):
//   q_ptr[QT+1], q_cols[nnz]: per 64-row query tile, ascending, the 64-key
//     tiles that hold a visible element;
//   k_ptr[QT+1], k_rows[nnz]: the transpose, per key tile its query tiles;
//   q_order[QT], k_order[QT]: the tiles by falling list length. The grid is
//     (N, B, QT) and a block takes tile order[blockIdx.z], so the longest
//     lists (a global row walks every key tile) are dispatched first and
//     the short ones fill in behind them.
// A listed tile is wholly visible under the block pattern (blocks are
// multiples of 64 tokens), so the kernels mask elements only for
//   key < klen[b], and, when causal, key <= query on the tile that holds the
// diagonal (kbase + 63 > q0; tiles wholly above it are not listed).
// A row with no visible key gives o = 0, lse = NEG_INF and zero gradients.
//
// All three kernels run 4 waves on a 64-row (or 64-key) tile; a wave owns a
// 16-row strip. bf16 operands, fp32 accumulation, 16x16x32 bf16 MFMA.
//  - bsa_fwd_kernel<H>: grid (N, B, QT). Q fragments in registers; walks
//    q_cols of its tile. The list is known up front, so the global loads of
//    the next listed K/V tile are issued into registers before the MFMA work
//    on the current one and committed to LDS (K row-major, V transposed)
//    after it: the gaps between listed tiles cost nothing. Online softmax as
//    in fa_fwd_kernel; P goes through per-wave LDS for the PV MFMA. Ends at
//    the first tile with kbase >= klen[b] (lists ascend). LDS 24 KB (H=64),
//    40 KB (H=128).
//  - bsa_bwd_dkdv_kernel<H>: grid (N, B, QT), after attn_delta_kernel. K and
//    V fragments and the dK/dV accumulators stay in registers; walks k_rows
//    of its key tile, staging Q and dO (row-major and transposed), lse and
//    delta; recomputes P^T from lse, dP^T = V dO^T, dS^T = P^T (dP^T - delta);
//    dV += P^T dO, dK += scale dS^T Q. Writes dK, dV once. LDS 40.5 KB
//    (H=64), 72.5 KB (H=128).
//  - bsa_bwd_dq_kernel<H>: grid (N, B, QT). Q and dO fragments, lse and delta
//    in registers; walks q_cols again, staging K, V (row-major) and K^T;
//    recomputes P and dS per listed tile and accumulates dQ += scale dS K in
//    registers. Writes dQ once. LDS 32 KB (H=64), 56 KB (H=128).
// No atomics, no fp32 gradient buffer; every sum has a fixed order.

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

#include "sparse_tile.h"

namespace {

// Rows >= valid are zeros.
template <int H>
__device__ __forceinline__ void tile_load(const unsigned short* src,
                                          long stride, int valid,
                                          TileRegs<H>& t) {
  constexpr int TPR = H / 8, RPP = BBLOCK / TPR;
  const int r0 = threadIdx.x / TPR;
  const int h0 = (threadIdx.x % TPR) * 8;
#pragma unroll
  for (int rp = 0; rp < H / 32; ++rp) {
    const int row = r0 + rp * RPP;
    if (row < valid) {
      t.v[rp] =
          *reinterpret_cast<const ushortx8*>(src + (long)row * stride + h0);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) t.v[rp][j] = 0;
    }
  }
}

// A-operand fragments of one 16-row strip of x [.,H]: row = row0 + (lane&15),
// zeros from row `limit` on.
template <int H>
__device__ __forceinline__ void load_strip(const unsigned short* x,
                                           long stride, int row0, int limit,
                                           bf16x8 (&frag)[H / 32]) {
  const int lane = threadIdx.x & 63;
  const int row = row0 + (lane & 15);
#pragma unroll
  for (int kk = 0; kk < H / 32; ++kk) {
    if (row < limit) {
      frag[kk] =
          load_bf16x8_bits(x + (long)row * stride + kk * 32 + (lane >> 4) * 8);
    } else {
      const float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      frag[kk] = pack_bf16x8(z);
    }
  }
}

// The slice [lo, hi) of a list for tile `tile`, clipped to the list.
__device__ __forceinline__ void list_range(const int* __restrict__ ptr,
                                           int tile, int nnz, int& lo,
                                           int& hi) {
  lo = max(ptr[tile], 0);
  hi = min(ptr[tile + 1], nnz);
}

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
template <int H>
__global__ __launch_bounds__(BBLOCK) void bsa_fwd_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const int* __restrict__ klen_ptr,
    const int* __restrict__ q_ptr, const int* __restrict__ q_cols, int nnz,
    const int* __restrict__ order,
    unsigned short* __restrict__ o, float* __restrict__ lse, int T, int N,
    int causal, float scale, long sq, long sk, long sv) {
  constexpr int ROWB = H * 2;
  constexpr int KH = H / 32;
  constexpr int HF = H / 16;
  extern __shared__ char smem[];
  char* k_lds = smem;                   // [64][H] swz
  char* vt_lds = k_lds + BT * ROWB;     // [H][64] swz
  char* p_lds = vt_lds + H * TP;        // [BNW][16][64] swz

  const int qt = order[blockIdx.z], n = blockIdx.x, b = blockIdx.y;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cl = lane & 15;
  const int klen = klen_ptr ? min(max(klen_ptr[b], 0), T) : T;
  const int KT = (T + BT - 1) / BT;
  if (qt < 0 || qt >= KT) return;  // uniform over the block
  const int qb = qt * BT;
  const int q0 = qb + wid * 16;
  const unsigned short* kb = k + (long)b * T * sk + n * H;
  const unsigned short* vb = v + (long)b * T * sv + n * H;

  bf16x8 qfrag[KH];
  load_strip<H>(q + (long)b * T * sq + n * H, sq, q0, T, qfrag);

  f32x4 acc_o[HF];
#pragma unroll
  for (int hf = 0; hf < HF; ++hf) acc_o[hf] = {0.f, 0.f, 0.f, 0.f};
  float m_run[4], l_run[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = NEG_INF;
    l_run[r] = 0.f;
  }

  int i, hi;
  list_range(q_ptr, qt, nnz, i, hi);
  TileRegs<H> kreg, vreg;
  int kt = i < hi ? q_cols[i] : KT;
  if (kt < 0 || kt >= KT || kt * BT >= klen) hi = i;  // nothing to walk
  if (i < hi) {
    tile_load<H>(kb + (long)kt * BT * sk, sk, klen - kt * BT, kreg);
    tile_load<H>(vb + (long)kt * BT * sv, sv, klen - kt * BT, vreg);
  }

  for (; i < hi; ++i) {
    const int kbase = kt * BT;
    tile_put_rows<H>(kreg, k_lds);
    tile_put_transposed<H>(vreg, vt_lds);
    __syncthreads();

    // Loads of the next listed tile, in flight under the MFMA work below.
    if (i + 1 < hi) {
      kt = q_cols[i + 1];
      if (kt < 0 || kt >= KT || kt * BT >= klen) {
        hi = i + 1;  // ascending: every later tile is past klen too
      } else {
        tile_load<H>(kb + (long)kt * BT * sk, sk, klen - kt * BT, kreg);
        tile_load<H>(vb + (long)kt * BT * sv, sv, klen - kt * BT, vreg);
      }
    }

    // S strip: 16 q rows x 64 keys.
    float s[NF][4];
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KH; ++kk) {
        bf16x8 bfr = lds_frag(k_lds, nf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2);
        acc = mfma16x16x32_bf16(qfrag[kk], bfr, acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) s[nf][r] = acc[r] * scale;
    }
    __builtin_amdgcn_s_setprio(0);

    // Element mask: only the tile on the diagonal and the one klen cuts.
    const bool diag = causal && kbase + BT - 1 > qb;
    if (diag || kbase + BT > klen) {
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        const int kcol = kbase + nf * 16 + cl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qrow = q0 + g * 4 + r;
          if (kcol >= klen || (diag && kcol > qrow)) s[nf][r] = NEG_INF;
        }
      }
    }

    // Online softmax. Row r lives across the 16 lanes with this lane's g.
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = s[0][r];
#pragma unroll
      for (int nf = 1; nf < NF; ++nf) mx = fmaxf(mx, s[nf][r]);
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
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

    // P -> per-wave LDS; same-wave DS ordering makes the reads below safe
    // without a barrier.
    char* pw = p_lds + wid * 16 * TP;
    strip_to_lds(s, 1.f, pw);

    // O += P @ V : A = P (rows = q, k = keys), B from Vt (k = keys, col = h).
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk2 = 0; kk2 < BT / 32; ++kk2) {
      bf16x8 pa = lds_frag(pw, cl, TP, (kk2 * 32 + g * 8) * 2);
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) {
        bf16x8 vfr = lds_frag(vt_lds, hf * 16 + cl, TP, (kk2 * 32 + g * 8) * 2);
        acc_o[hf] = mfma16x16x32_bf16(pa, vfr, acc_o[hf]);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }

  // Epilogue: divide by l, store O (bf16) and LSE (fp32). An empty list
  // leaves l = 0: o = 0, lse = NEG_INF.
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + g * 4 + r;
    if (qrow >= T) continue;
    const float inv_l = l_run[r] > 0.f ? 1.f / l_run[r] : 0.f;
    unsigned short* orow = o + (((long)b * T + qrow) * N + n) * H;
#pragma unroll
    for (int hf = 0; hf < HF; ++hf)
      orow[hf * 16 + cl] = float_to_bf16_bits(acc_o[hf][r] * inv_l);
    if (cl == 0)
      lse[((long)b * N + n) * T + qrow] =
          l_run[r] > 0.f ? m_run[r] + __logf(l_run[r]) : NEG_INF;
  }
}

// ---------------------------------------------------------------------------
// Backward: dK, dV per key tile
// ---------------------------------------------------------------------------
template <int H>
constexpr size_t dkdv_lds_bytes() {
  return (size_t)2 * BT * H * 2 + 2 * H * TP + BNW * 16 * TP +
         2 * BT * sizeof(float);
}

template <int H>
__global__ __launch_bounds__(BBLOCK) void bsa_bwd_dkdv_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const float* __restrict__ lse,
    const float* __restrict__ delta, const int* __restrict__ klen_ptr,
    const int* __restrict__ k_ptr, const int* __restrict__ k_rows, int nnz,
    const int* __restrict__ order,
    unsigned short* __restrict__ dk, unsigned short* __restrict__ dv, int T,
    int N, int causal, float scale, long sq, long sk, long sv) {
  constexpr int ROWB = H * 2;
  constexpr int KH = H / 32;
  constexpr int HF = H / 16;
  extern __shared__ char smem[];
  char* q_lds = smem;                        // [64][H] swz
  char* do_lds = q_lds + BT * ROWB;          // [64][H] swz
  char* qt_lds = do_lds + BT * ROWB;         // [H][64] swz
  char* dot_lds = qt_lds + H * TP;           // [H][64] swz
  char* a_lds = dot_lds + H * TP;            // [BNW][16][64] swz
  float* lse_s = (float*)(a_lds + BNW * 16 * TP);   // [64]
  float* delta_s = lse_s + BT;                      // [64]

  const int kt = order[blockIdx.z], n = blockIdx.x, b = blockIdx.y;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cl = lane & 15;
  const int klen = klen_ptr ? min(max(klen_ptr[b], 0), T) : T;
  const int QT = (T + BT - 1) / BT;
  if (kt < 0 || kt >= QT) return;  // uniform over the block
  const int kbase = kt * BT;
  const int k0 = kbase + wid * 16;  // this wave's first key
  const long lrow = ((long)b * N + n) * T;
  const unsigned short* qb_ptr = q + (long)b * T * sq + n * H;
  const unsigned short* dob_ptr = dout + ((long)b * T * N + n) * H;

  // K, V fragments (A layout): row = key, k = h; zeros from klen on.
  bf16x8 kfrag[KH], vfrag[KH];
  load_strip<H>(k + (long)b * T * sk + n * H, sk, k0, klen, kfrag);
  load_strip<H>(v + (long)b * T * sv + n * H, sv, k0, klen, vfrag);

  f32x4 acc_dk[HF], acc_dv[HF];
#pragma unroll
  for (int hf = 0; hf < HF; ++hf) {
    acc_dk[hf] = {0.f, 0.f, 0.f, 0.f};
    acc_dv[hf] = {0.f, 0.f, 0.f, 0.f};
  }

  int i, hi;
  list_range(k_ptr, kt, nnz, i, hi);
  if (kbase >= klen) hi = i;  // no key of this tile is visible

  for (; i < hi; ++i) {
    const int qt = k_rows[i];
    if (qt < 0 || qt >= QT) continue;  // uniform over the block
    const int qb = qt * BT;
    __syncthreads();
    {
      TileRegs<H> t;
      tile_load<H>(qb_ptr + (long)qb * sq, sq, T - qb, t);
      tile_put_rows<H>(t, q_lds);
      tile_put_transposed<H>(t, qt_lds);
      tile_load<H>(dob_ptr + (long)qb * N * H, (long)N * H, T - qb, t);
      tile_put_rows<H>(t, do_lds);
      tile_put_transposed<H>(t, dot_lds);
    }
    if (threadIdx.x < BT) {
      const int qrow = qb + threadIdx.x;
      lse_s[threadIdx.x] = qrow < T ? lse[lrow + qrow] : NEG_INF;
      delta_s[threadIdx.x] = qrow < T ? delta[lrow + qrow] : 0.f;
    }
    __syncthreads();

    const bool diag = causal && kbase + BT - 1 > qb;

    // P^T strip: rows = this wave's 16 keys, cols = 64 queries.
    float pt[NF][4];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KH; ++kk) {
        bf16x8 bq = lds_frag(q_lds, nf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2);
        acc = mfma16x16x32_bf16(kfrag[kk], bq, acc);
      }
      const int qcol = qb + nf * 16 + cl;
      const float l = lse_s[nf * 16 + cl];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + g * 4 + r;
        const bool vis =
            key < klen && !(diag && key > qcol) && l > NEG_INF * 0.5f;
        pt[nf][r] = vis ? __expf(acc[r] * scale - l) : 0.f;
      }
    }

    // dV += P^T @ dO (B from dOt).
    char* aw = a_lds + wid * 16 * TP;
    strip_to_lds(pt, 1.f, aw);
#pragma unroll
    for (int kk2 = 0; kk2 < BT / 32; ++kk2) {
      bf16x8 pa = lds_frag(aw, cl, TP, (kk2 * 32 + g * 8) * 2);
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) {
        bf16x8 bd = lds_frag(dot_lds, hf * 16 + cl, TP, (kk2 * 32 + g * 8) * 2);
        acc_dv[hf] = mfma16x16x32_bf16(pa, bd, acc_dv[hf]);
      }
    }

    // dS^T = P^T o (V dO^T - delta), B from dO rows.
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KH; ++kk) {
        bf16x8 bd = lds_frag(do_lds, nf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2);
        acc = mfma16x16x32_bf16(vfrag[kk], bd, acc);
      }
      const float dl = delta_s[nf * 16 + cl];
#pragma unroll
      for (int r = 0; r < 4; ++r) pt[nf][r] *= acc[r] - dl;
    }

    // dK += scale dS^T @ Q (B from Qt); the strip overwrites P^T in a_lds,
    // whose reads by this wave are done.
    strip_to_lds(pt, scale, aw);
#pragma unroll
    for (int kk2 = 0; kk2 < BT / 32; ++kk2) {
      bf16x8 da = lds_frag(aw, cl, TP, (kk2 * 32 + g * 8) * 2);
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) {
        bf16x8 bq = lds_frag(qt_lds, hf * 16 + cl, TP, (kk2 * 32 + g * 8) * 2);
        acc_dk[hf] = mfma16x16x32_bf16(da, bq, acc_dk[hf]);
      }
    }
  }

  // Written once; an empty list or a tile past klen leaves zeros.
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = k0 + g * 4 + r;
    if (key >= T) continue;
    const long off = (((long)b * T + key) * N + n) * H;
#pragma unroll
    for (int hf = 0; hf < HF; ++hf) {
      dk[off + hf * 16 + cl] = float_to_bf16_bits(acc_dk[hf][r]);
      dv[off + hf * 16 + cl] = float_to_bf16_bits(acc_dv[hf][r]);
    }
  }
}

// ---------------------------------------------------------------------------
// Backward: dQ per query tile
// ---------------------------------------------------------------------------
template <int H>
constexpr size_t dq_lds_bytes() {
  return (size_t)2 * BT * H * 2 + H * TP + BNW * 16 * TP;
}

template <int H>
__global__ __launch_bounds__(BBLOCK) void bsa_bwd_dq_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const float* __restrict__ lse,
    const float* __restrict__ delta, const int* __restrict__ klen_ptr,
    const int* __restrict__ q_ptr, const int* __restrict__ q_cols, int nnz,
    const int* __restrict__ order,
    unsigned short* __restrict__ dq, int T, int N, int causal, float scale,
    long sq, long sk, long sv) {
  constexpr int ROWB = H * 2;
  constexpr int KH = H / 32;
  constexpr int HF = H / 16;
  extern __shared__ char smem[];
  char* k_lds = smem;                   // [64][H] swz
  char* v_lds = k_lds + BT * ROWB;      // [64][H] swz
  char* kt_lds = v_lds + BT * ROWB;     // [H][64] swz
  char* a_lds = kt_lds + H * TP;        // [BNW][16][64] swz

  const int qt = order[blockIdx.z], n = blockIdx.x, b = blockIdx.y;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cl = lane & 15;
  const int klen = klen_ptr ? min(max(klen_ptr[b], 0), T) : T;
  const int KT = (T + BT - 1) / BT;
  if (qt < 0 || qt >= KT) return;  // uniform over the block
  const int qb = qt * BT;
  const int q0 = qb + wid * 16;
  const long lrow = ((long)b * N + n) * T;
  const unsigned short* kb = k + (long)b * T * sk + n * H;
  const unsigned short* vb = v + (long)b * T * sv + n * H;

  bf16x8 qfrag[KH], dofrag[KH];
  load_strip<H>(q + (long)b * T * sq + n * H, sq, q0, T, qfrag);
  load_strip<H>(dout + ((long)b * T * N + n) * H, (long)N * H, q0, T, dofrag);
  float l_row[4], d_row[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + g * 4 + r;
    l_row[r] = qrow < T ? lse[lrow + qrow] : NEG_INF;
    d_row[r] = qrow < T ? delta[lrow + qrow] : 0.f;
  }

  f32x4 acc_dq[HF];
#pragma unroll
  for (int hf = 0; hf < HF; ++hf) acc_dq[hf] = {0.f, 0.f, 0.f, 0.f};

  int i, hi;
  list_range(q_ptr, qt, nnz, i, hi);

  for (; i < hi; ++i) {
    const int kt = q_cols[i];
    if (kt < 0 || kt >= KT || kt * BT >= klen) break;  // ascending list
    const int kbase = kt * BT;
    __syncthreads();
    {
      TileRegs<H> t;
      tile_load<H>(kb + (long)kbase * sk, sk, klen - kbase, t);
      tile_put_rows<H>(t, k_lds);
      tile_put_transposed<H>(t, kt_lds);
      tile_load<H>(vb + (long)kbase * sv, sv, klen - kbase, t);
      tile_put_rows<H>(t, v_lds);
    }
    __syncthreads();

    const bool diag = causal && kbase + BT - 1 > qb;

    // P strip from lse, then dS = P o (dO V^T - delta).
    float ds[NF][4];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      f32x4 dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KH; ++kk) {
        bf16x8 bk = lds_frag(k_lds, nf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2);
        acc = mfma16x16x32_bf16(qfrag[kk], bk, acc);
        bf16x8 bv = lds_frag(v_lds, nf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2);
        dp = mfma16x16x32_bf16(dofrag[kk], bv, dp);
      }
      const int kcol = kbase + nf * 16 + cl;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = q0 + g * 4 + r;
        const bool vis = kcol < klen && !(diag && kcol > qrow) &&
                         l_row[r] > NEG_INF * 0.5f;
        const float p = vis ? __expf(acc[r] * scale - l_row[r]) : 0.f;
        ds[nf][r] = p * (dp[r] - d_row[r]);
      }
    }

    // dQ += scale dS @ K (B from Kt).
    char* aw = a_lds + wid * 16 * TP;
    strip_to_lds(ds, scale, aw);
#pragma unroll
    for (int kk2 = 0; kk2 < BT / 32; ++kk2) {
      bf16x8 da = lds_frag(aw, cl, TP, (kk2 * 32 + g * 8) * 2);
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) {
        bf16x8 bk = lds_frag(kt_lds, hf * 16 + cl, TP, (kk2 * 32 + g * 8) * 2);
        acc_dq[hf] = mfma16x16x32_bf16(da, bk, acc_dq[hf]);
      }
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + g * 4 + r;
    if (qrow >= T) continue;
    const long off = (((long)b * T + qrow) * N + n) * H;
#pragma unroll
    for (int hf = 0; hf < HF; ++hf)
      dq[off + hf * 16 + cl] = float_to_bf16_bits(acc_dq[hf][r]);
  }
}

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------
struct BsaShape {
  int B, T, N, H, QT, nnz;
  long sq, sk, sv;
};

BsaShape bsa_check(const torch::Tensor& q, const torch::Tensor& k,
                   const torch::Tensor& v,
                   const c10::optional<torch::Tensor>& klen,
                   const torch::Tensor& ptr, const torch::Tensor& idx,
                   const torch::Tensor& order) {
  BsaShape s;
  s.sq = check_token_rows(q, "block_sparse_attn", "q");
  s.sk = check_token_rows(k, "block_sparse_attn", "k");
  s.sv = check_token_rows(v, "block_sparse_attn", "v");
  s.B = q.size(0), s.T = q.size(1), s.N = q.size(2), s.H = q.size(3);
  TORCH_CHECK(s.H == 64 || s.H == 128,
              "block_sparse_attn: H must be 64 or 128, got ", s.H);
  TORCH_CHECK(s.B >= 1 && s.T >= 1 && s.N >= 1,
              "block_sparse_attn: B, T, N >= 1");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(),
              "block_sparse_attn: k and v must have the shape of q "
              "(self-attention, N == NKV)");
  s.QT = cdiv(s.T, BT);
  TORCH_CHECK(s.B <= 65535 && s.QT <= 65535,
              "block_sparse_attn: B and ceil(T/64) are grid dims");
  TORCH_CHECK(cuda_contig(ptr, torch::kInt32) && ptr.dim() == 1 &&
                  ptr.size(0) == s.QT + 1,
              "block_sparse_attn: the tile list pointers must be int32 [",
              s.QT + 1, "] for T = ", s.T);
  TORCH_CHECK(cuda_contig(idx, torch::kInt32) && idx.dim() == 1 &&
                  idx.size(0) <= (long)s.QT * s.QT,
              "block_sparse_attn: the tile list must be int32 with at most ",
              (long)s.QT * s.QT, " entries for T = ", s.T);
  s.nnz = idx.size(0);
  TORCH_CHECK(cuda_contig(order, torch::kInt32) && order.dim() == 1 &&
                  order.size(0) == s.QT,
              "block_sparse_attn: the tile order must be int32 [", s.QT,
              "] for T = ", s.T);
  if (klen.has_value())
    TORCH_CHECK(cuda_contig(*klen, torch::kInt32) && klen->dim() == 1 &&
                    klen->size(0) == s.B,
                "block_sparse_attn: klen must be int32 [B]");
  return s;
}

const int* int_ptr(const c10::optional<torch::Tensor>& t) {
  return t.has_value() ? t->data_ptr<int>() : nullptr;
}

}  // namespace

// -> o [B,T,N,H] bf16, lse [B,N,T] fp32.
std::vector<torch::Tensor> bsa_fwd(torch::Tensor q, torch::Tensor k,
                                   torch::Tensor v,
                                   c10::optional<torch::Tensor> klen,
                                   torch::Tensor q_ptr, torch::Tensor q_cols,
                                   torch::Tensor q_order, bool causal,
                                   double scale) {
  const BsaShape s = bsa_check(q, k, v, klen, q_ptr, q_cols, q_order);
  auto o = torch::empty({s.B, s.T, s.N, s.H}, q.options());
  auto lse =
      torch::empty({s.B, s.N, s.T}, q.options().dtype(torch::kFloat32));
  const size_t lds = (size_t)BT * s.H * 2 + s.H * TP + BNW * 16 * TP;
  auto kernel = s.H == 64 ? bsa_fwd_kernel<64> : bsa_fwd_kernel<128>;
  hipLaunchKernelGGL(kernel, dim3(s.N, s.B, s.QT), dim3(BBLOCK), lds,
                     at::cuda::getCurrentCUDAStream(), u16(q), u16(k), u16(v),
                     int_ptr(klen), q_ptr.data_ptr<int>(),
                     q_cols.data_ptr<int>(), s.nnz, q_order.data_ptr<int>(),
                     u16(o),
                     lse.data_ptr<float>(), s.T, s.N, (int)causal,
                     (float)scale, s.sq, s.sk, s.sv);
  return {o, lse};
}

// -> dq, dk, dv, contiguous bf16 [B,T,N,H].
std::vector<torch::Tensor> bsa_bwd(torch::Tensor dout, torch::Tensor q,
                                   torch::Tensor k, torch::Tensor v,
                                   torch::Tensor o, torch::Tensor lse,
                                   c10::optional<torch::Tensor> klen,
                                   torch::Tensor q_ptr, torch::Tensor q_cols,
                                   torch::Tensor q_order, torch::Tensor k_ptr,
                                   torch::Tensor k_rows, torch::Tensor k_order,
                                   bool causal, double scale) {
  const BsaShape s = bsa_check(q, k, v, klen, q_ptr, q_cols, q_order);
  bsa_check(q, k, v, klen, k_ptr, k_rows, k_order);
  check_contig(dout, torch::kBFloat16, "dout");
  check_contig(o, torch::kBFloat16, "o");
  check_contig(lse, torch::kFloat32, "lse");
  TORCH_CHECK(dout.sizes() == q.sizes() && o.sizes() == q.sizes() &&
                  lse.numel() == (long)s.B * s.N * s.T,
              "block_sparse_attn: dout/o must match q, lse must be [B,N,T]");
  TORCH_CHECK(aligned16(dout) && aligned16(o),
              "block_sparse_attn: dout and o must be 16-byte aligned");
  auto stream = at::cuda::getCurrentCUDAStream();
  auto delta = torch::empty({s.B, s.N, s.T}, lse.options());
  {
    auto kernel = s.H == 64 ? attn_delta_kernel<64> : attn_delta_kernel<128>;
    hipLaunchKernelGGL(
        kernel, dim3(cdiv((long)s.B * s.T * s.N, DELTA_BLOCK / (s.H / 8))),
        dim3(DELTA_BLOCK), 0, stream, u16(dout), u16(o),
        delta.data_ptr<float>(), s.B, s.T, s.N);
  }
  auto dq = torch::empty({s.B, s.T, s.N, s.H}, q.options());
  auto dk = torch::empty({s.B, s.T, s.N, s.H}, q.options());
  auto dv = torch::empty({s.B, s.T, s.N, s.H}, q.options());
  const dim3 grid(s.N, s.B, s.QT);
  {
    auto kernel =
        s.H == 64 ? bsa_bwd_dkdv_kernel<64> : bsa_bwd_dkdv_kernel<128>;
    const size_t lds =
        s.H == 64 ? dkdv_lds_bytes<64>() : dkdv_lds_bytes<128>();
    hipLaunchKernelGGL(kernel, grid, dim3(BBLOCK), lds, stream, u16(dout),
                       u16(q), u16(k), u16(v), lse.data_ptr<float>(),
                       delta.data_ptr<float>(), int_ptr(klen),
                       k_ptr.data_ptr<int>(), k_rows.data_ptr<int>(),
                       (int)k_rows.size(0), k_order.data_ptr<int>(), u16(dk),
                       u16(dv), s.T, s.N,
                       (int)causal, (float)scale, s.sq, s.sk, s.sv);
  }
  {
    auto kernel = s.H == 64 ? bsa_bwd_dq_kernel<64> : bsa_bwd_dq_kernel<128>;
    const size_t lds = s.H == 64 ? dq_lds_bytes<64>() : dq_lds_bytes<128>();
    hipLaunchKernelGGL(kernel, grid, dim3(BBLOCK), lds, stream, u16(dout),
                       u16(q), u16(k), u16(v), lse.data_ptr<float>(),
                       delta.data_ptr<float>(), int_ptr(klen),
                       q_ptr.data_ptr<int>(), q_cols.data_ptr<int>(), s.nnz,
                       q_order.data_ptr<int>(), u16(dq), s.T, s.N, (int)causal, (float)scale, s.sq,
                       s.sk, s.sv);
  }
  return {dq, dk, dv};
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
