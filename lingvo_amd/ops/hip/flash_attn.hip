// Fused flash-attention forward+backward for gfx950 (SURVEY.md K2-K4;
// reference einsums: lingvo/core/batch_major_attention.py:508-514 and
// AttenProbs:943 — BTNH layouts, causal/local/padding masks, clipped
// relative-position bias, GQA).
//
// Structure (guide §B "fused attention prefill"):
//  - fwd, two routes chosen on the host from shapes only:
//    'fused' (fa_fwd_fused_kernel): self-attention with N == NKV, H == 64,
//    T == S <= 384, no segment ids or chunkwise mask. Grid (N, B), one
//    workgroup of 8 waves per head with K and V^T resident in LDS; S^T =
//    K Q^T so a lane owns one query, P goes to the second MFMA from
//    registers (see the kernel's header).
//    'tiles' (fa_fwd_kernel, v1, correctness-first): every other shape.
//    Grid (ceil(T/128), N, B); block = 8 waves; each wave owns a
//    16-row Q strip. K staged in LDS row-major (XOR-swizzled) in tiles of
//    64 keys (128 from S = 512 on), V staged transposed [H][tile]; online
//    softmax in fp32 with per-row (m, l) tracked in the 16-lane C-layout
//    groups; P routed through per-wave
//    LDS for the PV MFMA. Saves LSE for backward.
//  - bwd, two routes chosen on the host from shapes only:
//    'fused' (fa_bwd_fused_kernel): self-attention with N == NKV, H == 64,
//    T == S <= 384, no segment ids or chunkwise mask. Grid (N, B), one
//    workgroup of 8 waves per head; strips of 16 keys live across the
//    waves with K/V fragments and dK/dV accumulators in registers; P and
//    dS go to the dV and dK MFMAs from registers (see the kernel's header);
//    the 32-row q-tiles are walked once, loads for the next tile in flight;
//    delta = rowsum(dO*O) is reduced while dO is staged; dQ is contracted
//    over all keys from a [32][S_pad] dS tile in LDS, rounded once and
//    stored as bf16; the bias gradient leaves as one fp32 row per
//    workgroup, summed over B by fa_dbias_reduce. No atomics, no fp32 dQ
//    buffer, fixed summation order.
//    'tiles' (attn_delta_kernel + fa_bwd_kernel + fa_dq_cast): every other
//    shape. Grid (ceil(S/128), N_kv, B), 8 waves; each block owns a
//    128-key tile, loops q-heads of the GQA group and 64-row q-tiles;
//    recomputes P^T from LSE; dK/dV in registers (written once; fp32
//    atomics across the heads of a GQA group); dQ accumulated through
//    fp32 global atomics into a zero-filled buffer and cast afterwards;
//    clipped rel-position bias gradient via LDS then global atomics.
//
// Masks: key k is visible from query q iff
//   k < klen[b]  AND  (win_l < 0 OR k >= q - win_l)
//                AND  (win_r < 0 OR k <= q + win_r).
// Causal = win_r 0. LocalSelfAttention (batch_major_attention.py:2656)
// = finite (win_l, win_r).

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include "attn_tile.h"

namespace {

// ---------------------------------------------------------------------------
// LDS staging helpers. Row-major tiles are stored with a per-row XOR
// swizzle on 16B granules (mfma.h swz) so B-fragment ds_read_b128 at
// row-stride >= 128B doesn't bank-conflict (guide §6 G4).
// ---------------------------------------------------------------------------

// Stage ROWS x H bf16 from global (row i at src + i*src_stride elems) into
// LDS row-major with swizzle. Rows >= valid_rows are zeroed.
template <int H, int ROWS, int NT>
__device__ void stage_regular(const unsigned short* src, long src_stride,
                              int valid_rows, char* dst) {
  constexpr int ROWB = H * 2;
  constexpr int TPR = ROWB / 16;             // threads per row (16B each)
  constexpr int RPP = NT / TPR;              // rows per pass
  const int tid = threadIdx.x;
  const int r0 = tid / TPR;
  const int byte0 = (tid % TPR) * 16;
#pragma unroll
  for (int rp = 0; rp < (ROWS + RPP - 1) / RPP; ++rp) {
    int row = r0 + rp * RPP;
    // constexpr-folded for ROWS % RPP == 0 (the fwd tile shapes).
    if ((ROWS % RPP) != 0 && row >= ROWS) break;
    ushortx8 v;
    if (row < valid_rows) {
      v = *reinterpret_cast<const ushortx8*>(src + (long)row * src_stride +
                                             byte0 / 2);
    } else {
      for (int j = 0; j < 8; ++j) v[j] = 0;
    }
    *reinterpret_cast<ushortx8*>(dst + row * ROWB + swz(row, byte0)) = v;
  }
}

// Stage ROWS x H bf16 from global into LDS TRANSPOSED as [H][ROWS]
// (ROWS=64, 128B rows), swizzled per h-row. Scalar 2B writes.
template <int H, int ROWS, int NT, int PITCHB = ROWS * 2>
__device__ void stage_transposed(const unsigned short* src, long src_stride,
                                 int valid_rows, char* dst) {
  // PITCHB must be >= 128 when the swizzle is in play: swz() XORs up to
  // 112 bytes into the row, so a 64-byte pitch would corrupt neighbors.
  constexpr int ROWB = H * 2;
  constexpr int TPR = ROWB / 16;
  constexpr int RPP = NT / TPR;
  const int tid = threadIdx.x;
  const int r0 = tid / TPR;
  const int h0 = (tid % TPR) * 8;
#pragma unroll
  for (int rp = 0; rp < (ROWS + RPP - 1) / RPP; ++rp) {
    int row = r0 + rp * RPP;
    if ((ROWS % RPP) != 0 && row >= ROWS) break;
    ushortx8 v;
    if (row < valid_rows) {
      v = *reinterpret_cast<const ushortx8*>(src + (long)row * src_stride +
                                             h0);
    } else {
      for (int j = 0; j < 8; ++j) v[j] = 0;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int h = h0 + j;
      *reinterpret_cast<unsigned short*>(
          dst + h * PITCHB + swz(h, row * 2)) = v[j];
    }
  }
}

__device__ __forceinline__ bool visible(int q, int k, int klen, int win_l,
                                        int win_r, int chunk_lo,
                                        int chunk_hi) {
  if (k >= klen) return false;
  if (win_l >= 0 && k < q - win_l) return false;
  if (win_r >= 0 && k > q + win_r) return false;
  // Chunkwise mask (reference ChunkwiseSelfAttention,
  // batch_major_attention.py:4008): caller precomputes the visible key
  // range [chunk_lo, chunk_hi) PER QUERY (one division per q, not per
  // element — per-element integer division cost 1.7x fwd time).
  if (k < chunk_lo || k >= chunk_hi) return false;
  return true;
}

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
constexpr int FWD_NW = 8;                 // waves per fwd block
constexpr int FWD_BLOCK = FWD_NW * WAVE_SIZE;
constexpr int FQT = FWD_NW * 16;          // q rows per fwd block

template <int H, int KTF, bool SEG>
__global__ __launch_bounds__(FWD_BLOCK) void fa_fwd_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v,
    const int* __restrict__ klen_ptr,          // [B] or null
    const unsigned short* __restrict__ bias,   // [N][2C+1] or null
    const int* __restrict__ qseg,              // [B][T] or null (packed)
    const int* __restrict__ kseg,              // [B][S] or null
    unsigned short* __restrict__ o, float* __restrict__ lse, int B, int T,
    int S, int N, int NKV, int win_l, int win_r, int bias_clip, float scale,
    int chunk, int lc,
    // Token-row strides of q/k/v in elements ([n][h] stays dense): N*H for
    // a contiguous tensor, the packed width for views of a QKV projection.
    long sq, long sk, long sv) {
  constexpr int ROWB = H * 2;
  constexpr int KH = H / 32;   // mfma K-steps over head dim
  constexpr int HF = H / 16;   // output col frags
  constexpr int NF = KTF / 16; // key frags per strip
  extern __shared__ char smem[];
  char* k_lds = smem;                        // [KTF][H] swz
  char* vt_lds = k_lds + KTF * ROWB;         // [H][KTF] swz
  char* p_lds = vt_lds + H * KTF * 2;        // [FWD_NW][16][KTF] swz

  const int qt = blockIdx.x;
  const int n = blockIdx.y;
  const int b = blockIdx.z;
  const int nkv = n / (N / NKV);
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;       // 16-lane group
  const int cl = lane & 15;      // col-in-frag
  const int klen = klen_ptr ? klen_ptr[b] : S;

  const int q0 = qt * FQT + wid * 16;  // this wave's first q row

  // Q fragments (A layout): row = cl, k = g*8 + kk*32. Folded zeros for
  // rows >= T.
  bf16x8 qfrag[KH];
#pragma unroll
  for (int kk = 0; kk < KH; ++kk) {
    int qrow = q0 + cl;
    if (qrow < T) {
      qfrag[kk] = load_bf16x8_bits(
          q + ((long)b * T + qrow) * sq + n * H + kk * 32 + g * 8);
    } else {
      float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      qfrag[kk] = pack_bf16x8(z);
    }
  }

  // Per-lane chunk windows for its 4 q rows (one division each).
  int cw_lo[4], cw_hi[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (chunk > 0) {
      const int qc = (q0 + g * 4 + r) / chunk;
      cw_lo[r] = (qc - lc) * chunk;
      cw_hi[r] = (qc + 1) * chunk;
    } else {
      cw_lo[r] = 0;
      cw_hi[r] = 0x7fffffff;
    }
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

  // KV tile range from the window.
  int kmax_excl =
      min(klen, win_r < 0 ? S : min(S, qt * FQT + FQT - 1 + win_r + 1));
  int kmin = win_l < 0 ? 0 : max(0, qt * FQT - win_l);
  if (chunk > 0) {
    // Skip key tiles entirely outside the q-tile's chunk window.
    const int qc_lo = (qt * FQT) / chunk;
    const int qc_hi = (qt * FQT + FQT - 1) / chunk;
    kmin = max(kmin, max(0, (qc_lo - lc)) * chunk);
    kmax_excl = min(kmax_excl, (qc_hi + 1) * chunk);
    if (kmax_excl <= kmin) {
      // No visible keys for this whole q-tile: emit zeros (fully-masked
      // rows output 0, matching the reference) and a NEG_INF lse.
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = q0 + g * 4 + r;
        if (qrow >= T) continue;
        unsigned short* orow = o + (((long)b * T + qrow) * N + n) * H;
#pragma unroll
        for (int hf = 0; hf < HF; ++hf) {
          orow[hf * 16 + cl] = float_to_bf16_bits(0.f);
        }
        if (cl == 0) lse[((long)b * N + n) * T + qrow] = NEG_INF;
      }
      return;
    }
  }
  const int kt_lo = kmin / KTF;
  const int kt_hi = (max(kmax_excl, 1) - 1) / KTF;

  for (int kt = kt_lo; kt <= kt_hi; ++kt) {
    const int kbase = kt * KTF;
    // Stage K and V^T.
    stage_regular<H, KTF, FWD_BLOCK>(
        k + ((long)b * S + kbase) * sk + nkv * H, sk, klen - kbase, k_lds);
    stage_transposed<H, KTF, FWD_BLOCK>(
        v + ((long)b * S + kbase) * sv + nkv * H, sv, klen - kbase, vt_lds);
    __syncthreads();

    // S strip: 16 q rows x KTF keys, fp32.
    float s[NF][4];  // [nf over keys][r]
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
      for (int r = 0; r < 4; ++r) s[nf][r] = acc[r];
    }
    __builtin_amdgcn_s_setprio(0);

    // Scale + mask + bias.
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
      const int kcol = kbase + nf * 16 + cl;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qrow = q0 + g * 4 + r;
        float val = s[nf][r] * scale;
        if (bias) {
          int d = qrow - kcol;
          d = d < -bias_clip ? -bias_clip : (d > bias_clip ? bias_clip : d);
          val += bf16_bits_to_float(
              bias[(long)n * (2 * bias_clip + 1) + d + bias_clip]);
        }
        if (!visible(qrow, kcol, klen, win_l, win_r, cw_lo[r], cw_hi[r]) ||
            qrow >= T)
          val = NEG_INF;
        if (SEG) {
          if (kcol < S && qrow < T &&
              qseg[(long)b * T + qrow] != kseg[(long)b * S + kcol])
            val = NEG_INF;
        }
        s[nf][r] = val;
      }
    }

    // Online softmax. Row r lives across the 16 lanes with this lane's g.
    float rowmax[4], rowsum[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float mx = s[0][r];
#pragma unroll
      for (int nf = 1; nf < NF; ++nf) mx = fmaxf(mx, s[nf][r]);
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
      rowmax[r] = mx;
    }
    float alpha[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float m_new = fmaxf(m_run[r], rowmax[r]);
      alpha[r] = (m_run[r] == NEG_INF) ? 0.f : __expf(m_run[r] - m_new);
      m_run[r] = m_new;
      float sum = 0.f;
#pragma unroll
      for (int nf = 0; nf < NF; ++nf) {
        float p = (s[nf][r] <= NEG_INF * 0.5f) ? 0.f
                                               : __expf(s[nf][r] - m_new);
        s[nf][r] = p;
        sum += p;
      }
#pragma unroll
      for (int off = 1; off < 16; off <<= 1) sum += __shfl_xor(sum, off);
      rowsum[r] = sum;
      l_run[r] = l_run[r] * alpha[r] + sum;
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) acc_o[hf][r] *= alpha[r];
    }

    // P -> per-wave LDS (bf16, C layout -> row-major [16][KTF], swizzled).
    char* pw = p_lds + wid * 16 * (KTF * 2);
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int row = g * 4 + r;
        int col = nf * 16 + cl;
        *reinterpret_cast<unsigned short*>(
            pw + row * (KTF * 2) + swz(row, col * 2)) =
            float_to_bf16_bits(s[nf][r]);
      }
    }
    // Same-wave DS ordering makes the reads below safe without a barrier.

    // O += P @ V : A = P (rows=q, k=keys), B from Vt (k=keys, col=h).
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int kk2 = 0; kk2 < KTF / 32; ++kk2) {
      bf16x8 pa = lds_frag(pw, cl, KTF * 2, (kk2 * 32 + g * 8) * 2);
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) {
        bf16x8 vb =
            lds_frag(vt_lds, hf * 16 + cl, KTF * 2, (kk2 * 32 + g * 8) * 2);
        acc_o[hf] = mfma16x16x32_bf16(pa, vb, acc_o[hf]);
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
  }

  // Epilogue: divide by l, store O (bf16) and LSE (fp32).
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + g * 4 + r;
    if (qrow >= T) continue;
    float inv_l = l_run[r] > 0.f ? 1.f / l_run[r] : 0.f;
    unsigned short* orow = o + (((long)b * T + qrow) * N + n) * H;
#pragma unroll
    for (int hf = 0; hf < HF; ++hf) {
      orow[hf * 16 + cl] = float_to_bf16_bits(acc_o[hf][r] * inv_l);
    }
    if (cl == 0) {
      lse[((long)b * N + n) * T + qrow] =
          l_run[r] > 0.f ? m_run[r] + __logf(l_run[r]) : NEG_INF;
    }
  }
}

// ---------------------------------------------------------------------------
// Forward, fused route: one workgroup per (head, batch), self-attention with
// N == NKV, H == 64 and T == S <= FWD_FUSED_MAX_S.
//
// The head's K (row-major) and V^T are staged into LDS once; strips of 16
// queries are dealt round-robin to the waves, and a wave walks its strip's
// keys in steps of 64 with an online softmax.
//
// S^T = K Q^T: in the MFMA C layout a lane then holds one query (its column
// cl) and keys g*4 + r of each 16-key fragment, so the row maximum and sum
// are reductions over the lane's own registers plus the four g-lanes of a
// query, and the rescale and 1/l are one scalar per lane. Logits are kept in
// the base-2 domain (scale and the bias row carry log2 e).
//
// O^T = V^T P^T with P^T as the B operand, straight from registers: two
// neighbouring S^T fragments give a lane the 8 k-slots of a 32-key step in
// the order slot g*8 + hs*4 + r <-> key hs*16 + g*4 + r. The contraction is a
// sum, so V^T is laid out in LDS in that slot order and its A fragment is one
// 16-byte read. A lane ends with 4 consecutive h of one query.
// ---------------------------------------------------------------------------
constexpr int FWD_FUSED_MAX_S = 384;
constexpr int FFK = 64;                    // keys per softmax step
// 8 waves: two workgroups share a CU at 128 registers a wave. 10 waves deal
// the workload's 19 strips more evenly but need 96 registers, spill, and
// measured 1.7x slower (docs/KERNEL_NOTES.md).
constexpr int FFW = 8;

typedef __attribute__((ext_vector_type(8))) float ff_floatx8;
typedef __attribute__((ext_vector_type(4))) __bf16 ff_bf16x4;

// Swizzle of a V^T row h: as swz(), but rows 8 apart differ too, so the
// transposed staging writes of one key group spread over the banks.
__device__ __forceinline__ int swz_vt(int h, int byte_in_row) {
  return byte_in_row ^ (((h ^ (h >> 3)) & 7) << 4);
}

// LDS of the fused forward: K rows padded to the 16-key strip, V^T rows of
// whole 64-key steps, the head's bias row in fp32. A step's K fragments past
// the last strip are read from the start of the V^T region, which is always
// larger than the 48 rows they can reach; those keys are masked.
static size_t fwd_fused_lds_bytes(int T, bool has_bias, int nbias) {
  return (size_t)cdiv(T, 16) * 16 * 128 + (size_t)64 * cdiv(T, FFK) * FFK * 2 +
         (has_bias ? nbias * sizeof(float) : 0);
}

// Registers are held to what lets two workgroups share a CU (2 * NW waves
// over 4 SIMDs); at T = 300 the LDS request allows two as well.
template <int NW, bool BIAS>
__global__ __launch_bounds__(NW * WAVE_SIZE, (2 * NW + 3) / 4) void
fa_fwd_fused_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v,
    const int* __restrict__ klen_ptr,          // [B] or null
    const unsigned short* __restrict__ bias,   // [N][2C+1] if BIAS
    unsigned short* __restrict__ o, float* __restrict__ lse, int T, int N,
    int win_l, int win_r, int bias_clip, float scale, long sq, long sk,
    long sv) {
  constexpr int H = 64;
  constexpr int NT = NW * WAVE_SIZE;
  constexpr int ROWB = H * 2;
  constexpr int HF = H / 16;
  constexpr int NF = FFK / 16;
  constexpr float LOG2E = 1.4426950408889634f;
  constexpr float LN2 = 0.6931471805599453f;
  const int nbias = 2 * bias_clip + 1;
  const int krows = ((T + 15) >> 4) << 4;
  const int vpitch = ((T + FFK - 1) / FFK) * FFK * 2;  // multiple of 128
  extern __shared__ char smem[];
  char* k_lds = smem;                          // [krows][H] swz
  char* vt_lds = k_lds + krows * ROWB;         // [H][slots] swz_vt
  float* bias_s = (float*)(vt_lds + H * vpitch);  // [nbias] * log2 e if BIAS

  const int n = blockIdx.x;
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int wid = tid / WAVE_SIZE;
  const int lane = tid & 63;
  const int g = lane >> 4;
  const int cl = lane & 15;
  const int klen = klen_ptr ? min(max(klen_ptr[b], 0), T) : T;
  const int kend = ((klen + FFK - 1) / FFK) * FFK;   // keys the steps touch
  const int wl = win_l < 0 ? 0x3fffffff : win_l;
  const int wr = win_r < 0 ? 0x3fffffff : win_r;
  const int nqs = (T + 15) >> 4;

  // Q fragments (B layout of K Q^T): query = cl, h = kk*32 + g*8. Clamped
  // row, never stored for rows >= T. The first strip's loads are in flight
  // across the staging below, the next strip's across the current one.
  bf16x8 qn[2];
  auto load_q = [&](int qs) {
    const long tok = (long)b * T + min(qs * 16 + cl, T - 1);
    const unsigned short* p = q + tok * sq + n * H + g * 8;
    qn[0] = load_bf16x8_bits(p);
    qn[1] = load_bf16x8_bits(p + 32);
  };
  load_q(min(wid, nqs - 1));

  // K: 16 bytes of one key row per thread. Clamped row, select at commit.
  for (int i = tid; i < min(kend, krows) * (ROWB / 16); i += NT) {
    const int key = i >> 3;
    const int c = i & 7;
    ushortx8 kv = *reinterpret_cast<const ushortx8*>(
        k + ((long)b * T + min(key, T - 1)) * sk + n * H + c * 8);
    const bool ok = key < klen;
#pragma unroll
    for (int j = 0; j < 8; ++j) kv[j] = ok ? kv[j] : (unsigned short)0;
    *reinterpret_cast<ushortx8*>(k_lds + key * ROWB + swz(key, c * 16)) = kv;
  }
  // V^T: 8 h of 4 consecutive keys per thread, which are 4 neighbouring
  // slots: one 8-byte write per h.
  for (int i = tid; i < (kend >> 2) * (ROWB / 16); i += NT) {
    const int key0 = (i >> 3) * 4;
    const int c = i & 7;
    ushortx8 vv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      vv[r] = *reinterpret_cast<const ushortx8*>(
          v + ((long)b * T + min(key0 + r, T - 1)) * sv + n * H + c * 8);
    const int slotb =
        ((key0 & ~31) + ((key0 >> 2) & 3) * 8 + ((key0 >> 4) & 1) * 4) * 2;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int h = c * 8 + j;
      ushortx4 w;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        w[r] = key0 + r < klen ? vv[r][j] : (unsigned short)0;
      *reinterpret_cast<ushortx4*>(vt_lds + h * vpitch + swz_vt(h, slotb)) = w;
    }
  }
  if (BIAS) {
    for (int i = tid; i < nbias; i += NT)
      bias_s[i] = bf16_bits_to_float(bias[(long)n * nbias + i]) * LOG2E;
  }
  __syncthreads();

  const float sc2 = scale * LOG2E;
  // Byte offsets in LDS of the first and last entry of the bias row.
  const int bias_lo = (int)((char*)bias_s - smem);
  const int bias_hi = bias_lo + (nbias - 1) * 4;
  for (int qs = wid; qs < nqs; qs += NW) {
    const bf16x8 qf0 = qn[0], qf1 = qn[1];
    if (qs + NW < nqs) load_q(qs + NW);
    const int q0 = qs * 16;
    const int qcol = q0 + cl;

    f32x4 acc_o[HF];
#pragma unroll
    for (int hf = 0; hf < HF; ++hf) acc_o[hf] = {0.f, 0.f, 0.f, 0.f};
    float m_run = NEG_INF;   // the query's running maximum, base-2 logits
    float l_run = 0.f;       // this lane's share of the query's sum

    // Steps of 64 keys with a key some query of the strip can see.
    const int klo = max(q0 - wl, 0);
    const int khi = min(klen, q0 + 16 + wr);     // exclusive
    for (int kb = klo / FFK; kb < (khi + FFK - 1) / FFK; ++kb) {
      const int kbase = kb * FFK;
      // Wave-uniform: no (query, key) of the step is masked.
      const bool full = (kbase + FFK <= klen) & (kbase >= q0 + 15 - wl) &
                        (kbase + FFK - 1 <= q0 + wr);
      float s[NF][4];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = mfma16x16x32_bf16(
            lds_frag(k_lds, kbase + f * 16 + cl, ROWB, (g * 8) * 2), qf0, acc);
        acc = mfma16x16x32_bf16(
            lds_frag(k_lds, kbase + f * 16 + cl, ROWB, (32 + g * 8) * 2), qf1,
            acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) s[f][r] = acc[r];
      }
      // Key of s[f][r] is kbase + g*4 + c with c = f*16 + r.
      if (BIAS) {
        // Byte offset in LDS of the row entry of c = 0; c lowers it.
        const int i0b = bias_lo + (qcol - kbase - g * 4 + bias_clip) * 4;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            int off;  // byte offset of the clamped row entry
            asm("v_med3_i32 %0, %1, %2, %3"
                : "=v"(off)
                : "v"(i0b - (f * 16 + r) * 4), "s"(bias_lo), "v"(bias_hi));
            s[f][r] = fmaf(s[f][r], sc2,
                           *reinterpret_cast<const float*>(smem + off));
          }
        }
      } else {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
#pragma unroll
          for (int r = 0; r < 4; ++r) s[f][r] *= sc2;
        }
      }
      if (!full) {
        // Visible c of this lane: [lo, lo + span).
        const int k0 = kbase + g * 4;
        const int lo = max(qcol - wl, 0) - k0;
        const int span = max(min(klen - 1, qcol + wr) - k0 - lo + 1, 0);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = f * 16 + r;
            s[f][r] = (unsigned)(c - lo) < (unsigned)span ? s[f][r] : NEG_INF;
          }
        }
      }
      float mx = s[0][0];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[f][r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run, mx);
      // A masked logit is NEG_INF; with the subtrahend kept above it both a
      // masked p and the alpha of a so far fully masked query come out 0.
      const float msub = fmaxf(m_new, NEG_INF * 0.1f);
      const float alpha = __builtin_amdgcn_exp2f(m_run - msub);
      m_run = m_new;
      float sum = 0.f;
      ff_floatx8 pf[NF / 2];
#pragma unroll
      for (int f = 0; f < NF; ++f) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(s[f][r] - msub);
          sum += p;
          pf[f >> 1][(f & 1) * 4 + r] = p;
        }
      }
      l_run = l_run * alpha + sum;
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc_o[hf][r] *= alpha;
      }
#pragma unroll
      for (int p2 = 0; p2 < NF / 2; ++p2) {
        const bf16x8 pb = __builtin_convertvector(pf[p2], bf16x8);
        const int slotb = (kbase + p2 * 32 + g * 8) * 2;
#pragma unroll
        for (int hf = 0; hf < HF; ++hf) {
          const int h = hf * 16 + cl;
          union {
            ushortx8 u;
            bf16x8 h;
          } va;
          va.u = *reinterpret_cast<const ushortx8*>(vt_lds + h * vpitch +
                                                    swz_vt(h, slotb));
          acc_o[hf] = mfma16x16x32_bf16(va.h, pb, acc_o[hf]);
        }
      }
    }

    float l = l_run;
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (qcol < T) {
      const float inv_l = l > 0.f ? 1.f / l : 0.f;
      unsigned short* orow = o + (((long)b * T + qcol) * N + n) * H + g * 4;
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) {
        union {
          ff_bf16x4 h;
          ushortx4 u;
        } ov;
        ov.h = __builtin_convertvector(acc_o[hf] * inv_l, ff_bf16x4);
        *reinterpret_cast<ushortx4*>(orow + hf * 16) = ov.u;
      }
      if (g == 0) {
        lse[((long)b * N + n) * T + qcol] =
            l > 0.f ? (m_run + __log2f(l)) * LN2 : NEG_INF;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Backward main
// ---------------------------------------------------------------------------
// 128-key tiles with 8 waves (q-tile staging amortized 2x). H=128
// uses 144KB LDS -> 1 block/CU; staging savings outweigh occupancy.
constexpr int KTB = 128;
constexpr int NWB = 8;
// q-tile 64. A 32-row variant (2 blocks/CU via ~64 KB LDS) measured
// SLOWER (bwd 0.73 -> 0.81 ms at the bench shape): doubled staging
// sync passes outweigh the occupancy gain.
constexpr int QTB = 64;

// Dynamic LDS bytes of fa_bwd_kernel.
static size_t bwd_lds_bytes(int H, bool bias_grad, int nbias) {
  return (size_t)QTB * H * 2 * 2     // q_lds + do_lds
         + (size_t)H * 128 * 2       // qt_lds + dot_lds (128B pitch)
         + (size_t)H * KTB * 2       // kt_lds
         + (size_t)QTB * KTB * 2     // ds_lds
         + (size_t)NWB * 16 * 128    // a_lds (128B pitch)
         + 2 * QTB * sizeof(float) + (bias_grad ? nbias * sizeof(float) : 0);
}

template <int H, bool BIAS_GRAD>
__global__ __launch_bounds__(NWB * WAVE_SIZE) void fa_bwd_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const float* __restrict__ lse,
    const float* __restrict__ delta, const int* __restrict__ klen_ptr,
    const unsigned short* __restrict__ bias,
    const int* __restrict__ qseg, const int* __restrict__ kseg,
    float* __restrict__ dq_acc,
    unsigned short* __restrict__ dk, unsigned short* __restrict__ dv,
    float* __restrict__ dbias, int B, int T, int S, int N, int NKV,
    int win_l, int win_r, int bias_clip, float scale, int chunk, int lc,
    // Token-row strides in elements of q/k/v (reads) and dk/dv (writes).
    long sq, long sk, long sv, long sdk, long sdv) {
  constexpr int ROWB = H * 2;
  constexpr int KH = H / 32;
  constexpr int HF = H / 16;
  const int nbias = 2 * bias_clip + 1;
  extern __shared__ char smem[];
  // qt/dot/a tiles keep a 128-byte row pitch regardless of QTB: the
  // swizzle XORs up to 112 bytes within a row.
  constexpr int TP = 128;
  char* q_lds = smem;                        // [QTB][H] swz
  char* qt_lds = q_lds + QTB * ROWB;         // [H][QTB] swz, pitch TP
  char* do_lds = qt_lds + H * TP;            // [QTB][H] swz
  char* dot_lds = do_lds + QTB * ROWB;       // [H][QTB] swz, pitch TP
  char* kt_lds = dot_lds + H * TP;           // [H][KTB] swz
  char* ds_lds = kt_lds + H * KTB * 2;       // [QTB][KTB] swz
  char* a_lds = ds_lds + QTB * KTB * 2;      // [NWB][16][QTB] swz, pitch TP
  float* lse_s = (float*)(a_lds + NWB * 16 * TP);       // [QTB]
  float* delta_s = lse_s + QTB;                         // [QTB]
  float* dbias_s = delta_s + QTB;                       // [nbias] if BIAS_GRAD

  const int kt = blockIdx.x;
  const int nkv = blockIdx.y;
  const int b = blockIdx.z;
  const int group = N / NKV;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int cl = lane & 15;
  const int klen = klen_ptr ? klen_ptr[b] : S;
  const int kbase = kt * KTB;
  const int k0 = kbase + wid * 16;  // wave's first key

  // Stage K^T once (shared by all heads in the group).
  stage_transposed<H, KTB, NWB * WAVE_SIZE>(
      k + ((long)b * S + kbase) * sk + nkv * H, sk, klen - kbase, kt_lds);

  // K, V fragments (A layout) from global: row = key (cl), k = h.
  bf16x8 kfrag[KH], vfrag[KH];
  {
    int key = k0 + cl;
    bool ok = key < klen;
#pragma unroll
    for (int kk = 0; kk < KH; ++kk) {
      if (ok) {
        const long tok = (long)b * S + key;
        const int col = nkv * H + kk * 32 + g * 8;
        kfrag[kk] = load_bf16x8_bits(k + tok * sk + col);
        vfrag[kk] = load_bf16x8_bits(v + tok * sv + col);
      } else {
        float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        kfrag[kk] = pack_bf16x8(z);
        vfrag[kk] = pack_bf16x8(z);
      }
    }
  }

  // q-tile range for this key tile.
  int qlo = win_r < 0 ? 0 : max(0, kbase - win_r);
  int qhi = win_l < 0 ? T - 1 : min(T - 1, kbase + KTB - 1 + win_l);
  if (chunk > 0) {
    const int kc_lo = kbase / chunk;
    const int kc_hi = (min(kbase + KTB, S) - 1) / chunk;
    qlo = max(qlo, kc_lo * chunk);
    qhi = min(qhi, (kc_hi + lc + 1) * chunk - 1);
    if (qhi < qlo) {
      // No visible queries: dK/dV of this key tile are zero. Write them
      // (group==1 outputs are uninitialized buffers).
      if (group == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + g * 4 + r;
          if (key >= S) continue;
          const long tok = (long)b * S + key;
#pragma unroll
          for (int hf = 0; hf < HF; ++hf) {
            dk[tok * sdk + nkv * H + hf * 16 + cl] = float_to_bf16_bits(0.f);
            dv[tok * sdv + nkv * H + hf * 16 + cl] = float_to_bf16_bits(0.f);
          }
        }
      }
      return;
    }
  }
  const int qt_lo = qlo / QTB, qt_hi = max(qhi, 0) / QTB;

  for (int head = 0; head < group; ++head) {
    const int n = nkv * group + head;

    f32x4 acc_dk[HF], acc_dv[HF];
#pragma unroll
    for (int hf = 0; hf < HF; ++hf) {
      acc_dk[hf] = {0.f, 0.f, 0.f, 0.f};
      acc_dv[hf] = {0.f, 0.f, 0.f, 0.f};
    }
    if (BIAS_GRAD) {
      for (int i = threadIdx.x; i < nbias; i += NWB * WAVE_SIZE)
        dbias_s[i] = 0.f;
    }

    for (int qt2 = qt_lo; qt2 <= qt_hi; ++qt2) {
      const int qb = qt2 * QTB;
      __syncthreads();
      stage_regular<H, QTB, NWB * WAVE_SIZE>(
          q + ((long)b * T + qb) * sq + n * H, sq, T - qb, q_lds);
      stage_regular<H, QTB, NWB * WAVE_SIZE>(
          dout + (((long)b * T + qb) * N + n) * H, (long)N * H, T - qb,
          do_lds);
      stage_transposed<H, QTB, NWB * WAVE_SIZE, TP>(
          q + ((long)b * T + qb) * sq + n * H, sq, T - qb, qt_lds);
      stage_transposed<H, QTB, NWB * WAVE_SIZE, TP>(
          dout + (((long)b * T + qb) * N + n) * H, (long)N * H, T - qb,
          dot_lds);
      for (int i = threadIdx.x; i < QTB; i += NWB * WAVE_SIZE) {
        int qrow = qb + i;
        lse_s[i] = qrow < T ? lse[((long)b * N + n) * T + qrow] : NEG_INF;
        delta_s[i] = qrow < T ? delta[((long)b * N + n) * T + qrow] : 0.f;
      }
      __syncthreads();

      // Per-lane chunk windows for this q-tile's 4 q columns.
      constexpr int NQ = QTB / 16;
      int bw_lo[NQ], bw_hi[NQ];
#pragma unroll
      for (int nf = 0; nf < NQ; ++nf) {
        if (chunk > 0) {
          const int qc = (qb + nf * 16 + cl) / chunk;
          bw_lo[nf] = (qc - lc) * chunk;
          bw_hi[nf] = (qc + 1) * chunk;
        } else {
          bw_lo[nf] = 0;
          bw_hi[nf] = 0x7fffffff;
        }
      }

      // S^T strip: rows = 16 keys (this wave), cols = QTB queries.
      float pt[NQ][4];  // P^T
      float dlg[NQ][4];  // dLogits
#pragma unroll
      for (int nf = 0; nf < NQ; ++nf) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KH; ++kk) {
          bf16x8 bq =
              lds_frag(q_lds, nf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2);
          acc = mfma16x16x32_bf16(kfrag[kk], bq, acc);
        }
        const int qcol = qb + nf * 16 + cl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + g * 4 + r;
          float val = acc[r] * scale;
          if (bias) {
            int d = qcol - key;
            d = d < -bias_clip ? -bias_clip : (d > bias_clip ? bias_clip : d);
            val += bf16_bits_to_float(bias[(long)n * nbias + d + bias_clip]);
          }
          bool vis = visible(qcol, key, klen, win_l, win_r, bw_lo[nf],
                             bw_hi[nf]) && qcol < T;
          if (vis && qseg &&
              qseg[(long)b * T + qcol] != kseg[(long)b * S + key])
            vis = false;
          float l = lse_s[nf * 16 + cl];
          pt[nf][r] =
              (vis && l > NEG_INF * 0.5f) ? __expf(val - l) : 0.f;
        }
      }

      // P^T -> a_lds; dV += P^T @ dO (B from dOt).
      char* aw = a_lds + wid * 16 * TP;
#pragma unroll
      for (int nf = 0; nf < NQ; ++nf) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = g * 4 + r;
          int col = nf * 16 + cl;
          *reinterpret_cast<unsigned short*>(
              aw + row * TP + swz(row, col * 2)) =
              float_to_bf16_bits(pt[nf][r]);
        }
      }
#pragma unroll
      for (int kk2 = 0; kk2 < QTB / 32; ++kk2) {
        bf16x8 pa = lds_frag(aw, cl, TP, (kk2 * 32 + g * 8) * 2);
#pragma unroll
        for (int hf = 0; hf < HF; ++hf) {
          bf16x8 bd =
              lds_frag(dot_lds, hf * 16 + cl, TP, (kk2 * 32 + g * 8) * 2);
          acc_dv[hf] = mfma16x16x32_bf16(pa, bd, acc_dv[hf]);
        }
      }

      // dP^T = V @ dO^T (B from do_lds rows).
#pragma unroll
      for (int nf = 0; nf < NQ; ++nf) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < KH; ++kk) {
          bf16x8 bd =
              lds_frag(do_lds, nf * 16 + cl, ROWB, (kk * 32 + g * 8) * 2);
          acc = mfma16x16x32_bf16(vfrag[kk], bd, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float dlogits = pt[nf][r] * (acc[r] - delta_s[nf * 16 + cl]);
          dlg[nf][r] = dlogits;
        }
      }

      // dS^T (scaled, bf16) -> a_lds (overwrite); dK += dS^T @ Q (B=Qt).
#pragma unroll
      for (int nf = 0; nf < NQ; ++nf) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int row = g * 4 + r;
          int col = nf * 16 + cl;
          *reinterpret_cast<unsigned short*>(
              aw + row * TP + swz(row, col * 2)) =
              float_to_bf16_bits(dlg[nf][r] * scale);
        }
      }
#pragma unroll
      for (int kk2 = 0; kk2 < QTB / 32; ++kk2) {
        bf16x8 da = lds_frag(aw, cl, TP, (kk2 * 32 + g * 8) * 2);
#pragma unroll
        for (int hf = 0; hf < HF; ++hf) {
          bf16x8 bq =
              lds_frag(qt_lds, hf * 16 + cl, TP, (kk2 * 32 + g * 8) * 2);
          acc_dk[hf] = mfma16x16x32_bf16(da, bq, acc_dk[hf]);
        }
      }

      // Full dS tile to LDS (transposed store: ds_lds[q][key]) for dQ.
#pragma unroll
      for (int nf = 0; nf < NQ; ++nf) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          int qrow = nf * 16 + cl;
          int key = wid * 16 + g * 4 + r;
          *reinterpret_cast<unsigned short*>(
              ds_lds + qrow * (KTB * 2) + swz(qrow, key * 2)) =
              float_to_bf16_bits(dlg[nf][r] * scale);
        }
      }
      __syncthreads();

      // dQ strips: rows q = qb + dw*16 + .. (A from ds_lds), B = K from
      // kt_lds; atomic-accumulate fp32. Only QTB/16 strips exist, so with
      // NWB > QTB/16 the extra waves skip this phase.
      if (wid < QTB / 16) {
        f32x4 acc_dq[HF];
#pragma unroll
        for (int hf = 0; hf < HF; ++hf) acc_dq[hf] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk2 = 0; kk2 < KTB / 32; ++kk2) {
          bf16x8 da = lds_frag(ds_lds, wid * 16 + cl, KTB * 2,
                               (kk2 * 32 + g * 8) * 2);
#pragma unroll
          for (int hf = 0; hf < HF; ++hf) {
            bf16x8 bk = lds_frag(kt_lds, hf * 16 + cl, KTB * 2,
                                 (kk2 * 32 + g * 8) * 2);
            acc_dq[hf] = mfma16x16x32_bf16(da, bk, acc_dq[hf]);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int qrow = qb + wid * 16 + g * 4 + r;
          if (qrow >= T) continue;
#pragma unroll
          for (int hf = 0; hf < HF; ++hf) {
            if (acc_dq[hf][r] != 0.f) {
              atomicAdd(
                  dq_acc + (((long)b * T + qrow) * N + n) * H + hf * 16 +
                      cl,
                  acc_dq[hf][r]);
            }
          }
        }
      } else if (BIAS_GRAD && wid >= QTB / 16) {
        // Bias grad via per-diagonal sums over the dS tile in ds_lds
        // (entries hold dlogits*scale; invisible positions are exact
        // zeros). One lane per diagonal d = qcol - key: elements
        // (qrow, key) with qb + qrow - kbase - key == d. Runs on the
        // waves otherwise idle during the dQ phase.
        const int ndiag = QTB + KTB - 1;
        const int lane_global = (wid - QTB / 16) * WAVE_SIZE + lane;
        const int nworkers = (NWB - QTB / 16) * WAVE_SIZE;
        const float inv_scale = 1.f / scale;
        for (int di = lane_global; di < ndiag; di += nworkers) {
          // diagonal offset within the tile: qrow - key = di - (KTB-1)
          const int doff = di - (KTB - 1);
          float sum = 0.f;
          const int q_lo = max(0, doff);
          const int q_hi = min(QTB - 1, KTB - 1 + doff);
          for (int qrow = q_lo; qrow <= q_hi; ++qrow) {
            const int key = qrow - doff;
            sum += bf16_bits_to_float(*reinterpret_cast<unsigned short*>(
                ds_lds + qrow * (KTB * 2) + swz(qrow, key * 2)));
          }
          if (sum != 0.f) {
            int d = (qb + doff) - kbase;  // global q - k distance
            d = d < -bias_clip ? -bias_clip
                               : (d > bias_clip ? bias_clip : d);
            atomicAdd(&dbias_s[d + bias_clip], sum * inv_scale);
          }
        }
      }
    }

    // Flush dbias for this head.
    if (BIAS_GRAD) {
      __syncthreads();
      for (int i = threadIdx.x; i < nbias; i += NWB * WAVE_SIZE) {
        if (dbias_s[i] != 0.f)
          atomicAdd(dbias + (long)n * nbias + i, dbias_s[i]);
      }
    }

    // dK/dV for this head's contribution: with GQA we accumulate across
    // heads; write after the head loop. To keep single-write semantics we
    // only write on the last head, so keep accumulating into global via
    // registers: here we add to global bf16 once per head via fp32 staging
    // in registers across heads instead. Simpler: accumulate across heads
    // in registers by NOT resetting acc_dk/acc_dv — but they are reset per
    // head above; so write-accumulate here:
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = k0 + g * 4 + r;
      if (key >= S) continue;  // acc is 0 for klen<=key<S: writes zeros
      const long tok = (long)b * S + key;
      // fp32 GQA buffers are always dense.
      const long off = (tok * NKV + nkv) * H;
#pragma unroll
      for (int hf = 0; hf < HF; ++hf) {
        if (group == 1) {
          dk[tok * sdk + nkv * H + hf * 16 + cl] =
              float_to_bf16_bits(acc_dk[hf][r]);
          dv[tok * sdv + nkv * H + hf * 16 + cl] =
              float_to_bf16_bits(acc_dv[hf][r]);
        } else {
          // GQA: multiple heads accumulate; use fp32 atomics into dq_acc?
          // dk/dv are bf16 outputs; for group>1 the host passes fp32
          // buffers aliased via dk/dv pointers being fp32. Handled on the
          // host by allocating fp32 and a separate cast. Here: atomicAdd.
          atomicAdd(reinterpret_cast<float*>(dk) + off + hf * 16 + cl,
                    acc_dk[hf][r]);
          atomicAdd(reinterpret_cast<float*>(dv) + off + hf * 16 + cl,
                    acc_dv[hf][r]);
        }
      }
    }
    __syncthreads();
  }
}

// dq_acc fp32 dense [rows, NH] -> bf16 dq with token-row stride sdq: the
// `.to(bf16)` cast of the dense path, written into a view of a packed
// dQKV buffer. One 8-wide vector per thread; grid.y walks rows.
__global__ void fa_dq_cast(const float* __restrict__ dq_acc,
                           unsigned short* __restrict__ dq, long rows,
                           int nh_vec, long sdq) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nh_vec) return;
  for (long r = blockIdx.y; r < rows; r += gridDim.y) {
    const float* src = dq_acc + (r * nh_vec + c) * 8;
    floatx4 a = *reinterpret_cast<const floatx4*>(src);
    floatx4 b = *reinterpret_cast<const floatx4*>(src + 4);
    ushortx8 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      o[j] = float_to_bf16_bits(a[j]);
      o[4 + j] = float_to_bf16_bits(b[j]);
    }
    *reinterpret_cast<ushortx8*>(dq + r * sdq + (long)c * 8) = o;
  }
}

// ---------------------------------------------------------------------------
// Backward, fused route: one workgroup per (head, batch), self-attention
// with N == NKV and T == S <= FUSED_MAX_S.
//
// Keys across waves: strip s (16 keys) belongs to wave s % NWF, which keeps
// the strip's K/V fragments and dK^T/dV^T accumulators in registers for the
// whole kernel. The q-tiles are walked once.
//
// S = Q K^T and dP = dO V^T: in the MFMA C layout a lane holds one key (its
// column cl) and queries g*4 + r of each 16-query fragment. The two query
// fragments of a 32-row tile are the 8 k-slots of one contraction step, slot
// g*8 + hs*4 + r <-> query hs*16 + g*4 + r, so P and dS, converted in pairs,
// are the B operands of dV^T = dO^T P and dK^T = Q^T dS straight from
// registers; Q^T and dO^T are staged in that slot order. lse and delta are
// one 16-byte broadcast read per fragment. Logits are base-2 (scale, the
// bias row and the staged lse carry log2 e). A lane ends with 4 consecutive
// h of one key: 8-byte dK/dV stores.
//
// Per tile every wave also writes its dS strips into one [FQTB][S_pad] LDS
// tile (that contraction crosses waves); after a barrier dQ^T = K^T dS^T
// is computed over the whole key range (K^T resident in LDS), rounded once
// and stored as bf16 straight into dq. delta = rowsum(dO * O) is reduced
// while the dO tile is staged. Global loads for tile i+1 are issued into
// registers before the MFMAs of tile i. The bias-gradient diagonals are
// summed in LDS by one owning thread each (fixed order, no atomics) and
// leave as one fp32 row per workgroup for fa_dbias_reduce.
// ---------------------------------------------------------------------------
// 8 waves x 3 strips, 32-row q-tiles. Of the four configurations measured
// (10x2 and 8x3 waves x strips, 64- and 32-row q-tiles) the only one that
// keeps its accumulators out of scratch, and the fastest at the Conformer
// shape (docs/KERNEL_NOTES.md).
constexpr int FQTB = 32;                       // q rows per tile
constexpr int NWF = 8;                         // waves
constexpr int SPW = 3;                         // key strips per wave
constexpr int FUSED_MAX_S = NWF * SPW * 16;

// Row pitch in bytes of the fused backward's dS tile.
constexpr int FUSED_DS_PITCH = FUSED_MAX_S * 2 + 16;

// Dynamic LDS bytes of fa_bwd_fused_kernel (H == 64).
static size_t fused_lds_bytes(bool has_bias, bool bias_grad, int nbias) {
  constexpr int H = 64;
  constexpr int SP = FUSED_MAX_S;
  return (size_t)FQTB * H * 2 * 2          // q_lds + do_lds
         + (size_t)H * FQTB * 2 * 2        // qt_lds + dot_lds
         + (size_t)H * SP * 2              // kt_lds
         + (size_t)FQTB * FUSED_DS_PITCH   // ds_lds
         + 2 * FQTB * sizeof(float)        // lse_s + delta_s
         + (has_bias ? nbias : 1) * sizeof(float)
         + (bias_grad ? (2 * SP + FQTB) * sizeof(float) : 0);
}

// Q^T and dO^T tiles: row h holds the tile's 32 queries in the k-slot order
// of the MFMA that contracts over them, slot g*8 + hs*4 + r <-> query
// hs*16 + g*4 + r, so an A fragment is one 16-byte read and the rows need
// no padding (64 bytes). The four 16-byte granules of a row are exchanged
// by h/8: a wave's fragment read still covers 1 KB exactly once, and the
// staging writes of one query row spread over four bank groups.
__device__ __forceinline__ int qslot_byte(int h, int q) {
  const int slot = ((q >> 2) & 3) * 8 + (q >> 4) * 4 + (q & 3);
  return (slot * 2) ^ (((h >> 3) & 3) << 4);
}

// One 16-byte fragment read at an LDS address.
__device__ __forceinline__ bf16x8 frag_at(const char* p) {
  union {
    ushortx8 u;
    bf16x8 h;
  } cv;
  cv.u = *reinterpret_cast<const ushortx8*>(p);
  return cv.h;
}

template <int H, bool BIAS_GRAD>
__global__ __launch_bounds__(NWF * WAVE_SIZE) void fa_bwd_fused_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const unsigned short* __restrict__ o,
    const float* __restrict__ lse, const int* __restrict__ klen_ptr,
    const unsigned short* __restrict__ bias,
    unsigned short* __restrict__ dq, unsigned short* __restrict__ dk,
    unsigned short* __restrict__ dv,
    float* __restrict__ dbias_part,            // [B][N][nbias] if BIAS_GRAD
    int T, int N, int win_l, int win_r, int bias_clip, float scale,
    long sq, long sk, long sv, long sdq, long sdk, long sdv) {
  static_assert(H == 64, "fused backward is built for H == 64");
  constexpr int NT = NWF * WAVE_SIZE;
  constexpr int SP = FUSED_MAX_S;  // padded key count
  constexpr int ROWB = H * 2;
  constexpr int KH = H / 32;
  constexpr int HF = H / 16;
  constexpr int NQ = FQTB / 16;
  constexpr int TP = FQTB * 2;   // pitch of the [..][FQTB] tiles
  constexpr int DSP = SP * 2;    // pitch of the K^T tile
  // Pitch of the dS tile: rows skewed by 16 bytes instead of swizzled, so a
  // lane's dS writes are constant offsets from one address.
  constexpr int DSQ = FUSED_DS_PITCH;
  constexpr int NDACC = 2 * SP + FQTB;
  constexpr int STG = FQTB * (ROWB / 16);       // staging threads (16B each)
  constexpr float LOG2E = 1.4426950408889634f;
  static_assert(SP % 64 == 0, "[..][SP] rows must span whole swizzle blocks");
  static_assert((NWF * SPW) % 2 == 0, "dQ contracts over pairs of strips");
  // A q-tile is one 32-deep contraction step of the dV and dK MFMAs.
  static_assert(FQTB == 32 && STG <= NT, "q-tile shape");
  // dQ^T output tiles (FQTB/16 x H/16) over the waves; a wave's tiles share
  // their dS B-fragment.
  constexpr int NTILE = NQ * HF;
  constexpr int TPW = (NTILE + NWF - 1) / NWF;
  static_assert(HF % TPW == 0, "a wave's dQ tiles must share one q strip");

  const int nbias = 2 * bias_clip + 1;
  extern __shared__ char smem[];
  char* q_lds = smem;                        // [FQTB][H] swz
  char* do_lds = q_lds + FQTB * ROWB;         // [FQTB][H] swz
  char* qt_lds = do_lds + FQTB * ROWB;        // [H][slot], qslot_byte
  char* dot_lds = qt_lds + H * TP;           // [H][slot], qslot_byte
  char* kt_lds = dot_lds + H * TP;           // [H][SP] swz
  char* ds_lds = kt_lds + H * DSP;           // [FQTB][SP], pitch DSQ
  float* lse_s = (float*)(ds_lds + FQTB * DSQ);          // [FQTB], * log2 e
  float* delta_s = lse_s + FQTB;                         // [FQTB]
  float* bias_s = delta_s + FQTB;   // [nbias] * log2 e; one zero without bias
  // Unclipped per-diagonal sums, slot = (q - key) + SP - 1.
  float* dacc = bias_s + (bias ? nbias : 1);            // [NDACC] if BIAS_GRAD
  const int bias_top = bias ? nbias - 1 : 0;

  const int n = blockIdx.x;
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int wid = tid / WAVE_SIZE;
  const int lane = tid & 63;
  const int g = lane >> 4;
  const int cl = lane & 15;
  const int S = T;
  const int klen = klen_ptr ? min(max(klen_ptr[b], 0), S) : S;
  const int nact = (klen + 15) / 16;          // strips with a visible key
  const int kact = ((nact + 1) & ~1) * 16;    // dQ contraction length
  const int nqt = (T + FQTB - 1) / FQTB;
  // Window half-widths with "no limit" folded in (T <= SP keeps the sums
  // far from overflow).
  const int wl = win_l < 0 ? 0x3fffffff : win_l;
  const int wr = win_r < 0 ? 0x3fffffff : win_r;
  // Logits are kept in the base-2 domain: scale, the bias row and lse carry
  // log2 e, and p is one v_exp_f32 of a difference.
  const float sc2 = scale * LOG2E;

  // Staging role of this thread: 16 bytes of one q/dO/O row; the last FQTB
  // threads carry lse.
  const int srow = tid / (ROWB / 16);
  const int sc = tid % (ROWB / 16);
  const bool stager = tid < STG;
  const int lrow = tid - (NT - FQTB);
  // Byte of query srow in the rows h = sc*8 .. sc*8 + 7 of Q^T and dO^T.
  const int sslot = qslot_byte(sc * 8, srow & (FQTB - 1));
  // Per-lane LDS offsets of the strip phase; everything else is a constant.
  // fq: fragment (row cl, h = kk*32 + g*8) of a 16-row block of q or dO.
  // ft: fragment (row cl, slots g*8 ..) of an even / odd 16-row block of Q^T
  // or dO^T. dsw: dS tile entry (row g*4, key cl of the wave's first strip).
  const int fq[KH] = {cl * ROWB + swz(cl, g * 16),
                      cl * ROWB + swz(cl, 64 + g * 16)};
  const int ft[2] = {cl * TP + ((g ^ (cl >> 3)) << 4),
                     cl * TP + ((g ^ (2 + (cl >> 3))) << 4)};
  char* dsw = ds_lds + g * 4 * DSQ + (wid * 16 + cl) * 2;
  ushortx8 pq, pdo, po;
  float plse = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) pq[j] = pdo[j] = po[j] = 0;

  // Clamped row, select at commit time: the loads stay unconditional so
  // they can be in flight across the MFMAs of the previous tile.
  auto prefetch = [&](int qb) {
    if (stager) {
      const long tok = (long)b * T + min(qb + srow, T - 1);
      pq = *reinterpret_cast<const ushortx8*>(q + tok * sq + n * H + sc * 8);
      pdo = *reinterpret_cast<const ushortx8*>(dout + (tok * N + n) * H +
                                               sc * 8);
      po = *reinterpret_cast<const ushortx8*>(o + (tok * N + n) * H + sc * 8);
    }
    if (lrow >= 0)
      plse = lse[((long)b * N + n) * T + min(qb + lrow, T - 1)];
  };
  prefetch(0);

  // One-time LDS setup: dS tile zeroed (columns of the odd padding strip
  // are read by dQ but never written), bias row, diagonal sums, K^T.
  for (int i = tid; i < FQTB * DSQ / 16; i += NT) {
    ushortx8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = 0;
    *reinterpret_cast<ushortx8*>(ds_lds + i * 16) = z;
  }
  if (bias) {
    for (int i = tid; i < nbias; i += NT)
      bias_s[i] = bf16_bits_to_float(bias[(long)n * nbias + i]) * LOG2E;
  } else if (tid == 0) {
    bias_s[0] = 0.f;
  }
  if (BIAS_GRAD) {
    for (int i = tid; i < NDACC; i += NT) dacc[i] = 0.f;
  }
  for (int i = tid; i < kact * (H / 8); i += NT) {
    const int key = i / (H / 8);
    const int h0 = (i % (H / 8)) * 8;
    ushortx8 kv = *reinterpret_cast<const ushortx8*>(
        k + ((long)b * S + min(key, klen - 1)) * sk + n * H + h0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int h = h0 + j;
      *reinterpret_cast<unsigned short*>(kt_lds + h * DSP + swz(h, key * 2)) =
          key < klen ? kv[j] : (unsigned short)0;
    }
  }

  // K, V fragments and accumulators of this wave's strips. A fragment holds
  // key cl, h = kk*32 + g*8 ..: the B operand of S = Q K^T and dP = dO V^T.
  // dK^T and dV^T accumulate as [h][key].
  bf16x8 kfrag[SPW][KH], vfrag[SPW][KH];
  f32x4 acc_dk[SPW][HF], acc_dv[SPW][HF];
#pragma unroll
  for (int si = 0; si < SPW; ++si) {
    const int key = (wid + si * NWF) * 16 + cl;
    const bool ok = key < klen;
#pragma unroll
    for (int kk = 0; kk < KH; ++kk) {
      if (ok) {
        const long tok = (long)b * S + key;
        const int col = n * H + kk * 32 + g * 8;
        kfrag[si][kk] = load_bf16x8_bits(k + tok * sk + col);
        vfrag[si][kk] = load_bf16x8_bits(v + tok * sv + col);
      } else {
        float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        kfrag[si][kk] = pack_bf16x8(z);
        vfrag[si][kk] = pack_bf16x8(z);
      }
    }
#pragma unroll
    for (int hf = 0; hf < HF; ++hf) {
      acc_dk[si][hf] = {0.f, 0.f, 0.f, 0.f};
      acc_dv[si][hf] = {0.f, 0.f, 0.f, 0.f};
    }
  }

  for (int qt = 0; qt < nqt; ++qt) {
    const int qb = qt * FQTB;
    // No barrier here: q/dO/lse/delta were last read before the barrier
    // that ends the strip phase, and the dS tile and dacc are next written
    // after the barrier below.
    if (stager) {
      const bool ok = qb + srow < T;
      float part = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        pq[j] = ok ? pq[j] : (unsigned short)0;
        pdo[j] = ok ? pdo[j] : (unsigned short)0;
        part += bf16_bits_to_float(pdo[j]) * bf16_bits_to_float(po[j]);
      }
      *reinterpret_cast<ushortx8*>(q_lds + srow * ROWB + swz(srow, sc * 16)) =
          pq;
      *reinterpret_cast<ushortx8*>(do_lds + srow * ROWB +
                                   swz(srow, sc * 16)) = pdo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int off = (sc * 8 + j) * TP + sslot;
        *reinterpret_cast<unsigned short*>(qt_lds + off) = pq[j];
        *reinterpret_cast<unsigned short*>(dot_lds + off) = pdo[j];
      }
      // delta: the row's ROWB/16 = 8 threads are neighbouring lanes.
#pragma unroll
      for (int off = 1; off < ROWB / 16; off <<= 1)
        part += __shfl_xor(part, off);
      if (sc == 0) delta_s[srow] = part;
    }
    // Rows past T and rows without a visible key get a large positive lse:
    // every p of the row is exp2 of a hugely negative number, an exact 0.
    if (lrow >= 0)
      lse_s[lrow] = (qb + lrow < T) & (plse > NEG_INF * 0.5f) ? plse * LOG2E
                                                             : -NEG_INF;
    __syncthreads();
    if (qt + 1 < nqt) prefetch(qb + FQTB);

    if (wid < nact) {   // wave-uniform: the wave has a strip with a key
      // The tile's operands are read again for each strip: held across the
      // wave's three strips (64 registers, or 32 for q and dO alone) they
      // push the accumulators into scratch (docs/KERNEL_NOTES.md).
      const int qbase = qb + g * 4;   // query of tile row c = 0 of this lane

#pragma unroll
      for (int si = 0; si < SPW; ++si) {
        const int strip = wid + si * NWF;
        if (strip >= nact) continue;   // wave-uniform
        // A lane holds key cl of the strip and tile rows c = nf*16 + r
        // (queries qbase + c). Visible rows of the key: [lo, lo + span).
        const int key = strip * 16 + cl;
        const int lo = max(key - wr, 0) - qbase;
        const int hi = min(key + wl, SP + FQTB) - qbase;
        const int span = key < klen ? max(hi - lo + 1, 0) : 0;
        const int i0 = qbase - key + bias_clip;   // bias row entry of c = 0
        ff_floatx8 pf, dsf;   // P and dS in slot order j = nf*4 + r
#pragma unroll
        for (int nf = 0; nf < NQ; ++nf) {
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};    // S = Q K^T
          f32x4 accd = {0.f, 0.f, 0.f, 0.f};   // dP = dO V^T
#pragma unroll
          for (int kk = 0; kk < KH; ++kk) {
            acc = mfma16x16x32_bf16(
                frag_at(q_lds + nf * 16 * ROWB + fq[kk]), kfrag[si][kk], acc);
            accd = mfma16x16x32_bf16(
                frag_at(do_lds + nf * 16 * ROWB + fq[kk]), vfrag[si][kk],
                accd);
          }
          const f32x4 l2 =
              *reinterpret_cast<const f32x4*>(lse_s + nf * 16 + g * 4);
          const f32x4 dl =
              *reinterpret_cast<const f32x4*>(delta_s + nf * 16 + g * 4);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = nf * 16 + r;
            // Without a bias the row is one zero: no per-logit branch.
            const int i = min(max(i0 + c, 0), bias_top);
            float val = fmaf(acc[r], sc2, bias_s[i]);
            val = (unsigned)(c - lo) < (unsigned)span ? val : NEG_INF;
            const float p = __builtin_amdgcn_exp2f(val - l2[r]);
            pf[nf * 4 + r] = p;
            dsf[nf * 4 + r] = p * (accd[r] - dl[r]) * scale;
          }
        }
        // dV^T += dO^T P and dK^T += Q^T dS with P and dS as B operands
        // straight from registers.
        const bf16x8 pb = __builtin_convertvector(pf, bf16x8);
        union {
          bf16x8 h;
          ushortx8 u;
        } db;
        db.h = __builtin_convertvector(dsf, bf16x8);
#pragma unroll
        for (int hf = 0; hf < HF; ++hf) {
          acc_dv[si][hf] = mfma16x16x32_bf16(
              frag_at(dot_lds + hf * 16 * TP + ft[hf & 1]), pb,
              acc_dv[si][hf]);
          acc_dk[si][hf] = mfma16x16x32_bf16(
              frag_at(qt_lds + hf * 16 * TP + ft[hf & 1]), db.h,
              acc_dk[si][hf]);
        }
        // dS (scaled, bf16) into the shared [q][key] tile for dQ: constant
        // offsets from one address per lane.
#pragma unroll
        for (int nf = 0; nf < NQ; ++nf) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            *reinterpret_cast<unsigned short*>(
                dsw + (nf * 16 + r) * DSQ + si * NWF * 32) = db.u[nf * 4 + r];
          }
        }
      }
    }
    __syncthreads();

    // dQ^T tiles: A = K^T rows (h), B = dS rows (q), contraction over the
    // active keys. A lane ends with 4 consecutive h of one q row.
    if (wid * TPW < NTILE) {
      const int qs = (wid * TPW) / HF;
      const int hf0 = (wid * TPW) % HF;
      f32x4 acc_dq[TPW];
#pragma unroll
      for (int i = 0; i < TPW; ++i) acc_dq[i] = {0.f, 0.f, 0.f, 0.f};
      for (int kk2 = 0; kk2 < kact / 32; ++kk2) {
        bf16x8 bs = frag_at(ds_lds + (qs * 16 + cl) * DSQ +
                            (kk2 * 32 + g * 8) * 2);
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
          bf16x8 ak = lds_frag(kt_lds, (hf0 + i) * 16 + cl, DSP,
                               (kk2 * 32 + g * 8) * 2);
          acc_dq[i] = mfma16x16x32_bf16(ak, bs, acc_dq[i]);
        }
      }
      const int qrow = qb + qs * 16 + cl;
      if (qrow < T) {
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
          ushortx4 ov;
#pragma unroll
          for (int r = 0; r < 4; ++r) ov[r] = float_to_bf16_bits(acc_dq[i][r]);
          *reinterpret_cast<ushortx4*>(dq + ((long)b * T + qrow) * sdq +
                                       n * H + (hf0 + i) * 16 + g * 4) = ov;
        }
      }
    }
    if (BIAS_GRAD) {
      // One thread per diagonal of the dS tile (entries hold
      // dlogits*scale; invisible positions are exact zeros), handed out
      // from the last thread down so the waves without a dQ tile go first.
      // A slot of dacc has one owner per tile: plain read-modify-write.
      const int ndiag = FQTB + kact - 1;
      for (int di = NT - 1 - tid; di < ndiag; di += NT) {
        const int doff = di - (kact - 1);   // qrow - key within the tile
        const int q_lo = max(0, doff);
        const int q_hi = min(FQTB - 1, kact - 1 + doff);
        float sum = 0.f;
        for (int qrow = q_lo; qrow <= q_hi; ++qrow) {
          const int key = qrow - doff;
          sum += bf16_bits_to_float(*reinterpret_cast<unsigned short*>(
              ds_lds + qrow * DSQ + key * 2));
        }
        dacc[qb + doff + SP - 1] += sum;
      }
    }
  }

  // dK/dV: every key row < S of this head is written once, 4 consecutive h
  // of the lane's key per store; strips past klen carry zero accumulators.
#pragma unroll
  for (int si = 0; si < SPW; ++si) {
    const int key = (wid + si * NWF) * 16 + cl;
    if (key >= S) continue;
    const long tok = (long)b * S + key;
    unsigned short* dkp = dk + tok * sdk + n * H + g * 4;
    unsigned short* dvp = dv + tok * sdv + n * H + g * 4;
#pragma unroll
    for (int hf = 0; hf < HF; ++hf) {
      union {
        ff_bf16x4 h;
        ushortx4 u;
      } ok, ov;
      ok.h = __builtin_convertvector(acc_dk[si][hf], ff_bf16x4);
      ov.h = __builtin_convertvector(acc_dv[si][hf], ff_bf16x4);
      *reinterpret_cast<ushortx4*>(dkp + hf * 16) = ok.u;
      *reinterpret_cast<ushortx4*>(dvp + hf * 16) = ov.u;
    }
  }

  if (BIAS_GRAD) {
    // Clip merge in fixed order: wave w sums the dacc slots that clamp to
    // bias slot i = w, w + NWF, ... (one slot inside, a range at the ends).
    __syncthreads();
    const float inv_scale = 1.f / scale;
    for (int i = wid; i < nbias; i += NWF) {
      int lo = i == 0 ? 0 : i - bias_clip + SP - 1;
      int hi = i == nbias - 1 ? NDACC - 1 : i - bias_clip + SP - 1;
      lo = max(lo, 0);
      hi = min(hi, NDACC - 1);
      float sum = 0.f;
      for (int j = lo + lane; j <= hi; j += WAVE_SIZE) sum += dacc[j];
      sum = wave_reduce_sum(sum);
      if (lane == 0)
        dbias_part[((long)b * N + n) * nbias + i] = sum * inv_scale;
    }
  }
}

// dbias[c] = sum over b of part[b][c], c over N * nbias, in fixed order.
constexpr int kDbSlices = 16;
__global__ __launch_bounds__(WAVE_SIZE * kDbSlices) void fa_dbias_reduce(
    const float* __restrict__ part, float* __restrict__ dbias, int B,
    int D) {
  __shared__ float red[kDbSlices][WAVE_SIZE];
  const int lane = threadIdx.x & 63;
  const int slice = threadIdx.x / WAVE_SIZE;
  const int c = blockIdx.x * WAVE_SIZE + lane;
  float s = 0.f;
  if (c < D) {
    for (int p = slice; p < B; p += kDbSlices) s += part[(long)p * D + c];
  }
  red[slice][lane] = s;
  __syncthreads();
  if (slice == 0 && c < D) {
    float t = 0.f;
#pragma unroll
    for (int p = 0; p < kDbSlices; ++p) t += red[p][lane];
    dbias[c] = t;
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------
// Largest dynamic LDS request a launch on the current device accepts.
static size_t fa_lds_limit_bytes() {
  int dev = 0, limit = 0;
  LV_CHECK_HIP(hipGetDevice(&dev));
  LV_CHECK_HIP(hipDeviceGetAttribute(
      &limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  return (size_t)limit;
}

// One launch function per kernel, and a dispatch from the run-time values to
// its template arguments; the kernel arguments pass through.
template <int H, int KTF, bool SEG, class... Args>
static void fa_fwd_launch(dim3 grid, hipStream_t stream, Args... args) {
  const size_t shmem =
      (size_t)KTF * H * 2 + (size_t)H * KTF * 2 + FWD_NW * 16 * KTF * 2;
  hipLaunchKernelGGL((fa_fwd_kernel<H, KTF, SEG>), grid, dim3(FWD_BLOCK),
                     shmem, stream, args...);
}

template <int H, int KTF, class... Args>
static void fa_fwd_dispatch_seg(bool seg, Args... args) {
  if (seg) {
    fa_fwd_launch<H, KTF, true>(args...);
  } else {
    fa_fwd_launch<H, KTF, false>(args...);
  }
}

template <class... Args>
static void fa_fwd_dispatch(int H, int ktf, bool seg, Args... args) {
  if (H == 64 && ktf == 128) {
    fa_fwd_dispatch_seg<64, 128>(seg, args...);
  } else if (H == 64) {
    fa_fwd_dispatch_seg<64, 64>(seg, args...);
  } else if (ktf == 128) {
    fa_fwd_dispatch_seg<128, 128>(seg, args...);
  } else {
    fa_fwd_dispatch_seg<128, 64>(seg, args...);
  }
}

template <class... Args>
static void fa_fwd_fused_dispatch(bool has_bias, dim3 grid, size_t shmem,
                                  hipStream_t stream, Args... args) {
  if (has_bias) {
    hipLaunchKernelGGL((fa_fwd_fused_kernel<FFW, true>), grid,
                       dim3(FFW * WAVE_SIZE), shmem, stream, args...);
  } else {
    hipLaunchKernelGGL((fa_fwd_fused_kernel<FFW, false>), grid,
                       dim3(FFW * WAVE_SIZE), shmem, stream, args...);
  }
}

template <int H, bool BIAS_GRAD, class... Args>
static void fa_bwd_launch(dim3 grid, size_t shmem, hipStream_t stream,
                          Args... args) {
  hipLaunchKernelGGL((fa_bwd_kernel<H, BIAS_GRAD>), grid,
                     dim3(NWB * WAVE_SIZE), shmem, stream, args...);
}

template <class... Args>
static void fa_bwd_dispatch(int H, bool bias_grad, Args... args) {
  if (H == 64 && bias_grad) {
    fa_bwd_launch<64, true>(args...);
  } else if (H == 64) {
    fa_bwd_launch<64, false>(args...);
  } else if (bias_grad) {
    fa_bwd_launch<128, true>(args...);
  } else {
    fa_bwd_launch<128, false>(args...);
  }
}

template <bool BIAS_GRAD, class... Args>
static void fa_bwd_fused_launch(dim3 grid, size_t shmem, hipStream_t stream,
                                Args... args) {
  hipLaunchKernelGGL((fa_bwd_fused_kernel<64, BIAS_GRAD>), grid,
                     dim3(NWF * WAVE_SIZE), shmem, stream, args...);
}

template <class... Args>
static void fa_bwd_fused_dispatch(bool bias_grad, Args... args) {
  if (bias_grad) {
    fa_bwd_fused_launch<true>(args...);
  } else {
    fa_bwd_fused_launch<false>(args...);
  }
}

static void check_btnh(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 4 &&
                  t.scalar_type() == torch::kBFloat16,
              name, " must be contiguous bf16 [B,T,N,H]");
}

// Stride contract for q/k/v and caller-provided dq/dk/dv: bf16 [B,T,N,H]
// whose [N][H] dims are dense, whose token rows (b, t) sit at one uniform
// stride that is a multiple of 8 elements and at least N*H, and whose base
// is 16-byte aligned (every access is an aligned 16-byte vector or lies
// inside one). Returns the row stride in elements.
static long check_strided_btnh(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 4 &&
                  t.scalar_type() == torch::kBFloat16,
              name, " must be a CUDA bf16 [B,T,N,H] tensor");
  const long N = t.size(2), H = t.size(3);
  TORCH_CHECK((H == 1 || t.stride(3) == 1) && (N == 1 || t.stride(2) == H),
              name, ": the [N][H] dims must be dense");
  const long row = t.size(1) == 1 && t.size(0) == 1 ? N * H : (
      t.size(1) == 1 ? t.stride(0) : t.stride(1));
  TORCH_CHECK(t.size(0) == 1 || t.size(1) == 1 ||
                  t.stride(0) == t.size(1) * row,
              name, ": batch stride must be T * row stride");
  TORCH_CHECK(row % 8 == 0 && row >= N * H, name,
              ": row stride must be a multiple of 8 elements and >= N*H, got ",
              row);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              ": base pointer must be 16-byte aligned");
  return row;
}

std::vector<torch::Tensor> fa_fwd(torch::Tensor q, torch::Tensor k,
                                  torch::Tensor v,
                                  c10::optional<torch::Tensor> klen,
                                  c10::optional<torch::Tensor> bias,
                                  c10::optional<torch::Tensor> qseg,
                                  c10::optional<torch::Tensor> kseg,
                                  int64_t win_l, int64_t win_r,
                                  int64_t bias_clip, double scale,
                                  int64_t chunk_size, int64_t left_chunks,
                                  const std::string& route) {
  // Every check comes before the first allocation or launch.
  const long sq = check_strided_btnh(q, "q");
  const long sk = check_strided_btnh(k, "k");
  const long sv = check_strided_btnh(v, "v");
  const int B = q.size(0), T = q.size(1), N = q.size(2), H = q.size(3);
  const int S = k.size(1), NKV = k.size(2);
  TORCH_CHECK(H == 64 || H == 128, "H must be 64 or 128, got ", H);
  TORCH_CHECK(N % NKV == 0, "GQA requires N % NKV == 0");
  TORCH_CHECK(k.size(0) == B && k.size(3) == H && v.sizes() == k.sizes(),
              "k/v must be [B,S,NKV,H]");
  const int nbias = 2 * (int)bias_clip + 1;
  const bool bias_row_ok =
      !bias.has_value() ||
      (bias_clip >= 0 && bias->is_cuda() && bias->is_contiguous() &&
       bias->scalar_type() == torch::kBFloat16 &&
       bias->numel() == (long)N * nbias);

  // Route, from shapes only (no device read, so the step still captures
  // into a graph).
  bool fused = false;
  TORCH_CHECK(route == "auto" || route == "tiles" || route == "fused",
              "fa_fwd: unknown route '", route, "'");
  const size_t fused_lds =
      fwd_fused_lds_bytes(std::max(T, 1), bias.has_value(), nbias);
  if (route != "tiles") {
    fused = true;
    const char* why = nullptr;
    if (H != 64) why = "H != 64";
    else if (N != NKV) why = "N != NKV";
    else if (T != S) why = "T != S";
    else if (S > FWD_FUSED_MAX_S) why = "S above the route's limit";
    else if (T < 1 || B < 1) why = "empty call";
    else if (qseg.has_value() || kseg.has_value()) why = "segment ids";
    else if (chunk_size > 0) why = "chunkwise mask";
    else if (B > 65535) why = "B above the grid limit";
    else if (!bias_row_ok) why = "bias is not bf16 [N, 2*bias_clip+1]";
    else if (fused_lds > fa_lds_limit_bytes()) why = "LDS request too large";
    if (why) {
      TORCH_CHECK(route == "auto", "fa_fwd: route '", route,
                  "' does not support this call: ", why);
      fused = false;
    }
  }

  auto o = torch::empty({B, T, N, H}, q.options());
  auto lse = torch::empty({B, N, T}, q.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
  const int* klp = klen.has_value() ? klen->data_ptr<int>() : nullptr;
  const unsigned short* bp =
      bias.has_value() ? (const unsigned short*)bias->data_ptr() : nullptr;
  if (fused) {
    fa_fwd_fused_dispatch(
        bp != nullptr, dim3(N, B), fused_lds, stream.stream(),
        (const unsigned short*)q.data_ptr(),
        (const unsigned short*)k.data_ptr(),
        (const unsigned short*)v.data_ptr(), klp, bp,
        (unsigned short*)o.data_ptr(), lse.data_ptr<float>(), T, N,
        (int)win_l, (int)win_r, (int)bias_clip, (float)scale, sq, sk, sv);
    return {o, lse};
  }
  dim3 grid((T + FQT - 1) / FQT, N, B);
  const int* qsp = qseg.has_value() ? qseg->data_ptr<int>() : nullptr;
  const int* ksp = kseg.has_value() ? kseg->data_ptr<int>() : nullptr;
  // Big KV tiles amortize staging barriers, but waste work on short
  // sequences (masked overhang): pick by S.
  const int ktf = S >= 512 ? 128 : 64;
  fa_fwd_dispatch(H, ktf, qsp != nullptr, grid, stream.stream(),
                  (const unsigned short*)q.data_ptr(),
                  (const unsigned short*)k.data_ptr(),
                  (const unsigned short*)v.data_ptr(), klp, bp, qsp, ksp,
                  (unsigned short*)o.data_ptr(), lse.data_ptr<float>(), B, T,
                  S, N, NKV, (int)win_l, (int)win_r, (int)bias_clip,
                  (float)scale, (int)chunk_size, (int)left_chunks, sq, sk, sv);
  return {o, lse};
}

std::vector<torch::Tensor> fa_bwd(torch::Tensor dout, torch::Tensor q,
                                  torch::Tensor k, torch::Tensor v,
                                  torch::Tensor o, torch::Tensor lse,
                                  c10::optional<torch::Tensor> klen,
                                  c10::optional<torch::Tensor> bias,
                                  c10::optional<torch::Tensor> qseg,
                                  c10::optional<torch::Tensor> kseg,
                                  bool bias_grad, int64_t win_l,
                                  int64_t win_r, int64_t bias_clip,
                                  double scale, int64_t chunk_size,
                                  int64_t left_chunks,
                                  c10::optional<torch::Tensor> dq_out,
                                  c10::optional<torch::Tensor> dk_out,
                                  c10::optional<torch::Tensor> dv_out,
                                  const std::string& route) {
  // Every check comes before the first allocation or launch, so a
  // rejected call leaves caller-provided outputs untouched.
  const long sq = check_strided_btnh(q, "q");
  const long sk = check_strided_btnh(k, "k");
  const long sv = check_strided_btnh(v, "v");
  check_btnh(dout, "dout");
  check_btnh(o, "o");
  const int B = q.size(0), T = q.size(1), N = q.size(2), H = q.size(3);
  const int S = k.size(1), NKV = k.size(2);
  TORCH_CHECK(H == 64 || H == 128, "H must be 64 or 128, got ", H);
  TORCH_CHECK(N % NKV == 0, "GQA requires N % NKV == 0");
  TORCH_CHECK(k.size(0) == B && k.size(3) == H && v.sizes() == k.sizes(),
              "k/v must be [B,S,NKV,H]");
  TORCH_CHECK(dout.size(0) == B && dout.size(1) == T && dout.size(2) == N &&
                  dout.size(3) == H && o.sizes() == dout.sizes(),
              "dout/o must be [B,T,N,H]");
  const int group = N / NKV;
  // Caller-provided outputs: dk/dv are written by the main kernel and dq by
  // the cast kernel, straight into (views of) the caller's buffers.
  const bool into = dq_out.has_value();
  TORCH_CHECK(dk_out.has_value() == into && dv_out.has_value() == into,
              "dq_out, dk_out and dv_out come together");
  long sdq = (long)N * H, sdk = (long)NKV * H, sdv = (long)NKV * H;
  if (into) {
    TORCH_CHECK(group == 1, "caller-provided outputs need N == NKV");
    sdq = check_strided_btnh(*dq_out, "dq_out");
    sdk = check_strided_btnh(*dk_out, "dk_out");
    sdv = check_strided_btnh(*dv_out, "dv_out");
    TORCH_CHECK(dq_out->sizes() == dout.sizes() &&
                    dk_out->sizes() == k.sizes() &&
                    dv_out->sizes() == k.sizes(),
                "dq_out/dk_out/dv_out must have the shapes of q/k/v");
  }
  const int nbias = 2 * (int)bias_clip + 1;
  const bool bg = bias.has_value() && bias_grad;
  // The fused kernel copies the head's whole bias row into LDS.
  const bool bias_row_ok =
      !bias.has_value() ||
      (bias_clip >= 0 && bias->is_cuda() && bias->is_contiguous() &&
       bias->scalar_type() == torch::kBFloat16 &&
       bias->numel() == (long)N * nbias);

  // Route, from shapes only (no device read, so the step still captures
  // into a graph).
  bool fused = false;
  TORCH_CHECK(route == "auto" || route == "tiles" || route == "fused",
              "fa_bwd: unknown route '", route, "'");
  const size_t fused_lds = fused_lds_bytes(bias.has_value(), bg, nbias);
  if (route != "tiles") {
    fused = true;
    const char* why = nullptr;
    if (H != 64) why = "H != 64";
    else if (group != 1) why = "N != NKV";
    else if (T != S) why = "T != S";
    else if (S > FUSED_MAX_S) why = "S above the route's limit";
    else if (qseg.has_value() || kseg.has_value()) why = "segment ids";
    else if (chunk_size > 0) why = "chunkwise mask";
    else if (B > 65535) why = "B above the grid limit";
    else if (!bias_row_ok) why = "bias is not bf16 [N, 2*bias_clip+1]";
    else if (!lse.is_cuda() || !lse.is_contiguous() ||
             lse.scalar_type() != torch::kFloat32 ||
             lse.numel() != (long)B * N * T)
      why = "lse is not fp32 [B,N,T]";
    else if (fused_lds > fa_lds_limit_bytes()) why = "LDS request too large";
    if (why) {
      TORCH_CHECK(route != "fused", "fa_bwd: route '", route,
                  "' does not support this call: ", why);
      fused = false;
    }
  }

  auto stream = at::cuda::getCurrentCUDAStream();
  const int* klp = klen.has_value() ? klen->data_ptr<int>() : nullptr;
  const unsigned short* bp =
      bias.has_value() ? (const unsigned short*)bias->data_ptr() : nullptr;

  if (fused) {
    torch::Tensor dq_t, dk_t, dv_t;
    if (into) {
      dq_t = *dq_out;
      dk_t = *dk_out;
      dv_t = *dv_out;
    } else {
      dq_t = torch::empty({B, T, N, H}, q.options());
      dk_t = torch::empty({B, S, NKV, H}, q.options());
      dv_t = torch::empty({B, S, NKV, H}, q.options());
    }
    auto fopts = q.options().dtype(torch::kFloat32);
    // Without a bias gradient the table's gradient is all zeros, as on the
    // tiles route.
    torch::Tensor dbias_t =
        bg ? torch::empty({N, nbias}, fopts)
           : torch::zeros({bias.has_value() ? N : 0,
                           bias.has_value() ? nbias : 0}, fopts);
    torch::Tensor part;
    if (bg) part = torch::empty({B, N, nbias}, fopts);
    fa_bwd_fused_dispatch(
        bg, dim3(N, B), fused_lds, stream.stream(),
        (const unsigned short*)dout.data_ptr(),
        (const unsigned short*)q.data_ptr(),
        (const unsigned short*)k.data_ptr(),
        (const unsigned short*)v.data_ptr(),
        (const unsigned short*)o.data_ptr(), lse.data_ptr<float>(), klp, bp,
        (unsigned short*)dq_t.data_ptr(), (unsigned short*)dk_t.data_ptr(),
        (unsigned short*)dv_t.data_ptr(),
        bg ? part.data_ptr<float>() : nullptr, T, N, (int)win_l, (int)win_r,
        (int)bias_clip, (float)scale, sq, sk, sv, sdq, sdk, sdv);
    if (bg) {
      const int D = N * nbias;
      hipLaunchKernelGGL(fa_dbias_reduce, dim3(cdiv(D, WAVE_SIZE)),
                         dim3(WAVE_SIZE * kDbSlices), 0, stream,
                         part.data_ptr<float>(), dbias_t.data_ptr<float>(), B,
                         D);
    }
    return {dq_t, dk_t, dv_t, dbias_t};
  }

  auto delta = torch::empty({B, N, T}, q.options().dtype(torch::kFloat32));
  {
    const long rows = (long)B * T * N;
    auto kernel = H == 64 ? attn_delta_kernel<64> : attn_delta_kernel<128>;
    hipLaunchKernelGGL(kernel, dim3(cdiv(rows, DELTA_BLOCK / (H / 8))),
                       dim3(DELTA_BLOCK), 0, stream,
                       (const unsigned short*)dout.data_ptr(),
                       (const unsigned short*)o.data_ptr(),
                       delta.data_ptr<float>(), B, T, N);
  }

  auto fopts = q.options().dtype(torch::kFloat32);
  auto dq_acc = torch::zeros({B, T, N, H}, fopts);
  torch::Tensor dk_t, dv_t;
  if (into) {
    dk_t = *dk_out;
    dv_t = *dv_out;
  } else if (group == 1) {
    dk_t = torch::empty({B, S, NKV, H}, q.options());
    dv_t = torch::empty({B, S, NKV, H}, q.options());
  } else {
    dk_t = torch::zeros({B, S, NKV, H}, fopts);
    dv_t = torch::zeros({B, S, NKV, H}, fopts);
  }
  torch::Tensor dbias_t = torch::zeros(
      {bias.has_value() ? N : 0, bias.has_value() ? nbias : 0},
      q.options().dtype(torch::kFloat32));

  const int* qsp = qseg.has_value() ? qseg->data_ptr<int>() : nullptr;
  const int* ksp = kseg.has_value() ? kseg->data_ptr<int>() : nullptr;

  fa_bwd_dispatch(
      H, bg, dim3((S + KTB - 1) / KTB, NKV, B), bwd_lds_bytes(H, bg, nbias),
      stream.stream(), (const unsigned short*)dout.data_ptr(),
      (const unsigned short*)q.data_ptr(),
      (const unsigned short*)k.data_ptr(),
      (const unsigned short*)v.data_ptr(), lse.data_ptr<float>(),
      delta.data_ptr<float>(), klp, bp, qsp, ksp, dq_acc.data_ptr<float>(),
      (unsigned short*)dk_t.data_ptr(), (unsigned short*)dv_t.data_ptr(),
      dbias_t.numel() ? dbias_t.data_ptr<float>() : nullptr, B, T, S, N, NKV,
      (int)win_l, (int)win_r, (int)bias_clip, (float)scale, (int)chunk_size,
      (int)left_chunks, sq, sk, sv, sdk, sdv);

  torch::Tensor dq;
  if (into) {
    dq = *dq_out;
    const long rows = (long)B * T;
    const int nh_vec = N * H / 8;
    dim3 cgrid(cdiv(nh_vec, 256), (unsigned)std::min<long>(rows, 4096));
    hipLaunchKernelGGL(fa_dq_cast, cgrid, dim3(256), 0, stream,
                       dq_acc.data_ptr<float>(), (unsigned short*)dq.data_ptr(),
                       rows, nh_vec, sdq);
  } else {
    dq = dq_acc.to(torch::kBFloat16);
  }
  auto dk = group == 1 ? dk_t : dk_t.to(torch::kBFloat16);
  auto dv = group == 1 ? dv_t : dv_t.to(torch::kBFloat16);
  return {dq, dk, dv, dbias_t};
}
