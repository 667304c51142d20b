// Transducer beam search for gfx950: time-synchronous, at most S labels per
// frame, prefix merging at the end of each frame (the contract is in
// ops/rnnt.py). R = B*W rows, row r = b*W + slot. Per level (S+1 per frame)
// two launches, per frame a third, after the last frame a fourth; the state
// gathers and the prediction-network step between them stay in torch. No
// launch waits on another workgroup, nothing is atomic, no host sync.
//
//  a. rnnt_joint_prune_kernel<MT,KC>: grid (row tiles, V splits), 4 waves.
//     The workgroup builds x = tanh(enc_p[b,t] + pred_p[r]) for its 16*MT
//     rows once (fp32, rounded to bf16) into a swizzled LDS tile that stays
//     resident: 16*MT x J, 64 KB at MT = 2, J = 1024. joint_w^T [V,J]
//     (K-contiguous) streams through two swizzled LDS buffers of 64 columns
//     x 128 k, the next chunk in registers while the MFMAs of this one run;
//     wave w owns columns 16w..16w+15 of the tile and all rows
//     (v_mfma_f32_16x16x32_bf16, fp32 accumulators). A finished 16*MT x 64
//     tile of logits is parked in LDS (two tiles, by parity) and scanned by
//     256/(16*MT) lanes per row, each over its own columns in rising order:
//     online (max, sum exp), the blank's logit, and a sorted top-KC list of
//     non-blank (logit, id) in registers (KC compile-time, as in topk.hip).
//     After the last tile the lanes of a row merge by shuffles and write the
//     split's partial. The [R,V] logits never reach memory. Columns >= V
//     are masked, rows >= R clamp to R-1 and are not stored.
//  b. rnnt_expand_kernel: one workgroup per utterance. Merges the splits'
//     partials in split order (lse, blank log-prob, top-C by counting),
//     writes the level's W pool entries and, below the last level, ranks
//     the W*C candidates by counting (larger score, then lower slot, then
//     lower token rank), writes the new level, the (parent row, token) the
//     host feeds to index_select and the prediction network, and appends
//     trie nodes at [b, (t*S+s)*W + rank].
//  c. rnnt_close_kernel: one workgroup per utterance and frame. Pool
//     entries with equal (64-bit hash, length, last token) fold by
//     log-sum-exp, in pool order, into the one with the lowest index; the W
//     best become the next beam, with the pool index each came from.
//  d. rnnt_finish_kernel: W lanes per utterance walk their chains back.
//
// Utterances with t >= T_b are frozen: expand and close leave their beam
// alone and hand identity indices to the gathers. Two prefixes are taken for
// one under the same 64-bit caveat as ctc_beam.hip. "Impossible" is the
// finite kNeg. Every element of every output is written.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <climits>

#include "common.h"
#include "host_checks.h"
#include "mfma.h"

namespace {

constexpr int kMaxW = 32;
constexpr int kMaxC = 16;
constexpr int kMaxS = 4;
constexpr int kMaxJ = 1024;
constexpr int kMaxSplit = 8;
constexpr int kMaxPool = (kMaxS + 1) * kMaxW;  // 160
constexpr int kThreads = 256;                  // joint kernel: 4 waves
constexpr int kColTile = 64;                   // 4 waves x 16 columns
constexpr int kKChunk = 128;                   // k per streamed chunk
constexpr int kWPitch = kKChunk * 2;           // bytes per column in LDS
constexpr int kWRegs = kColTile * kKChunk / 8 / kThreads;  // 16 B per lane: 4
constexpr int kLPitch = kColTile + 1;          // parked logits, fp32
constexpr float kNeg = -1e30f;
constexpr float kNegTest = -1e29f;
constexpr unsigned long long kHashSeed = 0x243F6A8885A308D3ull;

// ---- a. joint + prune -------------------------------------------------------
inline int APitch(int J) { return (J + 63) / 64 * 128; }  // bytes, swz-safe

inline size_t JointLds(int mt, int J) {
  return (size_t)16 * mt * APitch(J) + 2 * kColTile * kWPitch +
         2 * 16 * mt * kLPitch * sizeof(float);
}

template <int MT, int KC>
__global__ void __launch_bounds__(kThreads)
    rnnt_joint_prune_kernel(const unsigned short* __restrict__ enc_p,
                            const unsigned short* __restrict__ pred_p,
                            const unsigned short* __restrict__ wt,
                            const float* __restrict__ bias,
                            float4* __restrict__ part_stat,
                            int* __restrict__ part_id,
                            float* __restrict__ part_val, int R, int W, int Tn,
                            int t, int J, int V, int C, int blank,
                            int tiles_per_split) {
  constexpr int ROWS = 16 * MT;
  constexpr int TPR = kThreads / ROWS;  // lanes per row in the scan
  constexpr int CPT = kColTile / TPR;   // columns per lane per tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int pitch_a = (J + 63) / 64 * 128;
  char* a_lds = smem;                                   // [ROWS][pitch_a] swz
  char* w_lds = a_lds + ROWS * pitch_a;                 // [2][64][kWPitch] swz
  float* l_lds = (float*)(w_lds + 2 * kColTile * kWPitch);  // [2][ROWS][65]

  const int n = threadIdx.x;
  const int wid = n / WAVE_SIZE, lane = n & 63, g = lane >> 4, cl = lane & 15;
  const int row0 = blockIdx.x * ROWS;
  const int ntiles = (V + kColTile - 1) / kColTile;
  const int tile0 = blockIdx.y * tiles_per_split;
  const int my_tiles = min(tiles_per_split, ntiles - tile0);  // >= 1
  const int nk = (J + kKChunk - 1) / kKChunk;
  const int nq = my_tiles * nk;

  ushortx8 wreg[kWRegs];
  auto w_load = [&](int q) {
    const int col0 = (tile0 + q / nk) * kColTile, k0 = (q % nk) * kKChunk;
#pragma unroll
    for (int i = 0; i < kWRegs; ++i) {
      const int e = n + i * kThreads;
      const int col = col0 + (e >> 4), k = k0 + (e & 15) * 8;
      ushortx8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (col < V && k < J)
        v = *reinterpret_cast<const ushortx8*>(wt + (long)col * J + k);
      wreg[i] = v;
    }
  };
  auto w_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kWRegs; ++i) {
      const int e = n + i * kThreads;
      const int row = e >> 4;
      *reinterpret_cast<ushortx8*>(w_lds + buf * kColTile * kWPitch +
                                   row * kWPitch + swz(row, (e & 15) * 16)) =
          wreg[i];
    }
  };

  w_load(0);
  // The resident A tile.
  const int j8 = J / 8;
  for (int e = n; e < ROWS * j8; e += kThreads) {
    const int lr = e / j8, c8 = e % j8;
    const int r = min(row0 + lr, R - 1);
    const ushortx8 ev = *reinterpret_cast<const ushortx8*>(
        enc_p + ((long)(r / W) * Tn + t) * J + c8 * 8);
    const ushortx8 pv =
        *reinterpret_cast<const ushortx8*>(pred_p + (long)r * J + c8 * 8);
    float f[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
      f[j] = tanhf(bf16_bits_to_float(ev[j]) + bf16_bits_to_float(pv[j]));
    *reinterpret_cast<bf16x8*>(a_lds + lr * pitch_a + swz(lr, c8 * 16)) =
        pack_bf16x8(f);
  }
  w_store(0);
  __syncthreads();

  // Scan state of this lane: row n / TPR, columns (n % TPR) + j * TPR.
  const int srow = n / TPR, ssub = n % TPR;
  float lv[KC];
  int li[KC];
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    lv[k] = -INFINITY;
    li[k] = INT_MAX;
  }
  float m = kNeg, sum = 0.f, bl = kNeg;

  f32x4 acc[MT];
  for (int q = 0; q < nq; ++q) {
    const int kc = q % nk, lt = q / nk;
    const bool more = q + 1 < nq;  // uniform
    if (more) w_load(q + 1);
    if (kc == 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
    }
    const char* wb = w_lds + (q & 1) * kColTile * kWPitch;
    const int k0 = kc * kKChunk;
    const int ksteps = min(kKChunk, J - k0) / 32;
    const int brow = wid * 16 + cl;
    for (int kk = 0; kk < ksteps; ++kk) {
      const bf16x8 bf = *reinterpret_cast<const bf16x8*>(
          wb + brow * kWPitch + swz(brow, (kk * 32 + g * 8) * 2));
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int arow = mt * 16 + cl;
        const bf16x8 af = *reinterpret_cast<const bf16x8*>(
            a_lds + arow * pitch_a + swz(arow, (k0 + kk * 32 + g * 8) * 2));
        acc[mt] = mfma16x16x32_bf16(af, bf, acc[mt]);
      }
    }
    const bool done = kc == nk - 1;  // uniform: the tile's logits are complete
    float* lt_lds = l_lds + (lt & 1) * ROWS * kLPitch;
    if (done) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          lt_lds[(mt * 16 + g * 4 + r) * kLPitch + wid * 16 + cl] = acc[mt][r];
      }
    }
    if (more) w_store((q + 1) & 1);
    __syncthreads();
    if (done) {
      const int col0 = (tile0 + lt) * kColTile;
#pragma unroll
      for (int j = 0; j < CPT; ++j) {
        const int c = ssub + j * TPR, col = col0 + c;
        if (col >= V) continue;
        const float x = lt_lds[srow * kLPitch + c] + bias[col];
        if (x > m) {
          sum = sum * expf(m - x) + 1.f;
          m = x;
        } else {
          sum += expf(x - m);
        }
        if (col == blank) {
          bl = x;
          continue;
        }
        if (C == 0 || !(x > lv[KC - 1])) continue;
        lv[KC - 1] = x;
        li[KC - 1] = col;
#pragma unroll
        for (int k = KC - 1; k > 0; --k) {
          if (lv[k] > lv[k - 1]) {
            const float tv = lv[k];
            lv[k] = lv[k - 1];
            lv[k - 1] = tv;
            const int ti = li[k];
            li[k] = li[k - 1];
            li[k - 1] = ti;
          }
        }
      }
    }
  }

  // Merge the TPR lanes of a row (adjacent lanes of one wave).
#pragma unroll
  for (int off = TPR / 2; off > 0; off >>= 1) {
    const float om = __shfl_xor(m, off), os = __shfl_xor(sum, off);
    const float nm = fmaxf(m, om);
    sum = sum * expf(m - nm) + os * expf(om - nm);
    m = nm;
    bl = fmaxf(bl, __shfl_xor(bl, off));
  }
  const int r = row0 + srow;
  const bool writer = ssub == 0 && r < R;
  const long pr = (long)blockIdx.y * R + r;
  if (writer) part_stat[pr] = make_float4(m, sum, bl, 0.f);
  for (int rd = 0; rd < C; ++rd) {
    float bv = lv[0];
    int bi = li[0];
#pragma unroll
    for (int off = TPR / 2; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (writer) {
      part_id[pr * C + rd] = bi;
      part_val[pr * C + rd] = bv;
    }
    if (li[0] == bi && bi != INT_MAX) {  // the winner's owner pops it
#pragma unroll
      for (int k = 0; k + 1 < KC; ++k) {
        lv[k] = lv[k + 1];
        li[k] = li[k + 1];
      }
      lv[KC - 1] = -INFINITY;
      li[KC - 1] = INT_MAX;
    }
  }
}

// ---- b, c, d: the beam ------------------------------------------------------
__device__ __forceinline__ float Lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (!(m > kNegTest)) return kNeg;
  return m + logf(expf(a - m) + expf(b - m));
}

// Hash of prefix + tok from the hash of prefix (splitmix64 finaliser), as in
// ctc_beam.hip.
__device__ __forceinline__ unsigned long long Mix(unsigned long long h,
                                                  int tok) {
  unsigned long long x =
      h + 0x9E3779B97F4A7C15ull * (unsigned long long)(unsigned)(tok + 1);
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// A set of hypotheses: score, prefix hash, (length, last token, trie node, -).
struct Hyps {
  float* score;
  unsigned long long* hash;
  int4* meta;
};

__global__ void rnnt_init_kernel(Hyps a, const long* __restrict__ enc_len,
                                 int W, int Tn) {
  const int b = blockIdx.x, n = threadIdx.x;
  if (n >= W) return;
  const long tl = enc_len[b];
  const bool root = tl >= 0 && tl <= Tn && n == 0;
  a.score[b * W + n] = root ? 0.f : kNeg;
  a.hash[b * W + n] = kHashSeed;
  a.meta[b * W + n] = make_int4(0, -1, -1, 0);
}

__global__ void __launch_bounds__(kMaxW* kMaxC)
    rnnt_expand_kernel(const float4* __restrict__ part_stat,
                       const int* __restrict__ part_id,
                       const float* __restrict__ part_val,
                       const long* __restrict__ enc_len, Hyps a, Hyps pool,
                       int2* __restrict__ trie, long* __restrict__ parent,
                       long* __restrict__ tok_out, int R, int W, int C, int S,
                       int Tn, int t, int s, int NS, int blank) {
  __shared__ float l_val[kMaxW * kMaxSplit * kMaxC];
  __shared__ int l_id[kMaxW * kMaxSplit * kMaxC];
  __shared__ float m_lp[kMaxW * kMaxC];
  __shared__ int m_id[kMaxW * kMaxC];
  __shared__ float sc[kMaxW * kMaxC];
  __shared__ float s_lse[kMaxW], s_blank[kMaxW];
  __shared__ float c_score[kMaxW], n_score[kMaxW];
  __shared__ unsigned long long c_hash[kMaxW], n_hash[kMaxW];
  __shared__ int4 c_meta[kMaxW], n_meta[kMaxW];
  __shared__ int n_parent[kMaxW], n_tok[kMaxW];
  const int b = blockIdx.x, n = threadIdx.x, nt = blockDim.x;
  const long tl = enc_len[b];
  const int tb = (tl >= 0 && tl <= Tn) ? (int)tl : 0;
  if (t >= tb) {  // frozen: the rows pass through, close keeps level 0
    if (n < W && s < S) {
      parent[b * W + n] = b * W + n;
      tok_out[b * W + n] = blank;
    }
    return;
  }
  const int per = NS * C;  // list entries of one row
  if (n < W) {
    const int r = b * W + n;
    c_score[n] = a.score[r];
    c_hash[n] = a.hash[r];
    c_meta[n] = a.meta[r];
    n_score[n] = kNeg;
    n_hash[n] = 0;
    n_meta[n] = make_int4(0, -1, -1, 0);
    n_parent[n] = b * W;
    n_tok[n] = blank;
    // Splits in order: the same bits on every run.
    float mx = kNeg, bl = kNeg;
    for (int k = 0; k < NS; ++k) {
      const float4 st = part_stat[(long)k * R + r];
      mx = fmaxf(mx, st.x);
      bl = fmaxf(bl, st.z);
    }
    float sum = 0.f;
    for (int k = 0; k < NS; ++k) {
      const float4 st = part_stat[(long)k * R + r];
      sum += st.y * expf(st.x - mx);
    }
    const float lse = mx + logf(sum);
    s_lse[n] = lse;
    s_blank[n] = bl - lse;
  }
  const int staged = s < S ? W * per : 0;  // the last level: the blank alone
  for (int e = n; e < staged; e += nt) {
    const int i = e / per, k = (e % per) / C, j = e % C;
    const long src = ((long)k * R + b * W + i) * C + j;
    l_val[e] = part_val[src];
    l_id[e] = part_id[src];
  }
  for (int e = n; e < W * C; e += nt) {
    m_lp[e] = kNeg;
    m_id[e] = -1;
  }
  __syncthreads();

  // Row i's top C of its NS sorted lists, by counting.
  for (int e = n; e < staged; e += nt) {
    const int i = e / per;
    const float v = l_val[e];
    const int id = l_id[e];
    if (!(c_score[i] > kNegTest) || id == INT_MAX) continue;
    int rank = 0;
    for (int e2 = i * per; e2 < (i + 1) * per; ++e2) {
      const float v2 = l_val[e2];
      const int id2 = l_id[e2];
      rank += (v2 > v || (v2 == v && (id2 < id || (id2 == id && e2 < e))))
                  ? 1 : 0;
    }
    if (rank < C) {
      m_lp[i * C + rank] = v - s_lse[i];
      m_id[i * C + rank] = id;
    }
  }
  if (n < W) {  // the level's pool entries: stay in this frame
    const int p = b * (S + 1) * W + s * W + n;
    const bool live = c_score[n] > kNegTest;
    pool.score[p] = live ? c_score[n] + s_blank[n] : kNeg;
    pool.hash[p] = c_hash[n];
    pool.meta[p] = c_meta[n];
  }
  if (s == S) return;  // uniform
  __syncthreads();

  const int i = n / C;  // candidate n: slot i by its token of rank n % C
  int id = -1;
  float score = kNeg;
  if (n < W * C) {
    id = m_id[n];
    if (c_score[i] > kNegTest && id >= 0) score = c_score[i] + m_lp[n];
  }
  const bool live = score > kNegTest;
  if (n < kMaxW * kMaxC) sc[n] = live ? score : kNeg;
  __syncthreads();
  if (live) {
    int rank = 0;
    for (int q = 0; q < W * C; ++q)
      rank += (sc[q] > score || (sc[q] == score && q < n)) ? 1 : 0;
    if (rank < W) {
      const int node = (t * S + s) * W + rank;
      trie[(long)b * Tn * S * W + node] = make_int2(c_meta[i].z, id);
      n_score[rank] = score;
      n_hash[rank] = Mix(c_hash[i], id);
      n_meta[rank] = make_int4(c_meta[i].x + 1, id, node, 0);
      n_parent[rank] = b * W + i;
      n_tok[rank] = id;
    }
  }
  __syncthreads();
  if (n < W) {
    const int r = b * W + n;
    a.score[r] = n_score[n];
    a.hash[r] = n_hash[n];
    a.meta[r] = n_meta[n];
    parent[r] = n_parent[n];
    tok_out[r] = n_tok[n];
  }
}

__global__ void __launch_bounds__(kMaxPool + 32)
    rnnt_close_kernel(Hyps pool, const long* __restrict__ enc_len, Hyps a,
                      long* __restrict__ src, int W, int S, int Tn, int t) {
  __shared__ float q_score[kMaxPool], ms[kMaxPool];
  __shared__ unsigned long long q_hash[kMaxPool];
  __shared__ int4 q_meta[kMaxPool];
  __shared__ float o_score[kMaxW];
  __shared__ int o_from[kMaxW];
  const int b = blockIdx.x, n = threadIdx.x;
  const int P = (S + 1) * W;
  const long tl = enc_len[b];
  const int tb = (tl >= 0 && tl <= Tn) ? (int)tl : 0;
  if (t >= tb) {  // frozen: level 0 of the pool is the beam itself
    if (n < W) src[b * W + n] = (long)b * P + n;
    return;
  }
  if (n < P) {
    q_score[n] = pool.score[b * P + n];
    q_hash[n] = pool.hash[b * P + n];
    q_meta[n] = pool.meta[b * P + n];
  }
  if (n < W) {
    o_score[n] = kNeg;
    o_from[n] = -1;
  }
  __syncthreads();
  float mine = kNeg;
  if (n < P && q_score[n] > kNegTest) {
    const unsigned long long h = q_hash[n];
    const int len = q_meta[n].x, last = q_meta[n].y;
    auto same = [&](int q) {
      return q_score[q] > kNegTest && q_hash[q] == h && q_meta[q].x == len &&
             q_meta[q].y == last;
    };
    bool first = true;
    for (int q = 0; q < n; ++q) first = first && !same(q);
    if (first) {
      mine = q_score[n];
      for (int q = n + 1; q < P; ++q)
        if (same(q)) mine = Lse2(mine, q_score[q]);
    }
  }
  if (n < P) ms[n] = mine;
  __syncthreads();
  if (mine > kNegTest) {
    int rank = 0;
    for (int q = 0; q < P; ++q)
      rank += (ms[q] > mine || (ms[q] == mine && q < n)) ? 1 : 0;
    if (rank < W) {
      o_score[rank] = mine;
      o_from[rank] = n;
    }
  }
  __syncthreads();
  if (n < W) {
    const int r = b * W + n, from = o_from[n];
    a.score[r] = o_score[n];
    a.hash[r] = from >= 0 ? q_hash[from] : 0;
    a.meta[r] = from >= 0 ? q_meta[from] : make_int4(0, -1, -1, 0);
    src[r] = (long)b * P + (from >= 0 ? from : 0);
  }
}

__global__ void __launch_bounds__(WAVE_SIZE)
    rnnt_finish_kernel(Hyps a, const long* __restrict__ enc_len,
                       const int2* __restrict__ trie,
                       long* __restrict__ out_ids, long* __restrict__ out_lens,
                       float* __restrict__ out_scores,
                       float* __restrict__ valid, int W, int L, int Tn) {
  __shared__ int fin_len[kMaxW];
  const int b = blockIdx.x, n = threadIdx.x;
  const long tl = enc_len[b];
  const int2* tr = trie + (long)b * L * W;
  long* ids = out_ids + (long)b * W * L;
  int flen = 0, node = -1;
  if (n < W) {
    const float score = a.score[b * W + n];
    const bool alive = score > kNegTest;
    const int4 mt = a.meta[b * W + n];
    flen = alive ? mt.x : 0;
    node = mt.z;
    fin_len[n] = flen;
    out_lens[b * W + n] = flen;
    out_scores[b * W + n] = alive ? score : kNeg;
  }
  if (n == 0) valid[b] = (tl >= 0 && tl <= Tn) ? 1.f : 0.f;
  __syncthreads();
  for (long i = n; i < (long)W * L; i += blockDim.x)
    if ((int)(i % L) >= fin_len[i / L]) ids[i] = 0;
  if (n < W) {
    for (int p = flen - 1; p >= 0 && node >= 0; --p) {
      const int2 nd = tr[node];
      ids[(long)n * L + p] = nd.y;
      node = nd.x;
    }
  }
}

// ---- host -------------------------------------------------------------------
// Workspace tensors, in the order rnnt_beam_init returns them.
enum Ws {
  kAScore, kAHash, kAMeta, kPScore, kPHash, kPMeta, kTrie, kParent, kTok, kSrc,
  kPartStat, kPartId, kPartVal, kNumWs
};

Hyps HypsOf(const std::vector<torch::Tensor>& ws, int first) {
  return {ws[first].data_ptr<float>(),
          reinterpret_cast<unsigned long long*>(ws[first + 1].data_ptr()),
          reinterpret_cast<int4*>(ws[first + 2].data_ptr())};
}

struct Split {
  int mt, row_tiles, tiles_per_split, ns;
};

// How the joint launch covers [R,V]: the same on every level of a search.
Split SplitOf(int R, int V) {
  Split sp;
  sp.mt = R <= 16 ? 1 : 2;
  sp.row_tiles = cdiv(R, 16 * sp.mt);
  const int ntiles = cdiv(V, kColTile);
  const int want = std::max(1, std::min(kMaxSplit, 256 / sp.row_tiles));
  sp.tiles_per_split = cdiv(ntiles, std::min(want, ntiles));
  sp.ns = cdiv(ntiles, sp.tiles_per_split);
  return sp;
}

void CheckWs(const std::vector<torch::Tensor>& ws, const torch::Tensor& len,
             int64_t W, int64_t S, int64_t T) {
  TORCH_CHECK(ws.size() == kNumWs, "rnnt_beam: workspace of rnnt_beam_init");
  TORCH_CHECK(cuda_contig(len, torch::kInt64) && len.dim() == 1 &&
                  ws[kAScore].dim() == 2 && ws[kAScore].size(0) == len.size(0) &&
                  ws[kAScore].size(1) == W &&
                  ws[kPScore].size(1) == (S + 1) * W &&
                  ws[kTrie].size(1) == T * S * W,
              "rnnt_beam: workspace does not match B, W, S, T");
}

}  // namespace

// -> workspace (see Ws), the beam set to the empty hypothesis.
std::vector<torch::Tensor> rnnt_beam_init(torch::Tensor enc_lengths,
                                          int64_t frames, int64_t vocab,
                                          int64_t beam_width,
                                          int64_t token_beam,
                                          int64_t max_symbols) {
  TORCH_CHECK(cuda_contig(enc_lengths, torch::kInt64) &&
                  enc_lengths.dim() == 1 && enc_lengths.size(0) >= 1,
              "rnnt_beam_init: enc_lengths must be CUDA contiguous int64 [B]");
  TORCH_CHECK(beam_width >= 1 && beam_width <= kMaxW,
              "rnnt_beam_init: beam_width must be in [1, ", kMaxW, "]");
  TORCH_CHECK(token_beam >= 1 && token_beam <= kMaxC && token_beam < vocab,
              "rnnt_beam_init: token_beam must be in [1, min(", kMaxC,
              ", V-1)]");
  TORCH_CHECK(max_symbols >= 1 && max_symbols <= kMaxS,
              "rnnt_beam_init: max_symbols must be in [1, ", kMaxS, "]");
  const int64_t B = enc_lengths.size(0), W = beam_width, C = token_beam,
                S = max_symbols, T = frames, R = B * W;
  TORCH_CHECK(T >= 1 && vocab >= 2 && vocab < (1LL << 31) &&
                  B * T * S * W < (1LL << 31),
              "rnnt_beam_init: T >= 1, V >= 2, and B*T*S*W must fit in int32");
  auto f32 = enc_lengths.options().dtype(torch::kFloat32);
  auto i32 = enc_lengths.options().dtype(torch::kInt32);
  auto i64 = enc_lengths.options().dtype(torch::kInt64);
  const int ns = SplitOf((int)R, (int)vocab).ns;
  std::vector<torch::Tensor> ws(kNumWs);
  ws[kAScore] = torch::empty({B, W}, f32);
  ws[kAHash] = torch::empty({B, W}, i64);
  ws[kAMeta] = torch::empty({B, W, 4}, i32);
  ws[kPScore] = torch::empty({B, (S + 1) * W}, f32);
  ws[kPHash] = torch::empty({B, (S + 1) * W}, i64);
  ws[kPMeta] = torch::empty({B, (S + 1) * W, 4}, i32);
  ws[kTrie] = torch::empty({B, T * S * W, 2}, i32);
  ws[kParent] = torch::empty({R}, i64);
  ws[kTok] = torch::empty({R}, i64);
  ws[kSrc] = torch::empty({R}, i64);
  ws[kPartStat] = torch::empty({ns, R, 4}, f32);
  ws[kPartId] = torch::empty({ns, R, C}, i32);
  ws[kPartVal] = torch::empty({ns, R, C}, f32);
  hipLaunchKernelGGL(rnnt_init_kernel, dim3((int)B), dim3(WAVE_SIZE), 0,
                     at::cuda::getCurrentCUDAStream(), HypsOf(ws, kAScore),
                     enc_lengths.data_ptr<long>(), (int)W, (int)T);
  return ws;
}

// Level launch a: partials of log_softmax(tanh(enc_p[:,t] + pred_p) @ w + b)
// for every row. top = false on the level that needs the blank alone.
void rnnt_beam_joint(torch::Tensor enc_p, int64_t t, torch::Tensor pred_p,
                     torch::Tensor joint_wt, torch::Tensor joint_b,
                     std::vector<torch::Tensor> ws, int64_t blank, bool top) {
  TORCH_CHECK(ws.size() == kNumWs, "rnnt_beam_joint: workspace");
  TORCH_CHECK(enc_p.dim() == 3 && cuda_contig(enc_p, torch::kBFloat16) &&
                  aligned16(enc_p),
              "rnnt_beam_joint: enc_p must be CUDA contiguous bf16 [B,T,J]");
  const int64_t B = enc_p.size(0), T = enc_p.size(1), J = enc_p.size(2);
  const int64_t W = ws[kAScore].size(1), R = B * W;
  const int64_t C = ws[kPartId].size(2);
  TORCH_CHECK(ws[kAScore].size(0) == B && t >= 0 && t < T,
              "rnnt_beam_joint: workspace batch or frame out of range");
  TORCH_CHECK(J % 32 == 0 && J >= 32 && J <= kMaxJ,
              "rnnt_beam_joint: J must be a multiple of 32 in [32, ", kMaxJ,
              "]");
  TORCH_CHECK(cuda_rows(pred_p, torch::kBFloat16, R, J) && aligned16(pred_p),
              "rnnt_beam_joint: pred_p must be CUDA contiguous bf16 [B*W,J]");
  TORCH_CHECK(joint_wt.dim() == 2 && joint_wt.size(1) == J &&
                  cuda_contig(joint_wt, torch::kBFloat16) &&
                  aligned16(joint_wt),
              "rnnt_beam_joint: joint_wt must be CUDA contiguous bf16 [V,J]");
  const int64_t V = joint_wt.size(0);
  TORCH_CHECK(cuda_contig(joint_b, torch::kFloat32) && joint_b.dim() == 1 &&
                  joint_b.size(0) == V,
              "rnnt_beam_joint: joint_b must be CUDA contiguous fp32 [V]");
  TORCH_CHECK(blank >= 0 && blank < V && C < V,
              "rnnt_beam_joint: blank_id must be in [0, V), token_beam < V");
  const Split sp = SplitOf((int)R, (int)V);
  TORCH_CHECK(ws[kPartStat].size(0) == sp.ns && ws[kPartStat].size(1) == R,
              "rnnt_beam_joint: workspace does not match V");
  const size_t lds = JointLds(sp.mt, (int)J);
  const dim3 grid(sp.row_tiles, sp.ns), block(kThreads);
  auto stream = at::cuda::getCurrentCUDAStream();
  const int c_run = top ? (int)C : 0;
#define LV_JOINT(MT, KC)                                                      \
  do {                                                                        \
    auto kern = rnnt_joint_prune_kernel<MT, KC>;                              \
    LV_CHECK_HIP(hipFuncSetAttribute(                                         \
        reinterpret_cast<const void*>(kern),                                  \
        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));               \
    hipLaunchKernelGGL(kern, grid, block, lds, stream, u16(enc_p),            \
                       u16(pred_p), u16(joint_wt), joint_b.data_ptr<float>(), \
                       reinterpret_cast<float4*>(ws[kPartStat].data_ptr()),   \
                       ws[kPartId].data_ptr<int>(),                           \
                       ws[kPartVal].data_ptr<float>(), (int)R, (int)W,        \
                       (int)T, (int)t, (int)J, (int)V, c_run, (int)blank,     \
                       sp.tiles_per_split);                                   \
  } while (0)
#define LV_JOINT_MT(KC) \
  if (sp.mt == 1) LV_JOINT(1, KC); else LV_JOINT(2, KC)
  if (C <= 4) {
    LV_JOINT_MT(4);
  } else if (C <= 8) {
    LV_JOINT_MT(8);
  } else {
    LV_JOINT_MT(16);
  }
#undef LV_JOINT_MT
#undef LV_JOINT
  LV_CHECK_HIP(hipGetLastError());
}

// Level launch b. level == max_symbols writes the pool entries only.
void rnnt_beam_expand(std::vector<torch::Tensor> ws, torch::Tensor enc_lengths,
                      int64_t t, int64_t level, int64_t max_symbols,
                      int64_t frames, int64_t blank) {
  const int64_t W = ws.size() == kNumWs ? ws[kAScore].size(1) : 0;
  CheckWs(ws, enc_lengths, W, max_symbols, frames);
  TORCH_CHECK(t >= 0 && t < frames && level >= 0 && level <= max_symbols,
              "rnnt_beam_expand: frame or level out of range");
  const int B = (int)enc_lengths.size(0), C = (int)ws[kPartId].size(2);
  const int lanes = cdiv(std::max<int64_t>(W * C, W), WAVE_SIZE) * WAVE_SIZE;
  hipLaunchKernelGGL(
      rnnt_expand_kernel, dim3(B), dim3(lanes), 0,
      at::cuda::getCurrentCUDAStream(),
      reinterpret_cast<const float4*>(ws[kPartStat].data_ptr()),
      ws[kPartId].data_ptr<int>(), ws[kPartVal].data_ptr<float>(),
      enc_lengths.data_ptr<long>(), HypsOf(ws, kAScore), HypsOf(ws, kPScore),
      reinterpret_cast<int2*>(ws[kTrie].data_ptr()),
      ws[kParent].data_ptr<long>(), ws[kTok].data_ptr<long>(), B * (int)W,
      (int)W, C, (int)max_symbols, (int)frames, (int)t, (int)level,
      (int)ws[kPartStat].size(0), (int)blank);
}

// Frame launch c.
void rnnt_beam_close(std::vector<torch::Tensor> ws, torch::Tensor enc_lengths,
                     int64_t t, int64_t max_symbols, int64_t frames) {
  const int64_t W = ws.size() == kNumWs ? ws[kAScore].size(1) : 0;
  CheckWs(ws, enc_lengths, W, max_symbols, frames);
  TORCH_CHECK(t >= 0 && t < frames, "rnnt_beam_close: frame out of range");
  const int lanes = cdiv((max_symbols + 1) * W, WAVE_SIZE) * WAVE_SIZE;
  hipLaunchKernelGGL(rnnt_close_kernel, dim3((int)enc_lengths.size(0)),
                     dim3(lanes), 0, at::cuda::getCurrentCUDAStream(),
                     HypsOf(ws, kPScore), enc_lengths.data_ptr<long>(),
                     HypsOf(ws, kAScore), ws[kSrc].data_ptr<long>(), (int)W,
                     (int)max_symbols, (int)frames, (int)t);
}

// -> {topk_ids [B,W,T*S] i64, topk_lens [B,W] i64, topk_scores [B,W] fp32,
//     valid [B] fp32}
std::vector<torch::Tensor> rnnt_beam_finish(std::vector<torch::Tensor> ws,
                                            torch::Tensor enc_lengths,
                                            int64_t max_symbols,
                                            int64_t frames) {
  const int64_t W = ws.size() == kNumWs ? ws[kAScore].size(1) : 0;
  CheckWs(ws, enc_lengths, W, max_symbols, frames);
  const int64_t B = enc_lengths.size(0), L = frames * max_symbols;
  auto f32 = enc_lengths.options().dtype(torch::kFloat32);
  auto i64 = enc_lengths.options().dtype(torch::kInt64);
  auto topk_ids = torch::empty({B, W, L}, i64);
  auto topk_lens = torch::empty({B, W}, i64);
  auto topk_scores = torch::empty({B, W}, f32);
  auto valid = torch::empty({B}, f32);
  hipLaunchKernelGGL(rnnt_finish_kernel, dim3((int)B), dim3(WAVE_SIZE), 0,
                     at::cuda::getCurrentCUDAStream(), HypsOf(ws, kAScore),
                     enc_lengths.data_ptr<long>(),
                     reinterpret_cast<const int2*>(ws[kTrie].data_ptr()),
                     topk_ids.data_ptr<long>(), topk_lens.data_ptr<long>(),
                     topk_scores.data_ptr<float>(), valid.data_ptr<float>(),
                     (int)W, (int)L, (int)frames);
  return {topk_ids, topk_lens, topk_scores, valid};
}
