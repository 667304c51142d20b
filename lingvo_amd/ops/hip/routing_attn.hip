// Routing (k-means clustered) attention for gfx950, forward and backward
// (layers/attention_sparse.py RoutingAttention; ops/routing_attn.py).
//
// q, k, v [B,T,N,H] bf16, self-attention, H 64 or 128. q_cl, k_cl [B,N,T]
// hold a cluster id in [0, C) per query and key (ids outside are clamped);
// live [B,T] marks the unpadded keys. Query t sees key s of the same (b, n)
// iff s is live, k_cl[s] == q_cl[t], fewer than `window` live keys of that
// cluster precede s, and (not causal or s <= t). The visible set is a
// data-dependent gather, so the lists are built on the device and nothing of
// them is read by the host: every grid has its worst-case size and surplus
// workgroups return at once.
//
//  - routing_lists_kernel: grid (N, B), two waves, integers only. Wave 0
//    sorts the queries of one (b, n) by (cluster, position) with a stable
//    counting sort: per 64 positions the lanes of one cluster find each other
//    by __ballot, their rank is a popcount, and lane c keeps the running
//    count of cluster c in a register (hence C <= 64). It writes
//      q_perm [B,N,T]      the positions in that order,
//      q_start [B,N,C+1]   where each cluster starts in q_perm,
//      q_tiles [B,N,QTmax,3], q_ntiles [B,N]: (cluster, first, count) per
//        64-row tile of that order; a tile never spans two clusters, so there
//        are at most QTmax = ceil(T/64) + C - 1 of them.
//    Wave 1 walks the keys the same way and writes the first `window` live
//    members of each cluster, ascending, as k_sel [B,N,C,W] with k_cnt
//    [B,N,C] (W = min(window, T)). Keys left out (padded or past the window)
//    are in no list: dk and dv start as zero-filled allocations.
//  - routing_fwd_kernel<H>: grid (N, B, QTmax), 4 waves, one query tile of
//    one cluster; a wave owns 16 rows. Q rows are gathered through q_perm
//    into fragments; the cluster's key list is walked in 64-key tiles, K
//    rows gathered into LDS row-major and V rows transposed, 16 bytes per
//    load. The indices of a tile are loaded one tile ahead of its rows, and
//    the rows of the next tile are issued into registers after the barrier,
//    under the MFMA work. Past the end of a list the last valid row is read
//    again and the element mask removes it: the key positions of a tile sit
//    in LDS, INT_MAX where the list has ended, and one compare (kpos > qpos,
//    qpos = INT_MAX - 1 when not causal) masks both. Both lists ascend, so a
//    causal walk ends at the first tile whose first key lies past the tile's
//    last query. Online softmax as in bsa_fwd_kernel. o rows and lse are
//    scattered through q_perm; every query is in one tile, so every row is
//    written once. LDS 24.25 KB (H=64), 40.25 KB (H=128).
//  - routing_bwd_dkdv_kernel<H>: grid (N, B, KTmax), one 64-key tile of one
//    cluster's list (found by a scalar walk over k_cnt). K, V fragments and
//    the dK, dV accumulators stay in registers; walks the cluster's queries
//    q_perm[q_start[c] .. q_start[c+1]) in 64-row tiles, gathering Q, dO, lse
//    and delta. A key is in one list, so each selected row is written once.
//  - routing_bwd_dq_kernel<H>: grid (N, B, QTmax), the forward's walk with K,
//    V and K^T staged; writes each dq row once.
// No atomics on floats, no fp32 gradient buffer; every sum has a fixed order.
//
// Both backward kernels set dS = 0 where P rounds to 1 in fp32. There every
// other probability of the row is below 2^-24, so the true P (dP - delta) is
// below the fp32 rounding of dP - delta (delta sums dO.O in another order
// than the MFMA sums dO.V): the computed value would be noise of 1e-7 where a
// row that sees a single key (window 1, the first key of a causal cluster)
// has dq = dk = 0.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <climits>

#include "host_checks.h"
#include "mfma.h"

// Device code of this file is built without the packed-fp32 VALU forms, as
// block_sparse_attn.hip is; the tile helpers are included inside the region.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                      \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "sparse_tile.h"

namespace {

constexpr int MAX_CLUSTERS = WAVE_SIZE;  // lane c counts cluster c
constexpr int LISTS_BLOCK = 2 * WAVE_SIZE;
constexpr int KEY_DEAD = INT_MAX;        // kpos of a slot past the list's end
constexpr int QPOS_ANY = INT_MAX - 1;    // qpos when not causal

__device__ __forceinline__ int clampi(int x, int lo, int hi) {
  return min(max(x, lo), hi);
}

// ---------------------------------------------------------------------------
// Lists
// ---------------------------------------------------------------------------

// Calls f(cluster, lanes) once per distinct id c >= 0 among the 64 lanes, with
// the ballot of the lanes that hold it. Uniform: every lane runs every round.
template <typename F>
__device__ __forceinline__ void for_each_cluster(int c, F f) {
  unsigned long long rem = __ballot(c >= 0);
  while (rem) {
    const int lead = __ffsll(rem) - 1;
    const int cc = __shfl(c, lead);
    const unsigned long long m = __ballot(c == cc);
    f(cc, m);
    rem &= ~m;
  }
}

// Calls f(t, c) for t = lane, lane + 64, ... in ascending order, c the
// clamped id of position t or -1 (t >= T or not live). Four loads in flight.
template <typename I, typename F>
__device__ __forceinline__ void for_each_chunk(const I* __restrict__ cl,
                                               const bool* __restrict__ live,
                                               int T, int C, F f) {
  const int lane = threadIdx.x & 63;
  for (int t0 = 0; t0 < T; t0 += 4 * WAVE_SIZE) {
    int c[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = t0 + u * WAVE_SIZE + lane;
      c[u] = -1;
      if (t < T && (live == nullptr || live[t]))
        c[u] = clampi((int)cl[t], 0, C - 1);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) f(t0 + u * WAVE_SIZE + lane, c[u]);
  }
}

__device__ __forceinline__ int wave_exclusive_scan(int x) {
  const int lane = threadIdx.x & 63;
  int inc = x;
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const int y = __shfl_up(inc, off);
    if (lane >= off) inc += y;
  }
  return inc - x;
}

template <typename I>
__global__ __launch_bounds__(LISTS_BLOCK) void routing_lists_kernel(
    const I* __restrict__ q_cl, const I* __restrict__ k_cl,
    const bool* __restrict__ live, int* __restrict__ q_perm,
    int* __restrict__ q_start, int* __restrict__ q_tiles,
    int* __restrict__ q_ntiles, int* __restrict__ k_sel,
    int* __restrict__ k_cnt, int T, int N, int C, int W, int QTmax) {
  const int n = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const long bn = (long)b * N + n;
  const unsigned long long below = (1ull << lane) - 1;

  if (threadIdx.x < WAVE_SIZE) {  // wave 0: the queries
    const I* cl = q_cl + bn * T;
    int tot = 0;  // lane c: members of cluster c
    for_each_chunk(cl, (const bool*)nullptr, T, C, [&](int, int c) {
      for_each_cluster(c, [&](int cc, unsigned long long m) {
        if (lane == cc) tot += (int)__popcll(m);
      });
    });
    const int start = wave_exclusive_scan(tot);
    const int nt = (tot + BT - 1) / BT;
    const int tile0 = wave_exclusive_scan(nt);
    if (lane < C) {
      q_start[bn * (C + 1) + lane] = start;
      for (int j = 0; j < nt; ++j) {
        const int slot = tile0 + j;
        if (slot >= QTmax) break;
        int* e = q_tiles + (bn * QTmax + slot) * 3;
        e[0] = lane;
        e[1] = start + j * BT;
        e[2] = min(BT, tot - j * BT);
      }
    }
    if (lane == WAVE_SIZE - 1) {
      q_start[bn * (C + 1) + C] = T;
      q_ntiles[bn] = min(tile0 + nt, QTmax);
    }
    int run = start;  // lane c: next slot of cluster c in q_perm
    int* perm = q_perm + bn * T;
    for_each_chunk(cl, (const bool*)nullptr, T, C, [&](int t, int c) {
      for_each_cluster(c, [&](int cc, unsigned long long m) {
        const int base = __shfl(run, cc);
        if (c == cc) perm[min(base + (int)__popcll(m & below), T - 1)] = t;
        if (lane == cc) run += (int)__popcll(m);
      });
    });
  } else {  // wave 1: the keys
    const I* cl = k_cl + bn * T;
    int run = 0;  // lane c: live members of cluster c so far
    int* sel = k_sel + bn * C * W;
    for_each_chunk(cl, live ? live + (long)b * T : nullptr, T, C,
                   [&](int t, int c) {
      for_each_cluster(c, [&](int cc, unsigned long long m) {
        const int rank = __shfl(run, cc) + (int)__popcll(m & below);
        if (c == cc && rank < W) sel[(long)cc * W + rank] = t;
        if (lane == cc) run += (int)__popcll(m);
      });
    });
    if (lane < C) k_cnt[bn * C + lane] = min(run, W);
  }
}

// ---------------------------------------------------------------------------
// Gathered tiles
// ---------------------------------------------------------------------------

// The token positions of this thread's rows of the 64-row tile that starts at
// list[at]; past list[last] the last entry again.
template <int H>
__device__ __forceinline__ void tile_positions(const int* __restrict__ list,
                                               int at, int last, int T,
                                               int (&pos)[H / 32]) {
  constexpr int TPR = H / 8, RPP = BBLOCK / TPR;
  const int r0 = threadIdx.x / TPR;
#pragma unroll
  for (int rp = 0; rp < H / 32; ++rp)
    pos[rp] = clampi(list[min(at + r0 + rp * RPP, last)], 0, T - 1);
}

template <int H>
__device__ __forceinline__ void tile_gather(const unsigned short* base,
                                            long stride,
                                            const int (&pos)[H / 32],
                                            TileRegs<H>& t) {
  const int h0 = (threadIdx.x % (H / 8)) * 8;
#pragma unroll
  for (int rp = 0; rp < H / 32; ++rp)
    t.v[rp] =
        *reinterpret_cast<const ushortx8*>(base + (long)pos[rp] * stride + h0);
}

// The tile's token positions into LDS, `dead` from list slot `valid` on.
template <int H>
__device__ __forceinline__ void tile_put_positions(const int (&pos)[H / 32],
                                                   int valid, int dead,
                                                   int* dst) {
  constexpr int TPR = H / 8, RPP = BBLOCK / TPR;
  if (threadIdx.x % TPR) return;
  const int r0 = threadIdx.x / TPR;
#pragma unroll
  for (int rp = 0; rp < H / 32; ++rp) {
    const int row = r0 + rp * RPP;
    dst[row] = row < valid ? pos[rp] : dead;
  }
}

// A-operand fragments of the row of x [.,H] at token `pos` (row = lane&15).
template <int H>
__device__ __forceinline__ void strip_gather(const unsigned short* x,
                                             long stride, int pos,
                                             bf16x8 (&frag)[H / 32]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int kk = 0; kk < H / 32; ++kk)
    frag[kk] =
        load_bf16x8_bits(x + (long)pos * stride + kk * 32 + (lane >> 4) * 8);
}

// One query tile and its cluster's key list, read from the tables with every
// value clamped into its range.
struct QueryTile {
  const int* qp;  // q_perm at the tile's first row
  const int* kl;  // the cluster's key list
  int cnt, kc, qlast;
};

__device__ __forceinline__ bool query_tile(
    const int* __restrict__ q_perm, const int* __restrict__ q_tiles,
    const int* __restrict__ q_ntiles, const int* __restrict__ k_sel,
    const int* __restrict__ k_cnt, int T, int N, int C, int W, int QTmax,
    QueryTile& qt) {
  const long bn = (long)blockIdx.y * N + blockIdx.x;
  if ((int)blockIdx.z >= min(q_ntiles[bn], QTmax)) return false;
  const int* e = q_tiles + (bn * QTmax + blockIdx.z) * 3;
  const int c = clampi(e[0], 0, C - 1);
  const int first = clampi(e[1], 0, T - 1);
  qt.cnt = clampi(e[2], 1, min(BT, T - first));
  qt.qp = q_perm + bn * T + first;
  qt.kl = k_sel + (bn * C + c) * W;
  qt.kc = clampi(k_cnt[bn * C + c], 0, W);
  qt.qlast = clampi(qt.qp[qt.cnt - 1], 0, T - 1);
  return true;
}

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------
template <int H>
constexpr size_t fwd_lds_bytes() {
  return (size_t)BT * H * 2 + H * TP + BNW * 16 * TP + BT * sizeof(int);
}

template <int H>
__global__ __launch_bounds__(BBLOCK) void routing_fwd_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const int* __restrict__ q_perm,
    const int* __restrict__ q_tiles, const int* __restrict__ q_ntiles,
    const int* __restrict__ k_sel, const int* __restrict__ k_cnt,
    unsigned short* __restrict__ o, float* __restrict__ lse, int T, int N,
    int C, int W, int QTmax, int causal, float scale, long sq, long sk,
    long sv) {
  constexpr int ROWB = H * 2;
  constexpr int KH = H / 32;
  constexpr int HF = H / 16;
  extern __shared__ char smem[];
  char* k_lds = smem;                   // [64][H] swz
  char* vt_lds = k_lds + BT * ROWB;     // [H][64] swz
  char* p_lds = vt_lds + H * TP;        // [BNW][16][64] swz
  int* kpos_s = (int*)(p_lds + BNW * 16 * TP);  // [64]

  QueryTile qt;
  if (!query_tile(q_perm, q_tiles, q_ntiles, k_sel, k_cnt, T, N, C, W, QTmax,
                  qt))
    return;  // uniform over the block
  const int n = blockIdx.x, b = blockIdx.y;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cl = lane & 15;
  const unsigned short* kb = k + (long)b * T * sk + n * H;
  const unsigned short* vb = v + (long)b * T * sv + n * H;

  bf16x8 qfrag[KH];
  strip_gather<H>(q + (long)b * T * sq + n * H, sq,
                  clampi(qt.qp[min(wid * 16 + cl, qt.cnt - 1)], 0, T - 1),
                  qfrag);
  int qpos[4], qcmp[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    qpos[r] =
        clampi(qt.qp[min(wid * 16 + g * 4 + r, qt.cnt - 1)], 0, T - 1);
    qcmp[r] = causal ? qpos[r] : QPOS_ANY;
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

  const int klast = qt.kc - 1;
  int hi = (qt.kc + BT - 1) / BT;
  if (hi > 0 && causal && clampi(qt.kl[0], 0, T - 1) > qt.qlast) hi = 0;
  TileRegs<H> kreg, vreg;
  int pos[KH], pos_next[KH];
  int first_next = 0;  // first key of the tile after the one in registers
  if (hi > 0) {
    tile_positions<H>(qt.kl, 0, klast, T, pos);
    tile_gather<H>(kb, sk, pos, kreg);
    tile_gather<H>(vb, sv, pos, vreg);
    tile_positions<H>(qt.kl, BT, klast, T, pos_next);
    first_next = clampi(qt.kl[min(BT, klast)], 0, T - 1);
  }

  for (int i = 0; i < hi; ++i) {
    tile_put_rows<H>(kreg, k_lds);
    tile_put_transposed<H>(vreg, vt_lds);
    tile_put_positions<H>(pos, qt.kc - i * BT, KEY_DEAD, kpos_s);
    __syncthreads();

    // Rows of the next tile, in flight under the MFMA work below; their
    // indices came in one tile earlier.
    if (i + 1 < hi) {
      if (causal && first_next > qt.qlast) {
        hi = i + 1;  // ascending: every later key is past every query here
      } else {
#pragma unroll
        for (int rp = 0; rp < KH; ++rp) pos[rp] = pos_next[rp];
        tile_gather<H>(kb, sk, pos, kreg);
        tile_gather<H>(vb, sv, pos, vreg);
        tile_positions<H>(qt.kl, (i + 2) * BT, klast, T, pos_next);
        first_next = clampi(qt.kl[min((i + 2) * BT, klast)], 0, T - 1);
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
      const int kp = kpos_s[nf * 16 + cl];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        s[nf][r] = kp > qcmp[r] ? NEG_INF : acc[r] * scale;
    }
    __builtin_amdgcn_s_setprio(0);

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

  // Epilogue: divide by l, scatter O (bf16) and LSE (fp32). A row that saw no
  // key has l = 0: o = 0, lse = NEG_INF.
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (wid * 16 + g * 4 + r >= qt.cnt) continue;
    const float inv_l = l_run[r] > 0.f ? 1.f / l_run[r] : 0.f;
    unsigned short* orow = o + (((long)b * T + qpos[r]) * N + n) * H;
#pragma unroll
    for (int hf = 0; hf < HF; ++hf)
      orow[hf * 16 + cl] = float_to_bf16_bits(acc_o[hf][r] * inv_l);
    if (cl == 0)
      lse[((long)b * N + n) * T + qpos[r]] =
          l_run[r] > 0.f ? m_run[r] + __logf(l_run[r]) : NEG_INF;
  }
}

// ---------------------------------------------------------------------------
// Backward: dK, dV per key tile of a cluster's list
// ---------------------------------------------------------------------------
template <int H>
constexpr size_t dkdv_lds_bytes() {
  return (size_t)2 * BT * H * 2 + 2 * H * TP + BNW * 16 * TP +
         3 * BT * sizeof(float);
}

template <int H>
__global__ __launch_bounds__(BBLOCK) void routing_bwd_dkdv_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const float* __restrict__ lse,
    const float* __restrict__ delta, const int* __restrict__ q_perm,
    const int* __restrict__ q_start, const int* __restrict__ k_sel,
    const int* __restrict__ k_cnt, unsigned short* __restrict__ dk,
    unsigned short* __restrict__ dv, int T, int N, int C, int W, int causal,
    float scale, long sq, long sk, long sv) {
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
  int* qpos_s = (int*)(delta_s + BT);               // [64]

  const int n = blockIdx.x, b = blockIdx.y;
  const long bn = (long)b * N + n;
  // The cluster and the tile of its list that this workgroup owns.
  int c = 0, kt = blockIdx.z, kc = 0;
  for (; c < C; ++c) {
    kc = clampi(k_cnt[bn * C + c], 0, W);
    const int nt = (kc + BT - 1) / BT;
    if (kt < nt) break;
    kt -= nt;
  }
  if (c == C) return;  // uniform over the block
  const int* kl = k_sel + (bn * C + c) * W;
  const int qs = clampi(q_start[bn * (C + 1) + c], 0, T);
  const int qe = clampi(q_start[bn * (C + 1) + c + 1], qs, T);
  const int* qp = q_perm + bn * T;

  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cl = lane & 15;
  const int k0 = kt * BT + wid * 16;  // this wave's first slot of the list
  const long lrow = bn * T;
  const unsigned short* qb_ptr = q + (long)b * T * sq + n * H;
  const unsigned short* dob_ptr = dout + ((long)b * T * N + n) * H;
  const int kfirst = clampi(kl[kt * BT], 0, T - 1);

  // K, V fragments (A layout): row = key, k = h. A slot past the list's end
  // holds the last key again; its rows are not written.
  bf16x8 kfrag[KH], vfrag[KH];
  {
    const int kp = clampi(kl[min(k0 + cl, kc - 1)], 0, T - 1);
    strip_gather<H>(k + (long)b * T * sk + n * H, sk, kp, kfrag);
    strip_gather<H>(v + (long)b * T * sv + n * H, sv, kp, vfrag);
  }
  int kpos[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    kpos[r] = clampi(kl[min(k0 + g * 4 + r, kc - 1)], 0, T - 1);

  f32x4 acc_dk[HF], acc_dv[HF];
#pragma unroll
  for (int hf = 0; hf < HF; ++hf) {
    acc_dk[hf] = {0.f, 0.f, 0.f, 0.f};
    acc_dv[hf] = {0.f, 0.f, 0.f, 0.f};
  }

  for (int i = qs; i < qe; i += BT) {
    // Ascending lists: a query tile that ends before this tile's first key
    // sees none of its keys.
    if (causal && clampi(qp[min(i + BT, qe) - 1], 0, T - 1) < kfirst)
      continue;  // uniform over the block
    __syncthreads();
    {
      int pos[KH];
      tile_positions<H>(qp, i, qe - 1, T, pos);
      TileRegs<H> t;
      tile_gather<H>(qb_ptr, sq, pos, t);
      tile_put_rows<H>(t, q_lds);
      tile_put_transposed<H>(t, qt_lds);
      tile_gather<H>(dob_ptr, (long)N * H, pos, t);
      tile_put_rows<H>(t, do_lds);
      tile_put_transposed<H>(t, dot_lds);
    }
    if (threadIdx.x < BT) {
      const bool valid = i + (int)threadIdx.x < qe;
      const int qpos = clampi(qp[min(i + (int)threadIdx.x, qe - 1)], 0, T - 1);
      lse_s[threadIdx.x] = valid ? lse[lrow + qpos] : NEG_INF;
      delta_s[threadIdx.x] = valid ? delta[lrow + qpos] : 0.f;
      qpos_s[threadIdx.x] = causal ? qpos : QPOS_ANY;
    }
    __syncthreads();

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
      const int qc = qpos_s[nf * 16 + cl];
      const float l = lse_s[nf * 16 + cl];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool vis = kpos[r] <= qc && l > NEG_INF * 0.5f;
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
      for (int r = 0; r < 4; ++r)
        pt[nf][r] = pt[nf][r] == 1.f ? 0.f : pt[nf][r] * (acc[r] - dl);
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

  // Each selected key is written once; a cluster without queries leaves zeros.
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (k0 + g * 4 + r >= kc) continue;
    const long off = (((long)b * T + kpos[r]) * N + n) * H;
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
  return (size_t)2 * BT * H * 2 + H * TP + BNW * 16 * TP + BT * sizeof(int);
}

template <int H>
__global__ __launch_bounds__(BBLOCK) void routing_bwd_dq_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ k,
    const unsigned short* __restrict__ v, const float* __restrict__ lse,
    const float* __restrict__ delta, const int* __restrict__ q_perm,
    const int* __restrict__ q_tiles, const int* __restrict__ q_ntiles,
    const int* __restrict__ k_sel, const int* __restrict__ k_cnt,
    unsigned short* __restrict__ dq, int T, int N, int C, int W, int QTmax,
    int causal, float scale, long sq, long sk, long sv) {
  constexpr int ROWB = H * 2;
  constexpr int KH = H / 32;
  constexpr int HF = H / 16;
  extern __shared__ char smem[];
  char* k_lds = smem;                   // [64][H] swz
  char* v_lds = k_lds + BT * ROWB;      // [64][H] swz
  char* kt_lds = v_lds + BT * ROWB;     // [H][64] swz
  char* a_lds = kt_lds + H * TP;        // [BNW][16][64] swz
  int* kpos_s = (int*)(a_lds + BNW * 16 * TP);  // [64]

  QueryTile qt;
  if (!query_tile(q_perm, q_tiles, q_ntiles, k_sel, k_cnt, T, N, C, W, QTmax,
                  qt))
    return;  // uniform over the block
  const int n = blockIdx.x, b = blockIdx.y;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, cl = lane & 15;
  const long lrow = ((long)b * N + n) * T;
  const unsigned short* kb = k + (long)b * T * sk + n * H;
  const unsigned short* vb = v + (long)b * T * sv + n * H;

  bf16x8 qfrag[KH], dofrag[KH];
  {
    const int qf = clampi(qt.qp[min(wid * 16 + cl, qt.cnt - 1)], 0, T - 1);
    strip_gather<H>(q + (long)b * T * sq + n * H, sq, qf, qfrag);
    strip_gather<H>(dout + ((long)b * T * N + n) * H, (long)N * H, qf, dofrag);
  }
  int qpos[4], qcmp[4];
  float l_row[4], d_row[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    qpos[r] =
        clampi(qt.qp[min(wid * 16 + g * 4 + r, qt.cnt - 1)], 0, T - 1);
    qcmp[r] = causal ? qpos[r] : QPOS_ANY;
    l_row[r] = lse[lrow + qpos[r]];
    d_row[r] = delta[lrow + qpos[r]];
  }

  f32x4 acc_dq[HF];
#pragma unroll
  for (int hf = 0; hf < HF; ++hf) acc_dq[hf] = {0.f, 0.f, 0.f, 0.f};

  const int hi = (qt.kc + BT - 1) / BT;
  for (int i = 0; i < hi; ++i) {
    // Ascending lists: the walk ends at the first key past the last query.
    if (causal && clampi(qt.kl[i * BT], 0, T - 1) > qt.qlast) break;
    __syncthreads();
    {
      int pos[KH];
      tile_positions<H>(qt.kl, i * BT, qt.kc - 1, T, pos);
      TileRegs<H> t;
      tile_gather<H>(kb, sk, pos, t);
      tile_put_rows<H>(t, k_lds);
      tile_put_transposed<H>(t, kt_lds);
      tile_gather<H>(vb, sv, pos, t);
      tile_put_rows<H>(t, v_lds);
      tile_put_positions<H>(pos, qt.kc - i * BT, KEY_DEAD, kpos_s);
    }
    __syncthreads();

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
      const int kp = kpos_s[nf * 16 + cl];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool vis = kp <= qcmp[r] && l_row[r] > NEG_INF * 0.5f;
        const float p = vis ? __expf(acc[r] * scale - l_row[r]) : 0.f;
        ds[nf][r] = p == 1.f ? 0.f : p * (dp[r] - d_row[r]);
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
    if (wid * 16 + g * 4 + r >= qt.cnt) continue;
    const long off = (((long)b * T + qpos[r]) * N + n) * H;
#pragma unroll
    for (int hf = 0; hf < HF; ++hf)
      dq[off + hf * 16 + cl] = float_to_bf16_bits(acc_dq[hf][r]);
  }
}

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------
struct RoutingShape {
  int B, T, N, H, C, W, QTmax, KTmax;
  long sq, sk, sv;
};

// Shapes and limits from q, k, v and the scalars alone.
RoutingShape routing_shape(const torch::Tensor& q, const torch::Tensor& k,
                           const torch::Tensor& v, int64_t num_clusters,
                           int64_t window) {
  RoutingShape s;
  s.sq = check_token_rows(q, "routing_attn", "q");
  s.sk = check_token_rows(k, "routing_attn", "k");
  s.sv = check_token_rows(v, "routing_attn", "v");
  s.B = q.size(0), s.T = q.size(1), s.N = q.size(2), s.H = q.size(3);
  TORCH_CHECK(s.H == 64 || s.H == 128,
              "routing_attn: H must be 64 or 128, got ", s.H);
  TORCH_CHECK(s.B >= 1 && s.T >= 1 && s.N >= 1, "routing_attn: B, T, N >= 1");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(),
              "routing_attn: k and v must have the shape of q "
              "(self-attention, N == NKV)");
  TORCH_CHECK(num_clusters >= 1 && num_clusters <= MAX_CLUSTERS,
              "routing_attn: num_clusters must be in [1, ", MAX_CLUSTERS,
              "], got ", num_clusters);
  TORCH_CHECK(window >= 1, "routing_attn: window must be >= 1, got ", window);
  s.C = num_clusters;
  s.W = std::min<int64_t>(window, s.T);
  s.QTmax = cdiv(s.T, BT) + s.C - 1;
  s.KTmax = std::min<long>(s.QTmax, (long)s.C * cdiv(s.W, BT));
  TORCH_CHECK(s.B <= 65535 && s.QTmax <= 65535,
              "routing_attn: B and ceil(T/64) + num_clusters - 1 are grid "
              "dims, at most 65535");
  TORCH_CHECK((long)s.B * s.N * s.C * s.W < (1L << 31) &&
                  (long)s.B * s.N * s.QTmax * 3 < (1L << 31),
              "routing_attn: the lists must have fewer than 2^31 entries");
  return s;
}

struct RoutingLists {
  const int *q_perm, *q_start, *q_tiles, *q_ntiles, *k_sel, *k_cnt;
};

// lists = {q_perm, q_start, q_tiles, q_ntiles, k_sel, k_cnt} of routing_lists.
RoutingLists routing_check_lists(const RoutingShape& s,
                                 const std::vector<torch::Tensor>& lists) {
  TORCH_CHECK(lists.size() == 6, "routing_attn: six list tensors expected");
  const std::vector<std::vector<int64_t>> shapes = {
      {s.B, s.N, s.T},          {s.B, s.N, s.C + 1}, {s.B, s.N, s.QTmax, 3},
      {s.B, s.N},               {s.B, s.N, s.C, s.W}, {s.B, s.N, s.C}};
  for (size_t i = 0; i < 6; ++i)
    TORCH_CHECK(cuda_contig(lists[i], torch::kInt32) &&
                    lists[i].sizes() == c10::IntArrayRef(shapes[i]),
                "routing_attn: list ", i, " must be int32 ",
                c10::IntArrayRef(shapes[i]), ", got ", lists[i].sizes());
  return {lists[0].data_ptr<int>(), lists[1].data_ptr<int>(),
          lists[2].data_ptr<int>(), lists[3].data_ptr<int>(),
          lists[4].data_ptr<int>(), lists[5].data_ptr<int>()};
}

template <typename I>
void launch_lists(const RoutingShape& s, const torch::Tensor& q_cl,
                  const torch::Tensor& k_cl, const bool* live,
                  std::vector<torch::Tensor>& l) {
  hipLaunchKernelGGL(routing_lists_kernel<I>, dim3(s.N, s.B),
                     dim3(LISTS_BLOCK), 0, at::cuda::getCurrentCUDAStream(),
                     q_cl.data_ptr<I>(), k_cl.data_ptr<I>(), live,
                     l[0].data_ptr<int>(), l[1].data_ptr<int>(),
                     l[2].data_ptr<int>(), l[3].data_ptr<int>(),
                     l[4].data_ptr<int>(), l[5].data_ptr<int>(), s.T, s.N, s.C,
                     s.W, s.QTmax);
}

}  // namespace

int64_t routing_max_clusters() { return MAX_CLUSTERS; }

// q_cl, k_cl int32 or int64 [B,N,T]; live bool [B,T] or None.
// -> {q_perm, q_start, q_tiles, q_ntiles, k_sel, k_cnt}, int32 (see the top).
std::vector<torch::Tensor> routing_lists(torch::Tensor q, torch::Tensor k,
                                         torch::Tensor v, torch::Tensor q_cl,
                                         torch::Tensor k_cl,
                                         c10::optional<torch::Tensor> live,
                                         int64_t num_clusters,
                                         int64_t window) {
  const RoutingShape s = routing_shape(q, k, v, num_clusters, window);
  const auto idt = q_cl.scalar_type();
  TORCH_CHECK(idt == torch::kInt32 || idt == torch::kInt64,
              "routing_attn: q_cl and k_cl must be int32 or int64");
  for (const auto* t : {&q_cl, &k_cl})
    TORCH_CHECK(cuda_contig(*t, idt) && t->dim() == 3 && t->size(0) == s.B &&
                    t->size(1) == s.N && t->size(2) == s.T,
                "routing_attn: q_cl and k_cl must be contiguous CUDA [B,N,T] "
                "tensors of one integer type");
  if (live.has_value())
    TORCH_CHECK(cuda_contig(*live, torch::kBool) && live->dim() == 2 &&
                    live->size(0) == s.B && live->size(1) == s.T,
                "routing_attn: live must be a contiguous CUDA bool [B,T]");
  const auto io = q.options().dtype(torch::kInt32);
  std::vector<torch::Tensor> l = {
      torch::empty({s.B, s.N, s.T}, io),
      torch::empty({s.B, s.N, s.C + 1}, io),
      torch::empty({s.B, s.N, s.QTmax, 3}, io),
      torch::empty({s.B, s.N}, io),
      torch::empty({s.B, s.N, s.C, s.W}, io),
      torch::empty({s.B, s.N, s.C}, io)};
  const bool* lp = live.has_value() ? live->data_ptr<bool>() : nullptr;
  if (idt == torch::kInt32)
    launch_lists<int>(s, q_cl, k_cl, lp, l);
  else
    launch_lists<int64_t>(s, q_cl, k_cl, lp, l);
  return l;
}

// -> o [B,T,N,H] bf16, lse [B,N,T] fp32.
std::vector<torch::Tensor> routing_attn_fwd(torch::Tensor q, torch::Tensor k,
                                            torch::Tensor v,
                                            std::vector<torch::Tensor> lists,
                                            int64_t num_clusters,
                                            int64_t window, bool causal,
                                            double scale) {
  const RoutingShape s = routing_shape(q, k, v, num_clusters, window);
  const RoutingLists l = routing_check_lists(s, lists);
  auto o = torch::empty({s.B, s.T, s.N, s.H}, q.options());
  auto lse =
      torch::empty({s.B, s.N, s.T}, q.options().dtype(torch::kFloat32));
  auto kernel = s.H == 64 ? routing_fwd_kernel<64> : routing_fwd_kernel<128>;
  const size_t lds = s.H == 64 ? fwd_lds_bytes<64>() : fwd_lds_bytes<128>();
  hipLaunchKernelGGL(kernel, dim3(s.N, s.B, s.QTmax), dim3(BBLOCK), lds,
                     at::cuda::getCurrentCUDAStream(), u16(q), u16(k), u16(v),
                     l.q_perm, l.q_tiles, l.q_ntiles, l.k_sel, l.k_cnt, u16(o),
                     lse.data_ptr<float>(), s.T, s.N, s.C, s.W, s.QTmax,
                     (int)causal, (float)scale, s.sq, s.sk, s.sv);
  return {o, lse};
}

// -> dq, dk, dv, contiguous bf16 [B,T,N,H].
std::vector<torch::Tensor> routing_attn_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor o, torch::Tensor lse, std::vector<torch::Tensor> lists,
    int64_t num_clusters, int64_t window, bool causal, double scale) {
  const RoutingShape s = routing_shape(q, k, v, num_clusters, window);
  const RoutingLists l = routing_check_lists(s, lists);
  check_contig(dout, torch::kBFloat16, "dout");
  check_contig(o, torch::kBFloat16, "o");
  check_contig(lse, torch::kFloat32, "lse");
  TORCH_CHECK(dout.sizes() == q.sizes() && o.sizes() == q.sizes() &&
                  lse.numel() == (long)s.B * s.N * s.T,
              "routing_attn: dout/o must match q, lse must be [B,N,T]");
  TORCH_CHECK(aligned16(dout) && aligned16(o),
              "routing_attn: dout and o must be 16-byte aligned");
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
  // Keys in no list (padded, past the window) keep these zeros.
  auto dk = torch::zeros({s.B, s.T, s.N, s.H}, q.options());
  auto dv = torch::zeros({s.B, s.T, s.N, s.H}, q.options());
  {
    auto kernel = s.H == 64 ? routing_bwd_dkdv_kernel<64>
                            : routing_bwd_dkdv_kernel<128>;
    const size_t lds =
        s.H == 64 ? dkdv_lds_bytes<64>() : dkdv_lds_bytes<128>();
    hipLaunchKernelGGL(kernel, dim3(s.N, s.B, s.KTmax), dim3(BBLOCK), lds,
                       stream, u16(dout), u16(q), u16(k), u16(v),
                       lse.data_ptr<float>(), delta.data_ptr<float>(),
                       l.q_perm, l.q_start, l.k_sel, l.k_cnt, u16(dk), u16(dv),
                       s.T, s.N, s.C, s.W, (int)causal, (float)scale, s.sq,
                       s.sk, s.sv);
  }
  {
    auto kernel =
        s.H == 64 ? routing_bwd_dq_kernel<64> : routing_bwd_dq_kernel<128>;
    const size_t lds = s.H == 64 ? dq_lds_bytes<64>() : dq_lds_bytes<128>();
    hipLaunchKernelGGL(kernel, dim3(s.N, s.B, s.QTmax), dim3(BBLOCK), lds,
                       stream, u16(dout), u16(q), u16(k), u16(v),
                       lse.data_ptr<float>(), delta.data_ptr<float>(),
                       l.q_perm, l.q_tiles, l.q_ntiles, l.k_sel, l.k_cnt,
                       u16(dq), s.T, s.N, s.C, s.W, s.QTmax, (int)causal,
                       (float)scale, s.sq, s.sk, s.sv);
  }
  return {dq, dk, dv};
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
