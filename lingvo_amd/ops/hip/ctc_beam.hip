// CTC prefix beam search for gfx950: the W most probable label sequences of
// batch-major logits [B,T,V] (bf16 or fp32), each scored with the sum over
// all of its alignments. Two launches on one stream, no host sync.
//
//  1. ctc_prune_rows_kernel: one wave per (b,t) row, 16-byte loads with a
//     scalar head/tail. First sweep: the row maximum and, per lane, the
//     top-C non-blank raw logits in registers (C is a compile-time bound, as
//     in topk.hip: dynamic indexing would spill). Second sweep (the row is
//     in cache): sum of exp(x - max) in 64-bit fixed point. Both the maximum
//     and an integer sum are independent of which lane saw which element, so
//     the lse - and with it every later number - is the same bit pattern for
//     bf16 logits and for the same values in fp32, whose rows split into
//     head / vectors / tail differently. The lanes' lists are merged by C
//     rounds of a wave arg-max over shuffles (larger logit, then lower id).
//     Writes the frame table: cand_id [B,T,C] i32, cand_lp [B,T,C] fp32
//     (logit - lse), blank_lp [B,T]. It is the only pass over [B,T,V].
//  2. ctc_beam_kernel: one workgroup per utterance, one lane per candidate
//     of the frame: W stays (lane j keeps beam slot j) and W*C extends (slot
//     i by the frame's r-th token), W*(C+1) <= 544 lanes. The beam lives in
//     LDS, double-buffered: p_b, p_nb, a 64-bit hash of the prefix, its
//     length, last token and trie node. The frame table does not depend on
//     the beam and is staged into LDS kChunk frames ahead of use. Per frame:
//       form   every lane computes its candidate's (p_b', p_nb');
//       merge  stay lane j looks for the slot i with len_i == len_j - 1 and
//              Mix(hash_i, last_j) == hash_j, folds extend(i, last_j) into
//              its own p_nb' and stamps that lane dead in LDS;
//       select every live candidate counts the candidates that beat it
//              (larger score, then lower lane: stays in slot order, then
//              extends by (slot, token rank)) with 16-byte broadcast LDS
//              reads, and writes itself to the slot of its rank if < W;
//       trie   a surviving extend appends (parent node, token) at
//              [b, t, rank] of a global workspace.
//     After the last frame W lanes walk their chains back and write the
//     left-packed rows. Nothing is atomic and the result is the same bits on
//     every run.
//
// Two prefixes are taken for one when their 64-bit hashes, their lengths and
// their last tokens all agree; a false merge needs a 64-bit collision between
// two prefixes of one length inside one beam.
//
// "Impossible" is the finite sentinel kNeg, as in ctc.hip. Frames >= T_b are
// not visited; T_b == 0 gives the empty prefix with score 0; a length outside
// [0,T] gives valid = 0 and no hypothesis. Unused slots get length 0, ids 0
// and score kNeg. Every element of every output is written, and of the
// workspaces every element that is read.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <climits>

#include "common.h"
#include "host_checks.h"
#include "lse_rows.h"

namespace {

constexpr int kMaxW = 32;
constexpr int kMaxC = 16;
constexpr int kRowWaves = 4;  // rows per workgroup in the prune pass
constexpr int kChunk = 8;     // frames of the table staged at a time
constexpr int kMaxLanes =
    (kMaxW * (kMaxC + 1) + WAVE_SIZE - 1) / WAVE_SIZE * WAVE_SIZE;  // 576
// Table words one lane carries while a chunk is in flight (>= 64 lanes).
constexpr int kStagePer = kChunk * kMaxC / WAVE_SIZE;
constexpr float kNeg = -1e30f;
constexpr float kNegTest = -1e29f;
constexpr unsigned long long kHashSeed = 0x243F6A8885A308D3ull;

// ---- pass 1: prune ---------------------------------------------------------
// f(value, index) over row lr, each lane seeing its indices in rising order.
template <typename T, typename F>
__device__ __forceinline__ void ForRow(const T* __restrict__ lr, int V,
                                       int lane, F f) {
  typedef Elem<T> El;
  const int head = HeadElems(lr, V);
  const int nvec = (V - head) / El::kVec;
  for (int j = lane; j < head; j += WAVE_SIZE) f(El::ToFloat(lr[j]), j);
  for (int i = lane; i < nvec; i += WAVE_SIZE) {
    typename El::Vec v =
        *reinterpret_cast<const typename El::Vec*>(lr + head + i * El::kVec);
#pragma unroll
    for (int e = 0; e < El::kVec; ++e)
      f(El::ToFloat(v[e]), head + i * El::kVec + e);
  }
  for (int j = head + nvec * El::kVec + lane; j < V; j += WAVE_SIZE)
    f(El::ToFloat(lr[j]), j);
}

template <typename T, int KC>
__global__ void __launch_bounds__(kRowWaves* WAVE_SIZE)
    ctc_prune_rows_kernel(const T* __restrict__ logits,
                          const long* __restrict__ in_len,
                          int* __restrict__ cand_id,
                          float* __restrict__ cand_lp,
                          float* __restrict__ blank_lp, int B, int Tn, int V,
                          int C, int blank, int shift) {
  typedef Elem<T> El;
  const long row = (long)blockIdx.x * kRowWaves + threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  if (row >= (long)B * Tn) return;
  const int b = (int)(row / Tn);
  const int t = (int)(row % Tn);
  const long tl = in_len[b];
  const int tb = (tl >= 0 && tl <= Tn) ? (int)tl : 0;
  if (t >= tb) {  // padded frame: nothing to read, defined outputs
    if (lane < C) {
      cand_id[row * C + lane] = 0;
      cand_lp[row * C + lane] = kNeg;
    }
    if (lane == 0) blank_lp[row] = 0.f;
    return;
  }
  const T* lr = logits + row * V;

  // Sweep 1: maximum, and this lane's top KC (sorted, the lower id ahead
  // among equals since ids come in rising order).
  float lv[KC];
  int li[KC];
#pragma unroll
  for (int k = 0; k < KC; ++k) {
    lv[k] = -INFINITY;
    li[k] = INT_MAX;
  }
  float m = kNeg;
  ForRow(lr, V, lane, [&](float x, int j) {
    m = fmaxf(m, x);
    if (j == blank || !(x > lv[KC - 1])) return;
    lv[KC - 1] = x;
    li[KC - 1] = j;
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
  });
  m = wave_reduce_max(m);

  // Sweep 2: sum of exp(x - m) in fixed point, 2^-shift per unit; the host
  // picks shift so that V terms of at most 2^shift fit in 63 bits.
  const float scale = __uint_as_float((unsigned)(127 + shift) << 23);
  unsigned long long acc = 0;
  ForRow(lr, V, lane, [&](float x, int) {
    acc += (unsigned long long)(expf(x - m) * scale);
  });
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)acc, off);
    const unsigned hi = __shfl_xor((unsigned)(acc >> 32), off);
    acc += ((unsigned long long)hi << 32) | lo;
  }
  const float lse = m + logf((float)ldexp((double)acc, -shift));

  // Merge: C rounds of a wave arg-max over the lists' heads.
  float keep_v = 0.f;
  int keep_i = INT_MAX;
  for (int r = 0; r < C; ++r) {
    float bv = lv[0];
    int bi = li[0];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == r) {
      keep_v = bv;
      keep_i = bi;
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
  if (lane < C) {  // fewer than C finite logits: impossible candidates
    const bool real = keep_i != INT_MAX;
    cand_id[row * C + lane] = real ? keep_i : -1;
    cand_lp[row * C + lane] = real ? keep_v - lse : kNeg;
  }
  if (lane == 0) blank_lp[row] = El::ToFloat(lr[blank]) - lse;
}

// ---- pass 2: the search ----------------------------------------------------
__device__ __forceinline__ float Lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (!(m > kNegTest)) return kNeg;
  return m + logf(expf(a - m) + expf(b - m));
}

__device__ __forceinline__ float AddLp(float x, float lp) {
  return (x > kNegTest && lp > kNegTest) ? x + lp : kNeg;
}

// Hash of prefix + tok from the hash of prefix (splitmix64 finaliser).
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

struct Beam {  // one of the two LDS copies; an unused slot has len -2
  float pb[kMaxW];
  float pnb[kMaxW];
  unsigned long long hash[kMaxW];
  int len[kMaxW];
  int last[kMaxW];
  int node[kMaxW];
};

__global__ void __launch_bounds__(kMaxLanes)
    ctc_beam_kernel(const int* __restrict__ cand_id,
                    const float* __restrict__ cand_lp,
                    const float* __restrict__ blank_lp,
                    const long* __restrict__ in_len, int2* trie,
                    long* __restrict__ out_ids, long* __restrict__ out_lens,
                    float* __restrict__ out_scores, float* __restrict__ valid,
                    int Tn, int W, int C) {
  __shared__ Beam beam[2];
  __shared__ __attribute__((aligned(16))) float sc[kMaxLanes];
  __shared__ int dead[kMaxLanes];  // frame + 1 of the last merge-away
  __shared__ int s_id[2][kChunk * kMaxC];
  __shared__ float s_lp[2][kChunk * kMaxC];
  __shared__ float s_bl[2][kChunk];
  __shared__ int fin_len[kMaxW];
  const int b = blockIdx.x;
  const int n = threadIdx.x;
  const int N = W * (C + 1);
  const long tl = in_len[b];
  const bool ok = tl >= 0 && tl <= Tn;
  const int tb = ok ? (int)tl : 0;
  const int* gid = cand_id + (long)b * Tn * C;
  const float* glp = cand_lp + (long)b * Tn * C;
  const float* gbl = blank_lp + (long)b * Tn;
  int2* tr = trie + (long)b * Tn * W;

  // Table chunk starting at frame t0: global -> registers, registers -> LDS.
  int rid[kStagePer];
  float rlp[kStagePer];
  float rbl = 0.f;
  auto stage_load = [&](int t0) {
    const int nf = min(kChunk, tb - t0);  // <= 0: nothing left
#pragma unroll
    for (int k = 0; k < kStagePer; ++k) {
      const int e = n + k * (int)blockDim.x;
      if (e < nf * C) {
        rid[k] = gid[(long)t0 * C + e];
        rlp[k] = glp[(long)t0 * C + e];
      }
    }
    if (n < nf) rbl = gbl[t0 + n];
  };
  auto stage_store = [&](int t0, int buf) {
    const int nf = min(kChunk, tb - t0);
#pragma unroll
    for (int k = 0; k < kStagePer; ++k) {
      const int e = n + k * (int)blockDim.x;
      if (e < nf * C) {
        s_id[buf][e] = rid[k];
        s_lp[buf][e] = rlp[k];
      }
    }
    if (n < nf) s_bl[buf][n] = rbl;
  };

  dead[n] = 0;
  if (n < W) {  // the empty prefix in slot 0 of a valid row, nothing else
    const bool root = ok && n == 0;
    beam[0].pb[n] = root ? 0.f : kNeg;
    beam[0].pnb[n] = kNeg;
    beam[0].hash[n] = kHashSeed;
    beam[0].len[n] = root ? 0 : -2;
    beam[0].last[n] = -1;
    beam[0].node[n] = -1;
  }
  stage_load(0);
  stage_store(0, 0);
  __syncthreads();

  for (int t = 0; t < tb; ++t) {
    const Beam& cur = beam[t & 1];
    Beam& nxt = beam[(t & 1) ^ 1];
    const int chunk = t / kChunk, ft = t % kChunk, sb = chunk & 1;
    const bool prefetch = ft == 0;  // uniform
    if (prefetch) stage_load((chunk + 1) * kChunk);
    const int* fid = s_id[sb] + ft * C;
    const float* flp = s_lp[sb] + ft * C;

    // Form this lane's candidate; stays also merge.
    float cpb = kNeg, cpnb = kNeg;
    unsigned long long chash = 0;
    int clen = -2, clast = -1, cnode = -1;
    const bool is_stay = n < W;
    if (n < N) {
      const int slot = is_stay ? n : (n - W) / C;
      const float pb = cur.pb[slot], pnb = cur.pnb[slot];
      const float tot = Lse2(pb, pnb);
      const int len = cur.len[slot], e = cur.last[slot];
      const unsigned long long h = cur.hash[slot];
      if (tot > kNegTest && is_stay) {
        chash = h;
        clen = len;
        clast = e;
        cnode = cur.node[slot];
        cpb = AddLp(tot, s_bl[sb][ft]);
        int re = -1;  // rank of the last token among the frame's tokens
        if (len > 0)
          for (int r = 0; r < C; ++r)
            if (fid[r] == e) re = r;
        if (re >= 0) {
          cpnb = AddLp(pnb, flp[re]);
          for (int i = 0; i < W; ++i) {
            if (cur.len[i] != len - 1 || Mix(cur.hash[i], e) != h) continue;
            const float base = (cur.len[i] > 0 && cur.last[i] == e)
                                   ? cur.pb[i]
                                   : Lse2(cur.pb[i], cur.pnb[i]);
            cpnb = Lse2(cpnb, AddLp(base, flp[re]));
            dead[W + i * C + re] = t + 1;
            break;
          }
        }
      } else if (tot > kNegTest) {
        const int r = (n - W) % C;
        const int c = fid[r];
        cpnb = AddLp((len > 0 && c == e) ? pb : tot, flp[r]);
        chash = Mix(h, c);
        clen = len + 1;
        clast = c;
        cnode = cur.node[slot];  // the parent until the rank is known
      }
    }
    __syncthreads();

    const float score = Lse2(cpb, cpnb);
    const bool live = n < N && dead[n] != t + 1 && score > kNegTest;
    sc[n] = live ? score : kNeg;
    if (n < W) {
      nxt.pb[n] = kNeg;
      nxt.pnb[n] = kNeg;
      nxt.hash[n] = 0;
      nxt.len[n] = -2;
      nxt.last[n] = -1;
      nxt.node[n] = -1;
    }
    __syncthreads();

    // Select by rank.
    if (live) {
      int rank = 0;
      const floatx4* sc4 = reinterpret_cast<const floatx4*>(sc);
      const int n4 = (N + 3) / 4;  // sc is written up to blockDim.x >= 4*n4
      for (int q = 0; q < n4; ++q) {
        const floatx4 v = sc4[q];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          rank += (v[k] > score || (v[k] == score && 4 * q + k < n)) ? 1 : 0;
      }
      if (rank < W) {
        if (!is_stay) {
          tr[(long)t * W + rank] = make_int2(cnode, clast);
          cnode = t * W + rank;
        }
        nxt.pb[rank] = cpb;
        nxt.pnb[rank] = cpnb;
        nxt.hash[rank] = chash;
        nxt.len[rank] = clen;
        nxt.last[rank] = clast;
        nxt.node[rank] = cnode;
      }
    }
    if (prefetch) stage_store((chunk + 1) * kChunk, sb ^ 1);
    __syncthreads();
  }

  // Outputs. The trie words read below were stored by other waves of this
  // workgroup before one of the loop's barriers; see ctc_viterbi_kernel in
  // ctc.hip for why that is enough.
  const Beam& fin = beam[tb & 1];
  long* ids = out_ids + (long)b * W * Tn;
  int flen = 0;
  if (n < W) {
    const float score = Lse2(fin.pb[n], fin.pnb[n]);
    const bool alive = score > kNegTest;
    flen = alive ? fin.len[n] : 0;
    fin_len[n] = flen;
    out_lens[(long)b * W + n] = flen;
    out_scores[(long)b * W + n] = alive ? score : kNeg;
  }
  if (n == 0) valid[b] = ok ? 1.f : 0.f;
  __syncthreads();
  for (long i = n; i < (long)W * Tn; i += blockDim.x)
    if ((int)(i % Tn) >= fin_len[i / Tn]) ids[i] = 0;
  if (n < W) {
    int node = fin.node[n];
    for (int p = flen - 1; p >= 0 && node >= 0; --p) {
      const int2 nd = tr[node];
      ids[(long)n * Tn + p] = nd.y;
      node = nd.x;
    }
  }
}

template <typename T>
void LaunchPrune(const T* logits, const long* in_len, int* cand_id,
                 float* cand_lp, float* blank_lp, int B, int Tn, int V, int C,
                 int blank, int shift, hipStream_t stream) {
  const dim3 grid(cdiv((long)B * Tn, kRowWaves)), block(kRowWaves * WAVE_SIZE);
#define LV_PRUNE(KC)                                                         \
  hipLaunchKernelGGL((ctc_prune_rows_kernel<T, KC>), grid, block, 0, stream, \
                     logits, in_len, cand_id, cand_lp, blank_lp, B, Tn, V, C, \
                     blank, shift)
  if (C <= 4) {
    LV_PRUNE(4);
  } else if (C <= 8) {
    LV_PRUNE(8);
  } else {
    LV_PRUNE(16);
  }
#undef LV_PRUNE
}

}  // namespace

// -> {topk_ids [B,W,T] i64, topk_lens [B,W] i64, topk_scores [B,W] fp32,
//     valid [B] fp32}
std::vector<torch::Tensor> ctc_beam_search(torch::Tensor logits,
                                           torch::Tensor logit_lengths,
                                           int64_t beam_width,
                                           int64_t token_beam,
                                           int64_t blank) {
  TORCH_CHECK(logits.dim() == 3 &&
                  (cuda_contig(logits, torch::kBFloat16) ||
                   cuda_contig(logits, torch::kFloat32)),
              "ctc_beam_search: logits must be CUDA contiguous bf16 or fp32 "
              "[B,T,V]");
  const int64_t b = logits.size(0), t = logits.size(1), v = logits.size(2);
  TORCH_CHECK(b >= 1 && t >= 1, "ctc_beam_search: B >= 1 and T >= 1");
  TORCH_CHECK(v >= 2, "ctc_beam_search: V >= 2");
  TORCH_CHECK(b * t < (1LL << 31) && v < (1LL << 31),
              "ctc_beam_search: B*T and V must fit in int32");
  TORCH_CHECK(blank >= 0 && blank < v,
              "ctc_beam_search: blank_id must be in [0, V)");
  TORCH_CHECK(beam_width >= 1 && beam_width <= kMaxW,
              "ctc_beam_search: beam_width must be in [1, ", kMaxW, "]");
  TORCH_CHECK(token_beam >= 1 && token_beam <= kMaxC,
              "ctc_beam_search: token_beam must be in [1, ", kMaxC, "]");
  TORCH_CHECK(cuda_contig(logit_lengths, torch::kInt64) &&
                  logit_lengths.dim() == 1 && logit_lengths.size(0) == b &&
                  logit_lengths.get_device() == logits.get_device(),
              "ctc_beam_search: logit_lengths must be CUDA contiguous int64 "
              "[B] on the device of logits");
  TORCH_CHECK(t * beam_width < (1LL << 31),
              "ctc_beam_search: T*beam_width must fit in int32");
  const int B = (int)b, T = (int)t, V = (int)v, W = (int)beam_width;
  const int C = (int)std::min<int64_t>(token_beam, v - 1);
  // Fixed-point unit of the prune pass: V terms of at most 2^shift each.
  int bits = 0;
  while ((1LL << bits) < v) ++bits;
  const int shift = std::min(40, 62 - bits);

  auto f32 = logits.options().dtype(torch::kFloat32);
  auto i32 = logits.options().dtype(torch::kInt32);
  auto i64 = logits.options().dtype(torch::kInt64);
  auto cand_id = torch::empty({B, T, C}, i32);
  auto cand_lp = torch::empty({B, T, C}, f32);
  auto blank_lp = torch::empty({B, T}, f32);
  auto trie = torch::empty({B, T, W, 2}, i32);
  auto topk_ids = torch::empty({B, W, T}, i64);
  auto topk_lens = torch::empty({B, W}, i64);
  auto topk_scores = torch::empty({B, W}, f32);
  auto valid = torch::empty({B}, f32);
  auto stream = at::cuda::getCurrentCUDAStream();
  if (logits.scalar_type() == torch::kBFloat16) {
    LaunchPrune<unsigned short>(u16(logits), logit_lengths.data_ptr<long>(),
                                cand_id.data_ptr<int>(),
                                cand_lp.data_ptr<float>(),
                                blank_lp.data_ptr<float>(), B, T, V, C,
                                (int)blank, shift, stream);
  } else {
    LaunchPrune<float>(logits.data_ptr<float>(),
                       logit_lengths.data_ptr<long>(),
                       cand_id.data_ptr<int>(), cand_lp.data_ptr<float>(),
                       blank_lp.data_ptr<float>(), B, T, V, C, (int)blank,
                       shift, stream);
  }
  const int lanes = cdiv(W * (C + 1), WAVE_SIZE) * WAVE_SIZE;  // <= 576
  hipLaunchKernelGGL(ctc_beam_kernel, dim3(B), dim3(lanes), 0, stream,
                     cand_id.data_ptr<int>(), cand_lp.data_ptr<float>(),
                     blank_lp.data_ptr<float>(),
                     logit_lengths.data_ptr<long>(),
                     reinterpret_cast<int2*>(trie.data_ptr()),
                     topk_ids.data_ptr<long>(), topk_lens.data_ptr<long>(),
                     topk_scores.data_ptr<float>(), valid.data_ptr<float>(),
                     T, W, C);
  return {topk_ids, topk_lens, topk_scores, valid};
}
