// CTC loss for gfx950: forward (nll, valid) and backward (dlogits) over
// batch-major logits [B,T,V] in bf16 or fp32, with no fp32 [B,T,V]
// intermediate and no floating-point atomics.
//
// Three passes, ordered only by kernel boundaries on one stream:
//  1. ctc_rows_kernel: one wave per (b,t) row. Online logsumexp over the
//     row (16-byte loads, scalar head/tail for rows that are not 16-byte
//     aligned) -> lse[b,t], then a gather of the compact emission table
//     E[b,t,0..L] = log p_t(blank), log p_t(label_1..L_b).
//  2. ctc_lattice_kernel: grid (B, 2), one workgroup per utterance and
//     direction (alpha / beta), one lane per extended position
//     s < S = 2L+1, two LDS buffers swapped each frame, one
//     __syncthreads() per frame. Writes alpha, beta [B,T,S] and, from the
//     alpha workgroup, nll[b] and valid[b].
//  3. ctc_grad_kernel: one workgroup per (b,t) row. Dense vector stores of
//     g*softmax, __syncthreads(), then the lane that owns the first
//     occurrence of a label sums the occupancies of that label's repeats
//     and alone overwrites dlogits[b,t,label] with g*(softmax - occ),
//     recomputed in fp32 (so bf16 outputs are rounded once).
//
// "Impossible" is the finite sentinel kNeg (-1e30): logsumexp of
// impossible predecessors stays at the sentinel, never NaN.
//
// A row is invalid (valid = 0, nll = 0, dlogits = 0) when its lengths are
// outside [1,T] / [0,L], when a label inside its length is the blank or
// outside [0,V), when no alignment exists (T_b < L_b + repeats), or when
// its likelihood is not finite. Labels are range-checked before every use
// as an index, so an invalid row never reads or writes out of range.
// Every element of every output and workspace is written.
//
// Forced alignment (ctc_align) is pass 1 followed by ctc_viterbi_kernel:
// the best single alignment of each transcript instead of the sum over all
// of them, with the same validity rules. See the comment at that kernel.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include "common.h"
#include "lse_rows.h"

namespace {

constexpr int kCtcMaxL = 511;   // S = 2L+1 <= 1023 lanes of one workgroup
constexpr int kRowWaves = 4;    // rows per workgroup in the row pass
constexpr int kGradThreads = 256;
constexpr float kNeg = -1e30f;
constexpr float kNegTest = -1e29f;
// Dynamic LDS ctc_viterbi_kernel may take for its masks, next to 10 KB of
// static LDS: together under the 64 KB a workgroup gets by default.
constexpr int kLdsMaskBytes = 48 * 1024;

// Lengths of utterance b, zeroed when either is out of range.
__device__ __forceinline__ bool RowLengths(const long* in_len,
                                           const long* lab_len, int b, int T,
                                           int L, int* tb, int* lb) {
  const long t = in_len[b];
  const long l = lab_len[b];
  const bool ok = t >= 1 && t <= T && l >= 0 && l <= L;
  *tb = ok ? (int)t : 0;
  *lb = ok ? (int)l : 0;
  return ok;
}

// ---- pass 1: lse + emission table -----------------------------------------
template <typename T>
__global__ void __launch_bounds__(kRowWaves* WAVE_SIZE)
    ctc_rows_kernel(const T* __restrict__ logits,
                    const long* __restrict__ in_len,
                    const long* __restrict__ labels,
                    const long* __restrict__ lab_len,
                    float* __restrict__ lse_out, float* __restrict__ emis,
                    int B, int Tn, int V, int L, int blank) {
  typedef Elem<T> El;
  const long row = (long)blockIdx.x * kRowWaves + threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  if (row >= (long)B * Tn) return;
  const int b = (int)(row / Tn);
  const int t = (int)(row % Tn);
  int tb, lb;
  RowLengths(in_len, lab_len, b, Tn, L, &tb, &lb);
  float* er = emis + row * (L + 1);
  if (t >= tb) {  // padded frame: nothing to read, defined outputs
    for (int i = lane; i <= L; i += WAVE_SIZE) er[i] = 0.f;
    if (lane == 0) lse_out[row] = 0.f;
    return;
  }
  const T* lr = logits + row * V;
  float m = kNeg, s = 0.f;
  const int head = HeadElems(lr, V);
  const int nvec = (V - head) / El::kVec;
  for (int j = lane; j < head; j += WAVE_SIZE) OnlineLse(El::ToFloat(lr[j]), m, s);
  for (int i = lane; i < nvec; i += WAVE_SIZE) {
    typename El::Vec v =
        *reinterpret_cast<const typename El::Vec*>(lr + head + i * El::kVec);
#pragma unroll
    for (int e = 0; e < El::kVec; ++e) OnlineLse(El::ToFloat(v[e]), m, s);
  }
  for (int j = head + nvec * El::kVec + lane; j < V; j += WAVE_SIZE)
    OnlineLse(El::ToFloat(lr[j]), m, s);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float mo = __shfl_xor(m, off);
    const float so = __shfl_xor(s, off);
    const float mn = fmaxf(m, mo);
    s = s * expf(m - mn) + so * expf(mo - mn);
    m = mn;
  }
  const float lse = m + logf(s);
  if (lane == 0) lse_out[row] = lse;
  for (int i = lane; i <= L; i += WAVE_SIZE) {
    float e = 0.f;
    if (i == 0) {
      e = El::ToFloat(lr[blank]) - lse;
    } else if (i <= lb) {
      const long lbl = labels[(long)b * L + i - 1];
      if (lbl >= 0 && lbl < V) e = El::ToFloat(lr[lbl]) - lse;
    }
    er[i] = e;
  }
}

// ---- pass 2: alpha / beta --------------------------------------------------
__device__ __forceinline__ float Lse3(float a, float b, float c) {
  const float m = fmaxf(a, fmaxf(b, c));
  if (!(m > kNegTest)) return kNeg;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

// Lattice prologue of utterance b, one lane per position s: labels into LDS
// (range-checked), then whether the row has an alignment at all. Holds two
// workgroup barriers, so every lane calls it; the result is uniform.
__device__ __forceinline__ bool LabelsToLds(const long* __restrict__ labels,
                                            int b, int s, int V, int L,
                                            int blank, bool len_ok, int tb,
                                            int lb, int* lab) {
  int bad = 0, rep = 0;
  if (s < lb) {  // blockDim.x >= S > L >= lb
    const long v = labels[(long)b * L + s];
    bad = (v < 0 || v >= V || v == blank) ? 1 : 0;
    lab[s] = bad ? 0 : (int)v;
    if (s > 0) rep = (labels[(long)b * L + s - 1] == v) ? 1 : 0;
  }
  const int nbad = __syncthreads_count(bad);
  const int nrep = __syncthreads_count(rep);
  return len_ok && nbad == 0 && tb >= lb + nrep;
}

__global__ void __launch_bounds__(1024)
    ctc_lattice_kernel(const float* __restrict__ emis,
                       const long* __restrict__ in_len,
                       const long* __restrict__ labels,
                       const long* __restrict__ lab_len,
                       float* __restrict__ alpha, float* __restrict__ beta,
                       float* __restrict__ nll, float* __restrict__ valid,
                       int Tn, int V, int L, int blank) {
  __shared__ int lab[kCtcMaxL + 1];
  __shared__ float buf[2][1024];
  const int b = blockIdx.x;
  const int dir = blockIdx.y;
  const int s = threadIdx.x;
  const int S = 2 * L + 1;
  int tb, lb;
  const bool len_ok = RowLengths(in_len, lab_len, b, Tn, L, &tb, &lb);

  const bool feasible =
      LabelsToLds(labels, b, s, V, L, blank, len_ok, tb, lb, lab);

  float* out = (dir ? beta : alpha) + (long)b * Tn * S;
  if (!feasible) {  // uniform over the workgroup
    for (long i = s; i < (long)Tn * S; i += blockDim.x) out[i] = 0.f;
    if (dir == 0 && s == 0) {
      nll[b] = 0.f;
      valid[b] = 0.f;
    }
    return;
  }

  const int sb = 2 * lb + 1;
  const bool active = s < sb;
  const bool odd = (s & 1) != 0;
  const int eidx = odd ? (s + 1) / 2 : 0;
  // Position the third predecessor comes from (two back in the direction
  // of travel), allowed only between different labels.
  bool skip = false;
  if (active && odd) {
    if (dir == 0) {
      skip = s >= 3 && lab[(s - 1) / 2] != lab[(s - 3) / 2];
    } else {
      skip = s + 2 < sb && lab[(s + 1) / 2] != lab[(s - 1) / 2];
    }
  }
  const int step = dir ? -1 : 1;      // neighbour offset in s is -step
  const int n1 = s - step, n2 = s - 2 * step;
  const bool has1 = active && n1 >= 0 && n1 < sb;
  const bool init = dir ? (s == sb - 1 || s == sb - 2) : (s == 0 || s == 1);
  const float* eb = emis + (long)b * Tn * (L + 1) + eidx;

  int t = dir ? tb - 1 : 0;
  float e_cur = active ? eb[(long)t * (L + 1)] : 0.f;
  for (int k = 0; k < tb; ++k, t += step) {
    float e_next = 0.f;
    if (active && k + 1 < tb) e_next = eb[(long)(t + step) * (L + 1)];
    float v = kNeg;
    if (active) {
      if (k == 0) {
        v = init ? e_cur : kNeg;
      } else {
        const float* prev = buf[(k - 1) & 1];
        const float p0 = prev[s];
        const float p1 = has1 ? prev[n1] : kNeg;
        const float p2 = skip ? prev[n2] : kNeg;
        const float l3 = Lse3(p0, p1, p2);
        v = l3 > kNegTest ? e_cur + l3 : kNeg;
      }
    }
    buf[k & 1][s] = v;
    if (s < S) out[(long)t * S + s] = v;
    e_cur = e_next;
    __syncthreads();
  }
  // Frames past the utterance's end.
  for (long i = (long)tb * S + s; i < (long)Tn * S; i += blockDim.x)
    out[i] = 0.f;
  if (dir == 0 && s == 0) {
    const float* last = buf[(tb - 1) & 1];
    const float a1 = last[sb - 1];
    const float a2 = sb >= 2 ? last[sb - 2] : kNeg;
    const float m = fmaxf(a1, a2);
    const float ll = m + logf(expf(a1 - m) + expf(a2 - m));
    const bool ok = m > kNegTest && isfinite(ll);
    nll[b] = ok ? -ll : 0.f;
    valid[b] = ok ? 1.f : 0.f;
  }
}

// ---- forced alignment: the best single path --------------------------------
// The alpha workgroup of ctc_lattice_kernel with max in place of logsumexp:
// one workgroup per utterance, one lane per position, the same prologue,
// LDS buffers and one barrier per frame. Each lane records which
// predecessor won (0 stay, 1 step, 2 skip; among equal values the smallest),
// and a wave packs its 64 two-bit choices into two __ballot masks that lane
// 0 stores as one 16-byte word pair: bp [B,T,W,2], W = waves per workgroup.
//
// After the loop thread 0 walks the masks back from the better of the two
// end positions (the last one on a tie) and writes the frame ids, and for
// every label its span [start, end) and the sum of its frames' log-probs.
// The masks it reads were stored by other waves of this workgroup, the last
// of them before the loop's final __syncthreads(). That barrier is a
// workgroup-scope release and acquire, which is all the hand-off needs: the
// waves of a workgroup run on one CU and share its write-through L1, which
// serves their accesses in order, so a load issued after the barrier sees a
// store issued before it; and no lane loaded these words before they were
// stored, so no older copy of them exists. No other workgroup reads or
// writes them in this launch. The same in-order path covers the one
// store-after-store case: a feasible row whose best score turns out not to
// be possible has the masks its loop stored overwritten with zeros by other
// lanes after that barrier, and the later store lands last.
//
// A row without an alignment, or whose best score is not above kNegTest,
// gets valid = 0, score = 0, frame_ids = -1, spans -1, token_logp = 0 and
// zero masks. Frames >= T_b get frame_ids = -1 and zero masks, label slots
// >= L_b get spans -1 and token_logp = 0.
//
// kLdsMasks keeps the masks in dynamic LDS, [Tn, W] word pairs, instead of
// the global workspace (bp is then unused): the walk's chain of dependent
// loads then runs at LDS latency. The host picks it when they fit.
template <bool kLdsMasks>
__global__ void __launch_bounds__(1024)
    ctc_viterbi_kernel(const float* __restrict__ emis,
                       const long* __restrict__ in_len,
                       const long* __restrict__ labels,
                       const long* __restrict__ lab_len, ulonglong2* bp,
                       long* __restrict__ frame_ids,
                       long* __restrict__ token_start,
                       long* __restrict__ token_end,
                       float* __restrict__ token_logp,
                       float* __restrict__ score, float* __restrict__ valid,
                       int Tn, int V, int L, int blank) {
  __shared__ int lab[kCtcMaxL + 1];
  __shared__ float buf[2][1024];
  extern __shared__ ulonglong2 lds_masks[];
  const int b = blockIdx.x;
  const int s = threadIdx.x;
  const int lane = s & (WAVE_SIZE - 1);
  const int wave = s / WAVE_SIZE;
  const int W = blockDim.x / WAVE_SIZE;
  int tb, lb;
  const bool len_ok = RowLengths(in_len, lab_len, b, Tn, L, &tb, &lb);
  const bool feasible =
      LabelsToLds(labels, b, s, V, L, blank, len_ok, tb, lb, lab);

  // [Tn, W] word pairs of this utterance.
  ulonglong2* bpw = kLdsMasks ? lds_masks : bp + (long)b * Tn * W;
  long* fid = frame_ids + (long)b * Tn;
  long* ts = token_start + (long)b * L;
  long* te = token_end + (long)b * L;
  float* tl = token_logp + (long)b * L;
  const ulonglong2 zero2 = make_ulonglong2(0ull, 0ull);

  float best = kNeg;
  bool end_last = true;
  const int sb = 2 * lb + 1;
  if (feasible) {  // uniform over the workgroup
    const bool active = s < sb;
    const bool odd = (s & 1) != 0;
    const bool has1 = active && s >= 1;
    const bool skip =
        active && odd && s >= 3 && lab[(s - 1) / 2] != lab[(s - 3) / 2];
    const float* eb = emis + (long)b * Tn * (L + 1) + (odd ? (s + 1) / 2 : 0);
    float e_cur = active ? eb[0] : 0.f;
    for (int t = 0; t < tb; ++t) {
      float e_next = 0.f;
      if (active && t + 1 < tb) e_next = eb[(long)(t + 1) * (L + 1)];
      float v = kNeg;
      int mv = 0;
      if (active) {
        if (t == 0) {
          v = s < 2 ? e_cur : kNeg;
        } else {
          const float* prev = buf[(t - 1) & 1];
          float m = prev[s];
          if (has1) {
            const float p1 = prev[s - 1];
            if (p1 > m) {
              m = p1;
              mv = 1;
            }
          }
          if (skip) {
            const float p2 = prev[s - 2];
            if (p2 > m) {
              m = p2;
              mv = 2;
            }
          }
          v = m > kNegTest ? e_cur + m : kNeg;
        }
      }
      buf[t & 1][s] = v;
      const unsigned long long m0 = __ballot(mv & 1);
      const unsigned long long m1 = __ballot(mv >> 1);
      if (lane == 0) bpw[(long)t * W + wave] = make_ulonglong2(m0, m1);
      e_cur = e_next;
      __syncthreads();
    }
    const float* last = buf[(tb - 1) & 1];
    const float a1 = last[sb - 1];
    const float a2 = sb >= 2 ? last[sb - 2] : kNeg;
    end_last = a1 >= a2;
    best = end_last ? a1 : a2;
  }

  if (!(best > kNegTest)) {  // uniform: no alignment
    if (!kLdsMasks)
      for (long i = s; i < (long)Tn * W; i += blockDim.x) bpw[i] = zero2;
    for (int t = s; t < Tn; t += blockDim.x) fid[t] = -1;
    for (int j = s; j < L; j += blockDim.x) {
      ts[j] = -1;
      te[j] = -1;
      tl[j] = 0.f;
    }
    if (s == 0) {
      score[b] = 0.f;
      valid[b] = 0.f;
    }
    return;
  }

  // Frames past the utterance's end and unused label slots.
  if (!kLdsMasks)
    for (long i = (long)tb * W + s; i < (long)Tn * W; i += blockDim.x)
      bpw[i] = zero2;
  for (int t = tb + s; t < Tn; t += blockDim.x) fid[t] = -1;
  for (int j = lb + s; j < L; j += blockDim.x) {
    ts[j] = -1;
    te[j] = -1;
    tl[j] = 0.f;
  }
  if (s != 0) return;

  // Backtrace. Every label position of a path from {0,1} to {sb-2,sb-1} is
  // visited, so every slot j < lb is stored exactly once.
  score[b] = best;
  valid[b] = 1.f;
  const float* er = emis + (long)b * Tn * (L + 1);
  int sc = end_last ? sb - 1 : sb - 2;
  int end = 0;
  float acc = 0.f;
  bool open = false;
  for (int t = tb - 1; t >= 0; --t) {
    const ulonglong2 w = bpw[(long)t * W + sc / WAVE_SIZE];
    const int bit = sc & (WAVE_SIZE - 1);
    const int mv = (int)((w.x >> bit) & 1) | ((int)((w.y >> bit) & 1) << 1);
    const int j = sc >> 1;  // label index of an odd position
    if (sc & 1) {
      fid[t] = lab[j];
      if (!open) {
        open = true;
        end = t + 1;
        acc = 0.f;
      }
      acc += er[(long)t * (L + 1) + j + 1];
      if (mv != 0 || t == 0) {  // leaving the label (frame 0 has no move)
        ts[j] = t;
        te[j] = end;
        tl[j] = acc;
        open = false;
      }
    } else {
      fid[t] = blank;
    }
    sc = max(sc - mv, 0);  // in range whatever the words hold
  }
}

// ---- pass 3: dlogits -------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kGradThreads)
    ctc_grad_kernel(const T* __restrict__ logits,
                    const long* __restrict__ in_len,
                    const long* __restrict__ labels,
                    const long* __restrict__ lab_len,
                    const float* __restrict__ lse, const float* __restrict__ emis,
                    const float* __restrict__ alpha,
                    const float* __restrict__ beta,
                    const float* __restrict__ nll,
                    const float* __restrict__ valid,
                    const float* __restrict__ gout, T* __restrict__ dlogits,
                    int Tn, int V, int L, int blank) {
  typedef Elem<T> El;
  __shared__ int lab[kCtcMaxL + 1];
  __shared__ float occ[kCtcMaxL + 1];
  __shared__ float red[kGradThreads / WAVE_SIZE];
  const long row = blockIdx.x;
  const int b = (int)(row / Tn);
  const int t = (int)(row % Tn);
  const int tid = threadIdx.x;
  int tb, lb;
  RowLengths(in_len, lab_len, b, Tn, L, &tb, &lb);
  const bool live = valid[b] != 0.f && t < tb;  // uniform over the workgroup
  const T* lr = logits + row * V;
  T* dr = dlogits + row * V;
  const float g = live ? gout[b] : 0.f;
  const float lse_r = live ? lse[row] : 0.f;

  // Dense part: g * softmax, or zeros.
  const bool same_phase =
      ((reinterpret_cast<uintptr_t>(lr) ^ reinterpret_cast<uintptr_t>(dr)) &
       15) == 0;
  const int head = same_phase ? HeadElems(dr, V) : V;
  const int nvec = (V - head) / El::kVec;
  for (int j = tid; j < head; j += kGradThreads)
    dr[j] = El::FromFloat(live ? g * expf(El::ToFloat(lr[j]) - lse_r) : 0.f);
  for (int i = tid; i < nvec; i += kGradThreads) {
    typename El::Vec o;
    if (live) {
      typename El::Vec v =
          *reinterpret_cast<const typename El::Vec*>(lr + head + i * El::kVec);
#pragma unroll
      for (int e = 0; e < El::kVec; ++e)
        o[e] = El::FromFloat(g * expf(El::ToFloat(v[e]) - lse_r));
    } else {
#pragma unroll
      for (int e = 0; e < El::kVec; ++e) o[e] = El::FromFloat(0.f);
    }
    *reinterpret_cast<typename El::Vec*>(dr + head + i * El::kVec) = o;
  }
  for (int j = head + nvec * El::kVec + tid; j < V; j += kGradThreads)
    dr[j] = El::FromFloat(live ? g * expf(El::ToFloat(lr[j]) - lse_r) : 0.f);
  if (!live) return;

  // Occupancy of every lattice position of this frame. valid[b] != 0
  // implies every label in [0, lb) is a non-blank id inside [0, V).
  const int S = 2 * L + 1;
  const float* ar = alpha + row * S;
  const float* br = beta + row * S;
  const float* er = emis + row * (L + 1);
  const float nll_b = nll[b];
  const float e0 = er[0];
  float blank_occ = 0.f;
  for (int i = tid; i <= lb; i += kGradThreads) {
    blank_occ += expf(ar[2 * i] + br[2 * i] - e0 + nll_b);
    if (i < lb) {
      lab[i] = (int)labels[(long)b * L + i];
      occ[i] = expf(ar[2 * i + 1] + br[2 * i + 1] - er[i + 1] + nll_b);
    }
  }
  // The barriers inside also order the dense stores above before the
  // overwrites below, and lab/occ before their readers.
  blank_occ = block_reduce_sum<kGradThreads / WAVE_SIZE>(blank_occ, red);
  if (tid == 0)
    dr[blank] = El::FromFloat(
        g * (expf(El::ToFloat(lr[blank]) - lse_r) - blank_occ));
  for (int i = tid; i < lb; i += kGradThreads) {
    const int mine = lab[i];
    bool first = true;
    float acc = 0.f;
    for (int j = 0; j < lb; ++j) {
      if (lab[j] == mine) {
        if (j < i) {
          first = false;
          break;
        }
        acc += occ[j];
      }
    }
    if (first)
      dr[mine] =
          El::FromFloat(g * (expf(El::ToFloat(lr[mine]) - lse_r) - acc));
  }
}

// ---- host ------------------------------------------------------------------
bool CudaContig(const torch::Tensor& t, torch::ScalarType dt) {
  return t.is_cuda() && t.is_contiguous() && t.scalar_type() == dt;
}

struct CtcShape {
  int B, T, V, L;
};

CtcShape CheckCtcInputs(const torch::Tensor& logits,
                        const torch::Tensor& logit_lengths,
                        const torch::Tensor& labels,
                        const torch::Tensor& label_lengths, int64_t blank) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() &&
                  logits.dim() == 3 &&
                  (logits.scalar_type() == torch::kBFloat16 ||
                   logits.scalar_type() == torch::kFloat32),
              "ctc: logits must be CUDA contiguous bf16 or fp32 [B,T,V]");
  const int64_t b = logits.size(0), t = logits.size(1), v = logits.size(2);
  TORCH_CHECK(b >= 1 && t >= 1, "ctc: B >= 1 and T >= 1");
  TORCH_CHECK(v >= 2, "ctc: V >= 2");
  TORCH_CHECK(b * t < (1LL << 31) && v < (1LL << 31),
              "ctc: B*T and V must fit in int32");
  TORCH_CHECK(blank >= 0 && blank < v, "ctc: blank_id must be in [0, V)");
  TORCH_CHECK(CudaContig(labels, torch::kInt64) && labels.dim() == 2 &&
                  labels.size(0) == b,
              "ctc: labels must be CUDA contiguous int64 [B,L]");
  const int64_t l = labels.size(1);
  TORCH_CHECK(l <= kCtcMaxL, "ctc: L=", l, " is over the supported limit ",
              kCtcMaxL);
  TORCH_CHECK(CudaContig(logit_lengths, torch::kInt64) &&
                  logit_lengths.dim() == 1 && logit_lengths.size(0) == b,
              "ctc: logit_lengths must be CUDA contiguous int64 [B]");
  TORCH_CHECK(CudaContig(label_lengths, torch::kInt64) &&
                  label_lengths.dim() == 1 && label_lengths.size(0) == b,
              "ctc: label_lengths must be CUDA contiguous int64 [B]");
  TORCH_CHECK(logits.get_device() == labels.get_device() &&
                  logits.get_device() == logit_lengths.get_device() &&
                  logits.get_device() == label_lengths.get_device(),
              "ctc: all inputs must be on one device");
  return {(int)b, (int)t, (int)v, (int)l};
}

void CheckF32(const torch::Tensor& x, std::vector<int64_t> shape,
              const torch::Tensor& like, const char* name) {
  TORCH_CHECK(CudaContig(x, torch::kFloat32) && x.sizes().vec() == shape &&
                  x.get_device() == like.get_device(),
              "ctc: ", name, " must be CUDA contiguous fp32 of the shape "
              "ctc_fwd returned");
}

// Pass 1 on `stream`: lse [B,T] and emis [B,T,L+1].
void LaunchRows(const torch::Tensor& logits,
                const torch::Tensor& logit_lengths,
                const torch::Tensor& labels,
                const torch::Tensor& label_lengths, torch::Tensor& lse,
                torch::Tensor& emis, const CtcShape& sh, int64_t blank,
                hipStream_t stream) {
  const long rows = (long)sh.B * sh.T;
  const dim3 rgrid(cdiv(rows, kRowWaves)), rblock(kRowWaves * WAVE_SIZE);
  if (logits.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(ctc_rows_kernel<unsigned short>, rgrid, rblock, 0,
                       stream, (const unsigned short*)logits.data_ptr(),
                       logit_lengths.data_ptr<long>(),
                       labels.data_ptr<long>(),
                       label_lengths.data_ptr<long>(), lse.data_ptr<float>(),
                       emis.data_ptr<float>(), sh.B, sh.T, sh.V, sh.L,
                       (int)blank);
  } else {
    hipLaunchKernelGGL(ctc_rows_kernel<float>, rgrid, rblock, 0, stream,
                       logits.data_ptr<float>(),
                       logit_lengths.data_ptr<long>(),
                       labels.data_ptr<long>(),
                       label_lengths.data_ptr<long>(), lse.data_ptr<float>(),
                       emis.data_ptr<float>(), sh.B, sh.T, sh.V, sh.L,
                       (int)blank);
  }
}

}  // namespace

int64_t ctc_max_label_len() { return kCtcMaxL; }

// -> {nll [B], valid [B], lse [B,T], emis [B,T,L+1], alpha, beta [B,T,2L+1]}
std::vector<torch::Tensor> ctc_fwd(torch::Tensor logits,
                                   torch::Tensor logit_lengths,
                                   torch::Tensor labels,
                                   torch::Tensor label_lengths,
                                   int64_t blank) {
  const CtcShape sh =
      CheckCtcInputs(logits, logit_lengths, labels, label_lengths, blank);
  const int B = sh.B, T = sh.T, V = sh.V, L = sh.L, S = 2 * sh.L + 1;
  auto opts = logits.options().dtype(torch::kFloat32);
  auto nll = torch::empty({B}, opts);
  auto valid = torch::empty({B}, opts);
  auto lse = torch::empty({B, T}, opts);
  auto emis = torch::empty({B, T, L + 1}, opts);
  auto alpha = torch::empty({B, T, S}, opts);
  auto beta = torch::empty({B, T, S}, opts);
  auto stream = at::cuda::getCurrentCUDAStream();
  LaunchRows(logits, logit_lengths, labels, label_lengths, lse, emis, sh,
             blank, stream);
  const int threads = cdiv(S, WAVE_SIZE) * WAVE_SIZE;  // <= 1024
  hipLaunchKernelGGL(ctc_lattice_kernel, dim3(B, 2), dim3(threads), 0, stream,
                     emis.data_ptr<float>(), logit_lengths.data_ptr<long>(),
                     labels.data_ptr<long>(), label_lengths.data_ptr<long>(),
                     alpha.data_ptr<float>(), beta.data_ptr<float>(),
                     nll.data_ptr<float>(), valid.data_ptr<float>(), T, V, L,
                     (int)blank);
  return {nll, valid, lse, emis, alpha, beta};
}

torch::Tensor ctc_bwd(torch::Tensor logits, torch::Tensor logit_lengths,
                      torch::Tensor labels, torch::Tensor label_lengths,
                      torch::Tensor lse, torch::Tensor emis,
                      torch::Tensor alpha, torch::Tensor beta,
                      torch::Tensor nll, torch::Tensor valid,
                      torch::Tensor gout, int64_t blank) {
  const CtcShape sh =
      CheckCtcInputs(logits, logit_lengths, labels, label_lengths, blank);
  const int64_t B = sh.B, T = sh.T, L = sh.L, S = 2 * sh.L + 1;
  CheckF32(lse, {B, T}, logits, "lse");
  CheckF32(emis, {B, T, L + 1}, logits, "emis");
  CheckF32(alpha, {B, T, S}, logits, "alpha");
  CheckF32(beta, {B, T, S}, logits, "beta");
  CheckF32(nll, {B}, logits, "nll");
  CheckF32(valid, {B}, logits, "valid");
  CheckF32(gout, {B}, logits, "gout");
  auto dlogits = torch::empty_like(logits);
  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 grid((unsigned)(B * T)), block(kGradThreads);
  if (logits.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(
        ctc_grad_kernel<unsigned short>, grid, block, 0, stream,
        (const unsigned short*)logits.data_ptr(),
        logit_lengths.data_ptr<long>(), labels.data_ptr<long>(),
        label_lengths.data_ptr<long>(), lse.data_ptr<float>(),
        emis.data_ptr<float>(), alpha.data_ptr<float>(),
        beta.data_ptr<float>(), nll.data_ptr<float>(),
        valid.data_ptr<float>(), gout.data_ptr<float>(),
        (unsigned short*)dlogits.data_ptr(), sh.T, sh.V, sh.L, (int)blank);
  } else {
    hipLaunchKernelGGL(
        ctc_grad_kernel<float>, grid, block, 0, stream,
        logits.data_ptr<float>(), logit_lengths.data_ptr<long>(),
        labels.data_ptr<long>(), label_lengths.data_ptr<long>(),
        lse.data_ptr<float>(), emis.data_ptr<float>(),
        alpha.data_ptr<float>(), beta.data_ptr<float>(),
        nll.data_ptr<float>(), valid.data_ptr<float>(),
        gout.data_ptr<float>(), dlogits.data_ptr<float>(), sh.T, sh.V, sh.L,
        (int)blank);
  }
  return dlogits;
}

// -> {frame_ids [B,T] i64, token_start, token_end [B,L] i64,
//     token_logp [B,L], score [B], valid [B]}. lds_masks = false keeps the
// backpointer masks in the global workspace whatever the shape.
std::vector<torch::Tensor> ctc_align(torch::Tensor logits,
                                     torch::Tensor logit_lengths,
                                     torch::Tensor labels,
                                     torch::Tensor label_lengths,
                                     int64_t blank, bool lds_masks) {
  const CtcShape sh =
      CheckCtcInputs(logits, logit_lengths, labels, label_lengths, blank);
  const int B = sh.B, T = sh.T, L = sh.L, S = 2 * sh.L + 1;
  const int waves = cdiv(S, WAVE_SIZE);  // <= 16
  // Masks in LDS when the caller allows it and all T frames fit.
  const long mask_bytes = (long)T * waves * sizeof(ulonglong2);
  const bool in_lds = lds_masks && mask_bytes <= kLdsMaskBytes;
  auto f32 = logits.options().dtype(torch::kFloat32);
  auto i64 = logits.options().dtype(torch::kInt64);
  auto lse = torch::empty({B, T}, f32);
  auto emis = torch::empty({B, T, L + 1}, f32);
  auto bp = torch::empty({in_lds ? 0 : B, T, waves, 2}, i64);
  auto frame_ids = torch::empty({B, T}, i64);
  auto token_start = torch::empty({B, L}, i64);
  auto token_end = torch::empty({B, L}, i64);
  auto token_logp = torch::empty({B, L}, f32);
  auto score = torch::empty({B}, f32);
  auto valid = torch::empty({B}, f32);
  auto stream = at::cuda::getCurrentCUDAStream();
  LaunchRows(logits, logit_lengths, labels, label_lengths, lse, emis, sh,
             blank, stream);
  hipLaunchKernelGGL(in_lds ? ctc_viterbi_kernel<true>
                            : ctc_viterbi_kernel<false>,
                     dim3(B), dim3(waves * WAVE_SIZE),
                     in_lds ? (size_t)mask_bytes : 0, stream,
                     emis.data_ptr<float>(),
                     logit_lengths.data_ptr<long>(), labels.data_ptr<long>(),
                     label_lengths.data_ptr<long>(),
                     reinterpret_cast<ulonglong2*>(bp.data_ptr()),
                     frame_ids.data_ptr<long>(), token_start.data_ptr<long>(),
                     token_end.data_ptr<long>(),
                     token_logp.data_ptr<float>(), score.data_ptr<float>(),
                     valid.data_ptr<float>(), T, sh.V, L, (int)blank);
  return {frame_ids, token_start, token_end, token_logp, score, valid};
}
