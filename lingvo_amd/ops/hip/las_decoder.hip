// Fused LAS attention-decoder step kernels for gfx950 (SURVEY K4/K11;
// reference decode-path einsums lingvo/core/batch_major_attention.py:920,
// 1069 and tasks/asr/decoder.py teacher-forced loop).
//
// The teacher-forced recurrence is latency-bound: library GEMMs at M=B
// (=128) occupy ~10 of 256 CUs and cost ~107 us each. These kernels
// replace them:
//  - smallm_gemm: C[M,N] (+)= alpha * A[M,K] @ Wt[N,K]^T (+ pre): MFMA
//    16x16x32, ONE workgroup per 16-column n-tile so the whole chip is
//    busy; A stays L2-resident across workgroups. ~5-15 us per call.
//  - attend_fwd/attend_bwd: the dot-attention step (logits + masked
//    softmax + context, and its full backward incl. dEnc accumulation)
//    as one kernel per direction, one workgroup per batch row.
//  - attend_step_fwd/attend_step_bwd/attend_denc: the same step reading
//    enc once per kernel and leaving dEnc out; dEnc of the whole
//    recurrence is one contraction over the step index after the loop.
//
// Consumed by models/asr.py DecoderRecurrence (custom autograd Function
// that also batches all weight-gradient GEMMs across the L timesteps).

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <atomic>
#include <climits>

#include "common.h"
#include "host_checks.h"
#include "mfma.h"
#include "tile_gemm.h"

namespace {

// ---------------------------------------------------------------------------
// smallm_gemm: out[M,N] = alpha * (A[M,K] @ Wt[N,K]^T) + pre
//   pre_mode: 0 none, 1 row-vector [N], 2 full matrix [M,N],
//             3 accumulate into existing out
// A row-major [M, K] with row stride lda (a column slice of a wider
// matrix is fine), Wt row-major [N, ldw] with the mathematical W^T in its
// first K columns. K % 32 == 0.
// Grid: (ceil(N/16), ceil(M/128)); block 256 = 4 waves; wave w owns a
// quarter of K for all 8 m-tiles of its 128-row m-block and walks it with
// the shared K loop of tile_gemm.h.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void smallm_gemm_kernel(
    const unsigned short* __restrict__ a, const unsigned short* __restrict__ wt,
    const unsigned short* __restrict__ pre, unsigned short* __restrict__ out,
    int m, int n, int k, long lda, long ldw, float alpha, int pre_mode) {
  // K-SPLIT layout: every wave computes ALL 8 m-tiles over its quarter
  // of K (no per-iteration block syncs; the serial K chain is 4x
  // shorter than an M-split), then waves 1-3 spill partials to LDS and
  // wave 0 reduces + writes. The recurrence calls this back-to-back
  // with dependent inputs, so per-call LATENCY is the metric.
  const int nt = blockIdx.x;          // n-tile (16 cols)
  const int col0 = nt * 16;
  const int m0 = blockIdx.y * 128;    // m-block (rows handled here)
  const StepThread th = step_thread();
  const int wid = th.wid, g = th.g, cl = th.cl;
  const int col = col0 + cl;
  const bool col_ok = col < n;

  constexpr int MT = 8;               // m-tiles per block (128 rows)
  __shared__ float red[3][128][16];   // waves 1-3 partials

  const int kq = (k / 32 + 3) / 4 * 32;  // per-wave K quota (mult of 32)
  const int k_lo = wid * kq;
  const int k_hi = min(k, k_lo + kq);

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};

  // Rows beyond M and columns beyond N re-read the last valid one instead
  // of branching to a zero fragment: an output element depends on its own
  // A row and Wt row alone, and those elements are never stored.
  const unsigned short* brow =
      wt + (long)min(col, n - 1) * ldw + k_lo + g * 8;
  const unsigned short* arow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    arow[mt] = a + (long)min(m0 + mt * 16 + cl, m - 1) * lda + k_lo + g * 8;
  }
  tile_gemm<MT>(arow, brow, k_hi - k_lo, acc);

  // Cross-wave reduction: C layout row = mt*16 + g*4 + r, col = cl.
  if (wid > 0) park_acc<MT>(red[wid - 1], g, cl, acc);
  __syncthreads();
  if (wid != 0) return;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int lrow = mt * 16 + g * 4 + r;  // LDS-local row
      const int row = m0 + lrow;
      if (row >= m || !col_ok) continue;
      float v = (acc[mt][r] + red[0][lrow][cl] + red[1][lrow][cl] +
                 red[2][lrow][cl]) * alpha;
      long off = (long)row * n + col;
      if (pre_mode == 1) {
        v += bf16_bits_to_float(pre[col]);
      } else if (pre_mode == 2) {
        v += bf16_bits_to_float(pre[off]);
      } else if (pre_mode == 3) {
        v += bf16_bits_to_float(out[off]);
      }
      out[off] = float_to_bf16_bits(v);
    }
  }
}

// ---------------------------------------------------------------------------
// attend_fwd: per batch row b:
//   logits[s] = scale * dot(q[b], enc[b,s]) + (-1e30 if padded)
//   probs = softmax(logits); ctx[b] = sum_s probs[s] * enc[b,s]
// q [B, D] bf16; enc [B, S, D] bf16; pad [B, S] float; out probs [B, S]
// fp32, ctx [B, D] bf16. Grid: B blocks of 256 (4 waves).
// Dynamic LDS: q (D bf16) + logits (S f32) + 4*D f32 ctx partials.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attend_fwd_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ enc,
    const float* __restrict__ pad, float* __restrict__ probs,
    unsigned short* __restrict__ ctx, int b_total, int s_len, int d,
    float scale) {
  const int b = blockIdx.x;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  extern __shared__ char smem[];
  unsigned short* q_s = (unsigned short*)smem;            // [D]
  float* logit_s = (float*)(q_s + d);                     // [S]
  float* ctx_s = logit_s + s_len;                         // [4][D]
  float* red = ctx_s + 4 * d;                             // [4]

  for (int i = threadIdx.x; i < d; i += 256) q_s[i] = q[(long)b * d + i];
  __syncthreads();

  // Cache this lane's q slice in registers (vectorized over the s loop).
  constexpr int MAXDV = 4;  // supports d up to 2048
  const int ndv = d / (WAVE_SIZE * 8) + (d % (WAVE_SIZE * 8) ? 1 : 0);
  float qreg[MAXDV][8];
  for (int v = 0; v < ndv; ++v) {
    const int i = lane * 8 + v * WAVE_SIZE * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      qreg[v][j] = i < d ? bf16_bits_to_float(q_s[i + j]) : 0.f;
    }
  }

  // Pass 1: logits. Each wave processes 4 consecutive s per iteration
  // (independent loads pipeline the HBM/L2 latency that a one-s-at-a-
  // time loop serializes).
  const unsigned short* eb = enc + (long)b * s_len * d;
  for (int s0 = wid * 4; s0 < s_len; s0 += 16) {
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < ndv; ++v) {
      const int i = lane * 8 + v * WAVE_SIZE * 8;
      if (i < d) {
        bf16x8 ev[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (s0 + u < s_len) {
            ev[u] = load_bf16x8_bits(eb + (long)(s0 + u) * d + i);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (s0 + u < s_len) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              part[u] += qreg[v][j] * (float)ev[u][j];
            }
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (s0 + u < s_len) {
        float t = wave_reduce_sum(part[u]);
        if (lane == 0) {
          logit_s[s0 + u] = t * scale +
              (pad[(long)b * s_len + s0 + u] > 0.5f ? -1e30f : 0.f);
        }
      }
    }
  }
  __syncthreads();

  // Softmax over logits (block-wide).
  float lmax = -1e30f;
  for (int s = threadIdx.x; s < s_len; s += 256) {
    lmax = fmaxf(lmax, logit_s[s]);
  }
  lmax = wave_reduce_max(lmax);
  if (lane == 0) red[wid] = lmax;
  __syncthreads();
  lmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float lsum = 0.f;
  for (int s = threadIdx.x; s < s_len; s += 256) {
    float e = __expf(logit_s[s] - lmax);
    logit_s[s] = e;
    lsum += e;
  }
  lsum = wave_reduce_sum(lsum);
  __syncthreads();
  if (lane == 0) red[wid] = lsum;
  __syncthreads();
  lsum = red[0] + red[1] + red[2] + red[3];
  const float inv = lsum > 0.f ? 1.f / lsum : 0.f;

  // Pass 2: probs out + ctx accumulation (per-wave private partials).
  for (int i = threadIdx.x; i < 4 * d; i += 256) ctx_s[i] = 0.f;
  __syncthreads();
  float* my_ctx = ctx_s + wid * d;
  for (int s0 = wid * 4; s0 < s_len; s0 += 16) {
    float pv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      pv[u] = s0 + u < s_len ? logit_s[s0 + u] * inv : 0.f;
      if (lane == 0 && s0 + u < s_len) {
        probs[(long)b * s_len + s0 + u] = pv[u];
      }
    }
    for (int v = 0; v < ndv; ++v) {
      const int i = lane * 8 + v * WAVE_SIZE * 8;
      if (i < d) {
        bf16x8 ev[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (s0 + u < s_len) {
            ev[u] = load_bf16x8_bits(eb + (long)(s0 + u) * d + i);
          }
        }
        float accv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (s0 + u < s_len) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              accv[j] += pv[u] * (float)ev[u][j];
            }
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          my_ctx[i + j] += accv[j];
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < d; i += 256) {
    ctx[(long)b * d + i] = float_to_bf16_bits(
        ctx_s[i] + ctx_s[d + i] + ctx_s[2 * d + i] + ctx_s[3 * d + i]);
  }
}

// ---------------------------------------------------------------------------
// attend_bwd: per batch row b, given dctx [B,D] (bf16), probs [B,S] f32,
// q [B,D], enc:
//   dprobs[s] = dot(dctx, enc[b,s])
//   t = sum_s probs[s]*dprobs[s];  dl[s] = probs[s]*(dprobs[s]-t)*scale
//   dq[b] = sum_s dl[s]*enc[b,s]
//   denc[b,s] += dl[s]*q[b] + probs[s]*dctx      (fp32 accumulation)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attend_bwd_kernel(
    const unsigned short* __restrict__ dctx,
    const float* __restrict__ probs, const unsigned short* __restrict__ q,
    const unsigned short* __restrict__ enc, unsigned short* __restrict__ dq,
    float* __restrict__ denc, int b_total, int s_len, int d, float scale) {
  const int b = blockIdx.x;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  extern __shared__ char smem[];
  unsigned short* dctx_s = (unsigned short*)smem;         // [D]
  unsigned short* q_s = dctx_s + d;                       // [D]
  float* dl_s = (float*)(q_s + d);                        // [S]
  float* dq_s = dl_s + s_len;                             // [4][D]
  float* red = dq_s + 4 * d;                              // [4]

  for (int i = threadIdx.x; i < d; i += 256) {
    dctx_s[i] = dctx[(long)b * d + i];
    q_s[i] = q[(long)b * d + i];
  }
  __syncthreads();

  // Per-lane register caches of dctx and q slices.
  constexpr int MAXDV = 4;
  const int ndv = d / (WAVE_SIZE * 8) + (d % (WAVE_SIZE * 8) ? 1 : 0);
  float dcreg[MAXDV][8], qreg[MAXDV][8];
  for (int v = 0; v < ndv; ++v) {
    const int i = lane * 8 + v * WAVE_SIZE * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      dcreg[v][j] = i < d ? bf16_bits_to_float(dctx_s[i + j]) : 0.f;
      qreg[v][j] = i < d ? bf16_bits_to_float(q_s[i + j]) : 0.f;
    }
  }

  // Pass 1: dprobs (stored to dl_s) + t reduction.
  const unsigned short* eb = enc + (long)b * s_len * d;
  const float* pb = probs + (long)b * s_len;
  for (int s0 = wid * 4; s0 < s_len; s0 += 16) {
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    for (int v = 0; v < ndv; ++v) {
      const int i = lane * 8 + v * WAVE_SIZE * 8;
      if (i < d) {
        bf16x8 ev[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (s0 + u < s_len) {
            ev[u] = load_bf16x8_bits(eb + (long)(s0 + u) * d + i);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (s0 + u < s_len) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              part[u] += dcreg[v][j] * (float)ev[u][j];
            }
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (s0 + u < s_len) {
        float t = wave_reduce_sum(part[u]);
        if (lane == 0) dl_s[s0 + u] = t;
      }
    }
  }
  __syncthreads();
  float t_part = 0.f;
  for (int s = threadIdx.x; s < s_len; s += 256) {
    t_part += pb[s] * dl_s[s];
  }
  t_part = wave_reduce_sum(t_part);
  if (lane == 0) red[wid] = t_part;
  __syncthreads();
  const float t = red[0] + red[1] + red[2] + red[3];

  // dl[s] = probs[s] * (dprobs[s] - t) * scale.
  __syncthreads();
  for (int s = threadIdx.x; s < s_len; s += 256) {
    dl_s[s] = pb[s] * (dl_s[s] - t) * scale;
  }
  __syncthreads();

  // Pass 2: dq partials + denc writes.
  for (int i = threadIdx.x; i < 4 * d; i += 256) dq_s[i] = 0.f;
  __syncthreads();
  float* my_dq = dq_s + wid * d;
  float* db = denc + (long)b * s_len * d;
  for (int s0 = wid * 4; s0 < s_len; s0 += 16) {
    float dlv[4], ppv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      dlv[u] = s0 + u < s_len ? dl_s[s0 + u] : 0.f;
      ppv[u] = s0 + u < s_len ? pb[s0 + u] : 0.f;
    }
    for (int v = 0; v < ndv; ++v) {
      const int i = lane * 8 + v * WAVE_SIZE * 8;
      if (i < d) {
        bf16x8 ev[4];
        floatx4 lo[4], hi[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (s0 + u < s_len) {
            ev[u] = load_bf16x8_bits(eb + (long)(s0 + u) * d + i);
            floatx4* dbv =
                reinterpret_cast<floatx4*>(db + (long)(s0 + u) * d + i);
            lo[u] = dbv[0];
            hi[u] = dbv[1];
          }
        }
        float dqacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (s0 + u < s_len) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              dqacc[j] += dlv[u] * (float)ev[u][j];
              lo[u][j] += dlv[u] * qreg[v][j] + ppv[u] * dcreg[v][j];
            }
#pragma unroll
            for (int j = 4; j < 8; ++j) {
              dqacc[j] += dlv[u] * (float)ev[u][j];
              hi[u][j - 4] += dlv[u] * qreg[v][j] + ppv[u] * dcreg[v][j];
            }
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (s0 + u < s_len) {
            floatx4* dbv =
                reinterpret_cast<floatx4*>(db + (long)(s0 + u) * d + i);
            dbv[0] = lo[u];
            dbv[1] = hi[u];
          }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          my_dq[i + j] += dqacc[j];
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < d; i += 256) {
    dq[(long)b * d + i] = float_to_bf16_bits(
        dq_s[i] + dq_s[d + i] + dq_s[2 * d + i] + dq_s[3 * d + i]);
  }
}


// ---------------------------------------------------------------------------
// Deferred-dEnc route: attend_step_fwd / attend_step_bwd / attend_denc.
//
// The step kernels read enc ONCE. One workgroup per batch row, NW waves,
// each wave streams U rows of enc per iteration with the whole row slice
// held in registers (NDV 512-column slices of 8 bf16 per lane), so the
// dot product and the weighted accumulation use the same load.
// ---------------------------------------------------------------------------

// U rows x NDV slices of enc for this lane; rows past s_len and columns
// past d read nothing and hold zeros.
template <int NDV, int U>
__device__ __forceinline__ void load_enc_rows(
    const unsigned short* __restrict__ eb, int s0, int s_len, int d, int lane,
    bf16x8 (&ev)[U][NDV]) {
  const float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const bf16x8 zero = pack_bf16x8(z);
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int v = 0; v < NDV; ++v) {
      const int i = lane * 8 + v * WAVE_SIZE * 8;
      ev[u][v] = (s0 + u < s_len && i < d)
                     ? load_bf16x8_bits(eb + (long)(s0 + u) * d + i)
                     : zero;
    }
  }
}

// attend_step_fwd: attend_fwd with one pass over enc. Every wave keeps a
// running max and an fp32 context partial rescaled to it (online softmax);
// the raw logits go to LDS, and probs come from them with the final max
// and sum exactly as in attend_fwd. ctx is written as fp32 and as bf16.
// Dynamic LDS: logits (S f32) + NW*D f32 partials + NW f32.
template <int NDV, int U, int NW>
__global__ __launch_bounds__(NW * WAVE_SIZE) void attend_step_fwd_kernel(
    const unsigned short* __restrict__ q, const unsigned short* __restrict__ enc,
    const float* __restrict__ pad, float* __restrict__ probs,
    unsigned short* __restrict__ ctx, float* __restrict__ ctx32, int s_len,
    int d, float scale) {
  constexpr int NT = NW * WAVE_SIZE;
  const int b = blockIdx.x;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  extern __shared__ char smem[];
  float* logit_s = (float*)smem;                          // [S]
  float* ctx_s = logit_s + s_len;                         // [NW][D]
  float* red = ctx_s + NW * d;                            // [NW]

  float qreg[NDV][8];
#pragma unroll
  for (int v = 0; v < NDV; ++v) {
    const int i = lane * 8 + v * WAVE_SIZE * 8;
    if (i < d) {
      bf16x8 qv = load_bf16x8_bits(q + (long)b * d + i);
#pragma unroll
      for (int j = 0; j < 8; ++j) qreg[v][j] = (float)qv[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) qreg[v][j] = 0.f;
    }
  }

  const unsigned short* eb = enc + (long)b * s_len * d;
  const float* padb = pad + (long)b * s_len;
  float m = -1e30f;
  float acc[NDV][8];
#pragma unroll
  for (int v = 0; v < NDV; ++v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[v][j] = 0.f;
  }
  for (int s0 = wid * U; s0 < s_len; s0 += NW * U) {
    bf16x8 ev[U][NDV];
    load_enc_rows<NDV, U>(eb, s0, s_len, d, lane, ev);
    // Rows past s_len are masked like padded ones: their weight stays
    // <= 1 whatever the running max is, and their ev is zero.
    float mask[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      mask[u] = (s0 + u >= s_len || padb[s0 + u] > 0.5f) ? -1e30f : 0.f;
    }
    float lg[U];
    float mnew = m;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float part = 0.f;
#pragma unroll
      for (int v = 0; v < NDV; ++v) {
#pragma unroll
        for (int j = 0; j < 8; ++j) part += qreg[v][j] * (float)ev[u][v][j];
      }
      lg[u] = wave_reduce_sum(part) * scale + mask[u];
      if (s0 + u < s_len) {
        mnew = fmaxf(mnew, lg[u]);
        if (lane == 0) logit_s[s0 + u] = lg[u];
      }
    }
    const float f = __expf(m - mnew);
    m = mnew;
#pragma unroll
    for (int v = 0; v < NDV; ++v) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[v][j] *= f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float p = __expf(lg[u] - mnew);
#pragma unroll
      for (int v = 0; v < NDV; ++v) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[v][j] += p * (float)ev[u][v][j];
      }
    }
  }
  if (lane == 0) red[wid] = m;
  __syncthreads();
  float lmax = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) lmax = fmaxf(lmax, red[w]);
  {
    const float wgt = __expf(m - lmax);
#pragma unroll
    for (int v = 0; v < NDV; ++v) {
      const int i = lane * 8 + v * WAVE_SIZE * 8;
      if (i < d) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ctx_s[wid * d + i + j] = acc[v][j] * wgt;
      }
    }
  }
  // Softmax over the LDS logits (block-wide), as in attend_fwd.
  float lsum = 0.f;
  for (int s = threadIdx.x; s < s_len; s += NT) {
    float e = __expf(logit_s[s] - lmax);
    logit_s[s] = e;
    lsum += e;
  }
  lsum = wave_reduce_sum(lsum);
  __syncthreads();  // every thread has read red[] as the max
  if (lane == 0) red[wid] = lsum;
  __syncthreads();
  lsum = 0.f;
#pragma unroll
  for (int w = 0; w < NW; ++w) lsum += red[w];
  const float inv = lsum > 0.f ? 1.f / lsum : 0.f;
  for (int s = threadIdx.x; s < s_len; s += NT) {
    probs[(long)b * s_len + s] = logit_s[s] * inv;
  }
  for (int i = threadIdx.x; i < d; i += NT) {
    float c = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) c += ctx_s[w * d + i];
    c *= inv;
    ctx32[(long)b * d + i] = c;
    ctx[(long)b * d + i] = float_to_bf16_bits(c);
  }
}

// attend_step_bwd: per batch row b, with dctx = bf16(dctx_a + dctx_b)
// (dctx_b optional, row stride ldb) stored to dctx_out:
//   t = dot(dctx, ctx32[b])          (= sum_s probs[s]*dprobs[s])
//   dprobs[s] = dot(dctx, enc[b,s]); dl[s] = probs[s]*(dprobs[s]-t)*scale
//   dq[b] = sum_s dl[s]*enc[b,s]
// dl goes to dl_out for attend_denc; enc is read once and dEnc is not
// touched. Dynamic LDS: dctx (D f32) + NW*D f32 partials + NW f32.
template <int NDV, int U, int NW>
__global__ __launch_bounds__(NW * WAVE_SIZE) void attend_step_bwd_kernel(
    const unsigned short* __restrict__ dctx_a,
    const unsigned short* __restrict__ dctx_b, long ldb,
    const float* __restrict__ probs, const float* __restrict__ ctx32,
    const unsigned short* __restrict__ enc,
    unsigned short* __restrict__ dctx_out, float* __restrict__ dl_out,
    unsigned short* __restrict__ dq, int s_len, int d, float scale) {
  constexpr int NT = NW * WAVE_SIZE;
  const int b = blockIdx.x;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  extern __shared__ char smem[];
  float* dc_s = (float*)smem;                             // [D]
  float* dq_s = dc_s + d;                                 // [NW][D]
  float* red = dq_s + NW * d;                             // [NW]

  float t_part = 0.f;
  for (int i = threadIdx.x; i < d; i += NT) {
    unsigned short bits = dctx_a[(long)b * d + i];
    if (dctx_b != nullptr) {
      bits = float_to_bf16_bits(bf16_bits_to_float(bits) +
                                bf16_bits_to_float(dctx_b[(long)b * ldb + i]));
    }
    dctx_out[(long)b * d + i] = bits;
    const float v = bf16_bits_to_float(bits);
    dc_s[i] = v;
    t_part += v * ctx32[(long)b * d + i];
  }
  const float t = block_reduce_sum<NW>(t_part, red);  // syncs: dc_s visible

  float dcreg[NDV][8];
#pragma unroll
  for (int v = 0; v < NDV; ++v) {
    const int i = lane * 8 + v * WAVE_SIZE * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) dcreg[v][j] = i < d ? dc_s[i + j] : 0.f;
  }

  const unsigned short* eb = enc + (long)b * s_len * d;
  const float* pb = probs + (long)b * s_len;
  float* dlb = dl_out + (long)b * s_len;
  float acc[NDV][8];
#pragma unroll
  for (int v = 0; v < NDV; ++v) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[v][j] = 0.f;
  }
  for (int s0 = wid * U; s0 < s_len; s0 += NW * U) {
    bf16x8 ev[U][NDV];
    load_enc_rows<NDV, U>(eb, s0, s_len, d, lane, ev);
    float pv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) pv[u] = s0 + u < s_len ? pb[s0 + u] : 0.f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float part = 0.f;
#pragma unroll
      for (int v = 0; v < NDV; ++v) {
#pragma unroll
        for (int j = 0; j < 8; ++j) part += dcreg[v][j] * (float)ev[u][v][j];
      }
      const float dlv = pv[u] * (wave_reduce_sum(part) - t) * scale;
      if (lane == u && s0 + u < s_len) dlb[s0 + u] = dlv;
#pragma unroll
      for (int v = 0; v < NDV; ++v) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[v][j] += dlv * (float)ev[u][v][j];
      }
    }
  }
#pragma unroll
  for (int v = 0; v < NDV; ++v) {
    const int i = lane * 8 + v * WAVE_SIZE * 8;
    if (i < d) {
#pragma unroll
      for (int j = 0; j < 8; ++j) dq_s[wid * d + i + j] = acc[v][j];
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < d; i += NT) {
    float c = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) c += dq_s[w * d + i];
    dq[(long)b * d + i] = float_to_bf16_bits(c);
  }
}

// attend_denc: dEnc of the whole recurrence, once after the loop:
//   denc[b,s,:] = sum_l dl[l,b,s]*q[l,b,:] + probs[l,b,s]*dctx[l,b,:]
// Grid: (B * ceil(S/32), ceil(D/512)); block 256 = 4 waves. A workgroup
// owns 32 rows s of one batch row b and 512 columns; wave w owns rows
// 8w..8w+7, a lane owns 8 columns of each, 64 fp32 accumulators. The
// per-row scalars (dl, probs) of 64 steps l at a time are staged in LDS and
// read as wave-wide broadcasts; the q / dctx rows come from L2. The sum
// over l runs in a fixed order in fp32 and every element is stored once.
constexpr int kDencRows = 8;                 // rows per wave
constexpr int kDencTile = 4 * kDencRows;     // rows per workgroup
constexpr int kDencSteps = 64;               // steps l staged per LDS fill

__device__ __forceinline__ void store_denc(float* p, const float* a) {
  floatx4* pv = reinterpret_cast<floatx4*>(p);
  pv[0] = floatx4{a[0], a[1], a[2], a[3]};
  pv[1] = floatx4{a[4], a[5], a[6], a[7]};
}

__device__ __forceinline__ void store_denc(unsigned short* p, const float* a) {
  ushortx8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = float_to_bf16_bits(a[j]);
  *reinterpret_cast<ushortx8*>(p) = o;
}

template <typename OutT>
__global__ __launch_bounds__(256) void attend_denc_kernel(
    const float* __restrict__ dl, const float* __restrict__ probs,
    const unsigned short* __restrict__ qs,
    const unsigned short* __restrict__ dctx, OutT* __restrict__ out,
    int l_total, int b_total, int s_len, int d, int s_tiles) {
  const int b = blockIdx.x / s_tiles;
  const int s_base = (blockIdx.x % s_tiles) * kDencTile;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int c0 = blockIdx.y * WAVE_SIZE * 8 + lane * 8;
  __shared__ float sc[kDencSteps][kDencTile][2];          // {dl, probs}

  float acc[kDencRows][8];
#pragma unroll
  for (int r = 0; r < kDencRows; ++r) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[r][j] = 0.f;
  }
  for (int l0 = 0; l0 < l_total; l0 += kDencSteps) {
    __syncthreads();
    for (int idx = threadIdx.x; idx < kDencSteps * kDencTile; idx += 256) {
      const int ll = idx / kDencTile, r = idx % kDencTile;
      const int l = l0 + ll, s = s_base + r;
      const bool ok = l < l_total && s < s_len;
      const long off = ((long)l * b_total + b) * s_len + s;
      sc[ll][r][0] = ok ? dl[off] : 0.f;
      sc[ll][r][1] = ok ? probs[off] : 0.f;
    }
    __syncthreads();
    if (c0 < d) {
      const int l_cnt = min(kDencSteps, l_total - l0);
#pragma unroll 4
      for (int ll = 0; ll < l_cnt; ++ll) {
        const long off = ((long)(l0 + ll) * b_total + b) * d + c0;
        const bf16x8 qv = load_bf16x8_bits(qs + off);
        const bf16x8 dv = load_bf16x8_bits(dctx + off);
#pragma unroll
        for (int r = 0; r < kDencRows; ++r) {
          const float a = sc[ll][wid * kDencRows + r][0];
          const float p = sc[ll][wid * kDencRows + r][1];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            acc[r][j] += a * (float)qv[j];
            acc[r][j] += p * (float)dv[j];
          }
        }
      }
    }
  }
  if (c0 < d) {
#pragma unroll
    for (int r = 0; r < kDencRows; ++r) {
      const int s = s_base + wid * kDencRows + r;
      if (s < s_len) store_denc(out + ((long)b * s_len + s) * d + c0, acc[r]);
    }
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// Host wrappers
//
// Every shape, dtype and resource condition a kernel relies on is checked
// here, before any allocation and before the launch, so a bad call raises
// and leaves its output buffers untouched.
// ---------------------------------------------------------------------------

namespace {

// Largest dynamic LDS request a launch on the current device accepts.
// Queried once per device: the wrappers run several times per decoder step.
size_t lds_limit_bytes() {
  constexpr int kMaxDevices = 64;
  static std::atomic<int> cached[kMaxDevices];  // zero-initialised
  int dev = 0;
  LV_CHECK_HIP(hipGetDevice(&dev));
  const bool cacheable = dev >= 0 && dev < kMaxDevices;
  int limit = cacheable ? cached[dev].load(std::memory_order_relaxed) : 0;
  if (limit == 0) {
    LV_CHECK_HIP(hipDeviceGetAttribute(
        &limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    if (cacheable) cached[dev].store(limit, std::memory_order_relaxed);
  }
  return (size_t)limit;
}

constexpr int64_t kAttendMaxD = 4 * WAVE_SIZE * 8;  // MAXDV register slices

size_t attend_fwd_lds(int64_t s, int64_t d) {
  return (size_t)d * 2 + (size_t)s * 4 + (size_t)4 * d * 4 + 16;
}

size_t attend_bwd_lds(int64_t s, int64_t d) {
  return (size_t)d * 4 + (size_t)s * 4 + (size_t)4 * d * 4 + 16;
}

// Checks shared by attend_fwd (q, enc, pad) and attend_bwd (q, enc).
void check_attend_q_enc(const torch::Tensor& q, const torch::Tensor& enc) {
  TORCH_CHECK(cuda_contig(q, torch::kBFloat16) && q.dim() == 2,
              "q must be CUDA contiguous bf16 [B,D]");
  TORCH_CHECK(cuda_contig(enc, torch::kBFloat16) && enc.dim() == 3,
              "enc must be CUDA contiguous bf16 [B,S,D]");
  const int64_t b = q.size(0), d = q.size(1);
  TORCH_CHECK(b >= 1 && enc.size(0) == b && enc.size(2) == d,
              "enc must be [B,S,D] for q [B,D]");
  TORCH_CHECK(enc.size(1) >= 1, "S >= 1");
  TORCH_CHECK(d >= 8 && d % 8 == 0, "D % 8 == 0");
  TORCH_CHECK(d <= kAttendMaxD, "D <= 2048");
}

}  // namespace

void smallm_gemm(torch::Tensor a, torch::Tensor wt,
                 c10::optional<torch::Tensor> pre, torch::Tensor out,
                 int64_t k, int64_t wt_col0, double alpha,
                 int64_t pre_mode) {
  // a may be a column slice of a wider matrix: unit column stride, rows
  // and base 16-byte aligned for the bf16x8 fragment loads.
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == torch::kBFloat16 &&
              a.dim() == 2 && (a.size(1) == 1 || a.stride(1) == 1) &&
              (a.size(0) == 1 || (a.stride(0) >= a.size(1) &&
                                  a.stride(0) % 8 == 0)) && aligned16(a),
              "a must be CUDA bf16 [M,K] with unit column stride and "
              "16-byte aligned rows");
  TORCH_CHECK(cuda_contig(wt, torch::kBFloat16) && wt.dim() == 2,
              "wt must be CUDA contiguous bf16 [>=N,ldw]");
  TORCH_CHECK(cuda_contig(out, torch::kBFloat16) && out.dim() == 2,
              "out must be CUDA contiguous bf16 [M,N]");
  TORCH_CHECK(out.size(0) == a.size(0), "out must have M rows");
  const int m = a.size(0);
  const int n = out.size(1);
  TORCH_CHECK(m >= 1 && n >= 1, "M, N >= 1");
  TORCH_CHECK(k >= 32 && k % 32 == 0, "K%32");
  TORCH_CHECK(k == a.size(1), "a must be [M,K] exactly");

  TORCH_CHECK(wt.size(0) >= n, "wt rows >= N");
  const long ldw = wt.size(1);
  TORCH_CHECK(wt_col0 >= 0 && wt_col0 + k <= ldw, "wt K slice OOB");
  // 16-byte bf16x8 loads of Wt rows.
  TORCH_CHECK(ldw % 8 == 0 && wt_col0 % 8 == 0,
              "ldw % 8 == 0 and wt_col0 % 8 == 0");
  TORCH_CHECK(pre_mode >= 0 && pre_mode <= 3, "pre_mode in 0..3");
  const unsigned short* prep = nullptr;
  if (pre_mode == 1 || pre_mode == 2) {
    TORCH_CHECK(pre.has_value() && cuda_contig(*pre, torch::kBFloat16),
                "pre must be CUDA contiguous bf16");
    if (pre_mode == 1) {
      TORCH_CHECK(pre->numel() == n, "mode 1: pre must have N elements");
    } else {
      TORCH_CHECK(pre->dim() == 2 && pre->size(0) == m && pre->size(1) == n,
                  "mode 2: pre must be [M,N]");
    }
    prep = (const unsigned short*)pre->data_ptr();
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(smallm_gemm_kernel,
                     dim3(cdiv(n, 16), cdiv(m, 128)), dim3(256), 0,
                     stream, u16(a), u16(wt) + wt_col0, prep, u16(out), m, n,
                     (int)k, m == 1 ? (long)k : (long)a.stride(0), ldw,
                     (float)alpha, (int)pre_mode);
  LV_CHECK_HIP(hipGetLastError());
}

std::vector<torch::Tensor> attend_fwd(torch::Tensor q, torch::Tensor enc,
                                      torch::Tensor pad, double scale) {
  check_attend_q_enc(q, enc);
  const int b = q.size(0), d = q.size(1);
  const int s = enc.size(1);
  TORCH_CHECK(cuda_rows(pad, torch::kFloat32, b, s),
              "pad must be CUDA contiguous fp32 [B,S]");
  const size_t shmem = attend_fwd_lds(s, d);
  TORCH_CHECK(shmem <= lds_limit_bytes(), "attend_fwd: S=", s, " D=", d,
              " needs ", shmem, " bytes of LDS, over the device limit");
  auto probs = torch::empty({b, s}, q.options().dtype(torch::kFloat32));
  auto ctx = torch::empty({b, d}, q.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(attend_fwd_kernel, dim3(b), dim3(256), shmem, stream,
                     u16(q), u16(enc), pad.data_ptr<float>(),
                     probs.data_ptr<float>(), u16(ctx), b, s, d, (float)scale);
  LV_CHECK_HIP(hipGetLastError());
  return {probs, ctx};
}

std::vector<torch::Tensor> attend_bwd(torch::Tensor dctx,
                                      torch::Tensor probs, torch::Tensor q,
                                      torch::Tensor enc, torch::Tensor denc,
                                      double scale) {
  check_attend_q_enc(q, enc);
  const int b = q.size(0), d = q.size(1);
  const int s = enc.size(1);
  // dctx may arrive in any float type; it is cast to bf16 below.
  TORCH_CHECK(dctx.is_cuda() && dctx.is_floating_point() &&
              dctx.dim() == 2 && dctx.size(0) == b && dctx.size(1) == d,
              "dctx must be a CUDA float tensor [B,D]");
  TORCH_CHECK(cuda_rows(probs, torch::kFloat32, b, s),
              "probs must be CUDA contiguous fp32 [B,S]");
  TORCH_CHECK(cuda_contig(denc, torch::kFloat32) && denc.dim() == 3 &&
              denc.size(0) == b && denc.size(1) == s && denc.size(2) == d,
              "denc must be CUDA contiguous fp32 [B,S,D]");
  const size_t shmem = attend_bwd_lds(s, d);
  TORCH_CHECK(shmem <= lds_limit_bytes(), "attend_bwd: S=", s, " D=", d,
              " needs ", shmem, " bytes of LDS, over the device limit");
  auto dctx_c = dctx.to(torch::kBFloat16).contiguous();
  auto dq = torch::empty({b, d}, q.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(attend_bwd_kernel, dim3(b), dim3(256), shmem, stream,
                     u16(dctx_c), probs.data_ptr<float>(), u16(q), u16(enc),
                     u16(dq), denc.data_ptr<float>(), b, s, d, (float)scale);
  LV_CHECK_HIP(hipGetLastError());
  return {dq};
}

// Dynamic-LDS limit the attend_* launches are held to on the current
// device, and the bytes a call with these S, D asks for.
int64_t attend_lds_limit() { return (int64_t)lds_limit_bytes(); }

int64_t attend_lds_bytes(int64_t s, int64_t d, bool bwd) {
  return (int64_t)(bwd ? attend_bwd_lds(s, d) : attend_fwd_lds(s, d));
}

// ---------------------------------------------------------------------------
// Deferred-dEnc route
// ---------------------------------------------------------------------------

namespace {

// variant: 0 auto, 1..4 = (rows per wave iteration, waves) of
// (4,4) (8,4) (4,8) (8,8). 8 rows of more than two 512-column slices do
// not fit the register file, so those variants stop at D = 1024. Returns
// false for a variant that does not exist at this D.
bool step_variant(int64_t variant, int64_t d, int* u, int* nw) {
  if (variant == 0) variant = d <= 2 * WAVE_SIZE * 8 ? 3 : 1;
  if (variant < 1 || variant > 4) return false;
  *u = (variant == 2 || variant == 4) ? 8 : 4;
  *nw = variant >= 3 ? 8 : 4;
  return *u == 4 || d <= 2 * WAVE_SIZE * 8;
}

size_t attend_step_fwd_lds(int64_t s, int64_t d, int nw) {
  return (size_t)s * 4 + (size_t)nw * d * 4 + (size_t)nw * 4;
}

size_t attend_step_bwd_lds(int64_t s, int64_t d, int nw) {
  (void)s;
  return (size_t)d * 4 + (size_t)nw * d * 4 + (size_t)nw * 4;
}

#define LV_STEP_CASE(NDV, U, NW, KERNEL, ...)                               \
  if (ndv == NDV && u == U && nw == NW) {                                   \
    hipLaunchKernelGGL((KERNEL<NDV, U, NW>), dim3(b), dim3(NW * WAVE_SIZE), \
                       shmem, stream, __VA_ARGS__);                         \
  } else

#define LV_STEP_NDV(NDV, KERNEL, ...)         \
  LV_STEP_CASE(NDV, 4, 4, KERNEL, __VA_ARGS__) \
  LV_STEP_CASE(NDV, 8, 4, KERNEL, __VA_ARGS__) \
  LV_STEP_CASE(NDV, 4, 8, KERNEL, __VA_ARGS__) \
  LV_STEP_CASE(NDV, 8, 8, KERNEL, __VA_ARGS__)

#define LV_STEP_DISPATCH(KERNEL, ...)                          \
  LV_STEP_NDV(1, KERNEL, __VA_ARGS__)                          \
  LV_STEP_NDV(2, KERNEL, __VA_ARGS__)                          \
  LV_STEP_CASE(3, 4, 4, KERNEL, __VA_ARGS__)                   \
  LV_STEP_CASE(3, 4, 8, KERNEL, __VA_ARGS__)                   \
  LV_STEP_CASE(4, 4, 4, KERNEL, __VA_ARGS__)                   \
  LV_STEP_CASE(4, 4, 8, KERNEL, __VA_ARGS__) {                 \
    TORCH_CHECK(false, "no kernel for ndv=", ndv, " u=", u, " nw=", nw); \
  }

}  // namespace

void attend_step_fwd(torch::Tensor q, torch::Tensor enc, torch::Tensor pad,
                     double scale, torch::Tensor probs, torch::Tensor ctx,
                     torch::Tensor ctx32, int64_t variant) {
  check_attend_q_enc(q, enc);
  const int b = q.size(0), d = q.size(1);
  const int s = enc.size(1);
  TORCH_CHECK(cuda_rows(pad, torch::kFloat32, b, s),
              "pad must be CUDA contiguous fp32 [B,S]");
  TORCH_CHECK(cuda_rows(probs, torch::kFloat32, b, s),
              "probs must be CUDA contiguous fp32 [B,S]");
  TORCH_CHECK(cuda_rows(ctx, torch::kBFloat16, b, d),
              "ctx must be CUDA contiguous bf16 [B,D]");
  TORCH_CHECK(cuda_rows(ctx32, torch::kFloat32, b, d),
              "ctx32 must be CUDA contiguous fp32 [B,D]");
  int u = 0, nw = 0;
  TORCH_CHECK(step_variant(variant, d, &u, &nw),
              "variant in 0..4, and 2 or 4 only for D <= 1024");
  const size_t shmem = attend_step_fwd_lds(s, d, nw);
  TORCH_CHECK(shmem <= lds_limit_bytes(), "attend_step_fwd: S=", s, " D=", d,
              " needs ", shmem, " bytes of LDS, over the device limit");
  const int ndv = cdiv(d, WAVE_SIZE * 8);
  auto stream = at::cuda::getCurrentCUDAStream();
  LV_STEP_DISPATCH(attend_step_fwd_kernel, u16(q), u16(enc),
                   pad.data_ptr<float>(), probs.data_ptr<float>(), u16(ctx),
                   ctx32.data_ptr<float>(), s, d, (float)scale)
  LV_CHECK_HIP(hipGetLastError());
}

void attend_step_bwd(torch::Tensor dctx_a, c10::optional<torch::Tensor> dctx_b,
                     torch::Tensor probs, torch::Tensor ctx32,
                     torch::Tensor enc, double scale, torch::Tensor dctx_out,
                     torch::Tensor dl, torch::Tensor dq, int64_t variant) {
  check_attend_q_enc(dctx_a, enc);
  const int b = dctx_a.size(0), d = dctx_a.size(1);
  const int s = enc.size(1);
  const unsigned short* bp = nullptr;
  long ldb = 0;
  if (dctx_b.has_value()) {
    ldb = check_strided_rows(*dctx_b, b, d, "dctx_b");
    bp = (const unsigned short*)dctx_b->data_ptr();
  }
  TORCH_CHECK(cuda_rows(probs, torch::kFloat32, b, s),
              "probs must be CUDA contiguous fp32 [B,S]");
  TORCH_CHECK(cuda_rows(ctx32, torch::kFloat32, b, d),
              "ctx32 must be CUDA contiguous fp32 [B,D]");
  TORCH_CHECK(cuda_rows(dctx_out, torch::kBFloat16, b, d),
              "dctx_out must be CUDA contiguous bf16 [B,D]");
  TORCH_CHECK(cuda_rows(dl, torch::kFloat32, b, s),
              "dl must be CUDA contiguous fp32 [B,S]");
  TORCH_CHECK(cuda_rows(dq, torch::kBFloat16, b, d),
              "dq must be CUDA contiguous bf16 [B,D]");
  int u = 0, nw = 0;
  TORCH_CHECK(step_variant(variant, d, &u, &nw),
              "variant in 0..4, and 2 or 4 only for D <= 1024");
  const size_t shmem = attend_step_bwd_lds(s, d, nw);
  TORCH_CHECK(shmem <= lds_limit_bytes(), "attend_step_bwd: S=", s, " D=", d,
              " needs ", shmem, " bytes of LDS, over the device limit");
  const int ndv = cdiv(d, WAVE_SIZE * 8);
  auto stream = at::cuda::getCurrentCUDAStream();
  LV_STEP_DISPATCH(attend_step_bwd_kernel, u16(dctx_a), bp, ldb,
                   probs.data_ptr<float>(), ctx32.data_ptr<float>(), u16(enc),
                   u16(dctx_out), dl.data_ptr<float>(), u16(dq), s, d,
                   (float)scale)
  LV_CHECK_HIP(hipGetLastError());
}

void attend_denc(torch::Tensor dl, torch::Tensor probs, torch::Tensor qs,
                 torch::Tensor dctx, torch::Tensor out) {
  TORCH_CHECK(cuda_contig(dl, torch::kFloat32) && dl.dim() == 3,
              "dl must be CUDA contiguous fp32 [L,B,S]");
  const int64_t l = dl.size(0), b = dl.size(1), s = dl.size(2);
  TORCH_CHECK(l >= 1 && b >= 1 && s >= 1, "L, B, S >= 1");
  TORCH_CHECK(cuda_contig(probs, torch::kFloat32) &&
              probs.sizes() == dl.sizes(),
              "probs must be CUDA contiguous fp32 [L,B,S]");
  TORCH_CHECK(cuda_contig(qs, torch::kBFloat16) && qs.dim() == 3 &&
              qs.size(0) == l && qs.size(1) == b,
              "qs must be CUDA contiguous bf16 [L,B,D]");
  const int64_t d = qs.size(2);
  TORCH_CHECK(d >= 8 && d % 8 == 0, "D % 8 == 0");
  TORCH_CHECK(d <= kAttendMaxD, "D <= 2048");
  TORCH_CHECK(cuda_contig(dctx, torch::kBFloat16) &&
              dctx.sizes() == qs.sizes(),
              "dctx must be CUDA contiguous bf16 [L,B,D]");
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 3 &&
              out.size(0) == b && out.size(1) == s && out.size(2) == d &&
              (out.scalar_type() == torch::kFloat32 ||
               out.scalar_type() == torch::kBFloat16),
              "out must be CUDA contiguous fp32 or bf16 [B,S,D]");
  TORCH_CHECK(l <= INT_MAX && b <= INT_MAX && s <= INT_MAX, "sizes fit int");
  const int64_t s_tiles = (s + kDencTile - 1) / kDencTile;
  TORCH_CHECK(b * s_tiles <= INT_MAX, "B * ceil(S/32) fits the grid");
  const dim3 grid((unsigned)(b * s_tiles), cdiv(d, WAVE_SIZE * 8));
  auto stream = at::cuda::getCurrentCUDAStream();
  if (out.scalar_type() == torch::kFloat32) {
    hipLaunchKernelGGL(attend_denc_kernel<float>, grid, dim3(256), 0, stream,
                       dl.data_ptr<float>(), probs.data_ptr<float>(), u16(qs),
                       u16(dctx), out.data_ptr<float>(), (int)l, (int)b,
                       (int)s, (int)d, (int)s_tiles);
  } else {
    hipLaunchKernelGGL(attend_denc_kernel<unsigned short>, grid, dim3(256), 0,
                       stream, dl.data_ptr<float>(), probs.data_ptr<float>(),
                       u16(qs), u16(dctx), u16(out), (int)l, (int)b, (int)s,
                       (int)d, (int)s_tiles);
  }
  LV_CHECK_HIP(hipGetLastError());
}

// Dynamic LDS bytes attend_step_fwd / attend_step_bwd ask for at (S, D)
// with this variant, and the rows of s one attend_denc workgroup owns.
int64_t attend_step_lds_bytes(int64_t s, int64_t d, bool bwd,
                              int64_t variant) {
  int u = 0, nw = 0;
  TORCH_CHECK(step_variant(variant, d, &u, &nw),
              "variant in 0..4, and 2 or 4 only for D <= 1024");
  return (int64_t)(bwd ? attend_step_bwd_lds(s, d, nw)
                       : attend_step_fwd_lds(s, d, nw));
}

int64_t attend_denc_row_tile() { return kDencTile; }
