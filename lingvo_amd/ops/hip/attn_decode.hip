// Cached (KV-cache) attention for gfx950: the attention block of
// MultiHeadedAttention.ExtendStep / StreamStep (layers/attention.py) as one
// kernel plus, when the key range is split, one combine kernel. Forward
// only.
//
//   q        [B, C, N, H] bf16 (row stride sq, may be a view of the packed
//            QKV projection)
//   k/v cache [B, Smax, NKV, H] bf16, rows < q_start + C already written
//   out      [B, C, N, H] bf16
//
// Query row i sits at position p = q_start + i. Key j is visible iff
//   j <= p  AND  (win_l < 0 OR j >= p - win_l);
// logit = scale * q.k + bias[n, clamp(p - j, -clip, clip) + clip].
//
// attn_decode_kernel, grid (split x row tile, kv head, batch), 4 waves. A
// workgroup owns the M = C * (N / NKV) query rows that share its KV head
// (M <= 8; for larger M one tile of 8 of them) and one contiguous span of
// key positions. Single-query attention is a memory-bound read of K and V
// (guide Appendix B "Attention decode", §5 "GEMV / M <= 16"): K/V rows go
// from global memory straight into registers in 16-byte loads, H/8 lanes
// per key row, 64/(H/8) keys per wave load, AD_U K and AD_U V loads in
// flight per lane (4, or 2 for the 8-row tile so that it stays at two waves
// per SIMD); the dot products run on the VALU against q held in registers
// (pre-multiplied by scale * log2 e). Every lane group keeps a running
// (max, sum, o[8 of H]) per row in fp32 and rescales once per AD_U keys.
// A workgroup holds R <= 8 rows; M <= 8 (every C = 1 decode step with
// group <= 8) reads the span exactly once, larger M (streaming chunks, whose
// window is short) puts its 8-row tiles side by side in grid.x, so the span
// is read once from HBM and again out of L2 by the other tiles. At the end
// lane groups merge by butterfly shuffles, waves through LDS, both in a
// fixed order. With one split the result is normalised and stored as bf16; with
// more, the (o[H], max, sum) partial goes to an fp32 workspace
// [B, NKV, splits, M, H + 2] and attn_decode_combine merges the splits in
// split order. No atomics, no inter-workgroup waits.
//
// Masked keys never reach the arithmetic: the key index of a load is clamped
// into the span's visible range (so it is always a valid, visible-to-some-row
// cache row < Smax), K and V of a lane whose own key is outside that range
// are replaced by zeros with a select, and the per-row visibility selects
// the logit (-1e30) and the probability (0). A span without a visible key
// yields the empty partial (max -1e30, sum 0, o 0), which the merges absorb
// without NaN because -1e30 is finite.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include "common.h"

namespace {

constexpr int AD_NW = 4;
constexpr int AD_BLOCK = AD_NW * WAVE_SIZE;
constexpr int AD_MAX_ROWS = 64;
// Host split policy: aim at AD_TARGET_WGS workgroups (two per CU fit by
// registers), never below AD_MIN_SPAN keys per split.
constexpr int AD_TARGET_WGS = 512;
constexpr int AD_MIN_SPAN = 256;
constexpr int AD_MAX_SPLITS = 64;
constexpr float AD_NEG = -1e30f;
constexpr float AD_LOG2E = 1.4426950408889634f;

__device__ __forceinline__ void ad_unpack(const ushortx8& u, float* f) {
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = bf16_bits_to_float(u[e]);
}

// (m, l, o) += (m2, l2, o2) for online-softmax partials in the log2 domain.
template <int NE>
__device__ __forceinline__ void ad_merge(float& m, float& l, float* o,
                                         float m2, float l2,
                                         const float* o2) {
  const float mx = fmaxf(m, m2);
  const float a = exp2f(m - mx), a2 = exp2f(m2 - mx);
  l = l * a + l2 * a2;
#pragma unroll
  for (int e = 0; e < NE; ++e) o[e] = o[e] * a + o2[e] * a2;
  m = mx;
}

template <int H, int R, int AD_U>
__global__ __launch_bounds__(AD_BLOCK) void attn_decode_kernel(
    const unsigned short* __restrict__ q,
    const unsigned short* __restrict__ kc,
    const unsigned short* __restrict__ vc, const int* __restrict__ q_start_t,
    int q_start_i, const void* __restrict__ bias, int bias_f32,
    unsigned short* __restrict__ out, float* __restrict__ ws, int C, int N,
    int NKV, int Smax, int win_l, int clip, float scale_log2, int part_lo,
    int span, int splits, long sq, long sk, long sv) {
  constexpr int LPK = H / 8;           // lanes per key row
  constexpr int KPW = WAVE_SIZE / LPK; // key rows per wave load
  constexpr int KPI = KPW * AD_NW;     // key rows per workgroup load
  __shared__ float red[AD_NW][R][H + 2];

  const int kvh = blockIdx.y, b = blockIdx.z;
  const int group = N / NKV, M = C * group;
  const int ntiles = (M + R - 1) / R;
  const int split = blockIdx.x / ntiles;
  const int r0 = (blockIdx.x % ntiles) * R;  // this workgroup's row tile
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int w = threadIdx.x / WAVE_SIZE;
  const int g = lane / LPK, sub = lane % LPK;

  int qs = q_start_t != nullptr ? q_start_t[b] : q_start_i;
  qs = min(max(qs, 0), Smax - C);  // no key index >= Smax is ever formed
  const long k0l = (long)part_lo + (long)split * span;
  const int k0 = (int)(k0l < (long)Smax ? k0l : (long)Smax);
  const int k1 = (int)(k0l + span < (long)Smax ? k0l + span : (long)Smax);
  const int nbias = 2 * clip + 1;

  {
    // Keys some row of this tile can see, cut to the span (inclusive).
    const int i_lo = r0 / group;
    const int i_hi = min(r0 + R - 1, M - 1) / group;
    const int vis_lo = win_l >= 0 ? max(qs + i_lo - win_l, 0) : 0;
    const int j_lo = max(k0, vis_lo);
    const int j_hi = min(k1 - 1, qs + i_hi);

    float qf[R][8];
    int pos[R], head[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int rr = min(r0 + r, M - 1);
      const int i = rr / group;
      head[r] = kvh * group + rr % group;
      pos[r] = qs + i;
      const ushortx8 qu = *reinterpret_cast<const ushortx8*>(
          q + ((long)b * C + i) * sq + (long)head[r] * H + sub * 8);
      ad_unpack(qu, qf[r]);
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[r][e] *= scale_log2;
    }

    float m[R], l[R], o[R][8];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      m[r] = AD_NEG;
      l[r] = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[r][e] = 0.f;
    }

    for (int jb = j_lo; jb <= j_hi; jb += KPI * AD_U) {
      ushortx8 ku[AD_U], vu[AD_U];
      int jj[AD_U];
      bool ok[AD_U];
#pragma unroll
      for (int u = 0; u < AD_U; ++u) {
        jj[u] = jb + u * KPI + w * KPW + g;
        ok[u] = jj[u] <= j_hi;
        const int jc = min(jj[u], j_hi);  // j_lo <= jc <= j_hi < Smax
        const long row = (long)b * Smax + jc;
        ku[u] = *reinterpret_cast<const ushortx8*>(
            kc + row * sk + (long)kvh * H + sub * 8);
        vu[u] = *reinterpret_cast<const ushortx8*>(
            vc + row * sv + (long)kvh * H + sub * 8);
      }
      const ushortx8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int u = 0; u < AD_U; ++u) {
        ku[u] = ok[u] ? ku[u] : zero;
        vu[u] = ok[u] ? vu[u] : zero;
      }

      // Logits of all rows (log2 domain), reduced over the key row's lanes.
      float s[R][AD_U];
#pragma unroll
      for (int u = 0; u < AD_U; ++u) {
        float kf[8];
        ad_unpack(ku[u], kf);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          float d = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) d = fmaf(qf[r][e], kf[e], d);
          s[r][u] = d;
        }
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int u = 0; u < AD_U; ++u) {
          float d = s[r][u];
#pragma unroll
          for (int off = 1; off < LPK; off <<= 1)
            d += __shfl_xor(d, off, WAVE_SIZE);
          s[r][u] = d;
        }
      }

      // Online softmax: s becomes the probability against the new max.
#pragma unroll
      for (int r = 0; r < R; ++r) {
        bool vis[AD_U];
        float mx = m[r];
#pragma unroll
        for (int u = 0; u < AD_U; ++u) {
          const int dist = pos[r] - jj[u];
          vis[u] = ok[u] && dist >= 0 && (win_l < 0 || dist <= win_l);
          float x = s[r][u];
          if (bias != nullptr) {
            const long bi = (long)head[r] * nbias +
                            (min(max(dist, -clip), clip) + clip);
            const float bv =
                bias_f32 ? reinterpret_cast<const float*>(bias)[bi]
                         : bf16_bits_to_float(
                               reinterpret_cast<const unsigned short*>(
                                   bias)[bi]);
            x = fmaf(bv, AD_LOG2E, x);
          }
          x = vis[u] ? x : AD_NEG;
          s[r][u] = x;
          mx = fmaxf(mx, x);
        }
        const float a = exp2f(m[r] - mx);
        float ps = 0.f;
#pragma unroll
        for (int u = 0; u < AD_U; ++u) {
          const float p = vis[u] ? exp2f(s[r][u] - mx) : 0.f;
          s[r][u] = p;
          ps += p;
        }
        m[r] = mx;
        l[r] = l[r] * a + ps;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[r][e] *= a;
      }

#pragma unroll
      for (int u = 0; u < AD_U; ++u) {
        float vf[8];
        ad_unpack(vu[u], vf);
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            o[r][e] = fmaf(s[r][u], vf[e], o[r][e]);
        }
      }
    }

    // Merge the wave's key-row groups (butterfly, fixed order) ...
#pragma unroll
    for (int off = LPK; off < WAVE_SIZE; off <<= 1) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float m2 = __shfl_xor(m[r], off, WAVE_SIZE);
        const float l2 = __shfl_xor(l[r], off, WAVE_SIZE);
        float o2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          o2[e] = __shfl_xor(o[r][e], off, WAVE_SIZE);
        ad_merge<8>(m[r], l[r], o[r], m2, l2, o2);
      }
    }
    // ... then the waves through LDS.
    if (g == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int e = 0; e < 8; ++e) red[w][r][sub * 8 + e] = o[r][e];
        if (sub == 0) {
          red[w][r][H] = m[r];
          red[w][r][H + 1] = l[r];
        }
      }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < R * H; idx += AD_BLOCK) {
      const int r = idx / H, h = idx % H;
      const int rr = r0 + r;
      if (rr >= M) continue;
      float mm = red[0][r][H], ll = red[0][r][H + 1], oo = red[0][r][h];
#pragma unroll
      for (int ww = 1; ww < AD_NW; ++ww)
        ad_merge<1>(mm, ll, &oo, red[ww][r][H], red[ww][r][H + 1],
                    &red[ww][r][h]);
      if (splits == 1) {
        const int i = rr / group, n = kvh * group + rr % group;
        const float inv = ll > 0.f ? 1.f / ll : 0.f;
        out[(((long)b * C + i) * N + n) * H + h] =
            float_to_bf16_bits(oo * inv);
      } else {
        float* wrow =
            ws + ((((long)b * NKV + kvh) * splits + split) * M + rr) * (H + 2);
        wrow[h] = oo;
        if (h == 0) {
          wrow[H] = mm;
          wrow[H + 1] = ll;
        }
      }
    }
  }
}

// One block per (b, kv head, row), one thread per h: merges the row's
// partials in split order, normalises and stores bf16.
template <int H>
__global__ __launch_bounds__(H) void attn_decode_combine(
    const float* __restrict__ ws, unsigned short* __restrict__ out,
    int splits, int C, int N, int NKV) {
  const int group = N / NKV, M = C * group;
  const long blk = blockIdx.x;
  const int rr = (int)(blk % M);
  const long bk = blk / M;  // b * NKV + kvh
  const int kvh = (int)(bk % NKV);
  const long b = bk / NKV;
  const int h = threadIdx.x;
  const float* base = ws + (bk * splits * M + rr) * (H + 2);
  const long sstride = (long)M * (H + 2);
  float mm = AD_NEG;
  for (int s = 0; s < splits; ++s) mm = fmaxf(mm, base[s * sstride + H]);
  float ll = 0.f, oo = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float* p = base + s * sstride;
    const float a = exp2f(p[H] - mm);
    ll = fmaf(p[H + 1], a, ll);
    oo = fmaf(p[h], a, oo);
  }
  const int i = rr / group, n = kvh * group + rr % group;
  const float inv = ll > 0.f ? 1.f / ll : 0.f;
  out[((b * C + i) * N + n) * H + h] = float_to_bf16_bits(oo * inv);
}

// Same contract as flash_attn.hip check_strided_btnh: dense [N][H], one
// uniform token-row stride that is a multiple of 8 elements, 16-byte base.
long ad_check_strided(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 4 &&
                  t.scalar_type() == torch::kBFloat16,
              name, " must be a CUDA bf16 [B,T,N,H] tensor");
  const long N = t.size(2), H = t.size(3);
  TORCH_CHECK(t.stride(3) == 1 && (N == 1 || t.stride(2) == H), name,
              ": the [N][H] dims must be dense");
  const long row = t.size(1) == 1 && t.size(0) == 1
                       ? N * H
                       : (t.size(1) == 1 ? t.stride(0) : t.stride(1));
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

}  // namespace

// Split count for `keys` key positions shared by B * NKV * (8-row tiles of
// `rows`) workgroup columns; from shapes only.
int64_t attn_decode_num_splits(int64_t B, int64_t NKV, int64_t keys,
                               int64_t rows) {
  const int64_t tiles = rows > 8 ? (rows + 7) / 8 : 1;
  const int64_t cols = B * NKV > 0 ? B * NKV * tiles : 1;
  int64_t want = (AD_TARGET_WGS + cols - 1) / cols;
  const int64_t most = keys / AD_MIN_SPAN;
  if (want > most) want = most;
  if (want > AD_MAX_SPLITS) want = AD_MAX_SPLITS;
  return want < 1 ? 1 : want;
}

torch::Tensor attn_decode(torch::Tensor q, torch::Tensor key_cache,
                          torch::Tensor value_cache,
                          c10::optional<torch::Tensor> q_start_t,
                          int64_t q_start,
                          c10::optional<torch::Tensor> bias, int64_t win_l,
                          int64_t bias_clip, double scale,
                          int64_t num_splits) {
  // The whole contract is checked before anything is allocated or launched.
  const long sq = ad_check_strided(q, "q");
  const long sk = ad_check_strided(key_cache, "key_cache");
  const long sv = ad_check_strided(value_cache, "value_cache");
  const int64_t B = q.size(0), C = q.size(1), N = q.size(2), H = q.size(3);
  const int64_t Smax = key_cache.size(1), NKV = key_cache.size(2);
  TORCH_CHECK(H == 64 || H == 128, "H must be 64 or 128, got ", H);
  TORCH_CHECK(key_cache.size(0) == B && key_cache.size(3) == H &&
                  value_cache.sizes() == key_cache.sizes(),
              "caches must be [B,Smax,NKV,H]");
  TORCH_CHECK(B >= 1 && NKV >= 1 && N % NKV == 0,
              "GQA requires N % NKV == 0");
  const int64_t M = C * (N / NKV);
  TORCH_CHECK(C >= 1 && M <= AD_MAX_ROWS, "need 1 <= C and C * group <= ",
              AD_MAX_ROWS, ", got C=", C, " group=", N / NKV);
  TORCH_CHECK(C <= Smax, "C must be <= Smax");
  TORCH_CHECK(B <= 65535 && NKV <= 65535, "B and NKV must be <= 65535");
  TORCH_CHECK(Smax < (1LL << 30), "Smax must be < 2^30");
  TORCH_CHECK(num_splits >= 0, "num_splits must be >= 0");
  const int* qsp = nullptr;
  if (q_start_t.has_value()) {
    TORCH_CHECK(q_start_t->is_cuda() && q_start_t->dim() == 1 &&
                    q_start_t->size(0) == B &&
                    q_start_t->scalar_type() == torch::kInt32 &&
                    q_start_t->is_contiguous(),
                "q_start tensor must be contiguous int32 [B] on the GPU");
    qsp = q_start_t->data_ptr<int>();
  } else {
    TORCH_CHECK(q_start >= 0 && q_start + C <= Smax,
                "need 0 <= q_start and q_start + C <= Smax, got q_start=",
                q_start, " C=", C, " Smax=", Smax);
  }
  const void* bp = nullptr;
  int bias_f32 = 0;
  if (bias.has_value()) {
    TORCH_CHECK(bias_clip >= 0 && bias->is_cuda() && bias->dim() == 2 &&
                    bias->size(0) == N &&
                    bias->size(1) == 2 * bias_clip + 1 &&
                    bias->is_contiguous() &&
                    (bias->scalar_type() == torch::kBFloat16 ||
                     bias->scalar_type() == torch::kFloat32),
                "bias must be contiguous bf16/fp32 [N, 2*bias_clip+1]");
    bp = bias->data_ptr();
    bias_f32 = bias->scalar_type() == torch::kFloat32;
  }

  // Key range that is split: the visible range when the host knows it, the
  // whole cache when the lengths live on the device.
  int64_t part_lo = 0, part_hi = Smax;
  if (qsp == nullptr) {
    part_hi = q_start + C;
    if (win_l >= 0 && q_start - win_l > 0) part_lo = q_start - win_l;
  }
  const int64_t keys = part_hi - part_lo;
  const int64_t splits =
      num_splits > 0 ? num_splits : attn_decode_num_splits(B, NKV, keys, M);
  TORCH_CHECK(splits <= 65535, "num_splits must be <= 65535");
  const int64_t span = (keys + splits - 1) / splits;

  auto out = torch::empty({B, C, N, H}, q.options());
  torch::Tensor ws;
  if (splits > 1)
    ws = torch::empty({B, NKV, splits, M, H + 2},
                      q.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
  const int64_t tiles = M > 8 ? (M + 7) / 8 : 1;
  dim3 grid((unsigned)(splits * tiles), (unsigned)NKV, (unsigned)B);
  const float scale_log2 = (float)scale * AD_LOG2E;
  const int wl = (int)(win_l < 0 ? -1 : (win_l > Smax ? Smax : win_l));
#define AD_LAUNCH(HH, RR, UU)                                                   \
  hipLaunchKernelGGL((attn_decode_kernel<HH, RR, UU>), grid, dim3(AD_BLOCK), 0,  \
                     stream, (const unsigned short*)q.data_ptr(),            \
                     (const unsigned short*)key_cache.data_ptr(),            \
                     (const unsigned short*)value_cache.data_ptr(), qsp,     \
                     (int)q_start, bp, bias_f32,                             \
                     (unsigned short*)out.data_ptr(),                        \
                     splits > 1 ? ws.data_ptr<float>() : nullptr, (int)C,    \
                     (int)N, (int)NKV, (int)Smax, wl, (int)bias_clip,        \
                     scale_log2, (int)part_lo, (int)span, (int)splits, sq,   \
                     sk, sv)
#define AD_ROWS(HH)                                                          \
  if (M <= 1) {                                                              \
    AD_LAUNCH(HH, 1, 4);                                                        \
  } else if (M <= 2) {                                                       \
    AD_LAUNCH(HH, 2, 4);                                                        \
  } else if (M <= 4) {                                                       \
    AD_LAUNCH(HH, 4, 4);                                                        \
  } else {                                                                   \
    AD_LAUNCH(HH, 8, 2);                                                        \
  }
  if (H == 64) {
    AD_ROWS(64)
  } else {
    AD_ROWS(128)
  }
#undef AD_ROWS
#undef AD_LAUNCH
  if (splits > 1) {
    const unsigned nblk = (unsigned)(B * NKV * M);
    if (H == 64) {
      hipLaunchKernelGGL((attn_decode_combine<64>), dim3(nblk), dim3(64), 0,
                         stream, ws.data_ptr<float>(),
                         (unsigned short*)out.data_ptr(), (int)splits, (int)C,
                         (int)N, (int)NKV);
    } else {
      hipLaunchKernelGGL((attn_decode_combine<128>), dim3(nblk), dim3(128), 0,
                         stream, ws.data_ptr<float>(),
                         (unsigned short*)out.data_ptr(), (int)splits, (int)C,
                         (int)N, (int)NKV);
    }
  }
  LV_CHECK_HIP(hipGetLastError());
  return out;
}
