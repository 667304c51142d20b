// Fused LSTM scan step kernels for gfx950 (ROADMAP item 11; reference
// lingvo/core/lstm_frnn_layer.py LSTMFRNN, cell math rnn_cell.py:213).
//
// The biLSTM encoder scan is launch-bound: per step and direction the
// layer path issues a library GEMM at M=B, a bias add, the K11 gate
// kernel and ~6 elementwise kernels for the padded carry. Here ONE launch
// handles one scan step for ALL directions: the recurrent small-M GEMM
// ("smallm_gemm", las_decoder.hip) with the whole LSTM cell as epilogue.
// The only ordering between steps is the kernel boundary on one stream;
// nothing inside a kernel waits on another workgroup.
//
// Buffers (natural time order, D directions):
//   gates [D,T,B,4H] bf16  in: x@W_x(+b); out: full pre-activations
//   c, m  [D,T,B,H]  bf16
//   pad   [T,B]      fp32
//   WmT   [D,4H,H]   bf16  recurrent rows of wm transposed (fwd B operand)
//   Wm    [D,H,4H]   bf16  recurrent rows as stored (bwd B operand)
// Direction d runs reversed in time when bit d of rev_mask is set: scan
// step s works on t = rev ? T-1-s : s and its previous state lives at
// t -/+ 1 (zeros at s == 0).
//
// Grid (H/16, ceil(B / (16*MT)), D), block 256 = 4 waves. A workgroup
// owns hidden columns j0..j0+15 of one direction for 16*MT batch rows and
// is the only reader/writer of those (b, j) state elements, so in-place
// updates are safe. Each thread owns MT elements of that 16*MT x 16 tile
// in the pointwise part and issues their loads BEFORE the GEMM, so the
// step pays one round of load latency, not two.
//
// A step is latency-bound (the next launch depends on it), so the K loop
// (tile_gemm.h) is written for loads in flight, not for occupancy: no
// per-row branches (rows beyond B re-read row B-1: output row r of an MFMA
// depends on A row r alone, and the pointwise part never stores those
// rows) and KU k-steps of fragments loaded ahead of their MFMAs.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include "common.h"
#include "mfma.h"
#include "tile_gemm.h"

namespace {

__device__ __forceinline__ float sigf(float x) {
  return 1.f / (1.f + __expf(-x));
}

// ---------------------------------------------------------------------------
// Forward step. Wave w computes gate w's 16 columns for all MT m-tiles
// over the full K=H (no K remainder to split), parks its tile in LDS, and
// then all 256 threads run the cell math on the 16*MT x 16 state tile.
// ---------------------------------------------------------------------------
template <int MT>
__global__ __launch_bounds__(256) void lstm_scan_step_fwd(
    unsigned short* __restrict__ gates, unsigned short* __restrict__ c,
    unsigned short* __restrict__ m, const float* __restrict__ pad,
    const unsigned short* __restrict__ wmt, int t_len, int b, int h, int s,
    int rev_mask, float fgb, float cap) {
  const int j0 = blockIdx.x * 16;
  const int m0 = blockIdx.y * (16 * MT);
  const int d = blockIdx.z;
  const bool rev = (rev_mask >> d) & 1;
  const int t = rev ? t_len - 1 - s : s;
  const int t_prev = rev ? t + 1 : t - 1;
  const bool has_prev = s > 0;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int cl = lane & 15;

  __shared__ float rec[4][16 * MT][16];  // recurrent term per gate

  const long st = ((long)d * t_len + t) * b;         // row base at t
  const long sp = ((long)d * t_len + t_prev) * b;    // row base at t_prev

  // Pointwise operands of this thread's MT elements (element e is tile
  // row e*16 + tid/16, column tid%16), loaded ahead of the GEMM.
  const int lc = threadIdx.x & 15;
  const int j = j0 + lc;
  // Every load is unconditional and kept as raw bits: a branch or a
  // conversion here would wait for these loads before the GEMM has issued
  // its own. Without a previous step the state loads read (and discard)
  // this step's not yet written slots.
  const long sq = has_prev ? sp : st;
  unsigned short gin[MT][4], c_prev_u[MT], m_prev_u[MT];
  float pv[MT];
#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const int rowc = min(m0 + e * 16 + (threadIdx.x >> 4), b - 1);
    const unsigned short* gr = gates + (st + rowc) * 4 * h + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) gin[e][q] = gr[q * h];
    pv[e] = pad[(long)t * b + rowc];
    c_prev_u[e] = c[(sq + rowc) * h + j];
    m_prev_u[e] = m[(sq + rowc) * h + j];
  }

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
  if (has_prev) {
    const unsigned short* brow =
        wmt + ((long)d * 4 * h + (long)wid * h + j0 + cl) * h + g * 8;
    const unsigned short* arow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      arow[mt] = m + (sp + min(m0 + mt * 16 + cl, b - 1)) * h + g * 8;
    }
    tile_gemm<MT>(arow, brow, h, acc);
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      rec[wid][mt * 16 + g * 4 + r][cl] = acc[mt][r];
    }
  }
  __syncthreads();

#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const int lrow = e * 16 + (threadIdx.x >> 4);
    const int row = m0 + lrow;
    if (row >= b) continue;
    unsigned short* gr = gates + (st + row) * 4 * h + j;
    float pre[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // Round to bf16 first: backward recomputes from the stored value.
      const unsigned short u =
          float_to_bf16_bits(bf16_bits_to_float(gin[e][q]) +
                             rec[q][lrow][lc]);
      gr[q * h] = u;
      pre[q] = bf16_bits_to_float(u);
    }
    const float cand = tanhf(pre[0]);
    const float ig = sigf(pre[1]);
    const float fg = sigf(pre[2] + fgb);
    const float og = sigf(pre[3]);
    const float c_prev = has_prev ? bf16_bits_to_float(c_prev_u[e]) : 0.f;
    const float m_prev = has_prev ? bf16_bits_to_float(m_prev_u[e]) : 0.f;
    float cn = fg * c_prev + ig * cand;
    if (cap > 0.f) cn = fminf(cap, fmaxf(-cap, cn));
    const float mn = og * tanhf(cn);
    const float p = pv[e];
    c[(st + row) * h + j] =
        float_to_bf16_bits(cn * (1.f - p) + c_prev * p);
    m[(st + row) * h + j] =
        float_to_bf16_bits(mn * (1.f - p) + m_prev * p);
  }
}

// ---------------------------------------------------------------------------
// Backward step (s descending). GEMM prologue
//   dm_gemm[b, j0..] = dgates[t_next][B,4H] @ Wm[j0.., :]^T   (K = 4H)
// is K-split over the waves (wave w takes gate w's H columns of K) and
// reduced through LDS; skipped at the first processed step. The carries
// dc_carry / dm_pass stay fp32 in [D,B,H] scratch between launches.
// ---------------------------------------------------------------------------
template <int MT>
__global__ __launch_bounds__(256) void lstm_scan_step_bwd(
    const unsigned short* __restrict__ gates,
    const unsigned short* __restrict__ c, const float* __restrict__ pad,
    const unsigned short* __restrict__ wm,
    const unsigned short* __restrict__ dm_out,
    const unsigned short* __restrict__ dc_out,
    unsigned short* __restrict__ dgates, float* __restrict__ dc_carry,
    float* __restrict__ dm_pass, int t_len, int b, int h, int s,
    int rev_mask, float fgb, float cap) {
  const int j0 = blockIdx.x * 16;
  const int m0 = blockIdx.y * (16 * MT);
  const int d = blockIdx.z;
  const bool rev = (rev_mask >> d) & 1;
  const int t = rev ? t_len - 1 - s : s;
  const int t_prev = rev ? t + 1 : t - 1;
  const int t_next = rev ? t - 1 : t + 1;
  const bool has_prev = s > 0;
  const bool has_next = s < t_len - 1;
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int cl = lane & 15;

  __shared__ float red[4][16 * MT][16];  // per-wave K-split partials

  const long st = ((long)d * t_len + t) * b;
  const long sp = ((long)d * t_len + t_prev) * b;
  const long sn = ((long)d * t_len + t_next) * b;

  // Pointwise operands of this thread's MT elements, ahead of the GEMM.
  const int lc = threadIdx.x & 15;
  const int j = j0 + lc;
  // Unconditional raw loads, as in the forward kernel: what a missing
  // input would have supplied is read from a valid stand-in (c for a null
  // dm_out / dc_out, this step's slot for a missing previous step, the
  // not yet started carries at the first processed step) and discarded
  // after the GEMM.
  const long sq = has_prev ? sp : st;
  const unsigned short* dm_src = dm_out ? dm_out : c;
  const unsigned short* dc_src = dc_out ? dc_out : c;
  unsigned short gin[MT][4], c_prev_u[MT], dm_out_u[MT], dc_out_u[MT];
  float pv[MT], dm_in[MT], dc_in[MT];
#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const int rowc = min(m0 + e * 16 + (threadIdx.x >> 4), b - 1);
    const unsigned short* gr = gates + (st + rowc) * 4 * h + j;
    const long co = ((long)d * b + rowc) * h + j;  // [D,B,H] carry offset
#pragma unroll
    for (int q = 0; q < 4; ++q) gin[e][q] = gr[q * h];
    pv[e] = pad[(long)t * b + rowc];
    c_prev_u[e] = c[(sq + rowc) * h + j];
    dm_out_u[e] = dm_src[(st + rowc) * h + j];
    dc_out_u[e] = dc_src[(st + rowc) * h + j];
    dm_in[e] = dm_pass[co];
    dc_in[e] = dc_carry[co];
  }

  if (has_next) {
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
    const unsigned short* brow =
        wm + ((long)d * h + j0 + cl) * 4 * h + (long)wid * h + g * 8;
    const unsigned short* arow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      arow[mt] = dgates + (sn + min(m0 + mt * 16 + cl, b - 1)) * 4 * h +
                 (long)wid * h + g * 8;
    }
    tile_gemm<MT>(arow, brow, h, acc);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        red[wid][mt * 16 + g * 4 + r][cl] = acc[mt][r];
      }
    }
  }
  __syncthreads();

#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const int lrow = e * 16 + (threadIdx.x >> 4);
    const int row = m0 + lrow;
    if (row >= b) continue;
    const long co = ((long)d * b + row) * h + j;
    const float p = pv[e];
    float dmt = dm_out ? bf16_bits_to_float(dm_out_u[e]) : 0.f;
    float dct = dc_out ? bf16_bits_to_float(dc_out_u[e]) : 0.f;
    if (has_next) {
      dmt += red[0][lrow][lc] + red[1][lrow][lc] + red[2][lrow][lc] +
             red[3][lrow][lc] + dm_in[e];
      dct += dc_in[e];
    }

    const float cand = tanhf(bf16_bits_to_float(gin[e][0]));
    const float ig = sigf(bf16_bits_to_float(gin[e][1]));
    const float fg = sigf(bf16_bits_to_float(gin[e][2]) + fgb);
    const float og = sigf(bf16_bits_to_float(gin[e][3]));
    const float c_prev = has_prev ? bf16_bits_to_float(c_prev_u[e]) : 0.f;
    // c~ from this recomputation: the stored c[t] is post-blend.
    const float craw = fg * c_prev + ig * cand;
    float cn = craw;
    if (cap > 0.f) cn = fminf(cap, fmaxf(-cap, cn));
    const float tc = tanhf(cn);

    const float dml = (1.f - p) * dmt;  // live (unpadded) share
    const float do_ = dml * tc;
    float dc = (1.f - p) * dct + dml * og * (1.f - tc * tc);
    if (cap > 0.f && (craw > cap || craw < -cap)) dc = 0.f;

    unsigned short* dgr = dgates + (st + row) * 4 * h + j;
    dgr[0] = float_to_bf16_bits(dc * ig * (1.f - cand * cand));
    dgr[h] = float_to_bf16_bits(dc * cand * ig * (1.f - ig));
    dgr[2 * h] = float_to_bf16_bits(dc * c_prev * fg * (1.f - fg));
    dgr[3 * h] = float_to_bf16_bits(do_ * og * (1.f - og));
    dc_carry[co] = dc * fg + p * dct;
    dm_pass[co] = p * dmt;
  }
}

void check_bf16(const torch::Tensor& x, const char* name) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                  x.scalar_type() == torch::kBFloat16,
              name, " must be a contiguous bf16 device tensor");
}

void check_f32(const torch::Tensor& x, const char* name) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                  x.scalar_type() == torch::kFloat32,
              name, " must be a contiguous fp32 device tensor");
}

// Rows per workgroup: 16 * MT. rows == 0 picks the default.
int pick_mt(int64_t rows) {
  if (rows == 0) rows = 32;
  TORCH_CHECK(rows == 16 || rows == 32 || rows == 64 || rows == 128,
              "rows_per_block must be 0, 16, 32, 64 or 128");
  return (int)rows / 16;
}

}  // namespace

// Runs scan steps s_begin .. s_end-1 (ascending), one launch per step.
void lstm_scan_fwd(torch::Tensor gates, torch::Tensor c, torch::Tensor m,
                   torch::Tensor pad, torch::Tensor wmt, int64_t rev_mask,
                   double fgb, double cap, int64_t s_begin, int64_t s_end,
                   int64_t rows_per_block) {
  check_bf16(gates, "gates");
  check_bf16(c, "c");
  check_bf16(m, "m");
  check_bf16(wmt, "WmT");
  check_f32(pad, "pad");
  TORCH_CHECK(gates.dim() == 4 && c.dim() == 4, "gates/c must be 4-D");
  const int dn = gates.size(0), t = gates.size(1), b = gates.size(2);
  const int h = c.size(3);
  TORCH_CHECK(h % 32 == 0, "H % 32 == 0");
  TORCH_CHECK(dn >= 1 && dn <= 2 && t >= 1 && b >= 1, "bad D/T/B");
  TORCH_CHECK(gates.size(3) == 4 * h, "gates last dim must be 4H");
  TORCH_CHECK(c.sizes() == torch::IntArrayRef({dn, t, b, h}), "c shape");
  TORCH_CHECK(m.sizes() == c.sizes(), "m shape");
  TORCH_CHECK(pad.sizes() == torch::IntArrayRef({t, b}), "pad shape");
  TORCH_CHECK(wmt.sizes() == torch::IntArrayRef({dn, 4 * h, h}),
              "WmT shape");
  TORCH_CHECK(0 <= s_begin && s_begin <= s_end && s_end <= t, "step range");
  TORCH_CHECK(rev_mask >= 0 && (rev_mask >> dn) == 0,
              "rev_mask has bits beyond the D directions");
  const int mt = pick_mt(rows_per_block);
  const dim3 grid(h / 16, cdiv(b, 16 * mt), dn);
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_FWD(MT)                                                     \
  hipLaunchKernelGGL(                                                      \
      lstm_scan_step_fwd<MT>, grid, dim3(256), 0, stream,                  \
      (unsigned short*)gates.data_ptr(), (unsigned short*)c.data_ptr(),    \
      (unsigned short*)m.data_ptr(), pad.data_ptr<float>(),                \
      (const unsigned short*)wmt.data_ptr(), t, b, h, s, (int)rev_mask,    \
      (float)fgb, (float)cap)
  for (int s = (int)s_begin; s < (int)s_end; ++s) {
    switch (mt) {
      case 1: LAUNCH_FWD(1); break;
      case 2: LAUNCH_FWD(2); break;
      case 4: LAUNCH_FWD(4); break;
      default: LAUNCH_FWD(8); break;
    }
    LV_CHECK_HIP(hipGetLastError());
  }
#undef LAUNCH_FWD
}

// Runs scan steps s_end-1 .. s_begin (descending), one launch per step.
// The step s == T-1 starts the carries; later calls continue from the
// scratch left by the previous one.
void lstm_scan_bwd(torch::Tensor gates, torch::Tensor c, torch::Tensor pad,
                   torch::Tensor wm, c10::optional<torch::Tensor> dm_out,
                   c10::optional<torch::Tensor> dc_out,
                   torch::Tensor dgates, torch::Tensor dc_carry,
                   torch::Tensor dm_pass, int64_t rev_mask, double fgb,
                   double cap, int64_t s_begin, int64_t s_end,
                   int64_t rows_per_block) {
  check_bf16(gates, "gates");
  check_bf16(c, "c");
  check_bf16(wm, "Wm");
  check_bf16(dgates, "dgates");
  check_f32(pad, "pad");
  check_f32(dc_carry, "dc_carry");
  check_f32(dm_pass, "dm_pass");
  TORCH_CHECK(gates.dim() == 4 && c.dim() == 4, "gates/c must be 4-D");
  const int dn = gates.size(0), t = gates.size(1), b = gates.size(2);
  const int h = c.size(3);
  TORCH_CHECK(h % 32 == 0, "H % 32 == 0");
  TORCH_CHECK(dn >= 1 && dn <= 2 && t >= 1 && b >= 1, "bad D/T/B");
  TORCH_CHECK(gates.size(3) == 4 * h, "gates last dim must be 4H");
  TORCH_CHECK(c.sizes() == torch::IntArrayRef({dn, t, b, h}), "c shape");
  TORCH_CHECK(dgates.sizes() == gates.sizes(), "dgates shape");
  TORCH_CHECK(pad.sizes() == torch::IntArrayRef({t, b}), "pad shape");
  TORCH_CHECK(wm.sizes() == torch::IntArrayRef({dn, h, 4 * h}), "Wm shape");
  TORCH_CHECK(dc_carry.sizes() == torch::IntArrayRef({dn, b, h}) &&
                  dm_pass.sizes() == dc_carry.sizes(),
              "carry scratch shape");
  const unsigned short* dmp = nullptr;
  const unsigned short* dcp = nullptr;
  if (dm_out.has_value()) {
    check_bf16(*dm_out, "dm_out");
    TORCH_CHECK(dm_out->sizes() == c.sizes(), "dm_out shape");
    dmp = (const unsigned short*)dm_out->data_ptr();
  }
  if (dc_out.has_value()) {
    check_bf16(*dc_out, "dc_out");
    TORCH_CHECK(dc_out->sizes() == c.sizes(), "dc_out shape");
    dcp = (const unsigned short*)dc_out->data_ptr();
  }
  TORCH_CHECK(0 <= s_begin && s_begin <= s_end && s_end <= t, "step range");
  TORCH_CHECK(rev_mask >= 0 && (rev_mask >> dn) == 0,
              "rev_mask has bits beyond the D directions");
  const int mt = pick_mt(rows_per_block);
  const dim3 grid(h / 16, cdiv(b, 16 * mt), dn);
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_BWD(MT)                                                     \
  hipLaunchKernelGGL(                                                      \
      lstm_scan_step_bwd<MT>, grid, dim3(256), 0, stream,                  \
      (const unsigned short*)gates.data_ptr(),                             \
      (const unsigned short*)c.data_ptr(), pad.data_ptr<float>(),          \
      (const unsigned short*)wm.data_ptr(), dmp, dcp,                      \
      (unsigned short*)dgates.data_ptr(), dc_carry.data_ptr<float>(),      \
      dm_pass.data_ptr<float>(), t, b, h, s, (int)rev_mask, (float)fgb,    \
      (float)cap)
  for (int s = (int)s_end - 1; s >= (int)s_begin; --s) {
    switch (mt) {
      case 1: LAUNCH_BWD(1); break;
      case 2: LAUNCH_BWD(2); break;
      case 4: LAUNCH_BWD(4); break;
      default: LAUNCH_BWD(8); break;
    }
    LV_CHECK_HIP(hipGetLastError());
  }
#undef LAUNCH_BWD
}
