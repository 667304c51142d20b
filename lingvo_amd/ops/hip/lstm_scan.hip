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
#include "host_checks.h"
#include "lstm_cell.h"
#include "mfma.h"
#include "tile_gemm.h"

namespace {

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
  const StepThread th = step_thread();

  __shared__ float rec[4][16 * MT][16];  // recurrent term per gate

  const long st = ((long)d * t_len + t) * b;         // row base at t
  const long sp = ((long)d * t_len + t_prev) * b;    // row base at t_prev

  // Pointwise operands of this thread's MT elements, ahead of the GEMM.
  const int j = j0 + th.lc;
  // Every load is unconditional and kept as raw bits: a branch or a
  // conversion here would wait for these loads before the GEMM has issued
  // its own. Without a previous step the state loads read (and discard)
  // this step's not yet written slots.
  const long sq = has_prev ? sp : st;
  unsigned short gin[MT][4], c_prev_u[MT], m_prev_u[MT];
  float pv[MT];
#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const int rowc = min(m0 + e * 16 + th.lr, b - 1);
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
        wmt + ((long)d * 4 * h + (long)th.wid * h + j0 + th.cl) * h + th.g * 8;
    const unsigned short* arow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      arow[mt] = m + (sp + min(m0 + mt * 16 + th.cl, b - 1)) * h + th.g * 8;
    }
    tile_gemm<MT>(arow, brow, h, acc);
  }
  park_acc<MT>(rec[th.wid], th.g, th.cl, acc);
  __syncthreads();

#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const int lrow = e * 16 + th.lr;
    const int row = m0 + lrow;
    if (row >= b) continue;
    unsigned short* gr = gates + (st + row) * 4 * h + j;
    float pre[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // Round to bf16 first: backward recomputes from the stored value.
      const unsigned short u =
          float_to_bf16_bits(bf16_bits_to_float(gin[e][q]) +
                             rec[q][lrow][th.lc]);
      gr[q * h] = u;
      pre[q] = bf16_bits_to_float(u);
    }
    const LstmActs a = lstm_acts(pre[0], pre[1], pre[2], pre[3], fgb);
    const float c_prev = has_prev ? bf16_bits_to_float(c_prev_u[e]) : 0.f;
    const float m_prev = has_prev ? bf16_bits_to_float(m_prev_u[e]) : 0.f;
    const float cn = lstm_cell_update(a, c_prev, cap).c;
    const float mn = a.og * tanhf(cn);
    // Padding blend: a padded step (p = 1) carries the state through.
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
  const StepThread th = step_thread();

  __shared__ float red[4][16 * MT][16];  // per-wave K-split partials

  const long st = ((long)d * t_len + t) * b;
  const long sp = ((long)d * t_len + t_prev) * b;
  const long sn = ((long)d * t_len + t_next) * b;

  // Pointwise operands of this thread's MT elements, ahead of the GEMM.
  const int j = j0 + th.lc;
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
    const int rowc = min(m0 + e * 16 + th.lr, b - 1);
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
    const unsigned short* brow = wm + ((long)d * h + j0 + th.cl) * 4 * h +
                                 (long)th.wid * h + th.g * 8;
    const unsigned short* arow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      arow[mt] = dgates + (sn + min(m0 + mt * 16 + th.cl, b - 1)) * 4 * h +
                 (long)th.wid * h + th.g * 8;
    }
    tile_gemm<MT>(arow, brow, h, acc);
    park_acc<MT>(red[th.wid], th.g, th.cl, acc);
  }
  __syncthreads();

#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const int lrow = e * 16 + th.lr;
    const int row = m0 + lrow;
    if (row >= b) continue;
    const long co = ((long)d * b + row) * h + j;
    const float p = pv[e];
    float dmt = dm_out ? bf16_bits_to_float(dm_out_u[e]) : 0.f;
    float dct = dc_out ? bf16_bits_to_float(dc_out_u[e]) : 0.f;
    if (has_next) {
      dmt += sum_partials(red, lrow, th.lc) + dm_in[e];
      dct += dc_in[e];
    }

    const LstmActs a = lstm_acts(
        bf16_bits_to_float(gin[e][0]), bf16_bits_to_float(gin[e][1]),
        bf16_bits_to_float(gin[e][2]), bf16_bits_to_float(gin[e][3]), fgb);
    const float c_prev = has_prev ? bf16_bits_to_float(c_prev_u[e]) : 0.f;
    // c~ from this recomputation: the stored c[t] is post-blend.
    const LstmC cn = lstm_cell_update(a, c_prev, cap);
    // Padding blend: the live share (1 - p) of dm and dc goes through the
    // cell, the padded share p straight to the previous step.
    const LstmGrads dg = lstm_cell_bwd(a, c_prev, tanhf(cn.c), cn.raw, cap,
                                       (1.f - p) * dmt, (1.f - p) * dct);

    unsigned short* dgr = dgates + (st + row) * 4 * h + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) dgr[q * h] = float_to_bf16_bits(dg.dg[q]);
    dc_carry[co] = dg.dc_prev + p * dct;
    dm_pass[co] = p * dmt;
  }
}

constexpr auto kBf16 = torch::kBFloat16;
constexpr auto kF32 = torch::kFloat32;

struct ScanDims {
  int dn, t, b, h;
};

// The operands, step range and direction mask both sweeps take.
ScanDims check_scan(const torch::Tensor& gates, const torch::Tensor& c,
                    const torch::Tensor& pad, int64_t rev_mask,
                    int64_t s_begin, int64_t s_end) {
  check_contig(gates, kBf16, "gates");
  check_contig(c, kBf16, "c");
  check_contig(pad, kF32, "pad");
  TORCH_CHECK(gates.dim() == 4 && c.dim() == 4, "gates/c must be 4-D");
  const int dn = gates.size(0), t = gates.size(1), b = gates.size(2);
  const int h = c.size(3);
  TORCH_CHECK(h % 32 == 0, "H % 32 == 0");
  TORCH_CHECK(dn >= 1 && dn <= 2 && t >= 1 && b >= 1, "bad D/T/B");
  TORCH_CHECK(gates.size(3) == 4 * h, "gates last dim must be 4H");
  TORCH_CHECK(c.sizes() == torch::IntArrayRef({dn, t, b, h}), "c shape");
  TORCH_CHECK(pad.sizes() == torch::IntArrayRef({t, b}), "pad shape");
  TORCH_CHECK(0 <= s_begin && s_begin <= s_end && s_end <= t, "step range");
  TORCH_CHECK(rev_mask >= 0 && (rev_mask >> dn) == 0,
              "rev_mask has bits beyond the D directions");
  return {dn, t, b, h};
}

}  // namespace

// Runs scan steps s_begin .. s_end-1 (ascending), one launch per step.
void lstm_scan_fwd(torch::Tensor gates, torch::Tensor c, torch::Tensor m,
                   torch::Tensor pad, torch::Tensor wmt, int64_t rev_mask,
                   double fgb, double cap, int64_t s_begin, int64_t s_end,
                   int64_t rows_per_block) {
  const ScanDims z = check_scan(gates, c, pad, rev_mask, s_begin, s_end);
  const int dn = z.dn, t = z.t, b = z.b, h = z.h;
  check_contig(m, kBf16, "m");
  check_contig(wmt, kBf16, "WmT");
  TORCH_CHECK(m.sizes() == c.sizes(), "m shape");
  TORCH_CHECK(wmt.sizes() == torch::IntArrayRef({dn, 4 * h, h}),
              "WmT shape");
  const int mt = step_mt(rows_per_block, 1);
  const dim3 grid(h / 16, cdiv(b, 16 * mt), dn);
  auto stream = at::cuda::getCurrentCUDAStream();
  for (int s = (int)s_begin; s < (int)s_end; ++s) {
    dispatch_mt<1>(mt, [&](auto mt_c) {
      hipLaunchKernelGGL(
          lstm_scan_step_fwd<decltype(mt_c)::value>, grid, dim3(256), 0,
          stream, u16(gates), u16(c), u16(m), pad.data_ptr<float>(),
          u16(wmt), t, b, h, s, (int)rev_mask, (float)fgb, (float)cap);
    });
    LV_CHECK_HIP(hipGetLastError());
  }
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
  const ScanDims z = check_scan(gates, c, pad, rev_mask, s_begin, s_end);
  const int dn = z.dn, t = z.t, b = z.b, h = z.h;
  check_contig(wm, kBf16, "Wm");
  check_contig(dgates, kBf16, "dgates");
  check_contig(dc_carry, kF32, "dc_carry");
  check_contig(dm_pass, kF32, "dm_pass");
  TORCH_CHECK(dgates.sizes() == gates.sizes(), "dgates shape");
  TORCH_CHECK(wm.sizes() == torch::IntArrayRef({dn, h, 4 * h}), "Wm shape");
  TORCH_CHECK(dc_carry.sizes() == torch::IntArrayRef({dn, b, h}) &&
                  dm_pass.sizes() == dc_carry.sizes(),
              "carry scratch shape");
  const unsigned short* dmp = nullptr;
  const unsigned short* dcp = nullptr;
  if (dm_out.has_value()) {
    check_contig(*dm_out, kBf16, "dm_out");
    TORCH_CHECK(dm_out->sizes() == c.sizes(), "dm_out shape");
    dmp = (const unsigned short*)dm_out->data_ptr();
  }
  if (dc_out.has_value()) {
    check_contig(*dc_out, kBf16, "dc_out");
    TORCH_CHECK(dc_out->sizes() == c.sizes(), "dc_out shape");
    dcp = (const unsigned short*)dc_out->data_ptr();
  }
  const int mt = step_mt(rows_per_block, 1);
  const dim3 grid(h / 16, cdiv(b, 16 * mt), dn);
  auto stream = at::cuda::getCurrentCUDAStream();
  for (int s = (int)s_end - 1; s >= (int)s_begin; --s) {
    dispatch_mt<1>(mt, [&](auto mt_c) {
      hipLaunchKernelGGL(
          lstm_scan_step_bwd<decltype(mt_c)::value>, grid, dim3(256), 0,
          stream, u16(gates), u16(c), pad.data_ptr<float>(), u16(wm), dmp,
          dcp, u16(dgates), dc_carry.data_ptr<float>(),
          dm_pass.data_ptr<float>(), t, b, h, s, (int)rev_mask, (float)fgb,
          (float)cap);
    });
    LV_CHECK_HIP(hipGetLastError());
  }
}
