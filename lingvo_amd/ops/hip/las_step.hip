// Fused LAS decoder recurrence stages for gfx950: the step GEMMs of the
// teacher-forced decoder (ops/las_decoder.py) with the LSTM cell and the
// glue around it as their epilogue, on the step-kernel skeleton of
// tile_gemm.h that lstm_scan.hip uses too.
//
//  - las_step_fwd: one launch per LSTM layer and step.
//      gates = bf16(A1 @ Wt[:, :K1]^T + A2 @ Wt[:, K1:K1+K2]^T + pre)
//    (fp32 accumulation, ONE rounding), then the cell of lstm_cell.h on
//    the rounded gates; gates, c and m go straight into caller rows.
//  - las_cell_bwd: the cell backward with its data-gradient GEMM as
//    prologue,
//      dm = A @ Wt[:H]^T + add_b + add_f,   dc = dc_carry,
//    recomputing the cell from the stored gates and c_prev as
//    lstm_scan_step_bwd does; dgates goes into a caller row and dc_carry
//    (fp32) is updated in place. With N = 2H the workgroups of columns
//    >= H store their GEMM result to pass_out (fp32) instead: that is the
//    layer-1 -> layer-0 hand-over, where dgates1 @ wm1^T yields dm0 in its
//    first half and the next dm1 carry in its second.
//
// Grid (N/16, ceil(B / (16*MT))), block 256 = 4 waves. A workgroup owns 16
// hidden columns for 16*MT batch rows and is the only reader/writer of
// those (b, j) state elements, so the in-place dc_carry update is safe.
// Forward: wave w computes gate w over the full K. Backward: the K range
// is split over the four waves and reduced through LDS. Pointwise operands
// are loaded as raw bits before the GEMM; rows beyond B re-read row B-1 and
// are never stored. The only ordering between stages is the kernel boundary
// on one stream.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include <climits>
#include <cstdint>

#include "common.h"
#include "host_checks.h"
#include "lstm_cell.h"
#include "mfma.h"
#include "tile_gemm.h"

namespace {

// pre is [B,4H] (pre_ld = 4H) or a [4H] vector (pre_ld = 0). a1 / a2 are
// [B,K1] / [B,K2] with row strides lda1 / lda2; an empty range is skipped.
// c_prev == nullptr stands for a zero state.
template <int MT>
__global__ __launch_bounds__(256) void las_step_fwd_kernel(
    const unsigned short* __restrict__ a1, long lda1, int k1,
    const unsigned short* __restrict__ a2, long lda2, int k2,
    const unsigned short* __restrict__ wt, long ldw,
    const unsigned short* __restrict__ pre, long pre_ld,
    const unsigned short* __restrict__ c_prev,
    unsigned short* __restrict__ gates, unsigned short* __restrict__ c_out,
    unsigned short* __restrict__ m_out, int b, int h, float fgb, float cap) {
  const int j0 = blockIdx.x * 16;
  const int m0 = blockIdx.y * (16 * MT);
  const StepThread th = step_thread();

  __shared__ float rec[4][16 * MT][16];  // GEMM term per gate

  // Pointwise operands of this thread's MT elements, loaded ahead of the
  // GEMM as raw bits. The c_prev branch is on a kernel argument: it waits
  // on nothing.
  const int j = j0 + th.lc;
  unsigned short pin[MT][4], c_prev_u[MT];
#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const int rowc = min(m0 + e * 16 + th.lr, b - 1);
    const unsigned short* pr = pre + rowc * pre_ld + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) pin[e][q] = pr[q * h];
    c_prev_u[e] = c_prev ? c_prev[(long)rowc * h + j] : (unsigned short)0;
  }

  f32x4 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
  {
    const unsigned short* brow =
        wt + ((long)th.wid * h + j0 + th.cl) * ldw + th.g * 8;
    const unsigned short* a1row[MT];
    const unsigned short* a2row[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const long row = min(m0 + mt * 16 + th.cl, b - 1);
      a1row[mt] = a1 + row * lda1 + th.g * 8;
      a2row[mt] = a2 + row * lda2 + th.g * 8;
    }
    tile_gemm2<MT>(a1row, k1, a2row, k2, brow, acc);
  }
  park_acc<MT>(rec[th.wid], th.g, th.cl, acc);
  __syncthreads();

#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const int lrow = e * 16 + th.lr;
    const int row = m0 + lrow;
    if (row >= b) continue;
    unsigned short* gr = gates + (long)row * 4 * h + j;
    float p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // Round to bf16 first: backward recomputes from the stored value.
      const unsigned short u = float_to_bf16_bits(
          rec[q][lrow][th.lc] + bf16_bits_to_float(pin[e][q]));
      gr[q * h] = u;
      p[q] = bf16_bits_to_float(u);
    }
    const LstmActs a = lstm_acts(p[0], p[1], p[2], p[3], fgb);
    const float cn =
        lstm_cell_update(a, bf16_bits_to_float(c_prev_u[e]), cap).c;
    c_out[(long)row * h + j] = float_to_bf16_bits(cn);
    m_out[(long)row * h + j] = float_to_bf16_bits(a.og * tanhf(cn));
  }
}

// a [B,K] (row stride lda), wt [N,ldw] with N = H (pass_out == nullptr) or
// 2H. add_b (bf16, row stride ldb) and add_f (fp32 [B,H]) are optional
// addends of dm; has_dc says whether dc_carry holds a carry yet.
template <int MT>
__global__ __launch_bounds__(256) void las_cell_bwd_kernel(
    const unsigned short* __restrict__ a, long lda, int k,
    const unsigned short* __restrict__ wt, long ldw,
    const unsigned short* __restrict__ add_b, long ldb,
    const float* __restrict__ add_f,
    const unsigned short* __restrict__ gates,
    const unsigned short* __restrict__ c_prev, float* __restrict__ dc_carry,
    int has_dc, unsigned short* __restrict__ dgates,
    float* __restrict__ pass_out, int b, int h, float fgb, float cap) {
  const int n0 = blockIdx.x * 16;       // column of the GEMM result
  const bool cell = n0 < h;             // else: pass-through half
  const int j0 = cell ? n0 : n0 - h;    // hidden column
  const int m0 = blockIdx.y * (16 * MT);
  const StepThread th = step_thread();

  __shared__ float red[4][16 * MT][16];  // per-wave K-split partials

  const int j = j0 + th.lc;
  // Raw loads ahead of the GEMM. Every branch here is on kernel arguments
  // or blockIdx alone.
  unsigned short gin[MT][4], c_prev_u[MT], add_b_u[MT];
  float add_f_v[MT], dc_in[MT];
#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const long rowc = min(m0 + e * 16 + th.lr, b - 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) gin[e][q] = 0;
    c_prev_u[e] = 0;
    add_b_u[e] = 0;
    add_f_v[e] = 0.f;
    dc_in[e] = 0.f;
    if (cell) {
      const unsigned short* gr = gates + rowc * 4 * h + j;
#pragma unroll
      for (int q = 0; q < 4; ++q) gin[e][q] = gr[q * h];
      if (c_prev) c_prev_u[e] = c_prev[rowc * h + j];
      if (add_b) add_b_u[e] = add_b[rowc * ldb + j];
      if (add_f) add_f_v[e] = add_f[rowc * h + j];
      if (has_dc) dc_in[e] = dc_carry[rowc * h + j];
    }
  }

  {
    const int kq = (k / 32 + 3) / 4 * 32;  // per-wave K quota (mult of 32)
    const int k_lo = th.wid * kq;
    const int k_hi = min(k, k_lo + kq);
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
    const unsigned short* brow =
        wt + (long)(n0 + th.cl) * ldw + k_lo + th.g * 8;
    const unsigned short* arow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      arow[mt] = a + (long)min(m0 + mt * 16 + th.cl, b - 1) * lda + k_lo +
                 th.g * 8;
    }
    tile_gemm<MT>(arow, brow, k_hi - k_lo, acc);
    park_acc<MT>(red[th.wid], th.g, th.cl, acc);
  }
  __syncthreads();

#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const int lrow = e * 16 + th.lr;
    const int row = m0 + lrow;
    if (row >= b) continue;
    const long so = (long)row * h + j;
    const float gemm = sum_partials(red, lrow, th.lc);
    if (!cell) {
      pass_out[so] = gemm;
      continue;
    }
    const float dm = gemm + bf16_bits_to_float(add_b_u[e]) + add_f_v[e];

    // The cell recomputed in fp32 from the stored gates and c_prev.
    const LstmActs ac = lstm_acts(
        bf16_bits_to_float(gin[e][0]), bf16_bits_to_float(gin[e][1]),
        bf16_bits_to_float(gin[e][2]), bf16_bits_to_float(gin[e][3]), fgb);
    const float c0v = bf16_bits_to_float(c_prev_u[e]);
    const LstmC cn = lstm_cell_update(ac, c0v, cap);
    const LstmGrads dg =
        lstm_cell_bwd(ac, c0v, tanhf(cn.c), cn.raw, cap, dm, dc_in[e]);

    unsigned short* dgr = dgates + (long)row * 4 * h + j;
#pragma unroll
    for (int q = 0; q < 4; ++q) dgr[q * h] = float_to_bf16_bits(dg.dg[q]);
    dc_carry[so] = dg.dc_prev;
  }
}

// ---------------------------------------------------------------------------
// Host wrappers: every dtype, shape, stride and alignment is checked
// before the launch; nothing is allocated.
// ---------------------------------------------------------------------------

// bf16 [rows, K] read as MFMA fragments: unit column stride, 16-byte
// aligned rows, K % 32 == 0. Returns the row stride.
long check_frag_rows(const torch::Tensor& t, int64_t rows, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.dim() == 2 && t.size(0) == rows,
              name, " must be CUDA bf16 [", rows, ",K]");
  const int64_t k = t.size(1);
  TORCH_CHECK(k >= 32 && k % 32 == 0, name, ": K % 32 == 0");
  const int64_t ld = rows == 1 ? k : t.stride(0);
  TORCH_CHECK(t.stride(1) == 1 && ld >= k && ld % 8 == 0 && aligned16(t),
              name, " must have unit column stride and 16-byte aligned rows");
  return (long)ld;
}

// The [rows, >= k] weight operand of both stages.
bool weight_ok(const torch::Tensor& wt, int64_t rows, int64_t k) {
  return cuda_contig(wt, torch::kBFloat16) && wt.dim() == 2 &&
         wt.size(0) == rows && wt.size(1) >= k && wt.size(1) % 8 == 0 &&
         aligned16(wt);
}

}  // namespace

void las_step_fwd(c10::optional<torch::Tensor> a1,
                  c10::optional<torch::Tensor> a2, torch::Tensor wt,
                  torch::Tensor pre, c10::optional<torch::Tensor> c_prev,
                  torch::Tensor gates, torch::Tensor c_out,
                  torch::Tensor m_out, double fgb, double cap,
                  int64_t rows_per_block) {
  TORCH_CHECK(gates.dim() == 2 && c_out.dim() == 2, "gates/c_out must be 2-D");
  const int64_t b = gates.size(0), h = c_out.size(1);
  TORCH_CHECK(b >= 1 && h >= 16 && h % 16 == 0, "B >= 1 and H % 16 == 0");
  TORCH_CHECK(b * 4 * h <= INT_MAX, "B * 4H fits int");
  check_dense(gates, torch::kBFloat16, b, 4 * h, "gates");
  check_dense(c_out, torch::kBFloat16, b, h, "c_out");
  check_dense(m_out, torch::kBFloat16, b, h, "m_out");
  const unsigned short* a1p = nullptr;
  const unsigned short* a2p = nullptr;
  long lda1 = 0, lda2 = 0;
  int64_t k1 = 0, k2 = 0;
  if (a1.has_value()) {
    lda1 = check_frag_rows(*a1, b, "a1");
    k1 = a1->size(1);
    a1p = (const unsigned short*)a1->data_ptr();
  }
  if (a2.has_value()) {
    lda2 = check_frag_rows(*a2, b, "a2");
    k2 = a2->size(1);
    a2p = (const unsigned short*)a2->data_ptr();
  }
  TORCH_CHECK(weight_ok(wt, 4 * h, k1 + k2),
              "wt must be CUDA contiguous bf16 [4H, >= K1+K2], ldw % 8 == 0");
  TORCH_CHECK(cuda_contig(pre, torch::kBFloat16) &&
                  ((pre.dim() == 1 && pre.size(0) == 4 * h) ||
                   (pre.dim() == 2 && pre.size(0) == b &&
                    pre.size(1) == 4 * h)),
              "pre must be CUDA contiguous bf16 [4H] or [B,4H]");
  const unsigned short* cp = nullptr;
  if (c_prev.has_value()) {
    check_dense(*c_prev, torch::kBFloat16, b, h, "c_prev");
    cp = (const unsigned short*)c_prev->data_ptr();
  }
  const int mt = step_mt(rows_per_block, 2);
  const dim3 grid(h / 16, cdiv(b, 16 * mt));
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_mt<2>(mt, [&](auto mt_c) {
    hipLaunchKernelGGL(
        las_step_fwd_kernel<decltype(mt_c)::value>, grid, dim3(256), 0,
        stream, a1p, lda1, (int)k1, a2p, lda2, (int)k2, u16(wt),
        (long)wt.size(1), u16(pre), (long)(pre.dim() == 2 ? 4 * h : 0), cp,
        u16(gates), u16(c_out), u16(m_out), (int)b, (int)h, (float)fgb,
        (float)cap);
  });
  LV_CHECK_HIP(hipGetLastError());
}

void las_cell_bwd(torch::Tensor a, torch::Tensor wt,
                  c10::optional<torch::Tensor> add_b,
                  c10::optional<torch::Tensor> add_f, torch::Tensor gates,
                  c10::optional<torch::Tensor> c_prev, torch::Tensor dc_carry,
                  bool has_dc, torch::Tensor dgates,
                  c10::optional<torch::Tensor> pass_out, double fgb,
                  double cap, int64_t rows_per_block) {
  TORCH_CHECK(gates.dim() == 2 && dc_carry.dim() == 2,
              "gates/dc_carry must be 2-D");
  const int64_t b = gates.size(0), h = dc_carry.size(1);
  TORCH_CHECK(b >= 1 && h >= 16 && h % 16 == 0, "B >= 1 and H % 16 == 0");
  TORCH_CHECK(b * 4 * h <= INT_MAX, "B * 4H fits int");
  check_dense(gates, torch::kBFloat16, b, 4 * h, "gates");
  check_dense(dgates, torch::kBFloat16, b, 4 * h, "dgates");
  check_dense(dc_carry, torch::kFloat32, b, h, "dc_carry");
  const long lda = check_frag_rows(a, b, "a");
  const int64_t k = a.size(1);
  const int64_t n = pass_out.has_value() ? 2 * h : h;
  TORCH_CHECK(weight_ok(wt, n, k),
              "wt must be CUDA contiguous bf16 [H or 2H, >= K], ldw % 8 == 0");
  const unsigned short* abp = nullptr;
  long ldb = 0;
  if (add_b.has_value()) {
    ldb = check_strided_rows(*add_b, b, h, "add_b");
    abp = (const unsigned short*)add_b->data_ptr();
  }
  const float* afp = nullptr;
  if (add_f.has_value()) {
    check_dense(*add_f, torch::kFloat32, b, h, "add_f");
    afp = add_f->data_ptr<float>();
  }
  const unsigned short* cp = nullptr;
  if (c_prev.has_value()) {
    check_dense(*c_prev, torch::kBFloat16, b, h, "c_prev");
    cp = (const unsigned short*)c_prev->data_ptr();
  }
  float* pp = nullptr;
  if (pass_out.has_value()) {
    check_dense(*pass_out, torch::kFloat32, b, h, "pass_out");
    pp = pass_out->data_ptr<float>();
  }
  const int mt = step_mt(rows_per_block, 2);
  const dim3 grid(n / 16, cdiv(b, 16 * mt));
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_mt<2>(mt, [&](auto mt_c) {
    hipLaunchKernelGGL(
        las_cell_bwd_kernel<decltype(mt_c)::value>, grid, dim3(256), 0,
        stream, u16(a), lda, (int)k, u16(wt), (long)wt.size(1), abp, ldb, afp,
        u16(gates), cp, dc_carry.data_ptr<float>(), (int)has_dc, u16(dgates),
        pp, (int)b, (int)h, (float)fgb, (float)cap);
  });
  LV_CHECK_HIP(hipGetLastError());
}
