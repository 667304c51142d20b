// Fused LAS decoder recurrence stages for gfx950: the step GEMMs of the
// teacher-forced decoder (ops/las_decoder.py) with the LSTM cell and the
// glue around it as their epilogue, after the design of lstm_scan.hip.
//
//  - las_step_fwd: one launch per LSTM layer and step.
//      gates = bf16(A1 @ Wt[:, :K1]^T + A2 @ Wt[:, K1:K1+K2]^T + pre)
//    (fp32 accumulation, ONE rounding), then the cell of lstm_gates.hip on
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
#include "mfma.h"
#include "tile_gemm.h"

namespace {

__device__ __forceinline__ float sigf(float x) {
  return 1.f / (1.f + __expf(-x));
}

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
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int cl = lane & 15;

  __shared__ float rec[4][16 * MT][16];  // GEMM term per gate

  // Pointwise operands of this thread's MT elements (element e is tile
  // row e*16 + tid/16, column tid%16), loaded ahead of the GEMM as raw
  // bits. The c_prev branch is on a kernel argument: it waits on nothing.
  const int lc = threadIdx.x & 15;
  const int j = j0 + lc;
  unsigned short pin[MT][4], c_prev_u[MT];
#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const int rowc = min(m0 + e * 16 + (threadIdx.x >> 4), b - 1);
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
        wt + ((long)wid * h + j0 + cl) * ldw + g * 8;
    const unsigned short* a1row[MT];
    const unsigned short* a2row[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const long row = min(m0 + mt * 16 + cl, b - 1);
      a1row[mt] = a1 + row * lda1 + g * 8;
      a2row[mt] = a2 + row * lda2 + g * 8;
    }
    tile_gemm2<MT>(a1row, k1, a2row, k2, brow, acc);
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
    unsigned short* gr = gates + (long)row * 4 * h + j;
    float p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // Round to bf16 first: backward recomputes from the stored value.
      const unsigned short u = float_to_bf16_bits(
          rec[q][lrow][lc] + bf16_bits_to_float(pin[e][q]));
      gr[q * h] = u;
      p[q] = bf16_bits_to_float(u);
    }
    const float cand = tanhf(p[0]);
    const float ig = sigf(p[1]);
    const float fg = sigf(p[2] + fgb);
    const float og = sigf(p[3]);
    float cn = fg * bf16_bits_to_float(c_prev_u[e]) + ig * cand;
    if (cap > 0.f) cn = fminf(cap, fmaxf(-cap, cn));
    c_out[(long)row * h + j] = float_to_bf16_bits(cn);
    m_out[(long)row * h + j] = float_to_bf16_bits(og * tanhf(cn));
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
  const int wid = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4;
  const int cl = lane & 15;

  __shared__ float red[4][16 * MT][16];  // per-wave K-split partials

  const int lc = threadIdx.x & 15;
  const int j = j0 + lc;
  // Raw loads ahead of the GEMM. Every branch here is on kernel arguments
  // or blockIdx alone.
  unsigned short gin[MT][4], c_prev_u[MT], add_b_u[MT];
  float add_f_v[MT], dc_in[MT];
#pragma unroll
  for (int e = 0; e < MT; ++e) {
    const long rowc = min(m0 + e * 16 + (threadIdx.x >> 4), b - 1);
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
    const int k_lo = wid * kq;
    const int k_hi = min(k, k_lo + kq);
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = {0.f, 0.f, 0.f, 0.f};
    const unsigned short* brow = wt + (long)(n0 + cl) * ldw + k_lo + g * 8;
    const unsigned short* arow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      arow[mt] = a + (long)min(m0 + mt * 16 + cl, b - 1) * lda + k_lo + g * 8;
    }
    tile_gemm<MT>(arow, brow, k_hi - k_lo, acc);
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
    const long so = (long)row * h + j;
    const float gemm = red[0][lrow][lc] + red[1][lrow][lc] +
                       red[2][lrow][lc] + red[3][lrow][lc];
    if (!cell) {
      pass_out[so] = gemm;
      continue;
    }
    const float dm = gemm + bf16_bits_to_float(add_b_u[e]) + add_f_v[e];

    const float cand = tanhf(bf16_bits_to_float(gin[e][0]));
    const float ig = sigf(bf16_bits_to_float(gin[e][1]));
    const float fg = sigf(bf16_bits_to_float(gin[e][2]) + fgb);
    const float og = sigf(bf16_bits_to_float(gin[e][3]));
    const float c0v = bf16_bits_to_float(c_prev_u[e]);
    const float craw = fg * c0v + ig * cand;
    float cn = craw;
    if (cap > 0.f) cn = fminf(cap, fmaxf(-cap, cn));
    const float tc = tanhf(cn);

    const float do_ = dm * tc;
    float dc = dc_in[e] + dm * og * (1.f - tc * tc);
    if (cap > 0.f && (craw > cap || craw < -cap)) dc = 0.f;

    unsigned short* dgr = dgates + (long)row * 4 * h + j;
    dgr[0] = float_to_bf16_bits(dc * ig * (1.f - cand * cand));
    dgr[h] = float_to_bf16_bits(dc * cand * ig * (1.f - ig));
    dgr[2 * h] = float_to_bf16_bits(dc * c0v * fg * (1.f - fg));
    dgr[3 * h] = float_to_bf16_bits(do_ * og * (1.f - og));
    dc_carry[so] = dc * fg;
  }
}

// ---------------------------------------------------------------------------
// Host wrappers: every dtype, shape, stride and alignment is checked
// before the launch; nothing is allocated.
// ---------------------------------------------------------------------------

// Dense [rows, cols] tensor (a row of a contiguous stack is).
void check_dense(const torch::Tensor& t, torch::ScalarType st, int64_t rows,
                 int64_t cols, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == st && t.dim() == 2 &&
                  t.size(0) == rows && t.size(1) == cols &&
                  t.is_contiguous() && (uintptr_t)t.data_ptr() % 16 == 0,
              name, " must be a dense CUDA [", rows, ",", cols, "] tensor of ",
              st);
}

// bf16 [rows, K] read as MFMA fragments: unit column stride, 16-byte
// aligned rows, K % 32 == 0. Returns the row stride.
long check_frag_rows(const torch::Tensor& t, int64_t rows, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.dim() == 2 && t.size(0) == rows,
              name, " must be CUDA bf16 [", rows, ",K]");
  const int64_t k = t.size(1);
  TORCH_CHECK(k >= 32 && k % 32 == 0, name, ": K % 32 == 0");
  const int64_t ld = rows == 1 ? k : t.stride(0);
  TORCH_CHECK(t.stride(1) == 1 && ld >= k && ld % 8 == 0 &&
                  (uintptr_t)t.data_ptr() % 16 == 0,
              name, " must have unit column stride and 16-byte aligned rows");
  return (long)ld;
}

// bf16 [rows, cols] read element-wise with a row stride.
long check_strided_rows(const torch::Tensor& t, int64_t rows, int64_t cols,
                        const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.dim() == 2 && t.size(0) == rows && t.size(1) == cols &&
                  t.stride(1) == 1 && (rows == 1 || t.stride(0) >= cols),
              name, " must be CUDA bf16 [", rows, ",", cols,
              "] with unit column stride");
  return rows == 1 ? (long)cols : (long)t.stride(0);
}

// Rows per workgroup: 16 * MT. rows == 0 picks the default: 32 rows were
// the fastest of the three for every stage at B=512, H=640
// (docs/KERNEL_NOTES.md).
int pick_step_mt(int64_t rows) {
  if (rows == 0) rows = 32;
  TORCH_CHECK(rows == 32 || rows == 64 || rows == 128,
              "rows_per_block must be 0, 32, 64 or 128");
  return (int)rows / 16;
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
  TORCH_CHECK(wt.is_cuda() && wt.scalar_type() == torch::kBFloat16 &&
                  wt.dim() == 2 && wt.is_contiguous() &&
                  wt.size(0) == 4 * h && wt.size(1) >= k1 + k2 &&
                  wt.size(1) % 8 == 0 && (uintptr_t)wt.data_ptr() % 16 == 0,
              "wt must be CUDA contiguous bf16 [4H, >= K1+K2], ldw % 8 == 0");
  TORCH_CHECK(pre.is_cuda() && pre.scalar_type() == torch::kBFloat16 &&
                  pre.is_contiguous() &&
                  ((pre.dim() == 1 && pre.size(0) == 4 * h) ||
                   (pre.dim() == 2 && pre.size(0) == b &&
                    pre.size(1) == 4 * h)),
              "pre must be CUDA contiguous bf16 [4H] or [B,4H]");
  const unsigned short* cp = nullptr;
  if (c_prev.has_value()) {
    check_dense(*c_prev, torch::kBFloat16, b, h, "c_prev");
    cp = (const unsigned short*)c_prev->data_ptr();
  }
  const int mt = pick_step_mt(rows_per_block);
  const dim3 grid(h / 16, cdiv(b, 16 * mt));
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_FWD(MT)                                                      \
  hipLaunchKernelGGL(                                                       \
      las_step_fwd_kernel<MT>, grid, dim3(256), 0, stream, a1p, lda1,       \
      (int)k1, a2p, lda2, (int)k2, (const unsigned short*)wt.data_ptr(),    \
      (long)wt.size(1), (const unsigned short*)pre.data_ptr(),              \
      (long)(pre.dim() == 2 ? 4 * h : 0), cp,                               \
      (unsigned short*)gates.data_ptr(), (unsigned short*)c_out.data_ptr(), \
      (unsigned short*)m_out.data_ptr(), (int)b, (int)h, (float)fgb,        \
      (float)cap)
  switch (mt) {
    case 2: LAUNCH_FWD(2); break;
    case 4: LAUNCH_FWD(4); break;
    default: LAUNCH_FWD(8); break;
  }
#undef LAUNCH_FWD
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
  TORCH_CHECK(wt.is_cuda() && wt.scalar_type() == torch::kBFloat16 &&
                  wt.dim() == 2 && wt.is_contiguous() && wt.size(0) == n &&
                  wt.size(1) >= k && wt.size(1) % 8 == 0 &&
                  (uintptr_t)wt.data_ptr() % 16 == 0,
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
  const int mt = pick_step_mt(rows_per_block);
  const dim3 grid(n / 16, cdiv(b, 16 * mt));
  auto stream = at::cuda::getCurrentCUDAStream();
#define LAUNCH_BWD(MT)                                                     \
  hipLaunchKernelGGL(                                                      \
      las_cell_bwd_kernel<MT>, grid, dim3(256), 0, stream,                 \
      (const unsigned short*)a.data_ptr(), lda, (int)k,                    \
      (const unsigned short*)wt.data_ptr(), (long)wt.size(1), abp, ldb,    \
      afp, (const unsigned short*)gates.data_ptr(), cp,                    \
      dc_carry.data_ptr<float>(), (int)has_dc,                             \
      (unsigned short*)dgates.data_ptr(), pp, (int)b, (int)h, (float)fgb,  \
      (float)cap)
  switch (mt) {
    case 2: LAUNCH_BWD(2); break;
    case 4: LAUNCH_BWD(4); break;
    default: LAUNCH_BWD(8); break;
  }
#undef LAUNCH_BWD
  LV_CHECK_HIP(hipGetLastError());
}
