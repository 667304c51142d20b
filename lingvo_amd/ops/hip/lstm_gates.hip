// Fused LSTM gate pointwise math for gfx950: the cell of
// lstm_cell.h on stored gates, one kernel fwd / one bwd (recomputing
// activations from saved gates), replacing the ~12 eager pointwise kernels
// per step of the 'split' decoder loop and of the per-step cell layers.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include "common.h"
#include "host_checks.h"
#include "lstm_cell.h"

namespace {

// gr: the [4H] gate row of this element, col its hidden column.
__device__ __forceinline__ LstmActs load_acts(const unsigned short* gr,
                                              long col, int h, float fgb) {
  return lstm_acts(
      bf16_bits_to_float(gr[col]), bf16_bits_to_float(gr[h + col]),
      bf16_bits_to_float(gr[2 * h + col]),
      bf16_bits_to_float(gr[3 * h + col]), fgb);
}

__global__ void lstm_gates_fwd(const unsigned short* __restrict__ gates,
                               const unsigned short* __restrict__ c0,
                               unsigned short* __restrict__ c1,
                               unsigned short* __restrict__ m1, long n,
                               int h, float fgb, float cap) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const long row = i / h;
    const long col = i % h;
    const LstmActs a = load_acts(gates + row * 4 * h, col, h, fgb);
    const float c = lstm_cell_update(a, bf16_bits_to_float(c0[i]), cap).c;
    c1[i] = float_to_bf16_bits(c);
    m1[i] = float_to_bf16_bits(a.og * tanhf(c));
  }
}

__global__ void lstm_gates_bwd(const unsigned short* __restrict__ gates,
                               const unsigned short* __restrict__ c0,
                               const unsigned short* __restrict__ c1,
                               const unsigned short* __restrict__ dm1,
                               const unsigned short* __restrict__ dc1_ext,
                               unsigned short* __restrict__ dgates,
                               unsigned short* __restrict__ dc0, long n,
                               int h, float fgb, float cap) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x) {
    const long row = i / h;
    const long col = i % h;
    const LstmActs a = load_acts(gates + row * 4 * h, col, h, fgb);
    const float c0v = bf16_bits_to_float(c0[i]);
    // tanh of the STORED (bf16, post-clamp) c1, unlike the step kernels,
    // which recompute c in fp32; the clamp test is on the recomputed c.
    const float tc = tanhf(bf16_bits_to_float(c1[i]));
    const float dm = bf16_bits_to_float(dm1[i]);
    const float dc = dc1_ext ? bf16_bits_to_float(dc1_ext[i]) : 0.f;
    const LstmGrads d = lstm_cell_bwd(
        a, c0v, tc, lstm_cell_update(a, c0v, cap).raw, cap, dm, dc);
    unsigned short* dgr = dgates + row * 4 * h;
    dgr[col] = float_to_bf16_bits(d.dg[0]);
    dgr[h + col] = float_to_bf16_bits(d.dg[1]);
    dgr[2 * h + col] = float_to_bf16_bits(d.dg[2]);
    dgr[3 * h + col] = float_to_bf16_bits(d.dg[3]);
    dc0[i] = float_to_bf16_bits(d.dc_prev);
  }
}

// gates [..., 4H] and c0 [..., H], both contiguous bf16 on the device.
void check_gates_c0(const torch::Tensor& gates, const torch::Tensor& c0) {
  check_contig(gates, torch::kBFloat16, "gates");
  check_contig(c0, torch::kBFloat16, "c0");
  const int64_t nd = c0.dim();
  TORCH_CHECK(nd >= 1 && gates.dim() == nd &&
                  gates.sizes().slice(0, nd - 1) ==
                      c0.sizes().slice(0, nd - 1) &&
                  gates.size(-1) == 4 * c0.size(-1),
              "gates must be [..., 4H] for c0 [..., H]");
}

void check_like_c0(const torch::Tensor& t, const torch::Tensor& c0,
                   const char* name) {
  check_contig(t, torch::kBFloat16, name);
  TORCH_CHECK(t.sizes() == c0.sizes(), name, " must have the shape of c0");
}

}  // namespace

std::vector<torch::Tensor> lstm_gates_fwd_op(torch::Tensor gates,
                                             torch::Tensor c0, double fgb,
                                             double cap) {
  check_gates_c0(gates, c0);
  const long n = c0.numel();
  const int h = c0.size(-1);
  auto c1 = torch::empty_like(c0);
  auto m1 = torch::empty_like(c0);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(lstm_gates_fwd, dim3(memory_bound_grid(n, 256)),
                     dim3(256), 0, stream, u16(gates), u16(c0), u16(c1),
                     u16(m1), n, h, (float)fgb, (float)cap);
  return {c1, m1};
}

std::vector<torch::Tensor> lstm_gates_bwd_op(
    torch::Tensor gates, torch::Tensor c0, torch::Tensor c1,
    torch::Tensor dm1, c10::optional<torch::Tensor> dc1, double fgb,
    double cap) {
  check_gates_c0(gates, c0);
  check_like_c0(c1, c0, "c1");
  check_like_c0(dm1, c0, "dm1");
  if (dc1.has_value()) check_like_c0(*dc1, c0, "dc1");
  const long n = c0.numel();
  const int h = c0.size(-1);
  auto dgates = torch::empty_like(gates);
  auto dc0 = torch::empty_like(c0);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(lstm_gates_bwd, dim3(memory_bound_grid(n, 256)),
                     dim3(256), 0, stream, u16(gates), u16(c0), u16(c1),
                     u16(dm1), dc1.has_value() ? u16(*dc1) : nullptr,
                     u16(dgates), u16(dc0), n, h, (float)fgb, (float)cap);
  return {dgates, dc0};
}
