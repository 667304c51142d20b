// Depthwise 1-D time convolution fwd+bwd for gfx950 (SURVEY.md K7;
// reference op: lingvo/core/conv_layers_with_time_padding.py:608
// DepthwiseConv2DLayer / :717 CausalDepthwiseConv2DLayer with time-major
// paddings).
//
// x: [B, T, D] bf16 contiguous, w: [K, D] bf16, y: [B, T, D].
//   y[b,t,d] = sum_j x[b, t + j - pad, d] * w[j, d]   (+ bias[d])
// pad = K-1 for causal, (K-1)/2 for SAME. Out-of-range taps read 0.
// Inputs are pre-masked by paddings on the Python side; outputs are
// re-masked there too.
//
// Two routes. 'tiled' (dwconv_tiled.hip, the default) stages a time tile
// in LDS and slides a register window over it; it also has the fused
// GLU + padding front of the Conformer LConv (glu_dwconv1d_*). 'naive',
// below, is the yardstick: vectorized ushort8 IO, one thread per 8 channels
// of one (b, t) row, grid-stride; taps hit L1/L2 (row re-use across t).
// Each route has its own weight-gradient kernel; both write per-group
// fp32 partials that dwconv_bwd_dw_reduce sums in order.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <array>
#include <string>

#include "common.h"
#include "dwconv_tiled.h"

namespace {

constexpr int MAXK = 33;

// KT > 0: compile-time tap count (full unroll + software pipelining);
// KT == 0: runtime K fallback.
template <int KT>
__global__ void dwconv_fwd(const unsigned short* __restrict__ x,
                           const unsigned short* __restrict__ w,
                           const unsigned short* __restrict__ bias,
                           unsigned short* __restrict__ y, int B, int T,
                           int D, int Krt, int pad) {
  const int K = KT > 0 ? KT : Krt;
  const long nvec = (long)B * T * (D / 8);
  const int dvec = D / 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long)gridDim.x * blockDim.x) {
    const int dv = (int)(i % dvec);
    const long bt = i / dvec;
    const int t = (int)(bt % T);
    const long b = bt / T;
    float acc[8];
    if (bias) {
      ushortx8 bv = *reinterpret_cast<const ushortx8*>(bias + dv * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = bf16_bits_to_float(bv[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < (KT > 0 ? KT : 1); ++j) {
      if (KT == 0) break;
      int ts = t + j - pad;
      if (ts < 0 || ts >= T) continue;
      ushortx8 xv = *reinterpret_cast<const ushortx8*>(
          x + (b * T + ts) * D + dv * 8);
      ushortx8 wv = *reinterpret_cast<const ushortx8*>(w + j * D + dv * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        acc[e] += bf16_bits_to_float(xv[e]) * bf16_bits_to_float(wv[e]);
    }
    if (KT == 0) {
      for (int j = 0; j < K; ++j) {
        int ts = t + j - pad;
        if (ts < 0 || ts >= T) continue;
        ushortx8 xv = *reinterpret_cast<const ushortx8*>(
            x + (b * T + ts) * D + dv * 8);
        ushortx8 wv =
            *reinterpret_cast<const ushortx8*>(w + j * D + dv * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          acc[e] += bf16_bits_to_float(xv[e]) * bf16_bits_to_float(wv[e]);
      }
    }
    ushortx8 ov;
#pragma unroll
    for (int e = 0; e < 8; ++e) ov[e] = float_to_bf16_bits(acc[e]);
    *reinterpret_cast<ushortx8*>(y + (b * T + t) * D + dv * 8) = ov;
  }
}

template <int KT>
__global__ void dwconv_bwd_dx(const unsigned short* __restrict__ dy,
                              const unsigned short* __restrict__ w,
                              unsigned short* __restrict__ dx, int B, int T,
                              int D, int Krt, int pad) {
  const int K = KT > 0 ? KT : Krt;
  const long nvec = (long)B * T * (D / 8);
  const int dvec = D / 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long)gridDim.x * blockDim.x) {
    const int dv = (int)(i % dvec);
    const long bt = i / dvec;
    const int t = (int)(bt % T);
    const long b = bt / T;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
    for (int j = 0; j < (KT > 0 ? KT : 1); ++j) {
      if (KT == 0) break;
      int ty = t - j + pad;  // y position whose tap j touched x[t]
      if (ty < 0 || ty >= T) continue;
      ushortx8 gv = *reinterpret_cast<const ushortx8*>(
          dy + (b * T + ty) * D + dv * 8);
      ushortx8 wv = *reinterpret_cast<const ushortx8*>(w + j * D + dv * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        acc[e] += bf16_bits_to_float(gv[e]) * bf16_bits_to_float(wv[e]);
    }
    if (KT == 0) {
      for (int j = 0; j < K; ++j) {
        int ty = t - j + pad;
        if (ty < 0 || ty >= T) continue;
        ushortx8 gv = *reinterpret_cast<const ushortx8*>(
            dy + (b * T + ty) * D + dv * 8);
        ushortx8 wv =
            *reinterpret_cast<const ushortx8*>(w + j * D + dv * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          acc[e] += bf16_bits_to_float(gv[e]) * bf16_bits_to_float(wv[e]);
      }
    }
    ushortx8 ov;
#pragma unroll
    for (int e = 0; e < 8; ++e) ov[e] = float_to_bf16_bits(acc[e]);
    *reinterpret_cast<ushortx8*>(dx + (b * T + t) * D + dv * 8) = ov;
  }
}

// dw[j,d] = sum_{b,t} dy[b,t,d] * x[b,t+j-pad,d]; db[d] = sum dy.
// LDS-staged: each block owns 128 channels x a 64-row chunk; x and dy
// tiles are staged once (2-pass global traffic total), then 256 threads
// (d, tap-parity) accumulate from LDS. K/2 fp32 tap accumulators per
// thread; one atomicAdd per (tap, channel) per chunk-group.
constexpr int DW_CHUNK = 64;
constexpr int DW_DBLK = 128;

__global__ __launch_bounds__(256) void dwconv_bwd_dw(
    const unsigned short* __restrict__ dy,
    const unsigned short* __restrict__ x,
    float* __restrict__ dw_part,  // [ngroups, K, D] plain stores
    float* __restrict__ db_part,  // [ngroups, D]
    int B, int T, int D, int K, int pad,
    int ngroups) {
  // Thread decomposition (fully vectorized LDS reads): 16 d-groups of
  // 8 channels x 4 tap-quarters of 8 taps x 4 row-quarters of 16 rows.
  // Every x/dy access is a ushortx8 load; accumulators live in
  // registers across all chunks and flush once.
  // Row stride padded by 8 ushorts (4 banks): with an unpadded 128-
  // ushort (64-bank) stride, the 4 tap-quarter groups of a wave read
  // x_s rows 8 apart that land on IDENTICAL banks -> 4-way conflict on
  // every inner-loop LDS read.
  __shared__ unsigned short x_s[DW_CHUNK + MAXK - 1][DW_DBLK + 8];
  __shared__ unsigned short dy_s[DW_CHUNK][DW_DBLK + 8];
  const int tid = threadIdx.x;
  const int dg = tid & 15;          // d-group (8 channels)
  const int tq = (tid >> 4) & 3;    // tap quarter (taps 8tq..8tq+7)
  const int rq = tid >> 6;          // row quarter (rows 16rq..16rq+15)
  const int d0 = blockIdx.x * DW_DBLK + dg * 8;
  const long rows = (long)B * T;
  const int xrows = DW_CHUNK + K - 1;

  float dw8[8][8];
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
#pragma unroll
    for (int e = 0; e < 8; ++e) dw8[jj][e] = 0.f;
  }
  float db8[8] = {0, 0, 0, 0, 0, 0, 0, 0};

  const long nchunks = (rows + DW_CHUNK - 1) / DW_CHUNK;
  for (long c = blockIdx.y; c < nchunks; c += ngroups) {
    const long r0 = c * DW_CHUNK;
    for (int i = tid; i < xrows * (DW_DBLK / 8); i += 256) {
      int row = i / (DW_DBLK / 8);
      int d8 = (i % (DW_DBLK / 8)) * 8;
      long fr = r0 - pad + row;
      ushortx8 v;
      int gd = blockIdx.x * DW_DBLK + d8;
      if (fr >= 0 && fr < rows && gd + 7 < D) {
        v = *reinterpret_cast<const ushortx8*>(x + fr * D + gd);
      } else {
        for (int e = 0; e < 8; ++e) v[e] = 0;
      }
      *reinterpret_cast<ushortx8*>(&x_s[row][d8]) = v;
    }
    for (int i = tid; i < DW_CHUNK * (DW_DBLK / 8); i += 256) {
      int row = i / (DW_DBLK / 8);
      int d8 = (i % (DW_DBLK / 8)) * 8;
      long fr = r0 + row;
      ushortx8 v;
      int gd = blockIdx.x * DW_DBLK + d8;
      if (fr < rows && gd + 7 < D) {
        v = *reinterpret_cast<const ushortx8*>(dy + fr * D + gd);
      } else {
        for (int e = 0; e < 8; ++e) v[e] = 0;
      }
      *reinterpret_cast<ushortx8*>(&dy_s[row][d8]) = v;
    }
    __syncthreads();

    const int nrows = (int)min((long)DW_CHUNK, rows - r0);
    const int lr_hi = min((rq + 1) * 16, nrows);
    for (int lr = rq * 16; lr < lr_hi; ++lr) {
      ushortx8 gv = *reinterpret_cast<const ushortx8*>(&dy_s[lr][dg * 8]);
      float g[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = bf16_bits_to_float(gv[e]);
      const int t = (int)((r0 + lr) % T);
      if (tq == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) db8[e] += g[e];
      }
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int j = tq * 8 + jj;
        if (j >= K) break;
        const int ts = t + j - pad;
        if (ts < 0 || ts >= T) continue;
        ushortx8 xv =
            *reinterpret_cast<const ushortx8*>(&x_s[lr + j][dg * 8]);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          dw8[jj][e] += g[e] * bf16_bits_to_float(xv[e]);
        }
      }
    }
    __syncthreads();
  }

  // Cross-wave (rq) reduction in LDS, then ONE plain store per element
  // into this block's [K, DW_DBLK] partial slice. The previous global
  // atomicAdd flush serialized ~4k adds per dw address across the grid
  // and dominated the kernel's runtime.
  __shared__ float dw_lds[MAXK - 1][DW_DBLK];
  __shared__ float db_lds[DW_DBLK];
  for (int i = tid; i < K * DW_DBLK; i += 256) {
    dw_lds[i / DW_DBLK][i % DW_DBLK] = 0.f;
  }
  for (int i = tid; i < DW_DBLK; i += 256) db_lds[i] = 0.f;
  __syncthreads();
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    const int j = tq * 8 + jj;
    if (j >= K) break;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (dw8[jj][e] != 0.f) atomicAdd(&dw_lds[j][dg * 8 + e], dw8[jj][e]);
    }
  }
  if (tq == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (db8[e] != 0.f) atomicAdd(&db_lds[dg * 8 + e], db8[e]);
    }
  }
  __syncthreads();
  const long gbase = (long)blockIdx.y * K * D;
  for (int i = tid; i < K * DW_DBLK; i += 256) {
    const int j = i / DW_DBLK;
    const int d = blockIdx.x * DW_DBLK + i % DW_DBLK;
    if (d < D) dw_part[gbase + (long)j * D + d] = dw_lds[j][i % DW_DBLK];
  }
  for (int i = tid; i < DW_DBLK; i += 256) {
    const int d = blockIdx.x * DW_DBLK + i;
    if (d < D) db_part[(long)blockIdx.y * D + d] = db_lds[i];
  }
}

// Sums the per-group partials: dw[j][d] = sum_g dw_part[g][j][d].
__global__ void dwconv_bwd_dw_reduce(const float* __restrict__ dw_part,
                                     const float* __restrict__ db_part,
                                     float* __restrict__ dw,
                                     float* __restrict__ db, long kd, int D,
                                     int ngroups) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < kd + D;
       i += (long)gridDim.x * blockDim.x) {
    float sum = 0.f;
    if (i < kd) {
      for (int g = 0; g < ngroups; ++g) sum += dw_part[(long)g * kd + i];
      dw[i] = sum;
    } else {
      const long d = i - kd;
      for (int g = 0; g < ngroups; ++g) sum += db_part[(long)g * D + d];
      db[d] = sum;
    }
  }
}

}  // namespace

namespace {

const unsigned short* bf16_ptr(const torch::Tensor& t) {
  return (const unsigned short*)t.data_ptr();
}

const unsigned short* opt_ptr(const c10::optional<torch::Tensor>& t) {
  return t.has_value() ? bf16_ptr(*t) : nullptr;
}

bool is_bf16_cuda(const torch::Tensor& t) {
  return t.is_cuda() && t.is_contiguous() &&
         t.scalar_type() == torch::kBFloat16;
}

// 'auto' | 'naive' | 'tiled'. True for the tiled kernels, false for the
// per-thread tap loop.
bool pick_tiled(const std::string& route, int64_t B, int64_t T, int64_t D,
                int64_t K) {
  if (route == "naive") return false;
  const bool ok = dwconv_tiled_supported(B, T, D, K);
  if (route == "auto") return ok;
  TORCH_CHECK(route == "tiled",
              "route must be 'auto', 'naive' or 'tiled', got '", route, "'");
  TORCH_CHECK(ok, "route='tiled' does not support B=", B, " T=", T, " D=", D,
              " K=", K);
  return true;
}

// A caller-provided output, or a fresh one.
torch::Tensor out_or_empty(const c10::optional<torch::Tensor>& out,
                           at::IntArrayRef sizes,
                           const torch::TensorOptions& opts,
                           const char* name) {
  if (!out.has_value()) return torch::empty(sizes, opts);
  TORCH_CHECK(out->is_cuda() && out->is_contiguous() &&
              out->scalar_type() == opts.dtype().toScalarType() &&
              out->sizes() == sizes &&
              reinterpret_cast<uintptr_t>(out->data_ptr()) % 16 == 0,
              name, " must be a contiguous 16-byte aligned tensor of shape ",
              sizes);
  return *out;
}

void check_conv_args(const torch::Tensor& x, const torch::Tensor& w,
                     const c10::optional<torch::Tensor>& bias, int64_t D,
                     int64_t pad) {
  TORCH_CHECK(D % 8 == 0, "D must be divisible by 8");
  TORCH_CHECK(is_bf16_cuda(w) && w.dim() == 2 && w.size(1) == D,
              "w must be contiguous bf16 [K,D]");
  const int64_t K = w.size(0);
  TORCH_CHECK(K >= 1 && K < MAXK, "kernel size < ", MAXK);
  TORCH_CHECK(pad >= 0 && pad < K, "pad must be in [0, K)");
  TORCH_CHECK(!bias.has_value() ||
              (is_bf16_cuda(*bias) && bias->dim() == 1 && bias->size(0) == D),
              "bias must be contiguous bf16 [D]");
}

// dw/db of conv(u, w) from dy and u; the tiled kernel also takes h in
// place of u and recomputes the GLU (glu, padm).
void launch_bwd_dw(bool tiled, bool glu, const torch::Tensor& dy,
                   const torch::Tensor& x, const unsigned short* padm,
                   torch::Tensor& dw, torch::Tensor& db, int B, int T, int D,
                   int K, int pad, hipStream_t stream) {
  TORCH_CHECK(tiled || !glu, "the naive weight gradient takes u, not h");
  auto opts = dw.options();
  long nchunks = ((long)B * T + DW_CHUNK - 1) / DW_CHUNK;
  int dblks = (D + DW_DBLK - 1) / DW_DBLK;
  int ngroups = tiled ? (int)dwconv_tiled_dw_groups(B, T, D)
                      : (int)std::min<long>(
                            std::max<long>(1, 1024 / dblks), nchunks);
  auto dw_part = torch::empty({(long)ngroups * K * D}, opts);
  auto db_part = torch::empty({(long)ngroups * D}, opts);
  if (tiled) {
    dwconv_tiled_dw(glu, bf16_ptr(dy), bf16_ptr(x), padm,
                    dw_part.data_ptr<float>(), db_part.data_ptr<float>(), B,
                    T, D, K, pad, ngroups, stream);
  } else {
    dim3 grid_w(dblks, ngroups);
    hipLaunchKernelGGL(dwconv_bwd_dw, grid_w, dim3(256), 0, stream,
                       bf16_ptr(dy), bf16_ptr(x), dw_part.data_ptr<float>(),
                       db_part.data_ptr<float>(), B, T, D, K, pad, ngroups);
  }
  const long kd = (long)K * D;
  hipLaunchKernelGGL(dwconv_bwd_dw_reduce,
                     dim3((int)std::min<long>((kd + D + 255) / 256, 1024)),
                     dim3(256), 0, stream, dw_part.data_ptr<float>(),
                     db_part.data_ptr<float>(), dw.data_ptr<float>(),
                     db.data_ptr<float>(), kd, D, ngroups);
}

}  // namespace

torch::Tensor dwconv1d_fwd(torch::Tensor x, torch::Tensor w,
                           c10::optional<torch::Tensor> bias, int64_t pad,
                           const std::string& route,
                           c10::optional<torch::Tensor> y_out) {
  TORCH_CHECK(is_bf16_cuda(x) && x.dim() == 3, "x must be bf16 [B,T,D]");
  const int B = x.size(0), T = x.size(1), D = x.size(2);
  check_conv_args(x, w, bias, D, pad);
  const int K = w.size(0);
  if (x.numel() == 0) return out_or_empty(y_out, x.sizes(), x.options(), "y_out");
  const bool tiled = pick_tiled(route, B, T, D, K);
  auto y = out_or_empty(y_out, x.sizes(), x.options(), "y_out");
  auto stream = at::cuda::getCurrentCUDAStream();
  if (tiled) {
    dwconv_tiled_fwd(bf16_ptr(x), bf16_ptr(w), opt_ptr(bias),
                     (unsigned short*)y.data_ptr(), B, T, D, K, (int)pad,
                     stream);
    return y;
  }
  // Measured: full K unroll (KT=32) of the per-thread loop raises register
  // pressure and costs ~50% (8.2 -> 12.5 ms/step at the bench shape), so
  // the naive route keeps the runtime-K form.
  long nvec = (long)B * T * (D / 8);
  auto fwd_kern = dwconv_fwd<0>;
  hipLaunchKernelGGL(fwd_kern, dim3(memory_bound_grid(nvec, 256)), dim3(256),
                     0, stream, bf16_ptr(x), bf16_ptr(w), opt_ptr(bias),
                     (unsigned short*)y.data_ptr(), B, T, D, K, (int)pad);
  return y;
}

std::vector<torch::Tensor> dwconv1d_bwd(
    torch::Tensor dy, torch::Tensor x, torch::Tensor w, int64_t pad,
    const std::string& route, c10::optional<torch::Tensor> dx_out,
    c10::optional<torch::Tensor> dw_out,
    c10::optional<torch::Tensor> db_out) {
  TORCH_CHECK(is_bf16_cuda(x) && x.dim() == 3, "x must be bf16 [B,T,D]");
  TORCH_CHECK(is_bf16_cuda(dy) && dy.sizes() == x.sizes(),
              "dy must be contiguous bf16 shaped like x");
  const int B = x.size(0), T = x.size(1), D = x.size(2);
  check_conv_args(x, w, c10::nullopt, D, pad);
  const int K = w.size(0);
  auto opts = x.options().dtype(torch::kFloat32);
  if (x.numel() == 0) {
    // Nothing to sum: empty dx, zero dw and db.
    auto dx = out_or_empty(dx_out, x.sizes(), x.options(), "dx_out");
    auto dw = out_or_empty(dw_out, {K, D}, opts, "dw_out");
    auto db = out_or_empty(db_out, {D}, opts, "db_out");
    return {dx, dw.zero_(), db.zero_()};
  }
  const bool tiled = pick_tiled(route, B, T, D, K);
  auto dx = out_or_empty(dx_out, x.sizes(), x.options(), "dx_out");
  auto dw = out_or_empty(dw_out, {K, D}, opts, "dw_out");
  auto db = out_or_empty(db_out, {D}, opts, "db_out");
  auto stream = at::cuda::getCurrentCUDAStream();
  if (tiled) {
    dwconv_tiled_dx(bf16_ptr(dy), bf16_ptr(w), (unsigned short*)dx.data_ptr(),
                    B, T, D, K, (int)pad, stream);
  } else {
    long nvec = (long)B * T * (D / 8);
    auto dx_kern = dwconv_bwd_dx<0>;
    hipLaunchKernelGGL(dx_kern, dim3(memory_bound_grid(nvec, 256)), dim3(256),
                       0, stream, bf16_ptr(dy), bf16_ptr(w),
                       (unsigned short*)dx.data_ptr(), B, T, D, K, (int)pad);
  }
  launch_bwd_dw(tiled, false, dy, x, nullptr, dw, db, B, T, D, K, (int)pad,
                stream);
  return {dx, dw, db};
}

namespace {

// Shared argument checks of the fused GLU front; returns {B, T, D, K}.
std::array<int, 4> check_glu_args(const torch::Tensor& h,
                                  const c10::optional<torch::Tensor>& paddings,
                                  const torch::Tensor& w,
                                  const c10::optional<torch::Tensor>& bias,
                                  int64_t pad) {
  TORCH_CHECK(h.is_cuda() && h.dim() == 3 &&
              h.scalar_type() == torch::kBFloat16, "h must be bf16 [B,T,2D]");
  TORCH_CHECK(h.is_contiguous(), "h must be contiguous");
  TORCH_CHECK(w.dim() == 2 && h.size(2) == 2 * w.size(1),
              "h.shape[-1] must be 2*D with w [K,D]");
  const int64_t D = w.size(1);
  check_conv_args(h, w, bias, D, pad);
  TORCH_CHECK(h.numel() > 0, "empty input");
  TORCH_CHECK(!paddings.has_value() ||
              (is_bf16_cuda(*paddings) && paddings->dim() == 2 &&
               paddings->size(0) == h.size(0) &&
               paddings->size(1) == h.size(1)),
              "paddings must be contiguous bf16 [B,T]");
  return {(int)h.size(0), (int)h.size(1), (int)D, (int)w.size(0)};
}

}  // namespace

// y = conv(mask * glu(h), w) + bias without writing glu(h) to memory.
torch::Tensor glu_dwconv1d_fwd(torch::Tensor h,
                               c10::optional<torch::Tensor> paddings,
                               torch::Tensor w,
                               c10::optional<torch::Tensor> bias, int64_t pad,
                               const std::string& route,
                               c10::optional<torch::Tensor> y_out) {
  const auto s = check_glu_args(h, paddings, w, bias, pad);
  const int B = s[0], T = s[1], D = s[2], K = s[3];
  TORCH_CHECK(route != "naive", "the fused front has no naive route");
  pick_tiled(route == "auto" ? "tiled" : route, B, T, D, K);
  auto y = out_or_empty(y_out, {B, T, D}, h.options(), "y_out");
  glu_dwconv_tiled_fwd(bf16_ptr(h), opt_ptr(paddings), bf16_ptr(w),
                       opt_ptr(bias), (unsigned short*)y.data_ptr(), B, T, D,
                       K, (int)pad, at::cuda::getCurrentCUDAStream());
  return y;
}

// Returns {dh [B,T,2D] bf16, dw [K,D], db [D], colsum(dh) [2D]} (fp32).
std::vector<torch::Tensor> glu_dwconv1d_bwd(
    torch::Tensor dy, torch::Tensor h, c10::optional<torch::Tensor> paddings,
    torch::Tensor w, int64_t pad, const std::string& route,
    c10::optional<torch::Tensor> dh_out, c10::optional<torch::Tensor> dw_out,
    c10::optional<torch::Tensor> db_out,
    c10::optional<torch::Tensor> dcol_out) {
  const auto s = check_glu_args(h, paddings, w, c10::nullopt, pad);
  const int B = s[0], T = s[1], D = s[2], K = s[3];
  TORCH_CHECK(is_bf16_cuda(dy) && dy.dim() == 3 && dy.size(0) == B &&
              dy.size(1) == T && dy.size(2) == D,
              "dy must be contiguous bf16 [B,T,D]");
  TORCH_CHECK(route != "naive", "the fused front has no naive route");
  pick_tiled(route == "auto" ? "tiled" : route, B, T, D, K);
  auto opts = h.options().dtype(torch::kFloat32);
  auto dh = out_or_empty(dh_out, {B, T, 2 * D}, h.options(), "dh_out");
  auto dw = out_or_empty(dw_out, {K, D}, opts, "dw_out");
  auto db = out_or_empty(db_out, {D}, opts, "db_out");
  auto dcol = out_or_empty(dcol_out, {2 * D}, opts, "dcol_out");
  const int groups = (int)dwconv_tiled_groups(B, T);
  auto cs_part = torch::empty({groups, 2 * D}, opts);
  auto stream = at::cuda::getCurrentCUDAStream();
  glu_dwconv_tiled_dx(bf16_ptr(dy), bf16_ptr(h), opt_ptr(paddings),
                      bf16_ptr(w), (unsigned short*)dh.data_ptr(),
                      cs_part.data_ptr<float>(), B, T, D, K, (int)pad, stream);
  colsum_reduce(cs_part.data_ptr<float>(), dcol.data_ptr<float>(), groups,
                2L * D, stream);
  launch_bwd_dw(true, true, dy, h, opt_ptr(paddings), dw, db, B, T, D, K,
                (int)pad, stream);
  return {dh, dw, db, dcol};
}
