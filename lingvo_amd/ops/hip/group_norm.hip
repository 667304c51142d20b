// Fused padded-aware GroupNorm fwd+bwd for gfx950
// (reference op: lingvo/core/bn_layers.py:747 GroupNormLayer).
//
// x: [B, T, D] bf16, G groups over the channel dim; moments are per
// (b, g) over (valid T) x (D/G); padded frames are excluded from the
// moments and zeroed in the output. y = xhat * (1+gamma) + beta.
//
// One block (256 threads) per (b, g): block-reduce moments, then a
// second pass normalizes. dgamma/dbeta accumulate via fp32 atomics
// (small: D columns).

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <string>

#include "common.h"

namespace {

constexpr int GN_BLOCK = 256;
constexpr int GN_WAVES = GN_BLOCK / WAVE_SIZE;

__global__ __launch_bounds__(GN_BLOCK) void gn_fwd_kernel(
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ paddings,  // [B,T] bf16 or null
    unsigned short* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int B, int T, int D, int G, float eps,
    int act) {
  __shared__ float scratch[GN_WAVES];
  const int b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int cg = D / G;
  const int tid = threadIdx.x;

  float sum = 0.f, sumsq = 0.f, count = 0.f;
  for (int i = tid; i < T * cg; i += GN_BLOCK) {
    int t = i / cg;
    int c = g * cg + i % cg;
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    if (pad < 0.5f) {
      float v = bf16_bits_to_float(x[((long)b * T + t) * D + c]);
      sum += v;
      sumsq += v * v;
      count += 1.f;
    }
  }
  sum = block_reduce_sum<GN_WAVES>(sum, scratch);
  sumsq = block_reduce_sum<GN_WAVES>(sumsq, scratch);
  count = block_reduce_sum<GN_WAVES>(count, scratch);
  count = fmaxf(count, 1.f);
  float mu = sum / count;
  float var = sumsq / count - mu * mu;
  float rstd = rsqrtf(var + eps);
  if (tid == 0) {
    mean_out[(long)b * G + g] = mu;
    rstd_out[(long)b * G + g] = rstd;
  }

  for (int i = tid; i < T * cg; i += GN_BLOCK) {
    int t = i / cg;
    int c = g * cg + i % cg;
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    float v = bf16_bits_to_float(x[((long)b * T + t) * D + c]);
    float w = 1.f + bf16_bits_to_float(gamma[c]);
    float bb = bf16_bits_to_float(beta[c]);
    float out = (v - mu) * rstd * w + bb;
    if (act == 1) out = out / (1.f + __expf(-out));  // fused SiLU
    out *= (1.f - pad);
    y[((long)b * T + t) * D + c] = float_to_bf16_bits(out);
  }
}

// Vectorized fwd for cg % 8 == 0, laid out like gn_bwd_vec_kernel: each
// thread owns one 8-channel octet and strides over rows, so all traffic
// is ushortx8, the padding is read once per row and there is no divide
// or modulo per element. Moments stay fp32; they differ from the scalar
// kernel only through summation order.
__global__ __launch_bounds__(GN_BLOCK) void gn_fwd_vec_kernel(
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ paddings,  // [B,T] bf16 or null
    unsigned short* __restrict__ y, float* __restrict__ mean_out,
    float* __restrict__ rstd_out, int B, int T, int D, int G, float eps,
    int act) {
  __shared__ float scratch[GN_WAVES];
  const int b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int cg = D / G;
  const int noct = cg / 8;
  const int tid = threadIdx.x;
  const int oct = tid % noct;
  const int rt = tid / noct;
  const int rstep = GN_BLOCK / noct;
  // Threads past the last whole row lane idle (noct need not divide 256).
  const int t_first = rt < rstep ? rt : T;
  const long col0 = (long)g * cg + (rt < rstep ? oct : 0) * 8;

  float sum = 0.f, sumsq = 0.f, count = 0.f;
  for (int t = t_first; t < T; t += rstep) {
    const float pad =
        paddings ? bf16_bits_to_float(paddings[(long)b * T + t]) : 0.f;
    if (pad >= 0.5f) continue;
    const ushortx8 xv = *reinterpret_cast<const ushortx8*>(
        x + ((long)b * T + t) * D + col0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float v = bf16_bits_to_float(xv[e]);
      sum += v;
      sumsq += v * v;
    }
    count += 8.f;
  }
  sum = block_reduce_sum<GN_WAVES>(sum, scratch);
  sumsq = block_reduce_sum<GN_WAVES>(sumsq, scratch);
  count = block_reduce_sum<GN_WAVES>(count, scratch);
  count = fmaxf(count, 1.f);
  const float mu = sum / count;
  const float var = sumsq / count - mu * mu;
  const float rstd = rsqrtf(var + eps);
  if (tid == 0) {
    mean_out[(long)b * G + g] = mu;
    rstd_out[(long)b * G + g] = rstd;
  }

  float w[8], bb[8];
  {
    const ushortx8 gv = *reinterpret_cast<const ushortx8*>(gamma + col0);
    const ushortx8 bv = *reinterpret_cast<const ushortx8*>(beta + col0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      w[e] = 1.f + bf16_bits_to_float(gv[e]);
      bb[e] = bf16_bits_to_float(bv[e]);
    }
  }
  for (int t = t_first; t < T; t += rstep) {
    const float pad =
        paddings ? bf16_bits_to_float(paddings[(long)b * T + t]) : 0.f;
    const long base = ((long)b * T + t) * D + col0;
    const ushortx8 xv = *reinterpret_cast<const ushortx8*>(x + base);
    ushortx8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float out = (bf16_bits_to_float(xv[e]) - mu) * rstd * w[e] + bb[e];
      if (act == 1) out = out / (1.f + __expf(-out));  // fused SiLU
      out *= (1.f - pad);
      o[e] = float_to_bf16_bits(out);
    }
    *reinterpret_cast<ushortx8*>(y + base) = o;
  }
}

__global__ __launch_bounds__(GN_BLOCK) void gn_bwd_kernel(
    const unsigned short* __restrict__ dy,
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ paddings,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    unsigned short* __restrict__ dx, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int B, int T, int D, int G, int act) {
  __shared__ float scratch[GN_WAVES];
  const int b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int cg = D / G;
  const int tid = threadIdx.x;
  const float mu = mean[(long)b * G + g];
  const float rs = rstd[(long)b * G + g];

  // Pass 1: reductions over the group: s1=sum(dyw), s2=sum(dyw*xhat),
  // count; and per-channel dgamma/dbeta partials via LDS.
  __shared__ float dg_s[64];  // cg <= 64 supported
  __shared__ float db_s[64];
  for (int i = tid; i < cg; i += GN_BLOCK) {
    dg_s[i] = 0.f;
    db_s[i] = 0.f;
  }
  __syncthreads();
  float s1 = 0.f, s2 = 0.f, count = 0.f;
  for (int i = tid; i < T * cg; i += GN_BLOCK) {
    int t = i / cg;
    int ci = i % cg;
    int c = g * cg + ci;
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    if (pad < 0.5f) {
      float xv = bf16_bits_to_float(x[((long)b * T + t) * D + c]);
      float dyv = bf16_bits_to_float(dy[((long)b * T + t) * D + c]);
      float w = 1.f + bf16_bits_to_float(gamma[c]);
      float xhat = (xv - mu) * rs;
      float dxhat = dyv * w;
      s1 += dxhat;
      s2 += dxhat * xhat;
      count += 1.f;
      atomicAdd(&dg_s[ci], dyv * xhat);
      atomicAdd(&db_s[ci], dyv);
    }
  }
  s1 = block_reduce_sum<GN_WAVES>(s1, scratch);
  s2 = block_reduce_sum<GN_WAVES>(s2, scratch);
  count = block_reduce_sum<GN_WAVES>(count, scratch);
  count = fmaxf(count, 1.f);
  const float inv_n = 1.f / count;

  for (int i = tid; i < cg; i += GN_BLOCK) {
    int c = g * cg + i;
    if (dg_s[i] != 0.f) atomicAdd(dgamma + c, dg_s[i]);
    if (db_s[i] != 0.f) atomicAdd(dbeta + c, db_s[i]);
  }

  for (int i = tid; i < T * cg; i += GN_BLOCK) {
    int t = i / cg;
    int c = g * cg + i % cg;
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    float xv = bf16_bits_to_float(x[((long)b * T + t) * D + c]);
    float dyv = bf16_bits_to_float(dy[((long)b * T + t) * D + c]);
    float w = 1.f + bf16_bits_to_float(gamma[c]);
    float xhat = (xv - mu) * rs;
    float dxhat = dyv * w;
    float val = rs * (dxhat - inv_n * (s1 + xhat * s2)) * (1.f - pad);
    dx[((long)b * T + t) * D + c] = float_to_bf16_bits(val);
  }
}

// Vectorized bwd for cg % 8 == 0 (the production config: D=512, G=32,
// cg=16). Each thread owns one 8-channel octet and strides over rows:
// all x/dy traffic is ushortx8, and dgamma/dbeta partials accumulate
// in REGISTERS (the scalar kernel above pays two LDS atomics per
// element in its hot loop, which dominates its runtime).
// act == 1: the forward emitted silu(y_pre); incoming dy is w.r.t.
// silu's output, so fold silu'(y_pre) in (y_pre recomputed from the
// saved moments + beta — nothing extra stored).
__global__ __launch_bounds__(GN_BLOCK) void gn_bwd_vec_kernel(
    const unsigned short* __restrict__ dy,
    const unsigned short* __restrict__ x,
    const unsigned short* __restrict__ gamma,
    const unsigned short* __restrict__ beta,
    const unsigned short* __restrict__ paddings,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    unsigned short* __restrict__ dx, float* __restrict__ dgamma,
    float* __restrict__ dbeta, int B, int T, int D, int G, int act) {
  __shared__ float scratch[GN_WAVES];
  __shared__ float dg_s[64];
  __shared__ float db_s[64];
  const int b = blockIdx.x / G;
  const int g = blockIdx.x % G;
  const int cg = D / G;
  const int noct = cg / 8;
  const int tid = threadIdx.x;
  const int oct = tid % noct;
  const int rt = tid / noct;
  const int rstep = GN_BLOCK / noct;
  const float mu = mean[(long)b * G + g];
  const float rs = rstd[(long)b * G + g];
  const long col0 = (long)g * cg + oct * 8;

  float w[8], bb[8];
  {
    ushortx8 gv = *reinterpret_cast<const ushortx8*>(gamma + col0);
    ushortx8 bv = *reinterpret_cast<const ushortx8*>(beta + col0);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      w[e] = 1.f + bf16_bits_to_float(gv[e]);
      bb[e] = bf16_bits_to_float(bv[e]);
    }
  }
  for (int i = tid; i < cg; i += GN_BLOCK) {
    dg_s[i] = 0.f;
    db_s[i] = 0.f;
  }

  float s1 = 0.f, s2 = 0.f, count = 0.f;
  float dg8[8], db8[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    dg8[e] = 0.f;
    db8[e] = 0.f;
  }
  for (int t = rt; t < T; t += rstep) {
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    if (pad >= 0.5f) continue;
    const long base = ((long)b * T + t) * D + col0;
    ushortx8 xv = *reinterpret_cast<const ushortx8*>(x + base);
    ushortx8 dyv = *reinterpret_cast<const ushortx8*>(dy + base);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float xf = bf16_bits_to_float(xv[e]);
      float df = bf16_bits_to_float(dyv[e]);
      float xhat = (xf - mu) * rs;
      if (act == 1) {
        const float ypre = xhat * w[e] + bb[e];
        const float sg = 1.f / (1.f + __expf(-ypre));
        df *= sg * (1.f + ypre * (1.f - sg));
      }
      float dxhat = df * w[e];
      s1 += dxhat;
      s2 += dxhat * xhat;
      dg8[e] += df * xhat;
      db8[e] += df;
    }
    count += 8.f;
  }
  __syncthreads();  // dg_s/db_s zero-init visible
  s1 = block_reduce_sum<GN_WAVES>(s1, scratch);
  s2 = block_reduce_sum<GN_WAVES>(s2, scratch);
  count = block_reduce_sum<GN_WAVES>(count, scratch);
  count = fmaxf(count, 1.f);
  const float inv_n = 1.f / count;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if (dg8[e] != 0.f) atomicAdd(&dg_s[oct * 8 + e], dg8[e]);
    if (db8[e] != 0.f) atomicAdd(&db_s[oct * 8 + e], db8[e]);
  }
  __syncthreads();
  for (int i = tid; i < cg; i += GN_BLOCK) {
    int c = g * cg + i;
    if (dg_s[i] != 0.f) atomicAdd(dgamma + c, dg_s[i]);
    if (db_s[i] != 0.f) atomicAdd(dbeta + c, db_s[i]);
  }

  for (int t = rt; t < T; t += rstep) {
    float pad = paddings ? bf16_bits_to_float(paddings[(long)b * T + t])
                         : 0.f;
    const long base = ((long)b * T + t) * D + col0;
    ushortx8 xv = *reinterpret_cast<const ushortx8*>(x + base);
    ushortx8 dyv = *reinterpret_cast<const ushortx8*>(dy + base);
    ushortx8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float xf = bf16_bits_to_float(xv[e]);
      float df = bf16_bits_to_float(dyv[e]);
      float xhat = (xf - mu) * rs;
      if (act == 1) {
        const float ypre = xhat * w[e] + bb[e];
        const float sg = 1.f / (1.f + __expf(-ypre));
        df *= sg * (1.f + ypre * (1.f - sg));
      }
      float dxhat = df * w[e];
      float val = rs * (dxhat - inv_n * (s1 + xhat * s2)) * (1.f - pad);
      o[e] = float_to_bf16_bits(val);
    }
    *reinterpret_cast<ushortx8*>(dx + base) = o;
  }
}

}  // namespace

std::vector<torch::Tensor> group_norm_fwd(torch::Tensor x,
                                          torch::Tensor gamma,
                                          torch::Tensor beta,
                                          c10::optional<torch::Tensor> pad,
                                          int64_t groups, double eps,
                                          int64_t act,
                                          const std::string& route) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 3 &&
              x.scalar_type() == torch::kBFloat16);
  const int B = x.size(0), T = x.size(1), D = x.size(2);
  const int G = (int)groups;
  TORCH_CHECK(D % G == 0 && D / G <= 64, "cg must be <= 64");
  // 'auto' takes the vector kernel for cg % 8 == 0; 'scalar' forces the
  // per-element kernel (the tests' yardstick).
  TORCH_CHECK(route == "auto" || route == "scalar" || route == "vec",
              "route must be 'auto', 'scalar' or 'vec'");
  const bool can_vec = (D / G) % 8 == 0;
  TORCH_CHECK(route != "vec" || can_vec, "route='vec' needs cg % 8 == 0");
  const bool vec = can_vec && route != "scalar";
  auto y = torch::empty_like(x);
  auto opts = x.options().dtype(torch::kFloat32);
  auto mean = torch::empty({(long)B * G}, opts);
  auto rstd = torch::empty({(long)B * G}, opts);
  auto stream = at::cuda::getCurrentCUDAStream();
  TORCH_CHECK(act == 0 || (D / G) % 8 == 0,
              "fused activation needs cg % 8 == 0");
  hipLaunchKernelGGL(vec ? gn_fwd_vec_kernel : gn_fwd_kernel, dim3(B * G),
                     dim3(GN_BLOCK), 0, stream,
                     (const unsigned short*)x.data_ptr(),
                     (const unsigned short*)gamma.data_ptr(),
                     (const unsigned short*)beta.data_ptr(),
                     pad.has_value()
                         ? (const unsigned short*)pad->data_ptr()
                         : nullptr,
                     (unsigned short*)y.data_ptr(), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(), B, T, D, G, (float)eps,
                     (int)act);
  return {y, mean, rstd};
}

std::vector<torch::Tensor> group_norm_bwd(torch::Tensor dy, torch::Tensor x,
                                          torch::Tensor gamma,
                                          torch::Tensor beta,
                                          c10::optional<torch::Tensor> pad,
                                          torch::Tensor mean,
                                          torch::Tensor rstd,
                                          int64_t groups, int64_t act) {
  const int B = x.size(0), T = x.size(1), D = x.size(2);
  const int G = (int)groups;
  auto dx = torch::empty_like(x);
  auto opts = x.options().dtype(torch::kFloat32);
  auto dgamma = torch::zeros({D}, opts);
  auto dbeta = torch::zeros({D}, opts);
  auto stream = at::cuda::getCurrentCUDAStream();
  const int cg = D / G;
  const bool vec = cg % 8 == 0 && GN_BLOCK % (cg / 8) == 0;
  TORCH_CHECK(act == 0 || vec, "fused activation needs cg % 8 == 0");
  auto kern = vec ? gn_bwd_vec_kernel : gn_bwd_kernel;
  hipLaunchKernelGGL(kern, dim3(B * G), dim3(GN_BLOCK), 0, stream,
                     (const unsigned short*)dy.data_ptr(),
                     (const unsigned short*)x.data_ptr(),
                     (const unsigned short*)gamma.data_ptr(),
                     (const unsigned short*)beta.data_ptr(),
                     pad.has_value()
                         ? (const unsigned short*)pad->data_ptr()
                         : nullptr,
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),
                     (unsigned short*)dx.data_ptr(),
                     dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), B,
                     T, D, G, (int)act);
  return {dx, dgamma, dbeta};
}
