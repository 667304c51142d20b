// Fused deterministic dropout (+ optional residual add) for gfx950.
// Replaces the reference's DeterministicDropout (py_utils.py:3978): the
// mask is a pure function of (seed, element index), so backward
// recomputes it from the saved seed — no mask tensor is stored and
// fwd/bwd are one kernel each instead of rand+cmp+mul chains.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include "common.h"

namespace {

// Stateless hash RNG (xxhash-style avalanche): adequate for dropout.
__device__ __forceinline__ unsigned int hash_u32(unsigned long long seed,
                                                 unsigned long long idx) {
  unsigned long long h = seed ^ (idx * 0x9E3779B97F4A7C15ull);
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  return (unsigned int)h;
}

// ACT: 0 = identity, 1 = SiLU/Swish, 2 = ReLU — applied BEFORE the
// dropout mask, fusing the FFN activation pass into this kernel.
template <int ACT>
__device__ __forceinline__ float apply_act(float v) {
  if (ACT == 1) return v / (1.f + __expf(-v)) ;
  if (ACT == 2) return v > 0.f ? v : 0.f;
  return v;
}

template <int ACT>
__device__ __forceinline__ float act_grad(float v) {
  if (ACT == 1) {
    const float s = 1.f / (1.f + __expf(-v));
    return s * (1.f + v * (1.f - s));
  }
  if (ACT == 2) return v > 0.f ? 1.f : 0.f;
  return 1.f;
}

// scale folds a residual weight (e.g. the conformer's 0.5 half-FFN)
// and pad ([B*T] bf16, 1.0 == padded; row = element/D) folds the
// ApplyPadding mask into the same pass.
template <bool RESIDUAL, int ACT>
__global__ void dropout_fwd_kernel(const unsigned short* __restrict__ x,
                                   const unsigned short* __restrict__ res,
                                   unsigned short* __restrict__ y,
                                   long nvec, unsigned long long seed,
                                   const long* __restrict__ step_seed,
                                   float keep, float inv_keep,
                                   float scale,
                                   const unsigned short* __restrict__ pad,
                                   long dvec) {
  const unsigned int thresh = (unsigned int)(keep * 4294967296.0);
  if (step_seed) seed ^= (unsigned long long)(*step_seed);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long)gridDim.x * blockDim.x) {
    float sc = scale;
    if (pad) sc *= 1.f - bf16_bits_to_float(pad[i / dvec]);
    ushortx8 v = *reinterpret_cast<const ushortx8*>(x + i * 8);
    ushortx8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      bool kept = hash_u32(seed, i * 8 + e) < thresh;
      float f = kept ? apply_act<ACT>(bf16_bits_to_float(v[e])) * inv_keep
                           * sc
                     : 0.f;
      o[e] = float_to_bf16_bits(f);
    }
    if (RESIDUAL) {
      ushortx8 r = *reinterpret_cast<const ushortx8*>(res + i * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e)
        o[e] = float_to_bf16_bits(bf16_bits_to_float(o[e]) +
                                  bf16_bits_to_float(r[e]));
    }
    *reinterpret_cast<ushortx8*>(y + i * 8) = o;
  }
}

// One 8-wide vector of the backward: flat vector index i, row scale sc.
// Shared by the flat kernel and the column-sum kernel so both store the
// same bits.
template <int ACT>
__device__ __forceinline__ ushortx8 dropout_bwd_vec(
    const unsigned short* __restrict__ dy, const unsigned short* __restrict__ x,
    long i, unsigned long long seed, unsigned int thresh, float inv_keep,
    float sc) {
  ushortx8 v = *reinterpret_cast<const ushortx8*>(dy + i * 8);
  ushortx8 xv;
  if (ACT != 0) xv = *reinterpret_cast<const ushortx8*>(x + i * 8);
  ushortx8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    bool kept = hash_u32(seed, i * 8 + e) < thresh;
    float f = kept ? bf16_bits_to_float(v[e]) * inv_keep * sc : 0.f;
    if (ACT != 0) f *= act_grad<ACT>(bf16_bits_to_float(xv[e]));
    o[e] = float_to_bf16_bits(f);
  }
  return o;
}

template <int ACT>
__global__ void dropout_bwd_kernel(const unsigned short* __restrict__ dy,
                                   const unsigned short* __restrict__ x,
                                   unsigned short* __restrict__ dx,
                                   long nvec, unsigned long long seed,
                                   const long* __restrict__ step_seed,
                                   float keep, float inv_keep,
                                   float scale,
                                   const unsigned short* __restrict__ pad,
                                   long dvec) {
  const unsigned int thresh = (unsigned int)(keep * 4294967296.0);
  if (step_seed) seed ^= (unsigned long long)(*step_seed);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long)gridDim.x * blockDim.x) {
    float sc = scale;
    if (pad) sc *= 1.f - bf16_bits_to_float(pad[i / dvec]);
    *reinterpret_cast<ushortx8*>(dx + i * 8) =
        dropout_bwd_vec<ACT>(dy, x, i, seed, thresh, inv_keep, sc);
  }
}

// ---- backward + column sums of dx (the bias gradient of the linear that
// produced x) ---------------------------------------------------------------
// Row/column mapping: a block is 4 waves; lane l of every wave owns column
// vector blockIdx.x*64 + l (8 columns) and wave w walks rows
// r0+w, r0+w+4, ... of the block's row slab, so the pad index is the row
// (no division) and the 8 fp32 column accumulators stay in registers.
// The four waves are summed in fixed order through LDS into
// partials[blockIdx.y, D]; colsum_reduce_kernel then sums the slabs in
// fixed order. No atomics: two runs give the same bits.
constexpr int kColsumWaves = 4;
constexpr int kColsumCols = WAVE_SIZE * 8;  // columns per block

template <int ACT>
__global__ __launch_bounds__(WAVE_SIZE * kColsumWaves)
void dropout_bwd_colsum_kernel(const unsigned short* __restrict__ dy,
                               const unsigned short* __restrict__ x,
                               unsigned short* __restrict__ dx,
                               float* __restrict__ partials, long rows,
                               long dvec, long rows_per_block,
                               unsigned long long seed,
                               const long* __restrict__ step_seed, float keep,
                               float inv_keep, float scale,
                               const unsigned short* __restrict__ pad) {
  __shared__ float red[kColsumWaves][kColsumCols];
  const unsigned int thresh = (unsigned int)(keep * 4294967296.0);
  if (step_seed) seed ^= (unsigned long long)(*step_seed);
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  const int wave = threadIdx.x / WAVE_SIZE;
  const long cv = (long)blockIdx.x * WAVE_SIZE + lane;
  const long r0 = (long)blockIdx.y * rows_per_block;
  const long r1 = min(rows, r0 + rows_per_block);
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (cv < dvec) {
    for (long r = r0 + wave; r < r1; r += kColsumWaves) {
      const long i = r * dvec + cv;
      float sc = scale;
      if (pad) sc *= 1.f - bf16_bits_to_float(pad[r]);
      ushortx8 o = dropout_bwd_vec<ACT>(dy, x, i, seed, thresh, inv_keep, sc);
      *reinterpret_cast<ushortx8*>(dx + i * 8) = o;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += bf16_bits_to_float(o[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[wave][lane * 8 + e] = acc[e];
  __syncthreads();
  const long D = dvec * 8;
  for (int c = threadIdx.x; c < kColsumCols; c += blockDim.x) {
    const long col = (long)blockIdx.x * kColsumCols + c;
    if (col < D) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < kColsumWaves; ++w) s += red[w][c];
      partials[(long)blockIdx.y * D + col] = s;
    }
  }
}

// partials [nslab, D] -> out [D]. A block is 64 slices x 4 column quads:
// slice s sums slabs s, s+64, ... (float4 per slab), then the 64 slices are
// summed in order through LDS.
__global__ __launch_bounds__(256)
void colsum_reduce_kernel(const float* __restrict__ partials,
                          float* __restrict__ out, int nslab, long D) {
  __shared__ float red[64][16];
  const int q = threadIdx.x & 3;
  const int slice = threadIdx.x >> 2;
  const long col = (long)blockIdx.x * 16 + q * 4;
  floatx4 s = {0.f, 0.f, 0.f, 0.f};
  if (col < D) {
    for (int p = slice; p < nslab; p += 64)
      s += *reinterpret_cast<const floatx4*>(partials + (long)p * D + col);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) red[slice][q * 4 + j] = s[j];
  __syncthreads();
  if (threadIdx.x < 16) {
    const long c = (long)blockIdx.x * 16 + threadIdx.x;
    if (c < D) {
      float t = 0.f;
      for (int p = 0; p < 64; ++p) t += red[p][threadIdx.x];
      out[c] = t;
    }
  }
}

}  // namespace

void colsum_reduce(const float* partials, float* out, int nslab, long D,
                   hipStream_t stream) {
  hipLaunchKernelGGL(colsum_reduce_kernel, dim3(cdiv(D, 16)), dim3(256), 0,
                     stream, partials, out, nslab, D);
}

torch::Tensor dropout_fwd(torch::Tensor x, c10::optional<torch::Tensor> res,
                          int64_t seed, c10::optional<torch::Tensor> step_seed,
                          double keep, int64_t act, double scale,
                          c10::optional<torch::Tensor> pad, int64_t d) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
              x.scalar_type() == torch::kBFloat16 && x.numel() % 8 == 0);
  TORCH_CHECK(!(res.has_value() && act != 0),
              "residual+activation fusion unsupported");
  TORCH_CHECK(!pad.has_value() || (d > 0 && d % 8 == 0),
              "padding fusion needs D % 8 == 0");
  auto y = torch::empty_like(x);
  long nvec = x.numel() / 8;
  auto stream = at::cuda::getCurrentCUDAStream();
  const long* ssp = step_seed.has_value() ?
      step_seed->data_ptr<long>() : nullptr;
  const unsigned short* pp = pad.has_value() ?
      (const unsigned short*)pad->data_ptr() : nullptr;
  const long dvec = d > 0 ? d / 8 : 1;
#define LAUNCH_FWD(RES, ACT, RESPTR)                                         \
  hipLaunchKernelGGL((dropout_fwd_kernel<RES, ACT>),                         \
                     dim3(memory_bound_grid(nvec, 256)), dim3(256), 0,       \
                     stream, (const unsigned short*)x.data_ptr(), RESPTR,    \
                     (unsigned short*)y.data_ptr(), nvec,                    \
                     (unsigned long long)seed, ssp, (float)keep,             \
                     (float)(1.0 / keep), (float)scale, pp, dvec)
  if (res.has_value()) {
    LAUNCH_FWD(true, 0, (const unsigned short*)res->data_ptr());
  } else if (act == 1) {
    LAUNCH_FWD(false, 1, nullptr);
  } else if (act == 2) {
    LAUNCH_FWD(false, 2, nullptr);
  } else {
    LAUNCH_FWD(false, 0, nullptr);
  }
#undef LAUNCH_FWD
  return y;
}

torch::Tensor dropout_bwd(torch::Tensor dy, c10::optional<torch::Tensor> x,
                          int64_t seed, c10::optional<torch::Tensor> step_seed,
                          double keep, int64_t act, double scale,
                          c10::optional<torch::Tensor> pad, int64_t d) {
  TORCH_CHECK(act == 0 || x.has_value(),
              "activation-fused dropout bwd needs the pre-activation input");
  auto dx = torch::empty_like(dy);
  long nvec = dy.numel() / 8;
  auto stream = at::cuda::getCurrentCUDAStream();
  const long* ssp = step_seed.has_value() ?
      step_seed->data_ptr<long>() : nullptr;
  const unsigned short* xp = x.has_value() ?
      (const unsigned short*)x->data_ptr() : nullptr;
  const unsigned short* pp = pad.has_value() ?
      (const unsigned short*)pad->data_ptr() : nullptr;
  const long dvec = d > 0 ? d / 8 : 1;
#define LAUNCH_BWD(ACT)                                                      \
  hipLaunchKernelGGL((dropout_bwd_kernel<ACT>),                              \
                     dim3(memory_bound_grid(nvec, 256)), dim3(256), 0,       \
                     stream, (const unsigned short*)dy.data_ptr(), xp,       \
                     (unsigned short*)dx.data_ptr(), nvec,                   \
                     (unsigned long long)seed, ssp, (float)keep,             \
                     (float)(1.0 / keep), (float)scale, pp, dvec)
  if (act == 1) {
    LAUNCH_BWD(1);
  } else if (act == 2) {
    LAUNCH_BWD(2);
  } else {
    LAUNCH_BWD(0);
  }
#undef LAUNCH_BWD
  return dx;
}

// dropout_bwd that also returns the fp32 column sums [d] of the dx it
// stores (summed after bf16 rounding, i.e. dx.sum(0) in fp32). dx is
// bit-identical to dropout_bwd on the same inputs.
std::vector<torch::Tensor> dropout_bwd_colsum(
    torch::Tensor dy, c10::optional<torch::Tensor> x, int64_t seed,
    c10::optional<torch::Tensor> step_seed, double keep, int64_t act,
    double scale, c10::optional<torch::Tensor> pad, int64_t d) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() &&
              dy.scalar_type() == torch::kBFloat16,
              "dy must be contiguous CUDA bf16");
  TORCH_CHECK(d > 0 && d % 8 == 0 && dy.numel() % d == 0,
              "column sums need D % 8 == 0 and numel % D == 0");
  TORCH_CHECK(act == 0 || x.has_value(),
              "activation-fused dropout bwd needs the pre-activation input");
  const long rows = dy.numel() / d;
  TORCH_CHECK(!x.has_value() ||
              (x->is_cuda() && x->is_contiguous() &&
               x->scalar_type() == torch::kBFloat16 &&
               x->numel() == dy.numel()), "x must match dy");
  TORCH_CHECK(!pad.has_value() ||
              (pad->is_cuda() && pad->is_contiguous() &&
               pad->scalar_type() == torch::kBFloat16 &&
               pad->numel() == rows), "pad must be [rows] bf16");
  auto dx = torch::empty_like(dy);
  auto fopts = dy.options().dtype(torch::kFloat32);
  auto colsum = torch::empty({d}, fopts);
  if (rows == 0) {
    colsum.zero_();
    return {dx, colsum};
  }
  const long dvec = d / 8;
  const int gx = cdiv(dvec, WAVE_SIZE);
  // ~2048 blocks in all; slabs are whole multiples of the 4 waves.
  const long want_y = std::max<long>(1, 2048 / gx);
  long rpb = (rows + want_y - 1) / want_y;
  rpb = (rpb + kColsumWaves - 1) / kColsumWaves * kColsumWaves;
  const int gy = cdiv(rows, rpb);
  auto partials = torch::empty({(long)gy, (long)d}, fopts);
  auto stream = at::cuda::getCurrentCUDAStream();
  const long* ssp = step_seed.has_value() ?
      step_seed->data_ptr<long>() : nullptr;
  const unsigned short* xp = x.has_value() ?
      (const unsigned short*)x->data_ptr() : nullptr;
  const unsigned short* pp = pad.has_value() ?
      (const unsigned short*)pad->data_ptr() : nullptr;
#define LAUNCH_BWD_CS(ACT)                                                   \
  hipLaunchKernelGGL((dropout_bwd_colsum_kernel<ACT>), dim3(gx, gy),         \
                     dim3(WAVE_SIZE * kColsumWaves), 0, stream,              \
                     (const unsigned short*)dy.data_ptr(), xp,               \
                     (unsigned short*)dx.data_ptr(),                         \
                     partials.data_ptr<float>(), rows, dvec, rpb,            \
                     (unsigned long long)seed, ssp, (float)keep,             \
                     (float)(1.0 / keep), (float)scale, pp)
  if (act == 1) {
    LAUNCH_BWD_CS(1);
  } else if (act == 2) {
    LAUNCH_BWD_CS(2);
  } else {
    LAUNCH_BWD_CS(0);
  }
#undef LAUNCH_BWD_CS
  colsum_reduce(partials.data_ptr<float>(), colsum.data_ptr<float>(), gy,
                (long)d, stream);
  return {dx, colsum};
}
