// Space-to-depth transforms for the stride-2 conv frontend (gfx950).
//
// The conv-subsampling 3x3/s2 conv runs as 4 flat GEMMs over a
// space-to-depth'd, zero-padded buffer X [B*(Ho+1)*(Wo+1), 4C] (see
// layers/conformer.py _Conv3x3S2Nhwc). Composing that buffer from
// torch strided-slice copies costs 4 badly-coalesced passes per
// direction (~0.86 ms each at the bench shape); these kernels do each
// transform in ONE output-coalesced pass with ushortx8 vectors.
//
// Block order: s0=(0,1), s1=(1,1), s2=(1,0), s3=(0,0) in (a,b) cell
// coordinates — a = row parity, b = col parity.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include "common.h"

namespace {

// (a, b) for block index s.
__constant__ const int kBlkA[4] = {0, 1, 1, 0};
__constant__ const int kBlkB[4] = {1, 1, 0, 0};

// x [B, 2Ho, 2Wo, C] -> X [B, Ho+1, Wo+1, 4C]; row 0 / col 0 zero.
__global__ void s2d_fwd_kernel(const unsigned short* __restrict__ x,
                               unsigned short* __restrict__ out, long B,
                               long Ho, long Wo, long C) {
  const long Hp = Ho + 1, Wp = Wo + 1;
  const long cvec = C / 8;
  const long nvec = B * Hp * Wp * 4 * cvec;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long)gridDim.x * blockDim.x) {
    long t = i;
    const long c8 = t % cvec;
    t /= cvec;
    const int s = (int)(t % 4);
    t /= 4;
    const long wp = t % Wp;
    t /= Wp;
    const long hp = t % Hp;
    const long b = t / Hp;
    ushortx8 v;
    if (hp == 0 || wp == 0) {
      for (int e = 0; e < 8; ++e) v[e] = 0;
    } else {
      const long h = 2 * (hp - 1) + kBlkA[s];
      const long w = 2 * (wp - 1) + kBlkB[s];
      v = *reinterpret_cast<const ushortx8*>(
          x + ((b * (2 * Ho) + h) * (2 * Wo) + w) * C + c8 * 8);
    }
    *reinterpret_cast<ushortx8*>(out + i * 8) = v;
  }
}

// dX [B, Ho+1, Wo+1, 4C] -> dx [B, 2Ho, 2Wo, C] (inverse s2d; padded
// row/col dropped).
__global__ void s2d_inv_kernel(const unsigned short* __restrict__ dX,
                               unsigned short* __restrict__ dx, long B,
                               long Ho, long Wo, long C) {
  const long Hp = Ho + 1, Wp = Wo + 1;
  const long cvec = C / 8;
  const long nvec = B * (2 * Ho) * (2 * Wo) * cvec;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long)gridDim.x * blockDim.x) {
    long t = i;
    const long c8 = t % cvec;
    t /= cvec;
    const long w = t % (2 * Wo);
    t /= (2 * Wo);
    const long h = t % (2 * Ho);
    const long b = t / (2 * Ho);
    const int a = (int)(h & 1), bb = (int)(w & 1);
    // block for (a, b): s0=(0,1) s1=(1,1) s2=(1,0) s3=(0,0)
    const int s = a ? (bb ? 1 : 2) : (bb ? 0 : 3);
    const long src = (((b * Hp + h / 2 + 1) * Wp + w / 2 + 1) * 4 + s) *
                         C + c8 * 8;
    *reinterpret_cast<ushortx8*>(dx + i * 8) =
        *reinterpret_cast<const ushortx8*>(dX + src);
  }
}

// dout [B, Ho, Wo, Co] -> dO [B, Ho+1, Wo+1, Co] with zero border.
__global__ void pad_scatter_kernel(const unsigned short* __restrict__ src,
                                   unsigned short* __restrict__ out,
                                   long B, long Ho, long Wo, long Co) {
  const long Hp = Ho + 1, Wp = Wo + 1;
  const long cvec = Co / 8;
  const long nvec = B * Hp * Wp * cvec;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long)gridDim.x * blockDim.x) {
    long t = i;
    const long c8 = t % cvec;
    t /= cvec;
    const long wp = t % Wp;
    t /= Wp;
    const long hp = t % Hp;
    const long b = t / Hp;
    ushortx8 v;
    if (hp == 0 || wp == 0) {
      for (int e = 0; e < 8; ++e) v[e] = 0;
    } else {
      v = *reinterpret_cast<const ushortx8*>(
          src + ((b * Ho + hp - 1) * Wo + wp - 1) * Co + c8 * 8);
    }
    *reinterpret_cast<ushortx8*>(out + i * 8) = v;
  }
}

// ---- fused conv frontend ---------------------------------------------------
//
// The kernels below keep one channel octet per thread for the thread's whole
// life. A workgroup of kOctThreads threads is kOctThreads / cvec "slots" of
// cvec threads; slot q of workgroup g walks rows g*slots + q, then
// + gridDim.x*slots, ... Threads past slots*cvec idle (cvec need not divide
// the workgroup). Offsets into X, dX and the batch are 64-bit; row counts
// and offsets inside one utterance are 32-bit under the host contracts.
constexpr int kOctThreads = 256;

// Sums the 8 values of every thread over the slots of the workgroup in slot
// order and writes them to dst[c8*8 .. c8*8+8) (slot 0's threads store).
// red is [kOctThreads][8]. Every thread of the workgroup must call it.
__device__ __forceinline__ void slot_reduce_store(const float (&v)[8],
                                                  float (*red)[8], int slots,
                                                  int cvec, bool active,
                                                  float* __restrict__ dst) {
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 8; ++e) red[threadIdx.x][e] = v[e];
  __syncthreads();
  if (active && (int)threadIdx.x < cvec) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float s = 0.f;
      for (int q = 0; q < slots; ++q) s += red[q * cvec + threadIdx.x][e];
      dst[(long)threadIdx.x * 8 + e] = s;
    }
  }
}

// The input rows under s2d row hp of an utterance: rows 4(hp-1)-1 ..
// 4(hp-1)+3 of xb [T,F]. Rows outside [0,T) point at row 0 with ok = false.
struct PatchRows {
  const unsigned short* row[5];
  bool ok[5];
};

__device__ __forceinline__ PatchRows patch_rows(
    const unsigned short* __restrict__ xb, int hp, int T, int F) {
  PatchRows pr;
  const int r0 = 4 * (hp - 1) - 1;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    pr.ok[r] = r0 + r >= 0 && r0 + r < T;
    pr.row[r] = xb + (pr.ok[r] ? (r0 + r) * F : 0);
  }
  return pr;
}

// The 5x5 patch under s2d cell (hp, wp): columns 4(wp-1)-1 .. 4(wp-1)+3 of
// the rows above, zero outside [0,T) x [0,F). Output position (a, b) of the
// cell reads patch rows 2a+dt, columns 2b+df. T*F < 2^31 (host contract),
// so offsets inside an utterance are 32-bit.
__device__ __forceinline__ void load_patch(const PatchRows& pr, int wp, int F,
                                           float (&p)[5][5]) {
  const int c0 = 4 * (wp - 1) - 1;
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    const bool cin = c0 + c >= 0 && c0 + c < F;
    const int col = cin ? c0 + c : 0;
#pragma unroll
    for (int r = 0; r < 5; ++r)
      p[r][c] = (cin && pr.ok[r]) ? bf16_bits_to_float(pr.row[r][col]) : 0.f;
  }
}

// x [B,T,F], w1 [9,C], b1 [C] -> X [B, Ho+1, Wo+1, 4C]:
//   X[b,hp,wp,s*C+c] = relu(b1[c] + sum_k tap_k * w1[k,c]), one rounding;
// zero where hp == 0, wp == 0 or the conv1 position lies past (t1, h1).
// A slot walks whole s2d rows (b, hp), so the index arithmetic of a row is
// done once and the cells of the row follow at a fixed stride.
__global__ __launch_bounds__(kOctThreads)
void conv1_s2d_fwd_kernel(const unsigned short* __restrict__ x,
                          const unsigned short* __restrict__ w1,
                          const unsigned short* __restrict__ b1,
                          unsigned short* __restrict__ X, int B, int T, int F,
                          int t1, int h1, int Hp, int Wp, int C) {
  const int cvec = C / 8;
  const int slots = kOctThreads / cvec;
  const int slot = threadIdx.x / cvec;
  const int c8 = threadIdx.x - slot * cvec;
  if (slot >= slots) return;
  float w[9][8], bias[8];
  {
    const ushortx8 bv = *reinterpret_cast<const ushortx8*>(b1 + c8 * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) bias[e] = bf16_bits_to_float(bv[e]);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const ushortx8 wv =
          *reinterpret_cast<const ushortx8*>(w1 + (long)k * C + c8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) w[k][e] = bf16_bits_to_float(wv[e]);
    }
  }
  const int nrow = B * Hp;  // < 2^31 (host contract)
  for (int row = blockIdx.x * slots + slot; row < nrow;
       row += gridDim.x * slots) {
    const int b = row / Hp;
    const int hp = row - b * Hp;
    unsigned short* out = X + (long)row * Wp * 4 * C + c8 * 8;
    const PatchRows pr = patch_rows(x + (long)b * T * F, hp, T, F);
    for (int wp = 0; wp < Wp; ++wp, out += 4 * C) {
      const bool border = hp == 0 || wp == 0;
      float p[5][5];
      if (!border) load_patch(pr, wp, F, p);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int pa = s == 1 || s == 2, pb = s < 2;  // kBlkA / kBlkB
        ushortx8 v;
        const bool live = !border && 2 * (hp - 1) + pa < t1 &&
                          2 * (wp - 1) + pb < h1;
        if (live) {
          float acc[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] = bias[e];
#pragma unroll
          for (int dt = 0; dt < 3; ++dt)
#pragma unroll
            for (int df = 0; df < 3; ++df) {
              const float tap = p[2 * pa + dt][2 * pb + df];
#pragma unroll
              for (int e = 0; e < 8; ++e)
                acc[e] = fmaf(tap, w[3 * dt + df][e], acc[e]);
            }
#pragma unroll
          for (int e = 0; e < 8; ++e)
            v[e] = float_to_bf16_bits(fmaxf(acc[e], 0.f));
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = 0;
        }
        *reinterpret_cast<ushortx8*>(out + s * C) = v;
      }
    }
  }
}

// g = dX * (X > 0) over the live positions;
//   partials[blk, k*C + c] = sum tap_k * g (k < 9), partials[blk, 9*C + c] =
//   sum g. Border cells of dX are not read. Rows are walked as in the
// forward kernel.
__global__ __launch_bounds__(kOctThreads)
void conv1_s2d_bwd_kernel(const unsigned short* __restrict__ dX,
                          const unsigned short* __restrict__ X,
                          const unsigned short* __restrict__ x,
                          float* __restrict__ partials, int B, int T, int F,
                          int t1, int h1, int Hp, int Wp, int C) {
  __shared__ float red[kOctThreads][8];
  const int cvec = C / 8;
  const int slots = kOctThreads / cvec;
  const int slot = threadIdx.x / cvec;
  const int c8 = threadIdx.x - slot * cvec;
  const bool active = slot < slots;
  float acc[10][8];
#pragma unroll
  for (int k = 0; k < 10; ++k)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[k][e] = 0.f;
  const int nrow = B * Hp;
  if (active) {
    for (int row = blockIdx.x * slots + slot; row < nrow;
         row += gridDim.x * slots) {
      const int b = row / Hp;
      const int hp = row - b * Hp;
      if (hp == 0) continue;
      const PatchRows pr = patch_rows(x + (long)b * T * F, hp, T, F);
      const long at0 = (long)row * Wp * 4 * C + c8 * 8;
      const unsigned short* dp = dX + at0;
      const unsigned short* xp = X + at0;
      for (int wp = 1; wp < Wp; ++wp) {
        dp += 4 * C;
        xp += 4 * C;
        // All loads of the cell are issued before any is used. Positions
        // past (t1, h1) exist in both buffers and are masked, not skipped.
        ushortx8 dv[4], xv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          dv[s] = *reinterpret_cast<const ushortx8*>(dp + s * C);
          xv[s] = *reinterpret_cast<const ushortx8*>(xp + s * C);
        }
        float p[5][5];
        load_patch(pr, wp, F, p);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int pa = s == 1 || s == 2, pb = s < 2;
          const bool live = 2 * (hp - 1) + pa < t1 && 2 * (wp - 1) + pb < h1;
          float g[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            // X holds ReLU outputs: positive bf16 <=> bits in (0, 0x8000).
            // A positive NaN in X counts as > 0 here and passes dX, where
            // threshold_backward gives 0; finite data cannot tell them apart.
            g[e] = (live && xv[s][e] != 0 && xv[s][e] < 0x8000)
                       ? bf16_bits_to_float(dv[s][e]) : 0.f;
            acc[9][e] += g[e];
          }
#pragma unroll
          for (int dt = 0; dt < 3; ++dt)
#pragma unroll
            for (int df = 0; df < 3; ++df) {
              const float tap = p[2 * pa + dt][2 * pb + df];
#pragma unroll
              for (int e = 0; e < 8; ++e)
                acc[3 * dt + df][e] = fmaf(tap, g[e], acc[3 * dt + df][e]);
            }
        }
      }
    }
  }
  float* dst = partials + (long)blockIdx.x * 10 * C;
#pragma unroll
  for (int k = 0; k < 10; ++k)
    slot_reduce_store(acc[k], red, slots, cvec, active, dst + (long)k * C);
}

// O [B, Ho+1, Wo+1, Co] -> relu(O[:, 1:, 1:, :]) contiguous.
__global__ void unpad_relu_kernel(const unsigned short* __restrict__ O,
                                  unsigned short* __restrict__ y, long B,
                                  long Ho, long Wo, long Co) {
  const long Wp = Wo + 1;
  const long cvec = Co / 8;
  const long nvec = B * Ho * Wo * cvec;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec;
       i += (long)gridDim.x * blockDim.x) {
    long t = i;
    const long c8 = t % cvec;
    t /= cvec;
    const long w = t % Wo;
    t /= Wo;
    const long h = t % Ho;
    const long b = t / Ho;
    ushortx8 v = *reinterpret_cast<const ushortx8*>(
        O + ((b * (Ho + 1) + h + 1) * Wp + w + 1) * Co + c8 * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e)  // sign bit set: negative or -0; a NaN with
      v[e] = (v[e] & 0x8000) ? 0 : v[e];  // the sign bit set becomes 0 too,
                                          // where torch.relu keeps the NaN
    *reinterpret_cast<ushortx8*>(y + i * 8) = v;
  }
}

// dout, y [B, Ho, Wo, Co] -> dO [B, Ho+1, Wo+1, Co] = pad(dout * (y > 0))
// with a zero border, and partials[blk, Co] = column sums of the stored dO.
__global__ __launch_bounds__(kOctThreads)
void pad_scatter_relu_bwd_kernel(const unsigned short* __restrict__ dout,
                                 const unsigned short* __restrict__ y,
                                 unsigned short* __restrict__ dO,
                                 float* __restrict__ partials, long B,
                                 long Ho, long Wo, int Co) {
  __shared__ float red[kOctThreads][8];
  const long Hp = Ho + 1, Wp = Wo + 1;
  const int cvec = Co / 8;
  const int slots = kOctThreads / cvec;
  const int slot = threadIdx.x / cvec;
  const int c8 = threadIdx.x - slot * cvec;
  const bool active = slot < slots;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  const long nrow = B * Hp * Wp;
  if (active) {
    for (long row = (long)blockIdx.x * slots + slot; row < nrow;
         row += (long)gridDim.x * slots) {
      const long wp = row % Wp;
      const long hp = (row / Wp) % Hp;
      const long b = row / (Wp * Hp);
      ushortx8 v;
      if (hp == 0 || wp == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0;
      } else {
        const long src = ((b * Ho + hp - 1) * Wo + wp - 1) * Co + c8 * 8;
        const ushortx8 dv = *reinterpret_cast<const ushortx8*>(dout + src);
        const ushortx8 yv = *reinterpret_cast<const ushortx8*>(y + src);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          // as in conv1_s2d_bwd: a positive NaN in y passes dout
          v[e] = (yv[e] != 0 && yv[e] < 0x8000) ? dv[e] : 0;
          acc[e] += bf16_bits_to_float(v[e]);
        }
      }
      *reinterpret_cast<ushortx8*>(dO + row * Co + c8 * 8) = v;
    }
  }
  slot_reduce_store(acc, red, slots, cvec, active,
                    partials + (long)blockIdx.x * Co);
}

// Workgroups for an octet-per-thread kernel over `rows` rows. max_blocks > 0
// lowers the cap (tests use it to walk several rows per slot at small shapes).
inline int octet_grid(long rows, int cvec, int cap, long max_blocks = 0) {
  if (max_blocks > 0 && max_blocks < cap) cap = (int)max_blocks;
  const long slots = kOctThreads / cvec;
  const long want = (rows + slots - 1) / slots;
  return (int)std::max<long>(1, std::min<long>(want, cap));
}

inline bool bf16_cuda_contig(const torch::Tensor& t) {
  return t.is_cuda() && t.is_contiguous() &&
         t.scalar_type() == torch::kBFloat16;
}

}  // namespace

torch::Tensor conv1_s2d_fwd(torch::Tensor x, torch::Tensor w1,
                            torch::Tensor b1, int64_t max_blocks) {
  TORCH_CHECK(bf16_cuda_contig(x) && x.dim() == 3,
              "x must be contiguous CUDA bf16 [B,T,F]");
  TORCH_CHECK(bf16_cuda_contig(w1) && w1.dim() == 2 && w1.size(0) == 9,
              "w1 must be contiguous CUDA bf16 [9,C]");
  const long C = w1.size(1);
  TORCH_CHECK(C % 8 == 0 && C >= 8 && C / 8 <= kOctThreads,
              "C must be a multiple of 8, at most ", 8 * kOctThreads);
  TORCH_CHECK(bf16_cuda_contig(b1) && b1.dim() == 1 && b1.size(0) == C,
              "b1 must be contiguous CUDA bf16 [C]");
  const long B = x.size(0), T = x.size(1), F = x.size(2);
  TORCH_CHECK(T >= 1 && F >= 1, "empty time or frequency axis");
  const long t1 = (T + 1) / 2, h1 = (F + 1) / 2;
  const long Hp = (t1 + 1) / 2 + 1, Wp = (h1 + 1) / 2 + 1;
  TORCH_CHECK(T * F < (1L << 31) && B * Hp < (1L << 30),
              "utterance or batch too large for 32-bit row indices");
  auto X = torch::empty({B, Hp, Wp, 4 * C}, x.options());
  if (B == 0) return X;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(conv1_s2d_fwd_kernel,
                     dim3(octet_grid(B * Hp, (int)(C / 8), 4096, max_blocks)),
                     dim3(kOctThreads), 0, stream,
                     (const unsigned short*)x.data_ptr(),
                     (const unsigned short*)w1.data_ptr(),
                     (const unsigned short*)b1.data_ptr(),
                     (unsigned short*)X.data_ptr(), (int)B, (int)T, (int)F,
                     (int)t1, (int)h1, (int)Hp, (int)Wp, (int)C);
  return X;
}

// Returns {dw1 [9,C], db1 [C]} fp32 (views of one [10,C] buffer).
std::vector<torch::Tensor> conv1_s2d_bwd(torch::Tensor dX, torch::Tensor X,
                                         torch::Tensor x,
                                         int64_t max_blocks) {
  TORCH_CHECK(bf16_cuda_contig(x) && x.dim() == 3,
              "x must be contiguous CUDA bf16 [B,T,F]");
  TORCH_CHECK(bf16_cuda_contig(X) && X.dim() == 4 && X.size(3) % 32 == 0,
              "X must be contiguous CUDA bf16 [B,Ho+1,Wo+1,4C], C % 8 == 0");
  TORCH_CHECK(bf16_cuda_contig(dX) && dX.sizes() == X.sizes(),
              "dX must match X");
  const long B = x.size(0), T = x.size(1), F = x.size(2);
  const long C = X.size(3) / 4;
  TORCH_CHECK(T >= 1 && F >= 1, "empty time or frequency axis");
  const long t1 = (T + 1) / 2, h1 = (F + 1) / 2;
  const long Hp = (t1 + 1) / 2 + 1, Wp = (h1 + 1) / 2 + 1;
  TORCH_CHECK(X.size(0) == B && X.size(1) == Hp && X.size(2) == Wp,
              "X does not belong to x");
  TORCH_CHECK(C / 8 <= kOctThreads, "C must be at most ", 8 * kOctThreads);
  TORCH_CHECK(T * F < (1L << 31) && B * Hp < (1L << 30),
              "utterance or batch too large for 32-bit row indices");
  auto fopts = x.options().dtype(torch::kFloat32);
  auto out = torch::empty({10, C}, fopts);
  if (B == 0) {
    out.zero_();
    return {out.narrow(0, 0, 9), out.select(0, 9)};
  }
  const int grid = octet_grid(B * Hp, (int)(C / 8), 1024, max_blocks);
  auto partials = torch::empty({(long)grid, 10 * C}, fopts);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(conv1_s2d_bwd_kernel, dim3(grid), dim3(kOctThreads), 0,
                     stream, (const unsigned short*)dX.data_ptr(),
                     (const unsigned short*)X.data_ptr(),
                     (const unsigned short*)x.data_ptr(),
                     partials.data_ptr<float>(), (int)B, (int)T, (int)F,
                     (int)t1, (int)h1, (int)Hp, (int)Wp, (int)C);
  colsum_reduce(partials.data_ptr<float>(), out.data_ptr<float>(), grid,
                10 * C, stream);
  return {out.narrow(0, 0, 9), out.select(0, 9)};
}

torch::Tensor unpad_relu(torch::Tensor O) {
  TORCH_CHECK(bf16_cuda_contig(O) && O.dim() == 4 && O.size(3) % 8 == 0 &&
              O.size(1) >= 1 && O.size(2) >= 1,
              "O must be contiguous CUDA bf16 [B,Ho+1,Wo+1,Co], Co % 8 == 0");
  const long B = O.size(0), Ho = O.size(1) - 1, Wo = O.size(2) - 1,
             Co = O.size(3);
  auto y = torch::empty({B, Ho, Wo, Co}, O.options());
  const long nvec = y.numel() / 8;
  if (nvec == 0) return y;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(unpad_relu_kernel, dim3(memory_bound_grid(nvec, 256)),
                     dim3(256), 0, stream,
                     (const unsigned short*)O.data_ptr(),
                     (unsigned short*)y.data_ptr(), B, Ho, Wo, Co);
  return y;
}

// Returns {dO [B,Ho+1,Wo+1,Co] bf16, column sums of dO [Co] fp32}.
std::vector<torch::Tensor> pad_scatter_relu_bwd(torch::Tensor dout,
                                                torch::Tensor y,
                                                int64_t max_blocks) {
  TORCH_CHECK(bf16_cuda_contig(dout) && dout.dim() == 4 &&
              dout.size(3) % 8 == 0 && dout.size(3) >= 8 &&
              dout.size(3) / 8 <= kOctThreads,
              "dout must be contiguous CUDA bf16 [B,Ho,Wo,Co], Co % 8 == 0");
  TORCH_CHECK(bf16_cuda_contig(y) && y.sizes() == dout.sizes(),
              "y must match dout");
  const long B = dout.size(0), Ho = dout.size(1), Wo = dout.size(2),
             Co = dout.size(3);
  auto fopts = dout.options().dtype(torch::kFloat32);
  auto dO = torch::empty({B, Ho + 1, Wo + 1, Co}, dout.options());
  auto db = torch::empty({Co}, fopts);
  if (B == 0) {
    db.zero_();
    return {dO, db};
  }
  const int grid = octet_grid(B * (Ho + 1) * (Wo + 1), (int)(Co / 8), 2048,
                              max_blocks);
  auto partials = torch::empty({(long)grid, Co}, fopts);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(pad_scatter_relu_bwd_kernel, dim3(grid),
                     dim3(kOctThreads), 0, stream,
                     (const unsigned short*)dout.data_ptr(),
                     (const unsigned short*)y.data_ptr(),
                     (unsigned short*)dO.data_ptr(),
                     partials.data_ptr<float>(), B, Ho, Wo, (int)Co);
  colsum_reduce(partials.data_ptr<float>(), db.data_ptr<float>(), grid, Co,
                stream);
  return {dO, db};
}

torch::Tensor s2d_fwd(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 4 &&
              x.scalar_type() == torch::kBFloat16 && x.size(3) % 8 == 0 &&
              x.size(1) % 2 == 0 && x.size(2) % 2 == 0);
  const long B = x.size(0), Ho = x.size(1) / 2, Wo = x.size(2) / 2,
             C = x.size(3);
  auto out = torch::empty({B, Ho + 1, Wo + 1, 4 * C}, x.options());
  long nvec = out.numel() / 8;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(s2d_fwd_kernel, dim3(memory_bound_grid(nvec, 256)),
                     dim3(256), 0, stream,
                     (const unsigned short*)x.data_ptr(),
                     (unsigned short*)out.data_ptr(), B, Ho, Wo, C);
  return out;
}

torch::Tensor s2d_inv(torch::Tensor dX, int64_t C) {
  TORCH_CHECK(dX.is_cuda() && dX.is_contiguous() && dX.dim() == 4 &&
              dX.scalar_type() == torch::kBFloat16 && C % 8 == 0 &&
              dX.size(3) == 4 * C);
  const long B = dX.size(0), Ho = dX.size(1) - 1, Wo = dX.size(2) - 1;
  auto dx = torch::empty({B, 2 * Ho, 2 * Wo, C}, dX.options());
  long nvec = dx.numel() / 8;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(s2d_inv_kernel, dim3(memory_bound_grid(nvec, 256)),
                     dim3(256), 0, stream,
                     (const unsigned short*)dX.data_ptr(),
                     (unsigned short*)dx.data_ptr(), B, Ho, Wo, C);
  return dx;
}

torch::Tensor pad_scatter(torch::Tensor dout) {
  TORCH_CHECK(dout.is_cuda() && dout.is_contiguous() && dout.dim() == 4 &&
              dout.scalar_type() == torch::kBFloat16 &&
              dout.size(3) % 8 == 0);
  const long B = dout.size(0), Ho = dout.size(1), Wo = dout.size(2),
             Co = dout.size(3);
  auto out = torch::empty({B, Ho + 1, Wo + 1, Co}, dout.options());
  long nvec = out.numel() / 8;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(pad_scatter_kernel,
                     dim3(memory_bound_grid(nvec, 256)), dim3(256), 0,
                     stream, (const unsigned short*)dout.data_ptr(),
                     (unsigned short*)out.data_ptr(), B, Ho, Wo, Co);
  return out;
}
