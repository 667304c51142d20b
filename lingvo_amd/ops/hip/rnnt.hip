// Transducer (RNN-T) loss for gfx950: forward (nll, valid) and backward
// (dlogits) over joint logits [B,T,U1,V] in bf16 or fp32 (U1 = U+1), with
// no fp32 [B,T,U1,V] intermediate and no floating-point atomics.
//
// Three passes, ordered only by kernel boundaries on one stream:
//  1. rnnt_rows_kernel: one wave per (b,t,u) row. Online logsumexp over
//     the row (16-byte loads, scalar head/tail for rows that are not
//     16-byte aligned) -> lse[b,t,u] = (max, log sum), then the row's
//     two emissions E[b,t,u] = (log p(blank), log p(label_{u+1})).
//  2. rnnt_lattice_kernel: grid (B, 2), one workgroup per utterance and
//     direction (alpha / beta), one lane per u, one anti-diagonal
//     d = t + u per step (T_b + U_b steps), two LDS buffers swapped each
//     diagonal, one __syncthreads() per diagonal; the next diagonal's
//     emissions are loaded before the barrier. Writes alpha, beta
//     [B,T,U1] and, from the alpha workgroup, nll[b] and valid[b].
//  3. rnnt_grad_kernel: one wave per row. Softmax recomputed from logits
//     and lse; the blank and label columns get their transition terms in
//     fp32 inside the same pass, so every element is stored once (a bf16
//     gradient is rounded once). Plain vector stores.
//
// Recursion (T_b, U_b the row's lengths):
//   alpha(0,0) = 0
//   alpha(t,u) = lse2(alpha(t-1,u) + blank(t-1,u), alpha(t,u-1) + label(t,u-1))
//   ll         = alpha(T_b-1,U_b) + blank(T_b-1,U_b)
//   beta(T_b-1,U_b) = blank(T_b-1,U_b)
//   beta(t,u)  = lse2(beta(t+1,u) + blank(t,u), beta(t,u+1) + label(t,u))
//
// "Impossible" is the finite sentinel kNeg (-1e30), never -inf or NaN.
//
// Precision. Everything of the size of the logits is read and written in
// their dtype and computed in fp32. The [B,T,U1] tables are fp64: the
// gradient is built from exp(alpha + beta - ll), a difference of numbers of
// the size of |ll|, and in fp32 it carries an ulp of |ll| (1e-4 at 1000),
// tens to thousands of times the error of autograd through the fp32
// recursion. For the same reason the row pass keeps logsumexp as its two
// parts (max, log sum): log p = (x - max) - log(sum) is exact where p is
// large. The tables are 1/V of the logits, so fp64 costs no bandwidth.
//
// A row is invalid (valid = 0, nll = 0, dlogits = 0) when T_b is outside
// [1,T] or U_b outside [0,U], when a label inside U_b is the blank or
// outside [0,V), or when its likelihood is not finite. No label is used as
// an index before it is range-checked. Every element of every output and
// workspace is written; cells with t >= T_b or u > U_b hold zeros.

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include "common.h"
#include "lse_rows.h"

namespace {

constexpr int kRnntMaxU = 1023;  // U1 = U+1 <= 1024 lanes of one workgroup
constexpr int kRowWaves = 4;     // rows per workgroup in the row/grad passes
constexpr double kNeg = -1e30;
constexpr double kNegTest = -1e29;

// Lengths of utterance b, zeroed when either is out of range.
__device__ __forceinline__ bool RowLengths(const long* in_len,
                                           const long* lab_len, int b, int T,
                                           int U, int* tb, int* ub) {
  const long t = in_len[b];
  const long u = lab_len[b];
  const bool ok = t >= 1 && t <= T && u >= 0 && u <= U;
  *tb = ok ? (int)t : 0;
  *ub = ok ? (int)u : 0;
  return ok;
}

__device__ __forceinline__ double Lse2(double a, double b) {
  const double m = fmax(a, b);
  if (!(m > kNegTest)) return kNeg;
  return m + log(exp(a - m) + exp(b - m));
}

// ---- pass 1: lse + the two emissions of every row --------------------------
template <typename T>
__global__ void __launch_bounds__(kRowWaves* WAVE_SIZE)
    rnnt_rows_kernel(const T* __restrict__ logits,
                     const long* __restrict__ in_len,
                     const long* __restrict__ labels,
                     const long* __restrict__ lab_len,
                     float2* __restrict__ lse_out, double2* __restrict__ emis,
                     long rows, int Tn, int U1, int V, int blank) {
  typedef Elem<T> El;
  const long row = (long)blockIdx.x * kRowWaves + threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  if (row >= rows) return;
  const int u = (int)(row % U1);
  const long bt = row / U1;
  const int t = (int)(bt % Tn);
  const int b = (int)(bt / Tn);
  int tb, ub;
  RowLengths(in_len, lab_len, b, Tn, U1 - 1, &tb, &ub);
  if (t >= tb || u > ub) {  // outside the lattice: nothing to read
    if (lane == 0) {
      lse_out[row] = make_float2(0.f, 0.f);
      emis[row] = make_double2(0., 0.);
    }
    return;
  }
  const T* lr = logits + row * V;
  // The two emission columns, asked for ahead of the row so that their
  // latency (label, then logit) hides under it. Same address in every lane.
  const float x_blank = El::ToFloat(lr[blank]);
  float x_label = 0.f;
  bool has_label = false;
  if (u < ub) {
    const long lbl = labels[(long)b * (U1 - 1) + u];
    has_label = lbl >= 0 && lbl < V;
    if (has_label) x_label = El::ToFloat(lr[lbl]);
  }
  // The pass is bound by VALU work, not by memory, so the online update
  // runs once per 16-byte vector (one rescale, then kVec exponentials)
  // and the wave is reduced max first, then sum: one rescale per lane.
  float m = -1e30f, s = 0.f;
  const int head = HeadElems(lr, V);
  const int nvec = (V - head) / El::kVec;
  for (int j = lane; j < head; j += WAVE_SIZE) OnlineLse(El::ToFloat(lr[j]), m, s);
  for (int i = lane; i < nvec; i += WAVE_SIZE) {
    typename El::Vec v =
        *reinterpret_cast<const typename El::Vec*>(lr + head + i * El::kVec);
    float f[El::kVec];
    float vm = -1e30f;
#pragma unroll
    for (int e = 0; e < El::kVec; ++e) {
      f[e] = El::ToFloat(v[e]);
      vm = fmaxf(vm, f[e]);
    }
    if (vm > m) {
      s *= expf(m - vm);
      m = vm;
    }
#pragma unroll
    for (int e = 0; e < El::kVec; ++e) s += expf(f[e] - m);
  }
  for (int j = head + nvec * El::kVec + lane; j < V; j += WAVE_SIZE)
    OnlineLse(El::ToFloat(lr[j]), m, s);
  const float lane_m = m;
  m = wave_reduce_max(m);
  s = wave_reduce_sum(s * expf(lane_m - m));
  if (lane == 0) {
    const double norm = log((double)s);
    const double e_label =
        has_label ? ((double)x_label - (double)m) - norm : 0.;
    lse_out[row] = make_float2(m, logf(s));
    emis[row] = make_double2(((double)x_blank - (double)m) - norm, e_label);
  }
}

// ---- pass 2: alpha / beta over anti-diagonals ------------------------------
__global__ void __launch_bounds__(1024)
    rnnt_lattice_kernel(const double2* __restrict__ emis,
                        const long* __restrict__ in_len,
                        const long* __restrict__ labels,
                        const long* __restrict__ lab_len,
                        double* __restrict__ alpha, double* __restrict__ beta,
                        float* __restrict__ nll, float* __restrict__ valid,
                        int Tn, int U1, int V, int blank) {
  __shared__ double buf[2][1024 + 1];
  const int b = blockIdx.x;
  const int dir = blockIdx.y;
  const int u = threadIdx.x;  // blockDim.x >= U1
  int tb, ub;
  const bool len_ok = RowLengths(in_len, lab_len, b, Tn, U1 - 1, &tb, &ub);

  int bad = 0;
  if (u < ub) {
    const long v = labels[(long)b * (U1 - 1) + u];
    bad = (v < 0 || v >= V || v == blank) ? 1 : 0;
  }
  const int nbad = __syncthreads_count(bad);
  const bool feasible = len_ok && nbad == 0;  // uniform over the workgroup

  const long cells = (long)Tn * U1;
  double* out = (dir ? beta : alpha) + (long)b * cells;
  if (!feasible) {
    for (long i = u; i < cells; i += blockDim.x) out[i] = 0.;
    if (dir == 0 && u == 0) {
      nll[b] = 0.f;
      valid[b] = 0.f;
    }
    return;
  }
  // Cells outside the lattice; the loop below writes every cell inside.
  if (u < U1) {
    for (int t = 0; t < Tn; ++t)
      if (t >= tb || u > ub) out[(long)t * U1 + u] = 0.;
  }

  const double2* eb = emis + (long)b * cells + u;
  const int nd = tb + ub;  // diagonals 0 .. T_b-1 + U_b
  const bool lane_on = u <= ub;
  // Step k visits diagonal d = k (alpha) or nd-1-k (beta); this lane's
  // cell on it is t = d - u.
  const int step = dir ? -1 : 1;
  int t = (dir ? nd - 1 : 0) - u;
  // own: alpha(t-1,u) + blank(t-1,u) going forward, beta(t+1,u) going back.
  double own = kNeg;
  double2 e_cur = make_double2(0., 0.);
  if (lane_on && t >= 0 && t < tb) e_cur = eb[(long)t * U1];
  for (int k = 0; k < nd; ++k, t += step) {
    const bool on = lane_on && t >= 0 && t < tb;
    const int tn = t + step;
    double2 e_next = make_double2(0., 0.);
    if (lane_on && tn >= 0 && tn < tb && k + 1 < nd) e_next = eb[(long)tn * U1];
    const double* prev = buf[(k + 1) & 1];
    double share = kNeg;  // what the neighbouring lane reads next step
    if (on) {
      double v;
      if (dir == 0) {
        if (t == 0 && u == 0) {
          v = 0.;
        } else {
          const double from_label = (u > 0 && k > 0) ? prev[u - 1] : kNeg;
          v = Lse2(own, from_label);
        }
        const bool live = v > kNegTest;
        own = live ? v + e_cur.x : kNeg;
        share = (live && u < ub) ? v + e_cur.y : kNeg;
      } else {
        if (t == tb - 1 && u == ub) {
          v = e_cur.x;
        } else {
          const double nb = (u < ub && k > 0) ? prev[u + 1] : kNeg;
          const double via_blank =
              (t + 1 < tb && own > kNegTest) ? own + e_cur.x : kNeg;
          const double via_label = nb > kNegTest ? nb + e_cur.y : kNeg;
          v = Lse2(via_blank, via_label);
        }
        own = v;
        share = v;
      }
      out[(long)t * U1 + u] = v;
    }
    buf[k & 1][u] = share;
    e_cur = e_next;
    __syncthreads();
  }
  if (dir == 0 && u == ub) {
    // own = alpha(T_b-1,U_b) + blank(T_b-1,U_b) after the last diagonal.
    const bool ok = own > kNegTest && isfinite(own);
    nll[b] = ok ? (float)-own : 0.f;
    valid[b] = ok ? 1.f : 0.f;
  }
}

// ---- pass 3: dlogits -------------------------------------------------------
template <typename T>
__device__ __forceinline__ T GradElem(T x, int j, float scale, float2 lse,
                                      int blank, float cb, int lab, float cl) {
  typedef Elem<T> El;
  float v = scale * expf((El::ToFloat(x) - lse.x) - lse.y);
  if (j == blank) v -= cb;
  if (j == lab) v -= cl;
  return El::FromFloat(v);
}

template <typename T>
__global__ void __launch_bounds__(kRowWaves* WAVE_SIZE)
    rnnt_grad_kernel(const T* __restrict__ logits,
                     const long* __restrict__ in_len,
                     const long* __restrict__ labels,
                     const long* __restrict__ lab_len,
                     const float2* __restrict__ lse,
                     const double2* __restrict__ emis,
                     const double* __restrict__ alpha,
                     const double* __restrict__ beta,
                     const float* __restrict__ valid,
                     const float* __restrict__ gnll, T* __restrict__ dlogits,
                     long rows, int Tn, int U1, int V, int blank) {
  typedef Elem<T> El;
  const long row = (long)blockIdx.x * kRowWaves + threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x & (WAVE_SIZE - 1);
  if (row >= rows) return;
  const int u = (int)(row % U1);
  const long bt = row / U1;
  const int t = (int)(bt % Tn);
  const int b = (int)(bt / Tn);
  int tb, ub;
  RowLengths(in_len, lab_len, b, Tn, U1 - 1, &tb, &ub);
  const float g = gnll[b];
  // Uniform over the wave.
  const bool live = valid[b] != 0.f && t < tb && u <= ub && g != 0.f;
  const T* lr = logits + row * V;
  T* dr = dlogits + row * V;

  float scale = 0.f, cb = 0.f, cl = 0.f;
  float2 lse_r = make_float2(0.f, 0.f);
  int lab = -1;
  if (live) {
    // valid[b] != 0 implies every label in [0, ub) is a non-blank id
    // inside [0, V). The occupancy terms are differences of numbers of the
    // size of ll = beta(0,0): fp64, rounded to fp32 once.
    const double ll = beta[(long)b * Tn * U1];
    const double a = alpha[row] - ll;
    const double2 e = emis[row];
    const double gd = (double)g;
    lse_r = lse[row];
    scale = (float)(gd * exp(a + beta[row]));
    if (t + 1 < tb) {
      cb = (float)(gd * exp(a + e.x + beta[row + U1]));
    } else if (u == ub) {
      cb = (float)(gd * exp(a + e.x));
    }
    if (u < ub) {
      lab = (int)labels[(long)b * (U1 - 1) + u];
      cl = (float)(gd * exp(a + e.y + beta[row + 1]));
    }
  }

  const bool same_phase =
      ((reinterpret_cast<uintptr_t>(lr) ^ reinterpret_cast<uintptr_t>(dr)) &
       15) == 0;
  const int head = same_phase ? HeadElems(dr, V) : V;
  const int nvec = (V - head) / El::kVec;
  const T zero = El::FromFloat(0.f);
  for (int j = lane; j < head; j += WAVE_SIZE)
    dr[j] = live ? GradElem<T>(lr[j], j, scale, lse_r, blank, cb, lab, cl)
                 : zero;
  for (int i = lane; i < nvec; i += WAVE_SIZE) {
    const int j0 = head + i * El::kVec;
    typename El::Vec o;
    if (live) {
      typename El::Vec v =
          *reinterpret_cast<const typename El::Vec*>(lr + j0);
#pragma unroll
      for (int e = 0; e < El::kVec; ++e)
        o[e] = GradElem<T>(v[e], j0 + e, scale, lse_r, blank, cb, lab, cl);
    } else {
#pragma unroll
      for (int e = 0; e < El::kVec; ++e) o[e] = zero;
    }
    *reinterpret_cast<typename El::Vec*>(dr + j0) = o;
  }
  for (int j = head + nvec * El::kVec + lane; j < V; j += WAVE_SIZE)
    dr[j] = live ? GradElem<T>(lr[j], j, scale, lse_r, blank, cb, lab, cl)
                 : zero;
}

// ---- host ------------------------------------------------------------------
bool CudaContig(const torch::Tensor& t, torch::ScalarType dt) {
  return t.is_cuda() && t.is_contiguous() && t.scalar_type() == dt;
}

struct RnntShape {
  int B, T, U1, V;
};

RnntShape CheckRnntInputs(const torch::Tensor& logits,
                          const torch::Tensor& logit_lengths,
                          const torch::Tensor& labels,
                          const torch::Tensor& label_lengths, int64_t blank) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() &&
                  logits.dim() == 4 &&
                  (logits.scalar_type() == torch::kBFloat16 ||
                   logits.scalar_type() == torch::kFloat32),
              "rnnt: logits must be CUDA contiguous bf16 or fp32 [B,T,U+1,V]");
  const int64_t b = logits.size(0), t = logits.size(1), u1 = logits.size(2),
                v = logits.size(3);
  TORCH_CHECK(b >= 1 && t >= 1 && u1 >= 1, "rnnt: B >= 1, T >= 1, U+1 >= 1");
  TORCH_CHECK(v >= 2, "rnnt: V >= 2");
  TORCH_CHECK(u1 - 1 <= kRnntMaxU, "rnnt: U=", u1 - 1,
              " is over the supported limit ", kRnntMaxU);
  TORCH_CHECK(b * t * u1 < (1LL << 31) && v < (1LL << 31),
              "rnnt: B*T*(U+1) and V must fit in int32");
  TORCH_CHECK(blank >= 0 && blank < v, "rnnt: blank_id must be in [0, V)");
  TORCH_CHECK(CudaContig(labels, torch::kInt64) && labels.dim() == 2 &&
                  labels.size(0) == b && labels.size(1) + 1 == u1,
              "rnnt: labels must be CUDA contiguous int64 [B,U] with "
              "U+1 == logits.shape[2]");
  TORCH_CHECK(CudaContig(logit_lengths, torch::kInt64) &&
                  logit_lengths.dim() == 1 && logit_lengths.size(0) == b,
              "rnnt: logit_lengths must be CUDA contiguous int64 [B]");
  TORCH_CHECK(CudaContig(label_lengths, torch::kInt64) &&
                  label_lengths.dim() == 1 && label_lengths.size(0) == b,
              "rnnt: label_lengths must be CUDA contiguous int64 [B]");
  TORCH_CHECK(logits.get_device() == labels.get_device() &&
                  logits.get_device() == logit_lengths.get_device() &&
                  logits.get_device() == label_lengths.get_device(),
              "rnnt: all inputs must be on one device");
  return {(int)b, (int)t, (int)u1, (int)v};
}

void CheckSaved(const torch::Tensor& x, torch::ScalarType dt,
                std::vector<int64_t> shape, const torch::Tensor& like,
                const char* name) {
  TORCH_CHECK(CudaContig(x, dt) && x.sizes().vec() == shape &&
                  x.get_device() == like.get_device(),
              "rnnt: ", name, " must be CUDA contiguous, of the dtype and "
              "shape rnnt_fwd returned");
}

}  // namespace

int64_t rnnt_max_label_len() { return kRnntMaxU; }

// -> {nll [B] f32, valid [B] f32, lse [B,T,U1,2] f32 (max, log sum),
//     emis [B,T,U1,2] f64, alpha, beta [B,T,U1] f64}
std::vector<torch::Tensor> rnnt_fwd(torch::Tensor logits,
                                    torch::Tensor logit_lengths,
                                    torch::Tensor labels,
                                    torch::Tensor label_lengths,
                                    int64_t blank) {
  const RnntShape sh =
      CheckRnntInputs(logits, logit_lengths, labels, label_lengths, blank);
  const int B = sh.B, T = sh.T, U1 = sh.U1, V = sh.V;
  auto opts = logits.options().dtype(torch::kFloat32);
  auto nll = torch::empty({B}, opts);
  auto valid = torch::empty({B}, opts);
  auto opts64 = logits.options().dtype(torch::kFloat64);
  auto lse = torch::empty({B, T, U1, 2}, opts);
  auto emis = torch::empty({B, T, U1, 2}, opts64);
  auto alpha = torch::empty({B, T, U1}, opts64);
  auto beta = torch::empty({B, T, U1}, opts64);
  auto stream = at::cuda::getCurrentCUDAStream();
  const long rows = (long)B * T * U1;
  const dim3 rgrid(cdiv(rows, kRowWaves)), rblock(kRowWaves * WAVE_SIZE);
  double2* emis_p = reinterpret_cast<double2*>(emis.data_ptr<double>());
  float2* lse_p = reinterpret_cast<float2*>(lse.data_ptr<float>());
  if (logits.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(rnnt_rows_kernel<unsigned short>, rgrid, rblock, 0,
                       stream, (const unsigned short*)logits.data_ptr(),
                       logit_lengths.data_ptr<long>(),
                       labels.data_ptr<long>(),
                       label_lengths.data_ptr<long>(), lse_p, emis_p, rows, T,
                       U1, V, (int)blank);
  } else {
    hipLaunchKernelGGL(rnnt_rows_kernel<float>, rgrid, rblock, 0, stream,
                       logits.data_ptr<float>(),
                       logit_lengths.data_ptr<long>(),
                       labels.data_ptr<long>(),
                       label_lengths.data_ptr<long>(), lse_p, emis_p, rows, T,
                       U1, V, (int)blank);
  }
  const int threads = cdiv(U1, WAVE_SIZE) * WAVE_SIZE;  // <= 1024
  hipLaunchKernelGGL(rnnt_lattice_kernel, dim3(B, 2), dim3(threads), 0, stream,
                     emis_p, logit_lengths.data_ptr<long>(),
                     labels.data_ptr<long>(), label_lengths.data_ptr<long>(),
                     alpha.data_ptr<double>(), beta.data_ptr<double>(),
                     nll.data_ptr<float>(), valid.data_ptr<float>(), T, U1, V,
                     (int)blank);
  return {nll, valid, lse, emis, alpha, beta};
}

torch::Tensor rnnt_bwd(torch::Tensor logits, torch::Tensor logit_lengths,
                       torch::Tensor labels, torch::Tensor label_lengths,
                       torch::Tensor lse, torch::Tensor emis,
                       torch::Tensor alpha, torch::Tensor beta,
                       torch::Tensor valid, torch::Tensor gnll,
                       int64_t blank) {
  const RnntShape sh =
      CheckRnntInputs(logits, logit_lengths, labels, label_lengths, blank);
  const int64_t B = sh.B, T = sh.T, U1 = sh.U1;
  CheckSaved(lse, torch::kFloat32, {B, T, U1, 2}, logits, "lse");
  CheckSaved(emis, torch::kFloat64, {B, T, U1, 2}, logits, "emis");
  CheckSaved(alpha, torch::kFloat64, {B, T, U1}, logits, "alpha");
  CheckSaved(beta, torch::kFloat64, {B, T, U1}, logits, "beta");
  CheckSaved(valid, torch::kFloat32, {B}, logits, "valid");
  CheckSaved(gnll, torch::kFloat32, {B}, logits, "gnll");
  auto dlogits = torch::empty_like(logits);
  auto stream = at::cuda::getCurrentCUDAStream();
  const long rows = (long)B * T * U1;
  const dim3 grid(cdiv(rows, kRowWaves)), block(kRowWaves * WAVE_SIZE);
  const double2* emis_p =
      reinterpret_cast<const double2*>(emis.data_ptr<double>());
  const float2* lse_p = reinterpret_cast<const float2*>(lse.data_ptr<float>());
  if (logits.scalar_type() == torch::kBFloat16) {
    hipLaunchKernelGGL(
        rnnt_grad_kernel<unsigned short>, grid, block, 0, stream,
        (const unsigned short*)logits.data_ptr(),
        logit_lengths.data_ptr<long>(), labels.data_ptr<long>(),
        label_lengths.data_ptr<long>(), lse_p, emis_p,
        alpha.data_ptr<double>(), beta.data_ptr<double>(),
        valid.data_ptr<float>(), gnll.data_ptr<float>(),
        (unsigned short*)dlogits.data_ptr(), rows,
        sh.T, sh.U1, sh.V, (int)blank);
  } else {
    hipLaunchKernelGGL(
        rnnt_grad_kernel<float>, grid, block, 0, stream,
        logits.data_ptr<float>(), logit_lengths.data_ptr<long>(),
        labels.data_ptr<long>(), label_lengths.data_ptr<long>(),
        lse_p, emis_p, alpha.data_ptr<double>(), beta.data_ptr<double>(),
        valid.data_ptr<float>(), gnll.data_ptr<float>(),
        dlogits.data_ptr<float>(), rows, sh.T, sh.U1, sh.V, (int)blank);
  }
  return dlogits;
}
