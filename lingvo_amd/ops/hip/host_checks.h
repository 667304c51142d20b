// Host-side operand predicates of the op wrappers: CUDA, dtype, contiguous
// or dense rows, shape, 16-byte base. The bool forms go into a TORCH_CHECK
// with the wrapper's own message; the check_* forms raise with theirs.
#pragma once

#include <torch/extension.h>

#include <cstdint>

inline bool cuda_contig(const torch::Tensor& t, torch::ScalarType st) {
  return t.is_cuda() && t.is_contiguous() && t.scalar_type() == st;
}

// A [rows, cols] tensor of dtype st whose rows are dense (a row of a
// larger contiguous stack is).
inline bool cuda_rows(const torch::Tensor& t, torch::ScalarType st,
                      int64_t rows, int64_t cols) {
  return cuda_contig(t, st) && t.dim() == 2 && t.size(0) == rows &&
         t.size(1) == cols;
}

// The bf16 payload as the raw bits the kernels take.
inline unsigned short* u16(const torch::Tensor& t) {
  return (unsigned short*)t.data_ptr();
}

inline bool aligned16(const torch::Tensor& t) {
  return (uintptr_t)t.data_ptr() % 16 == 0;
}

inline void check_contig(const torch::Tensor& t, torch::ScalarType st,
                         const char* name) {
  TORCH_CHECK(cuda_contig(t, st), name, " must be a contiguous ",
              st == torch::kBFloat16 ? "bf16" : "fp32", " device tensor");
}

// bf16 [rows, cols] read element-wise with a row stride, which is returned.
inline long check_strided_rows(const torch::Tensor& t, int64_t rows,
                               int64_t cols, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.dim() == 2 && t.size(0) == rows && t.size(1) == cols &&
                  t.stride(1) == 1 && (rows == 1 || t.stride(0) >= cols),
              name, " must be CUDA bf16 [", rows, ",", cols,
              "] with unit column stride");
  return rows == 1 ? (long)cols : (long)t.stride(0);
}

inline void check_dense(const torch::Tensor& t, torch::ScalarType st,
                        int64_t rows, int64_t cols, const char* name) {
  TORCH_CHECK(cuda_rows(t, st, rows, cols) && aligned16(t), name,
              " must be a dense CUDA [", rows, ",", cols, "] tensor of ", st);
}
