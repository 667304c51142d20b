// Row helpers shared by the lattice losses (ctc.hip, rnnt.hip): 16-byte
// vectors of bf16 / fp32 logits, the unaligned head of a row, and the
// online logsumexp update.
#pragma once

#include <cstdint>

#include "common.h"

namespace {

// dtype helpers: 16-byte vectors of logits.
template <typename T>
struct Elem;

template <>
struct Elem<float> {
  static constexpr int kVec = 4;
  typedef floatx4 Vec;
  static __device__ __forceinline__ float ToFloat(float x) { return x; }
  static __device__ __forceinline__ float FromFloat(float x) { return x; }
};

template <>
struct Elem<unsigned short> {  // bf16 bits
  static constexpr int kVec = 8;
  typedef ushortx8 Vec;
  static __device__ __forceinline__ float ToFloat(unsigned short x) {
    return bf16_bits_to_float(x);
  }
  static __device__ __forceinline__ unsigned short FromFloat(float x) {
    return float_to_bf16_bits(x);
  }
};

// Elements before the first 16-byte boundary of row pointer p (<= n).
template <typename T>
__device__ __forceinline__ int HeadElems(const T* p, int n) {
  const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 15);
  const int head = mis ? (16 - mis) / (int)sizeof(T) : 0;
  return head < n ? head : n;
}

__device__ __forceinline__ void OnlineLse(float f, float& m, float& s) {
  if (f > m) {
    s *= expf(m - f);
    m = f;
  }
  s += expf(f - m);
}

}  // namespace
