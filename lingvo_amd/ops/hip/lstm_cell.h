// The LSTM cell of every recurrence kernel (lstm_gates.hip, lstm_scan.hip,
// las_step.hip), stated once. Reference: lingvo/core/rnn_cell.py:213
// LSTMCellSimple; gate order [i_i (cand), i_g (i), f_g (f), o_g (o)].
//   cand = tanh(g0), i = sig(g1), f = sig(g2 + fgb), o = sig(g3)
//   c = clamp(f * c_prev + i * cand, +-cap)  (cap <= 0: no clamp)
//   m = o * tanh(c)
// All fp32, in one fixed association: the kernels are compared bit for bit.
// What differs between kernels (which c the backward takes tanh of, the
// padding blend of the scan, the dtype of the carries) stays with the callers.
#pragma once

#include "common.h"

__device__ __forceinline__ float sigf(float x) {
  return 1.f / (1.f + __expf(-x));
}

struct LstmActs {
  float cand, ig, fg, og;
};

__device__ __forceinline__ LstmActs lstm_acts(float g0, float g1, float g2,
                                              float g3, float fgb) {
  return {tanhf(g0), sigf(g1), sigf(g2 + fgb), sigf(g3)};
}

struct LstmC {
  float raw, c;  // before and after the clamp
};

__device__ __forceinline__ LstmC lstm_cell_update(const LstmActs& a,
                                                  float c_prev, float cap) {
  const float raw = a.fg * c_prev + a.ig * a.cand;
  return {raw, cap > 0.f ? fminf(cap, fmaxf(-cap, raw)) : raw};
}

struct LstmGrads {
  float dg[4], dc_prev;  // dg in gate order
};

// tc is tanh of the cell value m was formed from, craw the pre-clamp cell
// value: a clamped cell passes no gradient to c_prev or to cand, i, f.
__device__ __forceinline__ LstmGrads lstm_cell_bwd(const LstmActs& a,
                                                   float c_prev, float tc,
                                                   float craw, float cap,
                                                   float dm, float dc_in) {
  const float do_ = dm * tc;
  float dc = dc_in + dm * a.og * (1.f - tc * tc);
  if (cap > 0.f && (craw > cap || craw < -cap)) dc = 0.f;
  return {{dc * a.ig * (1.f - a.cand * a.cand),
           dc * a.cand * a.ig * (1.f - a.ig),
           dc * c_prev * a.fg * (1.f - a.fg), do_ * a.og * (1.f - a.og)},
          dc * a.fg};
}
