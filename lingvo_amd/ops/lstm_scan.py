"""Fused (bi)LSTM scan: one HIP launch per timestep, forward and backward.

Wraps the lstm_scan.hip kernels in a single autograd.Function over the
WHOLE recurrence of up to two directions:
  - forward: the hoisted input projection as one library GEMM per
    direction (bias folded in), then T step launches; each launch does
    the recurrent small-M MFMA GEMM, the LSTM cell math and the padded
    state carry for every direction at once.
  - backward: T step launches (recurrent data-grad GEMM + gate backward,
    carries kept in fp32), then ALL weight gradients batched over time
    into whole-sequence library GEMMs (summing over t first is
    algebraically identical to per-step accumulation).

All buffers stay in natural time order: a reversed direction only walks
its time index backwards, so there are no flips, no per-step
.contiguous() and no stack. No host syncs and no data-dependent shapes:
the op is graph-capturable as a linear chain on one stream.

CPU tensors take a pure-torch implementation of the SAME algorithm,
including the hand-written backward (same equations as the kernels, not
autograd over the cell), so the derivation is checkable without a GPU.

Reference semantics: lingvo/core/lstm_frnn_layer.py LSTMFRNN over
rnn_cell.py:213 LSTMCellSimple (gate order cand, i, f, o).
"""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch

from lingvo_amd.ops import _loader


def _step_times(s: int, t_len: int, rev: bool) -> Tuple[int, int, int]:
  """Scan step s -> (t, t_prev, t_next) in natural time order."""
  if rev:
    t = t_len - 1 - s
    return t, t + 1, t - 1
  return s, s - 1, s + 1


def _cell_torch(g, c_prev, fgb, cap):
  """Torch twin of ops/hip/lstm_cell.h: the activations (cand, i, f, o) and
  the cell value before and after the clamp."""
  h = g.shape[-1] // 4
  cand = torch.tanh(g[:, :h])
  ig = torch.sigmoid(g[:, h:2 * h])
  fg = torch.sigmoid(g[:, 2 * h:3 * h] + fgb)
  og = torch.sigmoid(g[:, 3 * h:])
  craw = fg * c_prev + ig * cand
  cn = craw.clamp(-cap, cap) if cap > 0 else craw
  return cand, ig, fg, og, craw, cn


def _fwd_steps_torch(gates, c, m, pad, wm_rec, fgb, cap, revs):
  """Torch twin of lstm_scan_step_fwd, all steps. gates is updated in
  place to the full pre-activations."""
  dn, t_len = gates.shape[:2]
  for s in range(t_len):
    for d in range(dn):
      t, tp, _ = _step_times(s, t_len, revs[d])
      if s > 0:
        c_prev, m_prev = c[d, tp], m[d, tp]
        gates[d, t] += m_prev @ wm_rec[d]
      else:
        c_prev = torch.zeros_like(c[d, t])
        m_prev = c_prev
      _, _, _, og, _, cn = _cell_torch(gates[d, t], c_prev, fgb, cap)
      mn = og * torch.tanh(cn)
      p = pad[t].unsqueeze(-1)
      c[d, t] = cn * (1 - p) + c_prev * p
      m[d, t] = mn * (1 - p) + m_prev * p


def _bwd_steps_torch(gates, c, pad, wm_rec, dm_out, dc_out, dgates, fgb,
                     cap, revs):
  """Torch twin of lstm_scan_step_bwd, all steps (s descending)."""
  dn, t_len, b, g4 = gates.shape
  h = g4 // 4
  for d in range(dn):
    dc_carry = dm_pass = None
    for s in range(t_len - 1, -1, -1):
      t, tp, tn = _step_times(s, t_len, revs[d])
      p = pad[t].unsqueeze(-1)
      dm_tot = dm_out[d, t] if dm_out is not None else \
          torch.zeros(b, h, dtype=gates.dtype, device=gates.device)
      dc_tot = dc_out[d, t] if dc_out is not None else \
          torch.zeros(b, h, dtype=gates.dtype, device=gates.device)
      if s < t_len - 1:
        dm_tot = dm_tot + dgates[d, tn] @ wm_rec[d].t() + dm_pass
        dc_tot = dc_tot + dc_carry
      c_prev = c[d, tp] if s > 0 else torch.zeros_like(c[d, t])
      # c~ from this recomputation: the stored c[t] is post-blend.
      cand, ig, fg, og, craw, cn = _cell_torch(gates[d, t], c_prev, fgb, cap)
      tc = torch.tanh(cn)
      dmt = (1 - p) * dm_tot
      do_ = dmt * tc
      dc = (1 - p) * dc_tot + dmt * og * (1 - tc * tc)
      if cap > 0:
        dc = torch.where((craw > cap) | (craw < -cap),
                         torch.zeros_like(dc), dc)
      dgates[d, t, :, :h] = dc * ig * (1 - cand * cand)
      dgates[d, t, :, h:2 * h] = dc * cand * ig * (1 - ig)
      dgates[d, t, :, 2 * h:3 * h] = dc * c_prev * fg * (1 - fg)
      dgates[d, t, :, 3 * h:] = do_ * og * (1 - og)
      dc_carry = dc * fg + p * dc_tot
      dm_pass = p * dm_tot


class _LstmScanFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, pad, fgb, cap, revs, rows, *weights):
    # An output nobody differentiates arrives as None in backward (null
    # pointer to the kernel) instead of a zero-filled [D,T,B,H] tensor.
    ctx.set_materialize_grads(False)
    dn = len(revs)
    wms, bs = weights[:dn], weights[dn:]
    t_len, b, d_in = x.shape
    h = wms[0].shape[1] // 4
    on_gpu = x.is_cuda
    # Device path computes in bf16 (kernel contract); CPU keeps x's dtype.
    dt = torch.bfloat16 if on_gpu else x.dtype
    x2 = x.to(dt).reshape(t_len * b, d_in)
    pad_f = pad.to(torch.float32 if on_gpu else dt).contiguous()
    rev_mask = sum(1 << d for d in range(dn) if revs[d])

    gates = torch.empty(dn, t_len, b, 4 * h, dtype=dt, device=x.device)
    for d in range(dn):
      wx = wms[d][:d_in].to(dt)
      out = gates[d].view(t_len * b, 4 * h)
      if bs[d] is not None:
        torch.addmm(bs[d].to(dt), x2, wx, out=out)
      else:
        torch.mm(x2, wx, out=out)
    c = torch.empty(dn, t_len, b, h, dtype=dt, device=x.device)
    m = torch.empty_like(c)
    if on_gpu:
      ext = _loader.get_ext(required=True)
      wmt = torch.stack([w[d_in:].to(dt).t() for w in wms]).contiguous()
      ext.lstm_scan_fwd(gates, c, m, pad_f, wmt, rev_mask, fgb, cap, 0,
                        t_len, rows)
    else:
      _fwd_steps_torch(gates, c, m, pad_f, [w[d_in:].to(dt) for w in wms],
                       fgb, cap, revs)
    ctx.save_for_backward(x, pad_f, gates, c, m, *weights)
    ctx.cfg = (fgb, cap, tuple(revs), rev_mask, rows)
    return m, c

  @staticmethod
  def backward(ctx, dm, dc):
    x, pad_f, gates, c, m, *weights = ctx.saved_tensors
    fgb, cap, revs, rev_mask, rows = ctx.cfg
    dn = len(revs)
    wms, bs = weights[:dn], weights[dn:]
    t_len, b, d_in = x.shape
    h = c.shape[-1]
    dt = gates.dtype
    dev = gates.device
    n_in = 6 + 2 * dn
    if dm is None and dc is None:
      return (None,) * n_in
    need = ctx.needs_input_grad
    dm = None if dm is None else dm.to(dt).contiguous()
    dc = None if dc is None else dc.to(dt).contiguous()

    dgates = torch.empty_like(gates)
    if gates.is_cuda:
      ext = _loader.get_ext(required=True)
      wm_rec = torch.stack([w[d_in:].to(dt) for w in wms]).contiguous()
      dc_carry = torch.empty(dn, b, h, dtype=torch.float32, device=dev)
      dm_pass = torch.empty_like(dc_carry)
      ext.lstm_scan_bwd(gates, c, pad_f, wm_rec, dm, dc, dgates, dc_carry,
                        dm_pass, rev_mask, fgb, cap, 0, t_len, rows)
    else:
      _bwd_steps_torch(gates, c, pad_f, [w[d_in:].to(dt) for w in wms], dm,
                       dc, dgates, fgb, cap, revs)

    # Whole-sequence weight / input gradients.
    x2 = x.to(dt).reshape(t_len * b, d_in)
    zero_row = torch.zeros(1, b, h, dtype=dt, device=dev)
    dx2 = None
    dwms: List[torch.Tensor] = []
    dbs: List[Optional[torch.Tensor]] = []
    for d in range(dn):
      dg2 = dgates[d].view(t_len * b, 4 * h)
      # m shifted by one step in scan order, zero first row.
      m_shift = torch.cat([m[d, 1:], zero_row] if revs[d] else
                          [zero_row, m[d, :-1]])
      if need[6 + d]:
        dwm = torch.empty(d_in + h, 4 * h, dtype=dt, device=dev)
        torch.mm(x2.t(), dg2, out=dwm[:d_in])
        torch.mm(m_shift.view(t_len * b, h).t(), dg2, out=dwm[d_in:])
        dwms.append(dwm.to(wms[d].dtype))
      else:
        dwms.append(None)
      if bs[d] is not None and need[6 + dn + d]:
        acc_dt = torch.float32 if dt == torch.bfloat16 else dt
        dbs.append(dg2.sum(dim=0, dtype=acc_dt).to(bs[d].dtype))
      else:
        dbs.append(None)
      if need[0]:
        wxt = wms[d][:d_in].to(dt).t()
        dx2 = dg2 @ wxt if dx2 is None else dx2.addmm_(dg2, wxt)
    dx = None if dx2 is None else dx2.view(t_len, b, d_in).to(x.dtype)
    return (dx, None, None, None, None, None, *dwms, *dbs)


def lstm_scan(x: torch.Tensor, wm_list: Sequence[torch.Tensor],
              b_list: Sequence[Optional[torch.Tensor]], pad: torch.Tensor,
              forget_gate_bias: float = 0.0, cell_value_cap: float = 0.0,
              reverse_flags: Sequence[bool] = (False,),
              rows_per_block: int = 0):
  """Whole-sequence LSTM scan over D = len(wm_list) directions (1 or 2).

  x [T,B,Din]; wm_list[d] [(Din+H), 4H] (LSTMCellSimple.wm: input rows
  then recurrent rows); b_list[d] [4H] or None; pad [T,B] (1 = padded
  step: state carried through); reverse_flags[d]: scan right-to-left.
  cell_value_cap <= 0 disables the clamp. Zero initial state.
  rows_per_block: batch rows per workgroup of the step kernels (16, 32,
  64 or 128; 0 = kernel default; ignored on CPU).
  Returns (m [D,T,B,H], c [D,T,B,H]) in natural time order."""
  dn = len(wm_list)
  assert dn in (1, 2) and len(b_list) == dn and len(reverse_flags) == dn
  h4 = wm_list[0].shape[1]
  assert h4 % 4 == 0
  for w in wm_list:
    assert w.shape == wm_list[0].shape, 'directions must share Din and H'
    assert w.shape[0] == x.shape[-1] + h4 // 4
  assert rows_per_block in (0, 16, 32, 64, 128), rows_per_block
  if x.is_cuda:
    assert (h4 // 4) % 32 == 0, 'lstm_scan kernels need H % 32 == 0'
  return _LstmScanFn.apply(x, pad, float(forget_gate_bias),
                           float(cell_value_cap),
                           tuple(bool(r) for r in reverse_flags),
                           int(rows_per_block),
                           *wm_list, *b_list)
