"""fp64 LSTM cell shared by the tests of the recurrence kernels (plain
helpers, no fixtures): the cell of ops/hip/lstm_cell.h, gate order cand, i,
f, o, with the forget-gate bias FGB."""

import torch

FGB = 1.0


def _CellFwd(gates, c_prev, cap):
  """Returns the pre-clamp c, the clamped c and m."""
  h = gates.shape[-1] // 4
  cand, i_g, f_g, o_g = gates.split([h, h, h, h], dim=-1)
  craw = torch.sigmoid(f_g + FGB) * c_prev + \
      torch.sigmoid(i_g) * torch.tanh(cand)
  c = torch.clamp(craw, -cap, cap) if cap > 0 else craw
  return craw, c, torch.sigmoid(o_g) * torch.tanh(c)


def _CellBwd(gates, c_prev, dm, dc_in, cap):
  """fp64 backward of _CellFwd: dgates [B,4H], dc_prev [B,H], pre-clamp c."""
  h = gates.shape[-1] // 4
  cand, i_g, f_g, o_g = gates.split([h, h, h, h], dim=-1)
  cand, ig, fg, og = (torch.tanh(cand), torch.sigmoid(i_g),
                      torch.sigmoid(f_g + FGB), torch.sigmoid(o_g))
  craw = fg * c_prev + ig * cand
  c = torch.clamp(craw, -cap, cap) if cap > 0 else craw
  tc = torch.tanh(c)
  dc = dc_in + dm * og * (1 - tc * tc)
  if cap > 0:
    dc = torch.where(craw.abs() > cap, torch.zeros_like(dc), dc)
  dg = torch.cat([dc * ig * (1 - cand * cand), dc * cand * ig * (1 - ig),
                  dc * c_prev * fg * (1 - fg), dm * tc * og * (1 - og)], -1)
  return dg, dc * fg, craw


def _BitingCap(craw):
  """A cap that clamps about half of the cells: the midpoint of the two
  middle |c|, so that no cell sits on the cap itself."""
  v = craw.abs().flatten().sort().values
  cap = float(v[v.numel() // 2 - 1] + v[v.numel() // 2]) / 2
  share = float((craw.abs() > cap).double().mean())
  assert cap > 0
  return cap, share
