"""lstm_gates_fwd / lstm_gates_bwd (ops/hip/lstm_gates.hip) called directly
against the fp64 cell on the exact bf16 input values, cap off and biting,
with run-to-run bit identity, canaries around every operand (the ops allocate
their outputs, so a store behind an output cannot be caught here), and the
host rejections of both ops."""

import functools

import pytest
import torch

from lstm_cell_ref import FGB, _BitingCap, _CellBwd, _CellFwd

gpu = pytest.mark.gpu

# One element, a row tail with H off the 16-column tile, and more than one
# 256-thread block with H across a column-tile boundary.
CASES = [(1, 16), (5, 24), (130, 96)]
NEAR_CAP = 1e-5  # |pre-clamp c| within NEAR_CAP * cap of cap: left out (bwd)


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _Bits(t):
  return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _SameBits(a, b):
  return a.shape == b.shape and a.dtype == b.dtype and \
      torch.equal(_Bits(a), _Bits(b))


@functools.lru_cache(maxsize=None)
def _Case(b, h):
  """bf16-exact inputs (CPU) and the biting cap of their fp64 cell."""
  g = torch.Generator().manual_seed(300 + 7 * b + h)
  bf = lambda *shape, scale=1.0: \
      (torch.randn(*shape, generator=g) * scale).bfloat16()
  case = dict(gates=bf(b, 4 * h), c0=bf(b, h, scale=2.0), dm=bf(b, h),
              dc=bf(b, h, scale=0.5))
  craw, _, _ = _CellFwd(case['gates'].double(), case['c0'].double(), 0.0)
  case['craw'] = craw
  case['cap'], case['share'] = _BitingCap(craw)
  return case


def _Keep(case, cap):
  """Cells of the backward comparison: all but those on the cap."""
  if cap <= 0:
    return torch.ones_like(case['craw'], dtype=torch.bool)
  return (case['craw'].abs() - cap).abs() > NEAR_CAP * cap


@pytest.mark.parametrize('b,h', CASES)
def test_lstm_gates_cases_leave_out_at_most_one_percent(b, h):
  """From the fp64 reference alone: the biting cap clamps a real share of
  the cells and at most 1% of them sit on it."""
  case = _Case(b, h)
  assert 0.05 <= case['share'] <= 0.95, case['share']
  assert float((~_Keep(case, case['cap'])).double().mean()) <= 0.01


def _Row1(t, fill=-300.0):
  """t as row 1 of a canary-filled [3, ...] stack on the GPU, and a copy of
  the stack."""
  st = torch.full((3,) + tuple(t.shape), fill, dtype=t.dtype, device='cuda')
  st[1] = t
  return st, st.clone()


@gpu
@pytest.mark.parametrize('biting', [False, True])
@pytest.mark.parametrize('b,h', CASES)
def test_lstm_gates_fwd_matches_fp64(b, h, biting):
  """c within 2^-8 |ref| + 1e-6 (one bf16 rounding of an fp32 result); m
  within 2^-8 |ref| + 2^-8 (1 - tanh(c)^2) |c| + 1e-6. Two runs give the same
  bits; the operand stacks (canary rows included) are not written. The op
  allocates its outputs, so the canaries surround the operands."""
  ext = _Ext()
  case = _Case(b, h)
  cap = case['cap'] if biting else 0.0
  _, c_ref, m_ref = _CellFwd(case['gates'].double(), case['c0'].double(), cap)
  g_st, g_before = _Row1(case['gates'])
  c_st, c_before = _Row1(case['c0'])
  c1, m1 = ext.lstm_gates_fwd(g_st[1], c_st[1], FGB, cap)
  c1b, m1b = ext.lstm_gates_fwd(g_st[1], c_st[1], FGB, cap)
  torch.cuda.synchronize()
  assert _SameBits(g_st, g_before) and _SameBits(c_st, c_before)
  assert c1.shape == (b, h) and c1.dtype == torch.bfloat16
  assert _SameBits(c1, c1b) and _SameBits(m1, m1b)
  c_bound = 2.0 ** -8 * c_ref.abs() + 1e-6
  m_bound = 2.0 ** -8 * m_ref.abs() + \
      2.0 ** -8 * (1 - torch.tanh(c_ref) ** 2) * c_ref.abs() + 1e-6
  r_c = float(((c1.double().cpu() - c_ref).abs() / c_bound).max())
  r_m = float(((m1.double().cpu() - m_ref).abs() / m_bound).max())
  print(f'lstm_gates_fwd B={b} H={h} cap={cap:.4g}: c err/bound {r_c:.3f} '
        f'm err/bound {r_m:.3f}')
  assert r_c <= 1.0 and r_m <= 1.0, (r_c, r_m)
  if biting:
    assert float((c_ref.abs() >= cap).double().mean()) == case['share']


def _Fp32Yardstick(gates, c0, c1, dm, dc, cap):
  """lstm_gates_bwd's formulas as fp32 torch ops on the stored bf16 gates,
  c0 and c1 (tanh of the stored c1, clamp test on the recomputed c)."""
  h = c0.shape[-1]
  g0, g1, g2, g3 = gates.float().split([h, h, h, h], dim=-1)
  cand, ig, fg, og = (torch.tanh(g0), torch.sigmoid(g1),
                      torch.sigmoid(g2 + FGB), torch.sigmoid(g3))
  c0f, dmf = c0.float(), dm.float()
  tc = torch.tanh(c1.float())
  dcv = dmf * og * (1 - tc * tc)
  if dc is not None:
    dcv = dc.float() + dcv
  if cap > 0:
    craw = fg * c0f + ig * cand
    dcv = torch.where(craw.abs() > cap, torch.zeros_like(dcv), dcv)
  dg = torch.cat([dcv * ig * (1 - cand * cand), dcv * cand * ig * (1 - ig),
                  dcv * c0f * fg * (1 - fg), dmf * tc * og * (1 - og)], -1)
  return dg, dcv * fg


@gpu
@pytest.mark.parametrize('with_dc', [False, True])
@pytest.mark.parametrize('biting', [False, True])
@pytest.mark.parametrize('b,h', CASES)
def test_lstm_gates_bwd_matches_fp64(b, h, biting, with_dc):
  """dgates and dc0 per element within 2 err_yardstick + 2^-8 |ref| + 1e-6
  of the fp64 backward, the yardstick being the same formulas in fp32 torch
  ops on the same stored gates, c0 and c1 (the kernel takes tanh of the
  stored bf16 c1, so its error is measured, not derived). Cells on the cap
  are left out. Two runs give the same bits; no operand stack is written."""
  ext = _Ext()
  case = _Case(b, h)
  cap = case['cap'] if biting else 0.0
  dc_in = case['dc'].double() if with_dc else torch.zeros(b, h).double()
  dg_ref, dc_ref, _ = _CellBwd(case['gates'].double(), case['c0'].double(),
                               case['dm'].double(), dc_in, cap)
  stacks = [_Row1(case[n]) for n in ('gates', 'c0', 'dm', 'dc')]
  (g_st, _), (c0_st, _), (dm_st, _), (dc_st, _) = stacks
  c1 = ext.lstm_gates_fwd(g_st[1], c0_st[1], FGB, cap)[0]
  c1_st, c1_before = _Row1(c1)
  stacks.append((c1_st, c1_before))
  dc_arg = dc_st[1] if with_dc else None
  run = lambda: ext.lstm_gates_bwd(g_st[1], c0_st[1], c1_st[1], dm_st[1],
                                   dc_arg, FGB, cap)
  dg, dc0 = run()
  dg_b, dc0_b = run()
  yard = _Fp32Yardstick(g_st[1], c0_st[1], c1_st[1], dm_st[1], dc_arg, cap)
  torch.cuda.synchronize()
  for st, before in stacks:
    assert _SameBits(st, before)
  assert dg.shape == (b, 4 * h) and dc0.shape == (b, h)
  assert dg.dtype == dc0.dtype == torch.bfloat16
  assert _SameBits(dg, dg_b) and _SameBits(dc0, dc0_b)
  keep = _Keep(case, cap)
  for name, got, y, ref, mask in (
      ('dgates', dg, yard[0], dg_ref, keep.repeat(1, 4)),
      ('dc0', dc0, yard[1], dc_ref, keep)):
    err_y = (y.double().cpu() - ref).abs()
    bound = 2 * err_y + 2.0 ** -8 * ref.abs() + 1e-6
    ratio = float((((got.double().cpu() - ref).abs() / bound) * mask).max())
    print(f'lstm_gates_bwd B={b} H={h} cap={cap:.4g} dc1={with_dc} {name}: '
          f'err/bound {ratio:.3f} yardstick max err '
          f'{float((err_y * mask).max()):.3g}')
    assert ratio <= 1.0, (name, ratio)


# ---------------------------------------------------------------------------
# Host rejections: each raises and writes no operand
# ---------------------------------------------------------------------------

def _Mk(*shape, dtype=torch.bfloat16, device='cuda'):
  return torch.full(shape, 1.0, dtype=dtype, device=device)


def _Args(b=4, h=32):
  return dict(gates=_Mk(b, 4 * h), c0=_Mk(b, h), c1=_Mk(b, h), dm1=_Mk(b, h),
              dc1=_Mk(b, h))


def _RejectCases():
  return {
      'c0_fp32': lambda: dict(c0=_Mk(4, 32, dtype=torch.float32)),
      'dm1_strided': lambda: dict(dm1=_Mk(4, 64)[:, ::2]),
      'c1_wrong_shape': lambda: dict(c1=_Mk(3, 32)),
      'gates_3h_columns': lambda: dict(gates=_Mk(4, 96)),
      'gates_on_cpu': lambda: dict(gates=_Mk(4, 128, device='cpu')),
      'dc1_on_cpu': lambda: dict(dc1=_Mk(4, 32, device='cpu')),
      'dc1_fp32': lambda: dict(dc1=_Mk(4, 32, dtype=torch.float32)),
  }


@gpu
@pytest.mark.parametrize('name', sorted(_RejectCases()))
def test_lstm_gates_rejects(name):
  """lstm_gates_bwd raises for every case, lstm_gates_fwd for those that
  touch its two operands. The ops allocate their outputs, so a launch before
  the raise could not be seen here: the test proves that the call raises
  (the checks precede the allocations and the launch in the wrappers) and
  that the operands keep their bits."""
  ext = _Ext()
  args = _Args()
  changed = _RejectCases()[name]()
  args.update(changed)
  before = {n: t.clone() for n, t in args.items()}
  with pytest.raises(RuntimeError):
    ext.lstm_gates_bwd(args['gates'], args['c0'], args['c1'], args['dm1'],
                       args['dc1'], FGB, 0.0)
  if set(changed) <= {'gates', 'c0'}:
    with pytest.raises(RuntimeError):
      ext.lstm_gates_fwd(args['gates'], args['c0'], FGB, 0.0)
  torch.cuda.synchronize()
  for n, t in args.items():
    assert _SameBits(t.contiguous(), before[n].contiguous()), n
