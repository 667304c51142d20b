"""The 'fused' step route of the LAS decoder (ops/hip/las_step.hip):
las_step_fwd and las_cell_bwd called directly against fp64 references on the
exact bf16 input values, their host rejections, the whole recurrence with
step_route fused and split against an fp64 recurrence, and a hipGraph
capture of a small AsrModel step on the fused route."""

import functools
import math

import pytest
import torch

from lstm_cell_ref import FGB, _BitingCap, _CellBwd, _CellFwd

gpu = pytest.mark.gpu

BF16_ULP = 2.0 ** -7  # spacing of bf16 values relative to their magnitude
ROWS = (32, 64, 128)  # rows per workgroup of every compiled MT (2, 4, 8)
# B crosses one 16-row m-tile, the 32-row block and the 128-row block; H is
# two column tiles and a count that is no power of two.
BS = (1, 17, 33, 130)
HS = (32, 96)


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _Gen(seed):
  return torch.Generator().manual_seed(seed)


def _Bf16(*shape, g, scale=1.0):
  """Random values that are exact in bf16, as a CPU bf16 tensor."""
  return (torch.randn(*shape, generator=g) * scale).bfloat16()


def _Bits(t):
  return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _SameBits(a, b):
  return torch.equal(_Bits(a), _Bits(b))


def _Stack(b, n, dtype=torch.bfloat16, fill=-300.0):
  """A canary-filled [3, b, n] stack on the GPU and a copy of it."""
  st = torch.full((3, b, n), fill, dtype=dtype, device='cuda')
  return st, st.clone()


def _OnlyRow1Changed(stack, before):
  return _SameBits(stack[[0, 2]], before[[0, 2]])


# ---------------------------------------------------------------------------
# las_step_fwd
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _FwdCase(b, h, k1, k2, pre_is_matrix):
  g = _Gen(1000 * b + 10 * h + k1 + 3 * k2 + int(pre_is_matrix))
  case = dict(
      a1=_Bf16(b, k1, g=g) if k1 else None,
      a2=_Bf16(b, k2, g=g) if k2 else None,
      # 8 spare columns: the K ranges are a prefix of the weight rows.
      wt=_Bf16(4 * h, k1 + k2 + 8, g=g, scale=0.15),
      pre=_Bf16(b, 4 * h, g=g) if pre_is_matrix else _Bf16(4 * h, g=g),
      c_prev=_Bf16(b, h, g=g) if k2 else None)
  ref = case['pre'].double().expand(b, 4 * h).clone()
  mag = ref.abs()
  col = 0
  for a in (case['a1'], case['a2']):
    if a is not None:
      w = case['wt'][:, col:col + a.shape[1]].double()
      ref += a.double() @ w.t()
      mag += a.double().abs() @ w.abs().t()
      col += a.shape[1]
  case.update(gates=ref, mag=mag)
  return case


def _KPairs(h):
  return [(64, h), (32, h), (h, 0), (0, 0)]


@gpu
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('h', HS)
@pytest.mark.parametrize('b', BS)
def test_las_step_fwd_matches_fp64(b, h, rows):
  """gates within 2^-7 |ref| + 2^-20 sum|a||w|+|pre| of fp64 (smallm_gemm's
  bound); c and m within 2^-7 |ref| + 2^-20 max|ref| of the fp64 cell on the
  kernel's own stored gates; rows 0 and 2 of the stacks untouched. Every K
  pair, pre as matrix and vector, cap off and biting."""
  ext = _Ext()
  worst = 0.0
  for k1, k2 in _KPairs(h):
    for pre_is_matrix in (True, False):
      case = _FwdCase(b, h, k1, k2, pre_is_matrix)
      c_prev64 = case['c_prev'].double() if k2 else torch.zeros(b, h).double()
      craw, _, _ = _CellFwd(case['gates'], c_prev64, 0.0)
      cap_bite, share = _BitingCap(craw)
      assert 0.05 <= share <= 0.95, share
      dev = lambda t: None if t is None else t.cuda()
      for cap in (0.0, cap_bite):
        g_st, g_before = _Stack(b, 4 * h)
        c_st, c_before = _Stack(b, h)
        m_st, m_before = _Stack(b, h)
        ext.las_step_fwd(dev(case['a1']), dev(case['a2']), case['wt'].cuda(),
                         case['pre'].cuda(), dev(case['c_prev']), g_st[1],
                         c_st[1], m_st[1], FGB, cap, rows)
        torch.cuda.synchronize()
        tag = (f'las_step_fwd B={b} H={h} K=({k1},{k2}) rows={rows} '
               f'pre={"matrix" if pre_is_matrix else "vector"} cap={cap:.3g}')
        for st, before in ((g_st, g_before), (c_st, c_before),
                           (m_st, m_before)):
          assert _OnlyRow1Changed(st, before), tag
        got_g = g_st[1].double().cpu()
        bound = BF16_ULP * case['gates'].abs() + 2.0 ** -20 * case['mag']
        ratio = float(((got_g - case['gates']).abs() /
                       bound.clamp_min(1e-300)).max())
        assert ratio <= 1.0, (tag, 'gates', ratio)
        _, c_ref, m_ref = _CellFwd(got_g, c_prev64, cap)
        for name, st, ref in (('c', c_st, c_ref), ('m', m_st, m_ref)):
          bnd = BF16_ULP * ref.abs() + 2.0 ** -20 * float(ref.abs().max())
          r = float(((st[1].double().cpu() - ref).abs() / bnd).max())
          worst = max(worst, r)
          assert r <= 1.0, (tag, name, r)
        if cap > 0:
          clamped = float((c_ref.abs() >= cap).double().mean())
          assert 0.04 <= clamped <= 0.96, (tag, clamped)
  print(f'las_step_fwd B={b} H={h} rows={rows}: worst c/m err/bound '
        f'{worst:.3f}')


# ---------------------------------------------------------------------------
# las_cell_bwd
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _BwdCase(b, h, two_halves):
  """Inputs of one backward stage. two_halves: the layer-1 -> layer-0
  hand-over (K = 4H, N = 2H, strided bf16 addend, pass-through half); else
  the layer-1 stage (K = 64, N = H, bf16 and fp32 addends)."""
  g = _Gen(7000 + 100 * b + h + int(two_halves))
  k = 4 * h if two_halves else 64
  n = 2 * h if two_halves else h
  wide = _Bf16(b, 64 + h, g=g, scale=0.5)   # add_b as dcm[:, src:]
  case = dict(
      a=_Bf16(b, k, g=g, scale=0.5), wt=_Bf16(n, k, g=g, scale=0.15),
      wide=wide, add_b=wide[:, 64:], add_f=_Bf16(b, h, g=g, scale=0.5),
      gates=_Bf16(b, 4 * h, g=g), c_prev=_Bf16(b, h, g=g),
      dc=_Bf16(b, h, g=g, scale=0.5), k=k, n=n)
  case['gemm'] = case['a'].double() @ case['wt'].double().t()
  return case


def _RunBwdStages(ext, case, carry, cap, rows, two_halves):
  """The fused stage and the split sequence it replaces on the same inputs.
  Returns (fused, split) dicts of dgates, dc and, for two_halves, pass."""
  b, h = case['c_prev'].shape
  gates, c_prev = case['gates'].cuda(), case['c_prev'].cuda()
  a, wt = case['a'].cuda(), case['wt'].cuda()
  add_b = case['wide'].cuda()[:, 64:]
  add_f = case['add_f'].float().cuda()
  # Without incoming carries: the bf16 addend stays for the layer-1 stage
  # (it is the output gradient there) and goes for the hand-over.
  use_b = carry or not two_halves
  use_f = carry and not two_halves

  dg_st, dg_before = _Stack(b, 4 * h)
  dc_f = torch.full((b, h), 7.0, device='cuda')
  if carry:
    dc_f.copy_(case['dc'].float())
  pass_f = torch.full((b, h), 7.0, device='cuda') if two_halves else None
  ext.las_cell_bwd(a, wt, add_b if use_b else None, add_f if use_f else None,
                   gates, c_prev, dc_f, carry, dg_st[1], pass_f, FGB, cap,
                   rows)
  torch.cuda.synchronize()
  assert _OnlyRow1Changed(dg_st, dg_before)
  fused = dict(dgates=dg_st[1], dc=dc_f)

  # Split: smallm_gemm (+ add) + lstm_gates_bwd, bf16 between launches.
  c1 = ext.lstm_gates_fwd(gates, c_prev, FGB, cap)[0]
  dc_b = case['dc'].cuda() if carry else None
  if two_halves:
    dmm = torch.empty(b, 2 * h, dtype=torch.bfloat16, device='cuda')
    ext.smallm_gemm(a, wt, None, dmm, case['k'], 0, 1.0, 0)
    dm = dmm[:, :h].contiguous()
    if use_b:
      dm = (dm + add_b).contiguous()
    fused['pass'] = pass_f
    split_pass = dmm[:, h:]
  else:
    pre = add_b.contiguous()
    if use_f:
      pre = pre + case['add_f'].cuda()
    dm = torch.empty(b, h, dtype=torch.bfloat16, device='cuda')
    ext.smallm_gemm(a, wt, pre, dm, case['k'], 0, 1.0, 2)
  dg, dc0 = ext.lstm_gates_bwd(gates, c_prev, c1, dm, dc_b, FGB, cap)
  split = dict(dgates=dg, dc=dc0)
  if two_halves:
    split['pass'] = split_pass
  to64 = lambda d: {n: v.double().cpu() for n, v in d.items()}
  return to64(fused), to64(split), use_b, use_f


@gpu
@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('two_halves', [False, True])
@pytest.mark.parametrize('h', HS)
@pytest.mark.parametrize('b', BS)
def test_las_cell_bwd_matches_fp64(b, h, two_halves, rows):
  """Every output within 2 x the split sequence's error plus one bf16 ulp
  (bf16 outputs) or 2^-20 (fp32 outputs) of max|ref|, first and later
  steps, cap off and biting. Cells whose fp64 pre-clamp |c| lies within
  1e-4 of cap are left out of dgates and of dc, which carries the same
  clamp mask; they are at most 1% of the cells."""
  ext = _Ext()
  case = _BwdCase(b, h, two_halves)
  gates64, c_prev64 = case['gates'].double(), case['c_prev'].double()
  craw, _, _ = _CellFwd(gates64, c_prev64, 0.0)
  cap_bite, share = _BitingCap(craw)
  assert 0.05 <= share <= 0.95, share
  for carry in (False, True):
    for cap in (0.0, cap_bite):
      fused, split, use_b, use_f = _RunBwdStages(ext, case, carry, cap, rows,
                                                 two_halves)
      dm = case['gemm'][:, :h].clone()
      if use_b:
        dm += case['add_b'].double()
      if use_f:
        dm += case['add_f'].double()
      dc_in = case['dc'].double() if carry else torch.zeros(b, h).double()
      dg_ref, dc_ref, _ = _CellBwd(gates64, c_prev64, dm, dc_in, cap)
      want = dict(dgates=dg_ref, dc=dc_ref)
      if two_halves:
        want['pass'] = case['gemm'][:, h:]
      keep = torch.ones(b, h, dtype=torch.bool)
      if cap > 0:
        keep = (craw.abs() - cap).abs() > 1e-4
        assert float((~keep).double().mean()) <= 0.01
      for name, ref in want.items():
        mask = keep.repeat(1, 4) if name == 'dgates' else \
            keep if name == 'dc' else torch.ones_like(ref, dtype=torch.bool)
        e_fused = float(((fused[name] - ref).abs() * mask).max())
        e_split = float(((split[name] - ref).abs() * mask).max())
        floor = (BF16_ULP if name == 'dgates' else 2.0 ** -20) * \
            float(ref.abs().max())
        print(f'las_cell_bwd B={b} H={h} N={case["n"]} rows={rows} '
              f'carry={carry} cap={cap:.3g} {name}: fused {e_fused:.4g} '
              f'split {e_split:.4g} bound {2 * e_split + floor:.4g}')
        assert e_fused <= 2 * e_split + floor, (name, carry, cap)


# ---------------------------------------------------------------------------
# Host rejections: each raises and leaves pre-filled outputs unchanged
# ---------------------------------------------------------------------------

def _Mk(*shape, dtype=torch.bfloat16, fill=1.0):
  return torch.full(shape, fill, dtype=dtype, device='cuda')


def _FwdArgs(b=4, h=32, k=32):
  return dict(a1=_Mk(b, k), a2=_Mk(b, k), wt=_Mk(4 * h, 2 * k),
              pre=_Mk(4 * h), c_prev=_Mk(b, h), gates=_Mk(b, 4 * h, fill=5.0),
              c_out=_Mk(b, h, fill=5.0), m_out=_Mk(b, h, fill=5.0), rows=0)


def _FwdRejectCases():
  f32 = torch.float32
  return {
      'a1_fp32': lambda: dict(a1=_Mk(4, 32, dtype=f32)),
      'wt_fp32': lambda: dict(wt=_Mk(128, 64, dtype=f32)),
      'pre_fp32': lambda: dict(pre=_Mk(128, dtype=f32)),
      'gates_fp32': lambda: dict(gates=_Mk(4, 128, dtype=f32, fill=5.0)),
      'h_not_multiple_of_16': lambda: dict(
          wt=_Mk(96, 64), pre=_Mk(96), c_prev=_Mk(4, 24),
          gates=_Mk(4, 96, fill=5.0), c_out=_Mk(4, 24, fill=5.0),
          m_out=_Mk(4, 24, fill=5.0)),
      'k1_not_multiple_of_32': lambda: dict(a1=_Mk(4, 48), wt=_Mk(128, 80)),
      'k2_not_multiple_of_32': lambda: dict(a2=_Mk(4, 16), wt=_Mk(128, 48)),
      'a1_misaligned': lambda: dict(a1=_Mk(4, 40)[:, 4:36]),
      'a2_row_stride_not_multiple_of_8': lambda: dict(a2=_Mk(4, 36)[:, :32]),
      'a1_column_stride_2': lambda: dict(a1=_Mk(4, 64)[:, ::2]),
      'wt_too_narrow': lambda: dict(wt=_Mk(128, 56)),
      'a2_fewer_rows': lambda: dict(a2=_Mk(3, 32)),
      'c_prev_fewer_rows': lambda: dict(c_prev=_Mk(3, 32)),
      'c_out_fewer_rows': lambda: dict(c_out=_Mk(3, 32, fill=5.0)),
      'm_out_more_rows': lambda: dict(m_out=_Mk(5, 32, fill=5.0)),
      'pre_matrix_fewer_rows': lambda: dict(pre=_Mk(3, 128)),
      'gates_not_contiguous': lambda: dict(
          gates=_Mk(4, 256, fill=5.0)[:, ::2]),
      'rows_16': lambda: dict(rows=16),
  }


@gpu
@pytest.mark.parametrize('name', sorted(_FwdRejectCases()))
def test_las_step_fwd_rejects(name):
  ext = _Ext()
  args = _FwdArgs()
  args.update(_FwdRejectCases()[name]())
  outs = [args['gates'], args['c_out'], args['m_out']]
  before = [t.clone() for t in outs]
  with pytest.raises(RuntimeError):
    ext.las_step_fwd(args['a1'], args['a2'], args['wt'], args['pre'],
                     args['c_prev'], args['gates'], args['c_out'],
                     args['m_out'], FGB, 0.0, args['rows'])
  torch.cuda.synchronize()
  for t, t0 in zip(outs, before):
    assert _SameBits(t.contiguous(), t0.contiguous())


def _BwdArgs(b=4, h=32, k=32):
  f32 = torch.float32
  return dict(a=_Mk(b, k), wt=_Mk(2 * h, k), add_b=_Mk(b, h),
              add_f=None, gates=_Mk(b, 4 * h), c_prev=_Mk(b, h),
              dc_carry=_Mk(b, h, dtype=f32, fill=5.0),
              dgates=_Mk(b, 4 * h, fill=5.0),
              pass_out=_Mk(b, h, dtype=f32, fill=5.0), rows=0)


def _BwdRejectCases():
  f32 = torch.float32
  return {
      'a_fp32': lambda: dict(a=_Mk(4, 32, dtype=f32)),
      'dc_carry_bf16': lambda: dict(dc_carry=_Mk(4, 32, fill=5.0)),
      'pass_out_bf16': lambda: dict(pass_out=_Mk(4, 32, fill=5.0)),
      'add_f_bf16': lambda: dict(add_f=_Mk(4, 32)),
      'h_not_multiple_of_16': lambda: dict(
          wt=_Mk(48, 32), add_b=_Mk(4, 24), gates=_Mk(4, 96),
          c_prev=_Mk(4, 24), dc_carry=_Mk(4, 24, dtype=f32, fill=5.0),
          dgates=_Mk(4, 96, fill=5.0),
          pass_out=_Mk(4, 24, dtype=f32, fill=5.0)),
      'k_not_multiple_of_32': lambda: dict(a=_Mk(4, 48), wt=_Mk(64, 48)),
      'a_misaligned': lambda: dict(a=_Mk(4, 40)[:, 4:36]),
      'a_column_stride_2': lambda: dict(a=_Mk(4, 64)[:, ::2]),
      'add_b_column_stride_2': lambda: dict(add_b=_Mk(4, 64)[:, ::2]),
      'wt_rows_not_2h_with_pass_out': lambda: dict(wt=_Mk(32, 32)),
      'wt_rows_not_h_without_pass_out': lambda: dict(pass_out=None),
      'dgates_fewer_rows': lambda: dict(dgates=_Mk(3, 128, fill=5.0)),
      'c_prev_fewer_rows': lambda: dict(c_prev=_Mk(3, 32)),
      'pass_out_more_rows': lambda: dict(
          pass_out=_Mk(5, 32, dtype=f32, fill=5.0)),
      'rows_256': lambda: dict(rows=256),
  }


@gpu
@pytest.mark.parametrize('name', sorted(_BwdRejectCases()))
def test_las_cell_bwd_rejects(name):
  ext = _Ext()
  args = _BwdArgs()
  args.update(_BwdRejectCases()[name]())
  outs = [t for t in (args['dc_carry'], args['dgates'], args['pass_out'])
          if t is not None]
  before = [t.clone() for t in outs]
  with pytest.raises(RuntimeError):
    ext.las_cell_bwd(args['a'], args['wt'], args['add_b'], args['add_f'],
                     args['gates'], args['c_prev'], args['dc_carry'], True,
                     args['dgates'], args['pass_out'], FGB, 0.0, args['rows'])
  torch.cuda.synchronize()
  for t, t0 in zip(outs, before):
    assert _SameBits(t, t0)


@gpu
def test_smallm_gemm_takes_a_column_slice_of_a_wider_matrix():
  """a with a row stride gives the bits of the same call on a dense copy;
  a slice that starts off a 16-byte boundary raises."""
  ext = _Ext()
  g = _Gen(5)
  wide = _Bf16(37, 96, g=g).cuda()
  wt = _Bf16(24, 64, g=g, scale=0.2).cuda()
  out_v, out_c = _Mk(37, 24, fill=5.0), _Mk(37, 24, fill=5.0)
  ext.smallm_gemm(wide[:, 32:], wt, None, out_v, 64, 0, 1.0, 0)
  ext.smallm_gemm(wide[:, 32:].contiguous(), wt, None, out_c, 64, 0, 1.0, 0)
  assert _SameBits(out_v, out_c)
  before = out_v.clone()
  with pytest.raises(RuntimeError):
    ext.smallm_gemm(wide[:, 4:68], wt, None, out_v, 64, 0, 1.0, 0)
  torch.cuda.synchronize()
  assert _SameBits(out_v, before)


# ---------------------------------------------------------------------------
# Whole recurrence against fp64, both step routes
# ---------------------------------------------------------------------------

def _AttendPaddings(b, s):
  """Row 0 padded from S/2 on, row 1 fully padded, the last row with one
  padded step in the middle (as in test_las_decoder_deferred_gpu.py)."""
  pad = torch.zeros(b, s)
  pad[0, max(s // 2, 1):] = 1.0
  if b >= 3:
    pad[b - 1, s // 2] = 1.0
  elif s >= 4:
    pad[0, s // 4] = 1.0
  if b >= 2:
    pad[1, :] = 1.0
  return pad


def _RefRecurrence(emb_gates, w_cm0, b1, wm1, wq, enc, pad, fgb, cap):
  """decoder_recurrence's docstring as plain torch ops in the dtype of its
  inputs (as in test_las_decoder_deferred_gpu.py)."""
  b, l, g4 = emb_gates.shape
  h = g4 // 4
  src = wq.shape[1]

  def Cell(gates, c_prev):
    cand, i_g, f_g, o_g = gates.split([h, h, h, h], dim=-1)
    c = torch.sigmoid(f_g + fgb) * c_prev + \
        torch.sigmoid(i_g) * torch.tanh(cand)
    c = torch.clamp(c, -cap, cap)
    return c, torch.sigmoid(o_g) * torch.tanh(c)

  zeros = lambda n: torch.zeros(b, n, dtype=enc.dtype, device=enc.device)
  c0, m0, c1, m1, ctx = zeros(h), zeros(h), zeros(h), zeros(h), zeros(src)
  outs = []
  for t in range(l):
    c0, m0 = Cell(emb_gates[:, t] + torch.cat([ctx, m0], -1) @ w_cm0, c0)
    c1, m1 = Cell(b1 + torch.cat([m0, m1], -1) @ wm1, c1)
    q = m1 @ wq
    logits = torch.einsum('bd,bsd->bs', q, enc) / math.sqrt(src)
    probs = torch.softmax(logits - 1e30 * pad.to(logits.dtype), dim=-1)
    ctx = torch.einsum('bs,bsd->bd', probs, enc)
    outs.append(torch.cat([m1, ctx], -1))
  return torch.stack(outs, dim=1)


REC_NAMES = ('emb_gates', 'w_cm0', 'b1', 'wm1', 'wq', 'enc')


def _RunRecurrence(fn, inputs, pad, w, device, dtype):
  leaves = {n: inputs[n].to(device, dtype, copy=True).requires_grad_(True)
            for n in REC_NAMES}
  out = fn(*[leaves[n] for n in REC_NAMES], pad.to(device))
  (out.double() * w.to(device)).sum().backward()
  res = {'out': out.detach()}
  res.update({n: leaves[n].grad for n in REC_NAMES})
  return {n: v.double().cpu() for n, v in res.items()}


@gpu
# The shapes of the deferred-route test, H = 96 and a single step.
@pytest.mark.parametrize('b,l,s,h,src', [(3, 4, 21, 32, 64),
                                         (130, 2, 5, 32, 32),
                                         (2, 3, 40, 32, 64),
                                         (5, 3, 7, 96, 32),
                                         (2, 1, 5, 32, 32)])
def test_decoder_recurrence_step_routes_match_fp64(b, l, s, h, src):
  """Output and every gradient of the fused route against the fp64
  recurrence: err <= 2 err_bf16_eager + 2^-8 max|ref| and
  err <= 2 err_split + the same floor; 'auto' is 'fused' here, and two
  fused runs give the same bits."""
  from lingvo_amd.ops import las_decoder
  fgb, cap = 1.0, 10.0
  g = _Gen(40 + b)
  bf = lambda *shape, scale=1.0: _Bf16(*shape, g=g, scale=scale).double()
  inputs = dict(emb_gates=bf(b, l, 4 * h), w_cm0=bf(src + h, 4 * h, scale=0.2),
                b1=bf(4 * h, scale=0.5), wm1=bf(2 * h, 4 * h, scale=0.2),
                wq=bf(h, src, scale=0.3), enc=bf(b, s, src))
  pad = _AttendPaddings(b, s)
  w = torch.randn(b, l, h + src, generator=g).double()

  ref_fn = functools.partial(_RefRecurrence, fgb=fgb, cap=cap)

  def Route(step_route):
    return lambda eg, w_cm0, b1, wm1, wq, enc, pad: \
        las_decoder.decoder_recurrence(eg, w_cm0, b1, wm1, wq, enc, pad, fgb,
                                       cap, src, step_route=step_route)

  run = lambda fn: _RunRecurrence(fn, inputs, pad, w, 'cuda', torch.bfloat16)
  want = _RunRecurrence(ref_fn, inputs, pad, w, 'cpu', torch.float64)
  eager = run(ref_fn)
  split = run(Route('split'))
  fused = run(Route('fused'))
  again = run(Route('fused'))
  auto = run(Route('auto'))

  failed = []
  for n in ('out',) + REC_NAMES:
    assert fused[n].shape == want[n].shape, n
    assert torch.equal(again[n], fused[n]), n
    assert torch.equal(auto[n], fused[n]), n
    ref_max = float(want[n].abs().max())
    # A single step has no previous state: its w_cm0 gradient is zero, and
    # the bounds below then ask for an exact zero.
    assert ref_max > 0 or (l == 1 and n == 'w_cm0'), n
    e_fused = float((fused[n] - want[n]).abs().max())
    e_split = float((split[n] - want[n]).abs().max())
    e_eager = float((eager[n] - want[n]).abs().max())
    floor = 2.0 ** -8 * ref_max
    print(f'decoder_recurrence B={b} L={l} S={s} H={h} src={src} {n}: '
          f'fused {e_fused:.4g} split {e_split:.4g} bf16 eager '
          f'{e_eager:.4g} max|ref| {ref_max:.4g}')
    if not (e_fused <= 2 * e_eager + floor and
            e_fused <= 2 * e_split + floor):
      failed.append((n, e_fused, e_split, e_eager, floor))
  assert not failed, failed


@gpu
def test_decoder_recurrence_rejects_unknown_step_route():
  from lingvo_amd.ops import las_decoder
  x = torch.zeros(1, 1, 128, device='cuda')
  with pytest.raises(ValueError, match='step_route'):
    las_decoder.decoder_recurrence(x, x, x, x, x, x, x, 1.0, 10.0, 32,
                                   step_route='persistent')
  # 'fused' where the shapes do not qualify raises instead of falling back.
  y = torch.zeros(1, 1, 64, device='cuda')
  with pytest.raises(ValueError, match='step_route'):
    las_decoder.decoder_recurrence(y, y, y, y, y, y, y, 1.0, 10.0, 32,
                                   step_route='fused')


# ---------------------------------------------------------------------------
# hipGraph capture of a small AsrModel step on the fused route
# ---------------------------------------------------------------------------

@gpu
def test_captured_asr_step_runs_the_fused_stage(monkeypatch):
  from lingvo_amd.core import py_utils
  from lingvo_amd.core import registry
  ext = _Ext()
  calls = []
  real = ext.las_step_fwd

  def Spy(*args, **kwargs):
    calls.append(1)
    return real(*args, **kwargs)

  monkeypatch.setattr(ext, 'las_step_fwd', Spy)
  mp = registry.GetParams('asr.librispeech.Librispeech960ConformerS', 'Train')
  mp.input.Set(batch_size=4, frame_len=160, target_len=6)
  mp.task.random_seed = 11
  mp.task.encoder.Set(model_dim=128, num_layers=2, num_heads=2,
                      dropout_prob=0.1, specaug_tpl=None)
  mp.task.decoder.Set(rnn_cell_dim=32, emb_dim=16, source_dim=128,
                      dropout_prob=0.1)
  task = mp.Instantiate().to('cuda').GetTask()
  batch = task.input_generator.ToDevice(task.GetInputBatch(), 'cuda')
  loss_name = task.learners[0].p.loss_name

  def Step():
    for v in task.parameters():
      v.grad = None
    with py_utils.StepSeedScope(1234, 3):
      metrics, _ = task.FProp(task.theta, batch)
    loss = metrics[loss_name][0]
    loss.backward()
    return loss

  eager = float(Step().detach())
  per_step = len(calls)
  assert eager == eager and per_step > 0 and per_step % 2 == 0
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    Step()  # warm-up on the capture side
  torch.cuda.current_stream().wait_stream(side)
  for v in task.parameters():
    v.grad = None
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    static_loss = Step()
  graph.replay()
  torch.cuda.synchronize()
  assert len(calls) == 3 * per_step  # the fused stage ran in all three steps
  assert float(static_loss.detach()) == eager
