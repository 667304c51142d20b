"""The deferred-dEnc route of the LAS decoder (ops/hip/las_decoder.hip):
attend_step_fwd, attend_step_bwd and attend_denc called directly against
fp64 references on the exact bf16 input values, their host rejections, the
whole recurrence with either attend_route against an fp64 recurrence, and a
hipGraph capture of a small AsrModel step on the deferred route."""

import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu

BF16_ULP = 2.0 ** -7  # spacing of bf16 values relative to their magnitude
VARIANTS = (0, 1, 2, 3, 4)  # 0 auto; (rows, waves) (4,4) (8,4) (4,8) (8,8)


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _Gen(seed):
  return torch.Generator().manual_seed(seed)


def _Bf16(*shape, g, scale=1.0):
  """Random values that are exact in bf16, as a CPU bf16 tensor."""
  return (torch.randn(*shape, generator=g) * scale).bfloat16()


def _Bits(t):
  """Integer view for bit-for-bit comparisons (NaN-safe)."""
  return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _SameBits(a, b):
  return torch.equal(_Bits(a), _Bits(b))


def _Stack(rows, *shape, dtype, fill):
  """A [rows, *shape] canary-filled stack on the GPU and a copy of it."""
  st = torch.full((rows,) + shape, fill, dtype=dtype, device='cuda')
  return st, st.clone()


def _OnlyRowChanged(stack, before, row):
  keep = [r for r in range(stack.shape[0]) if r != row]
  return _SameBits(stack[keep], before[keep])


# ---------------------------------------------------------------------------
# attend_step_fwd / attend_step_bwd
# ---------------------------------------------------------------------------

# (B, S, D, q scale), as in test_las_decoder_gpu.py. S: below one 4-row
# group; tails after the 16- and 32-row strides; more than one block-wide
# softmax pass. D: one lane, a partly filled 512 slice, exactly one slice,
# one slice plus one lane, all four slices. Last: sharp logits.
ATTEND_SHAPES = [(3, 5, 8, 1.0), (3, 21, 72, 1.0), (3, 67, 512, 1.0),
                 (2, 300, 520, 1.0), (2, 19, 2048, 1.0), (3, 257, 64, 8.0)]


def _AttendPaddings(b, s):
  """Row 0 padded from S/2 on, row 1 fully padded, the last row with one
  padded step in the middle. With two rows the middle step goes to row 0,
  with one row there is no fully padded row."""
  pad = torch.zeros(b, s)
  pad[0, max(s // 2, 1):] = 1.0
  if b >= 3:
    pad[b - 1, s // 2] = 1.0
  elif s >= 4:
    pad[0, s // 4] = 1.0
  if b >= 2:
    pad[1, :] = 1.0
  return pad


@functools.lru_cache(maxsize=None)
def _AttendCase(b, s, d, q_scale):
  """Inputs (CPU, exact in bf16) and fp64 references, once per shape,
  shared by the forward and backward tests. Read-only."""
  g = _Gen(2000 + 31 * s + d)
  q = _Bf16(b, d, g=g, scale=q_scale)
  enc = _Bf16(b, s, d, g=g)
  pad = _AttendPaddings(b, s)
  scale = 1.0 / math.sqrt(d)
  q64, enc64 = q.double(), enc.double()
  logits = scale * torch.einsum('bd,bsd->bs', q64, enc64) - 1e30 * pad.double()
  probs = torch.softmax(logits, dim=-1)
  ctx = torch.einsum('bs,bsd->bd', probs, enc64)
  ctx_abs = torch.einsum('bs,bsd->bd', probs, enc64.abs())
  dctx_a = _Bf16(b, d, g=g)
  dctx_b = _Bf16(b, d, g=g, scale=0.5)
  return dict(q=q, enc=enc, pad=pad, scale=scale, probs=probs, ctx=ctx,
              ctx_abs=ctx_abs, dctx_a=dctx_a, dctx_b=dctx_b)


def _LdsFits(ext, s, d, bwd, variant):
  return ext.attend_step_lds_bytes(s, d, bwd, variant) <= \
      ext.attend_lds_limit()


def _VariantExists(d, variant):
  """8 rows per wave iteration exist up to two 512-column slices."""
  return variant not in (2, 4) or d <= 1024


def _CheckStepFwd(tag, case, probs, ctx, ctx32):
  """probs and ctx to the bounds of attend_fwd (5e-5 ref + 1e-7; one bf16
  ulp plus 1e-5 max|enc|); ctx32 to the probs bound carried through the
  sum, 5e-5 sum_s probs |enc| + 1e-5 max|enc|."""
  pad, ref_p, ref_c = case['pad'], case['probs'], case['ctx']
  b, s = pad.shape
  enc_max = float(case['enc'].abs().max())
  probs, ctx, ctx32 = (t.cpu().double() for t in (probs, ctx, ctx32))
  for t in (probs, ctx, ctx32):
    assert bool(torch.isfinite(t).all())
  p_err = (probs - ref_p).abs()
  p_bound = 5e-5 * ref_p + 1e-7
  c_err = (ctx - ref_c).abs()
  c_bound = BF16_ULP * ref_c.abs() + 1e-5 * enc_max
  c32_err = (ctx32 - ref_c).abs()
  c32_bound = 5e-5 * case['ctx_abs'] + 1e-5 * enc_max
  sum_err = float((probs.sum(-1) - 1.0).abs().max())
  print(f'attend_step_fwd {tag}: probs err/bound '
        f'{float((p_err / p_bound).max()):.3g} | row sum - 1 {sum_err:.3g}'
        f' | ctx err/bound {float((c_err / c_bound).max()):.3g}'
        f' | ctx32 err/bound {float((c32_err / c32_bound).max()):.3g}'
        f' max abs {float(c32_err.max()):.3g}')
  assert bool((p_err <= p_bound).all())
  assert bool((c_err <= c_bound).all())
  assert bool((c32_err <= c32_bound).all())
  assert sum_err <= 1e-5
  for row in range(b):
    if bool((pad[row] < 0.5).any()):
      assert bool((probs[row][pad[row] > 0.5] == 0).all()), row
    else:
      assert float(probs[row].min()) == float(probs[row].max()), row
      assert abs(float(probs[row, 0]) - 1.0 / s) <= 5e-5 / s + 1e-7


@gpu
@pytest.mark.parametrize('b,s,d,q_scale', ATTEND_SHAPES)
def test_attend_step_fwd_matches_fp64(b, s, d, q_scale):
  """Every variant writes row 1 of three-row canary stacks and nothing
  else. A variant whose LDS request is over the limit, or that does not
  exist at this D, raises and writes nothing."""
  ext = _Ext()
  case = _AttendCase(b, s, d, q_scale)
  q, enc, pad = case['q'].cuda(), case['enc'].cuda(), case['pad'].cuda()
  ran = 0
  for variant in VARIANTS:
    probs_st, probs_0 = _Stack(3, b, s, dtype=torch.float32, fill=-7.0)
    ctx_st, ctx_0 = _Stack(3, b, d, dtype=torch.bfloat16, fill=-7.0)
    c32_st, c32_0 = _Stack(3, b, d, dtype=torch.float32, fill=-7.0)
    call = lambda: ext.attend_step_fwd(q, enc, pad, case['scale'],
                                       probs_st[1], ctx_st[1], c32_st[1],
                                       variant)
    if not (_VariantExists(d, variant) and
            _LdsFits(ext, s, d, False, variant)):
      with pytest.raises(RuntimeError):
        call()
      torch.cuda.synchronize()
      assert _SameBits(probs_st, probs_0) and _SameBits(ctx_st, ctx_0)
      assert _SameBits(c32_st, c32_0)
      continue
    call()
    ran += 1
    _CheckStepFwd(f'B={b} S={s} D={d} v{variant}', case, probs_st[1],
                  ctx_st[1], c32_st[1])
    assert _OnlyRowChanged(probs_st, probs_0, 1)
    assert _OnlyRowChanged(ctx_st, ctx_0, 1)
    assert _OnlyRowChanged(c32_st, c32_0, 1)
    # The bf16 context is the fp32 one rounded once.
    assert _SameBits(ctx_st[1], c32_st[1].bfloat16())
  assert ran >= 2  # auto and (4,4) run at every shape


def _StepBwdRef(dctx, case):
  """fp64 dl and dq of the kernel's header formula, and the same formula
  in fp32 torch ops on the same (rounded) inputs: (dl, dq, dl32)."""
  probs, enc, scale = case['probs'], case['enc'], case['scale']
  d64, enc64 = dctx.double(), enc.double()
  dprobs = torch.einsum('bd,bsd->bs', d64, enc64)
  t = (probs * dprobs).sum(-1, keepdim=True)
  dl = probs * (dprobs - t) * scale
  dq = torch.einsum('bs,bsd->bd', dl, enc64)
  d32, enc32 = dctx.float(), enc.float()
  dprobs32 = torch.einsum('bd,bsd->bs', d32, enc32)
  t32 = (d32 * case['ctx'].float()).sum(-1, keepdim=True)
  dl32 = probs.float() * (dprobs32 - t32) * scale
  return dl, dq, dl32


@gpu
@pytest.mark.parametrize('with_b', [False, True])
@pytest.mark.parametrize('b,s,d,q_scale', ATTEND_SHAPES)
def test_attend_step_bwd_matches_fp64(b, s, d, q_scale, with_b):
  """probs and ctx32 are the fp64 references rounded to fp32, so a
  failure here is this kernel's. dq: one bf16 ulp plus 1e-5 max|ref|.
  dl: 2 err32 + 2^-20 max|ref|, err32 being the largest error of the same
  formula in fp32 torch ops. dctx_b is the first D columns of a wider
  buffer, as the recurrence passes it."""
  ext = _Ext()
  case = _AttendCase(b, s, d, q_scale)
  enc = case['enc'].cuda()
  probs = case['probs'].float().cuda()
  ctx32 = case['ctx'].float().cuda()
  dctx_a = case['dctx_a']
  if with_b:
    wide = torch.full((b, d + 24), float('nan'), dtype=torch.bfloat16)
    wide[:, :d] = case['dctx_b']
    dctx_b = wide.cuda()[:, :d]
    assert not dctx_b.is_contiguous()
    dctx = dctx_a + case['dctx_b']  # torch's bf16 add: one rounding
  else:
    dctx_b, dctx = None, dctx_a
  want_dl, want_dq, dl32 = _StepBwdRef(dctx, case)
  err32 = float((dl32.double() - want_dl).abs().max())
  dl_bound = 2 * err32 + 2.0 ** -20 * float(want_dl.abs().max())
  q_bound = BF16_ULP * want_dq.abs() + 1e-5 * float(want_dq.abs().max())

  first = None
  for variant in VARIANTS:
    if not (_VariantExists(d, variant) and
            _LdsFits(ext, s, d, True, variant)):
      continue
    outs = []
    for _ in range(2):
      dc_st, dc_0 = _Stack(3, b, d, dtype=torch.bfloat16, fill=-7.0)
      dl_st, dl_0 = _Stack(3, b, s, dtype=torch.float32, fill=-7.0)
      dq_st, dq_0 = _Stack(3, b, d, dtype=torch.bfloat16, fill=-7.0)
      ext.attend_step_bwd(dctx_a.cuda(), dctx_b, probs, ctx32, enc,
                          case['scale'], dc_st[1], dl_st[1], dq_st[1],
                          variant)
      assert _OnlyRowChanged(dc_st, dc_0, 1)
      assert _OnlyRowChanged(dl_st, dl_0, 1)
      assert _OnlyRowChanged(dq_st, dq_0, 1)
      outs.append((dc_st[1].cpu(), dl_st[1].cpu(), dq_st[1].cpu()))
    (dc, dl, dq), again = outs
    assert all(_SameBits(x, y) for x, y in zip(outs[0], again))
    assert _SameBits(dc, dctx)
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dq).all())
    dl_err = float((dl.double() - want_dl).abs().max())
    q_err = (dq.double() - want_dq).abs()
    print(f'attend_step_bwd B={b} S={s} D={d} v{variant} b={with_b}: dl err '
          f'{dl_err:.3g} fp32 torch {err32:.3g} bound {dl_bound:.3g} | dq '
          f'err/bound {float((q_err / q_bound).max()):.3g}')
    assert dl_err <= dl_bound
    assert bool((q_err <= q_bound).all())
    if first is None:
      first = (dl, dq)
  assert first is not None


# ---------------------------------------------------------------------------
# attend_denc
# ---------------------------------------------------------------------------

def _DencShapes():
  """(L, B, S, D) with T the kernel's row tile: S at 1, T-1, T, T+1 and
  300; L in 1, 2, 5, 64 and 70 (a second LDS fill of 64 steps); D one
  lane, three lanes, one slice, one slice plus a lane, four slices; B in
  1, 3, 130."""
  t = _Ext().attend_denc_row_tile()
  return [(1, 1, 1, 8), (2, 3, t - 1, 24), (5, 3, t, 520), (64, 1, t + 1, 512),
          (2, 130, t + 1, 24), (5, 2, 300, 512), (2, 1, 5, 2048),
          (70, 3, t + 1, 8)]


@gpu
@pytest.mark.parametrize('case_idx', range(8))
def test_attend_denc_matches_fp64_einsum(case_idx):
  """fp32 output: 2 err32 + 2^-20 max|ref|, err32 the largest error of the
  same einsums in fp32 torch ops; bf16 output adds one bf16 ulp of the
  reference. The output is rows 1..B of a [B+2,S,D] canary allocation.
  Step s=0 of the last batch row has dl = probs = 0: exact zeros."""
  ext = _Ext()
  l, b, s, d = _DencShapes()[case_idx]
  g = _Gen(300 + case_idx)
  dl = torch.randn(l, b, s, generator=g) * 0.1
  probs = torch.softmax(torch.randn(l, b, s, generator=g) * 2, dim=-1)
  dl[:, b - 1, 0] = 0.0
  probs[:, b - 1, 0] = 0.0
  qs = _Bf16(l, b, d, g=g)
  dctx = _Bf16(l, b, d, g=g)
  ein = lambda a, x: torch.einsum('lbs,lbd->bsd', a, x)
  want = ein(dl.double(), qs.double()) + ein(probs.double(), dctx.double())
  got32 = ein(dl, qs.float()) + ein(probs, dctx.float())
  err32 = float((got32.double() - want).abs().max())
  ref_max = float(want.abs().max())
  floor = 2 * err32 + 2.0 ** -20 * ref_max
  args = [t.cuda() for t in (dl, probs, qs, dctx)]
  for dtype in (torch.float32, torch.bfloat16):
    outs = []
    for _ in range(2):
      buf, buf_0 = _Stack(b + 2, s, d, dtype=dtype, fill=-7.0)
      ext.attend_denc(*args, buf[1:b + 1])
      assert _SameBits(buf[0], buf_0[0]) and _SameBits(buf[-1], buf_0[-1])
      outs.append(buf[1:b + 1].cpu())
    assert _SameBits(outs[0], outs[1])
    got = outs[0].double()
    assert bool(torch.isfinite(got).all())
    err = (got - want).abs()
    bound = floor + (BF16_ULP * want.abs() if dtype == torch.bfloat16 else 0)
    print(f'attend_denc L={l} B={b} S={s} D={d} {dtype}: max err '
          f'{float(err.max()):.3g} fp32 torch {err32:.3g} floor {floor:.3g} '
          f'max|ref| {ref_max:.3g}')
    assert bool((err <= bound).all())
    assert not bool(outs[0][b - 1, 0].any())


# ---------------------------------------------------------------------------
# Host rejections: one broken condition per call, outputs bit-unchanged.
# ---------------------------------------------------------------------------

def _Mk(*shape, dtype=torch.bfloat16, device='cuda', fill=1.0):
  return torch.full(shape, fill, dtype=dtype, device=device)


def _F32(*shape, **kw):
  return _Mk(*shape, dtype=torch.float32, **kw)


def _StepArgs(b=2, s=5, d=16):
  return dict(q=_Mk(b, d), enc=_Mk(b, s, d), pad=_F32(b, s, fill=0.0),
              probs=_F32(b, s, fill=3.0), ctx=_Mk(b, d, fill=3.0),
              ctx32=_F32(b, d, fill=3.0), dctx_a=_Mk(b, d), dctx_b=None,
              dctx_out=_Mk(b, d, fill=3.0), dl=_F32(b, s, fill=3.0),
              dq=_Mk(b, d, fill=3.0), variant=0)


def _BigS(ext, bwd):
  """An S whose LDS request is over the limit at D=16 (forward only: the
  backward request does not grow with S), else None."""
  return None if bwd else ext.attend_lds_limit() // 4 + 1


def _StepRejectCases():
  """name -> (overrides, applies to fwd, applies to bwd)."""
  both = lambda fn: (fn, True, True)
  fwd = lambda fn: (fn, True, False)
  bwd = lambda fn: (fn, False, True)
  return {
      'd_not_multiple_of_8': both(lambda: dict(
          q=_Mk(2, 12), dctx_a=_Mk(2, 12), enc=_Mk(2, 5, 12),
          ctx=_Mk(2, 12), ctx32=_F32(2, 12), dctx_out=_Mk(2, 12),
          dq=_Mk(2, 12))),
      'd_over_2048': both(lambda: dict(
          q=_Mk(2, 2056), dctx_a=_Mk(2, 2056), enc=_Mk(2, 5, 2056),
          ctx=_Mk(2, 2056), ctx32=_F32(2, 2056), dctx_out=_Mk(2, 2056),
          dq=_Mk(2, 2056))),
      's_zero': both(lambda: dict(
          enc=_Mk(2, 0, 16), pad=_F32(2, 0), probs=_F32(2, 0),
          dl=_F32(2, 0))),
      'enc_on_cpu': both(lambda: dict(enc=_Mk(2, 5, 16, device='cpu'))),
      'enc_fp32': both(lambda: dict(enc=_F32(2, 5, 16))),
      'enc_not_contiguous': both(lambda: dict(enc=_Mk(2, 5, 32)[:, :, ::2])),
      'enc_fewer_rows': both(lambda: dict(enc=_Mk(1, 5, 16))),
      'variant_5': both(lambda: dict(variant=5)),
      'variant_negative': both(lambda: dict(variant=-1)),
      'variant_8_rows_at_d_1032': both(lambda: dict(
          q=_Mk(2, 1032), dctx_a=_Mk(2, 1032), enc=_Mk(2, 5, 1032),
          ctx=_Mk(2, 1032), ctx32=_F32(2, 1032), dctx_out=_Mk(2, 1032),
          dq=_Mk(2, 1032), variant=2)),
      'q_fp32': fwd(lambda: dict(q=_F32(2, 16))),
      'q_on_cpu': fwd(lambda: dict(q=_Mk(2, 16, device='cpu'))),
      'q_not_contiguous': fwd(lambda: dict(q=_Mk(2, 32)[:, ::2])),
      'pad_bf16': fwd(lambda: dict(pad=_Mk(2, 5))),
      'pad_shorter_than_s': fwd(lambda: dict(pad=_F32(2, 4))),
      'probs_out_bf16': fwd(lambda: dict(probs=_Mk(2, 5))),
      'probs_out_not_contiguous': fwd(lambda: dict(probs=_F32(2, 10)[:, ::2])),
      'probs_out_other_s': fwd(lambda: dict(probs=_F32(2, 4))),
      'ctx_fp32': fwd(lambda: dict(ctx=_F32(2, 16))),
      'ctx_fewer_rows': fwd(lambda: dict(ctx=_Mk(1, 16))),
      'ctx_on_cpu': fwd(lambda: dict(ctx=_Mk(2, 16, device='cpu'))),
      'ctx32_out_bf16': fwd(lambda: dict(ctx32=_Mk(2, 16))),
      'ctx32_out_not_contiguous': fwd(lambda: dict(
          ctx32=_F32(2, 32)[:, ::2])),
      'dctx_a_fp32': bwd(lambda: dict(dctx_a=_F32(2, 16))),
      'dctx_a_on_cpu': bwd(lambda: dict(dctx_a=_Mk(2, 16, device='cpu'))),
      'dctx_a_not_contiguous': bwd(lambda: dict(dctx_a=_Mk(2, 32)[:, :16])),
      'dctx_b_fp32': bwd(lambda: dict(dctx_b=_F32(2, 16))),
      'dctx_b_on_cpu': bwd(lambda: dict(dctx_b=_Mk(2, 16, device='cpu'))),
      'dctx_b_column_stride_2': bwd(lambda: dict(dctx_b=_Mk(2, 32)[:, ::2])),
      'dctx_b_other_d': bwd(lambda: dict(dctx_b=_Mk(2, 8))),
      'dctx_b_transposed': bwd(lambda: dict(dctx_b=_Mk(16, 2).t())),
      'probs_in_bf16': bwd(lambda: dict(probs=_Mk(2, 5))),
      'probs_in_on_cpu': bwd(lambda: dict(probs=_F32(2, 5, device='cpu'))),
      'ctx32_in_bf16': bwd(lambda: dict(ctx32=_Mk(2, 16))),
      'ctx32_in_other_d': bwd(lambda: dict(ctx32=_F32(2, 8))),
      'dctx_out_fp32': bwd(lambda: dict(dctx_out=_F32(2, 16))),
      'dctx_out_not_contiguous': bwd(lambda: dict(
          dctx_out=_Mk(2, 32)[:, ::2])),
      'dl_bf16': bwd(lambda: dict(dl=_Mk(2, 5))),
      'dl_other_s': bwd(lambda: dict(dl=_F32(2, 6))),
      'dq_fp32': bwd(lambda: dict(dq=_F32(2, 16))),
      'dq_fewer_rows': bwd(lambda: dict(dq=_Mk(1, 16))),
      'dq_on_cpu': bwd(lambda: dict(dq=_Mk(2, 16, device='cpu'))),
  }


def _Snapshot(tensors):
  return [t.clone() for t in tensors]


def _Unchanged(tensors, before):
  torch.cuda.synchronize()
  return all(_SameBits(t.contiguous(), b.contiguous())
             for t, b in zip(tensors, before))


@gpu
@pytest.mark.parametrize('name', sorted(
    n for n, c in _StepRejectCases().items() if c[1]))
def test_attend_step_fwd_rejects(name):
  ext = _Ext()
  a = _StepArgs()
  a.update(_StepRejectCases()[name][0]())
  outs = [a['probs'], a['ctx'], a['ctx32']]
  before = _Snapshot(outs)
  with pytest.raises(RuntimeError):
    ext.attend_step_fwd(a['q'], a['enc'], a['pad'], 0.25, a['probs'],
                        a['ctx'], a['ctx32'], a['variant'])
  assert _Unchanged(outs, before)


@gpu
def test_attend_step_fwd_rejects_s_over_the_lds_limit():
  ext = _Ext()
  s = _BigS(ext, bwd=False)
  assert ext.attend_step_lds_bytes(s, 8, False, 1) > ext.attend_lds_limit()
  a = _StepArgs(b=1, s=s, d=8)
  outs = [a['probs'], a['ctx'], a['ctx32']]
  before = _Snapshot(outs)
  with pytest.raises(RuntimeError, match='LDS'):
    ext.attend_step_fwd(a['q'], a['enc'], a['pad'], 0.25, a['probs'],
                        a['ctx'], a['ctx32'], 1)
  assert _Unchanged(outs, before)


@gpu
@pytest.mark.parametrize('name', sorted(
    n for n, c in _StepRejectCases().items() if c[2]))
def test_attend_step_bwd_rejects(name):
  ext = _Ext()
  a = _StepArgs()
  a.update(_StepRejectCases()[name][0]())
  outs = [a['dctx_out'], a['dl'], a['dq']]
  before = _Snapshot(outs)
  with pytest.raises(RuntimeError):
    ext.attend_step_bwd(a['dctx_a'], a['dctx_b'], a['probs'], a['ctx32'],
                        a['enc'], 0.25, a['dctx_out'], a['dl'], a['dq'],
                        a['variant'])
  assert _Unchanged(outs, before)


def _DencArgs(l=2, b=2, s=5, d=16):
  return dict(dl=_F32(l, b, s), probs=_F32(l, b, s), qs=_Mk(l, b, d),
              dctx=_Mk(l, b, d), out=_F32(b, s, d, fill=3.0))


def _DencRejectCases():
  return {
      'dl_bf16': lambda: dict(dl=_Mk(2, 2, 5)),
      'dl_on_cpu': lambda: dict(dl=_F32(2, 2, 5, device='cpu')),
      'dl_two_dims': lambda: dict(dl=_F32(2, 10)),
      'dl_not_contiguous': lambda: dict(dl=_F32(2, 2, 10)[:, :, ::2]),
      's_zero': lambda: dict(dl=_F32(2, 2, 0), probs=_F32(2, 2, 0),
                             out=_F32(2, 0, 16)),
      'l_zero': lambda: dict(dl=_F32(0, 2, 5), probs=_F32(0, 2, 5),
                             qs=_Mk(0, 2, 16), dctx=_Mk(0, 2, 16)),
      'probs_other_s': lambda: dict(probs=_F32(2, 2, 4)),
      'probs_bf16': lambda: dict(probs=_Mk(2, 2, 5)),
      'qs_fp32': lambda: dict(qs=_F32(2, 2, 16)),
      'qs_other_l': lambda: dict(qs=_Mk(3, 2, 16)),
      'qs_not_contiguous': lambda: dict(qs=_Mk(2, 2, 32)[:, :, ::2]),
      'd_not_multiple_of_8': lambda: dict(
          qs=_Mk(2, 2, 12), dctx=_Mk(2, 2, 12), out=_F32(2, 5, 12)),
      'd_over_2048': lambda: dict(
          qs=_Mk(2, 2, 2056), dctx=_Mk(2, 2, 2056), out=_F32(2, 5, 2056)),
      'dctx_other_d': lambda: dict(dctx=_Mk(2, 2, 8)),
      'dctx_on_cpu': lambda: dict(dctx=_Mk(2, 2, 16, device='cpu')),
      'out_fp16': lambda: dict(out=_Mk(2, 5, 16, dtype=torch.float16)),
      'out_on_cpu': lambda: dict(out=_F32(2, 5, 16, device='cpu')),
      'out_other_s': lambda: dict(out=_F32(2, 4, 16)),
      'out_lbd_order': lambda: dict(out=_F32(5, 2, 16)),
      'out_not_contiguous': lambda: dict(out=_F32(2, 5, 32)[:, :, ::2]),
  }


@gpu
@pytest.mark.parametrize('name', sorted(_DencRejectCases()))
def test_attend_denc_rejects(name):
  ext = _Ext()
  a = _DencArgs()
  a.update(_DencRejectCases()[name]())
  before = _Snapshot([a['out']])
  with pytest.raises(RuntimeError):
    ext.attend_denc(a['dl'], a['probs'], a['qs'], a['dctx'], a['out'])
  assert _Unchanged([a['out']], before)


# ---------------------------------------------------------------------------
# Whole recurrence against fp64, both routes
# ---------------------------------------------------------------------------

def _RefRecurrence(emb_gates, w_cm0, b1, wm1, wq, enc, pad, fgb, cap):
  """decoder_recurrence's docstring as plain torch ops in the dtype of its
  inputs: 2-layer LSTM (gate order cand, i, f, o; forget-gate bias fgb;
  |c| clamped to cap), dot attention over enc with the additive -1e30
  padding mask, out = cat(m1, ctx)."""
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
# The shapes of test_las_decoder_gpu.py, and S=40 crossing attend_denc's
# 32-row tile with three steps to sum.
@pytest.mark.parametrize('b,l,s,h,src', [(3, 4, 21, 32, 64),
                                         (130, 2, 5, 32, 32),
                                         (2, 3, 40, 32, 64)])
def test_decoder_recurrence_routes_match_fp64(b, l, s, h, src):
  """Output and every gradient of either route against the fp64
  recurrence: err <= 2 err_bf16_eager + 2^-8 max|ref|, and the deferred
  route no worse than 2 err_accumulate + the same floor."""
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

  def Fused(route):
    return lambda eg, w_cm0, b1, wm1, wq, enc, pad: \
        las_decoder.decoder_recurrence(eg, w_cm0, b1, wm1, wq, enc, pad, fgb,
                                       cap, src, attend_route=route)

  want = _RunRecurrence(ref_fn, inputs, pad, w, 'cpu', torch.float64)
  eager = _RunRecurrence(ref_fn, inputs, pad, w, 'cuda', torch.bfloat16)
  acc = _RunRecurrence(Fused('accumulate'), inputs, pad, w, 'cuda',
                       torch.bfloat16)
  dfr = _RunRecurrence(Fused('deferred'), inputs, pad, w, 'cuda',
                       torch.bfloat16)
  auto = _RunRecurrence(Fused('auto'), inputs, pad, w, 'cuda',
                        torch.bfloat16)

  failed = []
  for n in ('out',) + REC_NAMES:
    assert dfr[n].shape == want[n].shape, n
    assert torch.equal(auto[n], dfr[n]), n  # 'auto' is 'deferred'
    ref_max = float(want[n].abs().max())
    assert ref_max > 0, n
    e_dfr = float((dfr[n] - want[n]).abs().max())
    e_acc = float((acc[n] - want[n]).abs().max())
    e_eager = float((eager[n] - want[n]).abs().max())
    floor = 2.0 ** -8 * ref_max
    bound = 2 * e_eager + floor
    print(f'decoder_recurrence B={b} L={l} S={s} H={h} src={src} {n}: '
          f'deferred {e_dfr:.4g} accumulate {e_acc:.4g} bf16 eager '
          f'{e_eager:.4g} max|ref| {ref_max:.4g} bound {bound:.4g}')
    if not (e_dfr <= bound and e_acc <= bound and
            e_dfr <= 2 * e_acc + floor):
      failed.append((n, e_dfr, e_acc, bound))
  assert not failed, failed


@gpu
def test_decoder_recurrence_rejects_unknown_route():
  from lingvo_amd.ops import las_decoder
  x = torch.zeros(1, device='cuda')
  with pytest.raises(ValueError, match='attend_route'):
    las_decoder.decoder_recurrence(x, x, x, x, x, x, x, 1.0, 10.0, 32,
                                   attend_route='fused')


# ---------------------------------------------------------------------------
# hipGraph capture of a small AsrModel step on the deferred route
# ---------------------------------------------------------------------------

@gpu
def test_captured_asr_step_returns_eager_loss(monkeypatch):
  from lingvo_amd.core import py_utils
  from lingvo_amd.core import registry
  ext = _Ext()
  calls = []
  real = ext.attend_denc

  def Spy(*args, **kwargs):
    calls.append(1)
    return real(*args, **kwargs)

  monkeypatch.setattr(ext, 'attend_denc', Spy)
  mp = registry.GetParams('asr.librispeech.Librispeech960ConformerS', 'Train')
  mp.input.Set(batch_size=4, frame_len=160, target_len=6)
  mp.task.random_seed = 11
  # Two heads of 64, the smallest the attention kernels take.
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
  assert eager == eager and len(calls) == 1
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
  assert len(calls) == 3  # the deferred route ran in all three steps
  assert float(static_loss.detach()) == eager
