"""LAS decoder-step HIP kernels (ops/hip/las_decoder.hip) called directly:
smallm_gemm, attend_fwd and attend_bwd against fp64 references of the same
op on the exact bf16 input values, the host wrappers' rejections, the
whole fused recurrence against an fp64 recurrence, and the eager fall-back
of AsrDecoder for shapes the kernels do not support."""

import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu

BF16_ULP = 2.0 ** -7  # spacing of bf16 values relative to their magnitude


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


# ---------------------------------------------------------------------------
# smallm_gemm
# ---------------------------------------------------------------------------

# M: 1 row; one full m-tile; one row into tile 1; a partial tile 6; all 8
# tiles; one row into the second m-block; a partial second m-block.
# N: 8 and 24, 40, 264 end in a partly filled 16-column tile.
# K: 1..16 MFMA k-steps, i.e. 1, 2, 3 (uneven wave quota), 4, 5 and 16.
GEMM_SHAPES = [(1, 16, 32), (16, 16, 32), (17, 24, 64), (100, 40, 96),
               (128, 64, 160), (129, 8, 128), (200, 264, 512)]
WT_COL0 = [0, 32]


def _WtBuffer(n, k, wt_col0, fill):
  """[N+3, wt_col0+K+8] weight buffer: more rows than N and columns on
  both sides of the K slice, so a wrong row, column or stride reads a
  value that is not the wanted one."""
  return torch.full((n + 3, wt_col0 + k + 8), fill, dtype=torch.float32)


@gpu
@pytest.mark.parametrize('wt_col0', WT_COL0)
@pytest.mark.parametrize('m,n,k', GEMM_SHAPES)
def test_smallm_gemm_selects_exact_weight_entries(m, n, k, wt_col0):
  """One-hot rows of A pick single entries of Wt: any error in the row,
  column or k mapping, or in a wave's K quota, moves an integer."""
  ext = _Ext()
  sel = (7 * torch.arange(m) + 3) % k
  a = torch.zeros(m, k)
  a[torch.arange(m), sel] = 1.0
  wt = _WtBuffer(n, k, wt_col0, 200.0)
  j = torch.arange(n + 3).unsqueeze(1)
  kk = torch.arange(k).unsqueeze(0)
  wt[:, wt_col0:wt_col0 + k] = ((j * 5 + kk * 3) % 251 - 125).float()
  want = wt[:n, wt_col0 + sel].t().contiguous().bfloat16()  # [M, N]
  assert torch.equal(want.float(), wt[:n, wt_col0 + sel].t())  # exact in bf16

  out = torch.full((m, n), -300.0, dtype=torch.bfloat16, device='cuda')
  ext.smallm_gemm(a.bfloat16().cuda(), wt.bfloat16().cuda(), None, out, k,
                  wt_col0, 1.0, 0)
  got = out.cpu()
  bad = (got != want).nonzero()
  assert torch.equal(got, want), (
      f'{bad.shape[0]} wrong elements, first at {bad[0].tolist()}: '
      f'got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}')


@gpu
@pytest.mark.parametrize('m,n,k', GEMM_SHAPES)
def test_smallm_gemm_random_values_match_fp64(m, n, k):
  """out = alpha * A @ W^T + {nothing, row vector, matrix, previous out}.

  Bound per element: 2^-7 |ref| + 2^-20 mag, with
  mag = |alpha| (|A| |W|^T) + |pre or out_prev|. The first term is one
  bf16 ulp for the single rounding of the result, the second covers the
  order of the fp32 accumulation. An fp32 matmul rounded once to bf16
  stays within half of this for K up to 1024."""
  ext = _Ext()
  worst = 0.0
  for wt_col0 in WT_COL0:
    g = _Gen(100 + m + n + k + wt_col0)
    a = _Bf16(m, k, g=g)
    wt = _WtBuffer(n, k, wt_col0, 0.0).bfloat16()
    wt.copy_(_Bf16(*wt.shape, g=g))
    pre_row = _Bf16(n, g=g, scale=2.0)
    pre_mat = _Bf16(m, n, g=g, scale=2.0)
    out_prev = _Bf16(m, n, g=g, scale=2.0)
    a64 = a.double()
    w64 = wt[:n, wt_col0:wt_col0 + k].double()
    prod = a64 @ w64.t()
    prod_abs = a64.abs() @ w64.abs().t()
    a_d, wt_d = a.cuda(), wt.cuda()
    for mode in (0, 1, 2, 3):
      pre = {0: None, 1: pre_row, 2: pre_mat, 3: None}[mode]
      add = {0: torch.zeros(m, n), 1: pre_row.expand(m, n), 2: pre_mat,
             3: out_prev}[mode].double()
      for alpha in (1.0, -0.5):
        out = (out_prev if mode == 3 else
               torch.full((m, n), float('nan'), dtype=torch.bfloat16)).cuda()
        ext.smallm_gemm(a_d, wt_d, None if pre is None else pre.cuda(),
                        out, k, wt_col0, alpha, mode)
        ref = alpha * prod + add
        bound = BF16_ULP * ref.abs() + 2.0 ** -20 * (
            abs(alpha) * prod_abs + add.abs())
        err = (out.cpu().double() - ref).abs()
        assert bool(torch.isfinite(out).all()), (mode, alpha, wt_col0)
        ratio = float((err / bound.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), (
            f'mode={mode} alpha={alpha} wt_col0={wt_col0}: '
            f'err/bound {ratio:.3g}, max err {float(err.max()):.4g}')
  print(f'smallm_gemm M={m} N={n} K={k}: worst err/bound {worst:.3g}')


@gpu
@pytest.mark.parametrize('mode', [0, 2, 3])
@pytest.mark.parametrize('m,n,k', [(17, 24, 64), (100, 40, 96),
                                   (129, 8, 128)])
def test_smallm_gemm_touches_only_its_m_rows(m, n, k, mode):
  """out and a are the first M rows of larger buffers: the rows behind
  out keep their bits, and the NaN rows behind a reach no output."""
  ext = _Ext()
  g = _Gen(7 + m)
  buf = torch.full((m + 16, n), -1234.0, dtype=torch.bfloat16, device='cuda')
  if mode == 3:
    buf[:m] = _Bf16(m, n, g=g).cuda()
  before = buf.clone()
  abuf = torch.full((m + 16, k), float('nan'), dtype=torch.bfloat16,
                    device='cuda')
  abuf[:m] = _Bf16(m, k, g=g).cuda()
  pre = _Bf16(m, n, g=g).cuda() if mode == 2 else None
  wt = _Bf16(n, k, g=g).cuda()
  out = buf[:m]
  ext.smallm_gemm(abuf[:m], wt, pre, out, k, 0, 1.0, mode)
  torch.cuda.synchronize()
  assert _SameBits(buf[m:], before[m:])
  assert bool(torch.isfinite(out).all())
  assert not _SameBits(buf[:m], before[:m])


# ---------------------------------------------------------------------------
# attend_fwd / attend_bwd
# ---------------------------------------------------------------------------

# (B, S, D, q scale). S: below one 4-step group; tails of 1 and 3 steps
# after the 16-step stride; more than one 256-stride softmax pass. D: one
# lane, a partly filled 512 slice, exactly one slice, one slice plus one
# lane, all four slices. Last: sharp logits.
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


def _AttendRef(q, enc, pad, scale):
  """fp64 softmax(scale q enc^T - 1e30 pad) and probs enc."""
  q64, enc64 = q.double(), enc.double()
  logits = scale * torch.einsum('bd,bsd->bs', q64, enc64) - 1e30 * pad.double()
  probs = torch.softmax(logits, dim=-1)
  return probs, torch.einsum('bs,bsd->bd', probs, enc64)


def _AttendBwdRef(dctx, probs, q, enc, scale):
  """fp64 backward of the attention step, as the kernel's header states it:
  dprobs = dctx enc^T; t = sum(probs dprobs); dl = probs (dprobs - t) scale;
  dq = dl enc; denc = dl (x) q + probs (x) dctx."""
  dctx64, q64, enc64 = dctx.double(), q.double(), enc.double()
  dprobs = torch.einsum('bd,bsd->bs', dctx64, enc64)
  t = (probs * dprobs).sum(-1, keepdim=True)
  dl = probs * (dprobs - t) * scale
  dq = torch.einsum('bs,bsd->bd', dl, enc64)
  denc = dl.unsqueeze(-1) * q64.unsqueeze(1) + \
      probs.unsqueeze(-1) * dctx64.unsqueeze(1)
  return dq, denc


@functools.lru_cache(maxsize=None)
def _AttendCase(b, s, d, q_scale):
  """Inputs (CPU, exact in bf16) and the fp64 references, computed once
  per shape and shared by the forward and backward tests. Read-only."""
  g = _Gen(1000 + 31 * s + d)
  q = _Bf16(b, d, g=g, scale=q_scale)
  enc = _Bf16(b, s, d, g=g)
  pad = _AttendPaddings(b, s)
  scale = 1.0 / math.sqrt(d)
  probs, ctx = _AttendRef(q, enc, pad, scale)
  dctx32 = torch.randn(b, d, generator=g)
  dq, denc = _AttendBwdRef(dctx32.bfloat16(), probs, q, enc, scale)
  denc0 = torch.randn(b + 1, s, d, generator=g) * float(denc.abs().max()) / 4
  return dict(q=q, enc=enc, pad=pad, scale=scale, probs=probs, ctx=ctx,
              dctx32=dctx32, dq=dq, denc=denc, denc0=denc0)


def _CheckAttendFwd(tag, case, probs, ctx):
  """The forward bounds. probs (fp32): 5e-5 ref + 1e-7 - fp32 torch math
  of the same inputs is within 3.1e-6 relative of fp64, which leaves the
  fast exp about 15x, and one bf16 rounding of the logits is 80x over.
  ctx (bf16): one bf16 ulp of the result plus 1e-5 max|enc| for the fp32
  sums."""
  pad, ref_p, ref_c = case['pad'], case['probs'], case['ctx']
  b, s = pad.shape
  probs, ctx = probs.cpu().double(), ctx.cpu().double()
  assert bool(torch.isfinite(probs).all()) and bool(torch.isfinite(ctx).all())
  p_err = (probs - ref_p).abs()
  p_bound = 5e-5 * ref_p + 1e-7
  c_err = (ctx - ref_c).abs()
  c_bound = BF16_ULP * ref_c.abs() + 1e-5 * float(case['enc'].abs().max())
  sum_err = float((probs.sum(-1) - 1.0).abs().max())
  print(f'attend_fwd {tag}: probs err/bound {float((p_err / p_bound).max()):.3g}'
        f' max abs {float(p_err.max()):.3g}'
        f' max rel {float((p_err / ref_p.clamp_min(1e-30))[ref_p > 1e-6].max()):.3g}'
        f' | row sum - 1 {sum_err:.3g}'
        f' | ctx err/bound {float((c_err / c_bound).max()):.3g}'
        f' max abs {float(c_err.max()):.3g}')
  assert bool((p_err <= p_bound).all())
  assert bool((c_err <= c_bound).all())
  assert sum_err <= 1e-5
  for row in range(b):
    if bool((pad[row] < 0.5).any()):
      # Padded steps of a row that has real ones get exactly nothing.
      assert bool((probs[row][pad[row] > 0.5] == 0).all()), row
    else:
      # The additive -1e30 absorbs every logit: uniform 1/S.
      assert float(probs[row].min()) == float(probs[row].max()), row
      assert abs(float(probs[row, 0]) - 1.0 / s) <= 5e-5 / s + 1e-7


@gpu
@pytest.mark.parametrize('b,s,d,q_scale', ATTEND_SHAPES)
def test_attend_fwd_matches_fp64(b, s, d, q_scale):
  ext = _Ext()
  case = _AttendCase(b, s, d, q_scale)
  probs, ctx = ext.attend_fwd(case['q'].cuda(), case['enc'].cuda(),
                              case['pad'].cuda(), case['scale'])
  assert probs.dtype == torch.float32 and probs.shape == (b, s)
  assert ctx.dtype == torch.bfloat16 and ctx.shape == (b, d)
  _CheckAttendFwd(f'B={b} S={s} D={d}', case, probs, ctx)


def _MaxS(ext, d, bwd):
  """Largest S whose dynamic LDS request fits the device's limit, from the
  layouts in the kernels' comments: q or (dctx, q) as bf16 [D], one fp32
  [S], four fp32 [D] partials, four fp32 for the block reduction."""
  limit = ext.attend_lds_limit()
  fixed = (4 if bwd else 2) * d + 16 * d + 16
  s = (limit - fixed) // 4
  assert ext.attend_lds_bytes(s, d, bwd) == fixed + 4 * s <= limit
  assert ext.attend_lds_bytes(s + 1, d, bwd) > limit
  return s


def _LdsEdgeCase(s, d):
  g = _Gen(5)
  q = _Bf16(1, d, g=g)
  enc = _Bf16(1, s, d, g=g)
  pad = _AttendPaddings(1, s)
  scale = 1.0 / math.sqrt(d)
  probs, ctx = _AttendRef(q, enc, pad, scale)
  return dict(q=q, enc=enc, pad=pad, scale=scale, probs=probs, ctx=ctx)


@gpu
def test_attend_fwd_at_and_over_the_lds_limit():
  """The longest source the device's LDS holds meets the same bounds (and
  runs the 256-stride softmax loops many times); one step more raises."""
  ext = _Ext()
  d = 8
  s = _MaxS(ext, d, bwd=False)
  assert s > 256 * 8
  case = _LdsEdgeCase(s, d)
  q, pad = case['q'].cuda(), case['pad'].cuda()
  probs, ctx = ext.attend_fwd(q, case['enc'].cuda(), pad, case['scale'])
  _CheckAttendFwd(f'B=1 S={s} D={d} (LDS limit)', case, probs, ctx)
  enc_over = torch.zeros(1, s + 1, d, dtype=torch.bfloat16, device='cuda')
  with pytest.raises(RuntimeError, match='LDS'):
    ext.attend_fwd(q, enc_over, torch.zeros(1, s + 1, device='cuda'),
                   case['scale'])


def _CheckAttendBwd(tag, dq, denc, want_dq, want_denc, denc_tol):
  """dq (bf16): one bf16 ulp of the result plus 1e-5 max|ref| for the fp32
  sums. denc (fp32 accumulator): denc_tol max|ref| absolute. fp32 torch
  math sits at half the dq bound and at 3e-7 for denc."""
  dq, denc = dq.cpu().double(), denc.cpu().double()
  q_err = (dq - want_dq).abs()
  q_bound = BF16_ULP * want_dq.abs() + 1e-5 * float(want_dq.abs().max())
  e_err = (denc - want_denc).abs()
  print(f'attend_bwd {tag}: dq err/bound {float((q_err / q_bound).max()):.3g}'
        f' max abs {float(q_err.max()):.3g} | denc max err'
        f' {float(e_err.max()):.3g} bound {denc_tol:.3g}')
  assert bool(torch.isfinite(dq).all()) and bool(torch.isfinite(denc).all())
  assert bool((q_err <= q_bound).all())
  assert float(e_err.max()) <= denc_tol


@gpu
@pytest.mark.parametrize('b,s,d,q_scale', ATTEND_SHAPES)
def test_attend_bwd_matches_fp64(b, s, d, q_scale):
  """probs is the fp64 reference softmax rounded to fp32, so a failure
  here is the backward kernel's. denc is the first B rows of a [B+1,S,D]
  buffer of random values of the gradient's magnitude."""
  ext = _Ext()
  case = _AttendCase(b, s, d, q_scale)
  q, enc = case['q'].cuda(), case['enc'].cuda()
  probs = case['probs'].float().cuda()
  dctx32 = case['dctx32'].cuda()
  dctx = dctx32.bfloat16()
  want_dq, want_inc = case['dq'], case['denc']
  gmax = float(want_inc.abs().max())
  before = case['denc0'][:b].double()
  buf = case['denc0'].cuda()
  tail = buf[b:].clone()
  denc = buf[:b]
  tag = f'B={b} S={s} D={d}'

  dq1 = ext.attend_bwd(dctx, probs, q, enc, denc, case['scale'])[0]
  assert dq1.dtype == torch.bfloat16 and dq1.shape == (b, d)
  _CheckAttendBwd(tag, dq1, denc, want_dq, before + want_inc, 1e-5 * gmax)
  assert _SameBits(buf[b:], tail)

  # Accumulate, not overwrite: the same call adds the same increment
  # again. Each call is held to 1e-5 max|ref|, so two are held to 2e-5.
  dq2 = ext.attend_bwd(dctx, probs, q, enc, denc, case['scale'])[0]
  assert _SameBits(dq2, dq1)
  _CheckAttendBwd(tag + ' 2nd call', dq2, denc, want_dq,
                  before + 2 * want_inc, 2e-5 * gmax)
  assert _SameBits(buf[b:], tail)

  # dctx in fp32 is rounded to bf16 by the wrapper: same bits out.
  buf32 = case['denc0'].cuda()
  dq3 = ext.attend_bwd(dctx32, probs, q, enc, buf32[:b], case['scale'])[0]
  buf_bf = case['denc0'].cuda()
  dq4 = ext.attend_bwd(dctx, probs, q, enc, buf_bf[:b], case['scale'])[0]
  assert _SameBits(dq3, dq4) and _SameBits(dq3, dq1)
  assert _SameBits(buf32, buf_bf)


@gpu
def test_attend_bwd_at_and_over_the_lds_limit():
  ext = _Ext()
  d = 8
  s = _MaxS(ext, d, bwd=True)
  case = _LdsEdgeCase(s, d)
  g = _Gen(6)
  dctx = _Bf16(1, d, g=g)
  want_dq, want_inc = _AttendBwdRef(dctx, case['probs'], case['q'],
                                    case['enc'], case['scale'])
  gmax = float(want_inc.abs().max())
  denc0 = torch.randn(1, s, d, generator=g) * gmax / 4
  denc = denc0.cuda()
  q = case['q'].cuda()
  dq = ext.attend_bwd(dctx.cuda(), case['probs'].float().cuda(), q,
                      case['enc'].cuda(), denc, case['scale'])[0]
  _CheckAttendBwd(f'B=1 S={s} D={d} (LDS limit)', dq, denc, want_dq,
                  denc0.double() + want_inc, 1e-5 * gmax)
  over = torch.zeros(1, s + 1, d, device='cuda')
  with pytest.raises(RuntimeError, match='LDS'):
    ext.attend_bwd(dctx.cuda(), torch.zeros(1, s + 1, device='cuda'), q,
                   over.bfloat16(), over, case['scale'])
  assert not bool(over.any())


# ---------------------------------------------------------------------------
# Rejections: every call breaks one condition that the wrapper checks
# before it allocates or launches anything.
# ---------------------------------------------------------------------------

def _GemmArgs(m=4, n=16, k=32, ldw=None):
  dev, dt = 'cuda', torch.bfloat16
  return dict(
      a=torch.ones(m, k, dtype=dt, device=dev),
      wt=torch.ones(n, ldw or k, dtype=dt, device=dev),
      pre=None, out=torch.full((m, n), 5.0, dtype=dt, device=dev),
      k=k, wt_col0=0, alpha=1.0, pre_mode=0)


def _GemmRejectCases():
  dev, dt = 'cuda', torch.bfloat16
  mk = lambda *s, **kw: torch.ones(*s, **{'dtype': dt, 'device': dev, **kw})
  return {
      'out_on_cpu': lambda: dict(out=mk(4, 16, device='cpu')),
      'out_not_bf16': lambda: dict(out=mk(4, 16, dtype=torch.float32)),
      'out_not_contiguous': lambda: dict(out=mk(4, 32)[:, ::2]),
      'out_one_dim': lambda: dict(out=mk(64)),
      'out_fewer_rows_than_a': lambda: dict(out=mk(3, 16)),
      'out_more_rows_than_a': lambda: dict(out=mk(5, 16)),
      'a_on_cpu': lambda: dict(a=mk(4, 32, device='cpu')),
      'a_wider_than_k': lambda: dict(a=mk(4, 64)),
      'k_not_multiple_of_32': lambda: dict(a=mk(4, 48), k=48,
                                           wt=mk(16, 48)),
      'wt_fewer_rows_than_n': lambda: dict(wt=mk(15, 32)),
      'wt_k_slice_out_of_bounds': lambda: dict(wt=mk(16, 56), wt_col0=32),
      'wt_negative_col0': lambda: dict(wt=mk(16, 64), wt_col0=-8),
      'ldw_not_multiple_of_8': lambda: dict(wt=mk(16, 36)),
      'wt_col0_not_multiple_of_8': lambda: dict(wt=mk(16, 40), wt_col0=4),
      'pre_mode_4': lambda: dict(pre_mode=4),
      'pre_mode_negative': lambda: dict(pre_mode=-1),
      'mode1_without_pre': lambda: dict(pre_mode=1),
      'mode1_pre_too_short': lambda: dict(pre_mode=1, pre=mk(15)),
      'mode1_pre_is_matrix': lambda: dict(pre_mode=1, pre=mk(4, 16)),
      'mode2_pre_is_row': lambda: dict(pre_mode=2, pre=mk(16)),
      'mode2_pre_fewer_rows': lambda: dict(pre_mode=2, pre=mk(3, 16)),
      'mode2_pre_transposed_shape': lambda: dict(pre_mode=2, pre=mk(16, 4)),
      'mode2_pre_on_cpu': lambda: dict(pre_mode=2,
                                       pre=mk(4, 16, device='cpu')),
      'mode2_pre_fp32': lambda: dict(pre_mode=2,
                                     pre=mk(4, 16, dtype=torch.float32)),
  }


@gpu
@pytest.mark.parametrize('name', sorted(_GemmRejectCases()))
def test_smallm_gemm_rejects(name):
  ext = _Ext()
  args = _GemmArgs()
  args.update(_GemmRejectCases()[name]())
  out = args['out']
  before = out.clone()
  with pytest.raises(RuntimeError):
    ext.smallm_gemm(args['a'], args['wt'], args['pre'], out, args['k'],
                    args['wt_col0'], args['alpha'], args['pre_mode'])
  torch.cuda.synchronize()
  assert _SameBits(out.contiguous(), before.contiguous())


def _AttendArgs(b=2, s=5, d=16):
  dev = 'cuda'
  return dict(
      dctx=torch.ones(b, d, dtype=torch.bfloat16, device=dev),
      probs=torch.full((b, s), 1.0 / s, device=dev),
      q=torch.ones(b, d, dtype=torch.bfloat16, device=dev),
      enc=torch.ones(b, s, d, dtype=torch.bfloat16, device=dev),
      pad=torch.zeros(b, s, device=dev),
      denc=torch.full((b, s, d), 3.0, device=dev))


def _AttendRejectCases():
  """name -> (overrides, applies to fwd, applies to bwd)."""
  dev, bf = 'cuda', torch.bfloat16
  mk = lambda *s, **kw: torch.ones(*s, **{'dtype': bf, 'device': dev, **kw})
  f32 = lambda *s, **kw: mk(*s, dtype=torch.float32, **kw)
  both = lambda fn: (fn, True, True)
  fwd = lambda fn: (fn, True, False)
  bwd = lambda fn: (fn, False, True)
  return {
      'd_not_multiple_of_8': both(lambda: dict(
          q=mk(2, 12), enc=mk(2, 5, 12), dctx=mk(2, 12),
          denc=f32(2, 5, 12))),
      'd_over_2048': both(lambda: dict(
          q=mk(2, 2056), enc=mk(2, 5, 2056), dctx=mk(2, 2056),
          denc=f32(2, 5, 2056))),
      'd_2560': both(lambda: dict(
          q=mk(2, 2560), enc=mk(2, 5, 2560), dctx=mk(2, 2560),
          denc=f32(2, 5, 2560))),
      's_zero': both(lambda: dict(
          enc=mk(2, 0, 16), pad=f32(2, 0), probs=f32(2, 0),
          denc=f32(2, 0, 16))),
      'q_on_cpu': both(lambda: dict(q=mk(2, 16, device='cpu'))),
      'q_fp32': both(lambda: dict(q=f32(2, 16))),
      'q_not_contiguous': both(lambda: dict(q=mk(2, 32)[:, ::2])),
      'q_three_dims': both(lambda: dict(q=mk(2, 1, 16))),
      'enc_on_cpu': both(lambda: dict(enc=mk(2, 5, 16, device='cpu'))),
      'enc_fp32': both(lambda: dict(enc=f32(2, 5, 16))),
      'enc_not_contiguous': both(lambda: dict(enc=mk(2, 5, 32)[:, :, ::2])),
      'enc_fewer_rows': both(lambda: dict(enc=mk(1, 5, 16))),
      'enc_other_d': both(lambda: dict(enc=mk(2, 5, 8))),
      'enc_two_dims': both(lambda: dict(enc=mk(2, 80))),
      'pad_on_cpu': fwd(lambda: dict(pad=f32(2, 5, device='cpu'))),
      'pad_bf16': fwd(lambda: dict(pad=mk(2, 5))),
      'pad_shorter_than_s': fwd(lambda: dict(pad=f32(2, 4))),
      'pad_fewer_rows': fwd(lambda: dict(pad=f32(1, 5))),
      'pad_not_contiguous': fwd(lambda: dict(pad=f32(2, 10)[:, ::2])),
      'probs_on_cpu': bwd(lambda: dict(probs=f32(2, 5, device='cpu'))),
      'probs_bf16': bwd(lambda: dict(probs=mk(2, 5))),
      'probs_shorter_than_s': bwd(lambda: dict(probs=f32(2, 4))),
      'probs_not_contiguous': bwd(lambda: dict(probs=f32(2, 10)[:, ::2])),
      'dctx_on_cpu': bwd(lambda: dict(dctx=mk(2, 16, device='cpu'))),
      'dctx_other_d': bwd(lambda: dict(dctx=mk(2, 8))),
      'dctx_integer': bwd(lambda: dict(dctx=mk(2, 16, dtype=torch.int32))),
      'denc_on_cpu': bwd(lambda: dict(denc=f32(2, 5, 16, device='cpu'))),
      'denc_bf16': bwd(lambda: dict(denc=mk(2, 5, 16))),
      'denc_shorter_than_s': bwd(lambda: dict(denc=f32(2, 4, 16))),
      'denc_fewer_rows': bwd(lambda: dict(denc=f32(1, 5, 16))),
      'denc_other_d': bwd(lambda: dict(denc=f32(2, 5, 8))),
      'denc_not_contiguous': bwd(lambda: dict(
          denc=f32(2, 5, 32)[:, :, ::2])),
  }


@gpu
@pytest.mark.parametrize('name', sorted(
    n for n, c in _AttendRejectCases().items() if c[1]))
def test_attend_fwd_rejects(name):
  ext = _Ext()
  args = _AttendArgs()
  args.update(_AttendRejectCases()[name][0]())
  with pytest.raises(RuntimeError):
    ext.attend_fwd(args['q'], args['enc'], args['pad'], 0.25)


@gpu
@pytest.mark.parametrize('name', sorted(
    n for n, c in _AttendRejectCases().items() if c[2]))
def test_attend_bwd_rejects(name):
  ext = _Ext()
  args = _AttendArgs()
  args.update(_AttendRejectCases()[name][0]())
  denc = args['denc']
  before = denc.clone()
  with pytest.raises(RuntimeError):
    ext.attend_bwd(args['dctx'], args['probs'], args['q'], args['enc'],
                   denc, 0.25)
  torch.cuda.synchronize()
  assert _SameBits(denc.contiguous(), before.contiguous())


# ---------------------------------------------------------------------------
# Whole recurrence against fp64
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
    # Additive mask, as in the kernel: a fully padded row attends
    # uniformly and its gradient still flows into q (masked_fill would
    # cut it).
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
# B=130 puts two rows into smallm_gemm's second m-block.
@pytest.mark.parametrize('b,l,s,h,src', [(3, 4, 21, 32, 64),
                                         (130, 2, 5, 32, 32)])
def test_decoder_recurrence_matches_fp64(b, l, s, h, src):
  """Output and every gradient of the fused recurrence against the fp64
  recurrence, with the same recurrence in bf16 torch ops (every op
  rounded) as the yardstick: err_fused <= 2 err_bf16 + 2^-8 max|ref|.
  The factor 2 allows for the gates being rounded twice (the second GEMM
  accumulates into bf16), the floor is half a bf16 ulp of the largest
  value."""
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
  fused_fn = lambda eg, w_cm0, b1, wm1, wq, enc, pad: \
      las_decoder.decoder_recurrence(eg, w_cm0, b1, wm1, wq, enc, pad, fgb,
                                     cap, src)
  want = _RunRecurrence(ref_fn, inputs, pad, w, 'cpu', torch.float64)
  eager = _RunRecurrence(ref_fn, inputs, pad, w, 'cuda', torch.bfloat16)
  fused = _RunRecurrence(fused_fn, inputs, pad, w, 'cuda', torch.bfloat16)

  failed = []
  for n in ('out',) + REC_NAMES:
    assert fused[n].shape == want[n].shape, n
    ref_max = float(want[n].abs().max())
    assert ref_max > 0, n
    e_fused = float((fused[n] - want[n]).abs().max())
    e_eager = float((eager[n] - want[n]).abs().max())
    bound = 2 * e_eager + 2.0 ** -8 * ref_max
    print(f'decoder_recurrence B={b} L={l} S={s} H={h} src={src} {n}: '
          f'fused {e_fused:.4g} bf16 eager {e_eager:.4g} '
          f'max|ref| {ref_max:.4g} bound {bound:.4g}')
    if not e_fused <= bound:
      failed.append((n, e_fused, bound))
  assert not failed, failed


# ---------------------------------------------------------------------------
# AsrDecoder falls back to the eager loop for unsupported shapes
# ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize('cell_dim,source_dim', [(48, 64), (64, 48),
                                                 (32, 2080)])
def test_asr_decoder_unsupported_shape_takes_eager_loop(cell_dim, source_dim):
  """rnn_cell_dim or source_dim no multiple of 32, or source_dim over
  2048: ComputePredictions is the per-cell loop, bit for bit."""
  import lingvo_amd.models.asr as asr_model
  from lingvo_amd.core.nested_map import NestedMap
  p = asr_model.AsrDecoder.Params().Set(
      name='dec', vocab_size=32, emb_dim=16, rnn_cell_dim=cell_dim,
      num_lstm_layers=2, source_dim=source_dim, dropout_prob=0.0,
      random_seed=5)
  p.dtype = torch.bfloat16
  torch.manual_seed(12)
  dec = p.Instantiate().to('cuda')
  b, s, l = 3, 5, 3
  g = _Gen(13)
  enc = torch.randn(b, s, source_dim, generator=g).to('cuda', torch.bfloat16)
  pad = _AttendPaddings(b, s).cuda()
  ids = torch.randint(3, 32, (b, l), generator=g).cuda()
  tgt = NestedMap(ids=ids, paddings=torch.zeros(b, l, device='cuda'))
  got = dec.ComputePredictions(dec.theta, enc, pad, tgt).atten_vecs
  want = dec._LoopPredictions(dec.theta, enc, pad, tgt).atten_vecs
  assert got.shape == (b, l, cell_dim + source_dim)
  assert bool(torch.isfinite(got).all())
  assert torch.equal(got, want)
