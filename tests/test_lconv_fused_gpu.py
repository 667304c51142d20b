"""GPU numerics of the tiled depthwise convolution and the fused LConv front.

References are float64 on the CPU from the exact bf16 inputs, with the GLU
output u left unrounded. The yardstick is the unfused route on the same
inputs: F.glu -> ApplyPadding -> depthwise_conv1d(route='naive') under
autograd. A new result may be off by at most twice the yardstick's own
error plus one bf16 ulp at the array's largest magnitude (2^-20 of it for
the fp32 outputs dw, db and d pw1_b). Every case also checks that the
outputs are fully overwritten inside a canary-filled allocation, that
padded rows of dh are exactly zero and that two runs agree to the bit.
Each case prints error/bound per array.
"""

import math

import pytest
import torch
import torch.nn.functional as F

from lingvo_amd.core import py_utils

gpu = pytest.mark.gpu

CB = 64  # channels per tile of the tiled kernels


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _TT():
  return int(_Ext().dwconv_tile_len())


def _BfUlp(x):
  """One bf16 ulp at magnitude x (8 significand bits)."""
  return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


def _Pad(k, causal):
  return k - 1 if causal else (k - 1) // 2


def _Conv64(u, w, bias, pad):
  """u [B,T,D], w [K,D] float64 -> [B,T,D]."""
  k = w.shape[0]
  x = F.pad(u.permute(0, 2, 1), (pad, k - 1 - pad))
  y = F.conv1d(x, w.t().unsqueeze(1), bias, groups=u.shape[2])
  return y.permute(0, 2, 1)


def _Paddings(kind, B, T, gen):
  if kind == 'none':
    return None
  p = torch.zeros(B, T)
  if kind == 'tail':
    lens = torch.randint(1, T + 1, (B,), generator=gen)
    lens[0] = T
    p = (torch.arange(T)[None, :] >= lens[:, None]).float()
  elif kind == 'inside':  # holes in the middle, so a halo crosses them
    p = (torch.rand(B, T, generator=gen) < 0.3).float()
  elif kind == 'fullpad':
    p[B - 1] = 1.0
    if B > 1 and T > 2:
      p[0, T // 2:] = 1.0
  else:
    assert kind == 'valid'
  return p


def _Inputs(B, T, D, K, pads, bias, seed=0):
  gen = torch.Generator().manual_seed(seed)
  h = torch.randn(B, T, 2 * D, generator=gen).bfloat16()
  w = (torch.randn(K, D, generator=gen) * 0.3).bfloat16()
  b = torch.randn(D, generator=gen).bfloat16() if bias else None
  dy = torch.randn(B, T, D, generator=gen).bfloat16()
  p = _Paddings(pads, B, T, gen)
  return h, w, b, dy, p


def _Ref64(h, w, b, dy, p, pad):
  h64 = h.double().requires_grad_(True)
  w64 = w.double().requires_grad_(True)
  b64 = None if b is None else b.double().requires_grad_(True)
  u = F.glu(h64, dim=-1)
  if p is not None:
    u = u * (1.0 - p.double())[..., None]
  y = _Conv64(u, w64, b64, pad)
  y.backward(dy.double())
  out = dict(y=y.detach(), dh=h64.grad, dw=w64.grad,
             dcol=h64.grad.sum((0, 1)))
  out['db'] = dy.double().sum((0, 1))
  return out


def _Yardstick(h, w, b, dy, p, pad):
  """Unfused route on the GPU; dw/db in fp32 straight from the kernels."""
  ext = _Ext()
  hg = h.cuda().requires_grad_(True)
  u = F.glu(hg, dim=-1)
  if p is not None:
    u = py_utils.ApplyPadding(p.cuda(), u)
  wg = w.cuda()
  bg = None if b is None else b.cuda()
  y = ext.dwconv1d_fwd(u.detach().contiguous(), wg, bg, pad, 'naive')
  dx, dw, db = ext.dwconv1d_bwd(dy.cuda(), u.detach().contiguous(), wg, pad,
                                'naive')
  u.backward(dx)
  dh = hg.grad
  # autograd's bias gradient of addmm: bf16 sum over rows.
  dcol = dh.reshape(-1, dh.shape[-1]).sum(0)
  return dict(y=y, dh=dh, dw=dw, db=db, dcol=dcol)


def _Canaried(shape, dtype):
  """A NaN-filled tensor of `shape` inside a canary-filled allocation."""
  n = math.prod(shape)
  guard = 64  # elements; keeps the inside 16-byte aligned for both dtypes
  itype = torch.int16 if dtype == torch.bfloat16 else torch.int32
  whole = torch.empty(guard + n + guard, device='cuda', dtype=dtype)
  canary = (torch.arange(whole.numel(), device='cuda') % 251 + 1).to(itype)
  whole.view(itype).copy_(canary)
  inside = whole[guard:guard + n].view(shape)
  inside.fill_(float('nan'))
  return whole, canary, itype, guard, inside


def _RunFused(h, w, b, dy, p, pad):
  ext = _Ext()
  B, T, D2 = h.shape
  D, K = D2 // 2, w.shape[0]
  hg, wg, dyg = h.cuda(), w.cuda(), dy.cuda()
  bg = None if b is None else b.cuda()
  pg = None if p is None else p.cuda().bfloat16()
  shapes = dict(y=((B, T, D), torch.bfloat16),
                dh=((B, T, D2), torch.bfloat16),
                dw=((K, D), torch.float32), db=((D,), torch.float32),
                dcol=((D2,), torch.float32))
  bufs = {k: _Canaried(*v) for k, v in shapes.items()}
  ext.glu_dwconv1d_fwd(hg, pg, wg, bg, pad, 'tiled', bufs['y'][4])
  ext.glu_dwconv1d_bwd(dyg, hg, pg, wg, pad, 'tiled', bufs['dh'][4],
                       bufs['dw'][4], bufs['db'][4], bufs['dcol'][4])
  torch.cuda.synchronize()
  got = {}
  for k, (whole, canary, itype, guard, inside) in bufs.items():
    bits = whole.view(itype)
    assert torch.equal(bits[:guard], canary[:guard]), f'{k}: canary before'
    assert torch.equal(bits[-guard:], canary[-guard:]), f'{k}: canary after'
    assert bool(torch.isfinite(inside.float()).all()), f'{k}: not overwritten'
    got[k] = inside
  # Second run, fresh outputs: same bits.
  y2 = ext.glu_dwconv1d_fwd(hg, pg, wg, bg, pad)
  again = ext.glu_dwconv1d_bwd(dyg, hg, pg, wg, pad)
  for k, t in zip(('y', 'dh', 'dw', 'db', 'dcol'), [y2] + list(again)):
    assert torch.equal(t, got[k]), f'{k}: two runs differ'
  if p is not None:
    assert not bool(got['dh'][p.cuda() > 0].any()), 'padded dh rows not zero'
  return got


def _Check(name, want, yard, got):
  failures = []
  for k in ('y', 'dh', 'dw', 'db', 'dcol'):
    ref = want[k]
    top = float(ref.abs().max())
    err_y = float((yard[k].double().cpu() - ref).abs().max())
    err_n = float((got[k].double().cpu() - ref).abs().max())
    slack = _BfUlp(top) if k in ('y', 'dh') else 2.0 ** -20 * top
    bound = 2 * err_y + slack
    print(f'{name} {k:4s} new {err_n:.4g} yardstick {err_y:.4g} '
          f'bound {bound:.4g} (max|ref| {top:.4g})')
    if not err_n <= bound:
      failures.append((k, err_n, bound))
  assert not failures, failures


def _Cases():
  tt = 160  # the default tile; test_tile_len_is_exported pins it
  cases = []

  def Add(B, T, D, K, causal, pads='tail', bias=True):
    cases.append(pytest.param(B, T, D, K, causal, pads, bias,
                              id=f'B{B}-T{T}-D{D}-K{K}-'
                              f'{"causal" if causal else "same"}-{pads}-'
                              f'{"bias" if bias else "nobias"}'))

  # time
  Add(2, 1, 16, 3, False, 'none')
  Add(2, 5, 16, 32, False)
  Add(2, 5, 16, 32, True, 'valid', False)
  Add(2, tt - 1, 16, 3, False)
  Add(1, tt, 16, 31, True, 'inside')
  Add(2, tt + 1, 24, 32, False, 'inside')
  Add(1, 2 * tt + 3, 8, 32, True)
  Add(2, 300, 64, 32, False)
  # taps
  Add(2, 40, 16, 1, False)
  for k in (2, 31, 32):
    Add(2, 40, 16, k, False, 'inside', k != 31)
    Add(2, 40, 16, k, True)
  Add(2, 40, 16, 3, True, 'none', False)
  # channels
  for d in (8, 24, CB, CB + 8, 512):
    Add(2, 20, d, 32 if d != 24 else 3, False, 'tail', d != CB)
  # many utterances, one tile each
  Add(130, 6, 16, 3, False)
  # More tiles than weight-gradient partial groups (1536 per 64-channel
  # block, over all blocks), so a workgroup of dwconv_tiled_dw_kernel walks
  # several tiles with its accumulators live: 200 tiles over 192 groups
  # (uneven work), 1700 over 1536, and two tiles per utterance (200 over 192)
  # so the tile -> (b, t0) decode matters on the second pass.
  Add(200, 6, 512, 32, False)
  Add(1700, 1, 8, 3, True, 'fullpad')
  Add(100, tt + 1, 512, 32, True, 'tail', False)
  # paddings
  Add(3, 50, 16, 32, False, 'fullpad')
  Add(3, 50, 16, 32, True, 'valid')
  return cases


@gpu
def test_tile_len_is_exported():
  assert _TT() == 160


@gpu
@pytest.mark.parametrize('B,T,D,K,causal,pads,bias', _Cases())
def test_fused_front_against_float64(B, T, D, K, causal, pads, bias):
  h, w, b, dy, p = _Inputs(B, T, D, K, pads, bias)
  pad = _Pad(K, causal)
  want = _Ref64(h, w, b, dy, p, pad)
  yard = _Yardstick(h, w, b, dy, p, pad)
  got = _RunFused(h, w, b, dy, p, pad)
  _Check(f'B{B} T{T} D{D} K{K} {"c" if causal else "s"} {pads}', want, yard,
         got)


def _PlainCases():
  tt = 160
  return [
      dict(B=2, T=50, D=64, K=3, causal=True),
      dict(B=2, T=100, D=512, K=32, causal=False),
      dict(B=1, T=37, D=256, K=31, causal=True),
      dict(B=2, T=1, D=8, K=32, causal=False),
      dict(B=2, T=5, D=24, K=32, causal=True),
      dict(B=1, T=tt - 1, D=CB + 8, K=32, causal=False),
      dict(B=1, T=tt, D=CB, K=2, causal=False),
      dict(B=2, T=tt + 1, D=16, K=31, causal=False),
      dict(B=1, T=2 * tt + 3, D=8, K=32, causal=True),
      dict(B=2, T=300, D=64, K=32, causal=False),
      # more tiles than weight-gradient partial groups (see _Cases)
      dict(B=200, T=6, D=512, K=32, causal=False),
      dict(B=1700, T=1, D=8, K=3, causal=True),
      dict(B=100, T=tt + 1, D=512, K=32, causal=True),
  ]


@gpu
@pytest.mark.parametrize('case', _PlainCases(), ids=lambda c: '-'.join(
    f'{k}{v}' for k, v in c.items()))
def test_plain_tiled_against_naive(case):
  ext = _Ext()
  B, T, D, K = case['B'], case['T'], case['D'], case['K']
  pad = _Pad(K, case['causal'])
  gen = torch.Generator().manual_seed(1)
  x = torch.randn(B, T, D, generator=gen).bfloat16()
  w = (torch.randn(K, D, generator=gen) * 0.3).bfloat16()
  b = torch.randn(D, generator=gen).bfloat16()
  dy = torch.randn(B, T, D, generator=gen).bfloat16()
  x64 = x.double().requires_grad_(True)
  y64 = _Conv64(x64, w.double(), b.double(), pad)
  y64.backward(dy.double())
  want = dict(y=y64.detach(), dx=x64.grad,
              dw=torch.einsum('btd,bjtd->jd', dy.double(), torch.stack(
                  [F.pad(x.double(), (0, 0, pad, K - 1 - pad))[:, j:j + T]
                   for j in range(K)], 1)),
              db=dy.double().sum((0, 1)))
  xg, wg, bg, dyg = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
  y = ext.dwconv1d_fwd(xg, wg, bg, pad, 'naive')
  dx, dw, db = ext.dwconv1d_bwd(dyg, xg, wg, pad, 'naive')
  res = dict(naive=dict(y=y, dx=dx, dw=dw, db=db))
  # Tiled outputs NaN-prefilled inside canary-filled allocations.
  shapes = dict(y=((B, T, D), torch.bfloat16), dx=((B, T, D), torch.bfloat16),
                dw=((K, D), torch.float32), db=((D,), torch.float32))
  bufs = {k: _Canaried(*v) for k, v in shapes.items()}
  ext.dwconv1d_fwd(xg, wg, bg, pad, 'tiled', bufs['y'][4])
  ext.dwconv1d_bwd(dyg, xg, wg, pad, 'tiled', bufs['dx'][4], bufs['dw'][4],
                   bufs['db'][4])
  torch.cuda.synchronize()
  res['tiled'] = {}
  for k, (whole, canary, itype, guard, inside) in bufs.items():
    bits = whole.view(itype)
    assert torch.equal(bits[:guard], canary[:guard]), f'{k}: canary before'
    assert torch.equal(bits[-guard:], canary[-guard:]), f'{k}: canary after'
    assert bool(torch.isfinite(inside.float()).all()), f'{k}: not overwritten'
    res['tiled'][k] = inside
  again = [ext.dwconv1d_fwd(xg, wg, bg, pad, 'tiled')] + list(
      ext.dwconv1d_bwd(dyg, xg, wg, pad, 'tiled'))
  for a, k in zip(again, ('y', 'dx', 'dw', 'db')):
    assert torch.equal(a, res['tiled'][k]), f'{k}: two runs differ'
  failures = []
  for k in ('y', 'dx', 'dw', 'db'):
    top = float(want[k].abs().max())
    err_y = float((res['naive'][k].double().cpu() - want[k]).abs().max())
    err_n = float((res['tiled'][k].double().cpu() - want[k]).abs().max())
    bound = 2 * err_y + (_BfUlp(top) if k in ('y', 'dx') else 2.0 ** -20 * top)
    print(f'{case} {k} new {err_n:.4g} yardstick {err_y:.4g} '
          f'bound {bound:.4g}')
    if not err_n <= bound:
      failures.append((k, err_n, bound))
  assert not failures, failures


@gpu
def test_host_rejections_leave_outputs_alone():
  ext = _Ext()
  B, T, D, K = 2, 6, 16, 3
  h, w, b, dy, p = _Inputs(B, T, D, K, 'tail', True)
  hg, wg, bg, dyg = h.cuda(), w.cuda(), b.cuda(), dy.cuda()
  pg = p.cuda().bfloat16()
  y = torch.full((B, T, D), 7.0, device='cuda', dtype=torch.bfloat16)
  dh = torch.full((B, T, 2 * D), 7.0, device='cuda', dtype=torch.bfloat16)
  h12 = torch.zeros(B, T, 24, device='cuda', dtype=torch.bfloat16)
  x12 = torch.zeros(B, T, 12, device='cuda', dtype=torch.bfloat16)
  w12 = torch.zeros(K, 12, device='cuda', dtype=torch.bfloat16)
  w33 = torch.zeros(33, D, device='cuda', dtype=torch.bfloat16)
  wide = torch.zeros(B, T, 4 * D, device='cuda', dtype=torch.bfloat16)
  strided = wide[..., :2 * D]
  short_pad = pg[:, :T - 1].contiguous()
  flat_pad = pg.reshape(-1)
  torch.cuda.synchronize()
  before = torch.cuda.memory_allocated()

  def Rejects(fn, *args):
    with pytest.raises(RuntimeError):
      fn(*args)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert bool((y == 7.0).all()) and bool((dh == 7.0).all())

  fwd, bwd = ext.glu_dwconv1d_fwd, ext.glu_dwconv1d_bwd
  Rejects(fwd, h12, None, w12, None, 1, 'auto', None)  # D % 8 != 0
  Rejects(fwd, hg, pg, w33, bg, 16, 'auto', y)         # K > 32
  Rejects(fwd, wide, pg, wg, bg, 1, 'auto', y)         # h.shape[-1] != 2D
  Rejects(fwd, strided, pg, wg, bg, 1, 'auto', y)      # non-contiguous h
  Rejects(bwd, dyg, strided, pg, wg, 1, 'auto', dh)
  Rejects(fwd, hg, short_pad, wg, bg, 1, 'auto', y)    # paddings not [B,T]
  Rejects(bwd, dyg, hg, flat_pad, wg, 1, 'auto', dh)
  # route='tiled' on shapes the tiled kernels do not take, and a bad route
  Rejects(ext.dwconv1d_fwd, x12, w12, None, 1, 'tiled')
  Rejects(ext.dwconv1d_fwd, dyg, w33, None, 16, 'tiled')
  Rejects(ext.dwconv1d_fwd, dyg, wg, bg, 1, 'bogus')


# ---- layer level -----------------------------------------------------------
B_, T_, D_ = 3, 24, 128


def _LConv(bf16=False, kernel_size=8):
  from lingvo_amd.layers import conformer
  torch.manual_seed(3)
  p = conformer.LConvLayer.Params().Set(name='lconv', input_dim=D_,
                                        kernel_size=kernel_size,
                                        num_groups=8)
  if bf16:
    p.fprop_dtype = torch.bfloat16
  layer = p.Instantiate()
  with torch.no_grad():
    for v in layer.parameters():  # biases and LN params start at 0
      v.add_(torch.randn_like(v) * 0.05)
  return layer.to('cuda').to(torch.bfloat16) if bf16 else layer


def _LayerGrads(layer, x, pad, wgt):
  for v in layer.parameters():
    v.grad = None
  x = x.detach().clone().requires_grad_(True)
  y = layer.FProp(layer.theta, x, pad)
  (y.float() * wgt).sum().backward()
  grads = {n: v.grad.detach().float().cpu()
           for n, v in layer.named_parameters()}
  grads['input'] = x.grad.detach().float().cpu()
  return y.detach(), grads


@gpu
def test_lconv_layer_fusion_on_against_off(monkeypatch):
  ext = _Ext()
  ran = []
  real_fwd, real_bwd = ext.glu_dwconv1d_fwd, ext.glu_dwconv1d_bwd
  monkeypatch.setattr(ext, 'glu_dwconv1d_fwd',
                      lambda *a, **k: (ran.append('fwd'), real_fwd(*a, **k))[1])
  monkeypatch.setattr(ext, 'glu_dwconv1d_bwd',
                      lambda *a, **k: (ran.append('bwd'), real_bwd(*a, **k))[1])
  layer = _LConv()
  g = torch.Generator().manual_seed(4)
  x = torch.randn(B_, T_, D_, generator=g)
  wgt = torch.randn(B_, T_, D_, generator=g)
  pad = (torch.arange(T_)[None, :] >=
         torch.tensor([24, 17, 5])[:, None]).float()
  y_ref, g_ref = _LayerGrads(layer, x, pad, wgt)  # fp32 CPU layer
  dev = _LConv(bf16=True)  # same seed, same values
  res = {}
  for fused in (True, False):
    prev = py_utils.SetGlueFusion(fused)
    try:
      res[fused] = _LayerGrads(dev, x.cuda().bfloat16(), pad.cuda(),
                               wgt.cuda())
    finally:
      py_utils.SetGlueFusion(prev)
    # The fused node ran once each way with fusion on, and not with it off.
    assert ran == ['fwd', 'bwd'], (fused, ran)
  y_on, y_off = res[True][0].float(), res[False][0].float()
  ulp = _BfUlp(float(y_off.abs().max()))
  print(f'forward on-vs-off max diff {float((y_on - y_off).abs().max()):.4g} '
        f'ulp {ulp:.4g}')
  assert float((y_on - y_off).abs().max()) <= ulp
  for fused in (True, False):
    for name, want in g_ref.items():
      got = res[fused][1][name]
      scale = max(1.0, float(want.abs().max()))
      err = float((got - want).abs().max()) / scale
      print(f'fusion={fused} {name}: scaled err {err:.4g}')
      assert err < 0.05, (fused, name, err)


def _Blocks():
  from lingvo_amd.layers import conformer
  torch.manual_seed(5)
  p = conformer.ConformerLayer.Params().Set(
      input_dim=D_, atten_num_heads=2, kernel_size=8, dropout_prob=0.1)
  layers = []
  for i in range(2):
    q = p.Copy().Set(name=f'blk{i}')
    q.fprop_dtype = torch.bfloat16
    layer = q.Instantiate()
    for v in layer.parameters():
      with torch.no_grad():
        v.add_(torch.randn_like(v) * 0.05)
    layer = layer.to('cuda').to(torch.bfloat16)
    layer.train()
    layers.append(layer)
  return layers


def _Step(layers, x, pad, w):
  with py_utils.StepSeedScope(1234, 3):
    h = x
    for layer in layers:
      h = layer.FProp(layer.theta, h, pad)
    loss = (h.float() * w).sum() / B_
  loss.backward()
  return loss


@gpu
def test_captured_conformer_step_returns_eager_loss(monkeypatch):
  ext = _Ext()
  calls = []
  real = ext.glu_dwconv1d_bwd

  def Spy(*args, **kwargs):
    calls.append(1)
    return real(*args, **kwargs)

  monkeypatch.setattr(ext, 'glu_dwconv1d_bwd', Spy)
  assert py_utils.GlueFusion()
  layers = _Blocks()
  g = torch.Generator().manual_seed(9)
  x = torch.randn(B_, T_, D_, generator=g)
  pad = (torch.arange(T_)[None, :] >=
         torch.tensor([24, 17, 5])[:, None]).float().cuda()
  w = torch.randn(B_, T_, D_, generator=g).cuda()

  def Fresh():
    for layer in layers:
      for v in layer.parameters():
        v.grad = None
    return x.to('cuda', torch.bfloat16).requires_grad_(True)

  eager = float(_Step(layers, Fresh(), pad, w).detach())
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    _Step(layers, Fresh(), pad, w)  # warm-up on the capture side
  torch.cuda.current_stream().wait_stream(side)
  static_x = Fresh()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    static_loss = _Step(layers, static_x, pad, w)
  graph.replay()
  torch.cuda.synchronize()
  assert len(calls) == 6  # two blocks, three steps: the fused front ran
  assert bool(torch.isfinite(static_x.grad.float()).all())
  assert float(static_loss.detach()) == eager


@gpu
def test_empty_batch_is_a_noop():
  ext = _Ext()
  D, K = 16, 3
  x = torch.zeros(0, 5, D, device='cuda', dtype=torch.bfloat16)
  w = torch.ones(K, D, device='cuda', dtype=torch.bfloat16)
  for route in ('auto', 'naive', 'tiled'):
    assert ext.dwconv1d_fwd(x, w, None, 1, route).shape == x.shape
    dx, dw, db = ext.dwconv1d_bwd(x, x, w, 1, route)
    assert dx.shape == x.shape
    assert not bool(dw.any()) and not bool(db.any())
  # The LConv front sends an empty batch down the unfused sequence.
  pw1_w = torch.ones(D, 2 * D, device='cuda', dtype=torch.bfloat16)
  pw1_b = torch.zeros(2 * D, device='cuda', dtype=torch.bfloat16)
  y = py_utils.MatmulBiasGluDwconv(x, pw1_w, pw1_b, None, w, None)
  assert y.shape == x.shape
