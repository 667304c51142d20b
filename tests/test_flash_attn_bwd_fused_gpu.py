"""Fused attention backward (route='fused': one workgroup per head, dQ
written once as bf16, delta and the bias-gradient reduction in-kernel).

Reference: fa._ref_attention under autograd in float64 on the same
bf16-rounded inputs. Yardstick: route='tiles', the per-key-tile kernel
with fp32 dQ atomics. For each of dq, dk, dv and dbias the worst error of
'fused' may be at most twice the worst error of 'tiles' on the same
inputs plus one bf16 ulp at the array's largest magnitude (2^-20 of it for
the fp32 dbias), and the scaled error stays under 0.06.
"""

import math

import pytest
import torch

from lingvo_amd.core import py_utils

gpu = pytest.mark.gpu

H = 64
# Largest S the default fused configuration takes (8 waves x 3 strips of
# 16 keys); flash_attn.hip fused_max_s.
MAX_S = 384

CASES = {
    # T: one key, one strip, strip + 1, odd, the workload's 19 strips and
    # 5 q-tiles, the route's largest.
    't1': dict(T=1),
    't16': dict(T=16),
    't17': dict(T=17),
    't37': dict(T=37),
    't300': dict(T=300),
    't_max': dict(T=MAX_S),
    # klen
    'klen_equal_s': dict(T=100, klen=[100, 100]),
    'klen_5_of_100': dict(T=100, klen=[5, 100]),
    'klen_zero_row': dict(T=100, klen=[0, 100]),
    'klen_per_row_b4': dict(B=4, T=100, klen=[100, 63, 17, 1]),
    # bias
    'bias_nograd_t37': dict(T=37, bias='nograd'),
    'bias_grad_clip127_t300': dict(T=300, bias='grad', klen=[300, 247]),
    'bias_grad_clip3_t37': dict(T=37, bias='grad', clip=3),
    # window
    'causal_t200': dict(T=200, win_r=0),
    'local_40_20_t192': dict(T=192, win_l=40, win_r=20),
}


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _BfUlp(x):
  """One bf16 ulp at magnitude x (8 significand bits)."""
  return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


def _Inputs(case, nkv=None, s=None):
  B, T, N = case.get('B', 2), case['T'], case.get('N', 2)
  S = s or T
  nkv = nkv or N
  clip = case.get('clip', 127)
  g = torch.Generator().manual_seed(T * 13 + B)
  q = torch.randn(B, T, N, H, generator=g).to('cuda', torch.bfloat16)
  k = torch.randn(B, S, nkv, H, generator=g).to('cuda', torch.bfloat16)
  v = torch.randn(B, S, nkv, H, generator=g).to('cuda', torch.bfloat16)
  dout = torch.randn(B, T, N, H, generator=g).to('cuda', torch.bfloat16)
  klen = None
  if case.get('klen'):
    klen = torch.tensor(case['klen'], device='cuda', dtype=torch.int32)
  bias = None
  if case.get('bias'):
    bias = (torch.randn(N, 2 * clip + 1, generator=g) * 0.3).to(
        'cuda', torch.bfloat16)
  return dict(q=q, k=k, v=v, dout=dout, klen=klen, bias=bias, clip=clip,
              bias_grad=case.get('bias') == 'grad',
              win_l=case.get('win_l', -1), win_r=case.get('win_r', -1),
              scale=1.0 / math.sqrt(H))


def _Fwd(x, qseg=None, kseg=None, chunk=0, left=0):
  return _Ext().fa_fwd(x['q'], x['k'], x['v'], x['klen'], x['bias'], qseg,
                       kseg, x['win_l'], x['win_r'], x['clip'], x['scale'],
                       chunk, left)


def _Bwd(x, o, lse, route, outs=(), qseg=None, kseg=None, chunk=0, left=0):
  return _Ext().fa_bwd(x['dout'], x['q'], x['k'], x['v'], o, lse, x['klen'],
                       x['bias'], qseg, kseg, x['bias_grad'], x['win_l'],
                       x['win_r'], x['clip'], x['scale'], chunk, left, *outs,
                       route=route)


def _Ref64(x):
  """dq, dk, dv, dbias of the float64 reference."""
  from lingvo_amd.ops import flash_attn as fa
  qr, kr, vr = (x[n].double().requires_grad_(True) for n in 'qkv')
  br = None
  if x['bias'] is not None:
    br = x['bias'].double().requires_grad_(True)
  fa._ref_attention(qr, kr, vr, x['klen'], br, x['win_l'], x['win_r'],
                    x['clip'], x['scale']).backward(x['dout'].double())
  return qr.grad, kr.grad, vr.grad, None if br is None else br.grad


def _CheckAgainstTiles(name, x, want, tiles, fused):
  names = ['dq', 'dk', 'dv'] + (['dbias'] if x['bias_grad'] else [])
  failures = []
  for i, what in enumerate(names):
    ref = want[i]
    top = float(ref.abs().max())
    err_t = float((tiles[i].double() - ref).abs().max())
    err_f = float((fused[i].double() - ref).abs().max())
    slack = 2.0 ** -20 * top if what == 'dbias' else _BfUlp(top)
    bound = 2 * err_t + slack
    rel = err_f / max(1e-3, top)
    print(f'{name} {what}: fused err {err_f:.4g} tiles err {err_t:.4g} '
          f'bound {bound:.4g} (max|ref| {top:.4g}) rel {rel:.4g}')
    if not (err_f <= bound and rel < 0.06):
      failures.append((what, err_f, bound, rel))
  assert not failures, failures


@gpu
@pytest.mark.parametrize('name', list(CASES))
def test_fused_against_fp64_and_tiles(name):
  x = _Inputs(CASES[name])
  o, lse = _Fwd(x)
  want = _Ref64(x)
  tiles = _Bwd(x, o, lse, 'tiles')
  fused = _Bwd(x, o, lse, 'fused')
  again = _Bwd(x, o, lse, 'fused')
  auto = _Bwd(x, o, lse, 'auto')
  torch.cuda.synchronize()
  assert fused[3].shape == tiles[3].shape
  _CheckAgainstTiles(name, x, want, tiles, fused)
  # Fixed summation order everywhere: two runs agree to the bit, and a
  # qualifying shape takes this route by default.
  for a, b, c in zip(fused, again, auto):
    assert torch.equal(a, b) and torch.equal(a, c)
  if x['klen'] is not None:
    for b, kl in enumerate(CASES[name]['klen']):
      if kl == 0:
        for t in fused[:3]:
          assert not bool(t[b].any())
      for t in fused[1:3]:  # dk, dv of padded keys
        assert not bool(t[b, kl:].any())
  if x['bias'] is not None and not x['bias_grad']:
    assert not bool(fused[3].any())


@gpu
def test_above_the_limit_takes_tiles():
  x = _Inputs(dict(T=MAX_S + 1, B=1))
  o, lse = _Fwd(x)
  want = _Ref64(x)
  auto = _Bwd(x, o, lse, 'auto')
  for got, ref in zip(auto[:3], want):
    assert float((got.double() - ref).abs().max()) < 0.06 * max(
        1e-3, float(ref.abs().max()))
  # Same kernel as 'tiles': dk and dv are written once per element; dq
  # sums four key tiles through atomics, so it is compared to one ulp.
  tiles = _Bwd(x, o, lse, 'tiles')
  assert torch.equal(auto[1], tiles[1]) and torch.equal(auto[2], tiles[2])
  assert float((auto[0].float() - tiles[0].float()).abs().max()) <= _BfUlp(
      float(tiles[0].float().abs().max()))
  with pytest.raises(RuntimeError, match='does not support'):
    _Bwd(x, o, lse, 'fused')
  with pytest.raises(RuntimeError, match='unknown route'):
    _Bwd(x, o, lse, 'fastest')


@gpu
@pytest.mark.parametrize('what', ['gqa', 'cross', 'segments', 'chunkwise'])
def test_fallbacks_stay_on_tiles(what):
  # One key tile (S <= 128), so dq's atomics add to zero once and the old
  # route is deterministic: 'auto' must equal 'tiles' to the bit.
  kw = {}
  if what == 'gqa':
    x = _Inputs(dict(T=64, N=4), nkv=2)
  elif what == 'cross':
    x = _Inputs(dict(T=48), s=80)
  else:
    x = _Inputs(dict(T=64))
    if what == 'segments':
      seg = (torch.arange(64, device='cuda')[None, :] >= 40).to(
          torch.int32).expand(2, 64).contiguous()
      kw = dict(qseg=seg, kseg=seg)
    else:
      kw = dict(chunk=16, left=1)
  o, lse = _Fwd(x, **kw)
  auto = _Bwd(x, o, lse, 'auto', **kw)
  tiles = _Bwd(x, o, lse, 'tiles', **kw)
  for a, b in zip(auto, tiles):
    assert torch.equal(a, b)
  with pytest.raises(RuntimeError, match='does not support'):
    _Bwd(x, o, lse, 'fused', **kw)


@gpu
def test_packed_outputs_with_canary():
  B, T, N = 2, 37, 2
  d3 = 3 * N * H
  g = torch.Generator().manual_seed(41)
  qkv = torch.randn(B, T, d3, generator=g).to('cuda', torch.bfloat16)
  q, k, v = (t.unflatten(-1, (N, H)) for t in qkv.split(N * H, dim=-1))
  x = dict(q=q, k=k, v=v,
           dout=torch.randn(B, T, N, H, generator=g).to('cuda',
                                                        torch.bfloat16),
           klen=torch.tensor([0, 20], device='cuda', dtype=torch.int32),
           bias=(torch.randn(N, 255, generator=g) * 0.3).to('cuda',
                                                            torch.bfloat16),
           clip=127, bias_grad=True, win_l=-1, win_r=-1,
           scale=1.0 / math.sqrt(H))
  o, lse = _Fwd(x)
  # The packed dQKV buffer sits inside a larger allocation: canary words
  # before it, after it and at the end of every token row.
  pad = 64
  whole = torch.full((pad + B * T * (d3 + 8) + pad,), float('nan'),
                     device='cuda', dtype=torch.bfloat16)
  canary = torch.arange(whole.numel(), device='cuda',
                        dtype=torch.int16) | 0x4000
  whole.view(torch.int16).copy_(canary)
  buf = whole[pad:pad + B * T * (d3 + 8)].view(B, T, d3 + 8)
  inside = torch.zeros_like(whole, dtype=torch.bool)
  inside[pad:pad + B * T * (d3 + 8)].view(B, T, d3 + 8)[..., :d3] = True
  whole[inside] = float('nan')
  outs = tuple(t.unflatten(-1, (N, H))
               for t in buf[..., :d3].split(N * H, dim=-1))
  got = _Bwd(x, o, lse, 'fused', outs)
  torch.cuda.synchronize()
  assert got[0].data_ptr() == outs[0].data_ptr()
  assert bool(torch.isfinite(buf[..., :d3].float()).all())
  assert torch.equal(whole.view(torch.int16)[~inside], canary[~inside])
  # Every element inside was written (no NaN is left) with the values of
  # the dense call.
  dense = _Bwd(x, o, lse, 'fused')
  for view, want in zip(outs, dense[:3]):
    assert torch.equal(view, want)
  assert torch.equal(got[3], dense[3])
  assert not bool(buf[0, :, :d3].any())       # klen 0
  assert not bool(outs[1][1, 20:].any()) and not bool(outs[2][1, 20:].any())


# ---- two Conformer blocks under graph capture ------------------------------
B_, T_, D_ = 3, 24, 128


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
    for v in layer.parameters():  # biases and LN params start at 0
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
  routes = []
  real = ext.fa_bwd

  def Spy(*args, **kwargs):
    if len(args) > 20:  # route passed positionally, after the three outs
      kwargs['route'] = args[20]
      args = args[:20]
    routes.append(kwargs.get('route', 'auto'))
    # 'fused' raises where the shape does not qualify, so the step below
    # provably runs the fused kernel.
    kwargs['route'] = 'fused'
    return real(*args, **kwargs)

  monkeypatch.setattr(ext, 'fa_bwd', Spy)
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
  assert len(routes) == 6 and set(routes) == {'auto'}
  assert bool(torch.isfinite(static_x.grad.float()).all())
  assert float(static_loss.detach()) == eager
