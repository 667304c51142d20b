"""Fused attention forward (route='fused': one workgroup per head, K and
V^T resident in LDS, S^T = K Q^T, P fed to the second MFMA from registers).

Reference: fa._ref_attention in float64 on the same bf16-rounded inputs,
and the float64 log-sum-exp of the same masked logits. Yardstick:
route='tiles'. The worst |o - ref| of 'fused' may be at most twice the worst
error of 'tiles' on the same inputs plus one bf16 ulp at max|ref|; lse
twice the 'tiles' error plus 2^-20 max|ref|. The backward fed with the new
o and lse keeps the bound of test_flash_attn_bwd_fused_gpu.py against the
all-'tiles' pipeline.
"""

import math

import pytest
import torch

from lingvo_amd.core import py_utils

gpu = pytest.mark.gpu

H = 64
# Largest S the route takes; flash_attn.hip FWD_FUSED_MAX_S.
MAX_S = 384
NEG_INF = -1e30

CASES = {
    # T: one key, one strip, strip + 1, odd, the workload's 19 strips and
    # 5 steps of 64 keys, the route's largest.
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
    'bias_clip3_t37': dict(T=37, bias='grad', clip=3),
    'bias_clip127_t300': dict(T=300, bias='nograd', N=3),
    'bias_grad_clip127_t300': dict(T=300, bias='grad', klen=[300, 247]),
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


def _Inputs(case, nkv=None, s=None, h=H):
  B, T, N = case.get('B', 2), case['T'], case.get('N', 2)
  S = s or T
  nkv = nkv or N
  clip = case.get('clip', 127)
  g = torch.Generator().manual_seed(T * 13 + B)
  q = torch.randn(B, T, N, h, generator=g).to('cuda', torch.bfloat16)
  k = torch.randn(B, S, nkv, h, generator=g).to('cuda', torch.bfloat16)
  v = torch.randn(B, S, nkv, h, generator=g).to('cuda', torch.bfloat16)
  dout = torch.randn(B, T, N, h, generator=g).to('cuda', torch.bfloat16)
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
              scale=1.0 / math.sqrt(h))


def _Fwd(x, route, qseg=None, kseg=None, chunk=0, left=0):
  return _Ext().fa_fwd(x['q'], x['k'], x['v'], x['klen'], x['bias'], qseg,
                       kseg, x['win_l'], x['win_r'], x['clip'], x['scale'],
                       chunk, left, route=route)


def _Bwd(x, o, lse, route):
  return _Ext().fa_bwd(x['dout'], x['q'], x['k'], x['v'], o, lse, x['klen'],
                       x['bias'], None, None, x['bias_grad'], x['win_l'],
                       x['win_r'], x['clip'], x['scale'], 0, 0, route=route)


def _Ref64(x, grads=False):
  """float64 o [B,T,N,H] and lse [B,N,T] (NEG_INF on fully masked rows);
  with grads also dq, dk, dv, dbias."""
  from lingvo_amd.ops import flash_attn as fa
  qr, kr, vr = (x[n].double().requires_grad_(grads) for n in 'qkv')
  br = None
  if x['bias'] is not None:
    br = x['bias'].double().requires_grad_(grads)
  o = fa._ref_attention(qr, kr, vr, x['klen'], br, x['win_l'], x['win_r'],
                        x['clip'], x['scale'])
  with torch.no_grad():
    T, S = qr.shape[1], kr.shape[1]
    logits = torch.einsum('btnh,bsnh->bnts', qr, kr) * x['scale']
    qpos = torch.arange(T, device='cuda')[:, None]
    kpos = torch.arange(S, device='cuda')[None, :]
    if br is not None:
      d = (qpos - kpos).clamp(-x['clip'], x['clip']) + x['clip']
      logits = logits + br[:, d]
    mask = torch.ones(T, S, dtype=torch.bool, device='cuda')
    if x['win_l'] >= 0:
      mask &= kpos >= qpos - x['win_l']
    if x['win_r'] >= 0:
      mask &= kpos <= qpos + x['win_r']
    mask = mask[None, None]
    if x['klen'] is not None:
      mask = mask & (kpos[None, None] < x['klen'][:, None, None, None])
    lse = torch.logsumexp(logits.masked_fill(~mask, float('-inf')), dim=-1)
    lse = torch.where(mask.any(-1).expand_as(lse), lse,
                      torch.full_like(lse, NEG_INF))
  if not grads:
    return o.detach(), lse
  o.backward(x['dout'].double())
  return (o.detach(), lse, qr.grad, kr.grad, vr.grad,
          None if br is None else br.grad)


def _CheckFwd(name, want, tiles, fused):
  failures = []
  o_ref, lse_ref = want
  live = lse_ref > NEG_INF * 0.5
  # Fully masked rows: o exactly 0, lse exactly NEG_INF.
  for o, lse in (tiles, fused):
    assert bool((lse[~live] == NEG_INF).all())
    assert not bool(o.permute(0, 2, 1, 3)[~live].any())
  top = float(o_ref.abs().max())
  err_t = float((tiles[0].double() - o_ref).abs().max())
  err_f = float((fused[0].double() - o_ref).abs().max())
  bound = 2 * err_t + _BfUlp(top)
  print(f'{name} o: fused err {err_f:.4g} tiles err {err_t:.4g} '
        f'bound {bound:.4g} (max|ref| {top:.4g})')
  if not err_f <= bound:
    failures.append(('o', err_f, bound))
  if bool(live.any()):
    top = float(lse_ref[live].abs().max())
    err_t = float((tiles[1].double() - lse_ref)[live].abs().max())
    err_f = float((fused[1].double() - lse_ref)[live].abs().max())
    bound = 2 * err_t + 2.0 ** -20 * top
    print(f'{name} lse: fused err {err_f:.4g} tiles err {err_t:.4g} '
          f'bound {bound:.4g} (max|ref| {top:.4g})')
    if not err_f <= bound:
      failures.append(('lse', err_f, bound))
  assert not failures, failures


@gpu
@pytest.mark.parametrize('name', list(CASES))
def test_fused_against_fp64_and_tiles(name):
  x = _Inputs(CASES[name])
  want = _Ref64(x)
  tiles = _Fwd(x, 'tiles')
  fused = _Fwd(x, 'fused')
  again = _Fwd(x, 'fused')
  auto = _Fwd(x, 'auto')
  torch.cuda.synchronize()
  assert fused[0].shape == tiles[0].shape and fused[1].shape == tiles[1].shape
  assert bool(torch.isfinite(fused[0].float()).all())
  _CheckFwd(name, want, tiles, fused)
  # Two runs agree to the bit, and a qualifying call takes this route by
  # default.
  for a, b, c in zip(fused, again, auto):
    assert torch.equal(a, b) and torch.equal(a, c)


@gpu
@pytest.mark.parametrize('name',
                         ['t37', 't300', 'bias_grad_clip127_t300'])
def test_backward_on_the_new_lse(name):
  x = _Inputs(CASES[name])
  want = _Ref64(x, grads=True)[2:]
  o_t, lse_t = _Fwd(x, 'tiles')
  o_f, lse_f = _Fwd(x, 'fused')
  tiles = _Bwd(x, o_t, lse_t, 'tiles')
  fused = _Bwd(x, o_f, lse_f, 'fused')
  torch.cuda.synchronize()
  names = ['dq', 'dk', 'dv'] + (['dbias'] if x['bias_grad'] else [])
  failures = []
  for i, what in enumerate(names):
    ref = want[i]
    top = float(ref.abs().max())
    err_t = float((tiles[i].double() - ref).abs().max())
    err_f = float((fused[i].double() - ref).abs().max())
    slack = 2.0 ** -20 * top if what == 'dbias' else _BfUlp(top)
    bound = 2 * err_t + slack
    print(f'{name} {what}: fused err {err_f:.4g} tiles err {err_t:.4g} '
          f'bound {bound:.4g} (max|ref| {top:.4g})')
    if not err_f <= bound:
      failures.append((what, err_f, bound))
  assert not failures, failures


@gpu
def test_above_the_limit_takes_tiles():
  x = _Inputs(dict(T=MAX_S + 1, B=1))
  want = _Ref64(x)
  auto = _Fwd(x, 'auto')
  tiles = _Fwd(x, 'tiles')
  assert float((auto[0].double() - want[0]).abs().max()) < 0.06 * float(
      want[0].abs().max())
  assert torch.equal(auto[0], tiles[0]) and torch.equal(auto[1], tiles[1])
  with pytest.raises(RuntimeError, match='does not support'):
    _Fwd(x, 'fused')
  with pytest.raises(RuntimeError, match='unknown route'):
    _Fwd(x, 'fastest')


@gpu
@pytest.mark.parametrize('what',
                         ['gqa', 'cross', 'segments', 'chunkwise', 'h128'])
def test_disqualified_calls_stay_on_tiles(what):
  kw = {}
  if what == 'gqa':
    x = _Inputs(dict(T=64, N=4), nkv=2)
  elif what == 'cross':
    x = _Inputs(dict(T=48), s=80)
  elif what == 'h128':
    x = _Inputs(dict(T=64), h=128)
  else:
    x = _Inputs(dict(T=64))
    if what == 'segments':
      seg = (torch.arange(64, device='cuda')[None, :] >= 40).to(
          torch.int32).expand(2, 64).contiguous()
      kw = dict(qseg=seg, kseg=seg)
    else:
      kw = dict(chunk=16, left=1)
  auto = _Fwd(x, 'auto', **kw)
  tiles = _Fwd(x, 'tiles', **kw)
  for a, b in zip(auto, tiles):
    assert torch.equal(a, b)
  with pytest.raises(RuntimeError, match='does not support'):
    _Fwd(x, 'fused', **kw)


@gpu
def test_packed_inputs_with_canary():
  B, T, N = 2, 37, 2
  d3 = 3 * N * H
  g = torch.Generator().manual_seed(41)
  # The packed QKV buffer sits inside a larger allocation.
  pad = 4096
  whole = torch.randn(pad + B * T * d3 + pad, generator=g).to(
      'cuda', torch.bfloat16)
  qkv = whole[pad:pad + B * T * d3].view(B, T, d3)
  q, k, v = (t.unflatten(-1, (N, H)) for t in qkv.split(N * H, dim=-1))
  x = dict(q=q, k=k, v=v,
           klen=torch.tensor([0, 20], device='cuda', dtype=torch.int32),
           bias=(torch.randn(N, 255, generator=g) * 0.3).to('cuda',
                                                            torch.bfloat16),
           clip=127, win_l=-1, win_r=-1, scale=1.0 / math.sqrt(H))
  before = whole.clone()
  # o and lse are allocated by fa_fwd: NaN-fill and free blocks of their
  # sizes first, which the caching allocator hands back as a rule.
  for numel, dt in ((B * T * N * H, torch.bfloat16), (B * N * T, torch.float32)):
    torch.full((numel,), float('nan'), device='cuda', dtype=dt)
  o, lse = _Fwd(x, 'fused')
  torch.cuda.synchronize()
  # Every element written: no NaN is left.
  assert bool(torch.isfinite(o.float()).all())
  assert bool((torch.isfinite(lse) | (lse == NEG_INF)).all())
  assert torch.equal(whole.view(torch.int16), before.view(torch.int16))
  assert not bool(o[0].any()) and bool((lse[0] == NEG_INF).all())
  xd = dict(x, q=q.contiguous(), k=k.contiguous(), v=v.contiguous())
  od, lsed = _Fwd(xd, 'fused')
  assert torch.equal(o, od) and torch.equal(lse, lsed)


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
  real = ext.fa_fwd

  def Spy(*args, **kwargs):
    if len(args) > 13:  # route passed positionally
      kwargs['route'] = args[13]
      args = args[:13]
    routes.append(kwargs.get('route', 'auto'))
    # 'fused' raises where the call does not qualify, so the step below
    # provably runs the fused kernel.
    kwargs['route'] = 'fused'
    return real(*args, **kwargs)

  monkeypatch.setattr(ext, 'fa_fwd', Spy)
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
  for _ in range(3):
    graph.replay()
    torch.cuda.synchronize()
    assert float(static_loss.detach()) == eager
  assert len(routes) == 6 and set(routes) == {'auto'}
  assert bool(torch.isfinite(static_x.grad.float()).all())
