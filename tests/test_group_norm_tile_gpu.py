"""GPU numerics of the tile-resident GroupNorm kernels (route='tile').

Reference: float64 on the CPU from the exact bf16 inputs (the construction of
tests/test_group_norm_fwd_vec_gpu.py, taken through float64 autograd for the
backward). Yardstick: the 'vec' route on the same inputs. The tile route may
be off by at most twice the yardstick's own error plus one bf16 ulp at the
largest |ref| for y and dx, and plus 2^-20 of it for the fp32 mean, rstd,
dgamma and dbeta.

Paddings: the last utterance is fully padded; with B >= 3 the first is
full-length and the ones between have a padded tail and one padded frame
inside; with B == 2 the first carries the tail and the inside frame (T >= 4),
and the full-length case is the B >= 3 shapes and the paddings=None case.
"""

import math

import pytest
import torch

gpu = pytest.mark.gpu

EPS = 1e-3
FP32 = ('mean', 'rstd', 'dgamma', 'dbeta')
NAMES = ('y', 'mean', 'rstd', 'dx', 'dgamma', 'dbeta')

# (B, T, D, G, with paddings)
SHAPES = [
    (2, 1, 64, 8, True),      # T = 1
    (3, 37, 512, 32, True),   # production width, T no multiple of a pass
    (2, 20, 16, 2, True),     # D < 64: one narrow slab
    (2, 20, 72, 9, True),     # D % 64 != 0: narrow last slab, cg = 8
    (2, 9, 128, 2, True),     # cg = 64: one group per slab
    (2, 9, 128, 4, True),     # cg = 32
    (130, 6, 64, 4, True),    # many workgroups; the [B, 2D] partial reduce
    (2, 300, 64, 4, True),    # the bench T on one slab
    (2, 9, 64, 4, False),     # no paddings
]


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _BfUlp(x):
  return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


def _Inputs(B, T, D, with_pad=True, seed=11):
  gen = torch.Generator().manual_seed(seed)
  x = (torch.randn(B, T, D, generator=gen) * 1.5 + 0.3).bfloat16()
  dy = torch.randn(B, T, D, generator=gen).bfloat16()
  gamma = (torch.randn(D, generator=gen) * 0.2).bfloat16()
  beta = (torch.randn(D, generator=gen) * 0.2).bfloat16()
  if not with_pad:
    return x, dy, gamma, beta, None
  lens = torch.randint(max(1, T // 2), T + 1, (B,), generator=gen)
  lens[0] = T
  lens[B - 1] = 0  # fully padded: count clamps to 1, outputs 0
  pad = (torch.arange(T)[None, :] >= lens[:, None]).float()
  if T >= 4:
    if B == 2:
      pad[0, T - 1] = 1.0  # a padded tail on the first utterance
    for b in range(0 if B == 2 else 1, B - 1):
      pad[b, 1] = 1.0      # a padded frame inside
  return x, dy, gamma, beta, pad.bfloat16()


def _Ref64(x, dy, gamma, beta, pad, G, act):
  """Forward as in test_group_norm_fwd_vec_gpu._Ref64, backward by float64
  autograd."""
  B, T, D = x.shape
  cg = D // G
  x64 = x.double().requires_grad_(True)
  g64 = gamma.double().requires_grad_(True)
  b64 = beta.double().requires_grad_(True)
  p64 = torch.zeros(B, T, dtype=torch.float64) if pad is None else pad.double()
  keep = (1.0 - p64)[..., None]                        # [B,T,1]
  xg = x64.view(B, T, G, cg)
  cnt = (keep.sum(1) * cg).clamp(min=1.0)              # [B,1]
  mean = (xg * keep[..., None]).sum((1, 3)) / cnt      # [B,G]
  msq = (xg * xg * keep[..., None]).sum((1, 3)) / cnt
  rstd = (msq - mean * mean + EPS).rsqrt()
  xhat = (xg - mean[:, None, :, None]) * rstd[:, None, :, None]
  y = xhat.reshape(B, T, D) * (1.0 + g64) + b64
  if act:
    y = y * torch.sigmoid(y)
  y = y * keep
  y.backward(dy.double())
  return dict(y=y.detach(), mean=mean.detach().reshape(-1),
              rstd=rstd.detach().reshape(-1), dx=x64.grad, dgamma=g64.grad,
              dbeta=b64.grad)


def _Run(ext, dev, G, act, route):
  x, dy, gamma, beta, pad = dev
  y, mean, rstd = ext.group_norm_fwd(x, gamma, beta, pad, G, EPS, act, route)
  dx, dgamma, dbeta = ext.group_norm_bwd(dy, x, gamma, beta, pad, mean, rstd,
                                         G, act, route)
  return dict(y=y, mean=mean, rstd=rstd, dx=dx, dgamma=dgamma, dbeta=dbeta)


def _NanFreedBlocks(B, T, D, G):
  """Leaves NaN in freed allocator blocks of every size the tile route
  requests, so that its outputs and workspace start from NaN."""
  blocks = [torch.full(s, float('nan'), device='cuda', dtype=dt)
            for _ in range(2)
            for s, dt in (((B, T, D), torch.bfloat16),
                          ((B * G,), torch.float32), ((B * G,), torch.float32),
                          ((B, 2 * D), torch.float32),
                          ((2 * D,), torch.float32))]
  torch.cuda.synchronize()
  del blocks


def _Check(case, got, yard, want):
  failures, ratios = [], {}
  for name in NAMES:
    ref = want[name]
    top = float(ref.abs().max())
    err_y = float((yard[name].double().cpu() - ref).abs().max())
    err_n = float((got[name].double().cpu() - ref).abs().max())
    bound = 2 * err_y + (2.0 ** -20 * top if name in FP32 else _BfUlp(top))
    ratios[name] = err_n / bound if bound > 0 else 0.0
    print(f'{case} {name:6s} new {err_n:.4g} yardstick {err_y:.4g} '
          f'bound {bound:.4g}')
    if not err_n <= bound:
      failures.append((name, err_n, bound))
  assert not failures, failures
  return ratios


@gpu
@pytest.mark.parametrize('act', [0, 1], ids=['plain', 'silu'])
@pytest.mark.parametrize('B,T,D,G,with_pad', SHAPES)
def test_gn_tile_against_float64(B, T, D, G, with_pad, act):
  ext = _Ext()
  host = _Inputs(B, T, D, with_pad)
  want = _Ref64(*host, G, act)
  dev = tuple(None if t is None else t.cuda() for t in host)
  pad = dev[4]
  yard = _Run(ext, dev, G, act, 'vec')
  _NanFreedBlocks(B, T, D, G)
  got = _Run(ext, dev, G, act, 'tile')
  again = _Run(ext, dev, G, act, 'tile')
  for name in NAMES:
    assert bool(torch.isfinite(got[name].float()).all()), \
        f'{name}: not fully written'
    assert torch.equal(got[name], again[name]), f'{name}: two runs differ'
  _Check(f'B{B} T{T} D{D} G{G} act{act}', got, yard, want)
  if pad is not None:
    # The fully padded utterance: outputs exactly 0, mean 0.
    assert not bool(got['y'][B - 1].any())
    assert not bool(got['dx'][B - 1].any())
    assert not bool(got['mean'].view(B, G)[B - 1].any())
    # Padded rows elsewhere are zero too.
    assert not bool(got['y'][pad > 0].any())
    assert not bool(got['dx'][pad > 0].any())


@gpu
@pytest.mark.parametrize('backward', [False, True], ids=['fwd', 'bwd'])
def test_tile_row_limit(backward):
  ext = _Ext()
  B, D, G, act = 1, 64, 4, 1
  rows = ext.group_norm_tile_max_rows(backward)
  assert rows >= 300, rows  # the bench T must fit
  # At the limit: the numeric check of this direction's outputs.
  host = _Inputs(B, rows, D, with_pad=False)
  want = _Ref64(*host, G, act)
  dev = tuple(None if t is None else t.cuda() for t in host)
  x, dy, gamma, beta, pad = dev
  yard = _Run(ext, dev, G, act, 'vec')
  names = ('dx', 'dgamma', 'dbeta') if backward else ('y', 'mean', 'rstd')
  if backward:
    mean, rstd = yard['mean'], yard['rstd']
    got = dict(zip(names, ext.group_norm_bwd(dy, x, gamma, beta, pad, mean,
                                             rstd, G, act, 'tile')))
  else:
    got = dict(zip(names, ext.group_norm_fwd(x, gamma, beta, pad, G, EPS,
                                             act, 'tile')))
  failures = []
  for name in names:
    ref = want[name]
    top = float(ref.abs().max())
    err_y = float((yard[name].double().cpu() - ref).abs().max())
    err_n = float((got[name].double().cpu() - ref).abs().max())
    bound = 2 * err_y + (2.0 ** -20 * top if name in FP32 else _BfUlp(top))
    print(f'T{rows} {name:6s} new {err_n:.4g} yardstick {err_y:.4g} '
          f'bound {bound:.4g}')
    if not err_n <= bound:
      failures.append((name, err_n, bound))
  assert not failures, failures

  # One row more: raises before anything is allocated or launched, so
  # freed NaN blocks of the output sizes are still NaN afterwards.
  T1 = rows + 1
  host = _Inputs(B, T1, D, with_pad=False)
  x, dy, gamma, beta, pad = (None if t is None else t.cuda() for t in host)
  mean = torch.zeros(B * G, device='cuda')
  rstd = torch.ones(B * G, device='cuda')
  torch.cuda.synchronize()
  before = torch.cuda.memory_stats()['allocation.all.allocated']
  prefilled = torch.full((B, T1, D), float('nan'), device='cuda',
                         dtype=torch.bfloat16)
  ptr = prefilled.data_ptr()
  del prefilled
  with pytest.raises(RuntimeError):
    if backward:
      ext.group_norm_bwd(dy, x, gamma, beta, pad, mean, rstd, G, act, 'tile')
    else:
      ext.group_norm_fwd(x, gamma, beta, pad, G, EPS, act, 'tile')
  torch.cuda.synchronize()
  # No allocation besides the prefilled block, which still holds its NaNs.
  assert torch.cuda.memory_stats()['allocation.all.allocated'] == before + 1
  block = torch.empty((B, T1, D), device='cuda', dtype=torch.bfloat16)
  if block.data_ptr() == ptr:  # the allocator handed the same block back
    assert bool(torch.isnan(block.float()).all())


@gpu
def test_auto_past_the_row_limit_is_the_vec_route():
  from lingvo_amd.ops import group_norm as gn_ops
  ext = _Ext()
  B, D, G = 1, 64, 4
  T = min(ext.group_norm_tile_max_rows(False),
          ext.group_norm_tile_max_rows(True)) + 1
  assert not ext.group_norm_tile_supported(T, D, G)
  assert ext.group_norm_tile_supported(T - 1, D, G)
  x, dy, gamma, beta, _ = (None if t is None else t.cuda()
                           for t in _Inputs(B, T, D, with_pad=False))
  outs = {}
  for route in ('auto', 'vec'):
    xr = x.clone().requires_grad_(True)
    y = gn_ops.group_norm(xr, gamma.float(), beta.float(), None, G, EPS,
                          act='SILU', route=route)
    y.backward(dy)
    outs[route] = (y.detach(), xr.grad)
  assert torch.equal(outs['auto'][0], outs['vec'][0])
  assert torch.equal(outs['auto'][1], outs['vec'][1])


@gpu
@pytest.mark.parametrize('B,T,D,G', [(2, 9, 48, 2), (2, 9, 40, 4)],
                         ids=['cg24', 'cg10'])
def test_tile_rejects_other_group_widths(B, T, D, G):
  ext = _Ext()
  x, dy, gamma, beta, pad = (t.cuda() for t in _Inputs(B, T, D))
  assert not ext.group_norm_tile_supported(T, D, G)
  with pytest.raises(RuntimeError):
    ext.group_norm_fwd(x, gamma, beta, pad, G, EPS, 0, 'tile')
  y, mean, rstd = ext.group_norm_fwd(x, gamma, beta, pad, G, EPS, 0)
  with pytest.raises(RuntimeError):
    ext.group_norm_bwd(dy, x, gamma, beta, pad, mean, rstd, G, 0, 'tile')
  with pytest.raises(RuntimeError):
    ext.group_norm_bwd(dy, x, gamma, beta, pad, mean, rstd, G, 0, 'nope')


class _Spy:
  """The extension with the route of every GroupNorm call recorded."""

  def __init__(self, ext):
    self._ext = ext
    self.routes = []

  def __getattr__(self, name):
    fn = getattr(self._ext, name)
    if name not in ('group_norm_fwd', 'group_norm_bwd'):
      return fn

    def Recorded(*args):
      self.routes.append((name, args[-1]))
      return fn(*args)
    return Recorded


@gpu
def test_op_routes_to_tile_and_matches_cpu_layer(monkeypatch):
  from lingvo_amd.layers import bn_layers
  from lingvo_amd.core.nested_map import NestedMap
  from lingvo_amd.ops import _loader
  from lingvo_amd.ops import group_norm as gn_ops
  B, T, D, G = 3, 24, 128, 8
  x, dy, gamma, beta, pad = _Inputs(B, T, D)
  gamma, beta, pad = gamma.float(), beta.float(), pad.float()

  layer = bn_layers.GroupNormLayer.Params().Set(
      name='gn', dim=D, num_groups=G, epsilon=EPS).Instantiate()
  xc = x.float().requires_grad_(True)
  gc = gamma.clone().requires_grad_(True)
  bc = beta.clone().requires_grad_(True)
  yc = layer.FProp(NestedMap(gamma=gc, beta=bc), xc, pad, act='SILU')
  yc.backward(dy.float())

  spy = _Spy(_Ext())
  monkeypatch.setattr(_loader, 'get_ext', lambda required=True: spy)
  xg = x.cuda().requires_grad_(True)
  gg = gamma.cuda().requires_grad_(True)
  bg = beta.cuda().requires_grad_(True)
  y = gn_ops.group_norm(xg, gg, bg, pad.cuda(), G, EPS, act='SILU')
  y.backward(dy.cuda())
  assert spy.routes == [('group_norm_fwd', 'tile'), ('group_norm_bwd', 'tile')]
  assert (y.float().cpu() - yc.detach()).abs().max() < 0.05
  for name, got, want in (('dx', xg.grad, xc.grad), ('dgamma', gg.grad, gc.grad),
                          ('dbeta', bg.grad, bc.grad)):
    scale = max(1.0, float(want.abs().max()))
    err = float((got.float().cpu() - want).abs().max()) / scale
    print(f'{name} scaled error against the fp32 CPU layer {err:.4g}')
    assert err < 0.05, (name, err)


@gpu
def test_tile_route_captures_into_a_graph():
  from lingvo_amd.ops import group_norm as gn_ops
  B, T, D, G = 3, 24, 128, 8
  x0, dy, gamma, beta, pad = (t.cuda() for t in _Inputs(B, T, D))
  gamma = gamma.float().requires_grad_(True)
  beta = beta.float().requires_grad_(True)
  x_in = x0.clone().requires_grad_(True)

  def Step():
    y = gn_ops.group_norm(x_in, gamma, beta, pad, G, EPS, act='SILU',
                          route='tile')
    return (y,) + torch.autograd.grad(y, (x_in, gamma, beta), dy)

  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(2):
      Step()
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    outs = Step()
  for seed in (21, 22, 23):  # several replays, each on refreshed x
    fresh = _Inputs(B, T, D, seed=seed)[0].cuda()
    with torch.no_grad():
      x_in.copy_(fresh)
    graph.replay()
    torch.cuda.synchronize()
    replayed = [o.clone() for o in outs]
    eager = Step()
    for name, a, b in zip(('y', 'dx', 'dgamma', 'dbeta'), replayed, eager):
      assert torch.equal(a, b), f'{name}: replay differs from eager'
