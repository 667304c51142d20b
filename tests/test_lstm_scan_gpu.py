"""Fused LSTM scan HIP kernels (ops/hip/lstm_scan.hip) through the layer
API: numerics against the fp32 CPU loop path, graph capture and the
per-timestep launch count."""

import pytest
import torch

from lingvo_amd.layers import lstm_frnn_layer as lf

gpu = pytest.mark.gpu

DIN = 16
# Project tolerances for bf16-kernel-vs-fp32 comparisons
# (test_ops_gpu.py: outputs 0.05 absolute, gradients 0.05 after scaling
# by max(1, |want|.max())).
OUT_TOL = 0.05
GRAD_TOL = 0.05


def _Paddings(b, t):
  """Trailing pads of different lengths, one fully padded row, one row
  with a padded step in the middle (0, 1, 0) - as far as T allows."""
  pad = torch.zeros(b, t)
  pad[0, max(t - 2, 1):] = 1.0
  if t >= 4:
    pad[0, 2] = 1.0
  pad[1, max(t - 4, 0):] = 1.0
  pad[2, :] = 1.0
  return pad


def _Cell(h):
  return lf.LSTMCellSimpleExt.Params().Set(
      num_input_nodes=DIN, num_output_nodes=h, forget_gate_bias=1.0,
      cell_value_cap=10.0)


def _Layers(cls, seed, **kw):
  """fp32 CPU loop layer + bf16 GPU fused and unfused copies."""
  torch.manual_seed(seed)
  ref = cls.Params().Set(name='r', **kw).Instantiate()
  with torch.no_grad():
    for v in ref.parameters():
      if v.dim() == 1:  # gate biases (zero-initialised by default)
        v.copy_(torch.randn_like(v) * 0.5)
  out = [ref]
  for fused in (True, False):
    p = cls.Params().Set(name='g', fused_scan=fused, **kw)
    p.fprop_dtype = torch.bfloat16
    layer = p.Instantiate()
    layer.load_state_dict(ref.state_dict())
    out.append(layer.to('cuda').to(torch.bfloat16))
  return out


def _ScaledErr(got, want):
  scale = max(1.0, float(want.abs().max()))
  return float((got.float().cpu() - want).abs().max()) / scale


def _Names(layer):
  return sorted(n for n, _ in layer.named_parameters())


def _ParamGrads(layer):
  params = dict(layer.named_parameters())
  return {n: params[n].grad for n in _Names(layer)}


@gpu
# H=160: the K loop's pipelined main part (128) and its tail (32), in
# forward (K = H) and in backward (K = H per wave).
@pytest.mark.parametrize('b,h,t', [(5, 32, 7), (130, 96, 5), (16, 64, 1),
                                   (5, 160, 3)])
def test_bidirectional_fused_scan_matches_fp32(b, h, t):
  ref, fused, loop = _Layers(lf.BidirectionalLstmFRNN, 1, fwd=_Cell(h),
                             bak=_Cell(h))
  torch.manual_seed(2)
  x = torch.randn(b, t, DIN)
  pad = _Paddings(b, t)
  w = torch.randn(b, t, 2 * h)

  xr = x.clone().requires_grad_(True)
  want = ref.FProp(ref.theta, xr, pad)
  (want * w).sum().backward()
  want_g = _ParamGrads(ref)
  assert len(want_g) == 4  # wm, b for both directions

  errs = {}
  for tag, layer in (('fused', fused), ('loop', loop)):
    xg = x.cuda().bfloat16().requires_grad_(True)
    out = layer.FProp(layer.theta, xg, pad.cuda())
    (out.float() * w.cuda()).sum().backward()
    e = {'out': float((out.detach().float().cpu() - want.detach()).abs().max()),
         'dx': _ScaledErr(xg.grad, xr.grad)}
    for n, g in _ParamGrads(layer).items():
      assert g is not None, n
      e[n] = _ScaledErr(g, want_g[n])
    errs[tag] = e
    print(f'lstm_scan B={b} H={h} T={t} {tag}: ' +
          ' '.join(f'{k}={v:.4g}' for k, v in e.items()))
  e = errs['fused']
  assert e.pop('out') < OUT_TOL
  for k, v in e.items():
    assert v < GRAD_TOL, (k, v)


@gpu
def test_reverse_unidirectional_final_state_loss_matches_fp32():
  b, h, t = 5, 32, 7
  ref, fused, loop = _Layers(lf.LstmFRNN, 3, cell=_Cell(h), reverse=True)
  torch.manual_seed(4)
  x = torch.randn(b, t, DIN)
  pad = _Paddings(b, t)
  wc = torch.randn(b, h)
  wm = torch.randn(b, h)

  xr = x.clone().requires_grad_(True)
  want, want_fin = ref.FProp(ref.theta, xr, pad)
  ((want_fin.c * wc).sum() + (want_fin.m * wm).sum()).backward()
  want_g = _ParamGrads(ref)

  for tag, layer in (('fused', fused), ('loop', loop)):
    xg = x.cuda().bfloat16().requires_grad_(True)
    out, fin = layer.FProp(layer.theta, xg, pad.cuda())
    ((fin.c.float() * wc.cuda()).sum() +
     (fin.m.float() * wm.cuda()).sum()).backward()
    e = {'out': float((out.detach().float().cpu() - want.detach()).abs().max()),
         'c': float((fin.c.detach().float().cpu() - want_fin.c.detach()).abs().max()),
         'm': float((fin.m.detach().float().cpu() - want_fin.m.detach()).abs().max()),
         'dx': _ScaledErr(xg.grad, xr.grad)}
    for n, g in _ParamGrads(layer).items():
      e[n] = _ScaledErr(g, want_g[n])
    print(f'lstm_scan reverse final-state {tag}: ' +
          ' '.join(f'{k}={v:.4g}' for k, v in e.items()))
    if tag == 'fused':
      for k in ('out', 'c', 'm'):
        assert e.pop(k) < OUT_TOL, k
      for k, v in e.items():
        assert v < GRAD_TOL, (k, v)


@gpu
@pytest.mark.parametrize('which', ['m_only', 'c_only'])
def test_unidirectional_single_output_loss_matches_fp32(which):
  """Loss on the outputs alone (the scan backward gets no dc) or on the
  final c alone (no dm): the kernel's null-pointer inputs."""
  b, h, t = 5, 32, 7
  ref, fused, _ = _Layers(lf.LstmFRNN, 8, cell=_Cell(h))
  torch.manual_seed(9)
  x = torch.randn(b, t, DIN)
  pad = _Paddings(b, t)
  w = torch.randn(b, t, h) if which == 'm_only' else torch.randn(b, h)

  def Loss(out, fin, w):
    return ((out.float() if which == 'm_only' else fin.c.float()) * w).sum()

  xr = x.clone().requires_grad_(True)
  Loss(*ref.FProp(ref.theta, xr, pad), w).backward()
  want_g = _ParamGrads(ref)
  xg = x.cuda().bfloat16().requires_grad_(True)
  Loss(*fused.FProp(fused.theta, xg, pad.cuda()), w.cuda()).backward()
  e = {'dx': _ScaledErr(xg.grad, xr.grad)}
  for n, g in _ParamGrads(fused).items():
    e[n] = _ScaledErr(g, want_g[n])
  print(f'lstm_scan {which}: ' + ' '.join(f'{k}={v:.4g}' for k, v in e.items()))
  assert float(xr.grad.abs().max()) > 0
  for k, v in e.items():
    assert v < GRAD_TOL, (k, v)


def _DirectScan(device, dtype, rows, data):
  """lstm_scan called directly with a loss on both m and c."""
  from lingvo_amd.ops import lstm_scan as scan_ops
  x, wms, bs, pad, w_m, w_c = data
  x = x.clone().to(device, dtype).requires_grad_(True)
  wms = [w.clone().to(device, dtype).requires_grad_(True) for w in wms]
  bs = [v.clone().to(device, dtype).requires_grad_(True) for v in bs]
  m, c = scan_ops.lstm_scan(x, wms, bs, pad.to(device), 1.0, 10.0,
                            (False, True), rows_per_block=rows)
  ((m.float() * w_m.to(device)).sum() +
   (c.float() * w_c.to(device)).sum()).backward()
  res = {'m': m, 'c': c, 'dx': x.grad}
  for d in range(2):
    res[f'dwm{d}'] = wms[d].grad
    res[f'db{d}'] = bs[d].grad
  return {k: v.detach().float().cpu() for k, v in res.items()}


@gpu
def test_every_row_block_size_matches_fp32_and_each_other():
  """Every kernel instantiation (16/32/64/128 rows per workgroup) at
  B=130, which is no multiple of any block and crosses a 128-row edge,
  and H=256, where each of them runs its pipelined K loop (needs K >= 256,
  128, 64, 64). Each is held to the project tolerances against the fp32
  CPU scan. Among themselves they run the same operations in the same
  order on every element, so they may differ only where the compiler
  contracted an fp32 expression differently in one instantiation: a last
  fp32 bit, which can flip a bf16 rounding (2^-8 relative) and feed
  through T=3 steps. 0.02 on O(1) states (|m| <= 1, |c| a few) allows a
  few such flips; an indexing error moves elements by O(0.1..1)."""
  b, h, t = 130, 256, 3
  torch.manual_seed(10)
  bf = lambda v: v.bfloat16().float()  # values exact in bf16 on both sides
  data = (bf(torch.randn(t, b, DIN)),
          [bf(torch.randn(DIN + h, 4 * h) * 0.1) for _ in range(2)],
          [bf(torch.randn(4 * h) * 0.5) for _ in range(2)],
          _Paddings(b, t).t().contiguous(),
          torch.randn(2, t, b, h), torch.randn(2, t, b, h))
  want = _DirectScan('cpu', torch.float32, 0, data)
  got = {rows: _DirectScan('cuda', torch.bfloat16, rows, data)
         for rows in (32, 16, 64, 128)}
  for rows, res in got.items():
    errs = {k: (float((res[k] - want[k]).abs().max()) if k in ('m', 'c')
                else _ScaledErr(res[k], want[k])) for k in want}
    print(f'lstm_scan rows={rows} vs fp32: ' +
          ' '.join(f'{k}={v:.4g}' for k, v in errs.items()))
    for k, v in errs.items():
      assert v < (OUT_TOL if k in ('m', 'c') else GRAD_TOL), (rows, k, v)
  for rows in (16, 64, 128):
    for k in ('m', 'c'):
      diff = float((got[rows][k] - got[32][k]).abs().max())
      print(f'lstm_scan rows={rows} vs rows=32: {k} max diff {diff:.4g}')
      assert diff <= 0.02, (rows, k, diff)


def _FusedBi(b, h, seed=5):
  _, fused, _ = _Layers(lf.BidirectionalLstmFRNN, seed, fwd=_Cell(h),
                        bak=_Cell(h))
  return fused


def _FwdBwd(layer, x, pad, w):
  for v in layer.parameters():
    v.grad = None
  x.grad = None
  out = layer.FProp(layer.theta, x, pad)
  (out.float() * w).sum().backward()
  return out


def _EagerResult(layer, xi, pad, w):
  """(out, dx, param grads) as detached copies. Nothing of the autograd
  graph survives the call: a live graph would keep the parameters'
  AccumulateGrad nodes, which stay bound to the stream they were created
  on, and a later capture would be forked onto that stream."""
  xe = xi.clone().requires_grad_(True)
  out = _FwdBwd(layer, xe, pad, w)
  return (out.detach().clone(), xe.grad.clone(),
          {n: g.clone() for n, g in _ParamGrads(layer).items()})


@gpu
def test_fused_scan_graph_capture_replays_bit_exact():
  b, h, t = 16, 64, 6
  layer = _FusedBi(b, h)
  torch.manual_seed(6)
  pad = _Paddings(b, t).cuda()
  w = torch.randn(b, t, 2 * h, device='cuda')
  inputs = [torch.randn(b, t, DIN, device='cuda').bfloat16()
            for _ in range(2)]
  eager = [_EagerResult(layer, xi, pad, w) for xi in inputs]

  static_x = inputs[0].clone().requires_grad_(True)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    _EagerResult(layer, static_x.detach(), pad, w)  # warm-up
  torch.cuda.current_stream().wait_stream(side)
  for v in layer.parameters():
    v.grad = None
  static_x.grad = None
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    static_out = layer.FProp(layer.theta, static_x, pad)
    (static_out.float() * w).sum().backward()

  for xi, (want_out, want_dx, want_g) in zip(inputs, eager):
    with torch.no_grad():
      static_x.copy_(xi)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_out, want_out)
    assert torch.equal(static_x.grad, want_dx)
    for n, g in _ParamGrads(layer).items():
      assert torch.equal(g, want_g[n]), n


def _DeviceKernelCount(layer, b, h, t):
  from torch.profiler import ProfilerActivity, profile
  torch.manual_seed(7)
  pad = _Paddings(b, t).cuda()
  w = torch.randn(b, t, 2 * h, device='cuda')
  x = torch.randn(b, t, DIN, device='cuda').bfloat16().requires_grad_(True)
  _FwdBwd(layer, x, pad, w)  # warm-up: one-time library setup
  torch.cuda.synchronize()
  with profile(activities=[ProfilerActivity.CUDA]) as prof:
    _FwdBwd(layer, x, pad, w)
    torch.cuda.synchronize()
  return sum(1 for e in prof.events()
             if e.device_type != torch.autograd.DeviceType.CPU)


@gpu
def test_fused_scan_adds_two_launches_per_timestep():
  """One forward and one backward launch per added timestep for both
  directions together; everything else is whole-sequence work."""
  b, h = 16, 64
  layer = _FusedBi(b, h)
  n6 = _DeviceKernelCount(layer, b, h, 6)
  n12 = _DeviceKernelCount(layer, b, h, 12)
  print(f'lstm_scan device kernels: T=6 {n6}, T=12 {n12}')
  assert n6 > 0
  assert n12 - n6 <= 2 * (12 - 6)
