"""GPU numerics of the fused conv frontend (conv1_s2d_fwd / conv1_s2d_bwd,
unpad_relu, pad_scatter_relu_bwd and the ConvSubsampling route that uses
them).

References are float64 on the CPU from the exact bf16 inputs. The yardstick
is the unfused op sequence on the same inputs on the GPU (unfold-matmul +
bias + relu + s2d forward; autograd through s2d_inv, threshold_backward,
the bias sum and the K = B*t1*h1 GEMM backward). A new result may be off by
at most twice the yardstick's own error plus one bf16 ulp at the array's
largest magnitude (2^-20 of it for the fp32 outputs dw1 and db1). Each case
prints error/bound per array.
"""

import math

import pytest
import torch
import torch.nn.functional as F

from lingvo_amd.core import py_utils

gpu = pytest.mark.gpu

# (B, T, F, C)
SHAPES = [
    (2, 8, 8, 8),       # everything even
    (1, 7, 5, 8),       # h1 odd
    (2, 6, 8, 8),       # t1 odd
    (2, 1, 1, 8),       # one frame, one bin
    (3, 10, 6, 16),     # two channel octets
    (130, 4, 4, 8),     # many batch rows
    (1, 12, 8, 256),    # the bench's 32 octets per row
    (2, 300, 80, 16),   # the slice the existing layer test uses
]
BLOCKS = [(0, 1), (1, 1), (1, 0), (0, 0)]  # s -> (a, b)


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _BfUlp(x):
  """One bf16 ulp at magnitude x (8 significand bits)."""
  return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


def _Dims(T, Fq):
  t1, h1 = (T + 1) // 2, (Fq + 1) // 2
  return t1, h1, (t1 + 1) // 2, (h1 + 1) // 2


def _Inputs(B, T, Fq, C, seed=0):
  gen = torch.Generator().manual_seed(seed)
  x = torch.randn(B, T, Fq, generator=gen).bfloat16()
  w1 = (torch.randn(9, C, generator=gen) * 0.4).bfloat16()
  b1 = (torch.randn(C, generator=gen) * 0.3).bfloat16()
  return x, w1, b1


def _Taps64(x):
  """x [B,T,F] float64 -> conv1 taps [B, t1, h1, 9] (k = 3*dt + df)."""
  B, T, Fq = x.shape
  t1, h1, _, _ = _Dims(T, Fq)
  xp = F.pad(x, (1, 2, 1, 2))
  taps = [xp[:, dt:dt + 2 * t1:2, df:df + 2 * h1:2]
          for dt in range(3) for df in range(3)]
  return torch.stack(taps, -1)


def _S2d(h):
  """h [B, t1, h1, C] -> padded s2d [B, Ho+1, Wo+1, 4C], any dtype."""
  B, t1, h1, C = h.shape
  Ho, Wo = (t1 + 1) // 2, (h1 + 1) // 2
  h = F.pad(h, (0, 0, 0, 2 * Wo - h1, 0, 2 * Ho - t1))
  X = h.new_zeros(B, Ho + 1, Wo + 1, 4 * C)
  for s, (a, b) in enumerate(BLOCKS):
    X[:, 1:, 1:, s * C:(s + 1) * C] = h[:, a::2, b::2, :]
  return X


def _S2dInv(X, t1, h1):
  """padded s2d [B, Ho+1, Wo+1, 4C] -> [B, t1, h1, C]."""
  B, Hp, Wp, C4 = X.shape
  C = C4 // 4
  h = X.new_zeros(B, 2 * (Hp - 1), 2 * (Wp - 1), C)
  for s, (a, b) in enumerate(BLOCKS):
    h[:, a::2, b::2, :] = X[:, 1:, 1:, s * C:(s + 1) * C]
  return h[:, :t1, :h1, :]


def _FwdRef64(x, w1, b1):
  taps = _Taps64(x.double())
  return _S2d(F.relu(taps @ w1.double() + b1.double()))


def _UnfusedFwd(xg, w1g, b1g):
  """The present op sequence; returns (X, h1 with grad history)."""
  B, T, Fq = xg.shape
  t1, h1, _, _ = _Dims(T, Fq)
  C = w1g.shape[1]
  cols = F.unfold(xg.unsqueeze(1), kernel_size=3, stride=2, padding=1)
  h = F.relu(torch.matmul(cols.transpose(1, 2), w1g) + b1g)
  h = h.reshape(B, t1, h1, C)
  hp = F.pad(h, (0, 0, 0, h1 % 2, 0, t1 % 2))
  return _Ext().s2d_fwd(hp.contiguous()), h


def _NanFilledThenFreed(shape):
  """Leaves a NaN-filled block of this size in the caching allocator."""
  junk = torch.full(shape, float('nan'), device='cuda', dtype=torch.bfloat16)
  torch.cuda.synchronize()
  del junk


def _Report(name, key, err_n, err_y, slack, top, failures):
  bound = 2 * err_y + slack
  print(f'{name} {key:4s} new {err_n:.4g} yardstick {err_y:.4g} '
        f'bound {bound:.4g} (max|ref| {top:.4g})')
  if not err_n <= bound:
    failures.append((key, err_n, bound))


def _Id(s):
  return 'B%d-T%d-F%d-C%d' % s


@gpu
@pytest.mark.parametrize('shape', SHAPES, ids=_Id)
def test_conv1_s2d_fwd_against_float64(shape):
  B, T, Fq, C = shape
  ext = _Ext()
  x, w1, b1 = _Inputs(B, T, Fq, C)
  t1, h1, Ho, Wo = _Dims(T, Fq)
  want = _FwdRef64(x, w1, b1)
  xg, w1g, b1g = x.cuda(), w1.cuda(), b1.cuda()
  yard, _ = _UnfusedFwd(xg, w1g, b1g)
  _NanFilledThenFreed((B, Ho + 1, Wo + 1, 4 * C))
  got = ext.conv1_s2d_fwd(xg, w1g, b1g)
  torch.cuda.synchronize()
  assert got.shape == (B, Ho + 1, Wo + 1, 4 * C)
  assert bool(torch.isfinite(got.float()).all()), 'output not overwritten'
  assert torch.equal(ext.conv1_s2d_fwd(xg, w1g, b1g), got), 'two runs differ'
  # Border and odd-edge cells are exactly zero.
  dead = _S2d(torch.ones(B, t1, h1, C)) == 0
  assert not bool(got.cpu()[dead].any()), 'padding cells not zero'
  failures = []
  top = float(want.abs().max())
  _Report(_Id(shape), 'X', float((got.double().cpu() - want).abs().max()),
          float((yard.double().cpu() - want).abs().max()), _BfUlp(top), top,
          failures)
  assert not failures, failures


def _CheckBwd(shape, max_blocks=0):
  B, T, Fq, C = shape
  ext = _Ext()
  x, w1, b1 = _Inputs(B, T, Fq, C)
  t1, h1, Ho, Wo = _Dims(T, Fq)
  xg, w1g, b1g = x.cuda(), w1.cuda(), b1.cuda()
  # Yardstick first: its own X (two roundings) carries its mask.
  w1y = w1g.clone().requires_grad_(True)
  b1y = b1g.clone().requires_grad_(True)
  Xy, hy = _UnfusedFwd(xg, w1y, b1y)
  gen = torch.Generator().manual_seed(1)
  dX = torch.randn(B, Ho + 1, Wo + 1, 4 * C, generator=gen).bfloat16()
  dXg = dX.cuda()
  dh = ext.s2d_inv(dXg, C)[:, :t1, :h1, :]
  hy.backward(dh)
  # The float64 reference takes the mask the kernel is given (X itself).
  X = Xy.detach()
  g = (dX.double() * (X.cpu() > 0))
  gh = _S2dInv(g, t1, h1)
  want = dict(dw1=torch.einsum('bthk,bthc->kc', _Taps64(x.double()), gh),
              db1=gh.sum((0, 1, 2)))
  # Border cells of dX must not be read.
  dXn = dXg.clone()
  dXn[:, 0] = float('nan')
  dXn[:, :, 0] = float('nan')
  dw1, db1 = ext.conv1_s2d_bwd(dXn, X, xg, max_blocks)
  torch.cuda.synchronize()
  assert dw1.shape == (9, C) and db1.shape == (C,)
  assert dw1.dtype == torch.float32 and db1.dtype == torch.float32
  assert bool(torch.isfinite(dw1).all()) and bool(torch.isfinite(db1).all())
  again = ext.conv1_s2d_bwd(dXn, X, xg, max_blocks)
  assert torch.equal(again[0], dw1) and torch.equal(again[1], db1)
  failures = []
  for key, new, yard in (('dw1', dw1, w1y.grad), ('db1', db1, b1y.grad)):
    top = float(want[key].abs().max())
    _Report(_Id(shape), key,
            float((new.double().cpu() - want[key]).abs().max()),
            float((yard.double().cpu() - want[key]).abs().max()),
            2.0 ** -20 * top, top, failures)
  assert not failures, failures


@gpu
@pytest.mark.parametrize('shape', SHAPES, ids=_Id)
def test_conv1_s2d_bwd_against_float64(shape):
  _CheckBwd(shape)


# The grids are capped (4096 / 1024 / 2048 workgroups) and a slot then walks
# several rows; at test shapes that needs a lower cap. B*Hp rows over slots
# per workgroup: 260 / 256, 152 / 128 and 33 / 8, so with one workgroup a slot
# walks up to 2, 2 and 5 rows, and with three the last shape is uneven
# (24 slots, 33 rows).
STRIDE_SHAPES = [(130, 4, 4, 8), (2, 300, 80, 16), (3, 40, 8, 256)]


@gpu
@pytest.mark.parametrize('max_blocks', [1, 3])
@pytest.mark.parametrize('shape', STRIDE_SHAPES, ids=_Id)
def test_conv1_kernels_walk_several_rows_per_slot(shape, max_blocks):
  ext = _Ext()
  x, w1, b1 = _Inputs(*shape)
  xg, w1g, b1g = x.cuda(), w1.cuda(), b1.cuda()
  full = ext.conv1_s2d_fwd(xg, w1g, b1g)
  _NanFilledThenFreed(tuple(full.shape))
  assert torch.equal(ext.conv1_s2d_fwd(xg, w1g, b1g, max_blocks), full)
  _CheckBwd(shape, max_blocks)


# (B, Ho, Wo, Co)
OUT_SHAPES = [(2, 2, 2, 8), (1, 1, 1, 8), (3, 3, 2, 16), (130, 1, 1, 8),
              (1, 3, 2, 256), (2, 75, 20, 16)]
# max_blocks 0 is the kernel's own grid; 1 and 3 make a slot of
# pad_scatter_relu_bwd walk several of the B*(Ho+1)*(Wo+1) rows (520 / 256,
# 12 / 8 and 3192 / 128 per workgroup).
OUT_CASES = [(s, 0) for s in OUT_SHAPES] + [
    (s, m) for s in OUT_SHAPES[3:] for m in (1, 3)]


@gpu
@pytest.mark.parametrize('shape,max_blocks', OUT_CASES,
                         ids=lambda v: ('B%d-%dx%d-C%d' % v
                                        if isinstance(v, tuple) else f'g{v}'))
def test_conv2_output_side_kernels(shape, max_blocks):
  B, Ho, Wo, Co = shape
  ext = _Ext()
  gen = torch.Generator().manual_seed(2)
  O = torch.randn(B, Ho + 1, Wo + 1, Co, generator=gen).bfloat16().cuda()
  dout = torch.randn(B, Ho, Wo, Co, generator=gen).bfloat16().cuda()
  y = ext.unpad_relu(O)
  assert y.is_contiguous()
  assert torch.equal(y, F.relu(O[:, 1:, 1:, :]))
  _NanFilledThenFreed((B, Ho + 1, Wo + 1, Co))
  dO, db2 = ext.pad_scatter_relu_bwd(dout, y, max_blocks)
  assert torch.equal(dO, ext.pad_scatter((dout * (y > 0)).contiguous()))
  again = ext.pad_scatter_relu_bwd(dout, y, max_blocks)
  assert torch.equal(again[0], dO) and torch.equal(again[1], db2)
  rows = B * (Ho + 1) * (Wo + 1)
  d64 = dO.double().cpu().reshape(rows, Co)
  err = (db2.double().cpu() - d64.sum(0)).abs()
  bound = (rows - 1) * 2.0 ** -24 * d64.abs().sum(0)
  print(f'{shape} db2 worst err/bound '
        f'{float((err / bound.clamp_min(1e-300)).max()):.4g}')
  assert bool((err <= bound).all())


def _Conv2Dx64(dO, w):
  """dO [B,Ho,Wo,Co], w [3,3,C,Co] float64 -> d input [B,2Ho,2Wo,C]."""
  B, Ho, Wo, Co = dO.shape
  x = torch.zeros(B, w.shape[2], 2 * Ho, 2 * Wo, dtype=torch.float64,
                  requires_grad=True)
  out = F.conv2d(x, w.permute(3, 2, 0, 1), stride=2, padding=1)
  out.backward(dO.permute(0, 3, 1, 2))
  return x.grad.permute(0, 2, 3, 1)


@gpu
@pytest.mark.parametrize('shape', [(2, 4, 4, 8), (3, 5, 3, 16),
                                   (2, 150, 40, 16)],
                         ids=lambda s: 'B%d-%dx%d-C%d' % s)
def test_conv2_dx_cell_order_against_float64(shape):
  """dX with cell (0,0) first and beta = 0 against the present order."""
  from lingvo_amd.layers import conformer
  B, H, W, C = shape  # conv2 input [B,H,W,C], square channels
  gen = torch.Generator().manual_seed(3)
  h = F.relu(torch.randn(B, H, W, C, generator=gen)).bfloat16()
  w = (torch.randn(3, 3, C, C, generator=gen) * 0.2).bfloat16()
  bias = torch.randn(C, generator=gen).bfloat16()
  Ho, Wo = (H + 1) // 2, (W + 1) // 2
  dout = torch.randn(B, Ho, Wo, C, generator=gen).bfloat16()
  # Present order.
  hg = h.cuda().requires_grad_(True)
  wg, bg = w.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
  y_old = F.relu(conformer._Conv3x3S2Nhwc.apply(hg, wg, bg))
  y_old.backward(dout.cuda())
  # Reordered, on the s2d buffer.
  X = _S2d(h).cuda().requires_grad_(True)
  wn, bn = w.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
  y_new = conformer._Conv3x3S2ReluFromS2d.apply(X, wn, bn)
  y_new.backward(dout.cuda())
  y_new, y_old = y_new.detach(), y_old.detach()
  ulp_y = _BfUlp(float(y_old.float().abs().max()))
  assert float((y_new.float() - y_old.float()).abs().max()) <= ulp_y
  dw_top = float(wg.grad.float().abs().max())
  assert float((wn.grad.float() - wg.grad.float()).abs().max()) <= \
      _BfUlp(dw_top)
  w64 = w.double()
  want_old = _Conv2Dx64(dout.double() * (y_old.cpu() > 0),
                        w64)[:, :H, :W, :]
  want_new = _Conv2Dx64(dout.double() * (y_new.cpu() > 0),
                        w64)[:, :H, :W, :]
  new = _S2dInv(X.grad.double().cpu(), H, W)
  old = hg.grad.double().cpu()
  top = float(want_new.abs().max())
  failures = []
  _Report(str(shape), 'dx', float((new - want_new).abs().max()),
          float((old - want_old).abs().max()), _BfUlp(top), top, failures)
  assert not failures, failures
  db_err = float((bn.grad.float() - bg.grad.float()).abs().max())
  assert db_err <= _BfUlp(float(bg.grad.float().abs().max()))


@gpu
def test_host_rejections_leave_outputs_alone():
  ext = _Ext()
  x, w1, b1 = _Inputs(2, 8, 8, 8)
  xg, w1g, b1g = x.cuda(), w1.cuda(), b1.cuda()
  X = ext.conv1_s2d_fwd(xg, w1g, b1g)
  dX = torch.ones_like(X)
  w12 = torch.zeros(9, 12, device='cuda', dtype=torch.bfloat16)
  b12 = torch.zeros(12, device='cuda', dtype=torch.bfloat16)
  wide = torch.zeros(2, 8, 16, device='cuda', dtype=torch.bfloat16)
  X48 = torch.zeros(2, 3, 3, 48, device='cuda', dtype=torch.bfloat16)
  Xwide = torch.zeros(2, 3, 3, 64, device='cuda', dtype=torch.bfloat16)
  o12 = torch.zeros(2, 3, 3, 12, device='cuda', dtype=torch.bfloat16)
  xf, w1f, dXf, Xf = xg.float(), w1g.float(), dX.float(), X.float()
  x_strided, X_strided = wide[..., :8], Xwide[..., :32]
  b_short, X_short = b1g[:4], X[:, :2].contiguous()
  keep = X.clone()
  torch.cuda.synchronize()
  before = torch.cuda.memory_allocated()

  def Rejects(fn, *args):
    with pytest.raises(RuntimeError):
      fn(*args)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == before
    assert torch.equal(X, keep)

  Rejects(ext.conv1_s2d_fwd, xg, w12, b12)          # C % 8 != 0
  Rejects(ext.conv1_s2d_fwd, xf, w1g, b1g)          # fp32
  Rejects(ext.conv1_s2d_fwd, xg, w1f, b1g)
  Rejects(ext.conv1_s2d_fwd, x_strided, w1g, b1g)   # non-contiguous
  Rejects(ext.conv1_s2d_fwd, xg, w1g, b_short)      # b1 not [C]
  Rejects(ext.conv1_s2d_bwd, dX, X48, xg)           # C % 8 != 0
  Rejects(ext.conv1_s2d_bwd, dXf, X, xg)
  Rejects(ext.conv1_s2d_bwd, dX, X_strided, xg)
  Rejects(ext.conv1_s2d_bwd, dX, X, wide)           # X not from x
  Rejects(ext.unpad_relu, o12)
  Rejects(ext.unpad_relu, Xf)
  Rejects(ext.pad_scatter_relu_bwd, o12, o12)
  Rejects(ext.pad_scatter_relu_bwd, X, X_short)


@gpu
def test_empty_batch_is_a_noop():
  ext = _Ext()
  _, w1, b1 = _Inputs(1, 8, 8, 8)
  x = torch.zeros(0, 8, 8, device='cuda', dtype=torch.bfloat16)
  X = ext.conv1_s2d_fwd(x, w1.cuda(), b1.cuda())
  assert X.shape == (0, 3, 3, 32)
  dw1, db1 = ext.conv1_s2d_bwd(X, X, x)
  assert dw1.shape == (9, 8) and not bool(dw1.any()) and not bool(db1.any())
  y = ext.unpad_relu(X)
  assert y.shape == (0, 2, 2, 32)
  dO, db2 = ext.pad_scatter_relu_bwd(y, y)
  assert dO.shape == (0, 3, 3, 32) and not bool(db2.any())


# ---- layer level -----------------------------------------------------------
def _Sub(freq, ch, bf16):
  from lingvo_amd.layers import conformer
  torch.manual_seed(7)
  p = conformer.ConvSubsampling.Params().Set(
      name='sub', input_freq_dim=freq, output_dim=32, channels=ch,
      random_seed=3)
  if bf16:
    p.dtype = torch.bfloat16
  layer = p.Instantiate()
  with torch.no_grad():
    for v in layer.parameters():  # biases start at 0
      v.add_(torch.randn_like(v) * 0.05)
  return layer.to('cuda') if bf16 else layer


def _SubGrads(layer, x, pad, wgt):
  for v in layer.parameters():
    v.grad = None
  out, _ = layer.FProp(layer.theta, x, pad)
  # A loss whose gradient terms add up coherently (the loss of
  # test_conv_subsampling_gpu_matches_fp32_conv2d, under fixed positive
  # weights). With random-sign upstream gradients every conv gradient is a
  # random walk over B*T/4*F/4 positions, and the few ReLU masks that flip
  # between bf16 and fp32 then weigh sqrt(flipped fraction) ~ 5% of the
  # reference on either route, which says nothing about the kernels.
  (out.float().square() * wgt).sum().backward()
  return out.detach(), {n: v.grad.detach().float().cpu()
                        for n, v in layer.named_parameters()}


@gpu
@pytest.mark.parametrize('B,T,Fq,ch', [(4, 300, 80, 16), (3, 26, 12, 8)])
def test_conv_subsampling_fusion_on_against_off(monkeypatch, B, T, Fq, ch):
  ext = _Ext()
  ran = []
  for name in ('conv1_s2d_fwd', 'conv1_s2d_bwd', 'unpad_relu',
               'pad_scatter_relu_bwd'):
    real = getattr(ext, name)
    monkeypatch.setattr(
        ext, name,
        lambda *a, _n=name, _r=real, **k: (ran.append(_n), _r(*a, **k))[1])
  cpu = _Sub(Fq, ch, bf16=False)
  dev = _Sub(Fq, ch, bf16=True)
  g = torch.Generator().manual_seed(4)
  x = torch.randn(B, T, Fq, generator=g).bfloat16()
  t4 = ((T + 1) // 2 + 1) // 2
  wgt = torch.rand(B, t4, 32, generator=g) + 0.5
  pad = torch.zeros(B, T)
  with torch.no_grad():  # the CPU layer holds the rounded bf16 values
    for vc, vd in zip(cpu.parameters(), dev.parameters()):
      vc.copy_(vd.float().cpu())
  _, g_ref = _SubGrads(cpu, x.float(), pad, wgt)
  assert len(g_ref) == 6
  res = {}
  for fused in (True, False):
    prev = py_utils.SetGlueFusion(fused)
    try:
      res[fused] = _SubGrads(dev, x.cuda(), pad.cuda(), wgt.cuda())
    finally:
      py_utils.SetGlueFusion(prev)
    # The fused nodes ran once each with fusion on, and not with it off.
    assert ran == ['conv1_s2d_fwd', 'unpad_relu', 'pad_scatter_relu_bwd',
                   'conv1_s2d_bwd'], (fused, ran)
  # Features that require grad take the unfused sequence.
  xr = x.cuda().requires_grad_(True)
  out, _ = dev.FProp(dev.theta, xr, pad.cuda())
  out.float().sum().backward()
  assert xr.grad is not None and len(ran) == 4
  y_on, y_off = res[True][0].float(), res[False][0].float()
  ulp = _BfUlp(float(y_off.abs().max()))
  diff = float((y_on - y_off).abs().max())
  print(f'forward on-vs-off max diff {diff:.4g} ulp {ulp:.4g}')
  assert diff <= ulp
  failures = []
  for fused in (True, False):
    for name, want in g_ref.items():
      got = res[fused][1][name]
      scale = max(1e-6, float(want.abs().max()))
      err = float((got - want).abs().max()) / scale
      print(f'fusion={fused} {name}: scaled err {err:.4g} '
            f'(max|ref| {float(want.abs().max()):.4g})')
      if not err < 0.05:
        failures.append((fused, name, err))
  assert not failures, failures


# ---- capture ---------------------------------------------------------------
B_, T_, F_, D_ = 3, 48, 16, 128


def _Model():
  from lingvo_amd.layers import conformer
  torch.manual_seed(5)
  sub = conformer.ConvSubsampling.Params().Set(
      name='sub', input_freq_dim=F_, output_dim=D_, channels=D_)
  sub.fprop_dtype = torch.bfloat16
  blk = conformer.ConformerLayer.Params().Set(
      input_dim=D_, atten_num_heads=2, kernel_size=8, dropout_prob=0.1)
  layers = [sub.Instantiate()]
  for i in range(2):
    q = blk.Copy().Set(name=f'blk{i}')
    q.fprop_dtype = torch.bfloat16
    layers.append(q.Instantiate())
  for layer in layers:
    with torch.no_grad():
      for v in layer.parameters():
        v.add_(torch.randn_like(v) * 0.05)
    layer.to('cuda').to(torch.bfloat16)
    layer.train()
  return layers


def _Step(layers, x, pad, w):
  with py_utils.StepSeedScope(1234, 3):
    h, p = layers[0].FProp(layers[0].theta, x, pad)
    for layer in layers[1:]:
      h = layer.FProp(layer.theta, h, p)
    loss = (h.float() * w).sum() / B_
  loss.backward()
  return loss


@gpu
def test_captured_step_with_fused_frontend_returns_eager_loss(monkeypatch):
  ext = _Ext()
  calls = []
  real = ext.conv1_s2d_bwd
  monkeypatch.setattr(ext, 'conv1_s2d_bwd',
                      lambda *a, **k: (calls.append(1), real(*a, **k))[1])
  assert py_utils.GlueFusion()
  layers = _Model()
  g = torch.Generator().manual_seed(9)
  x = torch.randn(B_, T_, F_, generator=g).to('cuda', torch.bfloat16)
  pad = (torch.arange(T_)[None, :] >=
         torch.tensor([48, 33, 9])[:, None]).float().cuda()
  w = torch.randn(B_, T_ // 4, D_, generator=g).cuda()

  def Fresh():
    for layer in layers:
      for v in layer.parameters():
        v.grad = None

  Fresh()
  eager = float(_Step(layers, x, pad, w).detach())
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    Fresh()
    _Step(layers, x, pad, w)  # warm-up on the capture side
  torch.cuda.current_stream().wait_stream(side)
  Fresh()
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    static_loss = _Step(layers, x, pad, w)
  graph.replay()
  torch.cuda.synchronize()
  assert len(calls) == 3  # three steps: the fused frontend ran in each
  grad = layers[0].conv1_w.grad
  assert grad is not None and bool(torch.isfinite(grad.float()).all())
  assert float(static_loss.detach()) == eager
