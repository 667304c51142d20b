"""dropout_bwd_colsum (dropout backward that also yields the bias gradient)
and the two linear+dropout autograd nodes built on it.

Yardsticks: ext.dropout_bwd for dx (bit-equal), an fp64 sum of dx for the
column sums, and the unfused op sequence (py_utils.SetGlueFusion(False))
for the autograd nodes.
"""

import functools

import pytest
import torch

from lingvo_amd.core import py_utils

gpu = pytest.mark.gpu

KEEP = 0.8
SEED = 12345
ACTS = {'NONE': 0, 'SWISH': 1, 'RELU': 2}


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _StepSeed():
  from lingvo_amd.ops import dropout as dropout_ops
  return dropout_ops._StepSeedBuf(torch.device('cuda', 0))


@functools.lru_cache(maxsize=None)
def _Inputs(rows, d):
  g = torch.Generator().manual_seed(rows * 4099 + d)
  dy = torch.randn(rows, d, generator=g).to('cuda', torch.bfloat16)
  x = (torch.randn(rows, d, generator=g) * 2).to('cuda', torch.bfloat16)
  pad = (torch.rand(rows, generator=g) < 0.3).to('cuda', torch.bfloat16)
  return dy, x, pad


@gpu
@pytest.mark.parametrize('with_pad', [False, True], ids=['nopad', 'pad'])
@pytest.mark.parametrize('act', list(ACTS))
@pytest.mark.parametrize('rows,d', [(1, 8), (7, 24), (257, 520),
                                    (1031, 512), (300, 2048)])
def test_colsum_kernel(rows, d, act, with_pad):
  ext = _Ext()
  dy, x, pad = _Inputs(rows, d)
  pad = pad if with_pad else None
  code = ACTS[act]
  xin = x if code else None
  args = (SEED, _StepSeed(), KEEP, code, 0.5, pad, d)
  want_dx = ext.dropout_bwd(dy, xin, *args)
  dx, colsum = ext.dropout_bwd_colsum(dy, xin, *args)
  dx2, colsum2 = ext.dropout_bwd_colsum(dy, xin, *args)
  assert colsum.dtype == torch.float32 and colsum.shape == (d,)
  assert torch.equal(dx, want_dx)
  assert torch.equal(dx, dx2) and torch.equal(colsum, colsum2)
  dx64 = dx.double()
  want = dx64.sum(0)
  # Worst-case fp32 recursive-summation bound, any order.
  bound = (rows - 1) * 2.0**-24 * dx64.abs().sum(0)
  err = (colsum.double() - want).abs()
  worst = float((err / bound.clamp_min(1e-300)).max()) if rows > 1 else 0.0
  print(f'colsum rows={rows} d={d} act={act} pad={with_pad}: '
        f'max err {float(err.max()):.3g} worst err/bound {worst:.3g}')
  assert bool((err <= bound).all()), (float(err.max()), worst)
  if with_pad:
    assert bool((dx[pad.bool()] == 0).all())


@gpu
def test_colsum_host_guards():
  ext = _Ext()
  dy, x, pad = _Inputs(7, 24)
  ss = _StepSeed()
  with pytest.raises(RuntimeError):  # D % 8 != 0
    ext.dropout_bwd_colsum(dy, None, SEED, ss, KEEP, 0, 1.0, None, 12)
  with pytest.raises(RuntimeError):  # act without the pre-activation
    ext.dropout_bwd_colsum(dy, None, SEED, ss, KEEP, 1, 1.0, None, 24)
  with pytest.raises(RuntimeError):  # pad is not [rows]
    ext.dropout_bwd_colsum(dy, None, SEED, ss, KEEP, 0, 1.0, pad[:5], 24)
  with pytest.raises(RuntimeError):  # not contiguous
    ext.dropout_bwd_colsum(dy.t(), None, SEED, ss, KEEP, 0, 1.0, None, 24)
  with pytest.raises(RuntimeError):  # fp32
    ext.dropout_bwd_colsum(dy.float(), None, SEED, ss, KEEP, 0, 1.0, None,
                           24)
  torch.cuda.synchronize()


def _RunLinear(kind, x, w, b, res, pad, g, fused):
  """One forward+backward of a helper with the switch at `fused`."""
  prev = py_utils.SetGlueFusion(fused)
  try:
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, w, b)]
    xi, wi, bi = leaves
    if kind == 'dropout':
      y = py_utils.MatmulBiasDropout(xi, wi, bi, KEEP, op_seed=7,
                                     act='SWISH')
    else:
      y = py_utils.MatmulBiasDropoutAdd(xi, wi, bi, KEEP, res, op_seed=7,
                                        scale=0.5, paddings=pad)
    y.backward(g)
    return y.detach(), [t.grad for t in leaves]
  finally:
    py_utils.SetGlueFusion(prev)


@gpu
@pytest.mark.parametrize('kind', ['dropout', 'dropout_add'])
@pytest.mark.parametrize('rows,din,dout', [(37, 64, 128), (130, 128, 64)])
def test_linear_dropout_nodes(rows, din, dout, kind):
  from lingvo_amd.ops import dropout as dropout_ops
  gen = torch.Generator().manual_seed(rows)
  bf = lambda *s: torch.randn(*s, generator=gen).to('cuda', torch.bfloat16)
  x, w, b = bf(rows, din), bf(din, dout) * 0.2, bf(dout)
  res, g = bf(rows, dout), bf(rows, dout)
  pad = (torch.rand(rows, generator=gen) < 0.3).float().cuda()

  y_on, grads_on = _RunLinear(kind, x, w, b, res, pad, g, True)
  y_off, grads_off = _RunLinear(kind, x, w, b, res, pad, g, False)
  assert torch.equal(y_on, y_off)

  # fp64 reference of the same function on the same bf16 values; the keep
  # mask is read off the kernel with the seed the helpers drew.
  s1, _ = py_utils.GenerateStepSeedPair(7)
  ones = torch.ones(rows, dout, device='cuda', dtype=torch.bfloat16)
  mask = (dropout_ops.dropout(ones, KEEP, s1) != 0).double()
  x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
  h = x64 @ w64 + b64
  if kind == 'dropout':
    y64 = torch.nn.functional.silu(h) * mask / KEEP
  else:
    y64 = res.double() + h * 0.5 * (1 - pad.double())[:, None] * mask / KEEP
  y64.backward(g.double())
  for name, ref, on, off in zip(('dx', 'dw', 'db'),
                                (x64.grad, w64.grad, b64.grad),
                                grads_on, grads_off):
    err_on = (on.double() - ref).abs()
    err_off = float((off.double() - ref).abs().max())
    bound = 2 * err_off + 2.0**-20 * ref.abs()
    print(f'{kind} {rows}x{din}x{dout} {name}: fused err '
          f'{float(err_on.max()):.3g} unfused err {err_off:.3g} '
          f'|ref| max {float(ref.abs().max()):.3g}')
    assert on.dtype == torch.bfloat16 and on.shape == ref.shape
    assert bool((err_on <= bound).all()), (name, float(err_on.max()), err_off)
