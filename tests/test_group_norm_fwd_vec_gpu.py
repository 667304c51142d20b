"""GPU numerics of the vectorised GroupNorm forward kernel.

Reference: float64 on the CPU from the exact bf16 inputs. Yardstick: the
scalar kernel (route='scalar') on the same inputs. The vector kernel may be
off by at most twice the yardstick's own error plus one bf16 ulp at the
largest |ref| for y, and plus 2^-20 of it for the fp32 mean / rstd.
"""

import math

import pytest
import torch

gpu = pytest.mark.gpu

EPS = 1e-3


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _BfUlp(x):
  return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


def _Inputs(B, T, D):
  gen = torch.Generator().manual_seed(11)
  x = (torch.randn(B, T, D, generator=gen) * 1.5 + 0.3).bfloat16()
  gamma = (torch.randn(D, generator=gen) * 0.2).bfloat16()
  beta = (torch.randn(D, generator=gen) * 0.2).bfloat16()
  lens = torch.randint(1, T + 1, (B,), generator=gen)
  lens[0] = T
  lens[B - 1] = 0  # a fully padded utterance: count clamps to 1, output 0
  pad = (torch.arange(T)[None, :] >= lens[:, None]).float().bfloat16()
  return x, gamma, beta, pad


def _Ref64(x, gamma, beta, pad, G, act):
  B, T, D = x.shape
  cg = D // G
  keep = (1.0 - pad.double())[..., None]               # [B,T,1]
  xg = x.double().view(B, T, G, cg)
  cnt = (keep.sum(1) * cg).clamp(min=1.0)              # [B,1]
  mean = (xg * keep[..., None]).sum((1, 3)) / cnt      # [B,G]
  msq = (xg * xg * keep[..., None]).sum((1, 3)) / cnt
  rstd = (msq - mean * mean + EPS).rsqrt()
  xhat = (xg - mean[:, None, :, None]) * rstd[:, None, :, None]
  y = xhat.reshape(B, T, D) * (1.0 + gamma.double()) + beta.double()
  if act:
    y = y * torch.sigmoid(y)
  return y * keep, mean.reshape(-1), rstd.reshape(-1)


@gpu
@pytest.mark.parametrize('act', [0, 1], ids=['plain', 'silu'])
@pytest.mark.parametrize('B,T,D,G', [(2, 1, 128, 8), (3, 37, 512, 32),
                                     (2, 20, 64, 8), (2, 9, 48, 2)])
def test_gn_fwd_vec_against_float64(B, T, D, G, act):
  ext = _Ext()
  x, gamma, beta, pad = _Inputs(B, T, D)
  want = _Ref64(x, gamma, beta, pad, G, act)
  args = (x.cuda(), gamma.cuda(), beta.cuda(), pad.cuda(), G, EPS, act)
  yard = ext.group_norm_fwd(*args, 'scalar')
  got = ext.group_norm_fwd(*args, 'vec')
  auto = ext.group_norm_fwd(*args)
  again = ext.group_norm_fwd(*args, 'vec')
  failures = []
  for k, name in enumerate(('y', 'mean', 'rstd')):
    assert torch.equal(got[k], auto[k]), f'{name}: auto is not the vec kernel'
    assert torch.equal(got[k], again[k]), f'{name}: two runs differ'
    assert bool(torch.isfinite(got[k].float()).all())
    ref = want[k]
    top = float(ref.abs().max())
    err_y = float((yard[k].double().cpu() - ref).abs().max())
    err_n = float((got[k].double().cpu() - ref).abs().max())
    bound = 2 * err_y + (_BfUlp(top) if name == 'y' else 2.0 ** -20 * top)
    print(f'B{B} T{T} D{D} G{G} act{act} {name:4s} new {err_n:.4g} '
          f'yardstick {err_y:.4g} bound {bound:.4g}')
    if not err_n <= bound:
      failures.append((name, err_n, bound))
  assert not failures, failures
  # The fully padded utterance: output exactly 0, mean 0, rstd from eps.
  assert not bool(got[0][B - 1].any())
  assert not bool(got[1].view(B, G)[B - 1].any())
  # Padded rows elsewhere are zero too.
  assert not bool(got[0][pad.cuda() > 0].any())


@gpu
def test_scalar_kernel_serves_other_group_widths():
  ext = _Ext()
  B, T, D, G = 2, 9, 40, 4  # cg = 10
  x, gamma, beta, pad = _Inputs(B, T, D)
  args = (x.cuda(), gamma.cuda(), beta.cuda(), pad.cuda(), G, EPS, 0)
  auto = ext.group_norm_fwd(*args)
  scalar = ext.group_norm_fwd(*args, 'scalar')
  for a, s in zip(auto, scalar):
    assert torch.equal(a, s)
  with pytest.raises(RuntimeError):
    ext.group_norm_fwd(*args, 'vec')
