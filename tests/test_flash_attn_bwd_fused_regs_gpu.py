"""Fused attention backward with P and dS fed to the MFMAs from registers.

The shapes are the ones at which the kernel's indexing can go wrong: the
32-row q-tile edge (the k-slot permutation with a half-empty and a one-row
second tile), odd strip counts (dQ contracts over pairs of strips), a wave's
second and third strip, klen inside a strip, an empty row, clips narrower
and wider than a tile, windows, and sharp logits for the base-2 path.

Rule of tests/test_flash_attn_bwd_fused_gpu.py: reference is float64
fa._ref_attention under autograd on the bf16-rounded inputs, yardstick is
route='tiles' on the same inputs; the worst error of 'fused' may be at most
twice the worst error of 'tiles' plus one bf16 ulp at max|ref| (2^-20 of it
for the fp32 dbias), and the scaled error stays under 0.06.
"""

import math

import pytest
import torch

gpu = pytest.mark.gpu

B, N, H = 2, 3, 64

CASES = {
    't31': dict(T=31),
    't32': dict(T=32),
    't33': dict(T=33),
    't48': dict(T=48),
    't49': dict(T=49),
    't129': dict(T=129),
    't257': dict(T=257),
    'klen_in_strip_t70': dict(T=70, klen=[70, 41]),
    'klen_zero_row_t70': dict(T=70, klen=[0, 70]),
    'bias_grad_clip3_t70': dict(T=70, bias='grad', clip=3),
    'bias_grad_clip127_t140': dict(T=140, bias='grad', clip=127),
    'causal_t70': dict(T=70, win_r=0),
    'window_5_3_t70': dict(T=70, win_l=5, win_r=3),
    'sharp_q_x8_t70': dict(T=70, qscale=8.0, bias='grad', clip=3,
                           klen=[70, 41]),
}


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _BfUlp(x):
  """One bf16 ulp at magnitude x (8 significand bits)."""
  return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


def _Inputs(case):
  T = case['T']
  clip = case.get('clip', 127)
  g = torch.Generator().manual_seed(T * 17 + clip)
  q = (torch.randn(B, T, N, H, generator=g) * case.get('qscale', 1.0)).to(
      'cuda', torch.bfloat16)
  k = torch.randn(B, T, N, H, generator=g).to('cuda', torch.bfloat16)
  v = torch.randn(B, T, N, H, generator=g).to('cuda', torch.bfloat16)
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


def _Fwd(x):
  return _Ext().fa_fwd(x['q'], x['k'], x['v'], x['klen'], x['bias'], None,
                       None, x['win_l'], x['win_r'], x['clip'], x['scale'],
                       0, 0)


def _Bwd(x, o, lse, route, outs=()):
  return _Ext().fa_bwd(x['dout'], x['q'], x['k'], x['v'], o, lse, x['klen'],
                       x['bias'], None, None, x['bias_grad'], x['win_l'],
                       x['win_r'], x['clip'], x['scale'], 0, 0, *outs,
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


@gpu
@pytest.mark.parametrize('name', list(CASES))
def test_fused_regs_against_fp64_and_tiles(name):
  case = CASES[name]
  x = _Inputs(case)
  o, lse = _Fwd(x)
  want = _Ref64(x)
  tiles = _Bwd(x, o, lse, 'tiles')
  fused = _Bwd(x, o, lse, 'fused')
  again = _Bwd(x, o, lse, 'fused')
  auto = _Bwd(x, o, lse, 'auto')
  torch.cuda.synchronize()
  names = ['dq', 'dk', 'dv'] + (['dbias'] if x['bias_grad'] else [])
  failures = []
  for i, what in enumerate(names):
    ref = want[i]
    assert bool(torch.isfinite(fused[i].float()).all()), what
    top = float(ref.abs().max())
    err_t = float((tiles[i].double() - ref).abs().max())
    err_f = float((fused[i].double() - ref).abs().max())
    slack = 2.0 ** -20 * top if what == 'dbias' else _BfUlp(top)
    bound = 2 * err_t + slack
    rel = err_f / max(1e-3, top)
    print(f'{name} {what}: fused err {err_f:.4g} tiles err {err_t:.4g} '
          f'bound {bound:.4g} err/bound {err_f / bound:.3f} '
          f'(max|ref| {top:.4g}) rel {rel:.4g}')
    if not (err_f <= bound and rel < 0.06):
      failures.append((what, err_f, bound, rel))
  assert not failures, failures
  for a, b, c in zip(fused, again, auto):
    assert torch.equal(a, b) and torch.equal(a, c)
  if case.get('klen'):
    for b, kl in enumerate(case['klen']):
      if kl == 0:
        for t in fused[:3]:
          assert not bool(t[b].any())
      for t in fused[1:3]:  # dk, dv of padded keys
        assert not bool(t[b, kl:].any())


@gpu
@pytest.mark.parametrize('extra', [0, 40])
def test_packed_outputs_with_8_byte_stores(extra):
  # dq, dk, dv are views into one [B, T, 3, N, H] buffer (extra == 0) or into
  # rows with a stride above 3NH; canary words before, after and, with
  # extra, at the end of every token row.
  T = 33
  d3 = 3 * N * H
  row = d3 + extra
  x = _Inputs(dict(T=T, klen=[33, 18], bias='grad', clip=3))
  o, lse = _Fwd(x)
  pad = 64
  whole = torch.empty(pad + B * T * row + pad, device='cuda',
                      dtype=torch.bfloat16)
  canary = torch.arange(whole.numel(), device='cuda',
                        dtype=torch.int16) | 0x4000
  whole.view(torch.int16).copy_(canary)
  buf = whole[pad:pad + B * T * row].view(B, T, row)
  inside = torch.zeros_like(whole, dtype=torch.bool)
  inside[pad:pad + B * T * row].view(B, T, row)[..., :d3] = True
  whole[inside] = float('nan')
  outs = tuple(t.unflatten(-1, (N, H))
               for t in buf[..., :d3].split(N * H, dim=-1))
  got = _Bwd(x, o, lse, 'fused', outs)
  dense = _Bwd(x, o, lse, 'fused')
  torch.cuda.synchronize()
  assert got[0].data_ptr() == outs[0].data_ptr()
  assert bool(torch.isfinite(buf[..., :d3].float()).all())
  assert torch.equal(whole.view(torch.int16)[~inside], canary[~inside])
  for view, want in zip(outs, dense[:3]):
    assert torch.equal(view, want)
  assert torch.equal(got[3], dense[3])
  assert not bool(outs[1][1, 18:].any()) and not bool(outs[2][1, 18:].any())
