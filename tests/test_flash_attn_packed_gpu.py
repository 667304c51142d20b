"""Packed-QKV flash attention: q/k/v read as strided views of the
[B,T,3*N*H] projection output, dq/dk/dv written into one dQKV buffer.

Yardstick: the same values as contiguous q/k/v through the unfused route
(py_utils.SetGlueFusion(False)), and fa._ref_attention in fp32.
"""

import math

import pytest
import torch

from lingvo_amd.core import py_utils

gpu = pytest.mark.gpu

CASES = {
    'b2_t128_n2_h64': dict(B=2, T=128, N=2, H=64),
    # T off every tile size, rel-bias, padded keys.
    't200_bias_klen137': dict(B=1, T=200, N=2, H=64, bias=True, klen=[137]),
    'b2_t130_n4_h128_klen': dict(B=2, T=130, N=4, H=128, klen=[77, 130]),
    't200_causal': dict(B=1, T=200, N=2, H=64, win_r=0),
}


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _Inputs(case):
  B, T, N, H = case['B'], case['T'], case['N'], case['H']
  g = torch.Generator().manual_seed(T * 7 + N)
  qkv = torch.randn(B, T, 3 * N * H, generator=g).to('cuda', torch.bfloat16)
  dout = torch.randn(B, T, N, H, generator=g).to('cuda', torch.bfloat16)
  klen = None
  if case.get('klen'):
    klen = torch.tensor(case['klen'], device='cuda', dtype=torch.int32)
  bias = None
  if case.get('bias'):
    bias = (torch.randn(N, 255, generator=g) * 0.3).cuda()
  return qkv, dout, klen, bias, case.get('win_l', -1), case.get('win_r', -1)


def _Split(t, n, h):
  return [x.unflatten(-1, (n, h)) for x in t.split(n * h, dim=-1)]


def _BfUlp(x):
  """One bf16 ulp at magnitude x (8 significand bits)."""
  return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


@gpu
@pytest.mark.parametrize('name', list(CASES))
def test_packed_matches_contiguous(name):
  from lingvo_amd.ops import flash_attn as fa
  case = CASES[name]
  N, H = case['N'], case['H']
  qkv, dout, klen, bias, win_l, win_r = _Inputs(case)

  # packed
  qkv_p = qkv.clone().requires_grad_(True)
  bias_p = None if bias is None else bias.clone().requires_grad_(True)
  o_p = fa.flash_attention_packed(qkv_p, N, klen, bias_p, win_l, win_r, 127)
  o_p.backward(dout)
  dq_p, dk_p, dv_p = _Split(qkv_p.grad, N, H)

  # contiguous q/k/v through the unfused route
  prev = py_utils.SetGlueFusion(False)
  try:
    q, k, v = (x.contiguous().requires_grad_(True)
               for x in _Split(qkv, N, H))
    bias_c = None if bias is None else bias.clone().requires_grad_(True)
    o_c = fa.flash_attention(q, k, v, klen, bias_c, win_l, win_r, 127)
    o_c.backward(dout)
  finally:
    py_utils.SetGlueFusion(prev)

  assert o_p.is_contiguous() and qkv_p.grad.shape == qkv.shape
  assert torch.equal(o_p, o_c)
  assert torch.equal(dk_p, k.grad)
  assert torch.equal(dv_p, v.grad)

  # fp32 reference for the order-dependent outputs.
  qr, kr, vr = (x.float().requires_grad_(True) for x in _Split(qkv, N, H))
  br = None if bias is None else bias.clone().requires_grad_(True)
  fa._ref_attention(qr, kr, vr, klen, br, win_l, win_r, 127,
                    1.0 / math.sqrt(H)).backward(dout.float())
  pairs = [('dq', dq_p, q.grad, qr.grad)]
  if bias is not None:
    pairs.append(('dbias', bias_p.grad, bias_c.grad, br.grad))
  for what, got_p, got_c, want in pairs:
    scale = max(1e-3, float(want.abs().max()))
    rel_p = float((got_p.float() - want).abs().max()) / scale
    rel_c = float((got_c.float() - want).abs().max()) / scale
    diff = float((got_p.float() - got_c.float()).abs().max())
    ulp = _BfUlp(float(got_c.float().abs().max()))
    print(f'{name} {what}: packed rel err {rel_p:.3g} contiguous '
          f'{rel_c:.3g} packed-vs-contiguous {diff:.3g} (ulp {ulp:.3g})')
    assert rel_p < 0.06 and rel_c < 0.06, (what, rel_p, rel_c)
    assert diff <= ulp, (what, diff, ulp)


def _FwdForBwd(case):
  ext = _Ext()
  N, H = case['N'], case['H']
  qkv, dout, klen, bias, win_l, win_r = _Inputs(case)
  bias_b = None if bias is None else bias.to(torch.bfloat16)
  q, k, v = _Split(qkv, N, H)
  scale = 1.0 / math.sqrt(H)
  o, lse = ext.fa_fwd(q, k, v, klen, bias_b, None, None, win_l, win_r, 127,
                      scale, 0, 0)

  def Bwd(q, k, v, *outs):
    return ext.fa_bwd(dout, q, k, v, o, lse, klen, bias_b, None, None,
                      bias is not None, win_l, win_r, 127, scale, 0, 0,
                      *outs)
  return (q, k, v), Bwd


@gpu
@pytest.mark.parametrize('name', ['t200_bias_klen137',
                                  'b2_t130_n4_h128_klen'])
def test_bwd_writes_every_output_and_nothing_else(name):
  case = CASES[name]
  B, T, N, H = case['B'], case['T'], case['N'], case['H']
  d3 = 3 * N * H
  (q, k, v), Bwd = _FwdForBwd(case)
  buf = torch.full((B, T, d3 + 8), float('nan'), device='cuda',
                   dtype=torch.bfloat16)
  canary = torch.arange(B * T * 8, device='cuda', dtype=torch.int16)
  buf[..., d3:].view(torch.int16).copy_(canary.view(B, T, 8))
  dq, dk, dv = _Split(buf[..., :d3], N, H)
  got = Bwd(q, k, v, dq, dk, dv)
  torch.cuda.synchronize()
  assert got[0].data_ptr() == dq.data_ptr()
  assert bool(torch.isfinite(buf[..., :d3].float()).all())
  assert torch.equal(buf[..., d3:].view(torch.int16).reshape(-1), canary)
  # and they are the values of the dense call
  want = Bwd(q, k, v)
  assert torch.equal(dk, want[1]) and torch.equal(dv, want[2])
  assert float((dq.float() - want[0].float()).abs().max()) <= _BfUlp(
      float(want[0].float().abs().max()))


@gpu
def test_host_rejections_leave_outputs_untouched():
  case = CASES['b2_t128_n2_h64']
  B, T, N, H = case['B'], case['T'], case['N'], case['H']
  d3 = 3 * N * H
  (q, k, v), Bwd = _FwdForBwd(case)

  def NanBuf(*shape):
    return torch.full(shape, float('nan'), device='cuda',
                      dtype=torch.bfloat16)

  good = NanBuf(B, T, d3)
  odd = NanBuf(B, T, d3 + 4)             # row stride not a multiple of 8
  flat = NanBuf(B * T * d3 + 8)
  shifted = flat[4:4 + B * T * d3].view(B, T, d3)   # base 8 bytes off
  wide = NanBuf(B, T, 3 * N, 2 * H)      # [N][H] not dense
  outs = {
      'stride': _Split(odd[..., :d3], N, H),
      'align': _Split(shifted, N, H),
      'dense': list(wide[..., :H].split(N, dim=2)),
  }
  bufs = (good, odd, flat, wide)
  before = [b.view(torch.int16).clone() for b in bufs]
  gq, gk, gv = _Split(good, N, H)
  for why, (bq, bk, bv) in outs.items():
    assert bq.shape == q.shape, why
    with pytest.raises(RuntimeError):
      Bwd(q, k, v, bq, gk, gv)           # bad dq_out
    with pytest.raises(RuntimeError):
      Bwd(q, k, v, gq, gk, bv)           # bad dv_out
    with pytest.raises(RuntimeError):
      Bwd(bq, k, v, gq, gk, gv)          # bad q
    with pytest.raises(RuntimeError):
      _Ext().fa_fwd(q, bk, v, None, None, None, None, -1, -1, 127, 0.125,
                    0, 0)                # bad k, forward
  with pytest.raises(RuntimeError):
    Bwd(q, k, v, gq, gk)                 # outputs come together
  torch.cuda.synchronize()
  for b, was in zip(bufs, before):
    assert torch.equal(b.view(torch.int16), was)


@gpu
def test_mha_packed_matches_unfused_and_cpu():
  from lingvo_amd.layers import attention
  b, t, d = 3, 37, 128
  torch.manual_seed(11)
  ref = attention.MultiHeadedAttention.Params().Set(
      name='mha', input_dim=d, hidden_dim=d, num_heads=2).Instantiate()
  with torch.no_grad():
    for v in ref.parameters():
      v.add_(torch.randn_like(v) * 0.05)
  p = ref.p.Copy()
  p.fprop_dtype = torch.bfloat16
  layer = p.Instantiate()
  layer.load_state_dict(ref.state_dict())
  layer = layer.to('cuda').to(torch.bfloat16)
  x = torch.randn(b, t, d).bfloat16().float()
  pad = (torch.arange(t)[None, :] >=
         torch.tensor([37, 20, 9])[:, None]).float()
  w = torch.randn(b, t, d)
  names = ('qkv_w', 'qkv_b', 'post_w')

  def Run(layer, dev, dtype, fused=True):
    prev = py_utils.SetGlueFusion(fused)
    try:
      for v in layer.parameters():
        v.grad = None
      xi = x.clone().to(dev, dtype).requires_grad_(True)
      out = layer.FProp(layer.theta, xi, pad.to(dev))
      (out.float() * w.to(dev)).sum().backward()
      params = dict(layer.named_parameters())
      grads = {n: params[n].grad.float().cpu().clone() for n in names}
      grads['x'] = xi.grad.float().cpu()
      return out.detach(), grads
    finally:
      py_utils.SetGlueFusion(prev)

  _, want = Run(ref, 'cpu', torch.float32)
  out_off, g_off = Run(layer, 'cuda', torch.bfloat16, fused=False)
  out_on, g_on = Run(layer, 'cuda', torch.bfloat16, fused=True)
  assert torch.equal(out_on, out_off)
  for n, ref_g in want.items():
    scale = max(1.0, float(ref_g.abs().max()))
    e_on = float((g_on[n] - ref_g).abs().max()) / scale
    e_off = float((g_off[n] - ref_g).abs().max()) / scale
    print(f'mha {n}: scaled grad err packed {e_on:.4g} unfused {e_off:.4g}')
    assert e_on < 0.05, (n, e_on)
