"""Cached-attention kernels (ops/hip/attn_decode.hip) on the GPU.

Reference: the composed twin of ops/attn_decode.py in float64 on the exact
bf16 inputs. Yardstick: the same twin in fp32 (impl='torch'), whose error is
printed next to the kernel's.

Bound per element: 2^-7 * max|v| over the row's visible keys. Derived, not
measured: one bf16 rounding of the output (<= 2^-9 |ref| <= 2^-9 max|v|),
one bf16 rounding of each probability were P to go through the matrix pipe
(<= 2^-9 sum p|v| <= 2^-9 max|v|; the shipped kernel keeps P in fp32, so
this share is unused), and the same amount again for fp32 accumulation and
exp: 4 * 2^-9 = 2^-7.
"""

import pytest
import torch

from lingvo_amd.ops import attn_decode

gpu = pytest.mark.gpu


def _Ext():
  from lingvo_amd.ops import _loader
  return _loader.get_ext(required=True)


def _Inputs(B, C, N, NKV, H, Smax, seed=0, qscale=1.0):
  g = torch.Generator().manual_seed(seed * 1000 + Smax * 7 + N + C)
  q = (torch.randn(B, C, N, H, generator=g) * qscale).to('cuda',
                                                         torch.bfloat16)
  kc = torch.randn(B, Smax, NKV, H, generator=g).to('cuda', torch.bfloat16)
  vc = torch.randn(B, Smax, NKV, H, generator=g).to('cuda', torch.bfloat16)
  return q, kc, vc


def _Bias(N, clip, seed=0):
  g = torch.Generator().manual_seed(77 + seed)
  return torch.randn(N, 2 * clip + 1, generator=g).to('cuda', torch.bfloat16)


def _Visible(q_start, B, C, Smax, win_l):
  """[B, C, Smax] bool."""
  if isinstance(q_start, torch.Tensor):
    qs = q_start.long().to('cuda')
  else:
    qs = torch.full((B,), q_start, device='cuda', dtype=torch.long)
  p = qs[:, None] + torch.arange(C, device='cuda')[None, :]
  j = torch.arange(Smax, device='cuda')
  vis = j[None, None, :] <= p[:, :, None]
  if win_l >= 0:
    vis &= j[None, None, :] >= p[:, :, None] - win_l
  return vis


def _Check(label, out, q, kc, vc, q_start, bias=None, win_l=-1, clip=127):
  """Asserts |out - ref64| <= 2^-7 max|v| per element; returns the worst
  err/bound of the kernel."""
  B, C, N, H = q.shape
  Smax, NKV = kc.shape[1], kc.shape[2]
  ref = attn_decode.cached_attention(
      q.double(), kc.double(), vc.double(), q_start,
      None if bias is None else bias.double(), win_l=win_l, bias_clip=clip,
      impl='torch')
  twin = attn_decode.cached_attention(q, kc, vc, q_start, bias, win_l=win_l,
                                      bias_clip=clip, impl='torch')
  vis = _Visible(q_start, B, C, Smax, win_l)
  vabs = vc.double().abs().amax(-1)                       # [B, Smax, NKV]
  vmax = (vabs[:, None] * vis[..., None]).amax(2)         # [B, C, NKV]
  bound = (2.0 ** -7) * vmax.repeat_interleave(N // NKV, dim=2)[..., None]
  assert out.shape == ref.shape and out.dtype == torch.bfloat16
  assert torch.isfinite(out.float()).all(), label
  ours = float(((out.double() - ref).abs() / bound).max())
  theirs = float(((twin.double() - ref).abs() / bound).max())
  print(f'attn_decode {label}: worst err/bound kernel {ours:.3f} '
        f'fp32 twin {theirs:.3f}')
  assert ours <= 1.0, (label, ours)
  return ours


def _Run(q, kc, vc, q_start, bias=None, win_l=-1, clip=127, num_splits=0):
  return attn_decode.cached_attention(q, kc, vc, q_start, bias, win_l=win_l,
                                      bias_clip=clip, num_splits=num_splits,
                                      impl='hip')


@gpu
def test_first_token_one_key():
  q, kc, vc = _Inputs(1, 1, 1, 1, 64, 1)
  out = _Run(q, kc, vc, 0)
  _Check('first token', out, q, kc, vc, 0)
  # One key: softmax is exactly 1 and the output is that value row.
  assert torch.equal(out[0, 0], vc[0, 0])


@gpu
@pytest.mark.parametrize('q_start', [14, 15, 16])
def test_around_sixteen_keys(q_start):
  q, kc, vc = _Inputs(2, 1, 4, 4, 64, 40)
  _Check(f'q_start={q_start}', _Run(q, kc, vc, q_start), q, kc, vc, q_start)


@gpu
@pytest.mark.parametrize('num_splits', [1, 2, 5, 0])
def test_gqa_h128_splits_within_bound_and_reproducible(num_splits):
  q, kc, vc = _Inputs(3, 1, 8, 2, 128, 300)
  a = _Run(q, kc, vc, 299, num_splits=num_splits)
  b = _Run(q, kc, vc, 299, num_splits=num_splits)
  _Check(f'h128 gqa splits={num_splits}', a, q, kc, vc, 299)
  assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@gpu
def test_mqa_eight_rows_per_workgroup():
  q, kc, vc = _Inputs(2, 1, 8, 1, 64, 70)
  _Check('mqa', _Run(q, kc, vc, 69), q, kc, vc, 69)


@gpu
def test_q_start_tensor_with_empty_splits():
  q, kc, vc = _Inputs(3, 1, 4, 2, 64, 256)
  qs = torch.tensor([0, 37, 255], device='cuda', dtype=torch.int32)
  out = _Run(q, kc, vc, qs, num_splits=4)
  _Check('q_start tensor', out, q, kc, vc, qs)
  # Row 0 sees one key: three of its four splits are empty. Same bits as
  # the int form of that row.
  alone = _Run(q[:1], kc[:1], vc[:1], 0, num_splits=4)
  assert torch.equal(out[:1].view(torch.int16), alone.view(torch.int16))
  # A length past the cache is clamped, never dereferenced.
  wild = torch.tensor([0, 37, 10 ** 6], device='cuda', dtype=torch.int32)
  out2 = _Run(q, kc, vc, wild, num_splits=4)
  assert torch.equal(out2.view(torch.int16), out.view(torch.int16))


@gpu
@pytest.mark.parametrize('form', ['int', 'tensor'])
def test_window_with_leading_splits_outside(form):
  q, kc, vc = _Inputs(2, 1, 4, 2, 64, 256)
  qs = 200 if form == 'int' else torch.full((2,), 200, device='cuda',
                                            dtype=torch.int32)
  out = _Run(q, kc, vc, qs, win_l=20, num_splits=4)
  _Check(f'window {form}', out, q, kc, vc, qs, win_l=20)


@gpu
@pytest.mark.parametrize('C,N,NKV', [(3, 2, 2), (16, 2, 2), (17, 2, 2),
                                     (4, 8, 2), (5, 8, 2)])
def test_chunks_causal_window_bias(C, N, NKV):
  q, kc, vc = _Inputs(2, C, N, NKV, 64, 64)
  bias = _Bias(N, 3)
  for q_start, splits in ((0, 0), (30, 0), (30, 3)):
    out = _Run(q, kc, vc, q_start, bias, win_l=8, clip=3, num_splits=splits)
    _Check(f'chunk C={C} N={N} NKV={NKV} q_start={q_start} splits={splits}',
           out, q, kc, vc, q_start, bias, win_l=8, clip=3)


@gpu
@pytest.mark.parametrize('clip', [127, 3])
def test_bias_clip(clip):
  q, kc, vc = _Inputs(2, 1, 4, 2, 64, 300)
  bias = _Bias(4, clip)
  out = _Run(q, kc, vc, 299, bias, clip=clip)
  _Check(f'bias clip={clip}', out, q, kc, vc, 299, bias, clip=clip)
  # fp32 table: same values, same result.
  out32 = _Run(q, kc, vc, 299, bias.float(), clip=clip)
  assert torch.equal(out32.view(torch.int16), out.view(torch.int16))


@gpu
def test_large_logits_online_softmax_across_splits():
  q, kc, vc = _Inputs(2, 1, 4, 2, 64, 300, qscale=20.0)
  out = _Run(q, kc, vc, 299, num_splits=5)
  _Check('logits x20', out, q, kc, vc, 299)


@gpu
def test_long_cache_auto_splits():
  q, kc, vc = _Inputs(1, 1, 16, 2, 128, 8192)
  assert _Ext().attn_decode_num_splits(1, 2, 8192) > 1
  _Check('S=8192', _Run(q, kc, vc, 8191), q, kc, vc, 8191)


@gpu
def test_q_view_of_packed_projection():
  B, C, N, NKV, H = 2, 3, 4, 2, 64
  _, kc, vc = _Inputs(B, C, N, NKV, H, 50)
  g = torch.Generator().manual_seed(5)
  qkv = torch.randn(B, C, (N + 2 * NKV) * H, generator=g).to(
      'cuda', torch.bfloat16)
  q = qkv.split([N * H, NKV * H, NKV * H], dim=-1)[0].reshape(B, C, N, H)
  assert not q.is_contiguous()
  out = _Run(q, kc, vc, 40)
  _Check('packed q view', out, q, kc, vc, 40)
  assert torch.equal(out.view(torch.int16),
                     _Run(q.contiguous(), kc, vc, 40).view(torch.int16))


@gpu
@pytest.mark.parametrize('num_splits', [3, 1])
def test_exact_key_mapping(num_splits):
  """Row r = i * group + g of a KV head asks with q = 16 e_r; all keys are
  0 except one key j*(b, n, i) per row, visible to it, whose component r is
  64. Its logit is 16 * 64 / 8 = 128 against 0 for every other key, so all
  other probabilities are exactly 0 in fp32 and the output must be
  V[b, j*, n // group, :] bit for bit. (The issue states this with
  component 0; rows of one KV head share their keys, so each row gets a
  component of its own.)"""
  B, C, N, NKV, H, Smax, q_start, win_l = 2, 5, 8, 2, 64, 96, 60, 40
  group = N // NKV
  g = torch.Generator().manual_seed(13)
  q = torch.zeros(B, C, N, H)
  kc = torch.zeros(B, Smax, NKV, H)
  vc = torch.randn(B, Smax, NKV, H, generator=g).bfloat16()
  want = torch.zeros(B, C, N, H, dtype=torch.bfloat16)
  for b in range(B):
    for kvh in range(NKV):
      # Distinct keys for the rows of one KV head, drawn from the positions
      # every row of the chunk sees: [q_start + C - 1 - win_l, q_start].
      lo = q_start + C - 1 - win_l
      perm = lo + torch.randperm(q_start - lo + 1, generator=g)
      for i in range(C):
        for gi in range(group):
          r = i * group + gi
          n = kvh * group + gi
          p = q_start + i
          j = int(perm[r])
          assert p - win_l <= j <= p
          q[b, i, n, r] = 16.0
          kc[b, j, kvh, r] = 64.0
          want[b, i, n] = vc[b, j, kvh]
  out = _Run(q.to('cuda', torch.bfloat16), kc.to('cuda', torch.bfloat16),
             vc.cuda(), q_start, win_l=win_l, num_splits=num_splits)
  assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


@gpu
@pytest.mark.parametrize('win_l,num_splits,form', [
    (-1, 1, 'int'), (-1, 3, 'int'), (20, 1, 'int'), (20, 4, 'tensor'),
    (-1, 4, 'tensor')])
def test_poisoned_invisible_rows_have_no_effect(win_l, num_splits, form):
  B, C, N, NKV, H, Smax, q_start = 2, 3, 4, 2, 64, 256, 100
  q, kc, vc = _Inputs(B, C, N, NKV, H, Smax)
  qs = q_start if form == 'int' else torch.full(
      (B,), q_start, device='cuda', dtype=torch.int32)
  outs = []
  for fill in (0.0, float('nan')):
    k2, v2 = kc.clone(), vc.clone()
    k2[:, q_start + C:] = fill
    v2[:, q_start + C:] = fill
    if win_l >= 0:
      k2[:, :q_start - win_l] = fill
      v2[:, :q_start - win_l] = fill
    outs.append(_Run(q, k2, v2, qs, win_l=win_l, num_splits=num_splits))
  assert torch.isfinite(outs[1].float()).all()
  assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


@gpu
def test_contract_violations_raise_before_any_allocation():
  B, C, N, NKV, H, Smax = 2, 1, 4, 2, 64, 32
  q, kc, vc = _Inputs(B, C, N, NKV, H, Smax)
  bias = _Bias(N, 3)
  wide = torch.zeros(B, C, N, H + 8, device='cuda', dtype=torch.bfloat16)
  flat = torch.zeros(B * C * N * H + 8, device='cuda', dtype=torch.bfloat16)
  ok = dict(q=q, key_cache=kc, value_cache=vc, q_start=5, impl='hip')
  bad = {
      'H=32': dict(ok, q=q[..., :32].contiguous(),
                   key_cache=kc[..., :32].contiguous(),
                   value_cache=vc[..., :32].contiguous()),
      'rows=65': dict(ok, q=torch.zeros(B, 13, 10, H, device='cuda',
                                        dtype=torch.bfloat16)),
      'fp16': dict(ok, q=q.half()),
      'fp32 cache': dict(ok, key_cache=kc.float(), value_cache=vc.float()),
      'N % NKV': dict(ok, key_cache=kc.repeat(1, 1, 2, 1)[:, :, :3],
                      value_cache=vc.repeat(1, 1, 2, 1)[:, :, :3]),
      'q not dense': dict(ok, q=wide[..., :H]),
      'q misaligned': dict(ok, q=flat[1:1 + B * C * N * H].view(B, C, N, H)),
      'cache not dense': dict(ok, key_cache=kc.transpose(1, 2).contiguous()
                              .transpose(1, 2)),
      'q_start < 0': dict(ok, q_start=-1),
      'q_start + C > Smax': dict(ok, q_start=Smax),
      'bias shape': dict(ok, bias=bias[:, :6], bias_clip=3),
      'num_splits < 0': dict(ok, num_splits=-1),
      'q_start tensor dtype': dict(ok, q_start=torch.zeros(
          B, device='cuda', dtype=torch.int64)),
      'q_start tensor on cpu': dict(ok, q_start=torch.zeros(
          B, dtype=torch.int32)),
  }
  ext = _Ext()
  raw_bad = {
      'raw q_start + C > Smax': (q, kc, vc, None, Smax, None, -1, 127,
                                 0.125, 0),
      'raw H=32': (q[..., :32].contiguous(), kc[..., :32].contiguous(),
                   vc[..., :32].contiguous(), None, 5, None, -1, 127, 0.125,
                   0),
      'raw num_splits < 0': (q, kc, vc, None, 5, None, -1, 127, 0.125, -1),
      'raw bias shape': (q, kc, vc, None, 5, bias, -1, 4, 0.125, 0),
      'raw q strides': (wide[..., :H], kc, vc, None, 5, None, -1, 127,
                        0.125, 0),
  }
  good = attn_decode.cached_attention(**ok)
  torch.cuda.synchronize()
  before = torch.cuda.memory_stats()['allocation.all.allocated']
  for name, kw in bad.items():
    with pytest.raises(ValueError):
      attn_decode.cached_attention(**kw)
      pytest.fail(name)
  for name, args in raw_bad.items():
    with pytest.raises(RuntimeError):
      ext.attn_decode(*args)
      pytest.fail(name)
  assert torch.cuda.memory_stats()['allocation.all.allocated'] == before
  # 'auto' takes the twin where only the shape or dtype does not qualify.
  for name in ('H=32', 'rows=65', 'fp32 cache'):
    kw = dict(bad[name], impl='auto')
    got = attn_decode.cached_attention(**kw)
    assert torch.equal(got, attn_decode.cached_attention(
        **dict(kw, impl='torch'))), name
  torch.cuda.synchronize()
  assert torch.equal(good, attn_decode.cached_attention(**ok))


# ---- layer level ----------------------------------------------------------

def _ScaledErr(got, want):
  return float((got.float().cpu() - want).abs().max()) / max(
      1.0, float(want.abs().max()))


def _LayerPair(params, seed):
  """fp32 CPU layer and its bf16 GPU copies with decode_impl auto/torch."""
  torch.manual_seed(seed)
  ref = params.Instantiate()
  with torch.no_grad():
    for v in ref.parameters():
      v.add_(torch.randn_like(v) * 0.05)
  ref.eval()
  gpu_layers = {}
  for impl in ('auto', 'torch'):
    layer = ref.p.Copy().Set(fprop_dtype=torch.bfloat16).Instantiate()
    layer.load_state_dict(ref.state_dict())
    layer = layer.to('cuda').to(torch.bfloat16)
    layer.eval()
    n = 0
    from lingvo_amd.layers import attention
    for m in layer.modules():
      if isinstance(m, attention.MultiHeadedAttention):
        m.decode_impl = impl
        n += 1
    assert n > 0
    gpu_layers[impl] = layer
  return ref, gpu_layers


def _AssertRoutes(label, errs):
  print(f'{label}: scaled err auto {errs["auto"]:.4g} '
        f'torch {errs["torch"]:.4g}')
  assert errs['auto'] < 0.05, (label, errs)
  assert errs['auto'] <= 2 * errs['torch'] + 2.0 ** -8, (label, errs)


@gpu
def test_mha_extend_step_20_steps():
  from lingvo_amd.layers import attention
  b, d, steps = 3, 128, 20
  p = attention.MultiHeadedAttention.Params().Set(
      name='mha', input_dim=d, hidden_dim=d, num_heads=2, causal=True)
  ref, layers = _LayerPair(p, 21)
  x = torch.randn(b, steps, d).bfloat16().float()

  def Run(layer, dev, dtype):
    st = layer.InitStates(layer.theta, b, steps, dev, dtype)
    outs = []
    with torch.no_grad():
      for t in range(steps):
        o, st = layer.ExtendStep(layer.theta, x[:, t:t + 1].to(dev, dtype),
                                 st)
        outs.append(o)
    return torch.cat(outs, dim=1)

  want = Run(ref, 'cpu', torch.float32)
  errs = {k: _ScaledErr(Run(l, 'cuda', torch.bfloat16), want)
          for k, l in layers.items()}
  _AssertRoutes('mha ExtendStep', errs)


@gpu
def test_mha_stream_step_chunks_of_4():
  from lingvo_amd.layers import attention
  b, d, t, c = 3, 128, 20, 4
  p = attention.MultiHeadedAttention.Params().Set(
      name='mha', input_dim=d, hidden_dim=d, num_heads=2, causal=True,
      left_context=6)
  ref, layers = _LayerPair(p, 22)
  x = torch.randn(b, t, d).bfloat16().float()
  pad = torch.zeros(b, t)

  def Run(layer, dev, dtype):
    st = layer.InitStates(layer.theta, b, t, dev, dtype)
    outs = []
    with torch.no_grad():
      for c0 in range(0, t, c):
        o, st = layer.StreamStep(layer.theta,
                                 x[:, c0:c0 + c].to(dev, dtype),
                                 pad[:, c0:c0 + c].to(dev), st)
        outs.append(o)
    return torch.cat(outs, dim=1)

  want = Run(ref, 'cpu', torch.float32)
  full = ref.FProp(ref.theta, x, pad).detach()
  assert (full - want).abs().max() < 1e-3
  errs = {k: _ScaledErr(Run(l, 'cuda', torch.bfloat16), want)
          for k, l in layers.items()}
  _AssertRoutes('mha StreamStep', errs)


@gpu
def test_stack_extend_step_12_steps():
  from lingvo_amd.layers import transformer
  b, d, steps = 3, 128, 12
  p = transformer.StackedTransformerLayers.Params().Set(
      name='stack', model_dim=d, num_layers=2, num_heads=2,
      mask_self_atten=True)
  ref, layers = _LayerPair(p, 23)
  x = torch.randn(b, steps, d).bfloat16().float()

  def Run(layer, dev, dtype):
    st = layer.InitStates(layer.theta, b, steps, dev, dtype)
    outs = []
    with torch.no_grad():
      for t in range(steps):
        o, st = layer.ExtendStep(layer.theta, x[:, t:t + 1].to(dev, dtype),
                                 st)
        outs.append(o)
    return torch.cat(outs, dim=1)

  want = Run(ref, 'cpu', torch.float32)
  errs = {k: _ScaledErr(Run(l, 'cuda', torch.bfloat16), want)
          for k, l in layers.items()}
  _AssertRoutes('stack ExtendStep', errs)
