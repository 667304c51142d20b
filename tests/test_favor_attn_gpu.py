"""ops/favor_attn.py on the GPU: the HIP kernels against
`_ref_favor_attention` in float64 on the same bf16-rounded inputs.

Tolerance (measured, per case): the twin run in fp32 with phi_q, phi_k and v
rounded to bf16 before the contractions (operand_dtype=torch.bfloat16) and
its outputs cast to bf16 is what any bf16 matrix-core route must lose; its
max-abs error against the float64 reference is the baseline. The kernels'
error may be at most 2 x baseline + one bf16 ulp at max|ref| for o, dq, dk
and dv: the factor covers the bf16 rounding of the carried state where it is
an MFMA operand and the chunked order of summation. The layer test applies
the same rule with the composed route (favor_impl='torch') as the yardstick.

The clamp of the denominator at 1e-6 makes the gradient discontinuous, so
the test asserts that no row with a visible key has a float64 denominator in
[0.5e-6, 2e-6].
"""

import math

import pytest
import torch

from lingvo_amd.layers import attention_sparse as asp
from lingvo_amd.ops import favor_attn

gpu = pytest.mark.gpu

B, N, H = 2, 2, 64

# Causal with m = 128 unless the case says otherwise.
CASES = {
    't1': dict(T=1),
    't63': dict(T=63),                        # one short of a chunk
    't64': dict(T=64),                        # one exact chunk
    't65': dict(T=65),                        # state into a one-row chunk
    't130': dict(T=130),                      # three chunks, ragged tail
    't65_noncausal': dict(T=65, causal=False),
    't130_noncausal_klen': dict(T=130, causal=False, klen=[130, 40]),
    't100_klen0': dict(T=100, klen=[0, 100]),
    't65_m32': dict(T=65, m=32),
    't65_m96': dict(T=65, m=96),
}


def _BfUlp(x):
  return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


def _Err(got, ref):
  return float((got.detach().double() - ref.detach()).abs().max())


def _Proj(m):
  layer = asp.PerformerAttention.Params().Set(
      name='perf', input_dim=2 * H, hidden_dim=2 * H, num_heads=2,
      num_random_features=m, random_seed=7).Instantiate()
  return layer.proj_mat


def _Inputs(case, device='cuda'):
  t, m = case['T'], case.get('m', 128)
  g = torch.Generator().manual_seed(t * 13 + m)
  rnd = lambda *shape: torch.randn(*shape, generator=g)
  bf = lambda x: x.to(device, torch.bfloat16)
  x = dict(q=bf(rnd(B, t, N, H) * 0.3), k=bf(rnd(B, t, N, H) * 0.3),
           v=bf(rnd(B, t, N, H)), dout=bf(rnd(B, t, N, H)),
           proj=_Proj(m).to(device))
  klen = case.get('klen')
  x['klen'] = None if klen is None else torch.tensor(
      klen, device=device, dtype=torch.int32)
  return x, t, case.get('causal', True)


def _Run(x, causal, dtype, fn):
  """[o, dq, dk, dv] of fn on the inputs cast to dtype."""
  leaves = [x[n].to(dtype).clone().requires_grad_(True) for n in 'qkv']
  o = fn(*leaves, x['proj'], x['klen'], causal)
  o.backward(x['dout'].to(dtype))
  return [o.detach()] + [t.grad for t in leaves]


def _Kernel(q, k, v, proj, klen, causal):
  return favor_attn.favor_attention(q, k, v, proj, klen=klen, causal=causal)


def _Rounded(q, k, v, proj, klen, causal):
  return favor_attn._ref_favor_attention(q, k, v, proj, klen, causal,
                                         operand_dtype=torch.bfloat16)


@gpu
@pytest.mark.parametrize('name', list(CASES))
def test_against_fp64_with_rounded_operand_baseline(name):
  x, t, causal = _Inputs(CASES[name])
  klen = CASES[name].get('klen') or [t] * B
  with torch.no_grad():
    _, den = favor_attn._ref_favor_attention(
        x['q'].double(), x['k'].double(), x['v'].double(), x['proj'],
        x['klen'], causal, return_den=True)
  for b_, kl in enumerate(klen):
    if kl > 0:  # every row sees key 0
      d = den[b_]
      assert not bool(((d >= 0.5e-6) & (d <= 2e-6)).any()), float(d.min())
  ref = _Run(x, causal, torch.float64, favor_attn._ref_favor_attention)
  base = [_Err(g.to(torch.bfloat16), r)
          for g, r in zip(_Run(x, causal, torch.float32, _Rounded), ref)]
  got = _Run(x, causal, torch.bfloat16, _Kernel)
  again = _Run(x, causal, torch.bfloat16, _Kernel)
  torch.cuda.synchronize()
  failures = []
  for n, g, g2, r, bs in zip(('o', 'dq', 'dk', 'dv'), got, again, ref, base):
    assert g.shape == r.shape and g.dtype == torch.bfloat16
    assert torch.equal(g, g2), n
    top = float(r.abs().max())
    bound = 2 * bs + _BfUlp(top)
    err = _Err(g, r)
    print(f'{name} {n}: err {err:.4g} baseline {bs:.4g} bound {bound:.4g} '
          f'ratio {err / max(bs, 1e-30):.3g} (max|ref| {top:.4g})')
    if not err <= bound:
      failures.append((n, err, bound))
  assert not failures, failures

  o, dq, dk, dv = got
  for b_, kl in enumerate(klen):
    assert not bool(dk[b_, kl:].any()) and not bool(dv[b_, kl:].any())
    if kl == 0:  # no visible key: zero output and gradients
      for z in (o, dq, dk, dv):
        assert not bool(z[b_].any())


def _Layer(dtype, impl, causal, state=None):
  p = asp.PerformerAttention.Params().Set(
      name='perf', input_dim=128, hidden_dim=128, num_heads=2, causal=causal,
      random_seed=11, favor_impl=impl, dtype=dtype)
  layer = p.Instantiate()
  if state is not None:
    layer.load_state_dict({k: v.to(dtype) for k, v in state.items()})
  return layer.to('cuda')


@gpu
@pytest.mark.parametrize('causal', [True, False])
def test_layer_kernel_route_against_composed(causal):
  T = 70
  auto = _Layer(torch.bfloat16, 'auto', causal)
  state = auto.state_dict()
  layers = dict(auto=auto, torch=_Layer(torch.bfloat16, 'torch', causal, state),
                ref=_Layer(torch.float64, 'torch', causal, state))
  g = torch.Generator().manual_seed(4)
  x = torch.randn(2, T, 128, generator=g).to(torch.bfloat16).cuda()
  wgt = torch.randn(2, T, 128, generator=g).cuda()
  lens = torch.tensor([T, 20], device='cuda')
  pad = (torch.arange(T, device='cuda')[None, :] >= lens[:, None])
  res = {}
  for name, layer in layers.items():
    dt = layer.post_w.dtype
    out = layer.FProp(layer.theta, x.to(dt), pad.to(dt))
    (out.double() * wgt).sum().backward()
    res[name] = dict(out=out.detach(),
                     **{k: v.grad for k, v in layer.named_parameters()})
  failures = []
  for key, ref in res['ref'].items():
    base = _Err(res['torch'][key], ref)
    err = _Err(res['auto'][key], ref)
    bound = 2 * base + _BfUlp(float(ref.abs().max()))
    print(f'layer {key}: err {err:.4g} composed {base:.4g} bound {bound:.4g}')
    if not err <= bound:
      failures.append((key, err, bound))
  assert not failures, failures


@gpu
def test_peak_memory_stays_under_one_outer_product_tensor():
  x, t, causal = _Inputs(dict(T=512))
  x = {n: (v[:1] if n in ('q', 'k', 'v', 'dout') else v)
       for n, v in x.items()}                                    # B = 1
  limit = 1 * t * N * 128 * H * 4  # one fp32 [B,T,N,m,H]
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  _Run(x, causal, torch.bfloat16, _Kernel)
  torch.cuda.synchronize()
  rise = torch.cuda.max_memory_allocated() - before
  print(f'peak rise: kernels {rise} limit {limit}')
  assert rise < limit
