"""ops/xl_attn.py on the GPU: the HIP kernels against `_ref_xl_attention` in
float64 on the same bf16-rounded inputs.

Tolerance (measured, per case): the flash kernels (fa_fwd, fa_bwd 'tiles')
run on the same k, v, klen and mask at T = S, M = 0, and their max-abs error
against flash_attn._ref_attention in float64 is the baseline. The XL
kernels' error may be at most 2 x baseline + one bf16 ulp at max|ref| for o,
dq, dk, dv (each logit is two rounded-operand dot products instead of one);
dr, du and dw are fp32 sums of dq-like terms and get 2 x the dq baseline
scaled by max|ref_d*| / max|ref_dq| (taken as 1 where both are zero: one
visible key per row), plus the ulp. The layer test applies
the same rule with the composed route (xl_impl='torch') as the yardstick.
"""

import math

import pytest
import torch

from lingvo_amd.ops import flash_attn as fa
from lingvo_amd.ops import xl_attn

gpu = pytest.mark.gpu

B, N, H = 2, 2, 64
SCALE = 1.0 / math.sqrt(H)

# Causal unless the case says otherwise.
CASES = {
    't1': dict(T=1),
    't16': dict(T=16),
    't17': dict(T=17),                       # strip + 1
    't129': dict(T=129),                     # crosses a q block
    't65_noncausal': dict(T=65, causal=False),
    't37_m5': dict(T=37, M=5),
    't20_m70': dict(T=20, M=70),             # memory > segment, 2 key tiles
    't1_m70': dict(T=1, M=70),               # decode-like
    't100_m28_klen': dict(T=100, M=28, klen=[128, 40]),
    't100_klen0': dict(T=100, klen=[0, 100]),
}


def _BfUlp(x):
  return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


def _Err(got, ref):
  return float((got.detach().double() - ref.detach()).abs().max())


def _Inputs(case):
  t, m = case['T'], case.get('M', 0)
  s = m + t
  g = torch.Generator().manual_seed(t * 13 + m)
  rnd = lambda *shape: torch.randn(*shape, generator=g)
  bf = lambda x: x.to('cuda', torch.bfloat16)
  x = dict(q=bf(rnd(B, t, N, H)), k=bf(rnd(B, s, N, H)),
           v=bf(rnd(B, s, N, H)), dout=bf(rnd(B, t, N, H)),
           r=bf(rnd(2 * s - 1, N, H) * 0.3), u=bf(rnd(N, H) * 0.3),
           w=bf(rnd(N, H) * 0.3),
           # the q and dout rows of the T = S flash baseline
           qs=bf(rnd(B, s, N, H)), douts=bf(rnd(B, s, N, H)))
  klen = case.get('klen')
  x['klen'] = None if klen is None else torch.tensor(
      klen, device='cuda', dtype=torch.int32)
  return x, t, m, s, case.get('causal', True)


def _FlashBaseline(x, causal):
  """Max-abs errors of o, dq, dk, dv of the flash kernels at T = S."""
  from lingvo_amd.ops import _loader
  ext = _loader.get_ext(required=True)
  q, dout = (x['qs'], x['douts']) if x['qs'].shape != x['q'].shape else (
      x['q'], x['dout'])
  win_r = 0 if causal else -1
  o, lse = ext.fa_fwd(q, x['k'], x['v'], x['klen'], None, None, None, -1,
                      win_r, 127, SCALE, 0, 0)
  got = ext.fa_bwd(dout, q, x['k'], x['v'], o, lse, x['klen'], None, None,
                   None, False, -1, win_r, 127, SCALE, 0, 0, route='tiles')
  ref = [t.double().requires_grad_(True) for t in (q, x['k'], x['v'])]
  ro = fa._ref_attention(*ref, x['klen'], None, -1, win_r, 127, SCALE)
  ro.backward(dout.double())
  return [_Err(o, ro)] + [_Err(a, b.grad) for a, b in zip(got[:3], ref)]


def _RunBoth(x, causal):
  """((o, dq, dk, dv, dr, du, dw) of the kernels, the same in float64)."""
  names = ('q', 'k', 'v', 'r', 'u', 'w')
  outs = []
  for dt, impl in ((torch.bfloat16, 'auto'), (torch.float64, 'torch')):
    leaves = [x[n].to(dt).clone().requires_grad_(True) for n in names]
    o = xl_attn.xl_attention(*leaves, klen=x['klen'], causal=causal,
                             impl=impl)
    o.backward(x['dout'].to(dt))
    outs.append([o.detach()] + [t.grad for t in leaves])
  return outs


@gpu
@pytest.mark.parametrize('name', list(CASES))
def test_against_fp64_with_flash_baseline(name):
  x, t, m, s, causal = _Inputs(CASES[name])
  base = dict(zip(('o', 'dq', 'dk', 'dv'), _FlashBaseline(x, causal)))
  got, ref = _RunBoth(x, causal)
  torch.cuda.synchronize()
  what = ('o', 'dq', 'dk', 'dv', 'dr', 'du', 'dw')
  top = {n: float(r.abs().max()) for n, r in zip(what, ref)}
  failures = []
  for n, g, r in zip(what, got, ref):
    assert g.shape == r.shape and g.dtype == torch.bfloat16
    # One visible key per row (T = 1, M = 0) makes every reference gradient
    # but dv zero; the 0/0 of the scaling is then taken as 1.
    b = base[n] if n in base else base['dq'] * (
        top[n] / top['dq'] if top['dq'] > 0 else 1.0)
    bound = 2 * b + _BfUlp(top[n])
    err = _Err(g, r)
    print(f'{name} {n}: err {err:.4g} baseline {b:.4g} bound {bound:.4g} '
          f'ratio {err / max(b, 1e-30):.3g} (max|ref| {top[n]:.4g})')
    if not err <= bound:
      failures.append((n, err, bound))
  assert not failures, failures

  o, dq, dk, dv, dr = got[:5]
  klen = CASES[name].get('klen') or [s] * B
  i = torch.arange(t)[:, None]
  j = torch.arange(s)[None, :]
  used = torch.zeros(2 * s - 1, dtype=torch.bool)
  for b_, kl in enumerate(klen):
    assert not bool(dk[b_, kl:].any()) and not bool(dv[b_, kl:].any())
    if kl == 0:  # no visible key: zero output and gradients
      for z in (o, dq, dk, dv):
        assert not bool(z[b_].any())
    vis = (j < kl) & ((j <= m + i) if causal else torch.ones_like(j <= i))
    used[(m + i - j + s - 1)[vis]] = True
  assert not bool(used[:max(0, s - t)].any())  # distances below -(T-1)
  assert not bool(dr[~used.cuda()].any())


@gpu
@pytest.mark.parametrize('causal', [True, False])
def test_zero_biases_reduce_to_flash(causal):
  x, t, _, s, _ = _Inputs(dict(T=100, klen=[100, 63]))
  zero = lambda n: torch.zeros_like(x[n])
  o = xl_attn.xl_attention(x['q'], x['k'], x['v'], zero('r'), zero('u'),
                           zero('w'), klen=x['klen'], causal=causal)
  want = fa.flash_attention(x['q'], x['k'], x['v'], x['klen'], None, -1,
                            0 if causal else -1)
  assert _Err(o, want.double()) <= _BfUlp(float(want.float().abs().max()))


def _Layer(dtype, impl, state=None):
  from lingvo_amd.layers import attention as attention_lib
  p = attention_lib.TransformerXLAttention.Params().Set(
      name='xl', input_dim=128, hidden_dim=128, num_heads=2, causal=True,
      random_seed=11, xl_impl=impl, dtype=dtype)
  layer = p.Instantiate()
  if state is None:
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
      for var in (layer.u_var, layer.v_var):
        var.copy_((torch.randn(var.shape, generator=g) * 0.3).to(dtype))
  else:
    layer.load_state_dict({k: v.to(dtype) for k, v in state.items()})
  return layer.to('cuda')


@gpu
def test_layer_kernel_route_against_composed():
  T, M = 24, 40
  auto = _Layer(torch.bfloat16, 'auto')
  state = auto.state_dict()
  assert float(state['pos_proj'].float().abs().max()) > 0
  layers = dict(auto=auto, torch=_Layer(torch.bfloat16, 'torch', state),
                ref=_Layer(torch.float64, 'torch', state))
  g = torch.Generator().manual_seed(4)
  x = torch.randn(2, M + T, 128, generator=g).to(torch.bfloat16).cuda()
  wgt = torch.randn(2, T, 128, generator=g).cuda()
  pad = torch.zeros(2, T, device='cuda')
  res = {}
  for name, layer in layers.items():
    xs = x.to(layer.u_var.dtype)
    out = layer.FProp(layer.theta, xs[:, M:], pad.to(xs.dtype),
                      memory=xs[:, :M])
    (out.double() * wgt).sum().backward()
    full = layer.FProp(layer.theta, xs, None)[:, M:]
    res[name] = dict(out=out.detach(), full=full.detach(),
                     **{k: v.grad for k, v in layer.named_parameters()})
  assert float(res['auto']['pos_proj'].float().abs().max()) > 0
  failures = []
  for key, ref in res['ref'].items():
    base = _Err(res['torch'][key], ref)
    err = _Err(res['auto'][key], ref)
    bound = 2 * base + _BfUlp(float(ref.abs().max()))
    print(f'layer {key}: err {err:.4g} composed {base:.4g} bound {bound:.4g}')
    if not err <= bound:
      failures.append((key, err, bound))
  # Segment recurrence in float64, so 'out' and 'full' above share a truth.
  assert _Err(res['ref']['full'], res['ref']['out']) < 1e-9
  assert not failures, failures


@gpu
def test_peak_memory_stays_under_one_logits_tensor():
  x, t, m, s, causal = _Inputs(dict(T=512, M=512))
  names = ('q', 'k', 'v', 'r', 'u', 'w')
  n4 = {n: (torch.cat([x[n], x[n]], dim=-2) if n not in 'uw' else
            torch.cat([x[n], x[n]], dim=0)) for n in names}   # N = 4
  dout = torch.cat([x['dout'], x['dout']], dim=-2)
  limit = B * 4 * t * s * 4  # one fp32 [B,N,T,S]
  rise = {}
  for impl in ('auto', 'torch'):
    leaves = [n4[n].clone().requires_grad_(True) for n in names]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    xl_attn.xl_attention(*leaves, causal=causal, impl=impl).backward(dout)
    torch.cuda.synchronize()
    rise[impl] = torch.cuda.max_memory_allocated() - before
    del leaves
  print(f'peak rise: kernels {rise["auto"]} composed {rise["torch"]} '
        f'limit {limit}')
  assert rise['auto'] < limit < rise['torch']
