"""ops/block_sparse_attn.py on the GPU: the HIP kernels against
`_ref_block_sparse_attention` in float64 on the same bf16-rounded inputs.

Tolerance (the rule of test_favor_attn_gpu.py): the twin run in fp32 with the
probabilities rounded to bf16 before the contraction
(operand_dtype=torch.bfloat16) and its outputs cast to bf16 is what any bf16
matrix-core route must lose; its max-abs error against the float64 reference
is the baseline. The kernels' error may be at most 2 x baseline + one bf16 ulp
at max|ref| for o, dq, dk and dv. The layer test applies the same rule with
the composed route (block_sparse_impl='torch') as the yardstick.
"""

import math

import pytest
import torch

from lingvo_amd.layers import attention_sparse as asp
from lingvo_amd.ops import block_sparse_attn as bsa

gpu = pytest.mark.gpu

B, N = 2, 2

ASYM = [[1, 0, 1], [0, 1, 0], [1, 1, 0]]
GAPS = [[int(j == i or (i == 3 and j in (0, 3, 6))) for j in range(7)]
        for i in range(7)]

# Block size 64 and H = 64 unless the case says otherwise.
CASES = {
    't64_one_tile': dict(T=64, mask=[[1]]),
    't65_tail_row': dict(T=65, mask=[[1, 1], [1, 1]]),
    't130_asym': dict(T=130, mask=ASYM),
    't448_gaps': dict(T=448, mask=GAPS),
    't192_empty_row': dict(T=192, mask=[[1, 1, 0], [0, 0, 0], [1, 0, 1]]),
    't192_empty_col': dict(T=192, mask=[[1, 1, 0], [0, 1, 0], [1, 0, 0]]),
    't200_causal': dict(T=200, causal=True,
                        mask=[[1, 0, 1, 0], [1, 1, 0, 0], [1, 1, 1, 0],
                              [1, 1, 1, 1]]),
    't130_klen': dict(T=130, mask=ASYM, klen=[130, 40]),
    't100_klen0': dict(T=100, mask=[[1, 1], [1, 1]], klen=[0, 100]),
    't300_bs128': dict(T=300, bs=128, mask=asp.LocalGlobalBlockMask(3, 1, 1)),
    't130_h128': dict(T=130, H=128, mask=ASYM),
}


def _BfUlp(x):
  return 2.0 ** (math.floor(math.log2(max(x, 1e-30))) - 7)


def _Err(got, ref):
  return float((got.detach().double() - ref.detach()).abs().max())


def _Inputs(case, b=B, device='cuda'):
  t, h = case['T'], case.get('H', 64)
  g = torch.Generator().manual_seed(t * 13 + h)
  rnd = lambda *shape: torch.randn(*shape, generator=g)
  bf = lambda x: x.to(device, torch.bfloat16)
  x = dict(q=bf(rnd(b, t, N, h) * 0.3), k=bf(rnd(b, t, N, h) * 0.3),
           v=bf(rnd(b, t, N, h)), dout=bf(rnd(b, t, N, h)))
  klen = case.get('klen')
  x['klen'] = None if klen is None else torch.tensor(
      klen, device=device, dtype=torch.int32)
  return x


def _Run(x, case, dtype, **kw):
  """[o, dq, dk, dv] of the op on the inputs cast to dtype."""
  leaves = [x[n].to(dtype).clone().requires_grad_(True) for n in 'qkv']
  fn = (bsa.block_sparse_attention if dtype == torch.bfloat16 else
        bsa._ref_block_sparse_attention)
  o = fn(*leaves, case['mask'], case.get('bs', 64), klen=x['klen'],
         causal=case.get('causal', False), **kw)
  o.backward(x['dout'].to(dtype))
  return [o.detach()] + [t.grad for t in leaves]


@gpu
@pytest.mark.parametrize('name', list(CASES))
def test_against_fp64_with_rounded_operand_baseline(name):
  case = CASES[name]
  x = _Inputs(case)
  ref = _Run(x, case, torch.float64)
  base = [_Err(g.to(torch.bfloat16), r) for g, r in zip(
      _Run(x, case, torch.float32, operand_dtype=torch.bfloat16), ref)]
  got = _Run(x, case, torch.bfloat16)
  again = _Run(x, case, torch.bfloat16)
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
  if name == 't192_empty_row':    # no visible key: exact zeros
    assert not bool(o[:, 64:128].any()) and not bool(dq[:, 64:128].any())
  if name == 't192_empty_col':    # seen by no query
    assert not bool(dk[:, 128:].any()) and not bool(dv[:, 128:].any())
  for b_, kl in enumerate(case.get('klen', [])):
    assert not bool(dk[b_, kl:].any()) and not bool(dv[b_, kl:].any())
    if kl == 0:
      assert not bool(o[b_].any()) and not bool(dq[b_].any())


def _Layer(dtype, impl, state=None):
  p = asp.BlockSparseAttention.Params().Set(
      name='bsa', input_dim=128, hidden_dim=128, num_heads=2, random_seed=11,
      block_size=64, block_mask=asp.LocalGlobalBlockMask(4, 1, 1),
      block_sparse_impl=impl, dtype=dtype)
  layer = p.Instantiate()
  if state is not None:
    layer.load_state_dict({k: v.to(dtype) for k, v in state.items()})
  return layer.to('cuda')


@gpu
def test_layer_kernel_route_against_composed():
  T = 250
  auto = _Layer(torch.bfloat16, 'auto')
  state = auto.state_dict()
  layers = dict(auto=auto, torch=_Layer(torch.bfloat16, 'torch', state),
                ref=_Layer(torch.float64, 'torch', state))
  g = torch.Generator().manual_seed(4)
  x = torch.randn(2, T, 128, generator=g).to(torch.bfloat16).cuda()
  wgt = torch.randn(2, T, 128, generator=g).cuda()
  lens = torch.tensor([T, 90], device='cuda')
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
def test_peak_memory_stays_under_one_logits_tensor():
  t = 4096
  case = dict(T=t, mask=asp.LocalGlobalBlockMask(64, 1, 1))
  x = _Inputs(case, b=1)
  limit = 1 * N * t * t * 4  # one fp32 [B,N,T,T]
  _Run(x, case, torch.bfloat16)  # builds and caches the tile lists
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  before = torch.cuda.memory_allocated()
  _Run(x, case, torch.bfloat16)
  torch.cuda.synchronize()
  rise = torch.cuda.max_memory_allocated() - before
  print(f'peak rise: kernels {rise} limit {limit}')
  assert rise < limit
