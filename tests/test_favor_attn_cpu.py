"""ops/favor_attn.py on the CPU: the composed twin against the layer's
composed math in fp64, the layer's route choice, and the argument checks."""

import pytest
import torch

from lingvo_amd.layers import attention_sparse as asp
from lingvo_amd.ops import favor_attn

B, T, N, H, M = 2, 9, 2, 8, 16


def _Layer(**kw):
  return asp.PerformerAttention.Params().Set(
      name='perf', input_dim=N * H, hidden_dim=N * H, num_heads=N,
      num_random_features=M, random_seed=3, **kw).Instantiate()


@pytest.mark.parametrize('lens', [None, [T, 0]])
@pytest.mark.parametrize('causal', [False, True])
def test_twin_equals_layer_composed_math(causal, lens):
  layer = _Layer(causal=causal).double()
  g = torch.Generator().manual_seed(5 + causal)
  q, k, v = (torch.randn(B, T, N, H, generator=g, dtype=torch.float64)
             for _ in range(3))
  klen = paddings = None
  if lens is not None:
    klen = torch.tensor(lens)
    paddings = (torch.arange(T)[None, :] >= klen[:, None]).double()
  want = layer._ComposedContext(q, k, v, paddings)
  got = favor_attn.favor_attention(q, k, v, layer.proj_mat, klen=klen,
                                   causal=causal)
  assert got.dtype == torch.float64
  assert float((got - want).abs().max()) < 1e-12
  if lens is not None:
    assert not bool(got[1].any())


@pytest.mark.parametrize('causal', [False, True])
def test_layer_routes_agree_on_cpu(causal):
  auto = _Layer(causal=causal, favor_impl='auto')
  composed = _Layer(causal=causal, favor_impl='torch')
  composed.load_state_dict(auto.state_dict())
  x = torch.randn(B, T, N * H, generator=torch.Generator().manual_seed(1))
  pad = (torch.arange(T)[None, :] >= torch.tensor([T, 4])[:, None]).float()
  assert torch.equal(auto.FProp(auto.theta, x, pad),
                     composed.FProp(composed.theta, x, pad))


def _Args(**over):
  a = dict(q=torch.zeros(B, T, N, H), k=torch.zeros(B, T, N, H),
           v=torch.zeros(B, T, N, H), proj=torch.zeros(M, H), klen=None)
  a.update(over)
  return a


@pytest.mark.parametrize('over, exc', [
    (dict(q=torch.zeros(B, T, N * H)), ValueError),               # rank
    (dict(proj=torch.zeros(M)), ValueError),
    (dict(k=torch.zeros(B, T + 1, N, H),
          v=torch.zeros(B, T + 1, N, H)), ValueError),            # S != T
    (dict(v=torch.zeros(B, T, N + 1, H)), ValueError),
    (dict(proj=torch.zeros(M, H + 1)), ValueError),
    (dict(klen=torch.zeros(B)), TypeError),                       # float klen
    (dict(klen=torch.zeros(B + 1, dtype=torch.int32)), TypeError),
    (dict(k=torch.zeros(B, T, N, H, dtype=torch.float64)), TypeError),
    (dict(q=torch.zeros(B, T, N, H, dtype=torch.int32)), TypeError),
    (dict(proj=torch.zeros(M, H, device='meta')), ValueError),    # device
    (dict(impl='fast'), ValueError),
])
def test_check_args_refuses(over, exc):
  with pytest.raises(exc, match='favor_attention'):
    favor_attn.favor_attention(**_Args(**over))
