"""ops/xl_attn.py on the CPU: the composed twin against the layer's composed
math in fp64, and the argument checks."""

import pytest
import torch

from lingvo_amd.layers import attention as attention_lib
from lingvo_amd.ops import xl_attn

B, T, N, H = 2, 10, 2, 16


@pytest.mark.parametrize('m', [0, 6])
@pytest.mark.parametrize('causal', [True, False])
def test_twin_equals_layer_composed_math(m, causal):
  layer = attention_lib.TransformerXLAttention.Params().Set(
      name='xl', input_dim=N * H, hidden_dim=N * H, num_heads=N,
      causal=causal, random_seed=3).Instantiate().double()
  g = torch.Generator().manual_seed(m * 2 + causal)
  with torch.no_grad():
    for var in (layer.u_var, layer.v_var):
      var.copy_(torch.randn(var.shape, generator=g) * 0.3)
  s = m + T
  q = torch.randn(B, T, N, H, generator=g, dtype=torch.float64)
  k = torch.randn(B, s, N, H, generator=g, dtype=torch.float64)
  v = torch.randn(B, s, N, H, generator=g, dtype=torch.float64)
  lens = torch.tensor([T, T - 3])
  paddings = (torch.arange(T)[None, :] >= lens[:, None]).double()
  theta = layer.theta
  want = layer._ComposedContext(theta, q, k, v, paddings, m)
  r = layer._RelEmb(torch.arange(-s + 1, s), theta).double()
  got = xl_attn.xl_attention(q, k, v, r, theta.u_var, theta.v_var,
                             klen=m + lens, causal=causal)
  assert got.dtype == torch.float64
  assert float((got - want).abs().max().detach()) < 1e-10


def _Args(**over):
  s = 14
  a = dict(q=torch.zeros(B, T, N, H), k=torch.zeros(B, s, N, H),
           v=torch.zeros(B, s, N, H), r=torch.zeros(2 * s - 1, N, H),
           u=torch.zeros(N, H), w=torch.zeros(N, H), klen=None)
  a.update(over)
  return a


@pytest.mark.parametrize('over, exc', [
    (dict(q=torch.zeros(B, T, N * H)), ValueError),               # rank
    (dict(k=torch.zeros(B, 14, N + 1, H)), ValueError),           # N != NKV
    (dict(v=torch.zeros(B, 13, N, H)), ValueError),               # v != k
    (dict(k=torch.zeros(B, 9, N, H), v=torch.zeros(B, 9, N, H),
          r=torch.zeros(17, N, H)), ValueError),                  # S < T
    (dict(r=torch.zeros(28, N, H)), ValueError),                  # 2S-1
    (dict(u=torch.zeros(N, H + 1)), ValueError),
    (dict(w=torch.zeros(H)), ValueError),
    (dict(k=torch.zeros(B, 14, N, H, dtype=torch.float64)), TypeError),
    (dict(q=torch.zeros(B, T, N, H, dtype=torch.int32)), TypeError),
    (dict(klen=torch.zeros(B)), TypeError),                       # float klen
    (dict(klen=torch.zeros(B + 1, dtype=torch.int32)), TypeError),
    (dict(r=torch.zeros(27, N, H, device='meta')), ValueError),   # device
])
def test_check_args_refuses(over, exc):
  with pytest.raises(exc, match='xl_attention'):
    xl_attn.xl_attention(**_Args(**over))


def test_impl_name_is_checked():
  with pytest.raises(ValueError, match='impl'):
    xl_attn.xl_attention(**_Args(), impl='fast')
