"""ops/routing_attn.py on the CPU: the dense twin against the layer's composed
loop over the clusters in float64, the torch twin of the list builder on a
hand-written example, and the argument refusals."""

import pytest
import torch

from lingvo_amd.layers import attention_sparse as asp
from lingvo_amd.ops import routing_attn as ra

# (T, C, window, causal); two heads of 8, random paddings with holes, batch
# row 1 fully padded.
TWIN_CASES = [(65, 1, 65, False), (130, 3, 40, False), (100, 16, 7, True),
              (130, 3, 1, False), (50, 2, 64, True)]


@pytest.mark.parametrize('t,c,window,causal', TWIN_CASES)
def test_twin_equals_the_layers_composed_loop(t, c, window, causal):
  layer = asp.RoutingAttention.Params().Set(
      name='a', input_dim=16, hidden_dim=16, num_heads=2, random_seed=21,
      num_clusters=c, atten_window=window, causal=causal,
      dtype=torch.float64).Instantiate()
  g = torch.Generator().manual_seed(t + c)
  q, k, v, dout = (torch.randn(2, t, 2, 8, generator=g, dtype=torch.float64)
                   for _ in range(4))
  q_cl = torch.randint(0, c, (2, 2, t), generator=g)
  k_cl = torch.randint(0, c, (2, 2, t), generator=g)
  pad = (torch.rand(2, t, generator=g) < 0.3).double()
  pad[1] = 1.0
  res = []
  for fn in (lambda *x: layer._ComposedContext(*x, q_cl, k_cl, pad),
             lambda *x: ra.routing_attention(*x, q_cl, k_cl, c, window, pad,
                                             causal)):
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
    o = fn(*leaves)
    o.backward(dout)
    res.append([o.detach()] + [x.grad for x in leaves])
  for name, want, got in zip(('o', 'dq', 'dk', 'dv'), *res):
    assert got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-12, name


def test_list_twin_on_a_hand_written_example():
  q_cl = torch.tensor([[[1, 0, 1, 1, 0, 2, 1, 0, 0, 1]]])
  k_cl = torch.tensor([[[0, 0, 1, 0, 2, 0, 1, 1, 0, 1]]])
  pad = torch.tensor([[0., 1, 0, 0, 0, 0, 0, 1, 0, 0]])
  q_perm, q_start, q_tiles, q_ntiles, k_sel, k_cnt = ra._ref_routing_lists(
      q_cl, k_cl, 4, 3, pad)
  assert q_perm.tolist() == [[[1, 4, 7, 8, 0, 2, 3, 6, 9, 5]]]
  assert q_start.tolist() == [[[0, 4, 9, 10, 10]]]
  assert q_ntiles.tolist() == [[3]]   # ceil(10/64) + 4 - 1 = 4 slots
  assert q_tiles.tolist() == [[[[0, 0, 4], [1, 4, 5], [2, 9, 1],
                                [-1, -1, -1]]]]
  # Key 1 is padded and key 8 is the fourth live member of cluster 0.
  assert k_sel.tolist() == [[[[0, 3, 5], [2, 6, 9], [4, -1, -1],
                              [-1, -1, -1]]]]
  assert k_cnt.tolist() == [[[3, 3, 1, 0]]]
  mask = ra.visible_mask(q_cl, k_cl, 3, pad, causal=True)[0, 0]
  assert mask[9].nonzero().flatten().tolist() == [2, 6, 9]
  assert mask[8].nonzero().flatten().tolist() == [0, 3, 5]
  assert not bool(mask[5, :4].any()) and bool(mask[5, 4])
  assert not bool(mask[0].any())      # cluster 1's first key is key 2


def test_argument_refusals():
  q = torch.randn(2, 10, 2, 8)
  ids = torch.zeros(2, 2, 10, dtype=torch.int64)
  ok = dict(q=q, k=q, v=q, q_cl=ids, k_cl=ids, num_clusters=2, window=4)
  ra.routing_attention(**ok)
  for change, error in (
      (dict(k=q[:, :5]), ValueError), (dict(v=q.double()), TypeError),
      (dict(q_cl=ids.float()), TypeError),
      (dict(k_cl=ids.permute(0, 2, 1)), ValueError),
      (dict(k_cl=ids.int()), TypeError), (dict(num_clusters=0), ValueError),
      (dict(window=0), ValueError),
      (dict(paddings=torch.zeros(2, 9)), ValueError),
      (dict(impl='hip'), ValueError)):
    with pytest.raises(error, match='routing_attention'):
      ra.routing_attention(**dict(ok, **change))
  assert ra.kernel_supports(64, 64) and ra.kernel_supports(128, 1)
  assert not ra.kernel_supports(64, 65) and not ra.kernel_supports(32, 4)
  p = asp.RoutingAttention.Params().Set(
      name='a', input_dim=16, hidden_dim=16, num_heads=2, routing_impl='hip')
  with pytest.raises(AssertionError):
    p.Instantiate()
