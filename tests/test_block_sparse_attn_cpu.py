"""ops/block_sparse_attn.py on the CPU: the tile lists the kernels walk, and
the dense twin against the layer's composed path."""

import pytest
import torch

from lingvo_amd.layers import attention_sparse as asp
from lingvo_amd.ops import block_sparse_attn as bsa

ASYM = [[1, 0, 1], [0, 1, 0], [1, 1, 0]]

LIST_CASES = [
    ([[1]], 64, 64, False),
    (ASYM, 64, 130, False),                          # ragged tail tile
    (ASYM, 64, 130, True),
    (asp.LocalGlobalBlockMask(3, 1, 1), 128, 300, False),   # 2 tiles a block
    (asp.LocalGlobalBlockMask(3, 1, 1), 128, 300, True),
    ([[1, 0, 0], [0, 0, 0], [1, 0, 1]], 64, 192, False),    # empty row, column
    (asp.LocalGlobalBlockMask(7, 1, 0), 64, 448, False),    # gaps in the lists
]


@pytest.mark.parametrize('mask,bs,t,causal', LIST_CASES)
def test_tile_lists_cover_exactly_the_visible_tiles(mask, bs, t, causal):
  pos = torch.arange(t)
  dense = torch.tensor(mask, dtype=torch.bool)[pos[:, None] // bs,
                                               pos[None, :] // bs]
  if causal:
    dense = dense & (pos[None, :] <= pos[:, None])
  nt = -(-t // 64)
  padded = torch.zeros(nt * 64, nt * 64, dtype=torch.bool)
  padded[:t, :t] = dense
  want = padded.reshape(nt, 64, nt, 64).any(3).any(1)      # [QT,KT]
  q_ptr, q_cols, k_ptr, k_rows, q_order, k_order = bsa.tile_lists(
      mask, bs, t, causal)
  for ptr, idx, order, tiles in ((q_ptr, q_cols, q_order, want),
                                 (k_ptr, k_rows, k_order, want.t())):
    assert ptr.dtype == idx.dtype == order.dtype == torch.int32
    assert sorted(order.tolist()) == list(range(nt))   # longest list first
    assert tiles.sum(1)[order.long()].diff().le(0).all()
    assert ptr.shape == (nt + 1,) and int(ptr[0]) == 0
    assert int(ptr[-1]) == idx.numel()
    for i in range(nt):
      got = idx[int(ptr[i]):int(ptr[i + 1])].tolist()
      assert got == tiles[i].nonzero().flatten().tolist(), i  # ascending too


@pytest.mark.parametrize('causal', [False, True])
def test_twin_equals_the_layers_composed_path(causal):
  layer = asp.BlockSparseAttention.Params().Set(
      name='a', input_dim=32, hidden_dim=32, num_heads=2, random_seed=21,
      block_size=4, block_mask=ASYM, causal=causal).Instantiate()
  g = torch.Generator().manual_seed(12)
  x = torch.randn(2, 11, 32, generator=g)
  pad = torch.zeros(2, 11)
  pad[1, 6:] = 1.0
  q, k, v = layer._Project(layer.theta, x)
  want = layer._ComposedContext(q, k, v, pad)
  got = bsa.block_sparse_attention(q, k, v, ASYM, 4,
                                   klen=torch.tensor([11, 6]), causal=causal,
                                   impl='torch')
  assert torch.equal(got, want)
