"""Softmax attention under a static block-level visibility pattern.

  o = block_sparse_attention(q, k, v, block_mask, block_size, klen=None,
                             causal=False, scale=None, impl='auto')

q, k, v [B,T,N,H] (self-attention: one length, N == NKV); block_mask a
bool / 0-1 tensor or nested list [QB,KB] with QB, KB >= ceil(T/block_size),
shared over batch and heads; klen [B] integer or None. Key k is visible from
query q iff

  block_mask[q // block_size][k // block_size]  and  k < klen[b]
  and (not causal or k <= q).

A query row with no visible key outputs 0 and has zero gradient. scale
defaults to H^(-1/2).

CUDA bf16 tensors with H in {64, 128} and block_size a positive multiple of
64 run the HIP kernels of ops/hip/block_sparse_attn.hip. The kernels work on
64x64 tiles and walk explicit tile lists that `tile_lists` builds on the
host from the static pattern (larger blocks are expanded into 64-token
tiles; causal drops the tiles wholly above the diagonal): work and memory
scale with the number of visible tiles, and no [T,T] tensor exists forward
or backward. The lists are cached on the device per pattern, block size, T,
causal and device. A hot caller passes block_mask as a CPU tensor: the cache
key is its bytes, a nested list is converted on every call (0.6 ms of host
time at 64x64 blocks against 0.02 ms for the tensor) and a CUDA mask is copied back. Other CUDA
inputs are refused by impl='auto' with the limit named. CPU tensors run the
dense masked twin `_ref_block_sparse_attention` (fp32, or fp64 for fp64
inputs); impl='torch' runs the twin on either device: the yardstick for
tests and timing.
"""

from __future__ import annotations

import functools
import math
from typing import Optional

import torch

from lingvo_amd.ops import _loader

# What the kernels are written for.
KERNEL_HEAD_DIMS = (64, 128)
KERNEL_TILE = 64


def kernel_supports(h: int, block_size: int) -> bool:
  return (h in KERNEL_HEAD_DIMS and block_size > 0 and
          block_size % KERNEL_TILE == 0)


def _RoundTo(x, dtype):
  """x rounded to dtype, kept in its own; straight-through for autograd."""
  return x + (x.detach().to(dtype).to(x.dtype) - x.detach())


def _HostMask(block_mask, block_size, t):
  """block_mask as a CPU bool [QB,KB] tensor, checked against T."""
  bm = torch.as_tensor(block_mask).detach().cpu()
  if bm.dim() != 2:
    raise ValueError('block_sparse_attention: block_mask must be [QB,KB], '
                     f'got {tuple(bm.shape)}')
  if block_size < 1:
    raise ValueError('block_sparse_attention: block_size must be >= 1, got '
                     f'{block_size}')
  need = -(-t // block_size)
  if bm.shape[0] < need or bm.shape[1] < need:
    raise ValueError(
        f'block_sparse_attention: block_mask {tuple(bm.shape)} is smaller '
        f'than ceil(T/block_size) = {need} blocks')
  return bm != 0


def _ref_block_sparse_attention(q, k, v, block_mask, block_size, klen=None,
                                causal=False, scale=None, operand_dtype=None):
  """Dense masked twin of the math in the module docstring; fp32, or fp64
  for fp64 inputs. With operand_dtype the probabilities are rounded to it
  before the contraction with v, whose sums stay wide."""
  b, t, n, h = q.shape
  ft = torch.float64 if q.dtype == torch.float64 else torch.float32
  scale = 1.0 / math.sqrt(h) if scale is None else scale
  bm = _HostMask(block_mask, block_size, t).to(q.device)
  tpos = torch.arange(t, device=q.device)
  blk = tpos // block_size
  mask = bm[blk[:, None], blk[None, :]]
  if causal:
    mask = mask & (tpos[None, :] <= tpos[:, None])
  mask4 = mask[None, None]
  if klen is not None:
    mask4 = mask4 & (tpos[None, :] < klen[:, None])[:, None, None, :]
  logits = torch.einsum('btnh,bsnh->bnts', q.to(ft), k.to(ft)) * scale
  logits = logits.masked_fill(~mask4, -1e30)
  probs = torch.softmax(logits, dim=-1)
  probs = torch.where(mask4.any(-1, keepdim=True), probs,
                      torch.zeros_like(probs))
  if operand_dtype is not None:
    probs = _RoundTo(probs, operand_dtype)
  return torch.einsum('bnts,bsnh->btnh', probs, v.to(ft))


def tile_lists(block_mask, block_size: int, t: int, causal: bool = False):
  """-> (q_ptr, q_cols, k_ptr, k_rows, q_order, k_order), int32 CPU tensors
  at 64-token granularity. q_ptr [QT+1] and q_cols [nnz]: for each 64-row
  query tile the ascending 64-key tiles that hold a visible element; k_ptr,
  k_rows: the transpose, per key tile its query tiles. q_order, k_order
  [QT]: the tiles by falling list length, the order in which the kernels
  dispatch them (longest first). klen is not part of the lists; the
  kernels cut them short."""
  if block_size < 1 or block_size % KERNEL_TILE:
    raise ValueError('tile_lists: block_size must be a positive multiple of '
                     f'{KERNEL_TILE}, got {block_size}')
  bm = _HostMask(block_mask, block_size, t)
  nt = -(-t // KERNEL_TILE)
  tile = torch.arange(nt)
  blk = tile * KERNEL_TILE // block_size
  tiles = bm[blk[:, None], blk[None, :]]             # [QT,KT]
  if causal:  # a tile holds some k <= q iff it is not above the diagonal
    tiles = tiles & (tile[None, :] <= tile[:, None])

  def csr(m):
    ptr = torch.zeros(nt + 1, dtype=torch.int32)
    ptr[1:] = m.sum(1).cumsum(0)
    order = torch.argsort(m.sum(1), descending=True, stable=True)
    # nonzero is row-major: ascending within a row.
    return ptr, m.nonzero()[:, 1].to(torch.int32), order.to(torch.int32)

  q, k = csr(tiles), csr(tiles.t())
  return q[:2] + k[:2] + (q[2], k[2])


@functools.lru_cache(maxsize=256)
def _CachedLists(mask_bytes, mask_shape, block_size, t, causal, device):
  bm = torch.frombuffer(bytearray(mask_bytes),
                        dtype=torch.bool).reshape(mask_shape)
  return tuple(x.to(device) for x in tile_lists(bm, block_size, t, causal))


def _DeviceLists(block_mask, block_size, t, causal, device):
  """tile_lists on `device`, built and uploaded once per pattern."""
  need = -(-t // block_size)
  bm = _HostMask(block_mask, block_size, t)[:need, :need].contiguous()
  return _CachedLists(bm.numpy().tobytes(), tuple(bm.shape), block_size, t,
                      causal, str(device))


class _BlockSparseAttnFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, q, k, v, klen, lists, causal, scale):
    ext = _loader.get_ext(required=True)
    o, lse = ext.bsa_fwd(q, k, v, klen, lists[0], lists[1], lists[4], causal,
                         scale)
    ctx.save_for_backward(q, k, v, o, lse,
                          klen if klen is not None else torch.empty(0), *lists)
    ctx.causal, ctx.scale = causal, scale
    return o

  @staticmethod
  def backward(ctx, dout):
    ext = _loader.get_ext(required=True)
    (q, k, v, o, lse, klen, q_ptr, q_cols, k_ptr, k_rows, q_order,
     k_order) = ctx.saved_tensors
    dq, dk, dv = ext.bsa_bwd(
        dout.contiguous(), q, k, v, o, lse, klen if klen.numel() else None,
        q_ptr, q_cols, q_order, k_ptr, k_rows, k_order, ctx.causal, ctx.scale)
    return dq, dk, dv, None, None, None, None


def _CheckArgs(q, k, v, klen, fn='block_sparse_attention'):
  if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
    raise ValueError(f'{fn}: q, k and v must be [B,T,N,H], got '
                     f'{tuple(q.shape)}, {tuple(k.shape)} and '
                     f'{tuple(v.shape)}')
  b, t = q.shape[:2]
  if b < 1 or t < 1:
    raise ValueError(f'{fn}: B >= 1 and T >= 1')
  if k.shape != q.shape or v.shape != q.shape:
    raise ValueError(f'{fn}: self-attention only: k and v must have the '
                     f'shape of q (S == T, N == NKV), got {tuple(k.shape)} '
                     f'and {tuple(v.shape)} for {tuple(q.shape)}')
  for name, x in (('q', q), ('k', k), ('v', v)):
    if not x.is_floating_point():
      raise TypeError(f'{fn}: {name} must be floating point, got {x.dtype}')
    if x.dtype != q.dtype:
      raise TypeError(f'{fn}: {name} is {x.dtype} but q is {q.dtype}')
  if klen is not None:
    if klen.dim() != 1 or klen.shape[0] != b or klen.is_floating_point() or \
        klen.dtype == torch.bool:
      raise TypeError(f'{fn}: klen must be an integer tensor [B]')
  for x in (k, v) + (() if klen is None else (klen,)):
    if x.device != q.device:
      raise ValueError(f'{fn}: all inputs must be on one device')


def block_sparse_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                           block_mask, block_size: int,
                           klen: Optional[torch.Tensor] = None,
                           causal: bool = False,
                           scale: Optional[float] = None,
                           impl: str = 'auto') -> torch.Tensor:
  """-> o [B,T,N,H]; see the module docstring."""
  if impl not in ('auto', 'torch'):
    raise ValueError("block_sparse_attention: impl must be 'auto' or "
                     f"'torch', got {impl!r}")
  _CheckArgs(q, k, v, klen)
  causal = bool(causal)
  block_size = int(block_size)
  t, h = q.shape[1], q.shape[3]
  scale = 1.0 / math.sqrt(h) if scale is None else float(scale)
  if impl == 'torch' or not q.is_cuda:
    return _ref_block_sparse_attention(q, k, v, block_mask, block_size, klen,
                                       causal, scale).to(q.dtype)
  if q.dtype != torch.bfloat16:
    raise TypeError(
        f'block_sparse_attention: the HIP kernels take bf16, got {q.dtype}')
  if not kernel_supports(h, block_size):
    raise ValueError(
        f'block_sparse_attention: the HIP kernels support H in '
        f'{KERNEL_HEAD_DIMS} with block_size a positive multiple of '
        f'{KERNEL_TILE}, got H={h}, block_size={block_size}')
  lists = _DeviceLists(block_mask, block_size, t, causal, q.device)
  if klen is not None:
    klen = klen.to(torch.int32).contiguous()
  return _BlockSparseAttnFn.apply(q.contiguous(), k.contiguous(),
                                  v.contiguous(), klen, lists, causal, scale)
