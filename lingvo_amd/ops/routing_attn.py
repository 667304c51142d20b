"""Softmax attention within k-means clusters (routing attention).

  o = routing_attention(q, k, v, q_cl, k_cl, num_clusters, window,
                        paddings=None, causal=False, scale=None, impl='auto')

q, k, v [B,T,N,H] (self-attention: one length, N == NKV); q_cl, k_cl integer
[B,N,T] with values in [0, num_clusters), the layout RoutingAttention._Route
returns; paddings [B,T] or None. A key is live iff paddings < 0.5 (holes are
allowed; it is not a length). Key s is visible from query t of the same
(b, n) iff

  k_cl[s] == q_cl[t]  and  s is live
  and fewer than `window` live keys of that cluster precede s
  and (not causal or s <= t).

A query with no visible key outputs 0 and has zero gradient; a key no query
sees has zero gradient. scale defaults to H^(-1/2).

CUDA bf16 tensors with H in {64, 128} and num_clusters <= 64 run the HIP
kernels of ops/hip/routing_attn.hip: a list kernel sorts the queries by
cluster and gathers each cluster's first `window` live keys on the device,
and the attention kernels walk those lists in 64x64 tiles, so a query costs
its own cluster's keys only and no [T,window] tensor exists forward or
backward. Nothing about the ids is read on the host: the op captures into a
graph. Other CUDA inputs are refused by impl='auto' with the limit named. CPU
tensors run the dense masked twin `_ref_routing_attention` (fp32, or fp64 for
fp64 inputs); impl='torch' runs the twin on either device: the yardstick for
tests.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from lingvo_amd.ops import _loader
from lingvo_amd.ops.block_sparse_attn import _RoundTo

# What the kernels are written for.
KERNEL_HEAD_DIMS = (64, 128)
KERNEL_MAX_CLUSTERS = 64  # one lane of a wave counts one cluster


def kernel_supports(h: int, num_clusters: int) -> bool:
  return h in KERNEL_HEAD_DIMS and 1 <= num_clusters <= KERNEL_MAX_CLUSTERS


def visible_mask(q_cl, k_cl, window, paddings=None, causal=False):
  """bool [B,N,T,S]: the rule of the module docstring."""
  b, n, t = k_cl.shape
  live = torch.ones(b, t, dtype=torch.bool, device=k_cl.device)
  if paddings is not None:
    live = paddings < 0.5
  live = live[:, None, :].expand(b, n, t)
  same = q_cl[:, :, :, None] == k_cl[:, :, None, :]          # [B,N,T,S]
  # Live keys of key s's own cluster before s.
  member = (k_cl[:, :, :, None] == k_cl[:, :, None, :]) & live[:, :, :, None]
  before = torch.tril(member.transpose(2, 3), -1).sum(-1)      # [B,N,S]
  mask = same & (live & (before < window))[:, :, None, :]
  if causal:
    pos = torch.arange(t, device=k_cl.device)
    mask = mask & (pos[None, :] <= pos[:, None])
  return mask


def _ref_routing_attention(q, k, v, q_cl, k_cl, num_clusters, window,
                           paddings=None, causal=False, scale=None,
                           operand_dtype=None):
  """Dense masked twin of the math in the module docstring; fp32, or fp64
  for fp64 inputs. With operand_dtype the probabilities are rounded to it
  before the contraction with v, whose sums stay wide."""
  del num_clusters  # the rule compares ids; their range does not enter
  h = q.shape[3]
  ft = torch.float64 if q.dtype == torch.float64 else torch.float32
  scale = 1.0 / math.sqrt(h) if scale is None else scale
  mask = visible_mask(q_cl, k_cl, window, paddings, causal)
  logits = torch.einsum('btnh,bsnh->bnts', q.to(ft), k.to(ft)) * scale
  logits = logits.masked_fill(~mask, -1e30)
  probs = torch.softmax(logits, dim=-1)
  probs = torch.where(mask.any(-1, keepdim=True), probs,
                      torch.zeros_like(probs))
  if operand_dtype is not None:
    probs = _RoundTo(probs, operand_dtype)
  return torch.einsum('bnts,bsnh->btnh', probs, v.to(ft))


def routing_lists(q, k, v, q_cl, k_cl, num_clusters, window, paddings=None):
  """The kernels' lists, built on the device (ops/hip/routing_attn.hip):
  (q_perm [B,N,T], q_start [B,N,C+1], q_tiles [B,N,QTmax,3], q_ntiles [B,N],
  k_sel [B,N,C,min(window,T)], k_cnt [B,N,C]), int32. Entries of q_tiles past
  q_ntiles and of k_sel past k_cnt are not written."""
  ext = _loader.get_ext(required=True)
  live = None if paddings is None else (paddings < 0.5).contiguous()
  return tuple(ext.routing_lists(q, k, v, q_cl.contiguous(),
                                 k_cl.contiguous(), live, num_clusters,
                                 window))


def _ref_routing_lists(q_cl, k_cl, num_clusters, window, paddings=None):
  """Torch twin of routing_lists from the ids alone; entries the kernel
  leaves unwritten are -1."""
  b, n, t = q_cl.shape
  w, tile = min(window, t), 64
  qtmax = -(-t // tile) + num_clusters - 1
  i32 = dict(dtype=torch.int32, device=q_cl.device)
  live = (torch.ones(b, t, dtype=torch.bool, device=q_cl.device)
          if paddings is None else paddings < 0.5)
  q_perm = torch.sort(q_cl, dim=-1, stable=True).indices.to(torch.int32)
  counts = (q_cl[..., None] == torch.arange(
      num_clusters, device=q_cl.device)).sum(2)
  q_start = torch.nn.functional.pad(counts.cumsum(-1), (1, 0)).to(torch.int32)
  q_tiles = torch.full((b, n, qtmax, 3), -1, **i32)
  q_ntiles = torch.zeros((b, n), **i32)
  k_sel = torch.full((b, n, num_clusters, w), -1, **i32)
  k_cnt = torch.zeros((b, n, num_clusters), **i32)
  for bi in range(b):
    for ni in range(n):
      rows = []
      for c in range(num_clusters):
        s, cnt = int(q_start[bi, ni, c]), int(counts[bi, ni, c])
        rows += [(c, s + j, min(tile, cnt - j)) for j in range(0, cnt, tile)]
        members = ((k_cl[bi, ni] == c) & live[bi]).nonzero()[:w, 0]
        k_sel[bi, ni, c, :len(members)] = members.to(torch.int32)
        k_cnt[bi, ni, c] = len(members)
      q_ntiles[bi, ni] = len(rows)
      q_tiles[bi, ni, :len(rows)] = torch.tensor(rows, **i32)
  return q_perm, q_start, q_tiles, q_ntiles, k_sel, k_cnt


class _RoutingAttnFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, q, k, v, q_cl, k_cl, paddings, num_clusters, window,
              causal, scale):
    ext = _loader.get_ext(required=True)
    lists = routing_lists(q, k, v, q_cl, k_cl, num_clusters, window, paddings)
    o, lse = ext.routing_attn_fwd(q, k, v, list(lists), num_clusters, window,
                                  causal, scale)
    ctx.save_for_backward(q, k, v, o, lse, *lists)
    ctx.args = (num_clusters, window, causal, scale)
    return o

  @staticmethod
  def backward(ctx, dout):
    ext = _loader.get_ext(required=True)
    q, k, v, o, lse, *lists = ctx.saved_tensors
    dq, dk, dv = ext.routing_attn_bwd(dout.contiguous(), q, k, v, o, lse,
                                      lists, *ctx.args)
    return (dq, dk, dv) + (None,) * 7


def _CheckArgs(q, k, v, q_cl, k_cl, num_clusters, window, paddings,
               fn='routing_attention'):
  if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
    raise ValueError(f'{fn}: q, k and v must be [B,T,N,H], got '
                     f'{tuple(q.shape)}, {tuple(k.shape)} and '
                     f'{tuple(v.shape)}')
  b, t, n = q.shape[:3]
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
  for name, x in (('q_cl', q_cl), ('k_cl', k_cl)):
    if x.dtype not in (torch.int32, torch.int64):
      raise TypeError(f'{fn}: {name} must be int32 or int64, got {x.dtype}')
    if tuple(x.shape) != (b, n, t):
      raise ValueError(f'{fn}: {name} must be [B,N,T] = {(b, n, t)}, got '
                       f'{tuple(x.shape)}')
  if q_cl.dtype != k_cl.dtype:
    raise TypeError(f'{fn}: q_cl is {q_cl.dtype} but k_cl is {k_cl.dtype}')
  if num_clusters < 1:
    raise ValueError(f'{fn}: num_clusters must be >= 1, got {num_clusters}')
  if window < 1:
    raise ValueError(f'{fn}: window must be >= 1, got {window}')
  if paddings is not None and tuple(paddings.shape) != (b, t):
    raise ValueError(f'{fn}: paddings must be [B,T] = {(b, t)}, got '
                     f'{tuple(paddings.shape)}')
  for x in (k, v, q_cl, k_cl) + (() if paddings is None else (paddings,)):
    if x.device != q.device:
      raise ValueError(f'{fn}: all inputs must be on one device')


def routing_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                      q_cl: torch.Tensor, k_cl: torch.Tensor,
                      num_clusters: int, window: int,
                      paddings: Optional[torch.Tensor] = None,
                      causal: bool = False, scale: Optional[float] = None,
                      impl: str = 'auto') -> torch.Tensor:
  """-> o [B,T,N,H]; see the module docstring."""
  if impl not in ('auto', 'torch'):
    raise ValueError("routing_attention: impl must be 'auto' or 'torch', got "
                     f'{impl!r}')
  num_clusters, window, causal = int(num_clusters), int(window), bool(causal)
  _CheckArgs(q, k, v, q_cl, k_cl, num_clusters, window, paddings)
  h = q.shape[3]
  scale = 1.0 / math.sqrt(h) if scale is None else float(scale)
  if impl == 'torch' or not q.is_cuda:
    return _ref_routing_attention(q, k, v, q_cl, k_cl, num_clusters, window,
                                  paddings, causal, scale).to(q.dtype)
  if q.dtype != torch.bfloat16:
    raise TypeError(
        f'routing_attention: the HIP kernels take bf16, got {q.dtype}')
  if not kernel_supports(h, num_clusters):
    raise ValueError(
        f'routing_attention: the HIP kernels support H in {KERNEL_HEAD_DIMS} '
        f'with num_clusters <= {KERNEL_MAX_CLUSTERS}, got H={h}, '
        f'num_clusters={num_clusters}')
  return _RoutingAttnFn.apply(q.contiguous(), k.contiguous(), v.contiguous(),
                              q_cl, k_cl, paddings, num_clusters, window,
                              causal, scale)
