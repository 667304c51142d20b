"""Flash-attention autograd wrapper.

`flash_attention(q, k, v, ...)` with [B, T, N, H] tensors. On GPU it runs
the hand-written gfx950 kernel; on CPU a composed fp32 torch reference
with identical mask semantics (used as the numerics oracle in tests).

Mask semantics: key k visible from query q iff
  k < klen[b] AND (win_l < 0 or k >= q - win_l)
              AND (win_r < 0 or k <= q + win_r)
Causal attention = win_r=0. LocalSelfAttention = finite (win_l, win_r)
(reference batch_major_attention.py:2656). Optional clipped relative
position bias table [N, 2*bias_clip+1] indexed by clamp(q-k) + clip.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from lingvo_amd.ops import _loader
from lingvo_amd.ops import fusion


def _ref_attention(q, k, v, klen, bias, win_l, win_r, bias_clip, scale,
                   q_segment_ids=None, k_segment_ids=None,
                   chunk_size=0, left_chunks=0):
  """fp32 reference with identical semantics (any backend); float64
  inputs are computed in float64."""
  B, T, N, H = q.shape
  S, NKV = k.shape[1], k.shape[2]
  group = N // NKV
  ft = torch.float64 if q.dtype == torch.float64 else torch.float32
  qf = q.to(ft).permute(0, 2, 1, 3)  # [B,N,T,H]
  kf = k.to(ft).permute(0, 2, 1, 3)
  vf = v.to(ft).permute(0, 2, 1, 3)
  if group > 1:
    kf = kf.repeat_interleave(group, dim=1)
    vf = vf.repeat_interleave(group, dim=1)
  logits = torch.einsum('bnth,bnsh->bnts', qf, kf) * scale
  qpos = torch.arange(T, device=q.device)[:, None]
  kpos = torch.arange(S, device=q.device)[None, :]
  if bias is not None:
    d = (qpos - kpos).clamp(-bias_clip, bias_clip) + bias_clip
    logits = logits + bias.to(ft)[:, d]  # [N,T,S] broadcast over B
  mask = torch.ones(T, S, dtype=torch.bool, device=q.device)
  if win_l >= 0:
    mask &= kpos >= qpos - win_l
  if win_r >= 0:
    mask &= kpos <= qpos + win_r
  if chunk_size > 0:
    qc, kc = qpos // chunk_size, kpos // chunk_size
    mask &= (kc <= qc) & (kc >= qc - left_chunks)
  mask = mask[None, None]
  if klen is not None:
    mask = mask & (kpos[None, None] < klen[:, None, None, None])
  if q_segment_ids is not None:
    seg = (q_segment_ids[:, :, None] == k_segment_ids[:, None, :])
    mask = mask & seg[:, None]
  logits = logits.masked_fill(~mask, -1e30)
  probs = torch.softmax(logits, dim=-1)
  # fully-masked rows -> 0
  probs = torch.where(mask.any(-1, keepdim=True), probs,
                      torch.zeros_like(probs))
  out = torch.einsum('bnts,bnsh->bnth', probs, vf)
  return out.permute(0, 2, 1, 3)


class _FlashAttnFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, q, k, v, klen, bias, qseg, kseg, win_l, win_r,
              bias_clip, scale, chunk_size, left_chunks, bwd_route='auto'):
    ext = _loader.get_ext(required=True)
    bias_b = None if bias is None else bias.to(torch.bfloat16).contiguous()
    o, lse = ext.fa_fwd(q, k, v, klen, bias_b, qseg, kseg, win_l, win_r,
                        bias_clip, scale, chunk_size, left_chunks)
    empty = torch.empty(0)
    ctx.bwd_route = bwd_route
    ctx.save_for_backward(q, k, v, o, lse,
                          klen if klen is not None else empty,
                          bias_b if bias_b is not None else empty,
                          qseg if qseg is not None else empty,
                          kseg if kseg is not None else empty)
    ctx.cfg = (win_l, win_r, bias_clip, scale, bias is not None and
               bias.requires_grad, None if bias is None else bias.dtype,
               chunk_size, left_chunks)
    return o

  @staticmethod
  def backward(ctx, dout):
    ext = _loader.get_ext(required=True)
    q, k, v, o, lse, klen, bias_b, qseg, kseg = ctx.saved_tensors
    (win_l, win_r, bias_clip, scale, bias_grad, bias_dtype, chunk_size,
     left_chunks) = ctx.cfg
    klen = klen if klen.numel() else None
    bias_b = bias_b if bias_b.numel() else None
    qseg = qseg if qseg.numel() else None
    kseg = kseg if kseg.numel() else None
    dq, dk, dv, dbias = ext.fa_bwd(
        dout.contiguous(), q, k, v, o, lse, klen, bias_b, qseg, kseg,
        bias_grad, win_l, win_r, bias_clip, scale, chunk_size,
        left_chunks, route=ctx.bwd_route)
    dbias_out = dbias.to(bias_dtype) if bias_grad else None
    return (dq, dk, dv, None, dbias_out, None, None, None, None, None,
            None, None, None, None)


class _FlashAttnPackedFn(torch.autograd.Function):
  """Self-attention on the packed projection output qkv [B,T,3*N*H]
  (N == NKV). The kernels read q/k/v as strided views of qkv, and the
  backward writes dq/dk/dv into the matching views of one dqkv buffer, so
  neither the three input copies nor the split-backward cat exist."""

  @staticmethod
  def _views(t, n, h):
    return [x.unflatten(-1, (n, h)) for x in t.split(n * h, dim=-1)]

  @staticmethod
  def forward(ctx, qkv, n, h, klen, bias, qseg, kseg, win_l, win_r,
              bias_clip, scale, chunk_size, left_chunks, bwd_route='auto'):
    ext = _loader.get_ext(required=True)
    ctx.bwd_route = bwd_route
    bias_b = None if bias is None else bias.to(torch.bfloat16).contiguous()
    q, k, v = _FlashAttnPackedFn._views(qkv, n, h)
    o, lse = ext.fa_fwd(q, k, v, klen, bias_b, qseg, kseg, win_l, win_r,
                        bias_clip, scale, chunk_size, left_chunks)
    empty = torch.empty(0)
    ctx.save_for_backward(qkv, o, lse,
                          klen if klen is not None else empty,
                          bias_b if bias_b is not None else empty,
                          qseg if qseg is not None else empty,
                          kseg if kseg is not None else empty)
    ctx.cfg = (n, h, win_l, win_r, bias_clip, scale, bias is not None and
               bias.requires_grad, None if bias is None else bias.dtype,
               chunk_size, left_chunks)
    return o

  @staticmethod
  def backward(ctx, dout):
    ext = _loader.get_ext(required=True)
    qkv, o, lse, klen, bias_b, qseg, kseg = ctx.saved_tensors
    (n, h, win_l, win_r, bias_clip, scale, bias_grad, bias_dtype,
     chunk_size, left_chunks) = ctx.cfg
    klen = klen if klen.numel() else None
    bias_b = bias_b if bias_b.numel() else None
    qseg = qseg if qseg.numel() else None
    kseg = kseg if kseg.numel() else None
    q, k, v = _FlashAttnPackedFn._views(qkv, n, h)
    dqkv = torch.empty_like(qkv)
    dq, dk, dv = _FlashAttnPackedFn._views(dqkv, n, h)
    dbias = ext.fa_bwd(
        dout.contiguous(), q, k, v, o, lse, klen, bias_b, qseg, kseg,
        bias_grad, win_l, win_r, bias_clip, scale, chunk_size,
        left_chunks, dq, dk, dv, ctx.bwd_route)[3]
    dbias_out = dbias.to(bias_dtype) if bias_grad else None
    return (dqkv, None, None, None, dbias_out, None, None, None, None,
            None, None, None, None, None)


def flash_attention_packed(qkv: torch.Tensor, num_heads: int,
                           klen: Optional[torch.Tensor] = None,
                           bias: Optional[torch.Tensor] = None,
                           win_l: int = -1, win_r: int = -1,
                           bias_clip: int = 127,
                           scale: Optional[float] = None,
                           q_segment_ids: Optional[torch.Tensor] = None,
                           k_segment_ids: Optional[torch.Tensor] = None,
                           chunk_size: int = 0, left_chunks: int = 0,
                           bwd_route: str = 'auto') -> torch.Tensor:
  """flash_attention on a packed self-attention projection: qkv is
  [B,T,3*N*H] bf16 CUDA laid out [q | k | v] with N == NKV == num_heads.
  Returns o [B,T,N,H]; the gradient is one [B,T,3*N*H] tensor.
  bwd_route forces the backward kernel (see flash_attention)."""
  assert qkv.is_cuda and qkv.dtype == torch.bfloat16
  assert qkv.shape[-1] % (3 * num_heads) == 0
  h = qkv.shape[-1] // (3 * num_heads)
  if scale is None:
    scale = 1.0 / math.sqrt(h)
  if klen is not None:
    klen = klen.to(torch.int32).contiguous()
  if q_segment_ids is not None:
    q_segment_ids = q_segment_ids.to(torch.int32).contiguous()
    k_segment_ids = k_segment_ids.to(torch.int32).contiguous()
  return _FlashAttnPackedFn.apply(
      qkv.contiguous(), num_heads, h, klen, bias, q_segment_ids,
      k_segment_ids, win_l, win_r, bias_clip, scale, chunk_size,
      left_chunks, bwd_route)


def _meets_stride_contract(t: torch.Tensor) -> bool:
  """The kernels' contract for q/k/v (flash_attn.hip check_strided_btnh):
  dense [N][H], one uniform token-row stride that is a multiple of 8
  elements, 16-byte aligned base."""
  if t.dim() != 4 or t.dtype != torch.bfloat16:
    return False
  b, s, n, h = t.shape
  if t.stride(3) != 1 or t.stride(2) != h:
    return False
  row = t.stride(1)
  return (row % 8 == 0 and row >= n * h and t.stride(0) == s * row and
          t.data_ptr() % 16 == 0)


def _kernel_input(t: torch.Tensor) -> torch.Tensor:
  t = t.to(torch.bfloat16)
  if fusion.enabled() and _meets_stride_contract(t):
    return t  # e.g. a split of a packed projection: no copy
  return t.contiguous()


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    klen: Optional[torch.Tensor] = None,
                    bias: Optional[torch.Tensor] = None,
                    win_l: int = -1, win_r: int = -1,
                    bias_clip: int = 127,
                    scale: Optional[float] = None,
                    q_segment_ids: Optional[torch.Tensor] = None,
                    k_segment_ids: Optional[torch.Tensor] = None,
                    chunk_size: int = 0, left_chunks: int = 0,
                    bwd_route: str = 'auto') -> torch.Tensor:
  """q [B,T,N,H], k/v [B,S,NKV,H] -> [B,T,N,H]. Optional packed-input
  segment ids [B,T]/[B,S]: attention is blocked across segments
  (reference PackSequences segment_ids consumed by the mask path).

  bwd_route picks the GPU backward kernel: 'auto' (by shape), 'tiles'
  (one workgroup per 128-key tile, dQ through fp32 atomics) or 'fused'
  (one workgroup per head; raises where the shape does not qualify)."""
  if scale is None:
    scale = 1.0 / math.sqrt(q.shape[-1])
  if klen is not None:
    klen = klen.to(torch.int32).contiguous()
  if q_segment_ids is not None:
    q_segment_ids = q_segment_ids.to(torch.int32).contiguous()
    k_segment_ids = k_segment_ids.to(torch.int32).contiguous()
  if q.is_cuda:
    orig = q.dtype
    out = _FlashAttnFn.apply(
        _kernel_input(q), _kernel_input(k), _kernel_input(v), klen, bias,
        q_segment_ids, k_segment_ids, win_l, win_r, bias_clip, scale,
        chunk_size, left_chunks, bwd_route)
    return out.to(orig) if orig != torch.bfloat16 else out
  out = _ref_attention(q, k, v, klen, bias, win_l, win_r, bias_clip, scale,
                       q_segment_ids, k_segment_ids, chunk_size,
                       left_chunks)
  return out.to(q.dtype)
