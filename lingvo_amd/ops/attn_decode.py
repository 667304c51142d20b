"""Cached (KV-cache) attention: the attention block of
MultiHeadedAttention.ExtendStep / StreamStep as one op.

`cached_attention(q, key_cache, value_cache, q_start, ...)` with q
[B, C, N, H] and caches [B, Smax, NKV, H] that already hold the rows for
positions < q_start + C (the append stays with the caller). Query row i sits
at position p = q_start + i; key j is visible iff

  j <= p AND (win_l < 0 or j >= p - win_l)

and the optional clipped relative-position bias [N, 2*bias_clip+1] is
indexed by clamp(p - j, -bias_clip, bias_clip) + bias_clip. `q_start` is a
host int or an int32 [B] tensor (per-row lengths, no host sync).

On bf16 CUDA tensors it runs ops/hip/attn_decode.hip (a split-K decode
kernel and a combine kernel); on CPU, for other dtypes and with
impl='torch' the composed fp32 twin below, which is the arithmetic
ExtendStep / StreamStep used to carry inline.
"""

from __future__ import annotations

import math
import numbers
from typing import Optional, Union

import torch

from lingvo_amd.ops import _loader

MAX_ROWS = 64  # C * (N / NKV) the kernel takes (attn_decode.hip AD_MAX_ROWS)
_HEAD_DIMS = (64, 128)
_IMPLS = ('auto', 'torch', 'hip')


def _twin(q, key_cache, value_cache, q_start, bias, win_l, bias_clip, scale):
  """Composed reference, fp32 (float64 for float64 q). Returns the compute
  dtype, [B, C, N, H]."""
  b, c, n, h = q.shape
  smax, nkv = key_cache.shape[1], key_cache.shape[2]
  group = n // nkv
  ft = torch.float64 if q.dtype == torch.float64 else torch.float32
  L = win_l if win_l >= 0 else smax
  dev = q.device
  if isinstance(q_start, torch.Tensor):
    lo, hi = 0, smax
    qpos = (q_start.to(dev).long()[:, None] +
            torch.arange(c, device=dev))[:, :, None]          # [B, C, 1]
  else:
    lo, hi = max(0, q_start - L), q_start + c
    qpos = (q_start + torch.arange(c, device=dev))[:, None]   # [C, 1]
  kf = key_cache[:, lo:hi].to(ft)
  vf = value_cache[:, lo:hi].to(ft)
  if group > 1:
    kf = kf.repeat_interleave(group, dim=2)
    vf = vf.repeat_interleave(group, dim=2)
  logits = torch.einsum('bcnh,bsnh->bncs', q.to(ft), kf)
  logits = logits / math.sqrt(h) if scale is None else logits * scale
  kpos = lo + torch.arange(hi - lo, device=dev)               # [S]
  mask = (kpos <= qpos) & (kpos >= qpos - L)
  if bias is not None:
    d = (qpos - kpos).clamp(-bias_clip, bias_clip) + bias_clip
    rel = bias.to(ft)[:, d]                    # [N, C, S] or [N, B, C, S]
    logits = logits + (rel[None] if d.dim() == 2 else rel.transpose(0, 1))
  mask = mask[None, None] if mask.dim() == 2 else mask[:, None]
  logits = logits.masked_fill(~mask, -1e30)
  probs = torch.softmax(logits, dim=-1)
  return torch.einsum('bncs,bsnh->bcnh', probs, vf)


def _check_common(q, key_cache, value_cache, q_start, bias, win_l, bias_clip,
                  num_splits, impl):
  if impl not in _IMPLS:
    raise ValueError(f'impl must be one of {_IMPLS}, got {impl!r}')
  if q.dim() != 4 or key_cache.dim() != 4:
    raise ValueError('q must be [B,C,N,H] and the caches [B,Smax,NKV,H]')
  b, c, n, h = q.shape
  smax, nkv = key_cache.shape[1], key_cache.shape[2]
  if (key_cache.shape[0] != b or key_cache.shape[3] != h or
      value_cache.shape != key_cache.shape):
    raise ValueError(
        f'caches must both be [B={b},Smax,NKV,H={h}], got '
        f'{tuple(key_cache.shape)} and {tuple(value_cache.shape)}')
  if nkv < 1 or n % nkv != 0:
    raise ValueError(f'GQA requires N % NKV == 0, got N={n} NKV={nkv}')
  if c < 1 or c > smax:
    raise ValueError(f'need 1 <= C <= Smax, got C={c} Smax={smax}')
  if isinstance(q_start, torch.Tensor):
    if (q_start.dim() != 1 or q_start.shape[0] != b or
        q_start.dtype != torch.int32):
      raise ValueError('a q_start tensor must be int32 [B]')
  else:
    if not isinstance(q_start, numbers.Integral):
      raise ValueError('q_start must be an int or an int32 [B] tensor')
    if q_start < 0 or q_start + c > smax:
      raise ValueError(
          f'need 0 <= q_start and q_start + C <= Smax, got q_start='
          f'{q_start} C={c} Smax={smax}')
  if bias is not None:
    if bias_clip < 0 or tuple(bias.shape) != (n, 2 * bias_clip + 1):
      raise ValueError(
          f'bias must be [N={n}, 2*bias_clip+1={2 * bias_clip + 1}], got '
          f'{tuple(bias.shape)}')
  if num_splits < 0:
    raise ValueError(f'num_splits must be >= 0, got {num_splits}')


def _meets_stride_contract(t: torch.Tensor) -> bool:
  """flash_attn._meets_stride_contract (dense [N][H], one uniform token-row
  stride that is a multiple of 8 elements, 16-byte aligned base), with the
  stride of a size-1 dim left free as in attn_decode.hip: q of a one-token
  step is a [B, 1, N, H] view of the packed projection whose stride(1) is
  whatever reshape chose."""
  b, s, n, h = t.shape
  if t.stride(3) != 1 or (n > 1 and t.stride(2) != h):
    return False
  if s > 1:
    row = t.stride(1)
    if b > 1 and t.stride(0) != s * row:
      return False
  else:
    row = t.stride(0) if b > 1 else n * h
  return row % 8 == 0 and row >= n * h and t.data_ptr() % 16 == 0


def kernel_qualifies(q, key_cache, value_cache) -> bool:
  """Shape/dtype part of the kernel's contract ('auto' takes the twin where
  this is False)."""
  if not (q.is_cuda and key_cache.is_cuda and value_cache.is_cuda):
    return False
  if not (q.dtype == key_cache.dtype == value_cache.dtype == torch.bfloat16):
    return False
  c, n, h = q.shape[1], q.shape[2], q.shape[3]
  return h in _HEAD_DIMS and c * (n // key_cache.shape[2]) <= MAX_ROWS


def cached_attention(q: torch.Tensor, key_cache: torch.Tensor,
                     value_cache: torch.Tensor,
                     q_start: Union[int, torch.Tensor],
                     bias: Optional[torch.Tensor] = None, win_l: int = -1,
                     bias_clip: int = 127, scale: Optional[float] = None,
                     num_splits: int = 0, impl: str = 'auto') -> torch.Tensor:
  """q [B,C,N,H], caches [B,Smax,NKV,H] -> [B,C,N,H] in q's dtype.

  impl: 'auto' runs the HIP kernels on bf16 CUDA tensors with H in
  {64, 128} and C * N/NKV <= 64, the composed twin elsewhere; 'torch'
  always the twin; 'hip' the kernels or an error. num_splits forces the
  key-range split count of the kernel (0: chosen from the shapes).

  The contract is checked before anything is allocated or launched."""
  _check_common(q, key_cache, value_cache, q_start, bias, win_l, bias_clip,
                num_splits, impl)
  if not isinstance(q_start, torch.Tensor):
    q_start = int(q_start)
  use_kernel = impl != 'torch' and kernel_qualifies(q, key_cache, value_cache)
  if impl == 'hip' and not use_kernel:
    raise ValueError(
        "impl='hip' needs bf16 CUDA q and caches, H in {64, 128} and "
        f'C * N/NKV <= {MAX_ROWS}; got q {tuple(q.shape)} {q.dtype} on '
        f'{q.device}, caches {tuple(key_cache.shape)} {key_cache.dtype}')
  if not use_kernel:
    out = _twin(q, key_cache, value_cache, q_start, bias, win_l, bias_clip,
                scale)
    return out.to(q.dtype)
  for name, t in (('q', q), ('key_cache', key_cache),
                  ('value_cache', value_cache)):
    if not _meets_stride_contract(t):
      raise ValueError(
          f'{name}: needs dense [N][H], a row stride that is a multiple of '
          f'8 elements and a 16-byte aligned base; got strides {t.stride()}')
  ext = _loader.get_ext(required=True)
  qs_t, qs_i = None, 0
  if isinstance(q_start, torch.Tensor):
    if not q_start.is_cuda:
      raise ValueError('a q_start tensor must live on the GPU')
    qs_t = q_start.contiguous()
  else:
    qs_i = q_start
  if bias is not None:
    if not bias.is_cuda:
      raise ValueError('bias must live on the GPU')
    if bias.dtype not in (torch.bfloat16, torch.float32):
      bias = bias.float()
    bias = bias.contiguous()
  if scale is None:
    scale = 1.0 / math.sqrt(q.shape[-1])
  return ext.attn_decode(q, key_cache, value_cache, qs_t, qs_i, bias,
                         int(win_l), int(bias_clip), float(scale),
                         int(num_splits))
