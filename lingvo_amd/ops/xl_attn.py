"""Transformer-XL relative attention (Dai et al. 2019).

  o = xl_attention(q, k, v, r, u, w, klen=None, causal=False, scale=None,
                   impl='auto')

q [B,T,N,H]; k, v [B,S,N,H] with S = M + T keys, the first M of them the
segment memory; r [2S-1,N,H] relative embeddings indexed by distance + (S-1);
u, w [N,H] the content and position biases; klen [B] integer or None.

  logit[i,j] = scale * ((q_i + u_n).k_j + (q_i + w_n).r[(M+i) - j + (S-1)])
  visible(i,j) = j < klen[b] and (not causal or j <= M + i)
  o_i = softmax_j(logit[i,.]) . v

scale defaults to 1/sqrt(H). A row with no visible key returns 0 and has
zero gradient. Gradients flow to q, k, v, r, u and w.

CUDA bf16 tensors with H == 64 run the HIP kernels of ops/hip/xl_attn.hip,
which never hold a [T,S] or [T,2S-1] tensor in memory; their scratch is two
fp32 [B,T,N,H] accumulators and one fp32 [2S-1,N,H]. Other H, other dtypes
and CPU tensors are refused by impl='auto' on CUDA and run the composed
torch twin `_ref_xl_attention` on CPU (fp32, or fp64 for fp64 inputs).
impl='torch' runs the twin on either device: the yardstick for tests and
timing.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from lingvo_amd.ops import _loader

# Head dim the kernels are written for.
KERNEL_HEAD_DIM = 64


def _ref_xl_attention(q, k, v, r, u, w, klen=None, causal=False, scale=None):
  """Composed twin of the math in the module docstring; fp32, or fp64 for
  fp64 inputs. Fully masked rows return 0."""
  b, t, n, h = q.shape
  s = k.shape[1]
  m = s - t
  scale = 1.0 / math.sqrt(h) if scale is None else scale
  ft = torch.float64 if q.dtype == torch.float64 else torch.float32
  qf, kf, vf, rf = q.to(ft), k.to(ft), v.to(ft), r.to(ft)
  ac = torch.einsum('btnh,bsnh->bnts', qf + u.to(ft), kf)
  bd_all = torch.einsum('btnh,lnh->bntl', qf + w.to(ft), rf)  # [B,N,T,2S-1]
  qpos = torch.arange(t, device=q.device)[:, None] + m
  kpos = torch.arange(s, device=q.device)[None, :]
  idx = (qpos - kpos + (s - 1))[None, None].expand(b, n, t, s)
  logits = (ac + bd_all.gather(3, idx)) * scale
  mask = (kpos <= qpos) if causal else torch.ones(
      t, s, dtype=torch.bool, device=q.device)
  mask = mask[None, None]
  if klen is not None:
    mask = mask & (kpos[None, None] < klen[:, None, None, None])
  logits = logits.masked_fill(~mask, -1e30)
  probs = torch.softmax(logits, dim=-1)
  probs = torch.where(mask.any(-1, keepdim=True), probs,
                      torch.zeros_like(probs))
  return torch.einsum('bnts,bsnh->btnh', probs, vf)


class _XlAttnFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, q, k, v, r, u, w, klen, causal, scale):
    ext = _loader.get_ext(required=True)
    o, lse = ext.xl_attn_fwd(q, k, v, r, u, w, klen, causal, scale)
    ctx.save_for_backward(q, k, v, r, u, w, o, lse,
                          klen if klen is not None else torch.empty(0))
    ctx.cfg = (causal, scale)
    return o

  @staticmethod
  def backward(ctx, dout):
    ext = _loader.get_ext(required=True)
    q, k, v, r, u, w, o, lse, klen = ctx.saved_tensors
    causal, scale = ctx.cfg
    dq, dk, dv, dr, du, dw = ext.xl_attn_bwd(
        dout.contiguous(), q, k, v, r, u, w, o, lse,
        klen if klen.numel() else None, causal, scale)
    return (dq, dk, dv, dr, du.to(u.dtype), dw.to(w.dtype), None, None, None)


def _CheckArgs(q, k, v, r, u, w, klen, fn='xl_attention'):
  if q.dim() != 4 or k.dim() != 4:
    raise ValueError(f'{fn}: q must be [B,T,N,H] and k [B,S,N,H], got '
                     f'{tuple(q.shape)} and {tuple(k.shape)}')
  b, t, n, h = q.shape
  s = k.shape[1]
  if b < 1 or t < 1:
    raise ValueError(f'{fn}: B >= 1 and T >= 1')
  if tuple(k.shape) != (b, s, n, h) or v.shape != k.shape:
    raise ValueError(f'{fn}: k and v must be [B,S,N,H] with the heads of q '
                     f'(N == NKV), got {tuple(k.shape)} and {tuple(v.shape)}')
  if s < t:
    raise ValueError(f'{fn}: S={s} keys for T={t} queries; S >= T '
                     '(S = M + T)')
  if tuple(r.shape) != (2 * s - 1, n, h):
    raise ValueError(f'{fn}: r must be [2S-1,N,H] = {(2 * s - 1, n, h)}, '
                     f'got {tuple(r.shape)}')
  if tuple(u.shape) != (n, h) or tuple(w.shape) != (n, h):
    raise ValueError(f'{fn}: u and w must be [N,H], got {tuple(u.shape)} '
                     f'and {tuple(w.shape)}')
  for name, x in (('q', q), ('k', k), ('v', v), ('r', r), ('u', u),
                  ('w', w)):
    if not x.is_floating_point():
      raise TypeError(f'{fn}: {name} must be floating point, got {x.dtype}')
  for name, x in (('k', k), ('v', v), ('r', r)):
    if x.dtype != q.dtype:
      raise TypeError(f'{fn}: {name} is {x.dtype} but q is {q.dtype}')
  if klen is not None:
    if klen.dim() != 1 or klen.shape[0] != b or klen.is_floating_point() or \
        klen.dtype == torch.bool:
      raise TypeError(f'{fn}: klen must be an integer tensor [B]')
  for x in (k, v, r, u, w) + (() if klen is None else (klen,)):
    if x.device != q.device:
      raise ValueError(f'{fn}: all inputs must be on one device')


def xl_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                 r: torch.Tensor, u: torch.Tensor, w: torch.Tensor,
                 klen: Optional[torch.Tensor] = None, causal: bool = False,
                 scale: Optional[float] = None,
                 impl: str = 'auto') -> torch.Tensor:
  """-> o [B,T,N,H]; see the module docstring."""
  if impl not in ('auto', 'torch'):
    raise ValueError(
        f"xl_attention: impl must be 'auto' or 'torch', got {impl!r}")
  _CheckArgs(q, k, v, r, u, w, klen)
  h = q.shape[3]
  scale = 1.0 / math.sqrt(h) if scale is None else float(scale)
  causal = bool(causal)
  if impl == 'torch' or not q.is_cuda:
    return _ref_xl_attention(q, k, v, r, u, w, klen, causal,
                             scale).to(q.dtype)
  if q.dtype != torch.bfloat16:
    raise TypeError(f'xl_attention: the HIP kernels take bf16, got {q.dtype}')
  if h != KERNEL_HEAD_DIM:
    raise ValueError(f'xl_attention: the HIP kernels support H == '
                     f'{KERNEL_HEAD_DIM} only, got H={h}')
  if klen is not None:
    klen = klen.to(torch.int32).contiguous()
  return _XlAttnFn.apply(q.contiguous(), k.contiguous(), v.contiguous(),
                         r.contiguous(), u.to(q.dtype).contiguous(),
                         w.to(q.dtype).contiguous(), klen, causal, scale)
