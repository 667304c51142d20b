"""Performer / FAVOR+ linear attention (Choromanski et al. 2021).

  o = favor_attention(q, k, v, proj, klen=None, causal=False, impl='auto')

q, k, v [B,T,N,H] (self-attention: one length, N == NKV); proj [m,H] the
random projection; klen [B] integer or None. With xs = x * H^(-1/4):

  z(x)  = xs . proj^T - |xs|^2 / 2                              [.., m]
  phi_q = exp(z(q) - max_m z(q)) / sqrt(m) + 1e-6
  phi_k = exp(z(k) - max_{t,m} z(k)) / sqrt(m) + 1e-6, one stabiliser per
          (b, n) over all T positions; then 0 at positions >= klen[b]
  num_t = sum_{s in vis(t)} (phi_q[t] . phi_k[s]) v_s
  den_t = max(sum_{s in vis(t)} phi_q[t] . phi_k[s], 1e-6)
  o_t   = num_t / den_t,   vis(t) = all s, or s <= t when causal

The stabilisers carry no gradient and the clamp passes none where it is
active. A batch row with klen = 0 returns 0 and has zero gradients.
Gradients flow to q, k and v, not to proj.

CUDA bf16 tensors with H == 64, m % 32 == 0 and m <= 128 run the HIP kernels
of ops/hip/favor_attn.hip: a chunked scan with the feature map fused in,
which holds no [B,T,N,m] and no [B,T,N,m,H] tensor; its only scratch is the
fp32 denominator [B,N,T] and the key stabiliser [B,N]. Other CUDA inputs are
refused by impl='auto'; CPU tensors run the composed torch twin
`_ref_favor_attention` (fp32, or fp64 for fp64 inputs). impl='torch' runs
the twin on either device: the yardstick for tests and timing.
"""

from __future__ import annotations

import math
from typing import Optional

import torch

from lingvo_amd.ops import _loader

# What the kernels are written for.
KERNEL_HEAD_DIM = 64
KERNEL_FEATURE_MULTIPLE = 32
KERNEL_MAX_FEATURES = 128


def kernel_supports(h: int, m: int) -> bool:
  return (h == KERNEL_HEAD_DIM and m % KERNEL_FEATURE_MULTIPLE == 0 and
          0 < m <= KERNEL_MAX_FEATURES)


def _RoundTo(x, dtype):
  """x rounded to dtype, kept in its own; straight-through for autograd."""
  return x + (x.detach().to(dtype).to(x.dtype) - x.detach())


def _ref_favor_attention(q, k, v, proj, klen=None, causal=False,
                         operand_dtype=None, return_den=False):
  """Composed twin of the math in the module docstring; fp32, or fp64 for
  fp64 inputs. With operand_dtype, phi_q, phi_k and v are rounded to it
  before the contractions, whose sums stay wide. return_den adds the
  clamped denominator [B,T,N] to the result."""
  b, t, n, h = q.shape
  m = proj.shape[0]
  ft = torch.float64 if q.dtype == torch.float64 else torch.float32
  pf = proj.detach().to(ft)
  scale = 1.0 / math.sqrt(h)

  def phi(x, is_key):
    xs = x.to(ft) * math.sqrt(scale)
    wx = torch.einsum('btnh,mh->btnm', xs, pf)
    z = wx - 0.5 * (xs * xs).sum(-1, keepdim=True)
    if is_key:
      stab = z.amax(dim=(1, 3), keepdim=True).detach()
    else:
      stab = z.amax(dim=-1, keepdim=True).detach()
    return torch.exp(z - stab) / math.sqrt(m) + 1e-6

  qp = phi(q, False)
  kp = phi(k, True)
  if klen is not None:
    live = torch.arange(t, device=q.device)[None, :] < klen[:, None]
    kp = kp * live.to(ft)[:, :, None, None]
  vf = v.to(ft)
  if operand_dtype is not None:
    qp, kp, vf = (_RoundTo(x, operand_dtype) for x in (qp, kp, vf))
  if causal:
    kv = torch.einsum('btnm,btnh->btnmh', kp, vf).cumsum(1)
    z = kp.cumsum(1)
    num = torch.einsum('btnm,btnmh->btnh', qp, kv)
    den = torch.einsum('btnm,btnm->btn', qp, z).clamp_min(1e-6)
  else:
    kv = torch.einsum('btnm,btnh->bnmh', kp, vf)
    z = kp.sum(1)
    num = torch.einsum('btnm,bnmh->btnh', qp, kv)
    den = torch.einsum('btnm,bnm->btn', qp, z).clamp_min(1e-6)
  o = num / den.unsqueeze(-1)
  return (o, den) if return_den else o


class _FavorAttnFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, q, k, v, proj, klen, causal):
    ext = _loader.get_ext(required=True)
    o, den, kstab = ext.favor_attn_fwd(q, k, v, proj, klen, causal)
    ctx.save_for_backward(q, k, v, proj, o, den, kstab,
                          klen if klen is not None else torch.empty(0))
    ctx.causal = causal
    return o

  @staticmethod
  def backward(ctx, dout):
    ext = _loader.get_ext(required=True)
    q, k, v, proj, o, den, kstab, klen = ctx.saved_tensors
    dq, dk, dv = ext.favor_attn_bwd(
        dout.contiguous(), q, k, v, proj, o, den, kstab,
        klen if klen.numel() else None, ctx.causal)
    return dq, dk, dv, None, None, None


def _CheckArgs(q, k, v, proj, klen, fn='favor_attention'):
  if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
    raise ValueError(f'{fn}: q, k and v must be [B,T,N,H], got '
                     f'{tuple(q.shape)}, {tuple(k.shape)} and '
                     f'{tuple(v.shape)}')
  b, t, n, h = q.shape
  if b < 1 or t < 1:
    raise ValueError(f'{fn}: B >= 1 and T >= 1')
  if k.shape != q.shape or v.shape != q.shape:
    raise ValueError(f'{fn}: self-attention only: k and v must have the '
                     f'shape of q (S == T, N == NKV), got {tuple(k.shape)} '
                     f'and {tuple(v.shape)} for {tuple(q.shape)}')
  if proj.dim() != 2 or proj.shape[0] < 1 or proj.shape[1] != h:
    raise ValueError(f'{fn}: proj must be [m,H] with H={h}, got '
                     f'{tuple(proj.shape)}')
  for name, x in (('q', q), ('k', k), ('v', v), ('proj', proj)):
    if not x.is_floating_point():
      raise TypeError(f'{fn}: {name} must be floating point, got {x.dtype}')
  for name, x in (('k', k), ('v', v)):
    if x.dtype != q.dtype:
      raise TypeError(f'{fn}: {name} is {x.dtype} but q is {q.dtype}')
  if klen is not None:
    if klen.dim() != 1 or klen.shape[0] != b or klen.is_floating_point() or \
        klen.dtype == torch.bool:
      raise TypeError(f'{fn}: klen must be an integer tensor [B]')
  for x in (k, v, proj) + (() if klen is None else (klen,)):
    if x.device != q.device:
      raise ValueError(f'{fn}: all inputs must be on one device')


def favor_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    proj: torch.Tensor, klen: Optional[torch.Tensor] = None,
                    causal: bool = False, impl: str = 'auto') -> torch.Tensor:
  """-> o [B,T,N,H]; see the module docstring."""
  if impl not in ('auto', 'torch'):
    raise ValueError(
        f"favor_attention: impl must be 'auto' or 'torch', got {impl!r}")
  _CheckArgs(q, k, v, proj, klen)
  causal = bool(causal)
  if impl == 'torch' or not q.is_cuda:
    return _ref_favor_attention(q, k, v, proj, klen, causal).to(q.dtype)
  if q.dtype != torch.bfloat16:
    raise TypeError(
        f'favor_attention: the HIP kernels take bf16, got {q.dtype}')
  h, m = q.shape[3], proj.shape[0]
  if not kernel_supports(h, m):
    raise ValueError(
        f'favor_attention: the HIP kernels support H == {KERNEL_HEAD_DIM} '
        f'with m % {KERNEL_FEATURE_MULTIPLE} == 0 and m <= '
        f'{KERNEL_MAX_FEATURES}, got H={h}, m={m}')
  if klen is not None:
    klen = klen.to(torch.int32).contiguous()
  return _FavorAttnFn.apply(q.contiguous(), k.contiguous(), v.contiguous(),
                            proj.detach().float().contiguous(), klen, causal)
