"""Depthwise time-convolution autograd wrappers (K7).

depthwise_conv1d is the plain op. glu_depthwise_conv1d and
linear_glu_dwconv are the fused front of the Conformer LConv module:
GLU, the padding mask and the convolution run in one kernel each way, so
the GLU output never reaches memory and the pw1 bias gradient comes out of
the backward kernel's column sums.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from lingvo_amd.ops import _loader

def tile_len() -> int:
  """Time rows per tile of the tiled kernels (tests place T around it)."""
  return int(_loader.get_ext(required=True).dwconv_tile_len())


class _DwConv1dFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, x, w, bias, pad, route):
    ext = _loader.get_ext(required=True)
    y = ext.dwconv1d_fwd(x, w, bias, pad, route)
    ctx.save_for_backward(x, w)
    ctx.pad = pad
    ctx.route = route
    ctx.has_bias = bias is not None
    ctx.wdtype = w.dtype
    return y

  @staticmethod
  def backward(ctx, dy):
    ext = _loader.get_ext(required=True)
    x, w = ctx.saved_tensors
    dx, dw, db = ext.dwconv1d_bwd(dy.contiguous(), x, w, ctx.pad, ctx.route)
    return (dx, dw.to(ctx.wdtype),
            db.to(ctx.wdtype) if ctx.has_bias else None, None, None)


def _pad_of(k: int, causal: bool) -> int:
  return k - 1 if causal else (k - 1) // 2


def depthwise_conv1d(x: torch.Tensor, w: torch.Tensor,
                     bias: Optional[torch.Tensor] = None,
                     causal: bool = False,
                     route: str = 'auto') -> torch.Tensor:
  """x [B,T,D], w [K,D] -> [B,T,D]; zero padding outside the sequence.
  route picks the GPU kernels: 'tiled' (LDS-tiled), 'naive' (per-thread tap
  loop, the yardstick) or 'auto' (tiled wherever it is supported)."""
  k = w.shape[0]
  pad = _pad_of(k, causal)
  if x.is_cuda:
    orig = x.dtype
    out = _DwConv1dFn.apply(
        x.to(torch.bfloat16).contiguous(), w.to(torch.bfloat16).contiguous(),
        None if bias is None else bias.to(torch.bfloat16).contiguous(), pad,
        route)
    return out.to(orig) if orig != torch.bfloat16 else out
  # CPU reference via grouped conv1d.
  xf = x.float().permute(0, 2, 1)  # [B,D,T]
  wf = w.float().t().unsqueeze(1)  # [D,1,K]
  left = pad
  right = (k - 1) - pad
  xf = F.pad(xf, (left, right))
  out = F.conv1d(xf, wf, bias.float() if bias is not None else None,
                 groups=x.shape[2])
  return out.permute(0, 2, 1).to(x.dtype)


def _bf16_pad(paddings: Optional[torch.Tensor],
              like: torch.Tensor) -> Optional[torch.Tensor]:
  """[B,T] (or [B,T,1]) paddings -> contiguous bf16 [B,T]."""
  if paddings is None:
    return None
  if paddings.dim() == 3 and paddings.shape[-1] == 1:
    paddings = paddings.squeeze(-1)
  if paddings.shape != like.shape[:2]:
    raise ValueError(f'paddings must be [B,T]={tuple(like.shape[:2])}, got '
                     f'{tuple(paddings.shape)}')
  return paddings.to(torch.bfloat16).contiguous()


class _GluDwConv1dFn(torch.autograd.Function):
  """conv(mask * glu(h), w) + bias; saves h, never materialises glu(h)."""

  @staticmethod
  def forward(ctx, h, pad_mask, w, bias, pad):
    ext = _loader.get_ext(required=True)
    y = ext.glu_dwconv1d_fwd(h, pad_mask, w, bias, pad)
    ctx.save_for_backward(h, w, *([] if pad_mask is None else [pad_mask]))
    ctx.pad = pad
    ctx.has_bias = bias is not None
    return y

  @staticmethod
  def backward(ctx, dy):
    ext = _loader.get_ext(required=True)
    h, w, *rest = ctx.saved_tensors
    dh, dw, db, _ = ext.glu_dwconv1d_bwd(dy.contiguous(), h,
                                         rest[0] if rest else None, w, ctx.pad)
    return (dh, None, dw.to(w.dtype),
            db.to(w.dtype) if ctx.has_bias else None, None)


def glu_depthwise_conv1d(h: torch.Tensor, paddings: Optional[torch.Tensor],
                         w: torch.Tensor,
                         bias: Optional[torch.Tensor] = None,
                         causal: bool = False) -> torch.Tensor:
  """depthwise_conv1d(ApplyPadding(paddings, F.glu(h)), w, bias, causal) for
  GPU bf16 h [B,T,2D] (contiguous), paddings [B,T] or None, w [K,D]."""
  return _GluDwConv1dFn.apply(h, _bf16_pad(paddings, h), w, bias,
                              _pad_of(w.shape[0], causal))


class _LinearGluDwConvFn(torch.autograd.Function):
  """addmm + the fused kernel forward; backward runs the fused kernels, the
  two GEMMs autograd would issue, and takes d pw1_b from the column sums."""

  @staticmethod
  def forward(ctx, x2, pw1_w, pw1_b, pad_mask, dw_w, dw_b, pad, bt):
    ext = _loader.get_ext(required=True)
    h = torch.addmm(pw1_b, x2, pw1_w).view(bt[0], bt[1], -1)
    y = ext.glu_dwconv1d_fwd(h, pad_mask, dw_w, dw_b, pad)
    ctx.save_for_backward(x2, pw1_w, h, dw_w,
                          *([] if pad_mask is None else [pad_mask]))
    ctx.pad = pad
    ctx.has_bias = dw_b is not None
    return y

  @staticmethod
  def backward(ctx, dy):
    ext = _loader.get_ext(required=True)
    x2, pw1_w, h, dw_w, *rest = ctx.saved_tensors
    dh, ddw, ddb, dcol = ext.glu_dwconv1d_bwd(
        dy.contiguous(), h, rest[0] if rest else None, dw_w, ctx.pad)
    dh2 = dh.view(-1, dh.shape[-1])
    dx = torch.mm(dh2, pw1_w.t()) if ctx.needs_input_grad[0] else None
    dw1 = torch.mm(x2.t(), dh2) if ctx.needs_input_grad[1] else None
    db1 = dcol.to(torch.bfloat16) if ctx.needs_input_grad[2] else None
    return (dx, dw1, db1, None, ddw.to(dw_w.dtype),
            ddb.to(dw_w.dtype) if ctx.has_bias else None, None, None)


def linear_glu_dwconv(x: torch.Tensor, pw1_w: torch.Tensor,
                      pw1_b: torch.Tensor, paddings: Optional[torch.Tensor],
                      dw_w: torch.Tensor, dw_b: Optional[torch.Tensor],
                      causal: bool = False) -> torch.Tensor:
  """glu_depthwise_conv1d(x @ pw1_w + pw1_b, ...) as one autograd node. GPU
  bf16 only; x [B,T,Din], pw1_w [Din,2D], dw_w [K,D], D % 8 == 0."""
  assert x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 3
  x2 = x.reshape(-1, x.shape[-1])
  y = _LinearGluDwConvFn.apply(
      x2, pw1_w, pw1_b, _bf16_pad(paddings, x), dw_w.contiguous(),
      None if dw_b is None else dw_b.contiguous(),
      _pad_of(dw_w.shape[0], causal), (x.shape[0], x.shape[1]))
  return y
