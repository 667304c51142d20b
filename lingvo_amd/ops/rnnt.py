"""Transducer (RNN-T) loss over joint logits.

  nll, valid = rnnt_loss(logits, logit_lengths, labels, label_lengths,
                         blank_id=0, impl='auto')

logits [B,T,U+1,V], labels [B,U] int64, lengths [B]. nll [B] is the
negative log-likelihood of each utterance summed over all alignments and
valid [B] (1 or 0, no gradient) says whether it has one. With T_b, U_b the
row's lengths, blank(t,u) = log p(blank | t,u) and
label(t,u) = log p(labels[u] | t,u):

  alpha(0,0) = 0
  alpha(t,u) = lse2(alpha(t-1,u) + blank(t-1,u), alpha(t,u-1) + label(t,u-1))
  nll        = -(alpha(T_b-1,U_b) + blank(T_b-1,U_b))

A row is invalid - valid = 0, nll = 0, zero gradient - when T_b is outside
[1,T] or U_b outside [0,U], when a label inside U_b is the blank or outside
[0,V), or when its likelihood is not finite. An empty target (U_b = 0) is
valid: the all-blank path. The gradient is exactly zero for t >= T_b and
for u > U_b.

CUDA tensors run the HIP kernels of ops/hip/rnnt.hip (bf16 or fp32 logits,
no fp32 [B,T,U+1,V] intermediate, deterministic backward). CPU tensors run
a torch twin of the same recursion, batched over B, one anti-diagonal per
step, with an analytic backward, in the dtype of the input (fp32 or fp64).
Both keep the small [B,T,U+1] tables (emissions, alpha, beta) in float64:
the gradient is built from exp(alpha + beta - ll), a difference of numbers
of the size of the likelihood, and in float32 its error (an ulp of |ll|,
1e-4 at |ll| = 1000) is tens to thousands of times that of autograd
through the float32 recursion. Everything of the size of the logits stays
in the input's dtype and float32. impl='torch' on either device is log_softmax in fp32 (fp64 for fp64
inputs) followed by the same per-diagonal recursion in torch ops,
differentiated by autograd: the route the kernels are timed against. It
materialises the fp32 [B,T,U+1,V] log-probabilities.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from lingvo_amd.ops import _loader

# Label width the kernels support: one lane per u, U+1 <= 1024 lanes of a
# workgroup.
MAX_LABEL_LEN = 1023

_NEG = -1e30
_NEG_TEST = -1e29


def _Validity(logit_lengths, labels, label_lengths, t, v, blank_id):
  """(valid [B] bool, T_b, U_b, labels safe to index with), in plain torch
  ops without a sync."""
  u = labels.shape[1]
  len_ok = ((logit_lengths >= 1) & (logit_lengths <= t) &
            (label_lengths >= 0) & (label_lengths <= u))
  tb = torch.where(len_ok, logit_lengths, torch.zeros_like(logit_lengths))
  ub = torch.where(len_ok, label_lengths, torch.zeros_like(label_lengths))
  pos = torch.arange(u, device=labels.device)[None, :]
  inside = pos < ub[:, None]
  bad = inside & ((labels < 0) | (labels >= v) | (labels == blank_id))
  valid = len_ok & ~bad.any(-1)
  safe = torch.where(inside & ~bad, labels, torch.zeros_like(labels))
  return valid, tb, ub, safe


def _Lse2(a, b):
  m = torch.maximum(a, b)
  out = m + torch.log(torch.exp(a - m) + torch.exp(b - m))
  return torch.where(m > _NEG_TEST, out, torch.full_like(out, _NEG))


def _Emissions(lp, safe, blank_id):
  """blank [B,T,U1] and label [B,T,U1] (zero in the last column) log-probs
  out of log-probabilities lp [B,T,U1,V]."""
  b, t, u1, _ = lp.shape
  blank_e = lp[..., blank_id]
  label_e = lp[:, :, :u1 - 1].gather(
      3, safe[:, None, :, None].expand(b, t, u1 - 1, 1))[..., 0]
  return blank_e, torch.cat([label_e, torch.zeros_like(blank_e[:, :, :1])],
                            dim=2)


class _Skew:
  """Diagonal-major view of a [B,T,U1] lattice: entry [b,d,u] is cell
  (t,u) = (d-u, u); `on` marks the entries whose cell is inside row b."""

  def __init__(self, t, u1, tb, ub, device):
    self.t, self.u1, self.d = t, u1, t + u1 - 1
    uu = torch.arange(u1, device=device)[None, :]
    dd = torch.arange(self.d, device=device)[:, None]
    tt = dd - uu                                            # [D,U1]
    self.t_idx = tt.clamp(0, t - 1)
    self.u_idx = uu.expand(self.d, u1)
    self.on = ((tt >= 0)[None] & (tt[None] < tb[:, None, None]) &
               (uu[None] <= ub[:, None, None]))             # [B,D,U1]
    self.final = ((tt[None] == tb[:, None, None] - 1) &
                  (uu[None] == ub[:, None, None]) & self.on)
    # The cell (t,u) of the [T,U1] layout sits at diagonal t+u.
    self.d_idx = (torch.arange(t, device=device)[:, None] + uu)  # [T,U1]

  def To(self, x):     # [B,T,U1] -> [B,D,U1]
    return x[:, self.t_idx, self.u_idx]

  def From(self, x):   # [B,D,U1] -> [B,T,U1]
    return x[:, self.d_idx, self.u_idx[:self.t]]


def _ShiftRight(x):
  """x[:, u-1] at position u, 'impossible' at u = 0."""
  return torch.cat([torch.full_like(x[:, :1], _NEG), x[:, :-1]], dim=1)


def _ShiftLeft(x):
  return torch.cat([x[:, 1:], torch.full_like(x[:, :1], _NEG)], dim=1)


def _Alpha(sk, blank_s, label_s):
  """Alpha over the skewed emissions, one anti-diagonal per step ->
  [B,D,U1] with 'impossible' outside each row's lattice."""
  neg = torch.full_like(blank_s[:, 0], _NEG)
  start = torch.zeros_like(neg)
  diags = [torch.where(sk.on[:, 0], start, neg)]
  for d in range(1, sk.d):
    prev = diags[-1]
    new = _Lse2(prev + blank_s[:, d - 1],
                _ShiftRight(prev + label_s[:, d - 1]))
    diags.append(torch.where(sk.on[:, d], new, neg))
  return torch.stack(diags, dim=1)


def _Beta(sk, blank_s, label_s):
  neg = torch.full_like(blank_s[:, 0], _NEG)
  diags = [None] * sk.d
  nxt = neg
  for d in range(sk.d - 1, -1, -1):
    new = _Lse2(nxt + blank_s[:, d], _ShiftLeft(nxt) + label_s[:, d])
    new = torch.where(sk.final[:, d], blank_s[:, d], new)
    nxt = torch.where(sk.on[:, d], new, neg)
    diags[d] = nxt
  return torch.stack(diags, dim=1)


def _LogLikelihood(sk, alpha_s, blank_s, tb, ub):
  """alpha(T_b-1,U_b) + blank(T_b-1,U_b) per row, and whether it is a
  likelihood."""
  b = alpha_s.shape[0]
  d_end = (tb - 1 + ub).clamp(min=0)
  rows = torch.arange(b, device=alpha_s.device)
  ll = alpha_s[rows, d_end, ub] + blank_s[rows, d_end, ub]
  return ll, (ll > _NEG_TEST) & torch.isfinite(ll)


def _TwinForward(logits, logit_lengths, labels, label_lengths, blank_id):
  """The kernels' arithmetic in torch ops, batched over B: row max and
  log-sum in logits.dtype, emissions and lattice in float64, nll back in
  logits.dtype. Returns nll, valid and what the backward needs."""
  b, t, u1, v = logits.shape
  valid, tb, ub, safe = _Validity(logit_lengths, labels, label_lengths, t, v,
                                  blank_id)
  tb = torch.where(valid, tb, torch.zeros_like(tb))
  ub = torch.where(valid, ub, torch.zeros_like(ub))
  row_max = logits.amax(-1)
  row_sum = torch.exp(logits - row_max[..., None]).sum(-1)
  # log p = (x - max) - log(sum): both parts small where p is not.
  lp = (logits - row_max[..., None]) - torch.log(row_sum)[..., None]
  x_blank, x_label = _Emissions(logits, safe, blank_id)
  norm = torch.log(row_sum.double())
  blank_e = (x_blank.double() - row_max.double()) - norm
  label_e = (x_label.double() - row_max.double()) - norm
  sk = _Skew(t, u1, tb, ub, logits.device)
  blank_s, label_s = sk.To(blank_e), sk.To(label_e)
  alpha_s = _Alpha(sk, blank_s, label_s)
  beta_s = _Beta(sk, blank_s, label_s)
  ll, ok = _LogLikelihood(sk, alpha_s, blank_s, tb, ub)
  valid = valid & ok
  nll = torch.where(valid, -ll, torch.zeros_like(ll)).to(logits.dtype)
  alpha, beta = sk.From(alpha_s), sk.From(beta_s)
  return nll, valid.to(logits.dtype), (lp, safe, blank_e, label_e, alpha,
                                       beta, tb, ub)


def _TwinBackward(gout, valid, saved, blank_id):
  """g * (softmax * occ - blank and label transitions): the occupancy
  terms in float64 out of alpha and beta (ll = beta(0,0)), the rest in the
  dtype of lp."""
  lp, safe, blank_e, label_e, alpha, beta, tb, ub = saved
  b, t, u1, _ = lp.shape
  dev = lp.device
  tt = torch.arange(t, device=dev)[None, :, None]
  uu = torch.arange(u1, device=dev)[None, None, :]
  tb3, ub3 = tb[:, None, None], ub[:, None, None]
  live = (valid > 0)[:, None, None] & (tt < tb3) & (uu <= ub3)  # [B,T,U1]
  ll3 = beta[:, :1, :1]
  zero = torch.zeros_like(alpha)
  neg_t = torch.full_like(alpha[:, :1], _NEG)
  neg_u = torch.full_like(alpha[:, :, :1], _NEG)
  beta_t1 = torch.cat([beta[:, 1:], neg_t], dim=1)        # beta(t+1,u)
  beta_u1 = torch.cat([beta[:, :, 1:], neg_u], dim=2)     # beta(t,u+1)
  last = (tt == tb3 - 1) & (uu == ub3)
  beta_t1 = torch.where(last, zero, beta_t1)
  g3 = gout.double()[:, None, None]
  occ = torch.where(live, g3 * torch.exp(alpha + beta - ll3), zero)
  cb = torch.where(live, g3 * torch.exp(alpha + blank_e + beta_t1 - ll3),
                   zero)
  cl = torch.where(live & (uu < ub3),
                   g3 * torch.exp(alpha + label_e + beta_u1 - ll3), zero)
  occ, cb, cl = occ.to(lp.dtype), cb.to(lp.dtype), cl.to(lp.dtype)
  grad = torch.exp(lp) * occ[..., None]
  grad[..., blank_id] -= cb
  if u1 > 1:
    grad[:, :, :u1 - 1].scatter_add_(
        3, safe[:, None, :, None].expand(b, t, u1 - 1, 1),
        -cl[:, :, :u1 - 1, None])
  keep = live & (g3 != 0)
  return torch.where(keep[..., None], grad, torch.zeros_like(grad))


class _RnntLossFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, logits, logit_lengths, labels, label_lengths, blank_id):
    ctx.blank_id = blank_id
    ctx.is_hip = logits.is_cuda
    if logits.is_cuda:
      ext = _loader.get_ext(required=True)
      nll, valid, lse, emis, alpha, beta = ext.rnnt_fwd(
          logits, logit_lengths, labels, label_lengths, blank_id)
      ctx.save_for_backward(logits, logit_lengths, labels, label_lengths,
                            lse, emis, alpha, beta, valid)
    else:
      ctx.in_dtype = logits.dtype
      x = logits if logits.dtype == torch.float64 else logits.float()
      nll, valid, saved = _TwinForward(x, logit_lengths, labels,
                                       label_lengths, blank_id)
      ctx.save_for_backward(nll, valid, *saved)
    ctx.mark_non_differentiable(valid)
    return nll, valid

  @staticmethod
  def backward(ctx, gnll, _gvalid):
    if ctx.is_hip:
      ext = _loader.get_ext(required=True)
      (logits, logit_lengths, labels, label_lengths, lse, emis, alpha, beta,
       valid) = ctx.saved_tensors
      dlogits = ext.rnnt_bwd(logits, logit_lengths, labels, label_lengths,
                             lse, emis, alpha, beta, valid,
                             gnll.float().contiguous(), ctx.blank_id)
    else:
      nll, valid, *saved = ctx.saved_tensors
      del nll
      dlogits = _TwinBackward(gnll, valid, saved,
                              ctx.blank_id).to(ctx.in_dtype)
    return dlogits, None, None, None, None


def _TorchRnnt(logits, logit_lengths, labels, label_lengths, blank_id):
  """log_softmax in fp32 (fp64 for fp64 inputs), then the per-diagonal
  alpha recursion in torch ops under autograd."""
  b, t, u1, v = logits.shape
  valid, tb, ub, safe = _Validity(logit_lengths, labels, label_lengths, t, v,
                                  blank_id)
  tb = torch.where(valid, tb, torch.zeros_like(tb))
  ub = torch.where(valid, ub, torch.zeros_like(ub))
  x = logits if logits.dtype == torch.float64 else logits.float()
  lp = F.log_softmax(x, dim=-1)
  blank_e, label_e = _Emissions(lp, safe, blank_id)
  sk = _Skew(t, u1, tb, ub, logits.device)
  blank_s, label_s = sk.To(blank_e), sk.To(label_e)
  alpha_s = _Alpha(sk, blank_s, label_s)
  ll, ok = _LogLikelihood(sk, alpha_s, blank_s, tb, ub)
  valid = valid & ok
  nll = torch.where(valid, -ll, torch.zeros_like(ll))
  return nll, valid.to(nll.dtype)


def _CheckArgs(logits, logit_lengths, labels, label_lengths, blank_id):
  if logits.dim() != 4:
    raise ValueError(f'rnnt_loss: logits must be [B,T,U+1,V], got '
                     f'{tuple(logits.shape)}')
  if not logits.is_floating_point():
    raise TypeError(f'rnnt_loss: logits must be floating point, got '
                    f'{logits.dtype}')
  if not logits.is_contiguous():
    raise ValueError('rnnt_loss: logits must be contiguous')
  b, t, u1, v = logits.shape
  if b < 1 or t < 1 or u1 < 1:
    raise ValueError('rnnt_loss: B >= 1, T >= 1 and U+1 >= 1')
  if v < 2:
    raise ValueError('rnnt_loss: V >= 2')
  if not 0 <= blank_id < v:
    raise ValueError(f'rnnt_loss: blank_id {blank_id} outside [0, {v})')
  if labels.dtype != torch.int64 or labels.dim() != 2 or \
      labels.shape[0] != b:
    raise TypeError('rnnt_loss: labels must be int64 [B,U]')
  if labels.shape[1] + 1 != u1:
    raise ValueError(f'rnnt_loss: labels [B,U={labels.shape[1]}] need '
                     f'logits.shape[2] == U+1, got {u1}')
  if labels.shape[1] > MAX_LABEL_LEN:
    raise ValueError(f'rnnt_loss: U={labels.shape[1]} is over the supported '
                     f'limit {MAX_LABEL_LEN}')
  if b * t * u1 >= 2**31:
    raise ValueError(f'rnnt_loss: B*T*(U+1) = {b * t * u1} is over the '
                     f'supported limit 2^31 - 1')
  for name, x in (('logit_lengths', logit_lengths),
                  ('label_lengths', label_lengths)):
    if x.dim() != 1 or x.shape[0] != b or x.is_floating_point() or \
        x.dtype == torch.bool:
      raise TypeError(f'rnnt_loss: {name} must be an integer tensor [B]')
  for x in (logit_lengths, labels, label_lengths):
    if x.device != logits.device:
      raise ValueError('rnnt_loss: all inputs must be on one device')


def rnnt_loss(logits: torch.Tensor, logit_lengths: torch.Tensor,
              labels: torch.Tensor, label_lengths: torch.Tensor,
              blank_id: int = 0, impl: str = 'auto'):
  """-> (nll [B], valid [B]); see the module docstring."""
  if impl not in ('auto', 'torch'):
    raise ValueError(
        f"rnnt_loss: impl must be 'auto' or 'torch', got {impl!r}")
  blank_id = int(blank_id)
  _CheckArgs(logits, logit_lengths, labels, label_lengths, blank_id)
  logit_lengths = logit_lengths.long().contiguous()
  label_lengths = label_lengths.long().contiguous()
  labels = labels.contiguous()
  if impl == 'torch':
    return _TorchRnnt(logits, logit_lengths, labels, label_lengths, blank_id)
  if logits.is_cuda and logits.dtype not in (torch.bfloat16, torch.float32):
    raise TypeError(f'rnnt_loss: the HIP kernels take bf16 or fp32 logits, '
                    f'got {logits.dtype}')
  return _RnntLossFn.apply(logits, logit_lengths, labels, label_lengths,
                           blank_id)
