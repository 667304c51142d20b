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

  beam = rnnt_beam_search(enc_p, enc_lengths, joint_w, joint_b, pred_fn,
                          init_states, beam_width=8, token_beam=8,
                          max_symbols=3, blank_id=0, impl='auto')

is time-synchronous transducer beam search with at most S = max_symbols
labels per frame and prefix merging at the end of each frame. enc_p
[B,T,J] is the projected encoder output, joint_w [J,V] and joint_b [V] the
softmax layer of the joint, joint(e, p) = tanh(e + p) @ joint_w + joint_b.
pred_fn(tok [R] long, states) -> (pred_p [R,J], new_states) is one
prediction-network step plus its projection over R = B*W rows; states is
a tuple of tensors with leading dimension R and init_states the one to
start from. The search, with W = beam_width and C = token_beam:

  beam: W slots (label sequence, score, prediction-network state).
        Start: slot 0 = empty sequence, score 0; the others dead (-1e30).
  for t in 0 .. T_b-1:
    A = beam; pool = []
    for s in 0 .. S:                     # s labels emitted so far in this frame
      lp = log_softmax(joint(enc_p[b,t], pred_p[A]))         # per live slot of A
      pool[s*W + i] = (A_i.seq, A_i.score + lp[i, blank])    # every live i
      if s == S: break
      candidates (i, r), r < C: A_i.seq + tok_r(i), A_i.score + lp[i, tok_r(i)]
          tok_r(i) = the non-blank token with the r-th largest raw logit in
          row i (equal logits: the lower id first); C is clamped to V-1
      A = the W best candidates (larger score; then lower i; then lower r)
      advance the prediction network by one step for the new A
    merge pool entries with equal label sequences: logaddexp into the entry
        with the lowest pool index; the others die
    beam = the W best live pool entries (larger score, then lower pool index)
  frames t >= T_b are not visited.

Two entries of one level never spell the same labels (they would share
their ancestor and their token), so duplicates arise only across levels,
in the pool. pred_fn is called once with the blank to start the history
and then once per level for all R rows; dead rows get the blank and their
outputs are ignored. The result is the final beam, descending, as an
RnntBeam:
  topk_ids    [B,W,T*S] int64  left-packed labels, padded with 0
  topk_lens   [B,W]     int64
  topk_scores [B,W]            fp32, or fp64 from fp64 CPU input
  valid       [B]              1 or 0
Unused slots have length 0, ids 0 and score -1e30. T_b == 0 gives the
empty hypothesis with score 0; a length outside [0,T] gives valid = 0 and
no hypothesis. No output carries a gradient.

impl='auto' on CUDA runs the kernels of ops/hip/rnnt_beam.hip: per level a
fused joint + prune launch (the [R,V] logits never reach memory) and an
expand launch, per frame a close launch, at the end a backtrace; the
state gathers and pred_fn stay in torch. No host sync; all T frames run
with static shapes and utterances past their length are frozen by the
kernels. Limits: bf16 enc_p, pred_p and joint_w (joint_b bf16 or fp32),
W <= 32, C <= 16, S <= 4, J % 32 == 0 and J <= 1024, any V >= 2; other
CUDA inputs are refused. CPU tensors and impl='torch' run _TwinRnntBeam,
the definition above over Python lists of label tuples, in the dtype of
the input (fp32 for bf16 input, with tanh(.) rounded to bf16 as the
kernels' MFMA operand is).
"""

from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from lingvo_amd.ops import _loader

# Label width the kernels support: one lane per u, U+1 <= 1024 lanes of a
# workgroup.
MAX_LABEL_LEN = 1023
# Beam search: one lane per candidate (W*C <= 512), (S+1)*W pool entries in
# LDS, and a resident 32 x J bf16 tile of at most 64 KB.
MAX_BEAM_WIDTH = 32
MAX_TOKEN_BEAM = 16
MAX_SYMBOLS = 4
MAX_JOINT_DIM = 1024

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


class RnntBeam(NamedTuple):
  """What rnnt_beam_search returns; see the module docstring."""
  topk_ids: torch.Tensor     # [B,W,T*S] int64
  topk_lens: torch.Tensor    # [B,W] int64
  topk_scores: torch.Tensor  # [B,W]
  valid: torch.Tensor        # [B]


def _Rows(states, index):
  return tuple(x.index_select(0, index) for x in states)


def _Pool(levels, b, w):
  """S+1 tensors [B*W,...] -> [B*(S+1)*W,...], entry b*(S+1)*W + s*W + i."""
  return torch.stack([x.reshape(b, w, *x.shape[1:]) for x in levels],
                     dim=1).flatten(0, 2)


def _TwinRnntBeam(enc_p, enc_lengths, joint_w, joint_b, pred_fn, init_states,
                  w, c, s_max, blank_id, operand_dtype=None, on_select=None):
  """The search of the module docstring, literally: Python lists of (label
  tuple, score) per utterance, scores in enc_p.dtype (fp32 or fp64), the
  prediction network batched over all B*W rows as the kernels' host loop
  runs it. operand_dtype rounds tanh(enc_p + pred_p) to that dtype before
  the product with joint_w, which stays wide: the operands the MFMA sees.
  on_select('select', b, scores, w) sees every selection's candidate
  scores, sorted, before the cut to w; on_select('tokens', row, logits, c)
  every live row's non-blank raw logits, sorted, before the cut to c."""
  b, t, _ = enc_p.shape
  v = joint_w.shape[1]
  c = min(c, v - 1)
  dev, dt = enc_p.device, enc_p.dtype
  npdt = np.float64 if dt == torch.float64 else np.float32
  jw, jb = joint_w.to(dt), joint_b.to(dt)
  tokens = torch.tensor([i for i in range(v) if i != blank_id], device=dev)
  r, p = b * w, (s_max + 1) * w
  lens = enc_lengths.cpu().tolist()
  ok = [0 <= n <= t for n in lens]

  def lse(x, y):
    m = max(x, y)
    return m + np.log(np.exp(x - m) + np.exp(y - m))

  def rows(values):
    return torch.tensor(values, dtype=torch.long, device=dev)

  beams = [[((), npdt(0))] if good else [] for good in ok]
  pred_p, states = pred_fn(rows([blank_id] * r), tuple(init_states))
  for f in range(t):
    active = [ok[i] and f < lens[i] for i in range(b)]
    if not any(active):
      break
    cur = [list(beams[i]) if active[i] else [] for i in range(b)]
    pool = [[] for _ in range(b)]
    lv_pred, lv_states = [], []
    for lvl in range(s_max + 1):
      lv_pred.append(pred_p)
      lv_states.append(states)
      x = torch.tanh(enc_p[:, f].repeat_interleave(w, dim=0) + pred_p.to(dt))
      if operand_dtype is not None:
        x = x.to(operand_dtype).to(dt)
      logits = x @ jw + jb
      lp = (logits - torch.logsumexp(logits, -1, keepdim=True)).cpu().numpy()
      order = torch.sort(logits[:, tokens], dim=-1, descending=True,
                         stable=True)  # ties: the lower id first
      top = tokens[order.indices[:, :c]].cpu().tolist()
      top_vals = order.values.cpu().numpy()
      parent = [i * w for i in range(b) for _ in range(w)]
      tok = [blank_id] * r
      for i in range(b):
        for k, (seq, score) in enumerate(cur[i]):
          pool[i].append((lvl * w + k, seq, score + lp[i * w + k, blank_id]))
        if lvl == s_max or not cur[i]:
          continue
        cands = []
        for k, (seq, score) in enumerate(cur[i]):
          if on_select is not None:
            on_select('tokens', i * w + k, top_vals[i * w + k].tolist(), c)
          cands += [(score + lp[i * w + k, tk], k, tk) for tk in top[i * w + k]]
        cands.sort(key=lambda h: -h[0])  # stable: then slot, then token rank
        if on_select is not None:
          on_select('select', i, [h[0] for h in cands], w)
        new = []
        for slot, (score, k, tk) in enumerate(cands[:w]):
          new.append((cur[i][k][0] + (tk,), score))
          parent[i * w + slot], tok[i * w + slot] = i * w + k, tk
        cur[i] = new
      if lvl < s_max:
        pred_p, states = pred_fn(rows(tok), _Rows(states, rows(parent)))
    # Level 0 of the pool is the beam itself: where a frozen row stays.
    src = [i * p + k for i in range(b) for k in range(w)]
    for i in range(b):
      if not active[i]:
        continue
      merged = {}  # insertion order is pool order
      for idx, seq, score in pool[i]:
        if seq in merged:
          merged[seq][1] = lse(merged[seq][1], score)
        else:
          merged[seq] = [idx, score]
      live = sorted(((score, idx, seq) for seq, (idx, score) in merged.items()),
                    key=lambda h: -h[0])
      if on_select is not None:
        on_select('select', i, [h[0] for h in live], w)
      beams[i] = [(seq, score) for score, _, seq in live[:w]]
      for k in range(w):
        src[i * w + k] = i * p + (live[k][1] if k < len(live) else 0)
    src = rows(src)
    pred_p = _Pool(lv_pred, b, w).index_select(0, src)
    states = tuple(
        _Pool([st[k] for st in lv_states], b, w).index_select(0, src)
        for k in range(len(states)))

  ids = torch.zeros(b, w, t * s_max, dtype=torch.long)
  out_lens = torch.zeros(b, w, dtype=torch.long)
  scores = torch.full((b, w), _NEG, dtype=dt)
  for i, beam in enumerate(beams):
    for k, (seq, score) in enumerate(beam):
      ids[i, k, :len(seq)] = torch.tensor(seq, dtype=torch.long)
      out_lens[i, k] = len(seq)
      scores[i, k] = float(score)
  valid = torch.tensor([float(good) for good in ok], dtype=dt)
  return RnntBeam(ids.to(dev), out_lens.to(dev), scores.to(dev),
                  valid.to(dev))


def _HipRnntBeam(enc_p, enc_lengths, joint_w, joint_b, pred_fn, init_states,
                 w, c, s_max, blank_id):
  """The host loop around the kernels of ops/hip/rnnt_beam.hip: launches,
  index_select and pred_fn, all on the current stream."""
  fn = 'rnnt_beam_search'
  ext = _loader.get_ext(required=True)
  b, t, j = enc_p.shape
  v = joint_w.shape[1]
  wt = joint_w.t().contiguous()  # [V,J]: K-contiguous for the B fragments
  bias = joint_b.float().contiguous()
  ws = ext.rnnt_beam_init(enc_lengths, t, v, w, min(c, v - 1), s_max)
  parent, tok, src = ws[7], ws[8], ws[9]
  start = torch.full((b * w,), blank_id, dtype=torch.long, device=enc_p.device)
  pred_p, states = pred_fn(start, tuple(init_states))
  for f in range(t):
    lv_pred, lv_states = [], []
    for lvl in range(s_max + 1):
      if pred_p.dtype != torch.bfloat16 or pred_p.shape != (b * w, j):
        raise TypeError(f'{fn}: the HIP kernels take bf16 pred_p [B*W,J] from '
                        f'pred_fn, got {pred_p.dtype} {tuple(pred_p.shape)}')
      pred_p = pred_p.contiguous()
      lv_pred.append(pred_p)
      lv_states.append(states)
      ext.rnnt_beam_joint(enc_p, f, pred_p, wt, bias, ws, blank_id,
                          lvl < s_max)
      ext.rnnt_beam_expand(ws, enc_lengths, f, lvl, s_max, t, blank_id)
      if lvl < s_max:
        pred_p, states = pred_fn(tok, _Rows(states, parent))
        states = tuple(states)
    ext.rnnt_beam_close(ws, enc_lengths, f, s_max, t)
    pred_p = _Pool(lv_pred, b, w).index_select(0, src)
    states = tuple(
        _Pool([st[k] for st in lv_states], b, w).index_select(0, src)
        for k in range(len(states)))
  return RnntBeam(*ext.rnnt_beam_finish(ws, enc_lengths, s_max, t))


def rnnt_beam_search(enc_p: torch.Tensor, enc_lengths: torch.Tensor,
                     joint_w: torch.Tensor, joint_b: torch.Tensor, pred_fn,
                     init_states, beam_width: int = 8, token_beam: int = 8,
                     max_symbols: int = 3, blank_id: int = 0,
                     impl: str = 'auto') -> RnntBeam:
  """-> RnntBeam of the beam_width best label sequences; see the module
  docstring."""
  fn = 'rnnt_beam_search'
  if impl not in ('auto', 'torch'):
    raise ValueError(f"{fn}: impl must be 'auto' or 'torch', got {impl!r}")
  w, c, s_max, blank_id = \
      int(beam_width), int(token_beam), int(max_symbols), int(blank_id)
  if enc_p.dim() != 3 or not enc_p.is_floating_point():
    raise ValueError(f'{fn}: enc_p must be floating point [B,T,J], got '
                     f'{enc_p.dtype} {tuple(enc_p.shape)}')
  b, t, j = enc_p.shape
  if b < 1 or t < 1:
    raise ValueError(f'{fn}: B >= 1 and T >= 1')
  if joint_w.dim() != 2 or joint_w.shape[0] != j or joint_w.shape[1] < 2:
    raise ValueError(f'{fn}: joint_w must be [J={j},V>=2], got '
                     f'{tuple(joint_w.shape)}')
  v = joint_w.shape[1]
  if joint_b.shape != (v,):
    raise ValueError(f'{fn}: joint_b must be [V={v}], got '
                     f'{tuple(joint_b.shape)}')
  if not 0 <= blank_id < v:
    raise ValueError(f'{fn}: blank_id {blank_id} outside [0, {v})')
  if enc_lengths.dim() != 1 or enc_lengths.shape[0] != b or \
      enc_lengths.is_floating_point() or enc_lengths.dtype == torch.bool:
    raise TypeError(f'{fn}: enc_lengths must be an integer tensor [B]')
  for x in (enc_lengths, joint_w, joint_b):
    if x.device != enc_p.device:
      raise ValueError(f'{fn}: all inputs must be on one device')
  for name, got, top in (('beam_width', w, MAX_BEAM_WIDTH),
                         ('token_beam', c, MAX_TOKEN_BEAM),
                         ('max_symbols', s_max, MAX_SYMBOLS)):
    if not 1 <= got <= top:
      raise ValueError(f'{fn}: {name} {got} outside [1, {top}]')
  enc_lengths = enc_lengths.long().contiguous()
  with torch.no_grad():
    enc_p, joint_w, joint_b = \
        enc_p.detach(), joint_w.detach(), joint_b.detach()
    if impl == 'auto' and enc_p.is_cuda:
      if enc_p.dtype != torch.bfloat16 or joint_w.dtype != torch.bfloat16:
        raise TypeError(f'{fn}: the HIP kernels take bf16 enc_p and joint_w, '
                        f'got {enc_p.dtype} and {joint_w.dtype}')
      if joint_b.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f'{fn}: the HIP kernels take bf16 or fp32 joint_b, '
                        f'got {joint_b.dtype}')
      if j % 32 != 0 or j > MAX_JOINT_DIM:
        raise ValueError(f'{fn}: the HIP kernels need J % 32 == 0 and J <= '
                         f'{MAX_JOINT_DIM}, got J={j}')
      return _HipRnntBeam(enc_p.contiguous(), enc_lengths, joint_w, joint_b,
                          pred_fn, init_states, w, c, s_max, blank_id)
    wide = enc_p.dtype in (torch.float32, torch.float64)
    x = enc_p if wide else enc_p.float()
    return _TwinRnntBeam(x, enc_lengths, joint_w, joint_b, pred_fn,
                         init_states, w, c, s_max, blank_id,
                         operand_dtype=None if wide else enc_p.dtype)
