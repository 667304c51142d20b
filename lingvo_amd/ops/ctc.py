"""CTC loss over batch-major logits.

  nll, valid = ctc_loss(logits, logit_lengths, labels, label_lengths,
                        blank_id=0, impl='auto')

logits [B,T,V], labels [B,L] int64, lengths [B]. nll [B] is the negative
log-likelihood of each utterance and valid [B] (1 or 0, no gradient) says
whether it has one. A row is invalid - valid = 0, nll = 0, zero gradient -
when its lengths are outside [1,T] / [0,L], when a label inside its length
is the blank or outside [0,V), or when no alignment exists
(T_b < L_b + number of adjacent equal labels). An empty target is valid:
the all-blank path.

CUDA tensors run the HIP kernels of ops/hip/ctc.hip (bf16 or fp32 logits,
no fp32 [B,T,V] intermediate, deterministic backward). CPU tensors run a
torch twin of the same recursion in the dtype of the input (fp32 or
fp64). impl='torch' routes to torch.nn.functional.ctc_loss on either
device: the yardstick for tests and benchmarks.

  al = ctc_forced_align(logits, logit_lengths, labels, label_lengths,
                        blank_id=0, impl='auto')

is the best single alignment of each transcript (Viterbi) under the same
inputs, checks and validity rules, as a CtcAlignment:
  frame_ids   [B,T] int64  the label (or blank_id) each frame is aligned to
  token_start [B,L] int64  first frame of each label
  token_end   [B,L] int64  one past its last frame
  token_logp  [B,L]        sum of its frames' log-probs
  score       [B]          log-prob of the whole path
  valid       [B]          1 or 0
Units are frames of `logits`. Among predecessors of equal value the
smallest jump wins (stay, then step, then skip), and of the two end
positions the last label wins a tie with the final blank. Frames >= T_b
get frame_ids -1, label slots >= L_b get spans -1 and token_logp 0, and an
invalid row - the rules above, or a best score that is not possible - gets
all of those and score 0. No output carries a gradient; logits that
require one are detached.

CUDA tensors run ctc_rows_kernel and ctc_viterbi_kernel of ops/hip/ctc.hip
(two launches, no host sync, fp32 score and token_logp). CPU tensors run
a batched torch twin of that recursion in the dtype of the input;
impl='torch' runs the twin on whichever device the inputs are on: the
composed-ops yardstick for the benchmark.
"""

from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn.functional as F

from lingvo_amd.ops import _loader

# Label width the kernels support: one lane per lattice position,
# 2L+1 <= 1023 lanes of a workgroup.
MAX_LABEL_LEN = 511

_NEG = -1e30
_NEG_TEST = -1e29


def _Validity(logit_lengths, labels, label_lengths, t, v, blank_id):
  """(valid [B] bool, T_b, L_b, labels safe to index with): the
  combinatorial invalid-row rules, in plain torch ops without a sync."""
  l = labels.shape[1]
  len_ok = ((logit_lengths >= 1) & (logit_lengths <= t) &
            (label_lengths >= 0) & (label_lengths <= l))
  tb = torch.where(len_ok, logit_lengths, torch.zeros_like(logit_lengths))
  lb = torch.where(len_ok, label_lengths, torch.zeros_like(label_lengths))
  pos = torch.arange(l, device=labels.device)[None, :]
  inside = pos < lb[:, None]
  bad = inside & ((labels < 0) | (labels >= v) | (labels == blank_id))
  rep = torch.zeros_like(inside)
  if l > 1:
    rep[:, 1:] = inside[:, 1:] & (labels[:, 1:] == labels[:, :-1])
  valid = len_ok & ~bad.any(-1) & (tb >= lb + rep.sum(-1))
  safe = torch.where(inside & ~bad, labels, torch.zeros_like(labels))
  return valid, tb, lb, safe


def _Lse3(a, b, c):
  m = torch.maximum(a, torch.maximum(b, c))
  out = m + torch.log(torch.exp(a - m) + torch.exp(b - m) +
                      torch.exp(c - m))
  return torch.where(m > _NEG_TEST, out, torch.full_like(out, _NEG))


def _ShiftRight(x, n):
  """x[:, s-n] at position s, 'impossible' where s < n."""
  if n >= x.shape[1]:
    return torch.full_like(x, _NEG)
  return torch.cat([torch.full_like(x[:, :n], _NEG), x[:, :-n]], dim=1)


def _ShiftLeft(x, n):
  if n >= x.shape[1]:
    return torch.full_like(x, _NEG)
  return torch.cat([x[:, n:], torch.full_like(x[:, :n], _NEG)], dim=1)


def _Emissions(logits, safe, blank_id):
  """(log-probs [B,T,V], extended labels [B,S], emissions [B,T,S]) of the
  blank-interleaved label sequence, S = 2L+1."""
  b, t, _ = logits.shape
  s = 2 * safe.shape[1] + 1
  lp = F.log_softmax(logits, dim=-1)
  ext = torch.full((b, s), blank_id, dtype=torch.long, device=logits.device)
  ext[:, 1::2] = safe
  return lp, ext, lp.gather(2, ext[:, None, :].expand(b, t, s))


def _TwinForward(logits, logit_lengths, labels, label_lengths, blank_id):
  """The kernels' recursion in torch ops, batched over B, in
  logits.dtype. Returns nll, valid and what the backward needs."""
  b, t, v = logits.shape
  l = labels.shape[1]
  s = 2 * l + 1
  dev = logits.device
  valid, tb, lb, safe = _Validity(logit_lengths, labels, label_lengths, t, v,
                                  blank_id)
  lp, ext, emis = _Emissions(logits, safe, blank_id)
  pos = torch.arange(s, device=dev)[None, :]
  sb = 2 * lb[:, None] + 1
  active = pos < sb
  odd = (pos % 2) == 1
  neg = torch.full((b, s), _NEG, dtype=logits.dtype, device=dev)
  # A step of two positions is allowed only between different labels.
  skip_a = torch.zeros(b, s, dtype=torch.bool, device=dev)
  skip_b = torch.zeros(b, s, dtype=torch.bool, device=dev)
  if s >= 3:
    diff = ext[:, 2:] != ext[:, :-2]
    skip_a[:, 2:] = odd[:, 2:] & active[:, 2:] & diff
    skip_b[:, :-2] = odd[:, :-2] & (pos[:, :-2] + 2 < sb) & diff

  alpha = torch.full((b, t, s), _NEG, dtype=logits.dtype, device=dev)
  beta = torch.full((b, t, s), _NEG, dtype=logits.dtype, device=dev)
  a = torch.where((pos < 2) & active, emis[:, 0], neg)
  alpha[:, 0] = a
  for i in range(1, t):
    l3 = _Lse3(a, _ShiftRight(a, 1),
               torch.where(skip_a, _ShiftRight(a, 2), neg))
    new = torch.where(active & (l3 > _NEG_TEST), emis[:, i] + l3, neg)
    a = torch.where((i < tb)[:, None], new, a)  # frozen past the end
    alpha[:, i] = a
  last = (pos == sb - 1) | (pos == sb - 2)
  bt = neg
  for i in range(t - 1, -1, -1):
    l3 = _Lse3(bt, _ShiftLeft(bt, 1),
               torch.where(skip_b, _ShiftLeft(bt, 2), neg))
    new = torch.where(active & (l3 > _NEG_TEST), emis[:, i] + l3, neg)
    new = torch.where((i == tb - 1)[:, None],
                      torch.where(last, emis[:, i], neg), new)
    bt = torch.where((i < tb)[:, None], new, neg)
    beta[:, i] = bt
  a1 = a.gather(1, (sb - 1).clamp(min=0))[:, 0]
  a2 = torch.where(sb[:, 0] >= 2,
                   a.gather(1, (sb - 2).clamp(min=0))[:, 0], neg[:, 0])
  m = torch.maximum(a1, a2)
  ll = m + torch.log(torch.exp(a1 - m) + torch.exp(a2 - m))
  valid = valid & (m > _NEG_TEST) & torch.isfinite(ll)
  nll = torch.where(valid, -ll, torch.zeros_like(ll))
  return nll, valid.to(logits.dtype), (lp, ext, emis, alpha, beta, tb)


def _TwinBackward(gout, nll, valid, saved):
  lp, ext, emis, alpha, beta, tb = saved
  b, t, v = lp.shape
  s = ext.shape[1]
  live = (valid > 0)[:, None] & \
      (torch.arange(t, device=lp.device)[None, :] < tb[:, None])  # [B,T]
  log_occ = alpha + beta - emis + nll[:, None, None]
  occ = torch.where(live[:, :, None], torch.exp(log_occ),
                    torch.zeros_like(log_occ))
  occ_v = torch.zeros_like(lp).scatter_add_(
      2, ext[:, None, :].expand(b, t, s), occ)
  grad = torch.exp(lp) - occ_v
  scale = torch.where(live, gout[:, None].expand(b, t),
                      torch.zeros_like(live, dtype=lp.dtype))
  return torch.where(live[:, :, None], grad * scale[:, :, None],
                     torch.zeros_like(grad))


class _CtcLossFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, logits, logit_lengths, labels, label_lengths, blank_id):
    ctx.blank_id = blank_id
    ctx.is_hip = logits.is_cuda
    if logits.is_cuda:
      ext = _loader.get_ext(required=True)
      nll, valid, lse, emis, alpha, beta = ext.ctc_fwd(
          logits, logit_lengths, labels, label_lengths, blank_id)
      ctx.save_for_backward(logits, logit_lengths, labels, label_lengths,
                            lse, emis, alpha, beta, nll, valid)
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
       nll, valid) = ctx.saved_tensors
      dlogits = ext.ctc_bwd(logits, logit_lengths, labels, label_lengths,
                            lse, emis, alpha, beta, nll, valid,
                            gnll.float().contiguous(), ctx.blank_id)
    else:
      nll, valid, *saved = ctx.saved_tensors
      dlogits = _TwinBackward(gnll.to(nll.dtype), nll, valid,
                              saved).to(ctx.in_dtype)
    return dlogits, None, None, None, None


def _TorchCtc(logits, logit_lengths, labels, label_lengths, blank_id):
  """torch.nn.functional.ctc_loss with this module's (nll, valid)
  contract. Invalid rows are masked and their labels made safe to index
  with first; torch reads the lengths on the host."""
  b, t, v = logits.shape
  valid, tb, lb, safe = _Validity(logit_lengths, labels, label_lengths, t, v,
                                  blank_id)
  x = logits if logits.dtype == torch.float64 else logits.float()
  safe = torch.where(safe == blank_id, torch.full_like(safe, (blank_id + 1) % v),
                     safe)
  if safe.shape[1] == 0:  # torch wants a target column to exist
    safe = torch.full((b, 1), (blank_id + 1) % v, dtype=torch.long,
                      device=labels.device)
  nll = F.ctc_loss(F.log_softmax(x, dim=-1).transpose(0, 1), safe,
                   tb.clamp(min=1), lb, blank=blank_id, reduction='none',
                   zero_infinity=True)
  valid = valid.to(nll.dtype)
  return nll * valid, valid


def _CheckArgs(logits, logit_lengths, labels, label_lengths, blank_id,
               fn='ctc_loss'):
  if logits.dim() != 3:
    raise ValueError(f'{fn}: logits must be [B,T,V], got '
                     f'{tuple(logits.shape)}')
  if not logits.is_floating_point():
    raise TypeError(f'{fn}: logits must be floating point, got '
                    f'{logits.dtype}')
  if not logits.is_contiguous():
    raise ValueError(f'{fn}: logits must be contiguous')
  b, t, v = logits.shape
  if b < 1 or t < 1:
    raise ValueError(f'{fn}: B >= 1 and T >= 1')
  if v < 2:
    raise ValueError(f'{fn}: V >= 2')
  if not 0 <= blank_id < v:
    raise ValueError(f'{fn}: blank_id {blank_id} outside [0, {v})')
  if labels.dtype != torch.int64 or labels.dim() != 2 or \
      labels.shape[0] != b:
    raise TypeError(f'{fn}: labels must be int64 [B,L]')
  if labels.shape[1] > MAX_LABEL_LEN:
    raise ValueError(f'{fn}: L={labels.shape[1]} is over the supported '
                     f'limit {MAX_LABEL_LEN}')
  for name, x in (('logit_lengths', logit_lengths),
                  ('label_lengths', label_lengths)):
    if x.dim() != 1 or x.shape[0] != b or x.is_floating_point() or \
        x.dtype == torch.bool:
      raise TypeError(f'{fn}: {name} must be an integer tensor [B]')
  for x in (logit_lengths, labels, label_lengths):
    if x.device != logits.device:
      raise ValueError(f'{fn}: all inputs must be on one device')


def ctc_loss(logits: torch.Tensor, logit_lengths: torch.Tensor,
             labels: torch.Tensor, label_lengths: torch.Tensor,
             blank_id: int = 0, impl: str = 'auto'):
  """-> (nll [B], valid [B]); see the module docstring."""
  if impl not in ('auto', 'torch'):
    raise ValueError(f"ctc_loss: impl must be 'auto' or 'torch', got {impl!r}")
  blank_id = int(blank_id)
  _CheckArgs(logits, logit_lengths, labels, label_lengths, blank_id)
  logit_lengths = logit_lengths.long().contiguous()
  label_lengths = label_lengths.long().contiguous()
  labels = labels.contiguous()
  if impl == 'torch':
    return _TorchCtc(logits, logit_lengths, labels, label_lengths, blank_id)
  if logits.is_cuda and logits.dtype not in (torch.bfloat16, torch.float32):
    raise TypeError(f'ctc_loss: the HIP kernels take bf16 or fp32 logits, '
                    f'got {logits.dtype}')
  return _CtcLossFn.apply(logits, logit_lengths, labels, label_lengths,
                          blank_id)


class CtcAlignment(NamedTuple):
  """What ctc_forced_align returns; see the module docstring."""
  frame_ids: torch.Tensor    # [B,T] int64
  token_start: torch.Tensor  # [B,L] int64
  token_end: torch.Tensor    # [B,L] int64
  token_logp: torch.Tensor   # [B,L]
  score: torch.Tensor        # [B]
  valid: torch.Tensor        # [B]


def _TwinAlign(logits, logit_lengths, labels, label_lengths, blank_id):
  """ctc_viterbi_kernel's recursion in torch ops, batched over B, in
  logits.dtype: max in place of logsumexp with a [B,T,S] int8 backpointer
  tensor, then a backtrace of one gather per frame. No host sync."""
  b, t, v = logits.shape
  l = labels.shape[1]
  s = 2 * l + 1
  dev = logits.device
  valid, tb, lb, safe = _Validity(logit_lengths, labels, label_lengths, t, v,
                                  blank_id)
  _, ext, emis = _Emissions(logits, safe, blank_id)
  pos = torch.arange(s, device=dev)[None, :]
  sb = 2 * lb[:, None] + 1
  active = pos < sb
  neg = torch.full((b, s), _NEG, dtype=logits.dtype, device=dev)
  # A step of two positions is allowed only between different labels.
  skip = torch.zeros(b, s, dtype=torch.bool, device=dev)
  if s >= 3:
    skip[:, 2:] = ((pos[:, 2:] % 2) == 1) & active[:, 2:] & \
        (ext[:, 2:] != ext[:, :-2])

  # Forward: which predecessor won (0 stay, 1 step, 2 skip); among equal
  # values the smallest jump, so only a strictly larger value replaces.
  a = torch.where((pos < 2) & active, emis[:, 0], neg)
  bp = torch.zeros(b, t, s, dtype=torch.int8, device=dev)
  for i in range(1, t):
    m = a
    mv = torch.zeros(b, s, dtype=torch.int8, device=dev)
    for jump, cand in ((1, _ShiftRight(a, 1)),
                       (2, torch.where(skip, _ShiftRight(a, 2), neg))):
      take = cand > m
      m = torch.where(take, cand, m)
      mv = torch.where(take, torch.full_like(mv, jump), mv)
    new = torch.where(active & (m > _NEG_TEST), emis[:, i] + m, neg)
    live = (i < tb)[:, None]
    a = torch.where(live, new, a)  # frozen past the end
    bp[:, i] = torch.where(live, mv, torch.zeros_like(mv))
  a1 = a.gather(1, (sb - 1).clamp(min=0))[:, 0]
  a2 = torch.where(sb[:, 0] >= 2,
                   a.gather(1, (sb - 2).clamp(min=0))[:, 0], neg[:, 0])
  end_last = a1 >= a2  # the last position wins a tie
  best = torch.where(end_last, a1, a2)
  valid = valid & (best > _NEG_TEST)

  # Backtrace: state [B,T] is the lattice position of each frame, -1 on
  # padded frames and invalid rows.
  cur = torch.where(end_last, sb[:, 0] - 1, sb[:, 0] - 2).clamp(min=0)
  state = torch.full((b, t), -1, dtype=torch.long, device=dev)
  for i in range(t - 1, -1, -1):
    on = valid & (i < tb)
    state[:, i] = torch.where(on, cur, torch.full_like(cur, -1))
    mv = bp[:, i].gather(1, cur[:, None])[:, 0].long()
    cur = torch.where(on, cur - mv, cur)
  on = state >= 0
  at = state.clamp(min=0)
  frame_ids = torch.where(on, ext.gather(1, at), torch.full_like(at, -1))
  logp = torch.where(on, emis.gather(2, at[:, :, None])[:, :, 0],
                     torch.zeros_like(emis[:, :, 0]))
  # Per label: first frame, one past the last frame, sum of log-probs.
  # Frames on a blank go to a spare column l.
  tok = torch.where(on & (at % 2 == 1), at // 2, torch.full_like(at, l))
  frame = torch.arange(t, device=dev)[None, :].expand(b, t)
  start = torch.full((b, l + 1), t, dtype=torch.long, device=dev)
  start = start.scatter_reduce(1, tok, frame, 'amin')[:, :l]
  end = torch.full((b, l + 1), -1, dtype=torch.long, device=dev)
  end = end.scatter_reduce(1, tok, frame, 'amax')[:, :l] + 1
  token_logp = torch.zeros(b, l + 1, dtype=logits.dtype, device=dev)
  token_logp = token_logp.scatter_add(1, tok, logp)[:, :l]
  used = valid[:, None] & \
      (torch.arange(l, device=dev)[None, :] < lb[:, None])
  return CtcAlignment(
      frame_ids=frame_ids,
      token_start=torch.where(used, start, torch.full_like(start, -1)),
      token_end=torch.where(used, end, torch.full_like(end, -1)),
      token_logp=torch.where(used, token_logp, torch.zeros_like(token_logp)),
      score=torch.where(valid, best, torch.zeros_like(best)),
      valid=valid.to(logits.dtype))


def ctc_forced_align(logits: torch.Tensor, logit_lengths: torch.Tensor,
                     labels: torch.Tensor, label_lengths: torch.Tensor,
                     blank_id: int = 0, impl: str = 'auto') -> CtcAlignment:
  """-> CtcAlignment of the best alignment; see the module docstring."""
  fn = 'ctc_forced_align'
  if impl not in ('auto', 'torch'):
    raise ValueError(f"{fn}: impl must be 'auto' or 'torch', got {impl!r}")
  blank_id = int(blank_id)
  _CheckArgs(logits, logit_lengths, labels, label_lengths, blank_id, fn=fn)
  logits = logits.detach()
  logit_lengths = logit_lengths.long().contiguous()
  label_lengths = label_lengths.long().contiguous()
  labels = labels.contiguous()
  if impl == 'auto' and logits.is_cuda:
    if logits.dtype not in (torch.bfloat16, torch.float32):
      raise TypeError(f'{fn}: the HIP kernels take bf16 or fp32 logits, got '
                      f'{logits.dtype}')
    ext = _loader.get_ext(required=True)
    # True: backpointer masks in LDS where all T frames fit.
    return CtcAlignment(*ext.ctc_align(logits, logit_lengths, labels,
                                       label_lengths, blank_id, True))
  x = logits if logits.dtype == torch.float64 else logits.float()
  return _TwinAlign(x, logit_lengths, labels, label_lengths, blank_id)
