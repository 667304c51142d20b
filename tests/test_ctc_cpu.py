"""CTC loss op (ops/ctc.py) on CPU: the torch twin and impl='torch'
against torch's own CTC in float64, wrapper guards, and
CtcDecoder.GreedyDecode. Also holds the reference and the edge batch that
test_ctc_gpu.py shares."""

import pytest
import torch
import torch.nn.functional as F

from lingvo_amd.ops import ctc

EDGE_WEIGHTS = [1.0, 0.5, 2.0, 0.0, 1.0, 3.0]


def EdgeBatch():
  """B=6, T=9, V=5, L=4, blank 0: (logits bf16-exact fp32, T_b, labels,
  L_b). Row 2 is the only one without an alignment."""
  g = torch.Generator().manual_seed(1234)
  logits = (3.0 * torch.randn(6, 9, 5, generator=g)).bfloat16().float()
  labels = torch.tensor([[1, 2, 3, 4],    # plain
                         [2, 2, 2, 0],    # all repeats, exactly feasible
                         [1, 1, 2, 2],    # needs 6 frames, has 5
                         [3, 0, 0, 0],    # T = 1
                         [0, 0, 0, 0],    # empty target
                         [4, 3, 4, 3]])   # T = L, single alignment
  label_lengths = torch.tensor([4, 3, 4, 1, 0, 4])
  logit_lengths = torch.tensor([9, 5, 5, 1, 3, 4])
  return logits, logit_lengths, labels, label_lengths


def BadLabelBatch():
  """Two rows that are invalid by the label-range rule only: a blank and
  an id >= V inside the valid length (V=5)."""
  g = torch.Generator().manual_seed(4321)
  logits = (3.0 * torch.randn(2, 9, 5, generator=g)).bfloat16().float()
  labels = torch.tensor([[1, 0, 3, 4], [1, 2, 5, 4]])
  return logits, torch.tensor([9, 9]), labels, torch.tensor([4, 3])


def Reference(logits, logit_lengths, labels, label_lengths, weights,
              blank_id=0):
  """torch's CTC on CPU in float64 on exactly these logits ->
  (nll, valid, dlogits) for the loss sum_b weights_b * nll_b. valid is
  isfinite of the call without zero_infinity, ANDed with the label-range
  rule (rows that break it get labels torch can index with)."""
  logits = logits.detach().cpu().double()
  logit_lengths, labels, label_lengths = (
      x.detach().cpu() for x in (logit_lengths, labels, label_lengths))
  v = logits.shape[-1]
  inside = torch.arange(labels.shape[1])[None, :] < label_lengths[:, None]
  bad = inside & ((labels < 0) | (labels >= v) | (labels == blank_id))
  in_range = ~bad.any(-1)
  safe = torch.where(bad | ~inside, torch.full_like(labels, (blank_id + 1) % v),
                     labels)
  if safe.shape[1] == 0:
    safe = torch.full((labels.shape[0], 1), (blank_id + 1) % v)
  leaf = logits.clone().requires_grad_(True)

  def Call(zero_infinity):
    return F.ctc_loss(F.log_softmax(leaf, dim=-1).transpose(0, 1), safe,
                      logit_lengths, label_lengths, blank=blank_id,
                      reduction='none', zero_infinity=zero_infinity)

  valid = torch.isfinite(Call(False).detach()) & in_range
  nll = Call(True) * in_range.double()
  (nll * torch.as_tensor(weights, dtype=torch.float64)).sum().backward()
  return nll.detach(), valid.double(), leaf.grad


def RandomBatch(b, t, v, l, seed, scale=1.0):
  """Random logits and labels; row 0 has full lengths, the others random
  ones (so some rows may have no alignment; the reference decides)."""
  g = torch.Generator().manual_seed(seed)
  logits = scale * torch.randn(b, t, v, generator=g)
  labels = torch.randint(1, v, (b, l), generator=g)
  logit_lengths = torch.randint(max(t // 2, 1), t + 1, (b,), generator=g)
  label_lengths = torch.randint(l // 2, l + 1, (b,), generator=g)
  logit_lengths[0] = t
  label_lengths[0] = l
  return logits, logit_lengths, labels, label_lengths


def RandomWeights(b, seed):
  g = torch.Generator().manual_seed(seed + 77)
  w = 0.5 + torch.rand(b, generator=g)
  if b >= 2:
    w[-1] = 0.0  # a zero-weight row
  return w.tolist()


def _Run(batch, weights, dtype, impl='auto'):
  logits, tl, labels, ll = batch
  x = logits.to(dtype).requires_grad_(True)
  nll, valid = ctc.ctc_loss(x, tl, labels, ll, impl=impl)
  assert not valid.requires_grad
  (nll * torch.as_tensor(weights, dtype=nll.dtype)).sum().backward()
  return nll.detach(), valid, x.grad


def _Close(got, want, tag):
  err = (got - want).abs()
  bound = 1e-9 + 1e-9 * want.abs()
  print(f'{tag}: max err {float(err.max()):.3g}')
  assert bool((err <= bound).all()), tag


_CASES = {
    'edge': lambda: (EdgeBatch(), EDGE_WEIGHTS),
    'b1t1v2l1': lambda: (RandomBatch(1, 1, 2, 1, 11), RandomWeights(1, 11)),
    'b3t12v7l5': lambda: (RandomBatch(3, 12, 7, 5, 12), RandomWeights(3, 12)),
    'b2t40v76l9': lambda: (RandomBatch(2, 40, 76, 9, 13),
                           RandomWeights(2, 13)),
}


@pytest.mark.parametrize('case', sorted(_CASES))
@pytest.mark.parametrize('impl', ['auto', 'torch'])
def test_float64_matches_reference(case, impl):
  batch, weights = _CASES[case]()
  want_nll, want_valid, want_grad = Reference(*batch, weights)
  nll, valid, grad = _Run(batch, weights, torch.float64, impl)
  assert nll.dtype == torch.float64 and grad.dtype == torch.float64
  assert torch.equal(valid, want_valid), (valid, want_valid)
  _Close(nll, want_nll, f'{case} {impl} nll')
  _Close(grad, want_grad, f'{case} {impl} dlogits')
  assert bool((nll[want_valid == 0] == 0).all())
  assert bool((grad[want_valid == 0] == 0).all())


def test_edge_batch_invalid_row_and_padded_frames():
  batch = EdgeBatch()
  _, tl, _, _ = batch
  nll, valid, grad = _Run(batch, EDGE_WEIGHTS, torch.float64)
  assert valid.tolist() == [1, 1, 0, 1, 1, 1]
  assert float(nll[2]) == 0.0
  assert bool((grad[2] == 0).all())      # infeasible row
  assert bool((grad[3] == 0).all())      # zero-weight row
  for b in range(6):
    assert bool((grad[b, int(tl[b]):] == 0).all()), b
  assert float(grad[0].abs().max()) > 0


@pytest.mark.parametrize('impl', ['auto', 'torch'])
def test_bad_labels_are_invalid_rows(impl):
  batch = BadLabelBatch()
  nll, valid, grad = _Run(batch, [1.0, 1.0], torch.float64, impl)
  want_nll, want_valid, want_grad = Reference(*batch, [1.0, 1.0])
  assert want_valid.tolist() == [0, 0]
  assert valid.tolist() == [0, 0]
  assert bool((nll == 0).all()) and bool((grad == 0).all())
  assert bool((want_nll == 0).all()) and bool((want_grad == 0).all())


def test_fp32_twin_returns_fp32_and_is_close():
  batch, weights = _CASES['b3t12v7l5']()
  want_nll, want_valid, want_grad = Reference(
      batch[0].float(), *batch[1:], weights)
  nll, valid, grad = _Run(batch, weights, torch.float32)
  assert nll.dtype == torch.float32 and grad.dtype == torch.float32
  assert torch.equal(valid.double(), want_valid)
  # fp32 recursion of depth 12 on O(10) values: far inside 1e-4.
  assert float((nll.double() - want_nll).abs().max()) < 1e-4
  assert float((grad.double() - want_grad).abs().max()) < 1e-4


def test_gradcheck():
  x = torch.randn(2, 4, 3, dtype=torch.float64,
                  generator=torch.Generator().manual_seed(5))
  x.requires_grad_(True)
  tl = torch.tensor([4, 3])
  labels = torch.tensor([[1, 2], [1, 1]])
  ll = torch.tensor([2, 1])
  assert torch.autograd.gradcheck(
      lambda a: ctc.ctc_loss(a, tl, labels, ll)[0], (x,))


def test_wrapper_guards():
  logits, tl, labels, ll = EdgeBatch()
  with pytest.raises(TypeError):
    ctc.ctc_loss(logits.long(), tl, labels, ll)              # logits dtype
  with pytest.raises(TypeError):
    ctc.ctc_loss(logits, tl, labels.int(), ll)               # labels dtype
  with pytest.raises(TypeError):
    ctc.ctc_loss(logits, tl.float(), labels, ll)             # lengths dtype
  with pytest.raises(ValueError):
    ctc.ctc_loss(logits.transpose(0, 1), tl, labels, ll)     # not contiguous
  for blank in (-1, 5):
    with pytest.raises(ValueError):
      ctc.ctc_loss(logits, tl, labels, ll, blank_id=blank)
  with pytest.raises(ValueError):
    ctc.ctc_loss(logits[:, :, :1].contiguous(), tl, labels, ll)  # V < 2
  with pytest.raises(ValueError):
    ctc.ctc_loss(logits, tl, labels, ll, impl='cudnn')
  wide = torch.ones(6, ctc.MAX_LABEL_LEN + 1, dtype=torch.long)
  with pytest.raises(ValueError):
    ctc.ctc_loss(logits, tl, wide, ll)                       # L over limit
  at_limit = torch.ones(6, ctc.MAX_LABEL_LEN, dtype=torch.long)
  nll, valid = ctc.ctc_loss(logits, tl, at_limit, ll)
  assert nll.shape == (6,)
  assert ctc.MAX_LABEL_LEN >= 511


def test_nonzero_blank_id():
  logits, tl, labels, ll = RandomBatch(3, 10, 6, 3, 21)
  labels = labels.clamp(max=4)  # blank is 5
  weights = [1.0, 2.0, 0.5]
  logits = logits.double()
  want = Reference(logits, tl, labels, ll, weights, blank_id=5)
  x = logits.clone().requires_grad_(True)
  nll, valid = ctc.ctc_loss(x, tl, labels, ll, blank_id=5)
  (nll * torch.tensor(weights, dtype=torch.float64)).sum().backward()
  assert torch.equal(valid, want[1])
  _Close(nll.detach(), want[0], 'blank5 nll')
  _Close(x.grad, want[2], 'blank5 dlogits')


# ---- CtcDecoder.GreedyDecode -------------------------------------------------
def _Collapse(frames, blank=0):
  out, prev = [], None
  for tok in frames:
    if tok != prev and tok != blank:
      out.append(tok)
    prev = tok
  return out


def _DecoderWithIdentityLogits(v):
  from lingvo_amd.models import asr
  dec = asr.CtcDecoder.Params().Set(
      name='ctc', vocab_size=v, source_dim=v, dropout_prob=0.0).Instantiate()
  dec.eval()
  with torch.no_grad():
    dec.softmax.linear_w.copy_(torch.eye(v))
    dec.softmax.bias.zero_()
  return dec


def test_greedy_decode_collapses_like_the_python_loop():
  v = 6
  dec = _DecoderWithIdentityLogits(v)
  frames = [
      [1, 1, 0, 1, 2, 2, 3, 0],   # repeat split by a blank: two tokens
      [4, 4, 4, 5, 5, 0, 0, 0],   # repeats with no blank between: merged
      [2, 0, 3, 3, 5, 5, 5, 5],   # last four frames are padding
      [0, 0, 0, 0, 0, 0, 0, 0],   # all blank
      [3, 1, 4, 1, 5, 2, 1, 3],   # nothing to collapse: full width
  ]
  lengths = [8, 8, 4, 8, 8]
  ids = torch.tensor(frames)
  enc = F.one_hot(ids, v).float() * 5.0
  pad = (torch.arange(8)[None, :] >= torch.tensor(lengths)[:, None]).float()
  hyps = dec.GreedyDecode(dec.theta, enc, pad)
  assert hyps.shape == (5, 8) and hyps.dtype == torch.long
  for b, (row, n) in enumerate(zip(frames, lengths)):
    want = _Collapse(row[:n])
    want = want + [0] * (8 - len(want))
    assert hyps[b].tolist() == want, (b, hyps[b].tolist(), want)
  assert hyps[0].tolist()[:4] == [1, 1, 2, 3]
  assert hyps[1].tolist()[:3] == [4, 5, 0]
  assert hyps[2].tolist() == [2, 3, 0, 0, 0, 0, 0, 0]
  assert hyps[3].tolist() == [0] * 8


def test_beam_search_decode_is_not_built():
  dec = _DecoderWithIdentityLogits(4)
  with pytest.raises(NotImplementedError, match='prefix beam search'):
    dec.BeamSearchDecode(dec.theta, torch.zeros(1, 3, 4), torch.zeros(1, 3))
