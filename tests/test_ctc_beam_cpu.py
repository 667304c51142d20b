"""CTC prefix beam search (ops.ctc.ctc_beam_search) on the CPU: the twin
against torch's CTC where nothing is pruned, the cases and checks the GPU
tests share, and the CtcDecoder / AsrModel wiring."""

import functools
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from lingvo_amd.ops import ctc

# Check 2. DELTA: rows whose reference has a smaller score gap at a keep/drop
# boundary or between neighbours of the final list are left out. SCORE_TOL is
# 4x the largest |kernel score - fp64 reference| measured on an MI355X over
# PRUNED (see docs/KERNEL_NOTES.md); DELTA >= 10 * SCORE_TOL.
DELTA = 1e-3
SCORE_TOL = 4 * 2.66e-6

# name: (B, T, V, W, C, scale of randn)
PRUNED = {
    't16_v24_w4_c4': (32, 16, 24, 4, 4, 4.0),
    't12_v16_w4_c4': (32, 12, 16, 4, 4, 4.0),
    't20_v40_w8_c6': (32, 20, 40, 8, 6, 5.0),
    't12_v17_w1_c4': (8, 12, 17, 1, 4, 4.0),    # W = 1, odd V
    't12_v2_w4_c8': (8, 12, 2, 4, 8, 4.0),      # C clamps to 1
    't9_v5_w8_c16': (8, 9, 5, 8, 16, 4.0),      # C clamps to 4
    # The widest workgroup; sharp rows keep 32 neighbours apart.
    't10_v77_w32_c16': (4, 10, 77, 32, 16, 12.0),
}
# name: (V, T, C), every prefix fits in W = 32
EXHAUSTIVE = {'v3_t4': (3, 4, 2), 'v4_t2': (4, 2, 3)}


def _Lengths(b, t, g):
  """T_b of 0, 1 and T-1 are present; the rest lie in [T/2, T]."""
  lengths = torch.randint(t // 2, t + 1, (b,), generator=g)
  lengths[:4] = torch.tensor([t, 0, 1, t - 1])
  return lengths


@functools.lru_cache(maxsize=None)
def PrunedCase(name):
  """(fp32 logits, lengths, W, C, fp64 reference, gap per row). Built once;
  callers must not modify it."""
  b, t, v, w, c, scale = PRUNED[name]
  g = torch.Generator().manual_seed(0)
  logits = torch.randn(b, t, v, generator=g) * scale
  lengths = _Lengths(b, t, g)
  gaps, final = [math.inf] * b, {}

  def on_select(row, scores):
    if len(scores) > w:
      gaps[row] = min(gaps[row], float(scores[w - 1] - scores[w]))
    final[row] = scores[:w]

  want = ctc._TwinBeam(logits.double(), lengths, w, c, 0, on_select)
  for row, scores in final.items():
    for hi, lo in zip(scores, scores[1:]):
      gaps[row] = min(gaps[row], float(hi - lo))
  return logits, lengths, w, c, want, gaps


def CheckPruned(got, name):
  """-> largest score error over the compared rows."""
  _, _, _, _, want, gaps = PrunedCase(name)
  got = [x.cpu() for x in got]
  assert torch.equal(got[3].double(), want.valid)
  worst = 0.0
  for row, gap in enumerate(gaps):
    if gap < DELTA:
      continue
    assert torch.equal(got[0][row], want.topk_ids[row]), (name, row)
    assert torch.equal(got[1][row], want.topk_lens[row]), (name, row)
    used = want.topk_scores[row] > -1e29
    assert bool((got[2][row][~used] < -1e29).all()), (name, row)
    err = (got[2][row][used].double() - want.topk_scores[row][used]).abs()
    worst = max(worst, float(err.max()) if err.numel() else 0.0)
  print(f'ctc beam {name}: max score error {worst:.3g}')
  assert worst <= SCORE_TOL, (name, worst)
  return worst


@functools.lru_cache(maxsize=None)
def ExhaustiveCase(name, blank):
  """(fp64 logits, lengths, C, per row {labels: log-prob} from torch's CTC
  for every label sequence that has an alignment)."""
  v, t, c = EXHAUSTIVE[name]
  g = torch.Generator().manual_seed(1)
  logits = (torch.randn(2, t, v, generator=g) * 2.0).double()  # fp32 values
  lengths = torch.tensor([t, t - 1])
  lp = F.log_softmax(logits, dim=-1)
  tokens = [i for i in range(v) if i != blank]
  want = []
  for row, tb in enumerate(lengths.tolist()):
    scores = {(): float(lp[row, :tb, blank].sum())}
    for n in range(1, tb + 1):
      for labels in itertools.product(tokens, repeat=n):
        nll = F.ctc_loss(lp[row, :tb, None], torch.tensor([labels]),
                         torch.tensor([tb]), torch.tensor([n]), blank=blank,
                         reduction='none')
        if math.isfinite(float(nll)):
          scores[labels] = -float(nll)
    want.append(scores)
  return logits, lengths, c, want


def CheckExhaustive(got, want, tol):
  ids, lens, scores, valid = (x.cpu() for x in got)
  assert valid.tolist() == [1, 1]
  for row, scores_want in enumerate(want):
    found = {tuple(ids[row, k, :lens[row, k]].tolist()): float(scores[row, k])
             for k in range(ids.shape[1]) if scores[row, k] > -1e29}
    assert found.keys() == scores_want.keys()
    for labels, s in scores_want.items():
      assert abs(found[labels] - s) <= tol, (labels, found[labels], s)


@pytest.mark.parametrize('blank_last', [False, True])
@pytest.mark.parametrize('name', list(EXHAUSTIVE))
def test_twin_sums_every_alignment(name, blank_last):
  blank = EXHAUSTIVE[name][0] - 1 if blank_last else 0
  logits, lengths, c, want = ExhaustiveCase(name, blank)
  got = ctc.ctc_beam_search(logits, lengths, 32, c, blank)
  assert got.topk_scores.dtype == torch.float64
  CheckExhaustive(got, want, 1e-12 * 32)  # a few fp64 ulps of |score| <= 32


@pytest.mark.parametrize('name', list(PRUNED))
def test_reference_is_decisive_on_most_rows(name):
  """The rule of check 2 on the reference alone, and the output contract:
  descending scores, left-packed rows, the sentinel in unused slots."""
  logits, lengths, w, _, want, gaps = PrunedCase(name)
  assert 4 * sum(g < DELTA for g in gaps) <= len(gaps), gaps
  assert DELTA >= 10 * SCORE_TOL
  b, t, _ = logits.shape
  assert want.topk_ids.shape == (b, w, t) and want.topk_lens.shape == (b, w)
  assert bool((want.topk_scores[:, :-1] >= want.topk_scores[:, 1:]).all())
  used = want.topk_scores > -1e29
  assert bool((want.topk_lens[~used] == 0).all())
  pad = torch.arange(t)[None, None, :] >= want.topk_lens[:, :, None]
  assert bool((want.topk_ids[pad] == 0).all())
  # T_b = 0: the empty prefix with score 0 and nothing else.
  assert want.topk_lens[1].tolist() == [0] * w
  assert want.topk_scores[1].tolist() == [0.0] + [-1e30] * (w - 1)


def test_bad_arguments_and_lengths():
  logits, lengths = torch.randn(3, 4, 5), torch.tensor([5, -1, 4])
  beam = ctc.ctc_beam_search(logits, lengths, 2, 2)
  assert beam.valid.tolist() == [0, 0, 1]
  assert bool((beam.topk_scores[:2] < -1e29).all())
  assert bool((beam.topk_lens[:2] == 0).all())
  for kwargs in ({'beam_width': 33}, {'beam_width': 0}, {'token_beam': 17},
                 {'token_beam': 0}, {'blank_id': 5}, {'impl': 'hip'}):
    with pytest.raises(ValueError, match='ctc_beam_search'):
      ctc.ctc_beam_search(logits, lengths, **kwargs)
  with pytest.raises(TypeError, match='logit_lengths'):
    ctc.ctc_beam_search(logits, lengths.float())


# ---- the layer and the task --------------------------------------------------
def CheckDecoderWiring(device):
  from lingvo_amd.models import asr
  dec = asr.CtcDecoder.Params().Set(
      name='ctc', vocab_size=11, source_dim=6, dropout_prob=0.0,
      beam_impl='auto', beam_token_beam=3).Instantiate().to(device)
  dec.eval()
  g = torch.Generator().manual_seed(2)
  enc = torch.randn(3, 9, 6, generator=g).to(device)
  pad = (torch.arange(9)[None, :] >= torch.tensor([9, 4, 0])[:, None])
  pad = pad.float().to(device)
  with torch.no_grad():
    out = dec.BeamSearchDecode(dec.theta, enc, pad, num_hyps=4)
    want = ctc.ctc_beam_search(dec._Logits(dec.theta, enc).contiguous(),
                               torch.tensor([9, 4, 0]).to(device), 4, 3)
  assert sorted(out.keys()) == ['topk_ids', 'topk_lens', 'topk_scores']
  assert out.topk_ids.shape == (3, 4, 9)
  for key in out.keys():
    assert torch.equal(out[key], getattr(want, key)), key
  with pytest.raises(ValueError, match='length_norm'):
    dec.BeamSearchDecode(dec.theta, enc, pad, length_norm=1.0)


def CheckTaskDecode(device):
  import test_asr_ctc_model as mlib
  mp = mlib._TinyParams('asr.librispeech.Librispeech960ConformerSCtcBeam')
  assert mp.task.decoder.beam_impl == 'auto' and mp.task.decode_num_hyps == 8
  mp.task.decode_num_hyps = 4
  task = mp.Instantiate().GetTask().to(device)
  task.eval()
  batch = task.GetInputBatch()
  if device != 'cpu':
    batch = task.input_generator.ToDevice(batch, device)
  out = task.Decode(batch)
  assert out.topk_decoded.dtype == torch.long
  assert out.topk_decoded.shape == (4, 40)  # [B, T']: 160 frames / 4


def test_decoder_beam_search_is_the_op_on_its_logits():
  CheckDecoderWiring('cpu')


def test_task_decodes_with_four_hyps():
  CheckTaskDecode('cpu')
