"""CTC forced alignment (ops/ctc.ctc_forced_align) on CPU: the torch twin
against a textbook per-row Viterbi in float64, hand-checkable alignments,
structural properties, wrapper guards, CtcDecoder.Align, AsrModel.Align and
the `align` inference subgraph. Also holds the reference and the checks
that test_ctc_align_gpu.py shares.

The reference knows nothing of ops/ctc.py: torch.log_softmax in a chosen
dtype, a Python loop over frames with numpy over lattice positions, -inf
for "impossible", and the tie rule of the op (among equal predecessors the
smallest jump; of the two end positions the last label on a tie). Run in
float64 it is the reference; run in float32 it is the error yardstick:

  bound = 2*err_yard + 2^-21*|ref|

where err_yard is the largest |score32 - score64| of the textbook over the
case's valid rows (the nll rule of test_ctc_gpu.py).
"""

import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from lingvo_amd.ops import ctc
import test_ctc_cpu as lib

Row = collections.namedtuple('Row', 'valid score path')
FIELDS = ('frame_ids', 'token_start', 'token_end', 'token_logp', 'score',
          'valid')


# ---- the textbook reference ---------------------------------------------------
def _RowInputs(batch, b, blank_id):
  """(T_b, labels of row b) or None when the row breaks a length or
  label-range rule."""
  logits, tl, labels, ll = batch
  t, v = logits.shape[1], logits.shape[2]
  tb, lb = int(tl[b]), int(ll[b])
  if not (1 <= tb <= t and 0 <= lb <= labels.shape[1]):
    return None
  lab = [int(x) for x in labels[b, :lb]]
  if any(x < 0 or x >= v or x == blank_id for x in lab):
    return None
  return tb, lab


def LogProbs(batch, b, tb, dtype):
  return torch.log_softmax(batch[0][b, :tb].to(dtype), dim=-1).numpy()


def Textbook(batch, dtype, blank_id=0):
  """Per-row Viterbi over the blank-interleaved labels in `dtype` -> a list
  of Row(valid, score, path): path[t] is the lattice position of frame t."""
  rows = []
  for b in range(batch[0].shape[0]):
    inputs = _RowInputs(batch, b, blank_id)
    if inputs is None:
      rows.append(Row(False, 0.0, None))
      continue
    tb, lab = inputs
    ext = [blank_id]
    for x in lab:
      ext += [x, blank_id]
    ext = np.array(ext)
    s = len(ext)
    e = LogProbs(batch, b, tb, dtype)[:, ext]  # [T_b, S]
    skip = np.zeros(s, dtype=bool)
    skip[2:] = (np.arange(2, s) % 2 == 1) & (ext[2:] != ext[:-2])
    ninf = np.array(-np.inf, dtype=e.dtype)
    a = np.full(s, ninf)
    a[:2] = e[0, :2]
    bp = np.zeros((tb, s), dtype=np.int64)
    for t in range(1, tb):
      p1 = np.concatenate([[ninf], a[:-1]])
      p2 = np.where(skip, np.concatenate([[ninf, ninf], a[:-2]])[:s], ninf)
      m, mv = a, np.zeros(s, dtype=np.int64)
      for jump, cand in ((1, p1), (2, p2)):
        take = cand > m  # strictly: the smallest jump wins a tie
        m = np.where(take, cand, m)
        mv = np.where(take, jump, mv)
      a = e[t] + m
      bp[t] = mv
    at = s - 1 if s == 1 or a[s - 1] >= a[s - 2] else s - 2
    score = float(a[at])
    if not np.isfinite(score):
      rows.append(Row(False, 0.0, None))
      continue
    path = np.zeros(tb, dtype=np.int64)
    for t in range(tb - 1, -1, -1):
      path[t] = at
      at -= bp[t, at]
    assert path[0] in (0, 1)
    rows.append(Row(True, score, path))
  return rows


def Expected(batch, rows, blank_id=0):
  """The six outputs in float64 that follow from the reference rows, with
  the defined fill values everywhere else."""
  logits, _, labels, _ = batch
  b, t = logits.shape[:2]
  l = labels.shape[1]
  out = dict(frame_ids=torch.full((b, t), -1, dtype=torch.long),
             token_start=torch.full((b, l), -1, dtype=torch.long),
             token_end=torch.full((b, l), -1, dtype=torch.long),
             token_logp=torch.zeros(b, l, dtype=torch.float64),
             score=torch.zeros(b, dtype=torch.float64),
             valid=torch.zeros(b, dtype=torch.float64))
  for i, row in enumerate(rows):
    if not row.valid:
      continue
    tb = len(row.path)
    lp = LogProbs(batch, i, tb, torch.float64)
    out['valid'][i] = 1.0
    out['score'][i] = row.score
    for f, s in enumerate(row.path):
      if s % 2 == 0:
        out['frame_ids'][i, f] = blank_id
        continue
      j = (s - 1) // 2
      tok = int(labels[i, j])
      out['frame_ids'][i, f] = tok
      if out['token_start'][i, j] < 0:
        out['token_start'][i, j] = f
      out['token_end'][i, j] = f + 1
      out['token_logp'][i, j] += float(lp[f, tok])
  return out


class Case:
  """A batch with its float64 reference and float32 yardstick. Build once
  per case; nothing here is modified afterwards."""

  def __init__(self, batch, blank_id=0):
    self.batch = batch
    self.blank_id = blank_id
    self.rows64 = Textbook(batch, torch.float64, blank_id)
    self.rows32 = Textbook(batch, torch.float32, blank_id)
    self.want = Expected(batch, self.rows64, blank_id)
    self.valid_rows = [i for i, r in enumerate(self.rows64) if r.valid]
    assert [r.valid for r in self.rows32] == [r.valid for r in self.rows64]
    self.err_yard = max(
        [abs(self.rows32[i].score - self.rows64[i].score)
         for i in self.valid_rows] or [0.0])
    # Rows where the textbook's own fp32 and fp64 runs pick one path.
    self.agree = [i for i in self.valid_rows if
                  np.array_equal(self.rows32[i].path, self.rows64[i].path)]

  def Bound(self, ref):
    return 2 * self.err_yard + 2.0**-21 * ref.abs()


def ToCpu64(al):
  """CtcAlignment -> dict of CPU tensors, floats in float64."""
  out = {}
  for name in FIELDS:
    x = getattr(al, name).detach().cpu()
    out[name] = x.double() if x.is_floating_point() else x
  return out


def Collapse(frames, blank):
  out, prev = [], None
  for tok in frames:
    if tok != prev and tok != blank:
      out.append(tok)
    prev = tok
  return out


def CheckFills(got, case):
  """Invalid rows, padded frames and unused label slots hold the defined
  values, whichever path the valid rows took."""
  logits, tl, labels, ll = case.batch
  for i, row in enumerate(case.rows64):
    if not row.valid:
      assert float(got['valid'][i]) == 0.0 and float(got['score'][i]) == 0.0
      assert bool((got['frame_ids'][i] == -1).all()), i
      tb, lb = 0, 0
    else:
      tb, lb = int(tl[i]), int(ll[i])
    assert bool((got['frame_ids'][i, tb:] == -1).all()), i
    assert bool((got['frame_ids'][i, :tb] >= 0).all()), i
    assert bool((got['token_start'][i, lb:] == -1).all()), i
    assert bool((got['token_end'][i, lb:] == -1).all()), i
    assert bool((got['token_logp'][i, lb:] == 0).all()), i


def PathSums(got, case):
  """In float64, from the reference log-probs: (path64 [B], the sum along
  the returned frame_ids; tok64 [B,L], the sum over each returned span)."""
  logits, tl, labels, ll = case.batch
  path64 = torch.zeros(logits.shape[0], dtype=torch.float64)
  tok64 = torch.zeros(labels.shape, dtype=torch.float64)
  for i in case.valid_rows:
    tb, lb = int(tl[i]), int(ll[i])
    lp = LogProbs(case.batch, i, tb, torch.float64)
    ids = got['frame_ids'][i, :tb].numpy()
    path64[i] = float(lp[np.arange(tb), ids].sum())
    for j in range(lb):
      lo, hi = int(got['token_start'][i, j]), int(got['token_end'][i, j])
      tok64[i, j] = float(lp[lo:hi, int(labels[i, j])].sum())
  return path64, tok64


def CheckStructure(got, case):
  """On every valid row: frame_ids collapse to the labels, spans are
  increasing, disjoint and cover exactly the label's frames. Returns
  PathSums for the score checks."""
  logits, tl, labels, ll = case.batch
  for i in case.valid_rows:
    tb, lb = int(tl[i]), int(ll[i])
    ids = got['frame_ids'][i, :tb].tolist()
    lab = labels[i, :lb].tolist()
    assert Collapse(ids, case.blank_id) == lab, i
    prev_end = 0
    for j in range(lb):
      lo, hi = int(got['token_start'][i, j]), int(got['token_end'][i, j])
      assert prev_end <= lo < hi <= tb, (i, j, lo, hi)
      assert ids[lo:hi] == [lab[j]] * (hi - lo), (i, j)
      # A repeat of the previous label needs a blank in between.
      if j and lab[j] == lab[j - 1]:
        assert lo > prev_end, (i, j)
      prev_end = hi
    assert sum(x != case.blank_id for x in ids) == sum(
        int(got['token_end'][i, j]) - int(got['token_start'][i, j])
        for j in range(lb)), i
  return PathSums(got, case)


def CheckScores(got, case, tag):
  """score and token_logp against the float64 sums along the returned
  path, and the returned path's optimality, by the module's bound. Prints
  the figures before it asserts."""
  path64, tok64 = CheckStructure(got, case)
  v = case.valid_rows
  ref_best = case.want['score']
  bound = case.Bound(ref_best)
  score_err = (got['score'] - path64).abs()
  gap = ref_best - path64
  tok_err = (got['token_logp'] - tok64).abs()
  tok_bound = case.Bound(tok64)
  print(f'ctc align {tag}: valid {len(v)}/{len(case.rows64)} '
        f'yard {case.err_yard:.3g} |ref| max '
        f'{float(ref_best.abs().max()):.4g} '
        f'score err {float(score_err[v].max()) if v else 0:.3g} '
        f'gap {float(gap[v].max()) if v else 0:.3g} '
        f'(bound {float(bound[v].min()) if v else 0:.3g}) '
        f'token err {float(tok_err[v].max()) if v else 0:.3g} '
        f'(bound >= {float(tok_bound[v].min()) if v else 0:.3g}) '
        f'fp32/fp64 paths agree {len(case.agree)}/{len(v)}')
  assert bool((score_err[v] <= bound[v]).all()), (score_err, bound)
  assert bool((gap[v] <= 2 * bound[v]).all()), (gap, bound)
  assert bool((tok_err[v] <= tok_bound[v]).all()), (
      float((tok_err[v] - tok_bound[v]).max()))


def CheckEqualsReference(got, case, rows):
  for name in ('frame_ids', 'token_start', 'token_end'):
    assert torch.equal(got[name][rows], case.want[name][rows]), name


# ---- the twin against the reference -------------------------------------------
_CASES = {
    'edge': lib.EdgeBatch,
    'l31_t70_v33': lambda: lib.RandomBatch(3, 70, 33, 31, 31, 3.0),
    'l32_t70_v33': lambda: lib.RandomBatch(3, 70, 33, 32, 32, 3.0),
}
_BUILT = {}


def _Case(name):
  if name not in _BUILT:
    _BUILT[name] = Case(_CASES[name]())
  return _BUILT[name]


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32],
                         ids=['fp64', 'fp32'])
@pytest.mark.parametrize('name', list(_CASES))
def test_twin_matches_textbook_viterbi(name, dtype):
  case = _Case(name)
  logits, tl, labels, ll = case.batch
  al = ctc.ctc_forced_align(logits.to(dtype), tl, labels, ll)
  assert isinstance(al, ctc.CtcAlignment)
  assert al.score.dtype == dtype and al.token_logp.dtype == dtype
  assert al.valid.dtype == dtype and al.frame_ids.dtype == torch.long
  assert al.token_start.dtype == torch.long
  assert al.token_end.dtype == torch.long
  got = ToCpu64(al)
  assert torch.equal(got['valid'], case.want['valid'])
  CheckFills(got, case)
  # Exact wherever the textbook's own fp32 and fp64 runs pick one path
  # (a condition of the reference alone), and that is every valid row.
  assert case.agree == case.valid_rows
  CheckEqualsReference(got, case, case.agree)
  CheckScores(got, case, f'{name} twin {str(dtype)[6:]}')
  err = (got['score'] - case.want['score']).abs()
  assert bool((err <= case.Bound(case.want['score'])).all())
  err = (got['token_logp'] - case.want['token_logp']).abs()
  assert bool((err <= case.Bound(case.want['token_logp'])).all())
  if name == 'edge':
    assert got['valid'].tolist() == [1, 1, 0, 1, 1, 1]
    assert got['frame_ids'][2].tolist() == [-1] * 9          # no alignment
    assert got['frame_ids'][4].tolist() == [0] * 3 + [-1] * 6  # empty target
    assert got['token_start'][4].tolist() == [-1] * 4
    # T = L: every frame is its label.
    assert got['frame_ids'][5].tolist() == [4, 3, 4, 3] + [-1] * 5
    assert got['token_start'][5].tolist() == [0, 1, 2, 3]
    assert got['token_end'][5].tolist() == [1, 2, 3, 4]


def test_impl_torch_is_the_twin():
  logits, tl, labels, ll = lib.EdgeBatch()
  a = ctc.ctc_forced_align(logits, tl, labels, ll, impl='auto')
  b = ctc.ctc_forced_align(logits, tl, labels, ll, impl='torch')
  for x, y in zip(a, b):
    assert torch.equal(x, y)


def test_outputs_carry_no_gradient():
  logits, tl, labels, ll = lib.EdgeBatch()
  al = ctc.ctc_forced_align(logits.clone().requires_grad_(True), tl, labels,
                            ll)
  assert not any(x.requires_grad for x in al)


# ---- hand-checkable alignments ------------------------------------------------
def _OneHot(frames, v):
  return F.one_hot(torch.tensor(frames), v).float() * 5.0


def _HotLogp(v):
  return 5.0 - float(torch.logsumexp(
      torch.tensor([5.0] + [0.0] * (v - 1), dtype=torch.float64), 0))


def test_hand_checkable_alignments():
  v = 6
  frames = [[1, 1, 0, 1, 2, 2, 3, 0],   # repeat split by a blank
            [2, 0, 3, 3, 5, 5, 5, 5]]   # last four frames are padding
  labels = torch.tensor([[1, 1, 2, 3], [2, 3, 0, 0]])
  al = ctc.ctc_forced_align(_OneHot(frames, v), torch.tensor([8, 4]), labels,
                            torch.tensor([4, 2]))
  assert al.valid.tolist() == [1, 1]
  assert al.frame_ids[0].tolist() == frames[0]
  assert al.token_start[0].tolist() == [0, 3, 4, 6]
  assert al.token_end[0].tolist() == [2, 4, 6, 7]
  assert al.frame_ids[1].tolist() == [2, 0, 3, 3, -1, -1, -1, -1]
  assert al.token_start[1].tolist() == [0, 2, -1, -1]
  assert al.token_end[1].tolist() == [1, 4, -1, -1]
  hot = _HotLogp(v)
  want_logp = torch.tensor([[2 * hot, hot, 2 * hot, hot],
                            [hot, 2 * hot, 0.0, 0.0]])
  assert float((al.token_logp - want_logp).abs().max()) < 1e-5
  want_score = torch.tensor([8 * hot, 4 * hot])
  assert float((al.score - want_score).abs().max()) < 1e-5


def test_hand_checkable_nonzero_blank():
  v = 6
  frames = [[5, 1, 1, 5, 2]]
  al = ctc.ctc_forced_align(_OneHot(frames, v), torch.tensor([5]),
                            torch.tensor([[1, 2]]), torch.tensor([2]),
                            blank_id=5)
  assert al.valid.tolist() == [1]
  assert al.frame_ids[0].tolist() == frames[0]
  assert al.token_start[0].tolist() == [1, 4]
  assert al.token_end[0].tolist() == [3, 5]
  assert abs(float(al.score[0]) - 5 * _HotLogp(v)) < 1e-5


def test_nonzero_blank_matches_textbook():
  logits, tl, labels, ll = lib.RandomBatch(3, 10, 6, 3, 21)
  case = Case((logits, tl, labels.clamp(max=4), ll), blank_id=5)
  got = ToCpu64(ctc.ctc_forced_align(logits.double(), tl, case.batch[2], ll,
                                     blank_id=5))
  assert torch.equal(got['valid'], case.want['valid'])
  CheckFills(got, case)
  CheckEqualsReference(got, case, slice(None))
  CheckScores(got, case, 'blank5 twin fp64')


# ---- invalid rows and guards --------------------------------------------------
@pytest.mark.parametrize('impl', ['auto', 'torch'])
def test_bad_labels_are_invalid_rows(impl):
  case = Case(lib.BadLabelBatch())
  assert case.valid_rows == []
  got = ToCpu64(ctc.ctc_forced_align(*case.batch, impl=impl))
  assert got['valid'].tolist() == [0, 0]
  CheckFills(got, case)
  assert bool((got['token_logp'] == 0).all())
  assert bool((got['token_start'] == -1).all())


def test_wrapper_guards():
  logits, tl, labels, ll = lib.EdgeBatch()
  align = ctc.ctc_forced_align
  with pytest.raises(ValueError, match='ctc_forced_align'):
    align(logits[0], tl, labels, ll)                       # logits rank
  with pytest.raises(TypeError, match='ctc_forced_align'):
    align(logits, tl, labels[0], ll)                       # labels rank
  with pytest.raises(TypeError, match='ctc_forced_align'):
    align(logits, tl[:, None], labels, ll)                 # lengths rank
  with pytest.raises(TypeError):
    align(logits.long(), tl, labels, ll)                   # logits dtype
  with pytest.raises(TypeError):
    align(logits, tl, labels.int(), ll)                    # labels dtype
  with pytest.raises(TypeError):
    align(logits, tl.float(), labels, ll)                  # lengths dtype
  with pytest.raises(ValueError):
    align(logits.transpose(0, 1), tl, labels, ll)          # not contiguous
  for blank in (-1, 5):
    with pytest.raises(ValueError):
      align(logits, tl, labels, ll, blank_id=blank)
  with pytest.raises(ValueError):
    align(logits.to('meta'), tl, labels, ll)               # devices differ
  wide = torch.ones(6, ctc.MAX_LABEL_LEN + 1, dtype=torch.long)
  with pytest.raises(ValueError, match='limit'):
    align(logits, tl, wide, ll)                            # L over the limit
  with pytest.raises(ValueError, match='impl'):
    align(logits, tl, labels, ll, impl='cudnn')
  at_limit = torch.ones(6, ctc.MAX_LABEL_LEN, dtype=torch.long)
  assert align(logits, tl, at_limit, ll).token_start.shape == (
      6, ctc.MAX_LABEL_LEN)


# ---- CtcDecoder.Align ---------------------------------------------------------
def DecoderWithIdentityLogits(v, **kwargs):
  from lingvo_amd.models import asr
  dec = asr.CtcDecoder.Params().Set(
      name='ctc', vocab_size=v, source_dim=v, dropout_prob=0.0,
      **kwargs).Instantiate()
  dec.eval()
  with torch.no_grad():
    dec.softmax.linear_w.copy_(torch.eye(v))
    dec.softmax.bias.zero_()
  return dec


IDENTITY_FRAMES = [[1, 1, 0, 1, 2, 2, 3, 0],
                   [2, 0, 3, 3, 5, 5, 5, 5]]
IDENTITY_LENGTHS = [8, 4]


def IdentityTargets():
  from lingvo_amd.core.nested_map import NestedMap
  return NestedMap(ids=torch.tensor([[1, 1, 2, 3], [2, 3, 0, 0]]),
                   paddings=torch.tensor([[0., 0., 0., 0.],
                                          [0., 0., 1., 1.]]))


def CheckIdentitySpans(out):
  assert out.valid.tolist() == [1, 1]
  assert out.frame_ids.cpu().tolist() == [[1, 1, 0, 1, 2, 2, 3, 0],
                                          [2, 0, 3, 3, -1, -1, -1, -1]]
  assert out.token_start.cpu().tolist() == [[0, 3, 4, 6], [0, 2, -1, -1]]
  assert out.token_end.cpu().tolist() == [[2, 4, 6, 7], [1, 4, -1, -1]]


@pytest.mark.parametrize('impl', ['auto', 'torch'])
def test_ctc_decoder_align(impl):
  v = 6
  dec = DecoderWithIdentityLogits(v, align_impl=impl)
  enc = _OneHot(IDENTITY_FRAMES, v)
  pad = (torch.arange(8)[None, :] >=
         torch.tensor(IDENTITY_LENGTHS)[:, None]).float()
  out = dec.Align(dec.theta, enc, pad, IdentityTargets())
  assert sorted(out.keys()) == sorted(FIELDS)
  CheckIdentitySpans(out)
  assert abs(float(out.score[0]) - 8 * _HotLogp(v)) < 1e-5
  assert not out.score.requires_grad


# ---- AsrModel.Align and the subgraph ------------------------------------------
def _TinyParams(key='asr.librispeech.Librispeech960ConformerSCtc', seed=7):
  from lingvo_amd.core import registry
  mp = registry.GetParams(key, 'Train')
  mp.task.fprop_dtype = torch.float32
  mp.task.train.bf16_weights = False
  mp.task.encoder.Set(num_layers=1, dropout_prob=0.0, specaug_tpl=None)
  mp.input.Set(batch_size=4, frame_len=160, target_len=6)
  mp.task.random_seed = seed
  return mp


def _TinyAttentionParams(ctc_weight):
  mp = _TinyParams('asr.librispeech.Librispeech960ConformerS')
  mp.task.decoder.Set(rnn_cell_dim=32, emb_dim=16)
  mp.task.ctc_weight = ctc_weight
  return mp


def _CheckModelAlignment(task, batch, out):
  from lingvo_amd.core import py_utils
  b, l = batch.tgt.ids.shape
  assert out.frame_ids.shape == (b, 40)  # [B, T']: 160 frames / 4
  assert out.token_start.shape == (b, l) and out.score.shape == (b,)
  assert out.valid.tolist() == [1.0] * b
  lengths = py_utils.LengthsFromPaddings(batch.tgt.paddings)
  for i in range(b):
    n = int(lengths[i])
    frames = [x for x in out.frame_ids[i].tolist() if x >= 0]  # unpadded
    assert Collapse(frames, 0) == batch.tgt.ids[i, :n].tolist(), i
    assert bool((out.token_end[i, :n] > out.token_start[i, :n]).all())
  assert not any(x.requires_grad for x in out.Flatten())


def test_asr_model_align_and_subgraph_agree():
  task = _TinyParams().Instantiate().GetTask()
  task.eval()
  batch = task.GetInputBatch()
  out = task.Align(batch)
  _CheckModelAlignment(task, batch, out)
  subgraphs = task.Inference()
  assert sorted(subgraphs.keys()) == ['align', 'default', 'encode']
  with torch.no_grad():
    served = subgraphs.align(batch.src.src_inputs, batch.src.paddings,
                             batch.tgt.ids, batch.tgt.paddings)
  for name in FIELDS:
    assert torch.equal(served[name], out[name]), name


def test_attention_model_has_no_align():
  task = _TinyAttentionParams(0.0).Instantiate().GetTask()
  task.eval()
  assert sorted(task.Inference().keys()) == ['default', 'encode']
  with pytest.raises(ValueError, match='CtcDecoder.*ctc_weight'):
    task.Align(task.GetInputBatch())


def test_joint_model_aligns_through_aux_ctc():
  task = _TinyAttentionParams(0.3).Instantiate().GetTask()
  task.eval()
  batch = task.GetInputBatch()
  out = task.Align(batch)
  _CheckModelAlignment(task, batch, out)
  assert 'align' in task.Inference()
  with torch.no_grad():
    enc, enc_pad = task.encoder.FProp(
        task.theta.encoder, batch.src.src_inputs, batch.src.paddings)
    want = task.aux_ctc.Align(task.theta.aux_ctc, enc, enc_pad, batch.tgt)
  assert torch.equal(out.frame_ids, want.frame_ids)


def test_predictor_serves_align(tmp_path):
  from lingvo_amd.runtime import inference
  mp = _TinyParams()
  path = inference.InferenceGraphExporter.Export(
      mp, str(tmp_path / 'ctc_bundle.pt'))
  pred = inference.Predictor(path, device='cpu')
  assert 'align' in pred.subgraphs
  task = mp.Instantiate().GetTask()
  batch = task.GetInputBatch()
  out = pred.Run('align', src_inputs=batch.src.src_inputs,
                 paddings=batch.src.paddings, tgt_ids=batch.tgt.ids,
                 tgt_paddings=batch.tgt.paddings)
  assert out.frame_ids.shape == (4, 40)
  assert out.valid.tolist() == [1.0] * 4
