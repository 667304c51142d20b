"""CTC forced-alignment kernels (ctc_align in ops/hip/ctc.hip) against the
textbook float64 Viterbi of test_ctc_align_cpu.py, on the cases of
test_ctc_gpu.py; then CtcDecoder.Align on the GPU and graph capture.

The reference runs on the values after rounding to the kernel's input
dtype. With path64 the float64 sum of the reference log-probs along the
path the kernel RETURNED, and err_yard the largest score error of the
textbook's own float32 CPU run over the case's valid rows:

  bound = 2*err_yard + 2^-21*|ref_best|
  |score - path64|     <= bound      (the score is that of the path)
  ref_best - path64    <= 2*bound    (a path chosen on fp32 scores can lose
                                      the error of both compared paths)
  |token_logp - tok64| <= 2*err_yard + 2^-21*|tok64|   per label

fp32 inputs: frame_ids and spans equal the reference on every valid row
where the textbook's fp32 and fp64 runs pick the same path, and that is
every row of every case. bf16 inputs make exact float64 ties inside the
lattice (12 of the 14 rows of the five cases with L >= 31), so bf16 gets
the score and structural checks only.
"""

import functools

import pytest
import torch

from lingvo_amd.ops import ctc
import test_ctc_cpu as lib
import test_ctc_align_cpu as alib

gpu = pytest.mark.gpu

L_MAX = ctc.MAX_LABEL_LEN

_CASES = {
    'edge': lib.EdgeBatch,
    # S = 63 / 65: the backtrace stays inside one ballot word / crosses into
    # a second one.
    'l31_t70_v33': lambda: lib.RandomBatch(3, 70, 33, 31, 31, 3.0),
    'l32_t70_v33': lambda: lib.RandomBatch(3, 70, 33, 32, 32, 3.0),
    # Sharp distributions: many states are impossible in fp32.
    'l32_t70_v33_x20': lambda: lib.RandomBatch(3, 70, 33, 32, 32, 60.0),
    'l64_t300_v32': lambda: lib.RandomBatch(2, 300, 32, 64, 64, 3.0),
    # Odd V, so rows are not 16-byte aligned.
    'l140_t300_v77': lambda: lib.RandomBatch(2, 300, 77, 140, 140, 3.0),
    # T = 1023, S = 1023: 16 waves.
    'lmax_v8': lambda: lib.RandomBatch(1, 2 * L_MAX + 1, 8, L_MAX, 511, 3.0),
    'b130_t6_v1024_l2': lambda: lib.RandomBatch(130, 6, 1024, 2, 130, 3.0),
    # The backpointer masks live in LDS while T * waves * 16 bytes <= 48 KB:
    # 8 waves and T = 384 is the last shape that fits, T = 385 the first
    # that takes the global workspace (lmax_v8 is far past it).
    'l255_t384_v8': lambda: lib.RandomBatch(2, 384, 8, 255, 384, 3.0),
    'l255_t385_v8': lambda: lib.RandomBatch(2, 385, 8, 255, 385, 3.0),
}
_DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16}


@functools.lru_cache(maxsize=None)
def _Case(name, dtype_name):
  """The case's inputs rounded to the dtype, with reference and yardstick
  on exactly those values. Built once; callers must not modify it."""
  logits, tl, labels, ll = _CASES[name]()
  return alib.Case((logits.to(_DTYPES[dtype_name]).float(), tl, labels, ll))


def _RunGpu(batch, dtype, blank_id=0):
  logits, tl, labels, ll = batch
  return ctc.ctc_forced_align(logits.to('cuda', dtype), tl.cuda(),
                              labels.cuda(), ll.cuda(), blank_id=blank_id)


@gpu
@pytest.mark.parametrize('dtype_name', list(_DTYPES))
@pytest.mark.parametrize('name', list(_CASES))
def test_kernels_match_textbook_viterbi(name, dtype_name):
  case = _Case(name, dtype_name)
  dtype = _DTYPES[dtype_name]
  al = _RunGpu(case.batch, dtype)
  al2 = _RunGpu(case.batch, dtype)
  assert al.score.dtype == torch.float32
  assert al.token_logp.dtype == torch.float32
  assert al.valid.dtype == torch.float32
  for x in (al.frame_ids, al.token_start, al.token_end):
    assert x.dtype == torch.long
  b, t = case.batch[0].shape[:2]
  l = case.batch[2].shape[1]
  assert al.frame_ids.shape == (b, t) and al.token_logp.shape == (b, l)
  got = alib.ToCpu64(al)
  assert torch.equal(got['valid'], case.want['valid'])
  for x, y in zip(al, al2):
    assert torch.equal(x, y)
  alib.CheckFills(got, case)
  alib.CheckScores(got, case, f'{name} {dtype_name}')
  if dtype_name == 'fp32':
    assert case.agree == case.valid_rows  # no row is excluded
    alib.CheckEqualsReference(got, case, case.agree)
  # The same arithmetic with the masks forced into the global workspace.
  from lingvo_amd.ops import _loader
  logits, tl, labels, ll = case.batch
  forced = _loader.get_ext(required=True).ctc_align(
      logits.to('cuda', dtype), tl.cuda(), labels.cuda(), ll.cuda(), 0, False)
  for x, y in zip(al, forced):
    assert torch.equal(x, y)


@gpu
@pytest.mark.parametrize('dtype_name', list(_DTYPES))
def test_bad_labels_are_invalid_rows(dtype_name):
  case = alib.Case(lib.BadLabelBatch())
  assert case.valid_rows == []
  got = alib.ToCpu64(_RunGpu(case.batch, _DTYPES[dtype_name]))
  assert got['valid'].tolist() == [0, 0]
  alib.CheckFills(got, case)
  assert bool((got['token_start'] == -1).all())
  assert bool((got['token_end'] == -1).all())
  assert bool((got['token_logp'] == 0).all())


@gpu
def test_host_guards_raise_before_launch():
  from lingvo_amd.ops import _loader
  ext = _loader.get_ext(required=True)
  logits, tl, labels, ll = (x.cuda() for x in lib.EdgeBatch())
  with pytest.raises(RuntimeError):
    ext.ctc_align(logits.half(), tl, labels, ll, 0, True)
  with pytest.raises(RuntimeError):
    ext.ctc_align(logits.transpose(0, 1), tl, labels, ll, 0, True)
  with pytest.raises(RuntimeError):
    ext.ctc_align(logits, tl, labels, ll, 5, True)
  with pytest.raises(RuntimeError):
    ext.ctc_align(logits, tl.int(), labels, ll, 0, True)
  with pytest.raises(RuntimeError):
    ext.ctc_align(logits, tl, labels[:5], ll, 0, True)
  wide = torch.ones(6, L_MAX + 1, dtype=torch.long, device='cuda')
  with pytest.raises(RuntimeError, match='limit'):
    ext.ctc_align(logits, tl, wide, ll, 0, True)
  with pytest.raises(TypeError, match='ctc_forced_align'):
    ctc.ctc_forced_align(logits.half(), tl, labels, ll)
  torch.cuda.synchronize()


# ---- the layer ---------------------------------------------------------------
@gpu
def test_ctc_decoder_align_bf16_matches_cpu_fp32():
  """Project layer bound: 0.05 scaled by max(1, |want|)
  (test_ctc_gpu.py); spans are equal on the identity-logits input."""
  import torch.nn.functional as F
  v = 6
  ref = alib.DecoderWithIdentityLogits(v)
  p = ref.p.Copy()
  p.fprop_dtype = torch.bfloat16
  layer = p.Instantiate()
  layer.load_state_dict(ref.state_dict())
  layer = layer.to('cuda').to(torch.bfloat16)
  layer.eval()
  enc = F.one_hot(torch.tensor(alib.IDENTITY_FRAMES), v).float() * 5.0
  pad = (torch.arange(8)[None, :] >=
         torch.tensor(alib.IDENTITY_LENGTHS)[:, None]).float()
  tgt = alib.IdentityTargets()
  want = ref.Align(ref.theta, enc, pad, tgt)
  got = layer.Align(layer.theta, enc.cuda().bfloat16(), pad.cuda(),
                    tgt.Transform(lambda x: x.cuda()))
  alib.CheckIdentitySpans(want)
  alib.CheckIdentitySpans(got)
  errs = {}
  for name in ('score', 'token_logp'):
    scale = max(1.0, float(want[name].abs().max()))
    errs[name] = float(
        (got[name].float().cpu() - want[name]).abs().max()) / scale
  print('ctc align layer bf16 vs cpu fp32: ' + ' '.join(
      f'{k}={e:.4g}' for k, e in errs.items()))
  for name, e in errs.items():
    assert e < 0.05, (name, e)


# ---- graph capture ------------------------------------------------------------
@gpu
def test_graph_captured_align_matches_eager():
  """Two launches, no host sync, every output element written: a captured
  ctc_forced_align replayed on refreshed inputs equals the eager call."""
  first = _Case('l32_t70_v33', 'fp32').batch
  second = _Case('l32_t70_v33_x20', 'fp32').batch  # same shapes and labels
  static = [x.cuda() for x in first]
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    ctc.ctc_forced_align(*static)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    captured = ctc.ctc_forced_align(*static)
  for batch in (second, first):
    for dst, src in zip(static, batch):
      dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    eager = ctc.ctc_forced_align(*(x.cuda() for x in batch))
    for name, x, y in zip(alib.FIELDS, captured, eager):
      assert torch.equal(x, y), name
  assert bool((captured.valid == 1).all())
