"""CTC prefix beam search kernels (ops/hip/ctc_beam.hip) against the cases
and fp64 references of test_ctc_beam_cpu.py, then bf16 against fp32, the
layer wiring on the GPU, and replay under graph capture."""

import pytest
import torch

from lingvo_amd.ops import ctc
import test_ctc_beam_cpu as blib

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize('blank_last', [False, True])
@pytest.mark.parametrize('name', list(blib.EXHAUSTIVE))
def test_kernels_sum_every_alignment(name, blank_last):
  blank = blib.EXHAUSTIVE[name][0] - 1 if blank_last else 0
  logits, lengths, c, want = blib.ExhaustiveCase(name, blank)
  got = ctc.ctc_beam_search(logits.float().cuda(), lengths.cuda(), 32, c,
                            blank)
  assert got.topk_scores.dtype == torch.float32
  assert got.topk_ids.dtype == got.topk_lens.dtype == torch.long
  # The case's fp64 logits are fp32 values, so both sides see the same.
  blib.CheckExhaustive(got, want, blib.SCORE_TOL)


@gpu
@pytest.mark.parametrize('name', list(blib.PRUNED))
def test_kernels_match_fp64_reference(name):
  logits, lengths, w, c, _, _ = blib.PrunedCase(name)
  got = ctc.ctc_beam_search(logits.cuda(), lengths.cuda(), w, c)
  blib.CheckPruned(got, name)
  again = ctc.ctc_beam_search(logits.cuda(), lengths.cuda(), w, c)
  for x, y in zip(got, again):
    assert torch.equal(x, y)


@gpu
@pytest.mark.parametrize('v', [17, 77, 1030])  # odd, odd, not a multiple of 8
def test_bf16_logits_give_the_bits_of_their_fp32_values(v):
  g = torch.Generator().manual_seed(v)
  logits = (torch.randn(5, 19, v, generator=g) * 4.0).bfloat16().cuda()
  lengths = torch.tensor([19, 0, 7, 18, 19]).cuda()
  low = ctc.ctc_beam_search(logits, lengths, 8, 8)
  full = ctc.ctc_beam_search(logits.float(), lengths, 8, 8)
  for x, y in zip(low, full):
    assert torch.equal(x, y)
  assert bool((low.topk_lens[0] > 0).any())


@gpu
def test_layer_and_task_on_the_gpu():
  blib.CheckDecoderWiring('cuda')
  blib.CheckTaskDecode('cuda')


@gpu
def test_graph_captured_search_matches_eager():
  first, lengths, w, c, _, _ = blib.PrunedCase('t16_v24_w4_c4')
  second = first.flip(0)
  static = first.cuda()
  lengths = lengths.cuda()
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    ctc.ctc_beam_search(static, lengths, w, c)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    captured = ctc.ctc_beam_search(static, lengths, w, c)
  for logits in (second, first, second):
    static.copy_(logits)
    graph.replay()
    torch.cuda.synchronize()
    eager = ctc.ctc_beam_search(logits.cuda(), lengths, w, c)
    for x, y in zip(captured, eager):
      assert torch.equal(x, y)
