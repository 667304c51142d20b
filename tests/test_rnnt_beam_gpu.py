"""Transducer beam search kernels (ops/hip/rnnt_beam.hip) against the fp64
twin that sees the same bf16 MFMA operands, then the decoder on the GPU."""

import functools

import pytest
import torch

from lingvo_amd.core.nested_map import NestedMap
from lingvo_amd.models import asr as asr_model
from lingvo_amd.ops import rnnt

gpu = pytest.mark.gpu

T = 6
# |topk_scores| tolerance: 4 x the largest difference between the twin run in
# fp32 and in fp64 (both with operand_dtype=bfloat16) over CASES, measured on
# the CPU with Measure() below: 6.04e-6 (case j1024_v1030). The kernels sum in
# fp32 like the fp32 twin, in another order.
SCORE_TOL = 4 * 6.04e-6
# The seeds are chosen so that, in the fp64 reference, every selection's gap
# between the last kept and the first dropped score and every live row's gap
# between its C-th and (C+1)-th logit is at least MARGIN (Measure() asserts
# it): no cut is decided by rounding.
MARGIN = 10 * SCORE_TOL

# name: (B, W, J, V, S, C, blank last, lengths, seed)
CASES = {
    'one_row_v3': (1, 1, 32, 3, 1, 8, False, [6], 1),
    'j96_v37': (3, 5, 96, 37, 3, 8, True, [6, 0, 4], 1),
    'j1024_v1030': (2, 32, 1024, 1030, 3, 8, False, [6, 3], 4),
    'j32_v1030_c1': (3, 5, 32, 1030, 1, 1, True, [4, 6, 0], 0),
    'full_beam_v3': (2, 32, 96, 3, 3, 8, True, [0, 6], 2),
    'j1024_v37_c1': (1, 1, 1024, 37, 3, 1, False, [6], 0),
}


def TablePred(table):
  """A prediction network that is exact in every dtype: the state is an
  index into `table` [N,J] that depends on the whole label history."""

  def Step(tok, states):
    idx = (states[0] * 31 + tok + 1) % table.shape[0]
    return table[idx], (idx,)

  return Step


@functools.lru_cache(maxsize=None)
def Case(name):
  """bf16-valued fp64 inputs on the CPU."""
  b, w, j, v, s, c, blank_last, lengths, seed = CASES[name]
  g = torch.Generator().manual_seed(seed)

  def Rand(*shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).bfloat16().double()

  return NestedMap(
      enc_p=Rand(b, T, j), table=Rand(64, j),
      joint_w=Rand(j, v, scale=3.0 / j**0.5), joint_b=Rand(v, scale=0.5),
      lengths=torch.tensor(lengths), w=w, c=c, s=s,
      blank=v - 1 if blank_last else 0)


def Twin(name, dtype, on_select=None):
  k = Case(name)
  return rnnt._TwinRnntBeam(
      k.enc_p.to(dtype), k.lengths, k.joint_w, k.joint_b, TablePred(k.table),
      (torch.zeros(k.enc_p.shape[0] * k.w, dtype=torch.long),), k.w, k.c, k.s,
      k.blank, operand_dtype=torch.bfloat16, on_select=on_select)


@functools.lru_cache(maxsize=None)
def Reference(name):
  return Twin(name, torch.float64)


def ScoreError(got, want):
  """Largest |score| difference; unused slots (-1e30 in either dtype) must
  be the same slots."""
  got, want = got.topk_scores.cpu().double(), want.topk_scores.cpu().double()
  live = want > -1e29
  assert torch.equal(got > -1e29, live)
  return float((got - want)[live].abs().max())


def Measure(name):
  """(fp32 twin against fp64 twin, smallest margin) of a case, on the CPU:
  how SCORE_TOL and the seeds were obtained."""
  gaps = []

  def OnSelect(kind, row, values, keep):
    del kind, row
    if len(values) > keep:
      gaps.append(float(values[keep - 1] - values[keep]))

  want = Twin(name, torch.float64, OnSelect)
  got = Twin(name, torch.float32)
  assert torch.equal(got.topk_ids, want.topk_ids)
  assert min(gaps) >= MARGIN, (name, min(gaps))
  return ScoreError(got, want), min(gaps)


@gpu
@pytest.mark.parametrize('name', list(CASES))
def test_kernels_match_fp64_twin(name):
  k, want = Case(name), Reference(name)

  def Run():
    return rnnt.rnnt_beam_search(
        k.enc_p.bfloat16().cuda(), k.lengths.cuda(),
        k.joint_w.bfloat16().cuda(),
        (k.joint_b.bfloat16() if k.blank else k.joint_b.float()).cuda(),
        TablePred(k.table.bfloat16().cuda()),
        (torch.zeros(k.enc_p.shape[0] * k.w, dtype=torch.long).cuda(),),
        beam_width=k.w, token_beam=k.c, max_symbols=k.s, blank_id=k.blank)

  got = Run()
  assert got.topk_scores.dtype == torch.float32
  assert torch.equal(got.topk_lens.cpu(), want.topk_lens)
  assert torch.equal(got.topk_ids.cpu(), want.topk_ids)
  assert torch.equal(got.valid.cpu().double(), want.valid)
  err = ScoreError(got, want)
  print(f'{name}: max |score - fp64 twin| = {err:.3e}')
  assert err <= SCORE_TOL
  for x, y in zip(got, Run()):
    assert torch.equal(x, y)


@gpu
def test_decoder_auto_matches_torch_on_the_gpu():
  torch.manual_seed(3)
  p = asr_model.TransducerDecoder.Params().Set(
      name='dec', vocab_size=37, emb_dim=16, rnn_cell_dim=32, source_dim=24,
      joint_dim=64, dropout_prob=0.0, beam_impl='auto', beam_token_beam=4,
      fprop_dtype=torch.bfloat16)
  dec = p.Instantiate().cuda()
  dec.eval()
  twin = p.Copy().Set(beam_impl='torch').Instantiate().cuda()
  twin.load_state_dict(dec.state_dict())
  twin.eval()
  enc = torch.randn(3, 5, 24, device='cuda')
  paddings = torch.tensor([[0, 0, 0, 0, 0], [0, 0, 0, 1, 1], [1, 1, 1, 1, 1]],
                          dtype=torch.float32, device='cuda')
  with torch.no_grad():
    got = dec.BeamSearchDecode(dec.theta, enc, paddings, num_hyps=4)
    want = twin.BeamSearchDecode(twin.theta, enc, paddings, num_hyps=4)
  assert torch.equal(got.topk_ids, want.topk_ids)
  assert torch.equal(got.topk_lens, want.topk_lens)
  assert bool((got.topk_lens[0] > 0).any())
  err = ScoreError(got, want)
  assert err <= SCORE_TOL, err
