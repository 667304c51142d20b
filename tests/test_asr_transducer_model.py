"""The transducer in the ASR task (CPU fp32): the TransducerDecoder configs
train, decode, serve and stream; an auxiliary CTC head beside it."""

import pytest
import torch

from lingvo_amd.core import registry
from lingvo_amd.core.nested_map import NestedMap
from lingvo_amd.models import asr as asr_lib

RNNT_S = 'asr.librispeech.Librispeech960ConformerSTransducer'
RNNT_L = 'asr.librispeech.Librispeech960WpmConformerLTransducer'


def _TinyParams(key=RNNT_S, seed=7):
  mp = registry.GetParams(key, 'Train')
  mp.task.fprop_dtype = torch.float32
  mp.task.train.bf16_weights = False
  mp.task.encoder.Set(num_layers=1, dropout_prob=0.0, specaug_tpl=None)
  mp.task.decoder.Set(dropout_prob=0.0, rnn_cell_dim=32, joint_dim=32,
                      emb_dim=16)
  mp.input.Set(batch_size=4, frame_len=160, target_len=6)
  mp.task.random_seed = seed
  return mp


def test_transducer_configs_are_registered():
  north = registry.GetParams(
      'asr.librispeech.Librispeech960WpmConformerL', 'Train')
  big = registry.GetParams(RNNT_L, 'Train')
  assert big.task.cls is asr_lib.AsrModel
  dec = big.task.decoder
  assert dec.cls is asr_lib.TransducerDecoder
  assert (dec.vocab_size, dec.emb_dim, dec.rnn_cell_dim, dec.num_lstm_layers,
          dec.joint_dim, dec.source_dim) == (1024, 128, 640, 1, 640, 512)
  assert dec.blank_id == 0 and dec.max_symbols_per_frame == 3
  assert dec.rnnt_impl == 'auto'
  assert big.task.encoder.ToText() == north.task.encoder.ToText()
  assert big.task.train.ToText() == north.task.train.ToText()
  assert big.input.ToText() == north.input.ToText()
  small = registry.GetParams(RNNT_S, 'Train')
  assert small.task.decoder.cls is asr_lib.TransducerDecoder
  assert small.task.decoder.source_dim == small.task.encoder.model_dim


def test_conformer_s_transducer_trains_cpu():
  mp = _TinyParams()
  # A constant rate on one batch: the config's 10k-step warm-up starts
  # near zero, where three steps move nothing.
  from lingvo_amd.core import schedule as schedule_lib
  mp.task.train.learner.Set(learning_rate=1e-3,
                            lr_schedule=schedule_lib.Constant.Params())
  task = mp.Instantiate().GetTask()
  batch = task.GetInputBatch()
  losses = []
  for _ in range(3):
    metrics = task.TrainStep(batch)
    losses.append(float(metrics['loss'][0].detach()))
    assert float(metrics['rnnt_valid_fraction'][0]) == 1.0
    assert float(metrics['loss'][1]) == 4.0
  print('ConformerSTransducer losses', losses)
  assert all(l == l and abs(l) != float('inf') for l in losses)
  assert losses[2] < losses[1] < losses[0], losses
  assert task.global_step == 3


# ---- greedy decode -----------------------------------------------------------
def _TextbookGreedy(dec, enc_b, num_frames):
  """Greedy transducer search for one utterance, frame by frame."""
  p = dec.p
  theta = dec.theta
  blank = torch.tensor([p.blank_id])
  states = dec._InitStates(1, enc_b.device)
  out, states = dec._PredictionStep(theta, blank, states)
  hyp = []
  for t in range(num_frames):
    enc_p = dec.enc_proj.FProp(theta.enc_proj, enc_b[None, t])
    for _ in range(p.max_symbols_per_frame):
      pred_p = dec.pred_proj.FProp(theta.pred_proj, out)
      tok = int(dec._Joint(theta, enc_p, pred_p).argmax(-1))
      if tok == p.blank_id:
        break
      hyp.append(tok)
      out, states = dec._PredictionStep(theta, torch.tensor([tok]), states)
  return hyp


def _SmallDecoder(max_symbols=3, bias_against_blank=0.0):
  dec = asr_lib.TransducerDecoder.Params().Set(
      name='rnnt', vocab_size=7, emb_dim=8, rnn_cell_dim=16,
      num_lstm_layers=2, source_dim=12, joint_dim=16, dropout_prob=0.0,
      max_symbols_per_frame=max_symbols, random_seed=5).Instantiate()
  dec.eval()
  with torch.no_grad():
    # Spread the logits, so that the argmax is far from a tie.
    dec.softmax.linear_w.mul_(8.0)
    dec.softmax.bias[0] -= bias_against_blank
  return dec


def test_greedy_decode_equals_the_per_utterance_loop():
  b, t = 5, 9
  lengths = [9, 9, 6, 3, 1]
  enc = 2.0 * torch.randn(b, t, 12, generator=torch.Generator().manual_seed(2))
  pad = (torch.arange(t)[None, :] >= torch.tensor(lengths)[:, None]).float()
  total = 0
  capped = False
  for max_symbols, against_blank in ((3, 0.0), (2, 50.0)):
    dec = _SmallDecoder(max_symbols, against_blank)
    with torch.no_grad():
      hyps = dec.GreedyDecode(dec.theta, enc, pad)
      assert hyps.shape == (b, t * max_symbols) and hyps.dtype == torch.long
      for i in range(b):
        want = _TextbookGreedy(dec, enc[i], lengths[i])
        total += len(want)
        capped = capped or len(want) == lengths[i] * max_symbols
        want = want + [0] * (t * max_symbols - len(want))
        assert hyps[i].tolist() == want, (i, hyps[i].tolist(), want)
  # The cases are not vacuous: labels were emitted, and with the blank
  # pushed down every frame of a row hit max_symbols_per_frame.
  assert total > 0 and capped


def test_greedy_decode_with_fusion_is_not_built():
  dec = _SmallDecoder()
  with pytest.raises(NotImplementedError):
    dec.GreedyDecode(dec.theta, torch.zeros(1, 3, 12), torch.zeros(1, 3),
                     fusion=object())


def test_compute_predictions_shape_and_history():
  dec = _SmallDecoder()
  ids = torch.tensor([[3, 4, 0], [1, 2, 5]])
  tgt = NestedMap(ids=ids, paddings=torch.tensor([[0., 0., 1.],
                                                  [0., 0., 0.]]))
  enc = torch.randn(2, 4, 12, generator=torch.Generator().manual_seed(1))
  with torch.no_grad():
    preds = dec.ComputePredictions(dec.theta, enc, torch.zeros(2, 4), tgt)
    assert preds.logits.shape == (2, 4, 4, 7)
    # Column u is conditioned on [blank, y_1..y_u] only.
    ids2 = ids.clone()
    ids2[:, 2] = 6
    preds2 = dec.ComputePredictions(
        dec.theta, enc, torch.zeros(2, 4),
        NestedMap(ids=ids2, paddings=tgt.paddings))
  assert torch.equal(preds.logits[:, :, :3], preds2.logits[:, :, :3])
  assert not torch.equal(preds.logits[:, :, 3], preds2.logits[:, :, 3])


# ---- the task ----------------------------------------------------------------
def test_transducer_decode_and_wer():
  task = _TinyParams().Instantiate().GetTask()
  task.eval()
  batch = task.GetInputBatch()
  out = task.Decode(batch)
  assert out.topk_decoded.dtype == torch.long
  assert out.topk_decoded.shape == (4, 40 * 3)  # [B, T' * max_symbols]
  dm = task.CreateDecoderMetrics()
  task.PostProcessDecodeOut(out, dm)
  assert dm.num_samples_in_batch.value == 4
  wer = dm.wer.value
  assert wer == wer and wer >= 0.0
  with torch.no_grad():
    served = task.Inference().default(batch.src.src_inputs,
                                      batch.src.paddings)
  assert torch.equal(served.hyps, out.topk_decoded)


def test_transducer_beam_decode_is_not_built():
  mp = _TinyParams()
  mp.task.decode_num_hyps = 2
  task = mp.Instantiate().GetTask()
  task.eval()
  with pytest.raises(NotImplementedError,
                     match='transducer beam search is not built'):
    task.Decode(task.GetInputBatch())


def test_aux_ctc_head_beside_the_transducer():
  mp = _TinyParams()
  mp.task.ctc_weight = 0.3
  mp.task.aux_ctc.dropout_prob = 0.0
  task = mp.Instantiate().GetTask()
  assert task.aux_ctc.p.vocab_size == mp.task.decoder.vocab_size
  assert task.aux_ctc.p.source_dim == mp.task.decoder.source_dim
  metrics, per_example = task.FProp(task.theta, task.GetInputBatch())
  for key in ('loss', 'att_loss', 'ctc_loss', 'ctc_valid_fraction',
              'rnnt_valid_fraction', 'log_pplx'):
    assert key in metrics, key
  got = float(metrics.loss[0].detach())
  want = 0.7 * float(metrics.att_loss[0]) + 0.3 * float(metrics.ctc_loss[0])
  assert got == got and abs(got) != float('inf')
  assert abs(got - want) <= 1e-6 * max(1.0, abs(want)), (got, want)
  assert per_example.per_example_ctc.shape == (4,)
  metrics.loss[0].backward()
  grads = {n: p.grad for n, p in task.named_parameters()}
  for head in ('aux_ctc.softmax.linear_w', 'decoder.softmax.linear_w',
               'decoder.pred_proj.w'):
    hits = [n for n in grads if n.endswith(head)]
    assert hits, (head, sorted(grads)[:5])
    assert grads[hits[0]] is not None
    assert float(grads[hits[0]].abs().max()) > 0, head


def test_streaming_recognizer_with_transducer_decoder_matches_offline():
  from lingvo_amd.layers import asr_frontend
  ep = asr_lib.ConformerEncoder.Params().Set(
      name='enc', input_dim=80, model_dim=32, num_layers=2, num_heads=2,
      kernel_size=4, dropout_prob=0.0, specaug_tpl=None, random_seed=13)
  ep.conformer_tpl.is_causal = True
  ep.conformer_tpl.conv_norm = 'layer'
  ep.conformer_tpl.atten_left_context = 64
  mp = asr_lib.AsrModel.Params().Set(
      name='m', encoder=ep, random_seed=13,
      decoder=asr_lib.TransducerDecoder.Params().Set(
          vocab_size=16, emb_dim=8, rnn_cell_dim=16, source_dim=32,
          joint_dim=16, dropout_prob=0.0))
  model = mp.Instantiate()
  model.eval()
  fe = asr_frontend.MelAsrFrontend.Params().Set(name='fe').Instantiate()
  wav = torch.randn(2, 16000, generator=torch.Generator().manual_seed(3))
  with torch.no_grad():
    mel, mel_pad = fe.FProp(fe.theta, wav, torch.zeros(2, 16000))
    enc, enc_pad = model.encoder.FProp(model.theta.encoder, mel, mel_pad)
    hyps_off = model.decoder.GreedyDecode(model.theta.decoder, enc, enc_pad)
  rec = asr_lib.StreamingRecognizer(model, fe, batch=2)
  for c0 in range(0, 16000, 3000):
    rec.Push(wav[:, c0:c0 + 3000])
  out = rec.Finish()
  assert out.hyps.shape == hyps_off.shape
  assert torch.equal(out.hyps, hyps_off)
