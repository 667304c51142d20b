"""Registered Librispeech ASR params (reference
lingvo/tasks/asr/params/librispeech.py:28-310).

Librispeech960WpmConformerL is the BASELINE.json north-star config:
Conformer-L per the Conformer paper (17 blocks, d=512, h=8, conv kernel
32) with an attention LSTM decoder, bf16 compute, synthetic 80-dim
features (no network for the real corpus)."""

from __future__ import annotations

import torch

from lingvo_amd.core import learner as learner_lib
from lingvo_amd.core import optimizer as optimizer_lib
from lingvo_amd.core import registry
from lingvo_amd.core import schedule as schedule_lib
from lingvo_amd.core.base_model_params import SingleTaskModelParams
from lingvo_amd.models import asr as asr_model


@registry.RegisterSingleTaskModel
class Librispeech960WpmConformerL(SingleTaskModelParams):
  """Conformer-L on (synthetic) Librispeech 960h, WPM targets."""

  BATCH_SIZE = 16
  FRAME_LEN = 1200
  TARGET_LEN = 64
  VOCAB = 1024

  def Train(self):
    return asr_model.SyntheticAsrInput.Params().Set(
        name='train', batch_size=self.BATCH_SIZE,
        frame_len=self.FRAME_LEN, target_len=self.TARGET_LEN,
        vocab_size=self.VOCAB)

  def Dev(self):
    return self.Train().Set(name='dev')

  def Test(self):
    return self.Train().Set(name='test')

  def Task(self):
    p = asr_model.AsrModel.Params().Set(name='librispeech_conformer_l')
    p.fprop_dtype = torch.bfloat16
    p.train.bf16_weights = True
    p.encoder.Set(input_dim=80, model_dim=512, num_layers=17, num_heads=8,
                  kernel_size=32, dropout_prob=0.1)
    p.decoder.Set(vocab_size=self.VOCAB, emb_dim=128, rnn_cell_dim=640,
                  num_lstm_layers=2, source_dim=512, dropout_prob=0.1)
    p.train.learner = learner_lib.Learner.Params().Set(
        learning_rate=1.0,
        optimizer=optimizer_lib.Adam.Params().Set(
            beta1=0.9, beta2=0.98, epsilon=1e-9),
        lr_schedule=schedule_lib.TransformerSchedule.Params().Set(
            warmup_steps=10_000, model_dim=512),
        clip_gradient_norm_to_value=5.0)
    return p


@registry.RegisterSingleTaskModel
class Librispeech960Grapheme(Librispeech960WpmConformerL):
  """Grapheme variant (reference librispeech.py:156): smaller vocab."""

  VOCAB = 76


@registry.RegisterSingleTaskModel
class Librispeech960ConformerS(Librispeech960WpmConformerL):
  """Conformer-S: 16 blocks, d=144, h=4 — quick tests."""

  def Task(self):
    p = super().Task()
    # d=144 is not H-kernel friendly; use d=256/h=4 -> H=64.
    p.encoder.Set(model_dim=256, num_layers=4, num_heads=4)
    p.decoder.Set(rnn_cell_dim=320, source_dim=256)
    return p


@registry.RegisterSingleTaskModel
class Librispeech960Base(Librispeech960WpmConformerL):
  """LAS baseline (reference librispeech.py:28 Librispeech960Base):
  conv frontend + 4x biLSTM-1024 encoder, attention LSTM decoder."""

  def Task(self):
    p = asr_model.AsrModel.Params().Set(name='librispeech_las')
    p.encoder = asr_model.LasEncoder.Params().Set(
        input_dim=80, model_dim=1024, num_lstm_layers=4,
        dropout_prob=0.2)
    p.fprop_dtype = torch.bfloat16
    p.train.bf16_weights = True
    p.decoder.Set(vocab_size=self.VOCAB, emb_dim=128, rnn_cell_dim=1024,
                  num_lstm_layers=2, source_dim=1024, dropout_prob=0.2)
    p.train.learner = learner_lib.Learner.Params().Set(
        learning_rate=2.5e-4,
        optimizer=optimizer_lib.Adam.Params().Set(
            beta1=0.9, beta2=0.999, epsilon=1e-6),
        lr_schedule=schedule_lib.ContinuousSchedule.Params().Set(
            start_step=50_000, half_life_steps=100_000),
        clip_gradient_norm_to_value=1.0)
    return p


@registry.RegisterSingleTaskModel
class Librispeech960BaseFusedScan(Librispeech960Base):
  """Librispeech960Base with the encoder biLSTMs on the fused scan
  (ops.lstm_scan). Same variables, so checkpoints interchange."""

  def Task(self):
    p = super().Task()
    p.encoder.fused_blstm_scan = True
    return p


@registry.RegisterSingleTaskModel
class Librispeech960BaseGrapheme(Librispeech960Base):
  """Grapheme-target LAS (reference librispeech.py:156)."""

  VOCAB = 76


@registry.RegisterSingleTaskModel
class Librispeech960Wpm(Librispeech960Base):
  """WPM-target LAS (reference librispeech.py:239
  Librispeech960Wpm: 16k word pieces, 96-dim embeddings, target len
  140). Synthetic inputs mirror the WPM shapes; plug a vocab file into
  tokenizers.WpmTokenizer for real data."""

  VOCAB = 16328
  TARGET_LEN = 140

  def Task(self):
    p = super().Task()
    p.name = 'librispeech_las_wpm'
    p.decoder.Set(vocab_size=self.VOCAB, emb_dim=96)
    return p


def _CtcHead(task_p):
  """Replaces the attention decoder of `task_p` with a CTC head of the
  same vocabulary over the same encoder outputs."""
  old = task_p.decoder
  task_p.decoder = asr_model.CtcDecoder.Params().Set(
      vocab_size=old.vocab_size, source_dim=old.source_dim,
      dropout_prob=old.dropout_prob)
  return task_p


@registry.RegisterSingleTaskModel
class Librispeech960WpmConformerLCtc(Librispeech960WpmConformerL):
  """CTC-only Conformer-L: the north-star encoder, learner and input with
  a CtcDecoder (frame-synchronous decode, no decoder recurrence)."""

  def Task(self):
    p = _CtcHead(super().Task())
    p.name = 'librispeech_conformer_l_ctc'
    return p


@registry.RegisterSingleTaskModel
class Librispeech960ConformerSCtc(Librispeech960ConformerS):
  """CTC-only Conformer-S: quick tests."""

  def Task(self):
    p = _CtcHead(super().Task())
    p.name = 'librispeech_conformer_s_ctc'
    return p


def _TransducerHead(task_p, joint_dim, rnn_cell_dim):
  """Replaces the attention decoder of `task_p` with a transducer decoder
  (one-layer LSTM prediction network + joint network) of the same
  vocabulary over the same encoder outputs."""
  old = task_p.decoder
  task_p.decoder = asr_model.TransducerDecoder.Params().Set(
      vocab_size=old.vocab_size, emb_dim=old.emb_dim,
      rnn_cell_dim=rnn_cell_dim, num_lstm_layers=1,
      source_dim=old.source_dim, joint_dim=joint_dim,
      dropout_prob=old.dropout_prob)
  return task_p


@registry.RegisterSingleTaskModel
class Librispeech960WpmConformerLTransducer(Librispeech960WpmConformerL):
  """Conformer-L transducer: the north-star encoder, learner and input with
  a TransducerDecoder (prediction network 1x640, joint 640, emb 128)."""

  def Task(self):
    p = _TransducerHead(super().Task(), joint_dim=640, rnn_cell_dim=640)
    p.name = 'librispeech_conformer_l_transducer'
    return p


@registry.RegisterSingleTaskModel
class Librispeech960ConformerSTransducer(Librispeech960ConformerS):
  """Conformer-S transducer: quick tests."""

  def Task(self):
    p = _TransducerHead(super().Task(), joint_dim=256, rnn_cell_dim=320)
    p.name = 'librispeech_conformer_s_transducer'
    return p


@registry.RegisterSingleTaskModel
class Librispeech960WpmConformerLJointCtc(Librispeech960WpmConformerL):
  """Joint CTC/attention Conformer-L: the attention decoder plus an
  auxiliary CTC head on the encoder, loss = 0.7 attention + 0.3 CTC."""

  def Task(self):
    p = super().Task()
    p.name = 'librispeech_conformer_l_joint_ctc'
    p.ctc_weight = 0.3
    return p
