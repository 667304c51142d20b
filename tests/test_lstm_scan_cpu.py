"""Fused LSTM scan (ops.lstm_scan) on CPU: the pure-torch twin of the HIP
step kernels, including its hand-written backward, against the existing
Recurrent-loop path in float64."""

import pytest
import torch

from lingvo_amd.core import registry
from lingvo_amd.layers import lstm_frnn_layer as lf

# Same mathematics on both paths, only the summation order differs
# (rounding ~1e-13 in float64 on O(1) values); a formula error is many
# orders of magnitude larger.
ATOL = 1e-9

B, T, DIN, H = 3, 7, 5, 32
CAP = 0.5


def _Paddings(b=B, t=T):
  """Trailing pads of different lengths, one fully padded row and one
  row with a padded step in the middle (0, 1, 0)."""
  pad = torch.zeros(b, t, dtype=torch.float64)
  pad[0, t - 2:] = 1.0
  pad[0, 2] = 1.0          # 0,1,0 in the middle
  pad[1, t - 4:] = 1.0
  pad[2, :] = 1.0          # fully padded
  return pad


def _Cell(h=H, **kw):
  cp = lf.LSTMCellSimpleExt.Params().Set(
      num_input_nodes=DIN, num_output_nodes=h, forget_gate_bias=1.0,
      cell_value_cap=CAP, dtype=torch.float64)
  return cp.Set(**kw)


def _Pair(cls, **kw):
  """(unfused, fused) float64 layers of `cls` with the same weights."""
  torch.manual_seed(0)
  ref = cls.Params().Set(name='r', fused_scan=False, **kw).Instantiate()
  fus = cls.Params().Set(name='f', fused_scan=True, **kw).Instantiate()
  ref = ref.double()
  fus = fus.double()
  with torch.no_grad():
    for v in ref.parameters():
      # Large weights / biases so the cell cap fires on some elements.
      v.copy_(torch.randn_like(v) * 0.7)
  fus.load_state_dict(ref.state_dict())
  return ref, fus


def _Inputs():
  torch.manual_seed(1)
  x = torch.randn(B, T, DIN, dtype=torch.float64) * 2.0
  return x, _Paddings()


def _AssertClampMixed(layer_cell, x, pad, reverse):
  """At least one c~ element is clamped and at least one is not."""
  from lingvo_amd.ops import lstm_scan as scan_ops
  m, c = scan_ops.lstm_scan(
      x.transpose(0, 1), [layer_cell.theta.wm], [layer_cell.theta.b],
      pad.transpose(0, 1), 1.0, CAP, (reverse,))
  # On an unpadded step c[t] is c~ itself, and clamp returns exactly
  # +-CAP where it fires.
  live = (pad.transpose(0, 1) == 0).unsqueeze(-1)
  clamped = (c[0].abs() == CAP) & live
  free = (c[0].abs() < CAP) & live
  assert bool(clamped.any()) and bool(free.any())


def _Grads(layer, names):
  return [dict(layer.named_parameters())[n].grad for n in names]


def test_bidirectional_fused_scan_matches_loop_float64():
  ref, fus = _Pair(lf.BidirectionalLstmFRNN, fwd=_Cell(), bak=_Cell())
  x, pad = _Inputs()
  _AssertClampMixed(ref.fwd_rnn.cell, x, pad, reverse=False)
  _AssertClampMixed(ref.bak_rnn.cell, x, pad, reverse=True)
  torch.manual_seed(2)
  w = torch.randn(B, T, 2 * H, dtype=torch.float64)
  outs, dxs = [], []
  for layer in (ref, fus):
    xi = x.clone().requires_grad_(True)
    out = layer.FProp(layer.theta, xi, pad)
    (out * w).sum().backward()
    outs.append(out.detach())
    dxs.append(xi.grad)
  assert outs[0].shape == (B, T, 2 * H)
  assert (outs[0] - outs[1]).abs().max() < ATOL
  assert (dxs[0] - dxs[1]).abs().max() < ATOL
  names = sorted(n for n, _ in ref.named_parameters())
  assert len(names) == 4  # wm and b for both directions
  for n, g_ref, g_fus in zip(names, _Grads(ref, names), _Grads(fus, names)):
    assert g_ref is not None and g_fus is not None, n
    assert float(g_ref.abs().max()) > 0, n
    assert (g_ref - g_fus).abs().max() < ATOL, n


def test_reverse_unidirectional_final_state_loss_float64():
  """Loss on the returned final state only: dm is zero everywhere but
  the last scan step and the cell gradient enters through dc."""
  ref, fus = _Pair(lf.LstmFRNN, cell=_Cell(), reverse=True)
  x, pad = _Inputs()
  _AssertClampMixed(ref.cell, x, pad, reverse=True)
  torch.manual_seed(3)
  wc = torch.randn(B, H, dtype=torch.float64)
  wm = torch.randn(B, H, dtype=torch.float64)
  res = []
  for layer in (ref, fus):
    xi = x.clone().requires_grad_(True)
    out, final = layer.FProp(layer.theta, xi, pad)
    ((final.c * wc).sum() + (final.m * wm).sum()).backward()
    res.append((out.detach(), final.c.detach(), final.m.detach(), xi.grad))
  for a, b in zip(*res):
    assert (a - b).abs().max() < ATOL
  assert float(res[0][3].abs().max()) > 0
  names = sorted(n for n, _ in ref.named_parameters())
  for n, g_ref, g_fus in zip(names, _Grads(ref, names), _Grads(fus, names)):
    assert (g_ref - g_fus).abs().max() < ATOL, n

  # c-only loss: the scan backward gets dm = None (grads are not
  # materialised).
  res = []
  for layer in (ref, fus):
    layer.zero_grad()
    xi = x.clone().requires_grad_(True)
    _, final = layer.FProp(layer.theta, xi, pad)
    (final.c * wc).sum().backward()
    res.append(xi.grad)
  assert (res[0] - res[1]).abs().max() < ATOL


@pytest.mark.parametrize('kw', [dict(couple_input_forget_gates=True),
                                dict(h=24)], ids=['cifg', 'h24'])
def test_ineligible_config_takes_loop_path_bit_identical(kw):
  kw = dict(kw)
  h = kw.pop('h', H)
  ref, fus = _Pair(lf.BidirectionalLstmFRNN, fwd=_Cell(h, **kw),
                   bak=_Cell(h, **kw))
  x, pad = _Inputs()
  res = []
  for layer in (ref, fus):
    xi = x.clone().requires_grad_(True)
    out = layer.FProp(layer.theta, xi, pad)
    out.square().sum().backward()
    res.append((out.detach(), xi.grad))
  assert torch.equal(res[0][0], res[1][0])
  assert torch.equal(res[0][1], res[1][1])
  names = sorted(n for n, _ in ref.named_parameters())
  for g_ref, g_fus in zip(_Grads(ref, names), _Grads(fus, names)):
    assert torch.equal(g_ref, g_fus)


def _SmallLas(key):
  model_p = registry.GetParams(key, 'Train')
  model_p.task.fprop_dtype = torch.float32
  model_p.task.train.bf16_weights = False
  model_p.task.random_seed = 5
  model_p.task.encoder.Set(model_dim=64, num_lstm_layers=2,
                           subsample_channels=8, dropout_prob=0.0)
  model_p.task.decoder.Set(rnn_cell_dim=32, source_dim=64, emb_dim=16,
                           vocab_size=32, dropout_prob=0.0)
  model_p.input.Set(batch_size=2, frame_len=32, target_len=6,
                    vocab_size=32)
  return model_p


def test_fused_scan_las_config_registered_and_checkpoint_compatible():
  key = 'asr.librispeech.Librispeech960BaseFusedScan'
  assert key in registry.GetAllRegisteredClasses()
  fused_p = _SmallLas(key)
  base_p = _SmallLas('asr.librispeech.Librispeech960Base')
  assert fused_p.task.encoder.fused_blstm_scan
  assert not base_p.task.encoder.fused_blstm_scan
  fused = fused_p.Instantiate()
  base = base_p.Instantiate()
  assert list(fused.state_dict().keys()) == list(base.state_dict().keys())
  for layer in fused.GetTask().encoder.rnn:
    assert layer.p.fused_scan
  # Same seed, same variables: the two configs compute the same loss.
  fused.load_state_dict(base.state_dict())
  task_f, task_b = fused.GetTask(), base.GetTask()
  batch = task_b.GetInputBatch()
  loss_b = task_b.TrainStep(batch)['loss'][0]
  loss_f = task_f.TrainStep(batch)['loss'][0]
  assert torch.isfinite(loss_f)
  loss_b, loss_f = float(loss_b.detach()), float(loss_f.detach())
  assert abs(loss_f - loss_b) < 1e-4 * max(1.0, abs(loss_b))


def _DirectInputs():
  torch.manual_seed(4)
  x = torch.randn(T, B, DIN, dtype=torch.float64)
  wms = [torch.randn(DIN + H, 4 * H, dtype=torch.float64) * 0.3
         for _ in range(2)]
  bs = [torch.randn(4 * H, dtype=torch.float64) * 0.3 for _ in range(2)]
  return x, wms, bs, _Paddings().t().contiguous()


def test_unused_output_gradient_reaches_backward_as_none(monkeypatch):
  from lingvo_amd.ops import lstm_scan as scan_ops
  seen = []
  real = scan_ops._bwd_steps_torch

  def Spy(gates, c, pad, wm_rec, dm_out, dc_out, *rest):
    seen.append((dm_out is None, dc_out is None))
    return real(gates, c, pad, wm_rec, dm_out, dc_out, *rest)

  monkeypatch.setattr(scan_ops, '_bwd_steps_torch', Spy)
  x, wms, bs, pad = _DirectInputs()
  for use_m, use_c in [(True, False), (False, True), (True, True)]:
    xi = x.clone().requires_grad_(True)
    m, c = scan_ops.lstm_scan(xi, wms, bs, pad, 1.0, CAP, (False, True))
    loss = (m.sum() if use_m else 0) + (c.square().sum() if use_c else 0)
    loss.backward()
    assert float(xi.grad.abs().max()) > 0
  assert seen == [(False, True), (True, False), (False, False)]


def test_backward_skips_gradients_nobody_needs():
  from lingvo_amd.ops import lstm_scan as scan_ops
  x, wms, bs, pad = _DirectInputs()
  torch.manual_seed(5)
  w = torch.randn(2, T, B, H, dtype=torch.float64)

  def Run(x_grad, w_grad):
    xi = x.clone().requires_grad_(x_grad)
    wi = [v.clone().requires_grad_(w_grad) for v in wms]
    bi = [v.clone().requires_grad_(True) for v in bs]
    m, _ = scan_ops.lstm_scan(xi, wi, bi, pad, 1.0, CAP, (False, True))
    (m * w).sum().backward()
    return xi.grad, [v.grad for v in wi], [v.grad for v in bi]

  full = Run(True, True)
  part = Run(False, False)
  assert part[0] is None and part[1] == [None, None]
  for a, b in zip(full[2], part[2]):
    assert torch.equal(a, b)
