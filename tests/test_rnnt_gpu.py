"""Transducer HIP kernels (ops/hip/rnnt.hip) against the float64 CPU
reference of test_rnnt_cpu.py, with the same reference recursion evaluated
in float32 on the same values as the error yardstick; then
TransducerDecoder on the GPU and a hipGraph-captured train step.

Bounds (ours gets a factor 2 over the yardstick's error; the CTC test's):
  nll      |err| <= 2*err32 + 2^-21*|ref|   (4 fp32 ulps)
  dlogits  |err| <= 2*err32 + 1e-6          (fp32 logits)
           ... + 2^-7*|ref|                 (bf16: one rounding)
err32 is the largest absolute error of the float32 reference over the
case's batch (nll) or over all its elements (dlogits), measured in the
test.
"""

import functools

import pytest
import torch

from lingvo_amd.ops import rnnt
import test_rnnt_cpu as lib

gpu = pytest.mark.gpu

U_MAX = rnnt.MAX_LABEL_LEN


def _Edge():
  return lib.EdgeBatch(), lib.EDGE_WEIGHTS


def _Random(b, t, v, u, seed, scale=3.0):
  return (lib.RandomBatch(b, t, v, u, seed, scale),
          lib.RandomWeights(b, seed))


# (B, T, V, U)
_CASES = {
    'edge': _Edge,
    # U1 = 64 / 65: one wave / just over one wave of lanes.
    'u63_t20_v33': lambda: _Random(2, 20, 33, 63, 63),
    'u64_t20_v33': lambda: _Random(2, 20, 33, 64, 64),
    # Sharp distributions: many states are impossible in fp32.
    'u64_t20_v33_x20': lambda: _Random(2, 20, 33, 64, 64, scale=60.0),
    'u64_t150_v32': lambda: _Random(2, 150, 32, 64, 150),   # 214 diagonals
    'u20_t40_v77': lambda: _Random(2, 40, 77, 20, 77),      # odd V
    'umax_t3_v8': lambda: _Random(1, 3, 8, U_MAX, 1023),    # 1024 lanes
    'u40_t1_v8': lambda: _Random(1, 1, 8, 40, 40),          # a single frame
    'b130_t6_v1024_u2': lambda: _Random(130, 6, 1024, 2, 130),
}


@functools.lru_cache(maxsize=None)
def _CaseAndReference(case, dtype):
  """Inputs rounded to `dtype`, the fp64 reference on exactly those values
  and the fp32 yardstick's errors against it. Computed once per (case,
  dtype); callers must not modify it."""
  (logits, tl, labels, ul), weights = _CASES[case]()
  logits = logits.to(dtype).float()
  batch = (logits, tl, labels, ul)
  ref = lib.Reference(*batch, weights)
  y_nll, _, y_grad = lib.Reference(*batch, weights, dtype=torch.float32)
  err32 = (float((y_nll.double() - ref[0]).abs().max()),
           float((y_grad.double() - ref[2]).abs().max()))
  return batch, weights, ref, err32


def _RunGpu(batch, weights, dtype, impl='auto'):
  logits, tl, labels, ul = batch
  x = logits.to('cuda', dtype).requires_grad_(True)
  nll, valid = rnnt.rnnt_loss(x, tl.cuda(), labels.cuda(), ul.cuda(),
                              impl=impl)
  (nll * torch.tensor(weights, device='cuda')).sum().backward()
  return nll.detach(), valid.detach(), x.grad


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16],
                         ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', list(_CASES))
def test_kernels_match_fp64_reference(case, dtype):
  batch, weights, (want_nll, want_valid, want_grad), err32 = \
      _CaseAndReference(case, dtype)
  tl, ul = batch[1], batch[3]
  nll, valid, grad = _RunGpu(batch, weights, dtype)
  nll2, valid2, grad2 = _RunGpu(batch, weights, dtype)
  assert nll.dtype == torch.float32 and grad.dtype == dtype

  nll_c, grad_c = nll.double().cpu(), grad.double().cpu()
  nll_err = (nll_c - want_nll).abs()
  nll_bound = 2 * err32[0] + 2.0**-21 * want_nll.abs()
  grad_err = (grad_c - want_grad).abs()
  grad_bound = 2 * err32[1] + 1e-6
  if dtype == torch.bfloat16:
    grad_bound = grad_bound + 2.0**-7 * want_grad.abs()
  grad_bound = grad_bound + torch.zeros_like(want_grad)
  worst = int((grad_err / grad_bound).argmax())
  print(f'rnnt {case} {"bf16" if dtype == torch.bfloat16 else "fp32"}: '
        f'valid {int(want_valid.sum())}/{len(want_valid)} '
        f'nll err {float(nll_err.max()):.3g} '
        f'(bound {float(nll_bound[nll_err.argmax()]):.3g}, '
        f'err32 {err32[0]:.3g}, |ref| max '
        f'{float(want_nll.abs().max()):.4g}) '
        f'dlogits err {float(grad_err.max()):.3g}, largest err/bound '
        f'{float(grad_err.reshape(-1)[worst]):.3g} / '
        f'{float(grad_bound.reshape(-1)[worst]):.3g} '
        f'(err32 {err32[1]:.3g})')

  assert torch.equal(valid.cpu().double(), want_valid)
  invalid = want_valid == 0
  assert bool((nll_c[invalid] == 0).all())
  assert bool((grad_c[invalid] == 0).all())
  for b, w in enumerate(weights):
    if w == 0.0:
      assert bool((grad_c[b] == 0).all()), b
    if want_valid[b]:
      assert bool((grad_c[b, int(tl[b]):] == 0).all()), b
      assert bool((grad_c[b, :, int(ul[b]) + 1:] == 0).all()), b
  assert torch.equal(nll, nll2) and torch.equal(valid, valid2)
  assert torch.equal(grad, grad2)
  assert bool(torch.isfinite(grad_c).all())
  assert bool((nll_err <= nll_bound).all()), (nll_err, nll_bound)
  assert bool((grad_err <= grad_bound).all()), (
      float(grad_err.reshape(-1)[worst]),
      float(grad_bound.reshape(-1)[worst]))


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16],
                         ids=['fp32', 'bf16'])
def test_bad_labels_are_invalid_rows(dtype):
  batch = lib.BadLabelBatch()
  nll, valid, grad = _RunGpu(batch, [1.0, 1.0, 1.0], dtype)
  assert valid.tolist() == [0, 0, 0]
  assert bool((nll == 0).all())
  assert bool((grad == 0).all())


@gpu
def test_forward_backward_memory_is_under_one_fp32_copy_of_the_logits():
  b, t, u, v = 4, 50, 16, 1024
  g = torch.Generator().manual_seed(9)
  x = torch.randn(b, t, u + 1, v, generator=g).to(
      'cuda', torch.bfloat16).requires_grad_(True)
  labels = torch.randint(1, v, (b, u), generator=g).cuda()
  tl = torch.full((b,), t, dtype=torch.long, device='cuda')
  ul = torch.full((b,), u, dtype=torch.long, device='cuda')
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  nll, _ = rnnt.rnnt_loss(x, tl, labels, ul)
  nll.sum().backward()
  torch.cuda.synchronize()
  extra = torch.cuda.max_memory_allocated() - base
  fp32_copy = 4 * b * t * (u + 1) * v
  print(f'rnnt fwd+bwd extra peak {extra / 2**20:.1f} MiB, one fp32 copy of '
        f'the logits {fp32_copy / 2**20:.1f} MiB')
  assert x.grad is not None and x.grad.dtype == torch.bfloat16
  assert extra < fp32_copy


@gpu
def test_host_guards_raise_before_launch():
  from lingvo_amd.ops import _loader
  ext = _loader.get_ext(required=True)
  assert ext.rnnt_max_label_len() == U_MAX == 1023
  logits, tl, labels, ul = (x.cuda() for x in lib.EdgeBatch())
  with pytest.raises(RuntimeError):
    ext.rnnt_fwd(logits.half(), tl, labels, ul, 0)            # dtype
  with pytest.raises(RuntimeError):
    ext.rnnt_fwd(logits.transpose(0, 1), tl, labels, ul, 0)   # contiguity
  with pytest.raises(RuntimeError):
    ext.rnnt_fwd(logits, tl.int(), labels, ul, 0)             # lengths dtype
  with pytest.raises(RuntimeError):
    ext.rnnt_fwd(logits, tl, labels, ul[:5], 0)               # lengths shape
  with pytest.raises(RuntimeError):
    ext.rnnt_fwd(logits, tl, labels.int(), ul, 0)             # labels dtype
  with pytest.raises(RuntimeError):
    ext.rnnt_fwd(logits, tl, labels[:, :2].contiguous(), ul, 0)  # U+1
  wide = torch.zeros(1, 1, U_MAX + 2, 2, device='cuda')
  with pytest.raises(RuntimeError, match='limit'):
    ext.rnnt_fwd(wide, tl[:1], torch.ones(1, U_MAX + 1, dtype=torch.long,
                                          device='cuda'), ul[:1], 0)
  for blank in (-1, 6):
    with pytest.raises(RuntimeError):
      ext.rnnt_fwd(logits, tl, labels, ul, blank)
  with pytest.raises(RuntimeError):
    ext.rnnt_fwd(logits[..., :1].contiguous(), tl, labels, ul, 0)  # V < 2
  with pytest.raises(RuntimeError):
    ext.rnnt_fwd(logits, tl.cpu(), labels, ul, 0)             # devices
  with pytest.raises(TypeError):
    rnnt.rnnt_loss(logits.half(), tl, labels, ul)
  torch.cuda.synchronize()


# ---- the layer ---------------------------------------------------------------
def _ScaledErr(got, want):
  scale = max(1.0, float(want.abs().max()))
  return float((got.float().cpu() - want).abs().max()) / scale


@gpu
def test_transducer_decoder_bf16_matches_cpu_fp32():
  """Project layer bound: 0.05 on outputs, 0.05 on gradients scaled by
  max(1, |want|.max()) (test_lstm_scan_gpu.py, test_ctc_gpu.py)."""
  from lingvo_amd.core.nested_map import NestedMap
  from lingvo_amd.models import asr
  b, t, d, v, u = 5, 12, 32, 16, 4
  torch.manual_seed(3)
  ref = asr.TransducerDecoder.Params().Set(
      name='rnnt', vocab_size=v, emb_dim=8, rnn_cell_dim=32,
      num_lstm_layers=1, source_dim=d, joint_dim=24,
      dropout_prob=0.0).Instantiate()
  p = ref.p.Copy()
  p.fprop_dtype = torch.bfloat16
  layer = p.Instantiate()
  layer.load_state_dict(ref.state_dict())
  layer = layer.to('cuda').to(torch.bfloat16)
  enc = torch.randn(b, t, d).bfloat16().float()
  enc_pad = (torch.arange(t)[None, :] >=
             torch.tensor([12, 10, 7, 5, 1])[:, None]).float()
  ids = torch.randint(1, v, (b, u))
  tgt_pad = (torch.arange(u)[None, :] >=
             torch.tensor([4, 3, 0, 2, 4])[:, None]).float()  # row 2: U_b = 0
  ids = ids * (1 - tgt_pad).long()

  def Run(layer, dev, dtype):
    x = enc.clone().to(dev, dtype).requires_grad_(True)
    tgt = NestedMap(ids=ids.to(dev), paddings=tgt_pad.to(dev))
    preds = layer.ComputePredictions(layer.theta, x, enc_pad.to(dev), tgt)
    assert preds.logits.shape == (b, t, u + 1, v)
    metrics, per_ex = layer.ComputeLoss(layer.theta, preds, tgt)
    metrics.loss[0].backward()
    grads = {n: v.grad for n, v in layer.named_parameters()}
    grads['enc'] = x.grad
    return metrics, per_ex, grads

  want_m, want_ex, want_g = Run(ref, 'cpu', torch.float32)
  got_m, got_ex, got_g = Run(layer, 'cuda', torch.bfloat16)
  assert float(want_m.rnnt_valid_fraction[0]) == 1.0
  assert float(got_m.rnnt_valid_fraction[0]) == 1.0
  assert float(got_m.loss[1]) == 5.0
  errs = {'loss': abs(float(got_m.loss[0].detach()) -
                      float(want_m.loss[0].detach())),
          'log_pplx': abs(float(got_m.log_pplx[0]) -
                          float(want_m.log_pplx[0]))}
  scaled = {n: _ScaledErr(got_g[n], want_g[n]) for n in want_g}
  print('rnnt layer bf16 vs cpu fp32: ' + ' '.join(
      f'{k}={v:.4g}' for k, v in {**errs, **scaled}.items()))
  assert len(scaled) >= 8 and all(g is not None for g in got_g.values())
  loss_scale = max(1.0, abs(float(want_m.loss[0].detach())))
  assert errs['loss'] / loss_scale < 0.05
  assert errs['log_pplx'] / max(1.0, abs(float(want_m.log_pplx[0]))) < 0.05
  for n, e in scaled.items():
    assert e < 0.05, (n, e)


@gpu
def test_graph_captured_transducer_train_step_matches_eager():
  from lingvo_amd.core import registry
  from lingvo_amd.runtime.graph_step import GraphedTrainStep

  def Task():
    mp = registry.GetParams(
        'asr.librispeech.Librispeech960ConformerSTransducer', 'Train')
    mp.input.Set(batch_size=4, frame_len=160, target_len=6)
    mp.task.random_seed = 11
    # No dropout or SpecAugment: the eager step and the captured one draw
    # their masks from differently seeded sources.
    mp.task.encoder.Set(dropout_prob=0.0, specaug_tpl=None)
    mp.task.decoder.dropout_prob = 0.0
    return mp.Instantiate().to('cuda').GetTask()

  eager_task = Task()
  batch = eager_task.input_generator.ToDevice(eager_task.GetInputBatch(),
                                              'cuda')
  eager = eager_task.TrainStep(batch)
  eager_loss = float(eager['loss'][0])
  graph_task = Task()
  step = GraphedTrainStep(graph_task, batch)
  graphed = step.Step(batch)
  graph_loss = float(graphed['loss'][0])
  torch.cuda.synchronize()
  print(f'rnnt ConformerS step loss: eager {eager_loss:.6f} '
        f'graph {graph_loss:.6f} valid '
        f'{float(graphed["rnnt_valid_fraction"][0]):.2f}')
  assert eager_loss == eager_loss and eager_loss > 0
  assert float(graphed['rnnt_valid_fraction'][0]) == 1.0
  # Same weights, batch and step seed; the conformer's bf16 kernels
  # accumulate with atomics, so allow one bf16 epsilon on the scalar.
  assert abs(graph_loss - eager_loss) <= 2.0**-8 * abs(eager_loss)
