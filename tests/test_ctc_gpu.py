"""CTC HIP kernels (ops/hip/ctc.hip) against torch's CTC on CPU in
float64, with torch's own fp32 GPU CTC on the same inputs as the error
yardstick; then CtcDecoder on the GPU and a hipGraph-captured train step.

Bounds (ours gets a factor 2 over the yardstick's error; both are fp32
log-domain recursions of the same depth):
  nll      |err| <= 2*err_torch + 2^-21*|ref|   (4 fp32 ulps)
  dlogits  |err| <= 2*err_torch + 1e-6          (fp32 logits)
           ... + 2^-7*|ref|                     (bf16: one rounding)
err_torch is the largest absolute error of impl='torch' over the case's
batch (nll) or over all its elements (dlogits), measured in the test.
"""

import functools

import pytest
import torch

from lingvo_amd.ops import ctc
import test_ctc_cpu as lib

gpu = pytest.mark.gpu

L_MAX = ctc.MAX_LABEL_LEN


def _Edge():
  return lib.EdgeBatch(), lib.EDGE_WEIGHTS


def _Random(b, t, v, l, seed, scale=3.0):
  return (lib.RandomBatch(b, t, v, l, seed, scale),
          lib.RandomWeights(b, seed))


_CASES = {
    'edge': _Edge,
    # S = 63 / 65: one wave / just over one wave of lattice positions.
    'l31_t70_v33': lambda: _Random(3, 70, 33, 31, 31),
    'l32_t70_v33': lambda: _Random(3, 70, 33, 32, 32),
    # Sharp distributions: many states are impossible in fp32.
    'l32_t70_v33_x20': lambda: _Random(3, 70, 33, 32, 32, scale=60.0),
    'l64_t300_v32': lambda: _Random(2, 300, 32, 64, 64),     # bench depth
    # Wpm target length; odd V, so rows are not 16-byte aligned.
    'l140_t300_v77': lambda: _Random(2, 300, 77, 140, 140),
    'lmax_v8': lambda: _Random(1, 2 * L_MAX + 1, 8, L_MAX, 511),
    'b130_t6_v1024_l2': lambda: _Random(130, 6, 1024, 2, 130),
}


@functools.lru_cache(maxsize=None)
def _CaseAndReference(case, dtype):
  """Inputs rounded to `dtype`, and the fp64 reference on exactly those
  values. Computed once per (case, dtype); callers must not modify it."""
  (logits, tl, labels, ll), weights = _CASES[case]()
  logits = logits.to(dtype).float()
  ref = lib.Reference(logits, tl, labels, ll, weights)
  return (logits, tl, labels, ll), weights, ref


def _RunGpu(batch, weights, dtype, impl):
  logits, tl, labels, ll = batch
  x = logits.to('cuda', dtype).requires_grad_(True)
  nll, valid = ctc.ctc_loss(x, tl.cuda(), labels.cuda(), ll.cuda(),
                            impl=impl)
  (nll * torch.tensor(weights, device='cuda')).sum().backward()
  return nll.detach(), valid.detach(), x.grad


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16],
                         ids=['fp32', 'bf16'])
@pytest.mark.parametrize('case', list(_CASES))
def test_kernels_match_fp64_reference(case, dtype):
  batch, weights, (want_nll, want_valid, want_grad) = _CaseAndReference(
      case, dtype)
  tl = batch[1]
  nll, valid, grad = _RunGpu(batch, weights, dtype, 'auto')
  nll2, valid2, grad2 = _RunGpu(batch, weights, dtype, 'auto')
  # The yardstick: torch's fp32 GPU kernels on the same values.
  t_nll, _, t_grad = _RunGpu(batch, weights, torch.float32, 'torch')
  assert nll.dtype == torch.float32 and grad.dtype == dtype

  nll_c, grad_c = nll.double().cpu(), grad.double().cpu()
  nll_err = (nll_c - want_nll).abs()
  nll_err_torch = float((t_nll.double().cpu() - want_nll).abs().max())
  nll_bound = 2 * nll_err_torch + 2.0**-21 * want_nll.abs()
  grad_err = (grad_c - want_grad).abs()
  grad_err_torch = float((t_grad.double().cpu() - want_grad).abs().max())
  grad_bound = 2 * grad_err_torch + 1e-6
  if dtype == torch.bfloat16:
    grad_bound = grad_bound + 2.0**-7 * want_grad.abs()
  grad_bound = grad_bound + torch.zeros_like(want_grad)
  worst = int(grad_err.argmax())
  print(f'ctc {case} {"bf16" if dtype == torch.bfloat16 else "fp32"}: '
        f'valid {int(want_valid.sum())}/{len(want_valid)} '
        f'nll err {float(nll_err.max()):.3g} '
        f'(bound {float(nll_bound[nll_err.argmax()]):.3g}, '
        f'torch {nll_err_torch:.3g}, |ref| max '
        f'{float(want_nll.abs().max()):.4g}) '
        f'dlogits err {float(grad_err.max()):.3g} '
        f'(bound {float(grad_bound.reshape(-1)[worst]):.3g}, '
        f'torch {grad_err_torch:.3g})')

  assert torch.equal(valid.cpu().double(), want_valid)
  invalid = want_valid == 0
  assert bool((nll_c[invalid] == 0).all())
  assert bool((grad_c[invalid] == 0).all())
  for b, w in enumerate(weights):
    if w == 0.0:
      assert bool((grad_c[b] == 0).all()), b
    assert bool((grad_c[b, int(tl[b]):] == 0).all()), b
  assert torch.equal(nll, nll2) and torch.equal(valid, valid2)
  assert torch.equal(grad, grad2)
  assert bool(torch.isfinite(grad_c).all())
  assert bool((nll_err <= nll_bound).all()), (nll_err, nll_bound)
  assert bool((grad_err <= grad_bound).all()), (
      float(grad_err.max()), float(grad_bound.reshape(-1)[worst]))


@gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16],
                         ids=['fp32', 'bf16'])
def test_bad_labels_are_invalid_rows(dtype):
  batch = lib.BadLabelBatch()
  nll, valid, grad = _RunGpu(batch, [1.0, 1.0], dtype, 'auto')
  assert valid.tolist() == [0, 0]
  assert bool((nll == 0).all())
  assert bool((grad == 0).all())


@gpu
def test_host_guards_raise_before_launch():
  from lingvo_amd.ops import _loader
  ext = _loader.get_ext(required=True)
  assert ext.ctc_max_label_len() == L_MAX
  logits, tl, labels, ll = (x.cuda() for x in lib.EdgeBatch())
  with pytest.raises(RuntimeError):
    ext.ctc_fwd(logits.half(), tl, labels, ll, 0)
  with pytest.raises(RuntimeError):
    ext.ctc_fwd(logits.transpose(0, 1), tl, labels, ll, 0)
  with pytest.raises(RuntimeError):
    ext.ctc_fwd(logits, tl, labels, ll, 5)
  with pytest.raises(RuntimeError):
    ext.ctc_fwd(logits, tl.int(), labels, ll, 0)
  with pytest.raises(RuntimeError):
    ext.ctc_fwd(logits, tl, labels[:5], ll, 0)
  wide = torch.ones(6, L_MAX + 1, dtype=torch.long, device='cuda')
  with pytest.raises(RuntimeError, match='limit'):
    ext.ctc_fwd(logits, tl, wide, ll, 0)
  with pytest.raises(TypeError):
    ctc.ctc_loss(logits.half(), tl, labels, ll)
  torch.cuda.synchronize()


# ---- the layer ---------------------------------------------------------------
def _ScaledErr(got, want):
  scale = max(1.0, float(want.abs().max()))
  return float((got.float().cpu() - want).abs().max()) / scale


@gpu
def test_ctc_decoder_bf16_matches_cpu_fp32():
  """Project layer bound: 0.05 on outputs, 0.05 on gradients scaled by
  max(1, |want|.max()) (test_lstm_scan_gpu.py)."""
  from lingvo_amd.core.nested_map import NestedMap
  from lingvo_amd.models import asr
  b, t, d, v, l = 5, 20, 32, 16, 4
  torch.manual_seed(3)
  ref = asr.CtcDecoder.Params().Set(
      name='ctc', vocab_size=v, source_dim=d, dropout_prob=0.0).Instantiate()
  p = ref.p.Copy()
  p.fprop_dtype = torch.bfloat16
  layer = p.Instantiate()
  layer.load_state_dict(ref.state_dict())
  layer = layer.to('cuda').to(torch.bfloat16)
  enc = torch.randn(b, t, d).bfloat16().float()
  enc_pad = (torch.arange(t)[None, :] >=
             torch.tensor([20, 17, 12, 9, 3])[:, None]).float()
  ids = torch.randint(1, v, (b, l))
  tgt_pad = (torch.arange(l)[None, :] >=
             torch.tensor([4, 3, 4, 2, 4])[:, None]).float()  # last: T < L
  ids = ids * (1 - tgt_pad).long()

  def Run(layer, dev, dtype):
    x = enc.clone().to(dev, dtype).requires_grad_(True)
    tgt = NestedMap(ids=ids.to(dev), paddings=tgt_pad.to(dev))
    preds = layer.ComputePredictions(layer.theta, x, enc_pad.to(dev), tgt)
    metrics, per_ex = layer.ComputeLoss(layer.theta, preds, tgt)
    metrics.loss[0].backward()
    grads = {n: v.grad for n, v in layer.named_parameters()}
    grads['enc'] = x.grad
    return metrics, per_ex, grads

  want_m, want_ex, want_g = Run(ref, 'cpu', torch.float32)
  got_m, got_ex, got_g = Run(layer, 'cuda', torch.bfloat16)
  assert abs(float(want_m.ctc_valid_fraction[0]) - 0.8) < 1e-6
  assert abs(float(got_m.ctc_valid_fraction[0]) - 0.8) < 1e-6
  assert float(got_m.loss[1]) == 4.0
  errs = {'loss': abs(float(got_m.loss[0].detach()) -
                      float(want_m.loss[0].detach())),
          'log_pplx': abs(float(got_m.log_pplx[0]) -
                          float(want_m.log_pplx[0]))}
  scaled = {n: _ScaledErr(got_g[n], want_g[n]) for n in want_g}
  print('ctc layer bf16 vs cpu fp32: ' + ' '.join(
      f'{k}={v:.4g}' for k, v in {**errs, **scaled}.items()))
  assert len(scaled) == 3 and all(g is not None for g in got_g.values())
  loss_scale = max(1.0, abs(float(want_m.loss[0].detach())))
  assert errs['loss'] / loss_scale < 0.05
  assert errs['log_pplx'] / max(1.0, abs(float(want_m.log_pplx[0]))) < 0.05
  for n, e in scaled.items():
    assert e < 0.05, (n, e)


@gpu
def test_graph_captured_ctc_train_step_matches_eager():
  from lingvo_amd.core import registry
  from lingvo_amd.runtime.graph_step import GraphedTrainStep

  def Task():
    mp = registry.GetParams('asr.librispeech.Librispeech960ConformerSCtc',
                            'Train')
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
  print(f'ctc ConformerS step loss: eager {eager_loss:.6f} '
        f'graph {graph_loss:.6f} valid '
        f'{float(graphed["ctc_valid_fraction"][0]):.2f}')
  assert eager_loss == eager_loss and eager_loss > 0
  assert float(graphed['ctc_valid_fraction'][0]) == 1.0
  # Same weights, batch and step seed; the conformer's bf16 kernels
  # accumulate with atomics, so allow one bf16 epsilon on the scalar.
  assert abs(graph_loss - eager_loss) <= 2.0**-8 * abs(eager_loss)
