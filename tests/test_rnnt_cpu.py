"""Transducer loss op (ops/rnnt.py) on CPU: the torch twin and impl='torch'
against an independent float64 reference (log_softmax, the alpha recursion
one anti-diagonal at a time, gradient by autograd), the reference itself
against a per-cell loop and a brute-force sum over alignments, and the
wrapper guards. Also holds the reference and the batches that
test_rnnt_gpu.py shares."""

import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from lingvo_amd.ops import rnnt

EDGE_WEIGHTS = [1.0, 0.5, 2.0, 1.5, 0.0, 3.0]


def EdgeBatch():
  """(B,T,U,V) = (6,5,3,6), blank 0: (logits bf16-exact fp32, T_b, labels,
  U_b). Row 4 has weight zero; row 5 (T_b = T+1) is the only invalid one."""
  g = torch.Generator().manual_seed(1234)
  logits = (3.0 * torch.randn(6, 5, 4, 6, generator=g)).bfloat16().float()
  labels = torch.tensor([[1, 2, 3],    # full lengths
                         [4, 5, 1],    # T_b = 1
                         [0, 0, 0],    # empty target
                         [2, 2, 0],    # T_b < T, U_b < U
                         [3, 1, 5],    # zero weight
                         [1, 2, 3]])   # T_b = T + 1
  label_lengths = torch.tensor([3, 3, 0, 2, 3, 3])
  logit_lengths = torch.tensor([5, 1, 4, 3, 5, 6])
  return logits, logit_lengths, labels, label_lengths


def BadLabelBatch():
  """Three rows that are invalid by the label-range rule only: the blank,
  V and -1 inside the valid length (V=5)."""
  g = torch.Generator().manual_seed(4321)
  logits = (3.0 * torch.randn(3, 4, 5, 5, generator=g)).bfloat16().float()
  labels = torch.tensor([[1, 0, 3, 4], [1, 2, 5, 4], [-1, 2, 3, 9]])
  return logits, torch.tensor([4, 4, 4]), labels, torch.tensor([4, 3, 2])


def RandomBatch(b, t, v, u, seed, scale=1.0):
  """Random logits [b,t,u+1,v] and labels; row 0 has full lengths, the
  others random ones."""
  g = torch.Generator().manual_seed(seed)
  logits = scale * torch.randn(b, t, u + 1, v, generator=g)
  labels = torch.randint(1, v, (b, u), generator=g)
  logit_lengths = torch.randint(max(t // 2, 1), t + 1, (b,), generator=g)
  label_lengths = torch.randint(u // 2, u + 1, (b,), generator=g)
  logit_lengths[0] = t
  label_lengths[0] = u
  return logits, logit_lengths, labels, label_lengths


def RandomWeights(b, seed):
  g = torch.Generator().manual_seed(seed + 77)
  w = 0.5 + torch.rand(b, generator=g)
  if b >= 2:
    w[-1] = 0.0  # a zero-weight row
  return w.tolist()


def _RowValid(tb, ub, labels_b, t, u, v, blank_id):
  if not (1 <= tb <= t and 0 <= ub <= u):
    return False
  return all(0 <= int(y) < v and int(y) != blank_id for y in labels_b[:ub])


def _RowLogLikelihood(lp, labels_b, tb, ub, blank_id):
  """ll of one valid row out of log-probs lp [T,U1,V]: the alpha recursion
  one anti-diagonal at a time, as vectors over u."""
  blank = lp[:tb, :ub + 1, blank_id]                        # [tb, ub+1]
  uu = torch.arange(ub + 1)
  ninf = torch.full((ub + 1,), -math.inf, dtype=lp.dtype)
  if ub > 0:
    lab = lp[:tb, :ub].gather(
        2, labels_b[:ub][None, :, None].expand(tb, ub, 1))[..., 0]
  a = torch.where(uu == 0, torch.zeros_like(ninf), ninf)    # diagonal 0
  for d in range(1, tb + ub):
    t_cur = d - uu
    on = (t_cur >= 0) & (t_cur < tb)
    # From (t-1, u) by a blank.
    t_prev = t_cur - 1
    has_b = on & (t_prev >= 0)
    via_blank = torch.where(has_b, a + blank[t_prev.clamp(0, tb - 1), uu],
                            ninf)
    # From (t, u-1) by label u.
    via_label = ninf
    if ub > 0:
      left = a[:-1] + lab[t_cur[1:].clamp(0, tb - 1), uu[:-1]]
      via_label = torch.cat([ninf[:1], torch.where(on[1:], left, ninf[1:])])
    new = torch.logaddexp(via_blank, via_label)
    a = torch.where(on, new, ninf)
  return a[ub] + blank[tb - 1, ub]


def Reference(logits, logit_lengths, labels, label_lengths, weights,
              blank_id=0, dtype=torch.float64):
  """-> (nll, valid, dlogits) in `dtype` (float64: the reference; float32:
  the error yardstick) for the loss sum_b weights_b * nll_b on exactly
  these logits. Written independently of ops/rnnt.py."""
  logits = logits.detach().cpu().to(dtype)
  b, t, u1, v = logits.shape
  leaf = logits.clone().requires_grad_(True)
  nll, valid = [], []
  for i in range(b):
    tb, ub = int(logit_lengths[i]), int(label_lengths[i])
    ok = _RowValid(tb, ub, labels[i].tolist(), t, u1 - 1, v, blank_id)
    if ok:
      ll = _RowLogLikelihood(F.log_softmax(leaf[i], dim=-1),
                             labels[i].cpu(), tb, ub, blank_id)
      ok = bool(torch.isfinite(ll))
    valid.append(1.0 if ok else 0.0)
    nll.append(-ll if ok else torch.zeros((), dtype=dtype))
  nll = torch.stack(nll)
  total = (nll * torch.as_tensor(weights, dtype=dtype)).sum()
  if total.requires_grad:
    total.backward()
  grad = leaf.grad if leaf.grad is not None else torch.zeros_like(logits)
  return nll.detach(), torch.tensor(valid, dtype=dtype), grad


# ---- the reference against two other formulations ---------------------------
def _CellLoop(lp, labels_b, tb, ub, blank_id=0):
  alpha = [[-math.inf] * (ub + 1) for _ in range(tb)]
  for t in range(tb):
    for u in range(ub + 1):
      if t == 0 and u == 0:
        alpha[t][u] = 0.0
        continue
      terms = []
      if t > 0:
        terms.append(alpha[t - 1][u] + float(lp[t - 1, u, blank_id]))
      if u > 0:
        terms.append(alpha[t][u - 1] +
                     float(lp[t, u - 1, int(labels_b[u - 1])]))
      m = max(terms)
      alpha[t][u] = m + math.log(sum(math.exp(x - m) for x in terms))
  return alpha[tb - 1][ub] + float(lp[tb - 1, ub, blank_id])


def _BruteForce(lp, labels_b, tb, ub, blank_id=0):
  """Sum over every alignment: the orders of tb-1 blanks and ub labels,
  then the final blank."""
  total = 0.0
  for label_slots in itertools.combinations(range(tb - 1 + ub), ub):
    t = u = 0
    logp = 0.0
    for step in range(tb - 1 + ub):
      if step in label_slots:
        logp += float(lp[t, u, int(labels_b[u])])
        u += 1
      else:
        logp += float(lp[t, u, blank_id])
        t += 1
    assert (t, u) == (tb - 1, ub)
    total += math.exp(logp + float(lp[t, u, blank_id]))
  return math.log(total)


@pytest.mark.parametrize('t,u', [(1, 0), (1, 2), (3, 0), (4, 3)])
def test_reference_equals_cell_loop_and_brute_force(t, u):
  v = 5
  g = torch.Generator().manual_seed(100 * t + u)
  logits = torch.randn(1, t, u + 1, v, generator=g, dtype=torch.float64)
  labels = torch.randint(1, v, (1, u), generator=g)
  nll, valid, _ = Reference(logits, torch.tensor([t]), labels,
                            torch.tensor([u]), [1.0])
  lp = F.log_softmax(logits[0], dim=-1)
  assert valid.tolist() == [1.0]
  assert abs(-float(nll[0]) - _CellLoop(lp, labels[0], t, u)) <= 1e-12
  assert abs(-float(nll[0]) - _BruteForce(lp, labels[0], t, u)) <= 1e-12


# ---- the op ------------------------------------------------------------------
def _Run(batch, weights, dtype, impl='auto', blank_id=0):
  logits, tl, labels, ll = batch
  x = logits.to(dtype).requires_grad_(True)
  nll, valid = rnnt.rnnt_loss(x, tl, labels, ll, blank_id=blank_id, impl=impl)
  assert not valid.requires_grad
  (nll * torch.as_tensor(weights, dtype=nll.dtype)).sum().backward()
  return nll.detach(), valid, x.grad


def _Close(got, want, tag, tol=1e-10):
  err = float((got - want).abs().max()) if want.numel() else 0.0
  print(f'{tag}: max err {err:.3g}')
  assert err <= tol, tag


_CASES = {
    'edge': lambda: (EdgeBatch(), EDGE_WEIGHTS),
    'b3t12u7v5': lambda: (RandomBatch(3, 12, 5, 7, 12), RandomWeights(3, 12)),
}


@pytest.mark.parametrize('case', sorted(_CASES))
@pytest.mark.parametrize('impl', ['auto', 'torch'])
def test_float64_matches_reference(case, impl):
  batch, weights = _CASES[case]()
  want_nll, want_valid, want_grad = Reference(*batch, weights)
  nll, valid, grad = _Run(batch, weights, torch.float64, impl)
  assert nll.dtype == torch.float64 and grad.dtype == torch.float64
  assert torch.equal(valid, want_valid), (valid, want_valid)
  _Close(nll, want_nll, f'{case} {impl} nll')
  _Close(grad, want_grad, f'{case} {impl} dlogits')


def _AssertEdgeZeros(nll, valid, grad):
  _, tl, _, ul = EdgeBatch()
  assert valid.tolist() == [1, 1, 1, 1, 1, 0]
  assert float(nll[5]) == 0.0
  assert bool((grad[5] == 0).all())      # invalid row
  assert bool((grad[4] == 0).all())      # zero-weight row
  for b in range(5):
    assert bool((grad[b, int(tl[b]):] == 0).all()), b
    assert bool((grad[b, :, int(ul[b]) + 1:] == 0).all()), b
  for b in (0, 1, 2, 3):
    assert float(grad[b].abs().max()) > 0


@pytest.mark.parametrize('impl', ['auto', 'torch'])
def test_edge_batch_validity_and_exact_zeros(impl):
  nll, valid, grad = _Run(EdgeBatch(), EDGE_WEIGHTS, torch.float64, impl)
  _AssertEdgeZeros(nll, valid, grad)


@pytest.mark.parametrize('impl', ['auto', 'torch'])
def test_bad_labels_are_invalid_rows(impl):
  batch = BadLabelBatch()
  w = [1.0, 1.0, 1.0]
  nll, valid, grad = _Run(batch, w, torch.float64, impl)
  want_nll, want_valid, want_grad = Reference(*batch, w)
  assert want_valid.tolist() == [0, 0, 0]
  assert valid.tolist() == [0, 0, 0]
  assert bool((nll == 0).all()) and bool((grad == 0).all())
  assert bool((want_nll == 0).all()) and bool((want_grad == 0).all())


def test_gradcheck():
  x = torch.randn(2, 3, 3, 4, dtype=torch.float64,
                  generator=torch.Generator().manual_seed(5))
  x.requires_grad_(True)
  tl = torch.tensor([3, 2])
  labels = torch.tensor([[1, 2], [3, 1]])
  ul = torch.tensor([2, 1])
  assert torch.autograd.gradcheck(
      lambda a: rnnt.rnnt_loss(a, tl, labels, ul)[0], (x,))


def test_wrapper_guards():
  logits, tl, labels, ul = EdgeBatch()
  with pytest.raises(TypeError):
    rnnt.rnnt_loss(logits.long(), tl, labels, ul)            # logits dtype
  with pytest.raises(ValueError):
    rnnt.rnnt_loss(logits.transpose(0, 1), tl, labels, ul)   # not contiguous
  with pytest.raises(TypeError):
    rnnt.rnnt_loss(logits, tl.float(), labels, ul)           # lengths dtype
  with pytest.raises(TypeError):
    rnnt.rnnt_loss(logits, tl, labels, ul[:5])               # lengths shape
  with pytest.raises(TypeError):
    rnnt.rnnt_loss(logits, tl, labels.int(), ul)             # labels dtype
  with pytest.raises(ValueError):
    rnnt.rnnt_loss(logits, tl, labels[:, :2], ul)            # U+1 != shape[2]
  wide = torch.zeros(1, 2, rnnt.MAX_LABEL_LEN + 2, 2)
  with pytest.raises(ValueError, match='limit'):
    rnnt.rnnt_loss(wide, torch.tensor([2]),
                   torch.ones(1, rnnt.MAX_LABEL_LEN + 1, dtype=torch.long),
                   torch.tensor([0]))                        # U over the limit
  for blank in (-1, 6):
    with pytest.raises(ValueError):
      rnnt.rnnt_loss(logits, tl, labels, ul, blank_id=blank)
  with pytest.raises(ValueError):
    rnnt.rnnt_loss(logits[..., :1].contiguous(), tl, labels, ul)  # V < 2
  # B*T*(U+1) >= 2^31: shapes only, nothing is allocated.
  big = torch.empty(2**20, 2**10, 2, 2, device='meta')
  with pytest.raises(ValueError, match='limit'):
    rnnt.rnnt_loss(big, torch.empty(2**20, dtype=torch.long, device='meta'),
                   torch.empty(2**20, 1, dtype=torch.long, device='meta'),
                   torch.empty(2**20, dtype=torch.long, device='meta'))
  with pytest.raises(ValueError):                            # devices differ
    rnnt.rnnt_loss(logits, tl, labels,
                   torch.empty(6, dtype=torch.long, device='meta'))
  with pytest.raises(ValueError):
    rnnt.rnnt_loss(logits, tl, labels, ul, impl='warp')
  assert rnnt.MAX_LABEL_LEN == 1023
  at_limit = torch.zeros(1, 1, rnnt.MAX_LABEL_LEN + 1, 2)
  nll, valid = rnnt.rnnt_loss(
      at_limit, torch.tensor([1]),
      torch.ones(1, rnnt.MAX_LABEL_LEN, dtype=torch.long), torch.tensor([3]))
  assert nll.shape == (1,) and valid.tolist() == [1.0]


def test_nonzero_blank_id():
  batch = RandomBatch(3, 10, 6, 3, 21)
  logits, tl, labels, ul = batch
  labels = labels.clamp(max=4)  # blank is 5
  batch = (logits, tl, labels, ul)
  weights = [1.0, 2.0, 0.5]
  want = Reference(*batch, weights, blank_id=5)
  for impl in ('auto', 'torch'):
    nll, valid, grad = _Run(batch, weights, torch.float64, impl, blank_id=5)
    assert torch.equal(valid, want[1])
    _Close(nll, want[0], f'blank5 {impl} nll')
    _Close(grad, want[2], f'blank5 {impl} dlogits')


def test_fp32_twin_returns_fp32_and_is_as_close_as_the_fp32_reference():
  batch, weights = _CASES['b3t12u7v5']()
  batch = (batch[0].float(),) + batch[1:]
  want_nll, want_valid, want_grad = Reference(*batch, weights)
  y_nll, _, y_grad = Reference(*batch, weights, dtype=torch.float32)
  nll, valid, grad = _Run(batch, weights, torch.float32)
  assert nll.dtype == torch.float32 and grad.dtype == torch.float32
  assert valid.dtype == torch.float32
  assert torch.equal(valid.double(), want_valid)
  nll_err32 = float((y_nll.double() - want_nll).abs().max())
  grad_err32 = float((y_grad.double() - want_grad).abs().max())
  nll_err = float((nll.double() - want_nll).abs().max())
  grad_err = float((grad.double() - want_grad).abs().max())
  print(f'fp32 twin: nll err {nll_err:.3g} (fp32 reference {nll_err32:.3g}) '
        f'dlogits err {grad_err:.3g} (fp32 reference {grad_err32:.3g})')
  assert nll_err <= 2 * nll_err32
  assert grad_err <= 2 * grad_err32
