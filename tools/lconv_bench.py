"""Depthwise-convolution / LConv-front microbenchmark at the Conformer-L
bench shape.

  python tools/lconv_bench.py [--batch 512] [--rounds 5] [--iters 3]

Routes are timed interleaved round by round in one process; each figure
includes everything the route launches. Prints per-route median and min
(ms per call) and, for the memory-bound forms, the GB the algorithm needs
over the median, to set against the ~6.3 TB/s achievable on one MI355X.

  plain fwd / bwd   depthwise_conv1d kernels, route 'naive' vs 'tiled'
  gn_fwd            GroupNorm + SiLU forward, scalar vs vector kernel
  front fwd / bwd   F.glu -> ApplyPadding -> conv(naive) -> autograd GLU
                    backward, mask and bf16 column sum, against the fused
                    glu_dwconv1d kernels
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..'))

import torch
import torch.nn.functional as F


def ab(title, fns, rounds, iters, gbytes=None):
  for fn in fns.values():  # warm up every route
    fn()
  torch.cuda.synchronize()
  times = {k: [] for k in fns}
  for _ in range(rounds):
    for k, fn in fns.items():
      t0 = time.perf_counter()
      for _ in range(iters):
        fn()
      torch.cuda.synchronize()
      times[k].append((time.perf_counter() - t0) / iters * 1e3)
  print(f'{title}: {rounds} rounds x {iters} iters (ms per call)')
  for k, v in times.items():
    med = statistics.median(v)
    rate = '' if not gbytes or k not in gbytes else \
        f'  {gbytes[k] / med:6.2f} TB/s of needed bytes'
    print(f'  {k:12s} median {med:8.3f}  min {min(v):8.3f}  '
          f'max {max(v):8.3f}{rate}')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=512)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=3)
  args = ap.parse_args()
  from lingvo_amd.core import py_utils
  from lingvo_amd.ops import _loader
  ext = _loader.get_ext(required=True)

  B, T, D, K = args.batch, 300, 512, 32
  pad = (K - 1) // 2
  g = torch.Generator(device='cuda').manual_seed(3)
  bf = dict(device='cuda', dtype=torch.bfloat16, generator=g)
  h = torch.randn(B, T, 2 * D, **bf)
  x = torch.randn(B, T, D, **bf)
  dy = torch.randn(B, T, D, **bf)
  w = torch.randn(K, D, **bf) * 0.3
  bias = torch.randn(D, **bf)
  lens = torch.randint(int(0.8 * T), T + 1, (B,), device='cuda', generator=g)
  padf = (torch.arange(T, device='cuda')[None, :] >= lens[:, None]).float()
  padb = padf.bfloat16()
  n = B * T
  gb = lambda elems: elems * 2 / 1e9  # bf16 GB; GB / ms == TB/s
  print(f'B={B} T={T} D={D} K={K}')

  routes = ['naive', 'tiled']
  ab('plain fwd',
     {r: (lambda r=r: ext.dwconv1d_fwd(x, w, bias, pad, r)) for r in routes},
     args.rounds, args.iters, {r: gb(2 * n * D) for r in routes})
  ab('plain bwd (dx + dw + db)',
     {r: (lambda r=r: ext.dwconv1d_bwd(dy, x, w, pad, r)) for r in routes},
     args.rounds, args.iters)

  gamma = torch.randn(D, **bf) * 0.1
  beta = torch.randn(D, **bf) * 0.1
  ab('gn_fwd (G=32, SiLU)',
     {r: (lambda r=r: ext.group_norm_fwd(x, gamma, beta, padb, 32, 1e-3, 1,
                                         r)) for r in ('scalar', 'vec')},
     args.rounds, args.iters, {r: gb(3 * n * D) for r in ('scalar', 'vec')})

  def UnfusedFwd():
    u = py_utils.ApplyPadding(padf, F.glu(h, dim=-1))
    return ext.dwconv1d_fwd(u, w, bias, pad, 'naive')

  hg = h.clone().requires_grad_(True)
  u_saved = py_utils.ApplyPadding(padf, F.glu(hg, dim=-1))

  def UnfusedBwd():
    dx, dw, db = ext.dwconv1d_bwd(dy, u_saved.detach(), w, pad, 'naive')
    hg.grad = None
    u_saved.backward(dx, retain_graph=True)
    return hg.grad.view(-1, 2 * D).sum(0), dw, db

  ab('front fwd',
     {'unfused': UnfusedFwd,
      'fused': lambda: ext.glu_dwconv1d_fwd(h, padb, w, bias, pad)},
     args.rounds, args.iters, {'fused': gb(3 * n * D)})
  # dx kernel: dy + h in, dh out; dw kernel: dy + h in.
  ab('front bwd (dh + dw + db + column sums)',
     {'unfused': UnfusedBwd,
      'fused': lambda: ext.glu_dwconv1d_bwd(dy, h, padb, w, pad)},
     args.rounds, args.iters, {'fused': gb(8 * n * D)})


if __name__ == '__main__':
  main()
