"""Conv-frontend microbenchmark at the Conformer-L bench shape.

  python tools/conv_frontend_bench.py [--batch 512] [--rounds 5] [--iters 3]

ConvSubsampling forward and forward+backward with the glue-fusion switch on
and off, interleaved round by round in one process; each figure includes
everything the route launches. Then kernels A (conv1_s2d_fwd) and B
(conv1_s2d_bwd) alone, with the GB each needs from shapes over the median,
to set against the ~6.3 TB/s copy rate of one MI355X.
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
        f'  needs {gbytes[k]:6.2f} GB: {gbytes[k] / med:5.2f} TB/s'
    print(f'  {k:14s} median {med:8.3f}  min {min(v):8.3f}  '
          f'max {max(v):8.3f}{rate}')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--batch', type=int, default=512)
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=3)
  args = ap.parse_args()
  from lingvo_amd.core import py_utils
  from lingvo_amd.layers import conformer
  from lingvo_amd.ops import _loader
  ext = _loader.get_ext(required=True)

  B, T, Fq, C, D = args.batch, 1200, 80, 256, 512
  torch.manual_seed(0)
  p = conformer.ConvSubsampling.Params().Set(
      name='sub', input_freq_dim=Fq, output_dim=D, channels=C)
  p.dtype = torch.bfloat16
  sub = p.Instantiate().to('cuda')
  x = torch.randn(B, T, Fq, device='cuda', dtype=torch.bfloat16)
  pad = torch.zeros(B, T, device='cuda')
  t1, h1 = (T + 1) // 2, (Fq + 1) // 2
  Hp, Wp = (t1 + 1) // 2 + 1, (h1 + 1) // 2 + 1
  print(f'B={B} T={T} F={Fq} C={C} D={D}')

  def Run(fused, backward):
    prev = py_utils.SetGlueFusion(fused)
    try:
      if not backward:
        with torch.no_grad():
          return sub.FProp(sub.theta, x, pad)[0]
      for v in sub.parameters():
        v.grad = None
      out, _ = sub.FProp(sub.theta, x, pad)
      out.backward(out.detach())
    finally:
      py_utils.SetGlueFusion(prev)

  for title, bwd in (('ConvSubsampling fwd', False),
                     ('ConvSubsampling fwd+bwd', True)):
    ab(title, {'fusion off': lambda: Run(False, bwd),
               'fusion on': lambda: Run(True, bwd)}, args.rounds, args.iters)
    torch.cuda.empty_cache()

  w1 = sub.theta.conv1_w.reshape(9, C).contiguous()
  b1 = sub.theta.conv1_b
  X = ext.conv1_s2d_fwd(x, w1, b1)
  dX = torch.randn_like(X)
  gb_x = X.numel() * 2 / 1e9          # GB; GB / ms == TB/s
  gb_in = x.numel() * 2 / 1e9
  live = B * t1 * h1 * C * 2 / 1e9    # non-padding cells
  ab('kernel A conv1_s2d_fwd', {'A': lambda: ext.conv1_s2d_fwd(x, w1, b1)},
     args.rounds, args.iters, {'A': gb_x + gb_in})
  ab('kernel B conv1_s2d_bwd', {'B': lambda: ext.conv1_s2d_bwd(dX, X, x)},
     args.rounds, args.iters, {'B': 2 * live + gb_in})


if __name__ == '__main__':
  main()
