"""Block-sparse attention microbenchmark: the HIP kernels against the composed
twin and dense flash attention.

  python tools/block_sparse_bench.py [--rounds 5] [--iters 3]
                                     [--densities 0.1,0.4] [--limit 300]

Times ops.block_sparse_attn.block_sparse_attention for impl='auto'
(ops/hip/block_sparse_attn.hip) and impl='torch' (the dense-mask arithmetic
of BlockSparseAttention's composed route), and ops.flash_attn.flash_attention
with no mask at the same T as the no-sparsity yardstick, on bf16 inputs,
forward and forward+backward. The pattern is LocalGlobalBlockMask with one
global block, block size 64, and the local width whose 64x64 tile density is
closest to each requested one; the density reached is printed. The routes
are interleaved round by round in one process; the per-route median and min
over the rounds and torch.cuda.max_memory_allocated of one forward+backward
are printed. A route that runs out of memory is reported as OOM.

Each (T, density) case runs in a child process of its own under a time limit
(--limit seconds); the first case that fails or overruns ends the run.
"""

from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..'))

B, N, H, BS = 8, 8, 64, 64
LENGTHS = (1024, 4096)


def _measure(fn, iters):
  import torch
  start = torch.cuda.Event(enable_timing=True)
  end = torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(iters):
    fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end) / iters


def _Pattern(t, density):
  """(mask, width, tile density) of the local width closest to `density`."""
  from lingvo_amd.layers import attention_sparse as asp
  nb = t // BS
  best = None
  for w in range(nb):
    m = asp.LocalGlobalBlockMask(nb, 1, w)
    d = sum(map(sum, m)) / (nb * nb)
    if best is None or abs(d - density) < abs(best[2] - density):
      best = (m, w, d)
  return best


def case(t, density, rounds, iters):
  import torch
  from lingvo_amd.ops import block_sparse_attn as bsa
  from lingvo_amd.ops import flash_attn
  mask, width, dens = _Pattern(t, density)
  mask = torch.tensor(mask, dtype=torch.bool)  # no per-call list conversion
  g =torch.Generator().manual_seed(0)
  q, k, v, dout = (
      (torch.randn(B, t, N, H, generator=g) * s).to('cuda', torch.bfloat16)
      for s in (0.3, 0.3, 1.0, 1.0))
  leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]

  def run(route, x):
    if route == 'flash':
      return flash_attn.flash_attention(*x)
    return bsa.block_sparse_attention(
        *x, mask, BS, impl='auto' if route == 'kernel' else 'torch')

  def fwd(route):
    with torch.no_grad():
      run(route, (q, k, v))

  def fwd_bwd(route):
    for x in leaves:
      x.grad = None
    run(route, leaves).backward(dout)

  routes = ['kernel', 'torch', 'flash']
  peak, times = {}, {}
  for route in list(routes):  # warm up; also the memory figure
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    try:
      fwd(route)
      fwd_bwd(route)
      torch.cuda.synchronize()
      peak[route] = torch.cuda.max_memory_allocated() / 2**20
      times[route] = dict(fwd=[], fwd_bwd=[])
    except torch.cuda.OutOfMemoryError:
      routes.remove(route)
      for x in leaves:
        x.grad = None
      torch.cuda.empty_cache()
      print(f'| {t} | {width} | {dens:.3f} | {route} | OOM | OOM | OOM | OOM '
            '| OOM |', flush=True)
  for _ in range(rounds):
    for route in routes:
      times[route]['fwd'].append(_measure(lambda: fwd(route), iters))
      times[route]['fwd_bwd'].append(_measure(lambda: fwd_bwd(route), iters))
  for route in routes:
    f, fb = times[route]['fwd'], times[route]['fwd_bwd']
    print(f'| {t} | {width} | {dens:.3f} | {route} | '
          f'{statistics.median(f):.3f} | {min(f):.3f} | '
          f'{statistics.median(fb):.3f} | {min(fb):.3f} | '
          f'{peak[route]:.0f} |', flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=3)
  ap.add_argument('--densities', default='0.1,0.4')
  ap.add_argument('--limit', type=float, default=300.,
                  help='seconds each case may take')
  ap.add_argument('--case', default='', help='T,density: run one case here')
  args = ap.parse_args()
  if args.case:
    t, density = args.case.split(',')
    case(int(t), float(density), args.rounds, args.iters)
    return
  print(f'B={B} N={N} H={H} block_size={BS}, LocalGlobalBlockMask(T/64, 1, '
        f'width); {args.rounds} rounds x {args.iters} iters, ms')
  print('| T | width | tile density | route | fwd median | fwd min | '
        'fwd+bwd median | fwd+bwd min | peak MB |')
  print('|---|---|---|---|---|---|---|---|---|', flush=True)
  for t in LENGTHS:
    for density in args.densities.split(','):
      subprocess.run(
          [sys.executable, os.path.abspath(__file__), '--case',
           f'{t},{density}', '--rounds', str(args.rounds), '--iters',
           str(args.iters)], check=True, timeout=args.limit)


if __name__ == '__main__':
  main()
