"""Transducer loss microbenchmark: the HIP kernels against the torch route.

  python tools/rnnt_bench.py [--rounds 5] [--iters 3] [--dtype bf16]
                             [--shapes 32,300,64,1024 4,300,140,16328]

Times forward + backward of ops.rnnt.rnnt_loss on [B,T,U+1,V] logits with
labels [B,U] for impl='auto' (ops/hip/rnnt.hip) and impl='torch'
(log_softmax in fp32 + the per-diagonal recursion in torch ops under
autograd). Each shape runs in a child process of its own under a time
limit; inside it the variants are interleaved round by round, and the
per-variant median and min over the rounds are printed. A shape that fails
or runs out of time ends the run.
"""

from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..'))

DEFAULT_SHAPES = ['32,300,64,1024', '4,300,140,16328']


def run_shape(shape, rounds, iters, dtype):
  import torch
  from lingvo_amd.ops import rnnt
  b, t, u, v = shape
  dt = {'bf16': torch.bfloat16, 'fp32': torch.float32}[dtype]
  g = torch.Generator().manual_seed(0)
  logits = torch.empty(b, t, u + 1, v, dtype=dt, device='cuda')
  for i in range(b):  # row by row: no fp32 copy of the whole tensor
    logits[i] = torch.randn(t, u + 1, v, generator=g).to('cuda', dt)
  logits.requires_grad_(True)
  labels = torch.randint(1, v, (b, u), generator=g).cuda()
  logit_lengths = torch.randint(int(0.8 * t), t + 1, (b,), generator=g).cuda()
  label_lengths = torch.randint(int(0.75 * u), u + 1, (b,),
                                generator=g).cuda()
  w = torch.rand(b, generator=g).cuda()

  def run(impl):
    logits.grad = None
    nll, _ = rnnt.rnnt_loss(logits, logit_lengths, labels, label_lengths,
                            impl=impl)
    (nll * w).sum().backward()

  variants = ['auto', 'torch']
  times = {name: [] for name in variants}
  peak = {}
  for name in variants:  # warm up, and one pass for peak memory
    run(name)
    logits.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run(name)
    torch.cuda.synchronize()
    peak[name] = (torch.cuda.max_memory_allocated() - base) / 2**20
  for _ in range(rounds):
    for name in variants:
      t0 = time.perf_counter()
      for _ in range(iters):
        run(name)
      torch.cuda.synchronize()
      times[name].append((time.perf_counter() - t0) / iters * 1e3)
  print(f'rnnt loss fwd+bwd, {dtype} logits, B={b} T={t} U={u} V={v}, '
        f'{rounds} rounds x {iters} iters (ms)')
  for name in variants:
    ts = times[name]
    print(f'  impl={name:6s} median {statistics.median(ts):8.2f}  '
          f'min {min(ts):8.2f}  extra peak memory {peak[name]:8.0f} MiB',
          flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', nargs='+', default=DEFAULT_SHAPES,
                  help='B,T,U,V per shape.')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=3)
  ap.add_argument('--dtype', choices=['bf16', 'fp32'], default='bf16')
  ap.add_argument('--timeout', type=int, default=240,
                  help='Seconds each shape may take.')
  ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
  args = ap.parse_args()
  if args.child:
    run_shape([int(x) for x in args.child.split(',')], args.rounds,
              args.iters, args.dtype)
    return
  for shape in args.shapes:
    cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable,
           os.path.abspath(__file__), '--child', shape, '--rounds',
           str(args.rounds), '--iters', str(args.iters), '--dtype',
           args.dtype]
    rc = subprocess.run(cmd).returncode
    if rc != 0:
      print(f'rnnt_bench: shape {shape} ended with status {rc}; stopping',
            file=sys.stderr)
      sys.exit(rc)


if __name__ == '__main__':
  main()
