"""CTC forced-alignment microbenchmark: the HIP kernels against the
composed torch ops, with the loss forward as the scale.

  python tools/ctc_align_bench.py [--rounds 5] [--iters 3] [--dtype bf16]
                                  [--shapes 512,300,1024,64 128,300,16328,140]

Times ops.ctc.ctc_forced_align on [B,T,V] logits with labels [B,L] for
impl='auto' (ctc_rows_kernel + ctc_viterbi_kernel of ops/hip/ctc.hip; also
with the backpointer masks forced out of LDS into global memory) and
impl='torch' (log_softmax in fp32 + the batched torch twin), and the
forward of ops.ctc.ctc_loss(impl='auto'), which reads the same bytes and
runs twice as many lattice workgroups. Each shape runs in a child process
of its own under a time limit; inside it the variants are interleaved
round by round, and the per-variant median and min over the rounds are
printed. A shape that fails or runs out of time ends the run.
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

DEFAULT_SHAPES = ['512,300,1024,64', '128,300,16328,140']


def run_shape(shape, rounds, iters, dtype):
  import torch
  from lingvo_amd.ops import ctc
  b, t, v, l = shape
  dt = {'bf16': torch.bfloat16, 'fp32': torch.float32}[dtype]
  g = torch.Generator().manual_seed(0)
  logits = torch.randn(b, t, v, generator=g).to('cuda', dt)
  labels = torch.randint(1, v, (b, l), generator=g).cuda()
  logit_lengths = torch.randint(int(0.8 * t), t + 1, (b,), generator=g).cuda()
  label_lengths = torch.randint(int(0.75 * l), l + 1, (b,),
                                generator=g).cuda()
  args = (logits, logit_lengths, labels, label_lengths)
  from lingvo_amd.ops import _loader
  ext = _loader.get_ext(required=True)
  variants = {
      'align auto': lambda: ctc.ctc_forced_align(*args, impl='auto'),
      # The same kernels with the backpointer masks in global memory.
      'align global': lambda: ext.ctc_align(*args, 0, False),
      'align torch': lambda: ctc.ctc_forced_align(*args, impl='torch'),
      'loss fwd auto': lambda: ctc.ctc_loss(*args, impl='auto'),
  }
  times = {name: [] for name in variants}
  peak = {}
  for name, run in variants.items():  # warm up, and one pass for peak memory
    run()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    peak[name] = (torch.cuda.max_memory_allocated() - base) / 2**20
  for _ in range(rounds):
    for name, run in variants.items():
      t0 = time.perf_counter()
      for _ in range(iters):
        run()
      torch.cuda.synchronize()
      times[name].append((time.perf_counter() - t0) / iters * 1e3)
  print(f'ctc forced alignment, {dtype} logits, B={b} T={t} V={v} L={l}, '
        f'{rounds} rounds x {iters} iters (ms)')
  for name in variants:
    ts = times[name]
    print(f'  {name:14s} median {statistics.median(ts):8.2f}  '
          f'min {min(ts):8.2f}  extra peak memory {peak[name]:8.0f} MiB',
          flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', nargs='+', default=DEFAULT_SHAPES,
                  help='B,T,V,L per shape.')
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
      print(f'ctc_align_bench: shape {shape} ended with status {rc}; '
            f'stopping', file=sys.stderr)
      sys.exit(rc)


if __name__ == '__main__':
  main()
