"""CTC prefix beam search microbenchmark: the HIP kernels next to best-path
decoding of the same logits.

  python tools/ctc_beam_bench.py [--rounds 5] [--iters 20] [--dtype bf16]
                                 [--beam 8] [--token-beam 8] [--twin]
                                 [--shapes 16,300,1024 128,300,1024]

Times, on [B,T,V] logits with lengths in [0.8 T, T]:
  beam auto    ops.ctc.ctc_beam_search(impl='auto'): ctc_prune_rows_kernel +
               ctc_beam_kernel of ops/hip/ctc_beam.hip
  beam layer   CtcDecoder.BeamSearchDecode on those logits
  greedy       CtcDecoder.GreedyDecode on those logits (argmax + collapse)
  beam twin    with --twin, the textbook CPU search (copies included), once
The first shape is the Conformer CTC config's decode batch (16 x 1200
frames / 4, V = 1024). Each shape runs in a child process of its own under
a time limit; inside it the variants are interleaved round by round, each
round ends in a device synchronise, and the per-variant median and min
over the rounds are printed. Kernel times come from running one child
under a kernel trace, e.g.
  rocprofv3 --kernel-trace --stats -d OUT -- python tools/ctc_beam_bench.py
      --child 16,300,1024
A shape that fails or runs out of time ends the run.
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

DEFAULT_SHAPES = ['16,300,1024', '128,300,1024']


def run_shape(shape, args):
  import torch
  from lingvo_amd.models import asr
  from lingvo_amd.ops import ctc
  if not torch.cuda.is_available():
    raise RuntimeError('ctc_beam_bench: needs a GPU')
  b, t, v = shape
  dt = {'bf16': torch.bfloat16, 'fp32': torch.float32}[args.dtype]
  g = torch.Generator().manual_seed(0)
  logits = (torch.randn(b, t, v, generator=g) * 3.0).to('cuda', dt)
  lengths = torch.randint(int(0.8 * t), t + 1, (b,), generator=g).cuda()
  pad = (torch.arange(t, device='cuda')[None, :] >= lengths[:, None]).float()

  class LogitsAreGiven(asr.CtcDecoder):  # decode the logits themselves

    def _Logits(self, theta, enc):
      return enc

  dec = LogitsAreGiven.Params().Set(
      name='ctc', vocab_size=v, source_dim=8, beam_impl='auto',
      beam_token_beam=args.token_beam).Instantiate().cuda()
  dec.eval()
  variants = {
      'beam auto': lambda: ctc.ctc_beam_search(
          logits, lengths, args.beam, args.token_beam),
      'beam layer': lambda: dec.BeamSearchDecode(
          dec.theta, logits, pad, num_hyps=args.beam),
      'greedy': lambda: dec.GreedyDecode(dec.theta, logits, pad),
  }
  times = {name: [] for name in variants}
  with torch.no_grad():
    for run in variants.values():  # warm up
      run()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
      for name, run in variants.items():
        t0 = time.perf_counter()
        for _ in range(args.iters):
          run()
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / args.iters * 1e3)
  print(f'ctc beam search, {args.dtype} logits, B={b} T={t} V={v} '
        f'W={args.beam} C={args.token_beam}, {args.rounds} rounds x '
        f'{args.iters} iters (ms)')
  for name, ts in times.items():
    print(f'  {name:11s} median {statistics.median(ts):8.3f}  '
          f'min {min(ts):8.3f}', flush=True)
  if args.twin:
    t0 = time.perf_counter()
    ctc.ctc_beam_search(logits, lengths, args.beam, args.token_beam,
                        impl='torch')
    print(f'  beam twin   once   {(time.perf_counter() - t0) * 1e3:8.1f}',
          flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', nargs='+', default=DEFAULT_SHAPES,
                  help='B,T,V per shape.')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=20)
  ap.add_argument('--dtype', choices=['bf16', 'fp32'], default='bf16')
  ap.add_argument('--beam', type=int, default=8)
  ap.add_argument('--token-beam', type=int, default=8)
  ap.add_argument('--twin', action='store_true')
  ap.add_argument('--timeout', type=int, default=240,
                  help='Seconds each shape may take.')
  ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
  args = ap.parse_args()
  if args.child:
    run_shape([int(x) for x in args.child.split(',')], args)
    return
  for shape in args.shapes:
    cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable,
           os.path.abspath(__file__), '--child', shape, '--rounds',
           str(args.rounds), '--iters', str(args.iters), '--dtype',
           args.dtype, '--beam', str(args.beam), '--token-beam',
           str(args.token_beam)] + (['--twin'] if args.twin else [])
    rc = subprocess.run(cmd).returncode
    if rc != 0:
      print(f'ctc_beam_bench: shape {shape} ended with status {rc}; '
            f'stopping', file=sys.stderr)
      sys.exit(rc)


if __name__ == '__main__':
  main()
