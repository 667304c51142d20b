"""FAVOR+ attention microbenchmark: the HIP kernels against the composed twin.

  python tools/favor_bench.py [--rounds 5] [--iters 3]

Times ops.favor_attn.favor_attention for impl='auto' (ops/hip/favor_attn.hip)
and impl='torch' (the composed arithmetic of PerformerAttention) on bf16
inputs with m = 128 features, forward and forward+backward: one
Conformer-like non-causal shape and a causal sweep over T. The routes are
interleaved round by round in one process; the per-route median over the
rounds and torch.cuda.max_memory_allocated of one forward+backward are
printed. A route that runs out of memory is reported as OOM.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..'))

N, H, M = 8, 64, 128
SHAPES = [(64, 300, False)] + [(4, t, True) for t in (256, 1024, 4096)]


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


def bench(rounds, iters):
  import torch
  from lingvo_amd.layers import attention_sparse as asp
  from lingvo_amd.ops import favor_attn
  proj = asp.PerformerAttention.Params().Set(
      name='perf', input_dim=N * H, hidden_dim=N * H, num_heads=N,
      num_random_features=M).Instantiate().proj_mat.cuda()
  print('| B | T | causal | route | fwd ms | fwd+bwd ms | peak MB |')
  print('|---|---|---|---|---|---|---|')
  for b, t, causal in SHAPES:
    g = torch.Generator().manual_seed(0)
    q, k, v, dout = (
        (torch.randn(b, t, N, H, generator=g) * s).to('cuda', torch.bfloat16)
        for s in (0.3, 0.3, 1.0, 1.0))
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]

    def fwd(impl):
      with torch.no_grad():
        favor_attn.favor_attention(q, k, v, proj, causal=causal, impl=impl)

    def fwd_bwd(impl):
      for x in leaves:
        x.grad = None
      favor_attn.favor_attention(*leaves, proj, causal=causal,
                                 impl=impl).backward(dout)

    routes = ['auto', 'torch']
    peak, times = {}, {}
    for impl in list(routes):  # warm up; also the memory figure
      torch.cuda.synchronize()
      torch.cuda.reset_peak_memory_stats()
      try:
        fwd(impl)
        fwd_bwd(impl)
        torch.cuda.synchronize()
        peak[impl] = torch.cuda.max_memory_allocated() / 2**20
        times[impl] = dict(fwd=[], fwd_bwd=[])
      except torch.cuda.OutOfMemoryError:
        routes.remove(impl)
        for x in leaves:
          x.grad = None
        torch.cuda.empty_cache()
        print(f'| {b} | {t} | {causal} | {impl} | OOM | OOM | OOM |',
              flush=True)
    for _ in range(rounds):
      for impl in routes:
        times[impl]['fwd'].append(_measure(lambda: fwd(impl), iters))
        times[impl]['fwd_bwd'].append(_measure(lambda: fwd_bwd(impl), iters))
    for impl in routes:
      print(f'| {b} | {t} | {causal} | {impl} | '
            f'{statistics.median(times[impl]["fwd"]):.3f} | '
            f'{statistics.median(times[impl]["fwd_bwd"]):.3f} | '
            f'{peak[impl]:.0f} |', flush=True)
    del q, k, v, dout, leaves
    torch.cuda.empty_cache()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=3)
  args = ap.parse_args()
  bench(args.rounds, args.iters)


if __name__ == '__main__':
  main()
