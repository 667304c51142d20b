"""Routing attention microbenchmark: the HIP kernels against the layer's
composed loop over the clusters and dense flash attention.

  python tools/routing_attn_bench.py [--rounds 5] [--iters 3] [--limit 300]

Times ops.routing_attn.routing_attention (ops/hip/routing_attn.hip, list
kernel included), RoutingAttention._ComposedContext (topk, gather and dense
fp32 attention of all queries per cluster: what the layer runs elsewhere) and
ops.flash_attn.flash_attention with no mask at the same T as the no-sparsity
yardstick, on bf16 inputs, forward and forward+backward. Cluster ids are
uniform random, so a cluster holds about T/C keys: window T/C cuts about half
of the clusters short, 2T/C almost none. The routes are interleaved round by
round in one process; the per-route median and min over the rounds and
torch.cuda.max_memory_allocated of one forward+backward are printed. A route
that runs out of memory is reported as OOM.

Each (T, C, window) case runs in a child process of its own under a time
limit (--limit seconds); the first case that fails or overruns ends the run.
"""

from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..'))

B, N, H = 8, 8, 64
LENGTHS = (1024, 4096)
CLUSTERS = (4, 16)


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


def case(t, c, window, rounds, iters):
  import torch
  from lingvo_amd.layers import attention_sparse as asp
  from lingvo_amd.ops import flash_attn
  from lingvo_amd.ops import routing_attn
  layer = asp.RoutingAttention.Params().Set(
      name='bench', input_dim=N * H, hidden_dim=N * H, num_heads=N,
      num_clusters=c, atten_window=window, dtype=torch.bfloat16).Instantiate()
  g = torch.Generator().manual_seed(0)
  q, k, v, dout = (
      (torch.randn(B, t, N, H, generator=g) * s).to('cuda', torch.bfloat16)
      for s in (0.3, 0.3, 1.0, 1.0))
  q_cl, k_cl = (torch.randint(0, c, (B, N, t), generator=g).cuda()
                for _ in range(2))
  leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]

  def run(route, x):
    if route == 'flash':
      return flash_attn.flash_attention(*x)
    if route == 'kernel':
      return routing_attn.routing_attention(*x, q_cl, k_cl, c, window)
    return layer._ComposedContext(*x, q_cl, k_cl, None).to(torch.bfloat16)

  def fwd(route):
    with torch.no_grad():
      run(route, (q, k, v))

  def fwd_bwd(route):
    for x in leaves:
      x.grad = None
    run(route, leaves).backward(dout)

  routes = ['kernel', 'composed', 'flash']
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
      print(f'| {t} | {c} | {window} | {route} | OOM | OOM | OOM | OOM '
            '| OOM |', flush=True)
  for _ in range(rounds):
    for route in routes:
      times[route]['fwd'].append(_measure(lambda: fwd(route), iters))
      times[route]['fwd_bwd'].append(_measure(lambda: fwd_bwd(route), iters))
  for route in routes:
    f, fb = times[route]['fwd'], times[route]['fwd_bwd']
    print(f'| {t} | {c} | {window} | {route} | '
          f'{statistics.median(f):.3f} | {min(f):.3f} | '
          f'{statistics.median(fb):.3f} | {min(fb):.3f} - {max(fb):.3f} | '
          f'{peak[route]:.0f} |', flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=3)
  ap.add_argument('--limit', type=float, default=300.,
                  help='seconds each case may take')
  ap.add_argument('--case', default='', help='T,C,window: run one case here')
  args = ap.parse_args()
  if args.case:
    t, c, window = map(int, args.case.split(','))
    case(t, c, window, args.rounds, args.iters)
    return
  print(f'B={B} N={N} H={H}, uniform random cluster ids; {args.rounds} rounds '
        f'x {args.iters} iters, ms')
  print('| T | C | window | route | fwd median | fwd min | fwd+bwd median | '
        'fwd+bwd min - max | peak MB |')
  print('|---|---|---|---|---|---|---|---|---|', flush=True)
  for t in LENGTHS:
    for c in CLUSTERS:
      for window in (t // c, 2 * t // c):
        subprocess.run(
            [sys.executable, os.path.abspath(__file__), '--case',
             f'{t},{c},{window}', '--rounds', str(args.rounds), '--iters',
             str(args.iters)], check=True, timeout=args.limit)


if __name__ == '__main__':
  main()
