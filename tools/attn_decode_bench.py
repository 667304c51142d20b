"""Cached-attention microbenchmark: the HIP kernels against the composed
twin, and TransformerLm.Generate with either route.

  python tools/attn_decode_bench.py [--rounds 5] [--iters 3]
                                    [--skip-generate] [--skip-kernel-count]

Times ops.attn_decode.cached_attention for impl='hip'
(ops/hip/attn_decode.hip) and impl='torch' (the fp32 composed arithmetic
ExtendStep / StreamStep used before) on a full bf16 cache: one decode step
(C=1, q_start=S-1) at B x S x (N, NKV, H), and a streaming step (C=8,
win_l=64). The routes are interleaved round by round in one process and the
per-route median and min over the rounds are printed, with the K/V bytes the
step has to read divided by the time (at small B*S the cache sits in L2 and
that figure is not an HBM rate). Then tokens/s of a greedy
TransformerLm.Generate on a small LM with decode_impl alternated, and the
number of device kernels one MultiHeadedAttention.ExtendStep launches with
either route.
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..'))

BATCHES = (1, 8, 64)
LENGTHS = (512, 2048, 8192)
HEADS = ((16, 16, 64), (16, 2, 128))
STREAM = dict(C=8, win_l=64, S=2048)


def _time_routes(fns, rounds, iters):
  import torch
  times = {name: [] for name in fns}
  for fn in fns.values():  # warm up
    fn()
  torch.cuda.synchronize()
  for _ in range(rounds):
    for name, fn in fns.items():
      start = torch.cuda.Event(enable_timing=True)
      end = torch.cuda.Event(enable_timing=True)
      start.record()
      for _ in range(iters):
        fn()
      end.record()
      end.synchronize()
      times[name].append(start.elapsed_time(end) / iters)
  return times


def bench_op(rounds, iters):
  import torch
  from lingvo_amd.ops import attn_decode
  print('| B | S | N,NKV,H | C | win_l | hip ms med (min) | torch ms med '
        '(min) | speedup | hip KV TB/s |')
  print('|---|---|---|---|---|---|---|---|---|')
  cases = [(b, s, h, 1, -1) for h in HEADS for b in BATCHES for s in LENGTHS]
  cases += [(b, STREAM['S'], h, STREAM['C'], STREAM['win_l'])
            for h in HEADS for b in BATCHES]
  for b, s, (n, nkv, h), c, win_l in cases:
    g = torch.Generator().manual_seed(0)
    q = torch.randn(b, c, n, h, generator=g).to('cuda', torch.bfloat16)
    kc = torch.randn(b, s, nkv, h, device='cuda').to(torch.bfloat16)
    vc = torch.randn(b, s, nkv, h, device='cuda').to(torch.bfloat16)
    q_start = s - c
    fns = {
        impl: (lambda impl=impl: attn_decode.cached_attention(
            q, kc, vc, q_start, win_l=win_l, impl=impl))
        for impl in ('hip', 'torch')
    }
    times = _time_routes(fns, rounds, iters)
    keys = s if win_l < 0 else min(s, win_l + c)
    kv_bytes = 2 * b * keys * nkv * h * 2
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f'| {b} | {s} | {n},{nkv},{h} | {c} | {win_l} | '
          f'{med["hip"]:.4f} ({min(times["hip"]):.4f}) | '
          f'{med["torch"]:.4f} ({min(times["torch"]):.4f}) | '
          f'{med["torch"] / med["hip"]:.1f}x | '
          f'{kv_bytes / (med["hip"] * 1e-3) / 1e12:.3f} |', flush=True)
    del q, kc, vc


def _set_impl(model, impl):
  from lingvo_amd.layers import attention
  for m in model.modules():
    if isinstance(m, attention.MultiHeadedAttention):
      m.decode_impl = impl


def bench_generate(rounds):
  import torch
  from lingvo_amd.models import lm
  b, prefix_len, max_new = 8, 16, 240
  p = lm.TransformerLm.Params().Set(
      name='lm', vocab_size=1024, model_dim=512, num_layers=4, num_heads=8,
      dropout_prob=0.0, fprop_dtype=torch.bfloat16)
  torch.manual_seed(0)
  model = p.Instantiate().to('cuda').to(torch.bfloat16)
  model.eval()
  prefix = torch.randint(3, 1024, (b, prefix_len), device='cuda')
  times = {'auto': [], 'torch': []}
  for r in range(rounds + 1):
    for impl in times:
      _set_impl(model, impl)
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      ids = model.Generate(model.theta, prefix, max_new, eos_id=-1)
      torch.cuda.synchronize()
      if r:  # round 0 warms up
        times[impl].append(time.perf_counter() - t0)
      assert ids.shape[1] == prefix_len + max_new
  steps = prefix_len + max_new - 1
  print(f'TransformerLm.Generate, 4 layers x 8 heads x 64, B={b}, '
        f'{steps} ExtendSteps per call, {rounds} rounds')
  for impl, ts in times.items():
    med = statistics.median(ts)
    print(f'  decode_impl={impl:5s} median {med * 1e3:8.1f} ms  min '
          f'{min(ts) * 1e3:8.1f} ms  {b * steps / med:9.0f} tokens/s',
          flush=True)


def count_kernels():
  import torch
  from torch.profiler import ProfilerActivity, profile
  from lingvo_amd.layers import attention
  b, d, steps = 8, 1024, 128
  p = attention.MultiHeadedAttention.Params().Set(
      name='mha', input_dim=d, hidden_dim=d, num_heads=16, causal=True,
      fprop_dtype=torch.bfloat16)
  layer = p.Instantiate().to('cuda').to(torch.bfloat16)
  layer.eval()
  x = torch.randn(b, 1, d, device='cuda', dtype=torch.bfloat16)
  for impl in ('auto', 'torch'):
    layer.decode_impl = impl
    st = layer.InitStates(layer.theta, b, steps, 'cuda', torch.bfloat16)
    with torch.no_grad():
      for _ in range(100):
        _, st = layer.ExtendStep(layer.theta, x, st)
      torch.cuda.synchronize()
      with profile(activities=[ProfilerActivity.CPU,
                               ProfilerActivity.CUDA]) as prof:
        _, st = layer.ExtendStep(layer.theta, x, st)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()
             if e.device_type == torch.autograd.DeviceType.CUDA]
    print(f'MultiHeadedAttention.ExtendStep decode_impl={impl}: '
          f'{len(names)} device kernels/copies at t=100')
    for nm in names:
      print(f'    {nm[:100]}')


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=3)
  ap.add_argument('--skip-generate', action='store_true')
  ap.add_argument('--skip-kernel-count', action='store_true')
  args = ap.parse_args()
  bench_op(args.rounds, args.iters)
  if not args.skip_generate:
    bench_generate(args.rounds)
  if not args.skip_kernel_count:
    count_kernels()


if __name__ == '__main__':
  main()
