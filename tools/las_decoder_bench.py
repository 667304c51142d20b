"""Attention-decoder step microbenchmark: the accumulate route's kernels
(attend_fwd, attend_bwd) against the deferred route's (attend_step_fwd,
attend_step_bwd, attend_denc), and the whole decoder_recurrence with either
route.

  python tools/las_decoder_bench.py [--rounds 5] [--iters 3]
                                    [--B 512 --S 300 --D 512 --L 64 --H 640]

Per-call times come from device events around `iters` back-to-back calls;
the routes are interleaved round by round in one process and the median and
min over the rounds are printed. 'moved' is the bytes a call reads and
writes as the kernel is written, 'needed' the bytes the result cannot do
without (enc once per step kernel; for attend_denc its inputs once and its
output once); TB/s is moved bytes over the median time, to be set against
the 6.29 TB/s of a device-to-device copy. Variants 1..4 of the step kernels
are (rows per wave iteration, waves per workgroup) = (4,4) (8,4) (4,8)
(8,8); 0 is what the wrappers pick.
"""

from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                '..'))

COPY_TBS = 6.29


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


def _row(name, ts, moved, needed):
  med = statistics.median(ts)
  tbs = moved / (med * 1e-3) / 1e12
  print(f'| {name} | {med:.4f} | {min(ts):.4f} | {max(ts) - min(ts):.4f} | '
        f'{moved / 1e6:.1f} | {needed / 1e6:.1f} | {tbs:.2f} | '
        f'{100 * tbs / COPY_TBS:.0f}% |', flush=True)


def bench_kernels(args):
  import torch
  from lingvo_amd.ops import _loader
  ext = _loader.get_ext(required=True)
  B, S, D, L = args.B, args.S, args.D, args.L
  dev, bf = 'cuda', torch.bfloat16
  g = torch.Generator(device=dev).manual_seed(0)
  rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
  enc = rnd(B, S, D).to(bf)
  q = rnd(B, D).to(bf)
  dctx = rnd(B, D).to(bf)
  dcm = rnd(B, D + 640).to(bf)
  pad = torch.zeros(B, S, device=dev)
  pad[:, S - S // 8:] = 1.0
  scale = 1.0 / math.sqrt(D)
  probs = torch.empty(B, S, device=dev)
  ctx = torch.empty(B, D, device=dev, dtype=bf)
  ctx32 = torch.empty(B, D, device=dev)
  ext.attend_step_fwd(q, enc, pad, scale, probs, ctx, ctx32)
  denc32 = torch.zeros(B, S, D, device=dev)
  dctx_o = torch.empty(B, D, device=dev, dtype=bf)
  dl = torch.empty(B, S, device=dev)
  dq = torch.empty(B, D, device=dev, dtype=bf)

  enc_b = enc.numel() * 2
  small_f = B * D * 2 + B * S * 8           # q, pad, probs
  small_b = B * D * 6 + B * S * 4           # dctx, q, dq, probs
  print(f'B={B} S={S} D={D}: enc {enc_b / 1e6:.1f} MB, fp32 denc '
        f'{denc32.numel() * 4 / 1e6:.1f} MB, copy {COPY_TBS} TB/s')
  print('| kernel | ms med | ms min | spread | moved MB | needed MB | '
        'TB/s | of copy |')
  print('|---|---|---|---|---|---|---|---|')

  fns = {'attend_fwd': lambda: ext.attend_fwd(q, enc, pad, scale)}
  for v in (0, 1, 2, 3, 4):
    fns[f'attend_step_fwd v{v}'] = (lambda v=v: ext.attend_step_fwd(
        q, enc, pad, scale, probs, ctx, ctx32, v))
  times = _time_routes(fns, args.rounds, args.iters)
  for name, ts in times.items():
    passes = 2 if name == 'attend_fwd' else 1
    _row(name, ts, passes * enc_b + small_f, enc_b + small_f)

  fns = {'attend_bwd': lambda: ext.attend_bwd(dctx, probs, q, enc, denc32,
                                              scale)}
  for v in (0, 1, 2, 3, 4):
    fns[f'attend_step_bwd v{v}'] = (lambda v=v: ext.attend_step_bwd(
        dctx, dcm[:, :D], probs, ctx32, enc, scale, dctx_o, dl, dq, v))
  times = _time_routes(fns, args.rounds, args.iters)
  for name, ts in times.items():
    if name == 'attend_bwd':
      _row(name, ts, 2 * enc_b + 2 * denc32.numel() * 4 + small_b,
           enc_b + small_b)
    else:
      _row(name, ts, enc_b + small_b + B * S * 4, enc_b + small_b)
  del denc32

  dl_st = rnd(L, B, S)
  probs_st = torch.softmax(rnd(L, B, S), -1)
  qs = rnd(L, B, D).to(bf)
  dctx_st = rnd(L, B, D).to(bf)
  out_bf = torch.empty(B, S, D, device=dev, dtype=bf)
  out_32 = torch.empty(B, S, D, device=dev)
  fns = {
      'attend_denc bf16 out': lambda: ext.attend_denc(dl_st, probs_st, qs,
                                                      dctx_st, out_bf),
      'attend_denc fp32 out': lambda: ext.attend_denc(dl_st, probs_st, qs,
                                                      dctx_st, out_32),
  }
  times = _time_routes(fns, args.rounds, args.iters)
  in_b = 2 * L * B * S * 4 + 2 * L * B * D * 2
  flop = 4.0 * L * B * S * D
  for name, ts in times.items():
    out_b = B * S * D * (2 if 'bf16' in name else 4)
    _row(name, ts, in_b + out_b, in_b + out_b)
    print(f'|   ({flop / 1e9:.1f} GFLOP: '
          f'{flop / (statistics.median(ts) * 1e-3) / 1e12:.1f} TFLOP/s fp32) '
          '| | | | | | | |')


def bench_recurrence(args):
  import torch
  from lingvo_amd.ops import las_decoder
  B, S, D, L, H = args.B, args.S, args.D, args.L, args.H
  dev, bf = 'cuda', torch.bfloat16
  g = torch.Generator(device=dev).manual_seed(1)
  rnd = lambda *s, sc=1.0: (torch.randn(*s, device=dev, generator=g) * sc
                            ).to(bf).requires_grad_(True)
  leaves = [rnd(B, L, 4 * H), rnd(D + H, 4 * H, sc=0.03), rnd(4 * H, sc=0.1),
            rnd(2 * H, 4 * H, sc=0.03), rnd(H, D, sc=0.05), rnd(B, S, D)]
  pad = torch.zeros(B, S, device=dev)
  pad[:, S - S // 8:] = 1.0
  w = torch.randn(B, L, H + D, device=dev, generator=g).to(bf)

  def run(route):
    for v in leaves:
      v.grad = None
    out = las_decoder.decoder_recurrence(*leaves, pad, 1.0, 10.0, D,
                                         attend_route=route)
    out.backward(w)

  fns = {r: (lambda r=r: run(r)) for r in ('accumulate', 'deferred')}
  times = _time_routes(fns, args.rounds, args.iters)
  print(f'decoder_recurrence fwd+bwd, B={B} L={L} S={S} H={H} src={D}')
  print('| attend_route | ms med | ms min | spread |')
  print('|---|---|---|---|')
  for name, ts in times.items():
    print(f'| {name} | {statistics.median(ts):.2f} | {min(ts):.2f} | '
          f'{max(ts) - min(ts):.2f} |', flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=3)
  ap.add_argument('--B', type=int, default=512)
  ap.add_argument('--S', type=int, default=300)
  ap.add_argument('--D', type=int, default=512)
  ap.add_argument('--L', type=int, default=64)
  ap.add_argument('--H', type=int, default=640)
  ap.add_argument('--skip-recurrence', action='store_true')
  args = ap.parse_args()
  bench_kernels(args)
  if not args.skip_recurrence:
    bench_recurrence(args)


if __name__ == '__main__':
  main()
