"""Attention-decoder step microbenchmark: the accumulate route's kernels
(attend_fwd, attend_bwd) against the deferred route's (attend_step_fwd,
attend_step_bwd, attend_denc), and the whole decoder_recurrence with either
route; smallm_gemm at the eight call shapes of a split decoder step; the
fused stage kernels (las_step_fwd, las_cell_bwd) per rows-per-workgroup
against the launches they replace; and the whole recurrence with step_route
split against fused.

  python tools/las_decoder_bench.py [--rounds 5] [--iters 3]
                                    [--B 512 --S 300 --D 512 --L 64 --H 640]
                                    [--only attend|gemm|stages|routes]

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


def _time_table(title, head, fns, args, flop=None):
  """Median / min / spread of interleaved routes; flop: name -> FLOP."""
  times = _time_routes(fns, args.rounds, args.iters)
  print(title)
  print(f'| {head} | ms med | ms min | spread | TFLOP/s |')
  print('|---|---|---|---|---|')
  for name, ts in times.items():
    med = statistics.median(ts)
    rate = f'{flop[name] / (med * 1e-3) / 1e12:.1f}' if flop else ''
    print(f'| {name} | {med:.4f} | {min(ts):.4f} | {max(ts) - min(ts):.4f} '
          f'| {rate} |', flush=True)


def _gemm_shapes(args):
  """(K, N) of the eight smallm_gemm calls of one split decoder step."""
  D, H = args.D, args.H
  return [('fwd ctx->g0', D, 4 * H), ('fwd m0->g0', H, 4 * H),
          ('fwd m0->g1', H, 4 * H), ('fwd m1->g1', H, 4 * H),
          ('fwd m1->q', H, D), ('bwd dq->dm1', D, H),
          ('bwd dg1->dmm', 4 * H, 2 * H), ('bwd dg0->dcm', 4 * H, D + H)]


def bench_gemm_shapes(args):
  import torch
  from lingvo_amd.ops import _loader
  ext = _loader.get_ext(required=True)
  B, bf = args.B, torch.bfloat16
  g = torch.Generator(device='cuda').manual_seed(2)
  rnd = lambda *s: torch.randn(*s, device='cuda', generator=g).to(bf)
  fns, flop = {}, {}
  for name, k, n in _gemm_shapes(args):
    a, wt = rnd(B, k), rnd(n, k)
    out = torch.empty(B, n, dtype=bf, device='cuda')
    key = f'{name} K={k} N={n}'
    fns[key] = (lambda a=a, wt=wt, out=out, k=k: ext.smallm_gemm(
        a, wt, None, out, k, 0, 1.0, 0))
    flop[key] = 2.0 * B * k * n
  _time_table(f'smallm_gemm at the step shapes, M={B}', 'call', fns, args,
              flop)


def bench_stages(args):
  """The fused stage kernels per rows-per-workgroup against the launches of
  the split route they replace, on the same buffers."""
  import torch
  from lingvo_amd.ops import _loader
  ext = _loader.get_ext(required=True)
  B, D, H, bf = args.B, args.D, args.H, torch.bfloat16
  g = torch.Generator(device='cuda').manual_seed(3)
  rnd = lambda *s, sc=1.0: (torch.randn(*s, device='cuda', generator=g) * sc
                            ).to(bf)
  f32 = lambda *s: torch.randn(*s, device='cuda', generator=g)
  ctx, m0, m1, c_prev = rnd(B, D), rnd(B, H), rnd(B, H), rnd(B, H)
  w1t, wm1t = rnd(4 * H, D + H, sc=0.03), rnd(4 * H, 2 * H, sc=0.03)
  eg, b1 = rnd(B, 4 * H), rnd(4 * H)
  gates = torch.empty(B, 4 * H, dtype=bf, device='cuda')
  c_out, m_out = torch.empty_like(c_prev), torch.empty_like(c_prev)

  def split_l0():
    ext.smallm_gemm(ctx, w1t, eg, gates, D, 0, 1.0, 2)
    ext.smallm_gemm(m0, w1t, None, gates, H, D, 1.0, 3)
    ext.lstm_gates_fwd(gates, c_prev, 1.0, 10.0)

  def split_l1():
    ext.smallm_gemm(m0, wm1t, b1, gates, H, 0, 1.0, 1)
    ext.smallm_gemm(m1, wm1t, None, gates, H, H, 1.0, 3)
    ext.lstm_gates_fwd(gates, c_prev, 1.0, 10.0)

  fns = {'layer 0 split (3 launches)': split_l0}
  for rows in (32, 64, 128):
    fns[f'layer 0 las_step_fwd rows={rows}'] = (
        lambda rows=rows: ext.las_step_fwd(ctx, m0, w1t, eg, c_prev, gates,
                                           c_out, m_out, 1.0, 10.0, rows))
  fns['layer 1 split (3 launches)'] = split_l1
  for rows in (32, 64, 128):
    fns[f'layer 1 las_step_fwd rows={rows}'] = (
        lambda rows=rows: ext.las_step_fwd(m0, m1, wm1t, b1, c_prev, gates,
                                           c_out, m_out, 1.0, 10.0, rows))
  _time_table(f'forward stage, B={B} H={H} src={D}', 'stage', fns, args)

  gates.copy_(rnd(B, 4 * H))
  c1 = ext.lstm_gates_fwd(gates, c_prev, 1.0, 10.0)[0]
  dq, dg1 = rnd(B, D, sc=0.1), rnd(B, 4 * H, sc=0.1)
  wq_b, wm1_b = rnd(H, D, sc=0.05), rnd(2 * H, 4 * H, sc=0.03)
  dm1_part, dm_carry_b, dc_b = rnd(B, H), rnd(B, H), rnd(B, H)
  dcm = rnd(B, D + H)
  dm_total = torch.empty(B, H, dtype=bf, device='cuda')
  dmm = torch.empty(B, 2 * H, dtype=bf, device='cuda')
  dgates = torch.empty(B, 4 * H, dtype=bf, device='cuda')
  dm1_f, dc_f, pass_f = f32(B, H), f32(B, H), f32(B, H)

  def split_b1():
    pre = dm1_part + dm_carry_b
    ext.smallm_gemm(dq, wq_b, pre, dm_total, D, 0, 1.0, 2)
    dg, _ = ext.lstm_gates_bwd(gates, c_prev, c1, dm_total, dc_b, 1.0, 10.0)
    dgates.copy_(dg)

  def split_b0():
    ext.smallm_gemm(dg1, wm1_b, None, dmm, 4 * H, 0, 1.0, 0)
    dm0 = (dmm[:, :H] + dcm[:, D:].contiguous()).contiguous()
    dg, _ = ext.lstm_gates_bwd(gates, c_prev, c1, dm0, dc_b, 1.0, 10.0)
    dgates.copy_(dg)
    dmm[:, H:].contiguous()

  fns = {'layer 1 bwd split (4 launches)': split_b1}
  for rows in (32, 64, 128):
    fns[f'layer 1 las_cell_bwd rows={rows}'] = (
        lambda rows=rows: ext.las_cell_bwd(dq, wq_b, dm1_part, dm1_f, gates,
                                           c_prev, dc_f, True, dgates, None,
                                           1.0, 10.0, rows))
  fns['layer 0 bwd split (6 launches)'] = split_b0
  for rows in (32, 64, 128):
    fns[f'layer 0 las_cell_bwd rows={rows}'] = (
        lambda rows=rows: ext.las_cell_bwd(dg1, wm1_b, dcm[:, D:], None,
                                           gates, c_prev, dc_f, True, dgates,
                                           pass_f, 1.0, 10.0, rows))
  _time_table(f'backward stage, B={B} H={H} src={D}', 'stage', fns, args)


def bench_step_routes(args):
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
                                         step_route=route)
    out.backward(w)

  fns = {r: (lambda r=r: run(r)) for r in ('split', 'fused')}
  _time_table(f'decoder_recurrence fwd+bwd, B={B} L={L} S={S} H={H} src={D}',
              'step_route', fns, args)


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
                                         attend_route=route,
                                         step_route='split')
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
  ap.add_argument('--only', choices=('attend', 'gemm', 'stages', 'routes'),
                  help='run one part: the attention kernels and routes, the '
                  'eight smallm_gemm shapes of a step, the fused stage '
                  'kernels, or step_route split against fused')
  args = ap.parse_args()
  if args.only in (None, 'attend'):
    bench_kernels(args)
    if not args.skip_recurrence:
      bench_recurrence(args)
  if args.only in (None, 'gemm'):
    bench_gemm_shapes(args)
  if args.only in (None, 'stages'):
    bench_stages(args)
  if args.only in (None, 'routes') and not args.skip_recurrence:
    bench_step_routes(args)


if __name__ == '__main__':
  main()
