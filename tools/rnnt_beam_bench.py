"""Transducer beam search microbenchmark: the HIP route next to the twin on
the GPU, and the kernels launch by launch.

  python tools/rnnt_beam_bench.py [--rounds 5] [--iters 3] [--shapes 16,300]
                                  [--beam 8] [--token-beam 8] [--symbols 3]
                                  [--joint 640] [--vocab 1024] [--no-twin]

Times, on bf16 enc_p [B,T,J] with lengths in [0.8 T, T], joint_w [J,V] and a
one-layer LSTM prediction network of the Conformer-L transducer's sizes
(emb 128, cell 640):
  search auto   ops.rnnt.rnnt_beam_search(impl='auto'): the kernels of
                ops/hip/rnnt_beam.hip plus the torch gathers and pred_fn
  search torch  impl='torch' on the GPU (the twin; host-driven), once
  pred_fn       one prediction-network step for B*W rows
  joint top     rnnt_joint_prune_kernel with the top-C lists
  joint blank   the same launch on the last level (blank alone)
  expand, close rnnt_expand_kernel, rnnt_close_kernel
The default shape is the Conformer-L transducer's decode batch (16 x 1200
frames / 4). Each shape runs in a child process of its own under a time
limit; the variants are interleaved round by round, each timed span ends in
a device synchronise, and the per-variant median and min over the rounds
are printed. The single launches are timed as a train of `--train` launches
per span. A shape that fails or runs out of time ends the run.
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


def run_shape(shape, args):
  import torch
  from lingvo_amd.models import asr
  from lingvo_amd.ops import _loader
  if not torch.cuda.is_available():
    raise RuntimeError('rnnt_beam_bench: needs a GPU')
  b, t = shape
  w, c, s, j, v = args.beam, args.token_beam, args.symbols, args.joint, \
      args.vocab
  torch.manual_seed(0)
  dec_p = asr.TransducerDecoder.Params().Set(
      name='dec', vocab_size=v, emb_dim=128, rnn_cell_dim=640, source_dim=512,
      joint_dim=j, dropout_prob=0.0, max_symbols_per_frame=s,
      beam_impl='auto', beam_token_beam=c, fprop_dtype=torch.bfloat16)
  dec = dec_p.Instantiate().cuda()
  dec.eval()
  twin = dec_p.Copy().Set(beam_impl='torch').Instantiate().cuda()
  twin.load_state_dict(dec.state_dict())
  twin.eval()
  theta = dec.theta
  enc = torch.randn(b, t, 512, device='cuda')
  lengths = torch.randint(int(0.8 * t), t + 1, (b,)).cuda()
  pad = (torch.arange(t, device='cuda')[None, :] >= lengths[:, None]).float()
  enc_p = dec.enc_proj.FProp(theta.enc_proj, enc.bfloat16()).contiguous()
  ext = _loader.get_ext(required=True)
  ws = ext.rnnt_beam_init(lengths, t, v, w, c, s)
  wt = theta.softmax.linear_w.t().contiguous()
  bias = theta.softmax.bias.float()
  tok = torch.zeros(b * w, dtype=torch.long, device='cuda')
  cells = dec._InitStates(b * w, 'cuda')
  pred_p = dec.pred_proj.FProp(
      theta.pred_proj, dec._PredictionStep(theta, tok, cells)[0]).contiguous()

  def Train(fn):
    def Run():
      for _ in range(args.train):
        fn()
    return Run

  variants = {
      'search auto': lambda: dec.BeamSearchDecode(theta, enc, pad,
                                                  num_hyps=w),
      'pred_fn': Train(lambda: dec.pred_proj.FProp(
          theta.pred_proj, dec._PredictionStep(theta, tok, cells)[0])),
      'joint top': Train(lambda: ext.rnnt_beam_joint(
          enc_p, 0, pred_p, wt, bias, ws, 0, True)),
      'joint blank': Train(lambda: ext.rnnt_beam_joint(
          enc_p, 0, pred_p, wt, bias, ws, 0, False)),
      'expand': Train(lambda: ext.rnnt_beam_expand(ws, lengths, 0, 0, s, t,
                                                   0)),
      'close': Train(lambda: ext.rnnt_beam_close(ws, lengths, 0, s, t)),
  }
  per = {name: 1 if name.startswith('search') else args.train
         for name in variants}
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
        times[name].append(
            (time.perf_counter() - t0) / args.iters / per[name] * 1e3)
    print(f'transducer beam search, bf16, B={b} T={t} J={j} V={v} W={w} '
          f'C={c} S={s}, {args.rounds} rounds x {args.iters} iters (ms; '
          f'single launches per launch, trains of {args.train})')
    for name, ts in times.items():
      print(f'  {name:12s} median {statistics.median(ts):9.4f}  '
            f'min {min(ts):9.4f}', flush=True)
    if not args.no_twin:
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      twin.BeamSearchDecode(twin.theta, enc, pad, num_hyps=w)
      torch.cuda.synchronize()
      print(f'  search torch once   {(time.perf_counter() - t0) * 1e3:9.1f}',
            flush=True)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--shapes', nargs='+', default=['16,300'],
                  help='B,T per shape.')
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--iters', type=int, default=3)
  ap.add_argument('--train', type=int, default=50)
  ap.add_argument('--beam', type=int, default=8)
  ap.add_argument('--token-beam', type=int, default=8)
  ap.add_argument('--symbols', type=int, default=3)
  ap.add_argument('--joint', type=int, default=640)
  ap.add_argument('--vocab', type=int, default=1024)
  ap.add_argument('--no-twin', action='store_true')
  ap.add_argument('--timeout', type=int, default=400,
                  help='Seconds each shape may take.')
  ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
  args = ap.parse_args()
  if args.child:
    run_shape([int(x) for x in args.child.split(',')], args)
    return
  for shape in args.shapes:
    cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable,
           os.path.abspath(__file__), '--child', shape]
    for flag in ('rounds', 'iters', 'train', 'beam', 'token_beam', 'symbols',
                 'joint', 'vocab'):
      cmd += ['--' + flag.replace('_', '-'), str(getattr(args, flag))]
    rc = subprocess.run(cmd + (['--no-twin'] if args.no_twin else [])).returncode
    if rc != 0:
      print(f'rnnt_beam_bench: shape {shape} ended with status {rc}; '
            f'stopping', file=sys.stderr)
      sys.exit(rc)


if __name__ == '__main__':
  main()
