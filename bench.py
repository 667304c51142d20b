"""Flagship benchmark: Librispeech Conformer-L train step (BASELINE.json).

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

Measures whole-job examples/sec for the Conformer-L ASR train step on
synthetic Librispeech-shaped data (random-init weights, bf16 compute),
DP over RCCL/xGMI for N>1. Launched by the driver via
torch.distributed.run for N>1 (one rank per GPU).

Robustness contract: for a single-rank GPU run the measurement executes
in a child process per mode (hipGraph first, eager fallback) so a GPU
memory fault in the captured path degrades to a slower eager number
instead of an rc=134 abort with no JSON. Phase markers go to stderr so a
crash is attributable to model-build / warmup / capture / replay-N.

A plain run does only what the headline figure needs: set up, warm up,
time --steps steps, optionally write --dump-outputs, print the one JSON
result line. Anything beyond that belongs behind --full (nothing does
today: peak memory, the profiler table and the decode measurement are
already opt-in through --memory, --profile and --decode).

--dump-outputs DIR writes what the last timed step computed as float32
DIR/<name>.npy: every metric the step returns (value and weight) and a
fixed, seeded sample of the updated parameters. Inputs, init and dropout
seeds are fixed, so two builds run with the same arguments can be
compared output for output.
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# Pre-tuned hipBLASLt/rocBLAS GEMM algorithm table for gfx950 (torch
# TunableOp; tuned on this pool's MI355X image: +5.5% step throughput
# over the heuristic picks). Read-only unless the user opts into
# re-tuning. Must be set before torch initializes.
_TUNED = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      'tools', 'tunableop_gfx950.csv')
if os.path.exists(_TUNED) and     'PYTORCH_TUNABLEOP_ENABLED' not in os.environ:
  os.environ['PYTORCH_TUNABLEOP_ENABLED'] = '1'
  os.environ['PYTORCH_TUNABLEOP_TUNING'] = '0'
  os.environ['PYTORCH_TUNABLEOP_FILENAME'] = _TUNED


def _phase(msg):
  print(f'# phase: {msg}', file=sys.stderr, flush=True)


def build_argparser():
  ap = argparse.ArgumentParser()
  ap.add_argument('--gpus', type=int, default=1)
  ap.add_argument('--steps', type=int, default=20)
  ap.add_argument('--warmup', type=int, default=5)
  ap.add_argument('--batch', type=int, default=512,
                  help='Per-GPU batch size (512 saturates one MI355X at '
                       'Conformer-L: 921 ex/s vs 674 at 128, using '
                       '~101 of 288 GB HBM; see BASELINE.md sweep).')
  ap.add_argument('--memory', action='store_true',
                  help='Report peak device memory in the JSON config.')
  ap.add_argument('--profile', default=None, metavar='PATH',
                  help='Write a torch.profiler key_averages table for '
                       'a few steps to PATH (after the timed region; '
                       'complements rocprofv3 kernel traces).')
  ap.add_argument('--no-graph', action='store_true',
                  help='Disable hipGraph step capture (eager steps).')
  ap.add_argument('--model', default='asr.librispeech.'
                  'Librispeech960WpmConformerL')
  ap.add_argument('--mode', choices=['auto', 'graph', 'eager'],
                  default='auto',
                  help='auto = child-process graph with eager fallback '
                       '(single rank); graph/eager = run that mode '
                       'inline in this process.')
  ap.add_argument('--decode', action='store_true',
                  help='Measure inference Decode() examples/sec instead '
                       'of the train step (beam width = model '
                       'decode_num_hyps; greedy when 1).')
  ap.add_argument('--decode-hyps', type=int, default=1,
                  help='Beam width for --decode.')
  ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                  help='After the timed steps, write the outputs of the '
                       'last timed step (metrics, and a seeded sample of '
                       'the updated parameters) as float32 DIR/<name>.npy.')
  ap.add_argument('--full', action='store_true',
                  help='Also run the measurements and checks that the '
                       'headline figure does not need. A plain run only '
                       'sets up, warms up, times --steps steps and prints '
                       'the result line; no extra measurement exists '
                       'today, so this currently adds nothing.')
  return ap


def main():
  args = build_argparser().parse_args()
  world = int(os.environ.get('WORLD_SIZE', '1'))
  if args.decode:
    run_decode_bench(args)
    return
  if args.no_graph:
    args.mode = 'eager'

  if args.mode == 'auto' and world == 1:
    import torch
    if not torch.cuda.is_available():
      run_bench(args, world)
      return
    # Orchestrate: run each mode in a child so an asynchronous GPU fault
    # (SIGABRT, uncatchable in-process) falls back instead of killing the
    # bench. The child prints the one JSON line; we relay it.
    base = [sys.executable, os.path.abspath(__file__),
            '--gpus', str(args.gpus), '--steps', str(args.steps),
            '--warmup', str(args.warmup), '--batch', str(args.batch),
            '--model', args.model]
    if args.memory:
      base.append('--memory')
    if args.profile:
      base += ['--profile', args.profile]
    if args.dump_outputs:
      base += ['--dump-outputs', os.path.abspath(args.dump_outputs)]
    if args.full:
      base.append('--full')
    for mode in ('graph', 'eager'):
      _phase(f'launching child mode={mode}')
      proc = subprocess.run(base + ['--mode', mode],
                            stdout=subprocess.PIPE, text=True)
      out = proc.stdout or ''
      json_line = None
      for line in out.splitlines():
        line = line.strip()
        if line.startswith('{') and '"metric"' in line:
          json_line = line
      if json_line is not None:
        # Relay any non-JSON prefix lines for context, then the result.
        for line in out.splitlines():
          if line.strip() != json_line:
            print(line)
        print(json_line, flush=True)
        return
      _phase(f'child mode={mode} rc={proc.returncode} without a result'
             f'{"; falling back to eager" if mode == "graph" else ""}')
    print('# bench: all modes failed', file=sys.stderr, flush=True)
    sys.exit(1)

  run_bench(args, world)


# --dump-outputs budget: any one array above 4M elements (16 MB as
# float32) is stored as a fixed, seeded sample of that size, and the whole
# dump must stay below 64 MB.
_DUMP_SAMPLE_ELEMS = 4 * 1024 * 1024
_DUMP_MAX_BYTES = 64 * 1024 * 1024


def _seeded_sample(flat):
  """`flat` itself when small, else a fixed seeded sample of its elements
  (the same indices for every run with the same element count)."""
  import torch
  if flat.numel() <= _DUMP_SAMPLE_ELEMS:
    return flat
  g = torch.Generator().manual_seed(20240)
  idx = torch.randint(0, flat.numel(), (_DUMP_SAMPLE_ELEMS,), generator=g)
  return flat[idx.to(flat.device)]


def _dump_arrays(dump_dir, named):
  """Writes (name, tensor-or-number) pairs as float32 DIR/<name>.npy."""
  import numpy as np
  import torch
  os.makedirs(dump_dir, exist_ok=True)
  total = 0
  for name, val in named:
    if isinstance(val, torch.Tensor):
      val = val.detach()
      if val.numel() > _DUMP_SAMPLE_ELEMS:
        val = _seeded_sample(val.reshape(-1))
      arr = val.to(torch.float32).cpu().numpy()
    elif isinstance(val, (bool, int, float)):
      arr = np.asarray(val, dtype=np.float32)
    else:
      continue
    total += arr.nbytes
    if total > _DUMP_MAX_BYTES:
      raise RuntimeError(f'--dump-outputs: over {_DUMP_MAX_BYTES} bytes '
                         f'at {name}')
    fname = name.replace('[', '.').replace(']', '').replace('/', '_')
    np.save(os.path.join(dump_dir, fname + '.npy'), arr)
  _phase(f'dumped {total} bytes of outputs to {dump_dir}')


def _step_outputs(task, metrics):
  """What a caller of the train step is left with: the returned metrics
  ((value, weight) per name) and the parameters the step updated, the
  latter flattened in name order and sampled to a fixed size."""
  import torch
  from lingvo_amd.core.nested_map import NestedMap
  named = sorted(task.named_parameters(), key=lambda kv: kv[0])
  flat = torch.cat([prm.detach().reshape(-1).float() for _, prm in named])
  return (NestedMap(metrics).FlattenItems() +
          [('params_sample', _seeded_sample(flat))])


def run_decode_bench(args):
  """Inference decode throughput (decode examples/sec).

  Times AsrModel.Decode() — encoder + autoregressive LSTM-attention
  decode (greedy or beam) — on synthetic batches."""
  _phase('importing torch')
  import torch
  from lingvo_amd.core import registry
  has_gpu = torch.cuda.is_available()
  device = 'cuda:0' if has_gpu else 'cpu'
  _phase('building model')
  model_p = registry.GetParams(args.model, 'Train')
  model_p.input.batch_size = args.batch
  if not has_gpu:
    model_p.task.fprop_dtype = torch.float32
    model_p.input.frame_len = 80
    model_p.task.encoder.num_layers = 1
  model_p.task.random_seed = 1234
  if 'decode_num_hyps' in model_p.task:
    model_p.task.decode_num_hyps = args.decode_hyps
  model = model_p.Instantiate().to(device)
  task = model.GetTask()
  task.eval()
  gen = task.input_generator
  batch = gen.GetPreprocessedInputBatch().Transform(
      lambda t: t.to(device) if isinstance(t, torch.Tensor) else t)
  _phase('decode warmup')
  for _ in range(max(1, args.warmup)):
    out = task.Decode(batch)
  if has_gpu:
    torch.cuda.synchronize()
  t0 = time.perf_counter()
  for i in range(args.steps):
    out = task.Decode(batch)
    if i % 5 == 0:
      _phase(f'decode step {i}')
  if has_gpu:
    torch.cuda.synchronize()
  elapsed = time.perf_counter() - t0
  if args.dump_outputs:
    from lingvo_amd.core.nested_map import NestedMap
    _dump_arrays(args.dump_outputs, NestedMap(out).FlattenItems())
  examples_per_sec = args.batch * args.steps / elapsed
  print(json.dumps({
      'metric': 'decode examples/sec, Librispeech Conformer-L',
      'value': round(examples_per_sec, 3),
      'unit': 'examples/sec',
      'n_gpus': 1, 'steps': args.steps, 'warmup': args.warmup,
      'ms_per_step': round(elapsed / args.steps * 1000.0, 3),
      'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
      'dtype': 'bf16' if has_gpu else 'fp32', 'data': 'synthetic',
      'config': {'model': args.model, 'global_batch': args.batch,
                 'beam': args.decode_hyps,
                 'parallelism': 'dp1'},
  }), flush=True)


def run_bench(args, world):
  _phase('importing torch')
  import torch
  import torch.distributed as dist
  from lingvo_amd.core import registry
  from lingvo_amd.parallel import ddp

  # Keep the NCCL watchdog from probing streams during hipGraph capture
  # (capture falls back to eager if it still objects).
  os.environ.setdefault('TORCH_NCCL_ASYNC_ERROR_HANDLING', '0')
  rank = ddp.InitDistributed()
  local_rank = int(os.environ.get('LOCAL_RANK', '0'))
  has_gpu = torch.cuda.is_available()
  device = f'cuda:{local_rank}' if has_gpu else 'cpu'
  if has_gpu:
    torch.cuda.set_device(device)

  use_graph = args.mode != 'eager' and has_gpu

  _phase('building model')
  model_p = registry.GetParams(args.model, 'Train')
  if not has_gpu:  # CPU smoke of the bench harness only
    args.batch = min(args.batch, 8)
    model_p.task.fprop_dtype = torch.float32
    model_p.input.frame_len = 80
    model_p.task.encoder.num_layers = 1
  model_p.input.batch_size = args.batch
  model_p.task.random_seed = 1234
  model = model_p.Instantiate().to(device)
  task = model.GetTask()
  sync = ddp.GradSync(task) if world > 1 else None
  finalize = sync.Finalize if sync else None

  if world > 1:
    # Per-rank sanity before any timed work: proves the process group is
    # live on this topology and catches rank bring-up bugs before the
    # driver's 8-GPU budget is spent.
    _phase(f'rank sanity: rank={rank}/{world} device={device}')
    t = torch.ones(1, device=device if has_gpu else 'cpu')
    dist.all_reduce(t)
    ok = abs(float(t.item()) - world) < 1e-6
    print(f'# rank {rank}/{world} device={device} allreduce='
          f'{float(t.item())} ok={ok}', file=sys.stderr, flush=True)
    if not ok:
      raise RuntimeError(f'rank {rank}: allreduce sanity failed')

  # Pre-generate a handful of synthetic batches on device. Each DP rank
  # draws a distinct stream (weak scaling: different data per rank).
  _phase('generating synthetic batches')
  gen = task.input_generator
  gen._batch_count = rank * 1009
  batches = []
  for _ in range(4):
    b = gen.GetPreprocessedInputBatch()
    batches.append(b.Transform(
        lambda t: t.to(device) if isinstance(t, torch.Tensor) else t))

  graphed = None
  if use_graph:
    try:
      _phase('hipGraph warmup + capture')
      from lingvo_amd.runtime.graph_step import GraphedTrainStep
      graphed = GraphedTrainStep(task, batches[0], grad_sync=sync)
      if rank == 0:
        print('# using hipGraph-captured train step', flush=True)
    except Exception as e:  # fall back to eager steps
      if rank == 0:
        print(f'# hipGraph capture failed ({e}); eager steps', flush=True)
      graphed = None

  def step(i):
    if graphed is not None:
      return graphed.Step(batches[i % len(batches)])
    return task.TrainStep(batches[i % len(batches)],
                          grad_sync_finalize=finalize)

  for i in range(args.warmup):
    _phase(f'warmup step {i}')
    metrics = step(i)
  if has_gpu:
    torch.cuda.synchronize()
  _phase('warmup done')

  if world > 1:
    dist.barrier()
  if has_gpu:
    torch.cuda.synchronize()
  t0 = time.perf_counter()
  for i in range(args.steps):
    metrics = step(i)
    if i % 5 == 0:
      _phase(f'timed step {i}')
  if has_gpu:
    torch.cuda.synchronize()
  if world > 1:
    dist.barrier()
  elapsed = time.perf_counter() - t0
  _phase('timed region done')

  # MAX step time over ranks == MIN throughput: reduce elapsed as MAX.
  if world > 1:
    e = torch.tensor([elapsed], device=device if has_gpu else 'cpu')
    dist.all_reduce(e, op=dist.ReduceOp.MAX)
    elapsed = float(e.item())

  # Before anything below steps again: `metrics` still holds what the
  # last timed step returned (graph replays overwrite it in place).
  if args.dump_outputs and rank == 0:
    _dump_arrays(args.dump_outputs, _step_outputs(task, metrics))

  peak_mem_gb = None
  if args.memory and has_gpu:
    peak_mem_gb = round(
        torch.cuda.max_memory_allocated(device) / 2**30, 3)

  if args.profile and rank == 0:
    from torch.profiler import profile, ProfilerActivity
    acts = [ProfilerActivity.CPU]
    if has_gpu:
      acts.append(ProfilerActivity.CUDA)
    with profile(activities=acts) as prof:
      for i in range(2):
        step(args.steps + i)
      if has_gpu:
        torch.cuda.synchronize()
    with open(args.profile, 'w') as f:
      f.write(prof.key_averages().table(
          sort_by='cuda_time_total' if has_gpu else 'cpu_time_total',
          row_limit=60))

  ms_per_step = elapsed / args.steps * 1000.0
  global_batch = args.batch * world
  examples_per_sec = global_batch * args.steps / elapsed
  loss = float(metrics['loss'][0].detach())

  if rank == 0:
    out = {
        'metric': 'train step examples/sec (whole node), Librispeech '
                  'Conformer-L',
        'value': round(examples_per_sec, 3),
        'unit': 'examples/sec',
        'n_gpus': world,
        'steps': args.steps,
        'warmup': args.warmup,
        'ms_per_step': round(ms_per_step, 3),
        'higher_is_better': True,
        'scaling': 'weak',
        'vs_baseline': None,
        'dtype': 'bf16' if has_gpu else 'fp32',
        'data': 'synthetic',
        'config': {
            'model': ('Conformer-L (17 blocks, d=512, h=8, kernel 32) + '
                      'LSTM attention decoder'
                      if args.model.endswith('WpmConformerL')
                      else args.model),
            'global_batch': global_batch,
            'seq_len': next(
                (model_p.input.Get(k) for k in
                 ('frame_len', 'seq_len', 'src_len')
                 if k in model_p.input), None),
            'parallelism': f'dp{world}',
            'final_loss': round(loss, 4),
            'step_mode': 'hipgraph' if graphed is not None else 'eager',
            **({'peak_mem_gb': peak_mem_gb}
               if peak_mem_gb is not None else {}),
        },
    }
    print(json.dumps(out), flush=True)
  if world > 1:
    dist.destroy_process_group()


if __name__ == '__main__':
  main()
