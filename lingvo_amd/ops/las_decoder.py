"""Fused LAS attention-decoder recurrence (teacher-forced training path).

Wraps the las_decoder.hip kernels in a single autograd.Function over the
WHOLE L-step recurrence:
  - forward: per step, two fused small-M GEMM+LSTM stages, one q
    projection and one fused attention kernel (6 launches/step vs ~12
    library calls, each kernel sized to fill the chip instead of the
    ~10-workgroup library GEMMs that made the loop latency-bound).
  - backward: reverse sweep with the same small-M GEMMs for data grads,
    then ALL weight gradients batched over the L steps into three large
    hipBLASLt GEMMs (the reference accumulates per-step wgrads; summing
    over time first is algebraically identical).

Reference semantics: lingvo/tasks/asr/decoder.py teacher-forced LAS
loop; decode one-step einsums batch_major_attention.py:920,1069.

The routes (attend_route, step_route) are described at decoder_recurrence;
every step route has its own forward loop and backward sweep below. They take
operands in bundles: weights (w1t, wm1t, wqt, b1_b) forward and (wq_b, wm1_b,
w_cm0_b) backward, attn (enc_b, pad_f, scale), cell (fgb, cap).
"""

from __future__ import annotations

import collections
import math

import torch

from lingvo_amd.ops import _loader

# What forward saves after its six inputs, all [L,B,*].
_Saved = collections.namedtuple(
    '_Saved', 'gates0 gates1 qs c0s m0s c1s m1s ctxs probs ctx32s')


def _fused_fwd_loop(ext, eg_t, weights, attn, cell, gates0, gates1, qs):
  """'fused' step route, four launches per step: each LSTM layer as one
  launch (both GEMM halves, the bias / embedding term and the cell) into rows
  of the [L,B,*] stacks. The first step skips the K ranges of the missing
  previous state."""
  (w1t, wm1t, wqt, b1_b), (enc_b, pad_f, scale), (fgb, cap) = \
      weights, attn, cell
  L, B, G4 = gates0.shape
  H, D, S = G4 // 4, qs.shape[-1], enc_b.shape[1]
  new = lambda n, dtype=torch.bfloat16: torch.empty(
      L, B, n, dtype=dtype, device=gates0.device)
  c0_st, m0_st, c1_st, m1_st, ctx_st = new(H), new(H), new(H), new(H), new(D)
  ctx32_st, probs_st = new(D, torch.float32), new(S, torch.float32)
  for t in range(L):
    prev = lambda st: st[t - 1] if t > 0 else None
    ext.las_step_fwd(prev(ctx_st), prev(m0_st), w1t, eg_t[t], prev(c0_st),
                     gates0[t], c0_st[t], m0_st[t], fgb, cap)
    ext.las_step_fwd(m0_st[t], prev(m1_st), wm1t, b1_b, prev(c1_st),
                     gates1[t], c1_st[t], m1_st[t], fgb, cap)
    ext.smallm_gemm(m1_st[t], wqt, None, qs[t], H, 0, 1.0, 0)
    ext.attend_step_fwd(qs[t], enc_b, pad_f, scale, probs_st[t], ctx_st[t],
                        ctx32_st[t])
  return dict(c0s=c0_st, m0s=m0_st, c1s=c1_st, m1s=m1_st, ctxs=ctx_st,
              probs=probs_st, ctx32s=ctx32_st)


def _split_fwd_loop(ext, eg_t, weights, attn, cell, gates0, gates1, qs,
                    src_dim, deferred):
  """'split' step route, 8 launches per step: one op per GEMM and cell, with
  either attention route ('accumulate' has no fp32 context)."""
  (w1t, wm1t, wqt, b1_b), (enc_b, pad_f, scale), (fgb, cap) = \
      weights, attn, cell
  L, B, G4 = gates0.shape
  H, D, S = G4 // 4, qs.shape[-1], enc_b.shape[1]
  dt, dev = torch.bfloat16, gates0.device
  c0s, m0s, c1s, m1s, ctxs, probs_l = [], [], [], [], [], []
  c0 = m0 = c1 = m1 = torch.zeros(B, H, dtype=dt, device=dev)
  ctxv = torch.zeros(B, D, dtype=dt, device=dev)
  if deferred:
    ctx_st = torch.empty(L, B, D, dtype=dt, device=dev)
    ctx32_st = torch.empty(L, B, D, dtype=torch.float32, device=dev)
    probs_st = torch.empty(L, B, S, dtype=torch.float32, device=dev)
  for t in range(L):
    g0 = gates0[t]
    ext.smallm_gemm(ctxv, w1t, eg_t[t], g0, src_dim, 0, 1.0, 2)
    ext.smallm_gemm(m0, w1t, None, g0, H, src_dim, 1.0, 3)
    c0, m0 = ext.lstm_gates_fwd(g0, c0, fgb, cap)
    g1 = gates1[t]
    ext.smallm_gemm(m0, wm1t, b1_b, g1, H, 0, 1.0, 1)
    ext.smallm_gemm(m1, wm1t, None, g1, H, H, 1.0, 3)
    c1, m1 = ext.lstm_gates_fwd(g1, c1, fgb, cap)
    q = qs[t]
    ext.smallm_gemm(m1, wqt, None, q, H, 0, 1.0, 0)
    if deferred:
      ctxv = ctx_st[t]
      ext.attend_step_fwd(q, enc_b, pad_f, scale, probs_st[t], ctxv,
                          ctx32_st[t])
    else:
      p, ctxv = ext.attend_fwd(q, enc_b, pad_f, scale)
      ctxs.append(ctxv)
      probs_l.append(p)
    for st, v in zip((c0s, m0s, c1s, m1s), (c0, m0, c1, m1)):
      st.append(v)
  if not deferred:
    ctx_st = torch.stack(ctxs)              # [L, B, D]
    probs_st = torch.stack(probs_l)
    ctx32_st = torch.empty(0, device=dev)
  return dict(c0s=torch.stack(c0s), m0s=torch.stack(m0s),
              c1s=torch.stack(c1s), m1s=torch.stack(m1s), ctxs=ctx_st,
              probs=probs_st, ctx32s=ctx32_st)


def _fused_bwd_sweep(ext, dctx_parts, dm1_parts, saved, weights, attn, cell,
                     src_dim, dctx_st, dl_st, dqs, dgates0, dgates1):
  """Reverse sweep of the 'fused' step route: four launches per step.

  The dc carries and the dm1 carry live in fp32 [B,H] scratch that the
  kernels update; the step processed first takes "no carry" as a flag, not
  a zero fill. dcm's two halves are read in place as strided views."""
  gates0, gates1, c0s, c1s = saved.gates0, saved.gates1, saved.c0s, saved.c1s
  probs, ctx32s = saved.probs, saved.ctx32s
  (wq_b, wm1_b, w_cm0_b), (enc_b, _, scale), (fgb, cap) = weights, attn, cell
  L, B, G4 = gates0.shape
  H = G4 // 4
  f32 = dict(dtype=torch.float32, device=gates0.device)
  dc0, dc1, dm1_carry = (torch.empty(B, H, **f32) for _ in range(3))
  dcm = torch.empty(B, src_dim + H, dtype=torch.bfloat16,
                    device=gates0.device)
  dctx_carry, dm0_carry = dcm[:, :src_dim], dcm[:, src_dim:]
  for t in range(L - 1, -1, -1):
    carry = t < L - 1
    ext.attend_step_bwd(dctx_parts[t], dctx_carry if carry else None,
                        probs[t], ctx32s[t], enc_b, scale, dctx_st[t],
                        dl_st[t], dqs[t])
    # dgates1[t] from dm1 = dq @ wq^T + out grad + carry.
    ext.las_cell_bwd(dqs[t], wq_b, dm1_parts[t],
                     dm1_carry if carry else None, gates1[t],
                     c1s[t - 1] if t > 0 else None, dc1, carry, dgates1[t],
                     None, fgb, cap)
    # dgates1[t] @ wm1^T: columns < H are dm0 (-> dgates0[t]), the rest is
    # the next dm1 carry.
    ext.las_cell_bwd(dgates1[t], wm1_b, dm0_carry if carry else None, None,
                     gates0[t], c0s[t - 1] if t > 0 else None, dc0, carry,
                     dgates0[t], dm1_carry, fgb, cap)
    ext.smallm_gemm(dgates0[t], w_cm0_b, None, dcm, G4, 0, 1.0, 0)


def _split_bwd_sweep(ext, dctx_parts, dm1_parts, saved, weights, attn, cell,
                     src_dim, dctx_st, dl_st, dqs, dgates0, dgates1, deferred,
                     denc):
  """Reverse sweep of the 'split' step route: one op per stage (12 launches
  per step), bf16 carries between them. The deferred attention route fills
  dctx_st / dl_st; 'accumulate' adds every step's increment into denc."""
  gates0, gates1, c0s, c1s = saved.gates0, saved.gates1, saved.c0s, saved.c1s
  qs, probs, ctx32s = saved.qs, saved.probs, saved.ctx32s
  (wq_b, wm1_b, w_cm0_b), (enc_b, _, scale), (fgb, cap) = weights, attn, cell
  L, B, G4 = gates0.shape
  H, D = G4 // 4, qs.shape[-1]
  bf16 = dict(dtype=torch.bfloat16, device=gates0.device)
  zeros_h = torch.zeros(B, H, **bf16)
  # deferred: the dcm[:, :src_dim] view, added inside attend_step_bwd.
  dctx_carry = None if deferred else torch.zeros(B, D, **bf16)
  dm0_carry = dm1_carry = zeros_h
  dc0_carry = dc1_carry = None
  dmm = torch.empty(B, 2 * H, **bf16)
  dcm = torch.empty(B, src_dim + H, **bf16)
  dm1_total = torch.empty(B, H, **bf16)
  for t in range(L - 1, -1, -1):
    if deferred:
      dq = dqs[t]
      ext.attend_step_bwd(dctx_parts[t], dctx_carry, probs[t], ctx32s[t],
                          enc_b, scale, dctx_st[t], dl_st[t], dq)
    else:
      dctx_total = dctx_parts[t] + dctx_carry
      dq = ext.attend_bwd(dctx_total, probs[t], qs[t], enc_b, denc,
                          scale)[0]
      dqs[t] = dq
    pre_m1 = dm1_parts[t] + dm1_carry
    # dm1_total = dq @ wq^T + (out grad + carry)
    ext.smallm_gemm(dq, wq_b, pre_m1, dm1_total, D, 0, 1.0, 2)
    c1_prev = c1s[t - 1] if t > 0 else zeros_h
    dg1, dc1_carry = ext.lstm_gates_bwd(
        gates1[t], c1_prev, c1s[t], dm1_total, dc1_carry, fgb, cap)
    dgates1[t] = dg1
    ext.smallm_gemm(dg1, wm1_b, None, dmm, G4, 0, 1.0, 0)
    dm0_total = (dmm[:, :H] + dm0_carry).contiguous()
    c0_prev = c0s[t - 1] if t > 0 else zeros_h
    dg0, dc0_carry = ext.lstm_gates_bwd(
        gates0[t], c0_prev, c0s[t], dm0_total, dc0_carry, fgb, cap)
    dgates0[t] = dg0
    ext.smallm_gemm(dg0, w_cm0_b, None, dcm, G4, 0, 1.0, 0)
    dctx_carry = dcm[:, :src_dim]
    if not deferred:
      dctx_carry = dctx_carry.contiguous()
    dm0_carry = dcm[:, src_dim:].contiguous()
    dm1_carry = dmm[:, H:].contiguous()


class _DecoderRecurrenceFn(torch.autograd.Function):

  @staticmethod
  def forward(ctx, emb_gates, w_cm0, b1, wm1, wq, enc, enc_pad, fgb, cap,
              src_dim, deferred, fused):
    ext = _loader.get_ext(required=True)
    B, L, G4 = emb_gates.shape
    D = wq.shape[1]
    scale = 1.0 / math.sqrt(D)
    dt = torch.bfloat16
    emb_gates_b = emb_gates.to(dt).contiguous()
    enc_b = enc.to(dt).contiguous()
    pad_f = enc_pad.float().contiguous()
    w1t = w_cm0.t().contiguous().to(dt)      # [4H, src+H]
    wm1t = wm1.t().contiguous().to(dt)       # [4H, 2H]
    wqt = wq.t().contiguous().to(dt)         # [D, H]
    b1_b = b1.to(dt).contiguous()

    dev = enc.device
    gates0 = torch.empty(L, B, G4, dtype=dt, device=dev)
    gates1 = torch.empty(L, B, G4, dtype=dt, device=dev)
    qs = torch.empty(L, B, D, dtype=dt, device=dev)
    # One [L,B,4H] copy up front instead of a per-step .contiguous().
    eg_t = emb_gates_b.permute(1, 0, 2).contiguous()
    args = (ext, eg_t, (w1t, wm1t, wqt, b1_b), (enc_b, pad_f, scale),
            (fgb, cap), gates0, gates1, qs)
    stacks = _fused_fwd_loop(*args) if fused else \
        _split_fwd_loop(*args, src_dim, deferred)
    saved = _Saved(gates0=gates0, gates1=gates1, qs=qs, **stacks)
    m1_st, ctx_st = saved.m1s, saved.ctxs
    ctx.save_for_backward(emb_gates_b, w_cm0, wm1, wq, enc_b, pad_f, *saved)
    ctx.cfg = (fgb, cap, src_dim, scale, b1.dtype, enc.dtype,
               emb_gates.dtype, deferred, fused)
    return torch.cat(                         # [B, L, H + D]
        [m1_st.permute(1, 0, 2), ctx_st.permute(1, 0, 2)], dim=-1)

  @staticmethod
  def backward(ctx, dout):
    ext = _loader.get_ext(required=True)
    emb_gates_b, w_cm0, wm1, wq, enc_b, pad_f, *saved = ctx.saved_tensors
    saved = _Saved(*saved)
    gates0, gates1, qs, m0s, m1s, ctxs, probs = (
        saved.gates0, saved.gates1, saved.qs, saved.m0s, saved.m1s,
        saved.ctxs, saved.probs)
    (fgb, cap, src_dim, scale, b1_dtype, enc_dtype, eg_dtype,
     deferred, fused) = ctx.cfg
    L, B, G4 = gates0.shape
    H = G4 // 4
    D = qs.shape[-1]
    S = enc_b.shape[1]
    dt = torch.bfloat16
    dev = dout.device
    dout = dout.to(dt)
    w_cm0_b = w_cm0.to(dt).contiguous()       # [src+H, 4H] = Wt for dX
    wm1_b = wm1.to(dt).contiguous()           # [2H, 4H]
    wq_b = wq.to(dt).contiguous()             # [H, D]

    dctx_st = dl_st = denc = None
    if deferred:
      dctx_st = torch.empty(L, B, D, dtype=dt, device=dev)
      dl_st = torch.empty(L, B, S, dtype=torch.float32, device=dev)
    else:
      denc = torch.zeros(B, S, D, dtype=torch.float32, device=dev)
    dgates0 = torch.empty(L, B, G4, dtype=dt, device=dev)
    dgates1 = torch.empty(L, B, G4, dtype=dt, device=dev)
    dqs = torch.empty(L, B, D, dtype=dt, device=dev)
    dout_t = dout.permute(1, 0, 2)
    dm1_parts = dout_t[:, :, :H].contiguous()   # [L, B, H]
    dctx_parts = dout_t[:, :, H:].contiguous()  # [L, B, D]
    args = (ext, dctx_parts, dm1_parts, saved, (wq_b, wm1_b, w_cm0_b),
            (enc_b, pad_f, scale), (fgb, cap), src_dim, dctx_st, dl_st, dqs,
            dgates0, dgates1)
    if fused:
      _fused_bwd_sweep(*args)
    else:
      _split_bwd_sweep(*args, deferred, denc)

    # Batched weight grads over all timesteps (identical to per-step
    # accumulation since wgrads sum over t).
    prev = lambda st: torch.cat([torch.zeros_like(st[:1]), st[:-1]])
    x0 = torch.cat([prev(ctxs), prev(m0s)], dim=-1).reshape(L * B, -1)
    dw_cm0 = (x0.t() @ dgates0.reshape(L * B, G4)).to(w_cm0.dtype)
    x1 = torch.cat([m0s, prev(m1s)], dim=-1).reshape(L * B, -1)
    dwm1 = (x1.t() @ dgates1.reshape(L * B, G4)).to(wm1.dtype)
    db1 = dgates1.float().sum(dim=(0, 1)).to(b1_dtype)
    dwq = (m1s.reshape(L * B, H).t() @ dqs.reshape(L * B, D)).to(wq.dtype)
    demb_gates = dgates0.permute(1, 0, 2).to(eg_dtype)
    if deferred:
      denc = torch.empty(
          B, S, D, device=dev,
          dtype=dt if enc_dtype == torch.bfloat16 else torch.float32)
      ext.attend_denc(dl_st, probs, qs, dctx_st, denc)
    return (demb_gates, dw_cm0, db1, dwm1, dwq, denc.to(enc_dtype),
            None, None, None, None, None, None)


def decoder_recurrence(emb_gates: torch.Tensor, w_cm0: torch.Tensor,
                       b1: torch.Tensor, wm1: torch.Tensor,
                       wq: torch.Tensor, enc: torch.Tensor,
                       enc_pad: torch.Tensor, fgb: float, cap: float,
                       src_dim: int,
                       attend_route: str = 'auto',
                       step_route: str = 'auto') -> torch.Tensor:
  """Teacher-forced 2-layer LSTM + dot-attention decoder over L steps.

  emb_gates [B,L,4H]: per-step precomputed gate contribution of the
  token embedding INCLUDING the layer-0 bias. w_cm0 [(src+H), 4H],
  wm1 [2H, 4H], b1 [4H], wq [H, src]. Returns [B, L, H + src]
  (cat of m1 and attention context per step).

  attend_route: 'deferred' reads enc once per step and forms dEnc in one
  kernel after the loop; 'accumulate' adds every step's increment into an
  fp32 dEnc buffer; 'auto' is 'deferred'.

  step_route: 'fused' runs each LSTM layer of a step as one launch (both
  GEMM halves and the cell, las_step.hip) and the backward cell stages with
  their data-gradient GEMMs as prologue, with fp32 carries; 'split' is one
  op per GEMM, cell and add. 'fused' needs the deferred attention route and
  H % 32 == 0, src_dim % 32 == 0 (every K range a multiple of the MFMA
  k-step); 'auto' picks it where those hold and 'split' elsewhere."""
  if attend_route not in ('auto', 'deferred', 'accumulate'):
    raise ValueError(f'unknown attend_route {attend_route!r}')
  if step_route not in ('auto', 'fused', 'split'):
    raise ValueError(f'unknown step_route {step_route!r}')
  deferred = attend_route != 'accumulate'
  H = emb_gates.shape[-1] // 4
  fused_ok = deferred and H % 32 == 0 and src_dim % 32 == 0
  if step_route == 'fused' and not fused_ok:
    raise ValueError(
        "step_route='fused' needs the deferred attend_route and "
        f'H % 32 == 0, src_dim % 32 == 0 (H={H}, src_dim={src_dim})')
  fused = fused_ok and step_route != 'split'
  return _DecoderRecurrenceFn.apply(emb_gates, w_cm0, b1, wm1, wq, enc,
                                    enc_pad, fgb, cap, src_dim, deferred,
                                    fused)
