"""Host-side wrappers over the C ABI (include/mgx.h): thin launch helpers + torch.autograd glue.

PyTorch is used for device memory, streams and autograd bookkeeping only; every op below runs a
hand-written HIP kernel from libmgx.so on the current HIP stream.  Nothing here falls back to
eager PyTorch: a missing library or a non-CUDA tensor raises.
"""
from __future__ import annotations

from typing import Tuple

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

BF16 = torch.bfloat16


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.MgxError("mgx ops need CUDA/HIP tensors (no CPU fallback); got a CPU tensor")
        if t is not None and not t.is_contiguous():
            raise _lib.MgxError("mgx ops need contiguous tensors")


# --------------------------------------------------------------------------------------------------
# deterministic-reduction mode (include/mgx.h: mgx_set_deterministic)
# --------------------------------------------------------------------------------------------------
_det_scratch = None          # the registered buffer must outlive the mode: kept here
_det_stream_scratch = {}     # stream pointer -> buffer of that stream (mgx_set_deterministic_stream)
_DET_BYTES = _lib.DEFINES["MGX_DET_SCRATCH_BYTES"]     # 16 MiB of sums + 16 MiB of poison words, aligned to its size


def _det_buffer(dev):
    """-> (base tensor to keep alive, 32 MiB-aligned data pointer inside it)"""
    base = torch.empty(2 * _DET_BYTES, dtype=torch.uint8, device=dev)
    return base, base.data_ptr() + (-base.data_ptr()) % _DET_BYTES


def set_deterministic(on: bool = True, device=None) -> None:
    """Switch the library's cross-workgroup sums (dE, vocabulary dW / db, block bias gradients, embedding gradient, loss
    statistics) to order-independent fixed-point integer atomics: repeated runs -- and a data-parallel run against the
    single-process run of the same global batch -- then agree bit for bit on everything the kernels compute.  Costs a few
    percent; ``MGX_DETERMINISTIC=1`` in the environment switches it on when the first model moves to the GPU.  Process-wide.
    The scratch registered here serves ONE stream at a time; the CU-masked side stream of ``configure_streams`` gets a buffer
    of its own (registered here when it exists already, by ``configure_streams`` when it is created later)."""
    global _det_scratch
    lib = _lib.load()
    if not on:
        check(lib.mgx_set_deterministic(None, 0), "mgx_set_deterministic")
        _det_scratch = None
        _det_stream_scratch.clear()
        return
    dev = device if device is not None else torch.device("cuda")
    buf, p = _det_buffer(dev)
    check(lib.mgx_set_deterministic(p, _DET_BYTES), "mgx_set_deterministic")
    _det_scratch = buf
    for plan in _STREAM_PLANS.values():
        _det_register_stream(plan.side)


def _det_register_stream(ms) -> None:
    """deterministic mode on: the masked stream ``ms`` issues calls that use the fixed-point scratch -> give it one of its own"""
    if ms is None or not deterministic() or ms.ptr in _det_stream_scratch:
        return
    buf, p = _det_buffer(ms.device)
    check(_lib.load().mgx_set_deterministic_stream(ms.ptr, p, _DET_BYTES), "mgx_set_deterministic_stream")
    _det_stream_scratch[ms.ptr] = buf


def deterministic() -> bool:
    return bool(_lib.load().mgx_deterministic())


# --------------------------------------------------------------------------------------------------
# CU-masked streams (include/mgx.h: mgx_stream_create_cu_mask) and the two-stream plan of the backward
# --------------------------------------------------------------------------------------------------
class MaskedStream:
    """A HIP stream whose kernels may only run on ``cus`` CUs: logical CUs ``first .. first + cus - 1`` of the driver's
    numbering, which deals consecutive CUs round the XCDs first -- so a run of n (a multiple of 8) is n/8 CUs of every XCD, and
    two disjoint runs are disjoint sets of CUs.  ``.stream`` is the ``torch.cuda.ExternalStream`` over it (events, allocator,
    ``with torch.cuda.stream(...)``), ``.ptr`` the raw ``hipStream_t`` the library's CU-count registry knows."""

    def __init__(self, cus: int, first: int = 0, device=None):
        lib = _lib.load()
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        total = torch.cuda.get_device_properties(self.device).multi_processor_count
        if cus <= 0 or first < 0 or first + cus > total:
            raise ValueError(f"MaskedStream: CUs {first}..{first + cus - 1} do not fit the device's {total}")
        words = (total + 31) // 32
        mask = (ctypes.c_uint32 * words)()
        for i in range(first, first + cus):
            mask[i // 32] |= 1 << (i % 32)
        out = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.mgx_stream_create_cu_mask(ctypes.byref(out), ctypes.cast(mask, ctypes.c_void_p), words), "mgx_stream_create_cu_mask")
        self.ptr, self.cus, self.first = out.value, cus, first
        self.stream = torch.cuda.ExternalStream(self.ptr, device=self.device)

    def close(self, destroy: bool = False):
        """forget the stream.  The HIP stream itself is only destroyed on request: the caching allocator keeps the stream of every
        block that was allocated on it or marked with ``record_stream`` and records an event on it when such a block is freed --
        long after this call, possibly at interpreter shutdown -- so destroying a stream that tensors have touched is a
        use-after-free.  A forgotten stream costs one idle hardware queue."""
        if self.ptr is not None:
            self.stream.synchronize()
            if destroy:
                _det_stream_scratch.pop(self.ptr, None)
                check(_lib.load().mgx_stream_destroy(self.ptr), "mgx_stream_destroy")
            self.ptr = None


_MASKED = {}                 # (device index, first, cus) -> MaskedStream: created once, reused by every later plan


def masked_stream(cus: int, first: int = 0, device=None) -> "MaskedStream":
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (idx, first, cus)
    ms = _MASKED.get(key)
    if ms is None or ms.ptr is None:
        ms = _MASKED[key] = MaskedStream(cus, first, dev)
    return ms


class StreamPlan:
    """``side``: the masked stream of the backward's off-critical-path kernels (dE from the stored dS tiles, the block's weight
    gradients -- they feed only the optimiser); ``main``: the masked stream of everything else (the complement of ``side``
    minus the CUs left to RCCL), or None when the caller's own stream stays unrestricted."""
    __slots__ = ("side", "main", "reserved", "last", "work")

    def __init__(self, side, main, reserved, work=3):
        self.side, self.main, self.reserved, self.last, self.work = side, main, reserved, None, work


_STREAM_PLANS = {}           # device index -> StreamPlan


def configure_streams(side_cus: int = 0, reserve_cus: int = 0, partition: bool = True, device=None, side_work: int = 3):
    """Run the HBM-bound, off-critical-path half of an encoder block's backward (``rel_attn_de_tiles_kernel`` and the grouped
    weight-gradient launch: ~0.8 of a block's ~3 ms at the bench shape, none of it needed before the optimiser step / the
    bucket's all-reduce) on a side stream restricted to ``side_cus`` CUs, BESIDE the MFMA-bound kernels of the critical path
    instead of between them.  ``partition``: also create the main stream, restricted to the other CUs -- run the training step
    inside ``with torch.cuda.stream(ops.main_stream())``; without it the caller's stream keeps the whole chip and the
    dispatcher shares the side stream's CUs between the two.  ``reserve_cus``: CUs (the highest-numbered ones) that neither
    stream may use -- left to RCCL's kernels under data parallelism.  ``side_cus = 0`` with
    ``reserve_cus > 0``: only the main stream, masked.  Both zero: back to one unrestricted stream.  ``side_work``: what goes to
    the side stream -- bit 0 the dE kernel, bit 1 the weight gradients.  Returns the plan (or None)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if _STREAM_PLANS.pop(idx, None) is not None:
        torch.cuda.synchronize(dev)                        # (the plan's streams stay alive in _MASKED: see MaskedStream.close)
    if side_cus <= 0 and reserve_cus <= 0:
        return None
    total = torch.cuda.get_device_properties(dev).multi_processor_count
    if side_cus % 8 or reserve_cus % 8 or side_cus + reserve_cus >= total:
        raise ValueError(f"configure_streams: side_cus and reserve_cus must be multiples of 8 (whole-XCD-balanced masks) summing to "
                         f"less than {total}")
    side = masked_stream(side_cus, 0, dev) if side_cus > 0 else None
    main = masked_stream(total - side_cus - reserve_cus, side_cus, dev) if (partition or side is None) else None
    if side is not None and side_work not in (1, 2, 3):
        raise ValueError("configure_streams: side_work is 1 (dE), 2 (weight gradients) or 3 (both)")
    plan = _STREAM_PLANS[idx] = StreamPlan(side, main, reserve_cus, side_work)
    _det_register_stream(side)
    return plan


def stream_plan(device=None):
    idx = torch.cuda.current_device() if device is None or torch.device(device).index is None else torch.device(device).index
    return _STREAM_PLANS.get(idx)


def main_stream(device=None):
    """the stream a training step should run on: the plan's masked main stream, else the current stream"""
    plan = stream_plan(device)
    return plan.main.stream if plan is not None and plan.main is not None else torch.cuda.current_stream(device)


def join_side_stream(device=None) -> None:
    """the current stream waits for everything issued on the side stream (called before the optimiser step, and by anything else
    that reads the gradients the side stream accumulates)"""
    plan = stream_plan(device)
    if plan is not None and plan.side is not None and plan.last is not None:
        torch.cuda.current_stream(device).wait_event(plan.last)
        plan.last = None


# --------------------------------------------------------------------------------------------------
# raw launchers (no autograd)
# --------------------------------------------------------------------------------------------------
def pad_bitmap(tok: torch.Tensor, pad: int, flag: torch.Tensor | None = None) -> torch.Tensor:
    """tok int32 [B,L] -> uint32 bitmap [B, L/32] (stored as int32).  ``flag`` (int32[1] on the device, optional) gets bit 0
    OR-ed in when a row starts with a pad token and holds a real token later (leading padding: fully masked queries; sticky;
    read it at a synchronisation point)."""
    _need_cuda(tok, flag)
    B, L = tok.shape
    bits = torch.empty(B, L // 32, dtype=torch.int32, device=tok.device)
    check(_lib.load().mgx_pad_bitmap(ptr(tok), ptr(bits), ptr(flag), B, L, pad, stream_ptr()), "mgx_pad_bitmap")
    return bits


def embed_pe_fwd(tok, table, pe, p_drop=0.0, seed=0):
    _need_cuda(tok, table, pe)
    B, L = tok.shape
    V, d = table.shape
    out = torch.empty(B, L, d, dtype=BF16, device=tok.device)
    check(_lib.load().mgx_embed_pe_fwd(ptr(tok), ptr(table), ptr(pe), ptr(out), B, L, d, V, float(p_drop),
                                       int(seed), stream_ptr()), "mgx_embed_pe_fwd")
    return out


def embed_bwd(tok, dout, dtable, p_drop=0.0, seed=0):
    _need_cuda(tok, dout, dtable)
    B, L = tok.shape
    V, d = dtable.shape
    check(_lib.load().mgx_embed_bwd(ptr(tok), ptr(dout), ptr(dtable), B, L, d, V, float(p_drop), int(seed),
                                    stream_ptr()), "mgx_embed_bwd")


def rel_attn_fwd(qkv, E, padbits, M=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """qkv bf16 [B,L,3d], E bf16 [M,64], padbits int32 [B,L/32] or None -> (ctx bf16 [B,L,d], lse f32 [B,h,L])"""
    _need_cuda(qkv, E, padbits)
    B, L, d3 = qkv.shape
    d = d3 // 3
    M = E.shape[0] if M is None else M
    ctx = torch.empty(B, L, d, dtype=BF16, device=qkv.device)
    lse = torch.empty(B, d // 64, L, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    ws = torch.empty(lib.mgx_rel_attn_fwd_workspace(L), dtype=torch.uint8, device=qkv.device)
    check(lib.mgx_rel_attn_fwd(ptr(qkv), ptr(E), ptr(padbits), ptr(ctx), ptr(lse), ptr(ws), ws.numel(), B, L, d, M,
                               stream_ptr()), "mgx_rel_attn_fwd")
    return ctx, lse


def rel_attn_fwd_nomask(qkv, E, Lk=None) -> torch.Tensor:
    """the reference's sampling call (mask=None): bidirectional attention over keys 0..Lk-1, relative term for j <= i only
    (mgx.h).  qkv bf16 [B,L,3d] -> ctx bf16 [B,L,d]; rows >= Lk are don't-cares.  Inference only."""
    _need_cuda(qkv, E)
    B, L, d3 = qkv.shape
    d = d3 // 3
    ctx = torch.empty(B, L, d, dtype=BF16, device=qkv.device)
    lse = torch.empty(B, d // 64, L, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    ws = torch.empty(lib.mgx_rel_attn_fwd_workspace(L), dtype=torch.uint8, device=qkv.device)
    check(lib.mgx_rel_attn_fwd_nomask(ptr(qkv), ptr(E), ptr(ctx), ptr(lse), ptr(ws), ws.numel(), B, L, L if Lk is None else int(Lk), d,
                                      E.shape[0], stream_ptr()), "mgx_rel_attn_fwd_nomask")
    return ctx


def rel_attn_weights(qkv, E, padbits, lse) -> torch.Tensor:
    """materialised attention weights f32 [B,h,L,L] (eval/debug output of the reference)"""
    _need_cuda(qkv, E, padbits, lse)
    B, L, d3 = qkv.shape
    d = d3 // 3
    w = torch.zeros(B, d // 64, L, L, dtype=torch.float32, device=qkv.device)
    lib = _lib.load()
    ws = torch.empty(lib.mgx_rel_attn_fwd_workspace(L), dtype=torch.uint8, device=qkv.device)
    check(lib.mgx_rel_attn_weights(ptr(qkv), ptr(E), ptr(padbits), ptr(lse), ptr(w), ptr(ws), ws.numel(), B, L, d,
                                   E.shape[0], stream_ptr()), "mgx_rel_attn_weights")
    return w


def rel_attn_bwd(qkv, E, padbits, ctx, dctx, lse, dE, parts=15, dqkv=None, workspace=None) -> torch.Tensor:
    """-> dqkv bf16 [B,L,3d]; dE f32 [M,64] accumulated in place.  parts selects sub-kernels (bench, cross-checks):
    1 pre-pass | 4 dK/dV (stores its dS tiles in the workspace) | 2 dQ from those tiles | 8 dE from those tiles |
    16 dE by recomputation | 32 dQ by recomputation (instead of 2) | 64 dK/dV by the 32-key kernel (instead of 4: cross-check)."""
    _need_cuda(qkv, E, padbits, ctx, dctx, lse, dE)
    B, L, d3 = qkv.shape
    d = d3 // 3
    lib = _lib.load()
    dqkv = torch.empty_like(qkv) if dqkv is None else dqkv
    need = lib.mgx_rel_attn_bwd_workspace(B, L, d)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=qkv.device)
    check(lib.mgx_rel_attn_bwd_parts(ptr(qkv), ptr(E), ptr(padbits), ptr(ctx), ptr(dctx), ptr(lse), ptr(dqkv), ptr(dE),
                                     ptr(workspace), workspace.numel(), B, L, d, E.shape[0], int(parts), stream_ptr()),
          "mgx_rel_attn_bwd")
    return dqkv


def add_ln_fwd(x, res, gamma, beta, eps=1e-6, p_drop=0.0, seed=0):
    _need_cuda(x, res, gamma, beta)
    d = x.shape[-1]
    rows = x.numel() // d
    out = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(_lib.load().mgx_add_ln_fwd(ptr(x), ptr(res), ptr(gamma), ptr(beta), ptr(out), ptr(mean), ptr(rstd), rows,
                                     d, float(eps), float(p_drop), int(seed), stream_ptr()), "mgx_add_ln_fwd")
    return out, mean, rstd


_LN_WS = {}


def add_ln_bwd(dout, x, res, gamma, mean, rstd, dgamma, dbeta, p_drop=0.0, seed=0, dxsum=None):
    """-> (dx, dres); dgamma/dbeta (and dxsum = colsum(dx), if given) are accumulated in place."""
    _need_cuda(dout, x, res, gamma, mean, rstd, dgamma, dbeta, dxsum)
    d = x.shape[-1]
    rows = x.numel() // d
    dres = torch.empty_like(x)
    dx = torch.empty_like(x) if p_drop > 0 else dres
    lib = _lib.load()
    key = (x.device, d)
    ws = _LN_WS.get(key)          # per-device scratch, reused by every call on the (single) compute stream
    need = lib.mgx_add_ln_bwd_workspace(rows, d)
    if ws is None or ws.numel() < need:
        ws = _LN_WS[key] = torch.empty(need, dtype=torch.uint8, device=x.device)
    check(lib.mgx_add_ln_bwd(ptr(dout), ptr(x), ptr(res), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dres),
                             ptr(dgamma), ptr(dbeta), ptr(dxsum), ptr(ws), ws.numel(), rows, d, float(p_drop), int(seed),
                             stream_ptr()), "mgx_add_ln_bwd")
    return dx, dres


def smooth_ce_fwd(logits, target, V, eps_ls, pad):
    """logits bf16 [rows, ld] -> (stats f32[4], argmax int32[rows], row_lse f32[rows])"""
    _need_cuda(logits, target)
    ld = logits.shape[-1]
    rows = logits.numel() // ld
    stats = torch.zeros(4, dtype=torch.float32, device=logits.device)
    argmax = torch.empty(rows, dtype=torch.int32, device=logits.device)
    row_lse = torch.empty(rows, dtype=torch.float32, device=logits.device)
    check(_lib.load().mgx_smooth_ce_fwd(ptr(logits), ptr(target), ptr(stats), ptr(argmax), ptr(row_lse), rows, V, ld,
                                        float(eps_ls), int(pad), stream_ptr()), "mgx_smooth_ce_fwd")
    return stats, argmax, row_lse


def smooth_ce_bwd(logits, target, stats, row_lse, V, eps_ls, pad, gscale=1.0, gscale_dev=None):
    """gscale_dev: optional 0-d / 1-element f32 device tensor multiplied into the gradient inside the kernel"""
    _need_cuda(logits, target, stats, row_lse)
    if gscale_dev is not None:
        _need_cuda(gscale_dev)
        if gscale_dev.dtype != torch.float32 or gscale_dev.numel() != 1:
            raise ValueError("gscale_dev must be one float32 element")
    ld = logits.shape[-1]
    rows = logits.numel() // ld
    dlogits = torch.empty_like(logits)
    check(_lib.load().mgx_smooth_ce_bwd(ptr(logits), ptr(target), ptr(stats), ptr(row_lse), ptr(dlogits), rows, V, ld,
                                        float(eps_ls), int(pad), float(gscale), ptr(gscale_dev), stream_ptr()), "mgx_smooth_ce_bwd")
    return dlogits


def adam_step(p, g, m, v, shadow, lr, beta1, beta2, eps, step, gscale=1.0):
    _need_cuda(p, g, m, v, shadow)
    check(_lib.load().mgx_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow), p.numel(), float(lr), float(beta1),
                                    float(beta2), float(eps), int(step), float(gscale), stream_ptr()), "mgx_adam_step")


GRAD_NORM_PARTS = _lib.DEFINES["MGX_GRAD_NORM_PARTS"]      # the doubles of mgx_grad_norm's workspace
_ClipState = _lib.STRUCTS["mgx_clip_state"]
CLIP_STATE_BYTES = ctypes.sizeof(_ClipState)


def clip_buffers(device):
    """-> (workspace f64 [GRAD_NORM_PARTS], state: the 32 bytes of mgx_clip_state as int64 [4], zeroed) for grad_norm"""
    return (torch.empty(GRAD_NORM_PARTS, dtype=torch.float64, device=device),
            torch.zeros(CLIP_STATE_BYTES // 8, dtype=torch.int64, device=device))


def _check_clip_state(state):
    _need_cuda(state)
    if state.numel() * state.element_size() < CLIP_STATE_BYTES:
        raise ValueError(f"state must hold the {CLIP_STATE_BYTES} bytes of mgx_clip_state")


def grad_norm(g, gscale, max_norm, workspace, state):
    """norm of g * gscale and torch's clip coefficient for max_norm (inf = never clip), left in `state` on the device: no host
    round trip.  A non-finite gradient marks the step as skipped (include/mgx.h: mgx_grad_norm)."""
    _need_cuda(g, workspace)
    _check_clip_state(state)
    if workspace.dtype != torch.float64 or workspace.numel() < GRAD_NORM_PARTS:
        raise ValueError(f"workspace must be float64 [{GRAD_NORM_PARTS}]")
    check(_lib.load().mgx_grad_norm(ptr(g), g.numel(), float(gscale), float(max_norm), ptr(workspace), ptr(state), stream_ptr()),
          "mgx_grad_norm")


def adam_step_clipped(p, g, m, v, shadow, lr, beta1, beta2, eps, step, state):
    """adam_step with the gradient scale grad_norm left in `state`; writes nothing when that call marked the step as skipped"""
    _need_cuda(p, g, m, v, shadow)
    _check_clip_state(state)
    check(_lib.load().mgx_adam_step_clipped(ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow), p.numel(), float(lr), float(beta1),
                                            float(beta2), float(eps), int(step), ptr(state), stream_ptr()), "mgx_adam_step_clipped")


ADAM_CHUNK = 64                                            # elements per byte of mgx_adam_step_groups' group_of
ADAM_MAX_GROUPS = 256


def adam_group_chunks(offsets, names, group_of_name, numel=None):
    """the chunk table of mgx_adam_step_groups as a list of ints, one per ADAM_CHUNK elements of a flat buffer: ``offsets[name]``
    = (start, numel) as in layers.FlatStore, ``names`` in buffer order, ``group_of_name[name]`` the parameter's group.  Every
    chunk from a parameter's start up to the next parameter's start (the buffer's end, ``numel``, for the last) takes that
    parameter's group: the zero padding behind a parameter belongs to it.  Pure host code; ValueError for a start that is no
    multiple of ADAM_CHUNK (a chunk would hold two parameters), overlapping parameters or a group outside 0 .. 255"""
    starts = [offsets[n][0] for n in names]
    ends = starts[1:] + [max([numel or 0] + [offsets[n][0] + offsets[n][1] for n in names])]
    table = [0] * (starts[0] // ADAM_CHUNK if names else 0)               # a gap before the first parameter: nothing lives there
    for n, lo, hi in zip(names, starts, ends):
        k = group_of_name[n]
        if lo % ADAM_CHUNK:
            raise ValueError(f"parameter {n} starts at element {lo}, not a multiple of {ADAM_CHUNK}")
        if hi < lo + offsets[n][1]:
            raise ValueError(f"parameter {n} overlaps the next one")
        if not (isinstance(k, int) and 0 <= k < ADAM_MAX_GROUPS):
            raise ValueError(f"group of {n} must be an int in 0 .. {ADAM_MAX_GROUPS - 1}, got {k!r}")
        table += [k] * ((hi - lo + ADAM_CHUNK - 1) // ADAM_CHUNK)
    return table


def adam_step_groups(p, g, m, v, shadow, ema, lr, beta1, beta2, eps, step, gscale, state, group_of, lr_scale, weight_decay,
                     ema_decay=0.0):
    """AdamW per chunk group, frozen chunks and the weight EMA in the one sweep (include/mgx.h: mgx_adam_step_groups).  state None:
    the gradient scale is gscale; else grad_norm's, and a skipped step writes nothing.  shadow and ema may be None"""
    _need_cuda(p, g, m, v, shadow, ema, group_of, lr_scale, weight_decay)
    if state is not None:
        _check_clip_state(state)
    n = p.numel()
    if group_of.dtype != torch.uint8 or group_of.numel() < (n + ADAM_CHUNK - 1) // ADAM_CHUNK:
        raise ValueError(f"group_of must be uint8 [{(n + ADAM_CHUNK - 1) // ADAM_CHUNK}]")
    if lr_scale.dtype != torch.float32 or weight_decay.dtype != torch.float32 or lr_scale.numel() != weight_decay.numel():
        raise ValueError("lr_scale and weight_decay must be float32 arrays of one length, the number of groups")
    if ema is not None and (ema.dtype != torch.float32 or ema.numel() != n):
        raise ValueError("ema must be float32 with p's number of elements")
    check(_lib.load().mgx_adam_step_groups(ptr(p), ptr(g), ptr(m), ptr(v), ptr(shadow), ptr(ema), n, float(lr), float(beta1),
                                           float(beta2), float(eps), int(step), float(gscale), ptr(state), ptr(group_of),
                                           ptr(lr_scale), ptr(weight_decay), lr_scale.numel(), float(ema_decay), stream_ptr()),
          "mgx_adam_step_groups")


def read_clip_state(state) -> dict:
    """the fields of mgx_clip_state; copies the 32 bytes to the host, so it SYNCHRONISES"""
    s = _ClipState.from_buffer_copy(state.detach().cpu().contiguous().view(torch.uint8)[:CLIP_STATE_BYTES].numpy())
    return {"norm": s.norm, "scale": s.scale, "skipped_last": s.skipped_last, "clipped": s.n_clipped, "skipped": s.n_skipped}


def cast_bf16(p, shadow):
    _need_cuda(p, shadow)
    check(_lib.load().mgx_cast_bf16(ptr(p), ptr(shadow), p.numel(), stream_ptr()), "mgx_cast_bf16")


class FragWeight:
    """a projection weight [N,K] kept in MFMA fragment order (pack_frag; rows zero-padded to a multiple of 32) for the
    decode-size (<= 32 rows) projections: linear_fwd / linear_ln_fwd / decode_embed_linear take it in place of the matrix"""

    def __init__(self, w: torch.Tensor):
        N, K = w.shape
        Np = (N + 31) // 32 * 32
        wp = torch.zeros(Np, K, dtype=BF16, device=w.device)
        wp[:N] = w
        self.data, self.shape = pack_frag(wp), (N, K)


def linear_fwd(a, w, bias, act=0):
    """a bf16 [M,K], w bf16 [N,K] (or a FragWeight, rows <= 32), bias f32 [N] or None -> bf16 [M,N] = act(a @ w.T + bias)"""
    K = a.shape[-1]
    Mrows = a.numel() // K
    N = w.shape[0]
    out = torch.empty(*a.shape[:-1], N, dtype=BF16, device=a.device)
    if isinstance(w, FragWeight):
        _need_cuda(a, w.data, bias)
        check(_lib.load().mgx_skinny_fwd_frag(ptr(a), ptr(w.data), ptr(bias), ptr(out), Mrows, N, K, int(act), stream_ptr()),
              "mgx_skinny_fwd_frag")
        return out
    _need_cuda(a, w, bias)
    check(_lib.load().mgx_linear_fwd(ptr(a), ptr(w), ptr(bias), ptr(out), Mrows, N, K, int(act), stream_ptr()),
          "mgx_linear_fwd")
    return out


def linear_ln_fwd(x, res, gamma, beta, w, bias, act=0, eps=1e-6):
    """decode-size rows (<= 32): z = LayerNorm(x + res), c = act(z @ w^T + bias) in one launch -> (c, z)"""
    N, K = w.shape
    Mrows = x.numel() // K
    c = torch.empty(*x.shape[:-1], N, dtype=BF16, device=x.device)
    z = torch.empty_like(x)
    if isinstance(w, FragWeight):
        _need_cuda(x, res, gamma, beta, w.data, bias)
        check(_lib.load().mgx_linear_ln_fwd_frag(ptr(x), ptr(res), ptr(gamma), ptr(beta), float(eps), ptr(w.data), ptr(bias), ptr(c),
                                                 ptr(z), Mrows, N, K, int(act), stream_ptr()), "mgx_linear_ln_fwd_frag")
        return c, z
    _need_cuda(x, res, gamma, beta, w, bias)
    check(_lib.load().mgx_linear_ln_fwd(ptr(x), ptr(res), ptr(gamma), ptr(beta), float(eps), ptr(w), ptr(bias), ptr(c), ptr(z),
                                        Mrows, N, K, int(act), stream_ptr()), "mgx_linear_ln_fwd")
    return c, z


def linear_dx(dy, w, relu_y=None, addend=None):
    """dy bf16 [..,N], w bf16 [N,K] -> dx bf16 [..,K] = dy @ w (zeroed where relu_y <= 0) (+ addend)"""
    _need_cuda(dy, w, relu_y, addend)
    N, K = w.shape
    Mrows = dy.numel() // N
    dx = torch.empty(*dy.shape[:-1], K, dtype=BF16, device=dy.device)
    if addend is not None and (addend.dtype != BF16 or addend.numel() != dx.numel() or not addend.is_contiguous()):
        raise ValueError("linear_dx: addend must be a contiguous bf16 tensor of dx's shape")
    check(_lib.load().mgx_linear_dx(ptr(dy), ptr(w), ptr(relu_y), ptr(addend), ptr(dx), Mrows, N, K, stream_ptr()),
          "mgx_linear_dx")
    return dx


def linear_dw(dy, x, gw, gb=None):
    """gw f32 [N,K] += dy^T @ x ; gb f32 [N] += colsum(dy).  A weight the ring kernel takes (mgx_linear_dw_grouped_workspace() > 0:
    many rows, tiles mostly full -- the vocabulary projection) goes there as a group of one: partial tiles + fix-up pass instead of
    fp32 atomics"""
    _need_cuda(dy, x, gw, gb)
    N, K = gw.shape
    Mrows = dy.numel() // N
    if dy.is_contiguous() and x.is_contiguous():
        one = (_DwProblem * 1)(_DwProblem(ptr(dy), ptr(x), ptr(gw), ptr(gb), N, K))
        if _lib.load().mgx_linear_dw_grouped_workspace(ctypes.cast(one, ctypes.c_void_p), 1, Mrows):
            return linear_dw_grouped([(dy, x, gw, gb)])
    check(_lib.load().mgx_linear_dw(ptr(dy), ptr(x), ptr(gw), ptr(gb), Mrows, N, K, stream_ptr()), "mgx_linear_dw")


# ---- Event_Melody_RNN training ops (raw launchers; the autograd node lives in melody_rnn.py) ----------------------
def gru_cell_fwd(gi, gh, h_prev, h_next, y):
    """h_next f32 / y bf16 [B,H] <- GRU cell(gi, gh bf16 [B,3H], h_prev f32 [B,H])"""
    _need_cuda(gi, gh, h_prev, h_next, y)
    B, H = h_prev.shape
    check(_lib.load().mgx_gru_cell_fwd(ptr(gi), ptr(gh), ptr(h_prev), ptr(h_next), ptr(y), B, H, stream_ptr()), "mgx_gru_cell_fwd")


def gru_cell_bwd(gi, gh, h_prev, dh_direct, d_rec, dy, dgi, dgh, dh_prev_direct):
    _need_cuda(gi, gh, h_prev, dh_direct, d_rec, dy, dgi, dgh, dh_prev_direct)
    B, H = h_prev.shape
    check(_lib.load().mgx_gru_cell_bwd(ptr(gi), ptr(gh), ptr(h_prev), ptr(dh_direct), ptr(d_rec), ptr(dy), ptr(dgi), ptr(dgh),
                                       ptr(dh_prev_direct), B, H, stream_ptr()), "mgx_gru_cell_bwd")


def pack_frag(w: torch.Tensor) -> torch.Tensor:
    """W [N,K] (N % 32 == 0, K % 16 == 0) -> bf16 copy in MFMA fragment order (mgx.h, fused GRU step): unit
    ((nt*K/16 + ks)*64 + lane) = W[32 nt + lane % 32][16 ks + 8 (lane // 32) .. +7]"""
    N, K = w.shape
    if N % 32 or K % 16:
        raise ValueError("pack_frag: need N % 32 == 0 and K % 16 == 0")
    return w.to(BF16).view(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().view(N, K)


def gru_step_fwd(gi, h_prev_bf, h_prev, whh, bhh, h_next, y, gh_out):
    """one fused time step (whh = pack_frag(W_hh)): gh_out bf16 [B,3H] = h_prev_bf @ W_hh.T + bhh, then h_next f32 / y bf16 [B,H] = cell(gi, gh, h_prev)"""
    _need_cuda(gi, h_prev_bf, h_prev, whh, bhh, h_next, y, gh_out)
    B, H = h_prev.shape
    check(_lib.load().mgx_gru_step_fwd(ptr(gi), ptr(h_prev_bf), ptr(h_prev), ptr(whh), ptr(bhh), ptr(h_next), ptr(y), ptr(gh_out),
                                       B, H, stream_ptr()), "mgx_gru_step_fwd")


def gru_step_x_fwd(x, wih, bih, h_prev_bf, h_prev, whh, bhh, h_next, y):
    """sampling step of one GRU layer in one launch (wih, whh = pack_frag of the weights): both projections + the cell;
    (h_next, y) must not alias (h_prev, h_prev_bf)"""
    _need_cuda(x, wih, bih, h_prev_bf, h_prev, whh, bhh, h_next, y)
    B, H = h_prev.shape
    check(_lib.load().mgx_gru_step_x_fwd(ptr(x), ptr(wih), ptr(bih), wih.shape[1], ptr(h_prev_bf), ptr(h_prev), ptr(whh), ptr(bhh),
                                         ptr(h_next), ptr(y), B, H, stream_ptr()), "mgx_gru_step_x_fwd")


def gru_step_x_fwd_save(x, wih, bih, h_prev_bf, h_prev, whh, bhh, h_next, y, gi_out, gh_out):
    """gru_step_x_fwd that also stores the two rounded projections, gi_out / gh_out bf16 [B,3H], as gru_step_bwd reads them
    (the step of the free-running training forward); h_next / y are bit-identical to gru_step_x_fwd's"""
    _need_cuda(x, wih, bih, h_prev_bf, h_prev, whh, bhh, h_next, y, gi_out, gh_out)
    B, H = h_prev.shape
    if x.shape != (B, wih.shape[1]) or gi_out.shape != (B, 3 * H) or gh_out.shape != (B, 3 * H) or h_next.shape != (B, H) or y.shape != (B, H):
        raise ValueError("gru_step_x_fwd_save: x [B,Kx], gi_out / gh_out [B,3H], h_next / y [B,H]")
    check(_lib.load().mgx_gru_step_x_fwd_save(ptr(x), ptr(wih), ptr(bih), wih.shape[1], ptr(h_prev_bf), ptr(h_prev), ptr(whh),
                                              ptr(bhh), ptr(h_next), ptr(y), ptr(gi_out), ptr(gh_out), B, H, stream_ptr()),
          "mgx_gru_step_x_fwd_save")


def dropout_bf16_at(x, out, index0, p_drop, seed_dev):
    """dropout_bf16 on a slice: x / out hold elements index0 .. of a larger buffer and get that buffer's mask; the seed is read from
    ``seed_dev`` (an int64 [1] view of device memory) when the kernel runs"""
    _need_cuda(x, out, seed_dev)
    if out.numel() != x.numel() or out.dtype != BF16 or x.dtype != BF16 or seed_dev.dtype != torch.int64 or seed_dev.numel() < 1:
        raise ValueError("dropout_bf16_at: x / out bf16 of one size, seed_dev int64 [1]")
    check(_lib.load().mgx_dropout_bf16_at(ptr(x), ptr(out), x.numel(), int(index0), float(p_drop), ptr(seed_dev), stream_ptr()),
          "mgx_dropout_bf16_at")


def gru_next_event(logits, V, flag_dev, events, temperature, seed_dev, step, emb, tok, used_out, x_out):
    """next input of every row of the free-running training forward (mgx.h: forced / greedy / drawn by the step's device-side
    flag) and its embedding: tok, used_out int32 [B], x_out bf16 [B,Ep] = emb[tok]"""
    _need_cuda(logits, flag_dev, events, seed_dev, emb, tok, used_out, x_out)
    B, ld = logits.shape
    Ep = emb.shape[1]
    if (logits.dtype != BF16 or emb.dtype != BF16 or x_out.dtype != BF16 or emb.shape[0] < V or x_out.shape != (B, Ep)
            or flag_dev.dtype != torch.int32 or seed_dev.dtype != torch.int64
            or any(t.dtype != torch.int32 or t.numel() != B for t in (tok, used_out) + (() if events is None else (events,)))):
        raise ValueError("gru_next_event: logits bf16 [B,ld], emb bf16 [>=V,Ep], x_out bf16 [B,Ep], flag int32 [1], seed int64 [1], "
                         "tok / used_out / events int32 [B]")
    check(_lib.load().mgx_gru_next_event(ptr(logits), V, ld, ptr(flag_dev), ptr(events), float(temperature), ptr(seed_dev),
                                         int(step) & 0xFFFFFFFF, ptr(emb), Ep, ptr(tok), ptr(used_out), ptr(x_out), B, stream_ptr()),
          "mgx_gru_next_event")


def gru_step_bwd(gi, gh, h_prev, dh_direct, dgh_next, whh_t, dy, dgi, dgh, dh_out, final=False):
    """one fused backward step: d_rec = dgh_next @ W_hh (whh_t = pack_frag(W_hh.T)), then the cell backward (see mgx.h)"""
    _need_cuda(gi, gh, h_prev, dh_direct, dgh_next, whh_t, dy, dgi, dgh, dh_out)
    B, H = dh_out.shape
    check(_lib.load().mgx_gru_step_bwd(ptr(gi), ptr(gh), ptr(h_prev), ptr(dh_direct), ptr(dgh_next), ptr(whh_t), ptr(dy), ptr(dgi),
                                       ptr(dgh), ptr(dh_out), B, H, 1 if final else 0, stream_ptr()), "mgx_gru_step_bwd")


def dropout_bf16(x, p_drop, seed):
    """stateless inverted dropout; the same call on a gradient is the backward"""
    _need_cuda(x)
    if p_drop <= 0:
        return x
    out = torch.empty_like(x)
    check(_lib.load().mgx_dropout_bf16(ptr(x), ptr(out), x.numel(), float(p_drop), int(seed), stream_ptr()), "mgx_dropout_bf16")
    return out


def scatter_add_rows(idx, src, dst):
    """dst f32 [V,cols][idx[r]] += src bf16 [n,ld][r, :cols]"""
    _need_cuda(idx, src, dst)
    V, cols = dst.shape
    n, ld = src.shape
    check(_lib.load().mgx_scatter_add_rows(ptr(idx), ptr(src), ptr(dst), n, ld, cols, V, stream_ptr()), "mgx_scatter_add_rows")


_DW_WS = {}


_DwProblem = _lib.STRUCTS["mgx_dw_problem"]


def linear_dw_grouped(problems):
    """problems: list of (dy bf16 [..,N], x bf16 [..,K], gw f32 [N,K], gb f32 [N] or None) sharing the row count:
    all weight (and bias) gradients in one launch."""
    arr = (_DwProblem * len(problems))()
    Mrows = None
    for i, (dy, x, gw, gb) in enumerate(problems):
        _need_cuda(dy, x, gw, gb)
        N, K = gw.shape
        rows = dy.numel() // N
        if Mrows is None:
            Mrows = rows
        if rows != Mrows or x.numel() != rows * K or not (dy.is_contiguous() and x.is_contiguous()):
            raise ValueError("linear_dw_grouped: all problems need contiguous dy [M,N], x [M,K] with the same M")
        arr[i] = _DwProblem(ptr(dy), ptr(x), ptr(gw), ptr(gb), N, K)
    lib = _lib.load()
    parr = ctypes.cast(arr, ctypes.c_void_p)
    need = lib.mgx_linear_dw_grouped_workspace(parr, len(problems), Mrows)
    dev = problems[0][0].device
    # scratch for the fp32 partial tiles of the M-splits, one per (device, stream): two calls on different streams must not
    # share partial tiles, and a buffer is only ever replaced by a larger one for the stream that asked (the caching allocator
    # keeps the old block alive until that stream's work on it is done; never while a graph is being captured)
    key = (dev, stream_ptr())
    ws = _DW_WS.get(key)
    if need and (ws is None or ws.numel() < need):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("linear_dw_grouped: the workspace must exist before graph capture (run one step eagerly first)")
        ws = _DW_WS[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    check(lib.mgx_linear_dw_grouped(parr, len(problems), Mrows, ptr(ws) if need else None, need, stream_ptr()),
          "mgx_linear_dw_grouped")


# ---- decode path (no autograd) ----------------------------------------------------------------------
# Every wrapper below checks its tensors on the host first (ValueError), then asks for device memory (_need_cuda), then calls
# the library; the tensor contract is stated once, in _tensor_is / _check_tensor.
def _tensor_is(t, dtypes, entries=None, shape=None, at_least=None):
    """whether ``t`` is a contiguous tensor of one of ``dtypes`` (a dtype or a tuple of them; None: any) that holds ``entries``
    entries in any shape, or has ``shape`` -- an int per fixed dimension, a name per free one -- and, with ``at_least``, no
    fewer entries than that"""
    if t is None or not (dtypes is None or t.dtype == dtypes or (isinstance(dtypes, tuple) and t.dtype in dtypes)):
        return False
    if entries is not None and t.numel() != entries:
        return False
    if shape is not None and (t.dim() != len(shape) or any(not isinstance(s, str) and n != s for n, s in zip(t.shape, shape))):
        return False
    return (at_least is None or t.numel() >= at_least) and t.is_contiguous()


def _check_tensor(what, name, t, dtypes, entries=None, shape=None, at_least=None, optional=False):
    """the tensor contract of wrapper ``what``'s argument ``name`` (_tensor_is), refused with a ValueError of one form; None
    passes where the argument is ``optional``"""
    if (t is None and optional) or _tensor_is(t, dtypes, entries, shape, at_least):
        return
    kinds = " / ".join({torch.bfloat16: "bf16"}.get(d, str(d).replace("torch.", ""))
                       for d in (dtypes if isinstance(dtypes, tuple) else (dtypes,)) if d is not None)
    form = (f" of {entries} entries" if entries is not None else "") + \
        (" [" + ", ".join(str(s) for s in shape) + "]" if shape is not None else "") + \
        (f" of at least {at_least} entries" if at_least is not None else "")
    got = "None" if t is None else f"{t.dtype} {tuple(t.shape)}" + ("" if t.is_contiguous() else f", strides {t.stride()}")
    raise ValueError(f"{what}: {name} must be a contiguous {kinds + ' ' if kinds else ''}tensor{form}, got {got}")


def _step_pos(what, pos_dev, B, ragged, base=None, with_base=False):
    """the step-position arguments of a decode call (include/mgx.h, "Step positions"), checked on the host (ValueError):
    ``pos_dev`` contiguous int32, one shared counter or -- ``ragged`` -- one position per row, B entries; ``base``, the window's
    base, of the positions' shape or None.  Returns (pos_dev, per_row) as the C arguments, (pos_dev, base_dev, per_row) with
    ``with_base``"""
    n = B if ragged else 1
    if not _tensor_is(pos_dev, torch.int32, entries=n):
        kind = f"ragged decode: the positions must be a contiguous int32 tensor of {B} entries" if ragged else \
            "a shared position is one contiguous int32"
        raise ValueError(f"{what}: {kind} (got {pos_dev.dtype}, {pos_dev.numel()} entries)")
    if base is not None and not _tensor_is(base, torch.int32, entries=n):
        raise ValueError(f"{what}: base must be a contiguous int32 tensor of the positions' {n} entries "
                         f"(got {base.dtype}, {base.numel()} entries)")
    per_row = 1 if ragged else 0
    return (ptr(pos_dev), ptr(base), per_row) if with_base else (ptr(pos_dev), per_row)


def decode_embed(tok, table, pe, pos_dev, out, *, ragged=False):
    pos = _step_pos("decode_embed", pos_dev, tok.numel(), ragged)
    _need_cuda(tok, table, pe, pos_dev, out)
    V, d = table.shape
    check(_lib.load().mgx_decode_embed(ptr(tok), ptr(table), ptr(pe), *pos, ptr(out), tok.numel(), d, V, stream_ptr()),
          "mgx_decode_embed")
    return out


def decode_embed_linear(tok, table, pe, pos_dev, w, bias, hout, *, ragged=False):
    """h = table[tok]*sqrt(d) + pe[t] (written to ``hout`` bf16 [B,d]) and c bf16 [B,N] = h w^T + bias in one launch;
    ``ragged``: t = pos_dev[b] per row"""
    V, d = table.shape
    N = w.shape[0]
    c = torch.empty(tok.numel(), N, dtype=torch.bfloat16, device=hout.device)
    pos = _step_pos("decode_embed_linear", pos_dev, tok.numel(), ragged)
    frag = isinstance(w, FragWeight)                    # the weight in MFMA fragment order
    wd = w.data if frag else w
    _need_cuda(tok, table, pe, pos_dev, wd, bias, hout)
    lib = _lib.load()
    fn, name = (lib.mgx_decode_embed_linear_frag, "mgx_decode_embed_linear_frag") if frag else \
        (lib.mgx_decode_embed_linear, "mgx_decode_embed_linear")
    check(fn(ptr(tok), ptr(table), ptr(pe), *pos, ptr(wd), ptr(bias), ptr(c), ptr(hout), tok.numel(), N, d, V, stream_ptr()), name)
    return c, hout


def rel_attn_decode_splits(B, Lmax, d) -> int:
    return int(_lib.load().mgx_rel_attn_decode_splits(B, Lmax, d))


def rel_attn_decode_workspace(B, Lmax, d, device):
    """scratch for the split-K partials of mgx_rel_attn_decode (None when the cache is short enough for one workgroup per
    (b,h)); allocate once per generation: the decode step is graph-captured, so the buffer must outlive the graph"""
    n = _lib.load().mgx_rel_attn_decode_workspace(B, Lmax, d)
    return torch.empty(n, dtype=torch.uint8, device=device) if n else None


_FP8_CACHE = (torch.uint8, torch.float8_e4m3fn)


def _check_kv_cache(kcache, vcache, kscale, vscale, what) -> bool:
    """validates a K/V cache pair: bf16 [B, h, Lmax, 64], or the 8-bit cache (ABI 20) -- codes uint8 / float8_e4m3fn
    [B, h, Lmax, 64] with scales f32 [B, h, Lmax] -- all contiguous.  Returns whether it is the 8-bit cache."""
    _check_tensor(what, "kcache", kcache, (torch.bfloat16,) + _FP8_CACHE, shape=("B", "h", "Lmax", 64))
    fp8 = kcache.dtype in _FP8_CACHE
    if fp8 and vcache.dtype not in _FP8_CACHE:
        raise ValueError(f"{what}: the 8-bit caches must both be uint8 or float8_e4m3fn, got {kcache.dtype} / {vcache.dtype}")
    _check_tensor(what, "vcache", vcache, _FP8_CACHE if fp8 else torch.bfloat16, shape=tuple(kcache.shape))
    if not fp8:
        if kscale is not None or vscale is not None:
            raise ValueError(f"{what}: kscale / vscale belong to the 8-bit cache (uint8 or float8_e4m3fn), the caches are bf16")
        return False
    for s in (kscale, vscale):                            # named together: the message says what stands beside the 8-bit caches
        _check_tensor(what, "kscale / vscale", s, torch.float32, shape=tuple(kcache.shape[:3]))
    return True


def kv_store_fp8(qkv, n, kcache, vcache, kscale, vscale):
    """quantize rows 0..n-1 of the K and V columns of qkv bf16 [B, Lrows, 3d] into the 8-bit caches (format: include/mgx.h,
    ABI 20); the other cache rows are left as they are"""
    if not _check_kv_cache(kcache, vcache, kscale, vscale, "kv_store_fp8"):
        raise ValueError("kv_store_fp8: the caches must be the 8-bit cache (uint8 or float8_e4m3fn), got bf16")
    B, heads, Lmax, _ = kcache.shape
    d = heads * 64
    _check_tensor("kv_store_fp8", "qkv", qkv, torch.bfloat16, shape=(B, "Lrows", 3 * d))
    _need_cuda(qkv, kcache, vcache, kscale, vscale)
    check(_lib.load().mgx_kv_store_fp8(ptr(qkv), qkv.shape[1], int(n), ptr(kcache), ptr(vcache), ptr(kscale), ptr(vscale),
                                       B, Lmax, d, stream_ptr()), "mgx_kv_store_fp8")


def rel_attn_decode(qkv_new, kcache, vcache, E, pos_dev, ctx, workspace=None, *, ragged=False, kscale=None, vscale=None):
    """kcache / vcache bf16 [B, h, Lmax, 64] (head-major: workgroup (b, h) streams one contiguous run of rows);
    ``ragged``: row b's position is pos_dev[b] (each < Lmax: not checked, the positions live on the device).
    uint8 / float8_e4m3fn caches are the 8-bit cache (ABI 20) and need ``kscale`` / ``vscale`` f32 [B, h, Lmax]."""
    fp8 = _check_kv_cache(kcache, vcache, kscale, vscale, "rel_attn_decode")
    B, heads, Lmax, _ = kcache.shape
    pos = _step_pos("rel_attn_decode", pos_dev, B, ragged)
    _need_cuda(qkv_new, kcache, vcache, E, pos_dev, ctx, workspace, kscale, vscale)
    tail = (ptr(E), *pos, ptr(ctx), ptr(workspace), 0 if workspace is None else workspace.numel(), B, Lmax, heads * 64, E.shape[0],
            stream_ptr())
    if fp8:
        check(_lib.load().mgx_rel_attn_decode_fp8(ptr(qkv_new), ptr(kcache), ptr(vcache), ptr(kscale), ptr(vscale), *tail),
              "mgx_rel_attn_decode_fp8")
    else:
        check(_lib.load().mgx_rel_attn_decode(ptr(qkv_new), ptr(kcache), ptr(vcache), *tail), "mgx_rel_attn_decode")
    return ctx


# ---- N samples per prompt over a shared prompt cache (ABI 26; contract in include/mgx.h) -----------------------------
SHARED_MAX_N = _lib.DEFINES["MGX_SHARED_MAX_N"]
SHARED_NQ = _lib.DEFINES["MGX_SHARED_NQ"]                 # queries per workgroup of the kernel


def rel_attn_decode_shared_splits(Bp, N, Lpre, Lown, d) -> int:
    return int(_lib.load().mgx_rel_attn_decode_shared_splits(Bp, N, Lpre, Lown, d))


def rel_attn_decode_shared_workspace(Bp, N, Lpre, Lown, d, device):
    """scratch for the split-K partials of mgx_rel_attn_decode_shared (None for one split), as rel_attn_decode_workspace"""
    n = _lib.load().mgx_rel_attn_decode_shared_workspace(Bp, N, Lpre, Lown, d)
    return torch.empty(n, dtype=torch.uint8, device=device) if n else None


def rel_attn_decode_shared(qkv_new, kpre, vpre, kown, vown, E, pos_rows, pre_rows, ctx, workspace, N):
    """the decode attention of R = Bp * N rows, row b * N + n = sample n of prompt b: kpre / vpre bf16 [Bp, h, Lpre, 64] hold
    every prompt's first pre_rows[b] keys once (never written), kown / vown bf16 [R, h, Lown, 64] what each row appended itself;
    pos_rows int32 [R] (the N rows of a prompt hold one position), pre_rows int32 [Bp], both on the device and not checked"""
    what = "rel_attn_decode_shared"
    N = int(N)
    if not 1 <= N <= SHARED_MAX_N:
        raise ValueError(f"{what}: N must lie in 1 .. {SHARED_MAX_N}, got {N}")
    for kname, k, vname, v in (("kpre", kpre, "vpre", vpre), ("kown", kown, "vown", vown)):
        _check_tensor(what, kname, k, torch.bfloat16, shape=("rows", "h", "L", 64))
        _check_tensor(what, vname, v, torch.bfloat16, shape=tuple(k.shape))
    Bp, heads, Lpre, _ = kpre.shape
    R, d = Bp * N, heads * 64
    if kown.shape[0] != R or kown.shape[1] != heads:
        raise ValueError(f"{what}: kown / vown must hold Bp * N = {R} rows of {heads} heads, got {tuple(kown.shape)}")
    _check_tensor(what, "qkv_new", qkv_new, torch.bfloat16, shape=(R, 3 * d))
    _check_tensor(what, "ctx", ctx, torch.bfloat16, shape=(R, d))
    _check_tensor(what, "E", E, torch.bfloat16, shape=("M", 64))
    _step_pos(what, pos_rows, R, True)
    _check_tensor(what, "pre_rows", pre_rows, torch.int32, entries=Bp)
    _need_cuda(qkv_new, kpre, vpre, kown, vown, E, pos_rows, pre_rows, ctx, workspace)
    check(_lib.load().mgx_rel_attn_decode_shared(ptr(qkv_new), ptr(kpre), ptr(vpre), ptr(kown), ptr(vown), ptr(E), ptr(pos_rows),
                                                 ptr(pre_rows), ptr(ctx), ptr(workspace),
                                                 0 if workspace is None else workspace.numel(), Bp, N, Lpre, kown.shape[2], d,
                                                 E.shape[0], stream_ptr()), "mgx_rel_attn_decode_shared")
    return ctx


def grammar_table(grammar, device):
    """a grammar -- the [V, ceil(V/32)] bit table "token v may follow token t" (e.g. REMI_EventSeq.next_token_table()), a numpy
    uint32 / int32 array or a tensor -- as the contiguous int32 device tensor the kernels' ``allow_table`` takes; None stays None"""
    if grammar is None:
        return None
    table = torch.as_tensor(np.ascontiguousarray(grammar).view(np.int32) if isinstance(grammar, np.ndarray) else grammar)
    return table.to(device=device, dtype=torch.int32).contiguous()


def _check_allow_table(allow_table, V, what=None):
    if allow_table is not None and not (_tensor_is(allow_table, None, shape=(V, (V + 31) // 32)) and allow_table.element_size() == 4):
        raise ValueError((f"{what}: " if what else "") + "allow_table must be a contiguous 32-bit integer tensor of shape [V, ceil(V/32)]")


def sample_topk_topp(logits, V, pos_dev, next_tok, out_tokens=None, probs_out=None, temperature=1.0, top_k=0, top_p=1.0,
                     seed=0, advance=True, allow_table=None, row0=0, *, ragged=False, base=None):
    """allow_table: optional int32/uint32 [V, ceil(V/32)] grammar mask on the device (bit v of row t: v may follow t);
    row0: index of the first row in the whole batch when the tensors are a sub-batch's rows (the draw is by global row);
    ragged: row b's position is pos_dev[b] (draw, out_tokens column pos_dev[b] + 1, and every entry advanced);
    base (ABI 21): int32 of pos_dev's shape, the out_tokens column of window position 0 -- the draw and the column written
    take base + pos_dev in place of pos_dev; advance moves pos_dev only"""
    ld = logits.shape[-1]
    B = logits.numel() // ld
    pos = _step_pos("sample_topk_topp", pos_dev, B, ragged, base, with_base=True)
    _check_allow_table(allow_table, V, "sample_topk_topp")
    _need_cuda(logits, pos_dev, next_tok, out_tokens, probs_out, allow_table, base)
    check(_lib.load().mgx_sample_topk_topp(ptr(logits), int(V), ld, float(temperature), int(top_k), float(top_p), int(seed), *pos,
                                           ptr(next_tok), ptr(out_tokens), 0 if out_tokens is None else out_tokens.shape[-1],
                                           ptr(probs_out), B, int(row0), 1 if advance else 0, ptr(allow_table), stream_ptr()),
          "mgx_sample_topk_topp")
    return next_tok


def decode_reanchor(pos_dev, base, out_tokens, seq, hop, pad_token, *, ragged=False):
    """the re-anchor of the decode window (ABI 21): pos_dev -= hop and base += hop (int32 [1] shared, or [B] with ``ragged``),
    then seq int32 [B, n_pad] = the window's tokens out_tokens[b, base_b : base_b + pos_b], right-padded with pad_token"""
    _check_tensor("decode_reanchor", "seq", seq, torch.int32, shape=("B", "n_pad"))
    B, n_pad = seq.shape
    pos = _step_pos("decode_reanchor", pos_dev, B, ragged, base, with_base=True)
    _check_tensor("decode_reanchor", "out_tokens", out_tokens, torch.int32, shape=(B, "out_ld"))
    _need_cuda(pos_dev, base, out_tokens, seq)
    check(_lib.load().mgx_decode_reanchor(*pos, ptr(out_tokens), out_tokens.shape[1], ptr(seq), n_pad, int(hop), int(pad_token), B,
                                          stream_ptr()), "mgx_decode_reanchor")
    return seq


# ---- length budgets on the decode path (ABI 27; contracts in include/mgx.h) ------------------------------------------
NO_BUDGET = 2 ** 31 - 1                                   # remaining = INT32_MAX: the row has no budget


def budget_mask(logits, V, cost, remaining, done):
    """in place, before the sampler: logits bf16 [B, ld] of a live row (done[b] == 0) get -inf at every id v < V with
    cost[v] > remaining[b]; done rows, columns >= V and every other id stay bit for bit"""
    B = remaining.numel()
    ld = logits.shape[-1]
    _check_tensor("budget_mask", "logits", logits, torch.bfloat16, entries=B * ld)
    _check_tensor("budget_mask", "cost", cost, torch.int32, shape=("V",))
    for name, t in (("remaining", remaining), ("done", done)):
        _check_tensor("budget_mask", name, t, torch.int32, shape=(B,))
    if not 0 < int(V) <= min(ld, cost.numel()):
        raise ValueError(f"budget_mask: V must lie in 1 .. min(ld, the entries of cost) = {min(ld, cost.numel())}, got {V}")
    _need_cuda(logits, cost, remaining, done)
    check(_lib.load().mgx_budget_mask(ptr(logits), int(V), ld, ptr(cost), ptr(remaining), ptr(done), B, stream_ptr()),
          "mgx_budget_mask")
    return logits


def budget_account(next_tok, out_tokens, pos_dev, cost, remaining, done, count, pad_token, inclusive=True, *, ragged=False,
                   base=None):
    """after the sampler and its advance: charges cost[next_tok[b]] to every live row, ends the rows whose budget is spent
    (``inclusive``: the last token stays; else it becomes pad_token) and writes pad_token over what an ended row sampled --
    next_tok[b] and out_tokens[b, base + pos], the column the sampler has just written.  ``ragged`` / ``base`` as in
    sample_topk_topp"""
    B = remaining.numel()
    pos = _step_pos("budget_account", pos_dev, B, ragged, base, with_base=True)
    _check_tensor("budget_account", "cost", cost, torch.int32, shape=("V",))
    for name, t in (("next_tok", next_tok), ("remaining", remaining), ("done", done), ("count", count)):
        _check_tensor("budget_account", name, t, torch.int32, shape=(B,))
    _check_tensor("budget_account", "out_tokens", out_tokens, torch.int32, shape=(B, "out_ld"))
    _need_cuda(next_tok, out_tokens, pos_dev, base, cost, remaining, done, count)
    check(_lib.load().mgx_budget_account(ptr(next_tok), ptr(out_tokens), out_tokens.shape[1], *pos, ptr(cost), ptr(remaining),
                                         ptr(done), ptr(count), int(pad_token), 1 if inclusive else 0, B, stream_ptr()),
          "mgx_budget_account")
    return next_tok


# ---- repetition control on the decode path (ABI 31; contract in include/mgx.h) ---------------------------------------
REPEAT_MAX_WINDOW = _lib.DEFINES["MGX_REPEAT_MAX_WINDOW"]
REPEAT_MAX_NGRAM = _lib.DEFINES["MGX_REPEAT_MAX_NGRAM"]


def repeat_penalty(logits, V, out_tokens, pos_dev, subject, pen, window, ngram=0, span=0, ban=1e4, *, ragged=False, base=None):
    """in place, before the sampler: logits bf16 [B, ld] lose pen[cnt] at every id v < V with subject[v] != 0 that occurs cnt > 0
    times in the last ``window`` columns of its row of out_tokens int32 [B, out_ld] (up to and including column base + pos, the
    row's last token), and ``ban`` at every id that would complete an ``ngram``-gram the row holds already (inside the last
    ``span`` columns; 0: the whole row).  subject int32 [V] and pen float32 [window + 1] are None exactly with window == 0.
    ``ragged`` / ``base`` as in sample_topk_topp"""
    ld = logits.shape[-1]
    B = logits.numel() // ld
    pos = _step_pos("repeat_penalty", pos_dev, B, ragged, base, with_base=True)
    _check_tensor("repeat_penalty", "logits", logits, torch.bfloat16, entries=B * ld)
    _check_tensor("repeat_penalty", "out_tokens", out_tokens, torch.int32, shape=(B, "out_ld"))
    window = int(window)
    if (window == 0) != (subject is None) or (window == 0) != (pen is None):
        raise ValueError(f"repeat_penalty: subject and pen are None exactly with window == 0 (window={window})")
    if window:
        _check_tensor("repeat_penalty", "subject", subject, torch.int32, shape=("n",), at_least=int(V))
        _check_tensor("repeat_penalty", "pen", pen, torch.float32, shape=(window + 1,))
    _need_cuda(logits, out_tokens, pos_dev, base, subject, pen)
    check(_lib.load().mgx_repeat_penalty(ptr(logits), int(V), ld, ptr(out_tokens), out_tokens.shape[1], *pos, ptr(subject), ptr(pen),
                                         window, int(ngram), int(span), float(ban), B, stream_ptr()), "mgx_repeat_penalty")
    return logits


# ---- per-class sampling on the decode path (ABI 33; contract in include/mgx.h) ---------------------------------------
CLASS_MAX = _lib.DEFINES["MGX_CLASS_MAX"]


def class_logits(logits, V, cls, inv_temp, top_k, top_p, temperature, tok=None, allow_table=None):
    """in place, before the sampler: every row of logits bf16 [B, ld] becomes bf16(ln p') over its ids v < V, -inf where p' is 0 --
    p' keeps every class's total probability at ``temperature`` and gives the ids inside class c the softmax at inv_temp[c],
    filtered by top_k[c] / top_p[c] (the sampler's rules).  cls int32 [>= V], the class of every id; inv_temp float32, top_k
    int32, top_p float32 [C] each, on the device.  tok int32 [B] and allow_table [V, ceil(V/32)]: the sampler's grammar and
    the rows' input tokens, both or neither.  The sampler then runs at temperature 1"""
    ld = logits.shape[-1]
    B = logits.numel() // ld
    _check_tensor("class_logits", "logits", logits, torch.bfloat16, entries=B * ld)
    _check_tensor("class_logits", "cls", cls, torch.int32, shape=("n",), at_least=int(V))
    C = inv_temp.numel()
    for name, t, dt in (("inv_temp", inv_temp, torch.float32), ("top_k", top_k, torch.int32), ("top_p", top_p, torch.float32)):
        _check_tensor("class_logits", name, t, dt, shape=(C,))
    if (tok is None) != (allow_table is None):
        raise ValueError("class_logits: tok and allow_table are given together or not at all")
    _check_allow_table(allow_table, V, "class_logits")
    _check_tensor("class_logits", "tok", tok, torch.int32, entries=B, optional=True)
    _need_cuda(logits, cls, inv_temp, top_k, top_p, tok, allow_table)
    check(_lib.load().mgx_class_logits(ptr(logits), int(V), ld, ptr(cls), C, ptr(inv_temp), ptr(top_k), ptr(top_p),
                                       float(temperature), ptr(tok), ptr(allow_table), B, stream_ptr()), "mgx_class_logits")
    return logits


# ---- entropy-aware sampling on the decode path (ABI 34; contracts in include/mgx.h) ----------------------------------
def entropy_mask(logits, V, temperature, min_p=0.0, typical_p=1.0, mu=None, lse_out=None, tok=None, allow_table=None):
    """in place, before the sampler: a pure mask on logits bf16 [B, ld] -- the ids v < V that the Mirostat cut (``mu`` float32 [B]:
    surprise in bits at most mu[b]), min-p and typical sampling drop, in that order and each on the survivors of the one before,
    become -inf; every other value stays bit for bit.  ``lse_out`` float32 [B] receives the row's log-sum-exp at ``temperature``
    (what entropy_account reads).  tok int32 [B] and allow_table [V, ceil(V/32)]: the sampler's grammar and the rows' input
    tokens, both or neither.  The sampler then runs at the same ``temperature``"""
    ld = logits.shape[-1]
    B = logits.numel() // ld
    _check_tensor("entropy_mask", "logits", logits, torch.bfloat16, entries=B * ld)
    _check_tensor("entropy_mask", "mu", mu, torch.float32, entries=B, optional=True)
    _check_tensor("entropy_mask", "lse_out", lse_out, torch.float32, entries=B, optional=True)
    if (tok is None) != (allow_table is None):
        raise ValueError("entropy_mask: tok and allow_table are given together or not at all")
    _check_allow_table(allow_table, V, "entropy_mask")
    _check_tensor("entropy_mask", "tok", tok, torch.int32, entries=B, optional=True)
    _need_cuda(logits, mu, lse_out, tok, allow_table)
    check(_lib.load().mgx_entropy_mask(ptr(logits), int(V), ld, float(temperature), float(min_p), float(typical_p), ptr(mu),
                                       ptr(lse_out), ptr(tok), ptr(allow_table), B, stream_ptr()), "mgx_entropy_mask")
    return logits


def entropy_account(next_tok, logits, V, temperature, lse, pos_dev, mu=None, tau=0.0, eta=0.0, surprise_out=None, *, ragged=False,
                    base=None):
    """after the sampler and its advance, before budget_account: s = (lse[b] - logits[b, next_tok[b]] / temperature) / ln 2, the
    surprise in bits of the token just drawn, moves the Mirostat threshold -- mu[b] -= eta * (s - tau), ``mu`` float32 [B] -- and is
    filed in ``surprise_out`` float32 [B, out_ld] at the column the sampler has just written.  ``ragged`` / ``base`` as in
    sample_topk_topp"""
    ld = logits.shape[-1]
    B = logits.numel() // ld
    pos = _step_pos("entropy_account", pos_dev, B, ragged, base, with_base=True)
    _check_tensor("entropy_account", "logits", logits, torch.bfloat16, entries=B * ld)
    _check_tensor("entropy_account", "next_tok", next_tok, torch.int32, entries=B)
    _check_tensor("entropy_account", "lse", lse, torch.float32, entries=B)
    _check_tensor("entropy_account", "mu", mu, torch.float32, entries=B, optional=True)
    _check_tensor("entropy_account", "surprise_out", surprise_out, torch.float32, shape=(B, "out_ld"), optional=True)
    _need_cuda(next_tok, logits, lse, pos_dev, base, mu, surprise_out)
    check(_lib.load().mgx_entropy_account(ptr(next_tok), ptr(logits), int(V), ld, float(temperature), ptr(lse), ptr(mu), float(tau),
                                          float(eta), ptr(surprise_out), 0 if surprise_out is None else surprise_out.shape[1], *pos,
                                          B, stream_ptr()), "mgx_entropy_account")
    return mu


# ---- draft and verify on the decode path (ABI 32; contracts in include/mgx.h) ----------------------------------------
LOOKAHEAD_MAX_T = _lib.DEFINES["MGX_LOOKAHEAD_MAX_T"]
LOOKAHEAD_MAX_NGRAM = _lib.DEFINES["MGX_LOOKAHEAD_MAX_NGRAM"]


def _check_lookahead_T(what, T):
    if not 2 <= int(T) <= LOOKAHEAD_MAX_T:
        raise ValueError(f"{what}: T must lie in 2 .. {LOOKAHEAD_MAX_T}, got {T}")
    return int(T)


def lookahead_draft(tok, out_tokens, pos_dev, draft, pos_rows, Lmax, pad_token, *, guide=None, ngram=3, base=None):
    """the guesses of one draft-and-verify step: draft int32 [B, T] (column 0: tok) and pos_rows int32 [B * T] =
    min(pos_dev[b] + i, Lmax - 1).  ``guide`` int32 [B, guide_ld]: its columns; else the continuation of the latest earlier
    occurrence of the row's last ``ngram`` (then fewer) tokens in out_tokens int32 [B, out_ld], extended periodically; pad_token
    without a match.  pos_dev int32 [B], always one position per row; ``base`` as in sample_topk_topp"""
    what = "lookahead_draft"
    B = tok.numel()
    _check_tensor(what, "draft", draft, torch.int32, shape=(B, "T"))
    T = _check_lookahead_T(what, draft.shape[1])
    pos = _step_pos(what, pos_dev, B, True, base, with_base=True)
    _check_tensor(what, "tok", tok, torch.int32, entries=B)
    _check_tensor(what, "pos_rows", pos_rows, torch.int32, entries=B * T)
    _check_tensor(what, "out_tokens", out_tokens, torch.int32, shape=(B, "out_ld"))
    _check_tensor(what, "guide", guide, torch.int32, shape=(B, "guide_ld"), optional=True)
    if guide is None and not 1 <= int(ngram) <= LOOKAHEAD_MAX_NGRAM:
        raise ValueError(f"{what}: ngram must lie in 1 .. {LOOKAHEAD_MAX_NGRAM}, got {ngram}")
    _need_cuda(tok, out_tokens, pos_dev, base, guide, draft, pos_rows)
    check(_lib.load().mgx_lookahead_draft(ptr(tok), ptr(out_tokens), out_tokens.shape[1], pos[0], pos[1], ptr(guide),
                                          0 if guide is None else guide.shape[1], int(ngram), int(pad_token), ptr(draft),
                                          ptr(pos_rows), B, T, int(Lmax), stream_ptr()), "mgx_lookahead_draft")
    return draft


def rel_attn_decode_multi_splits(B, T, Lmax, d) -> int:
    return int(_lib.load().mgx_rel_attn_decode_multi_splits(B, T, Lmax, d))


def rel_attn_decode_multi_workspace(B, T, Lmax, d, device):
    """scratch for the split-K partials of mgx_rel_attn_decode_multi (None for one split), as rel_attn_decode_workspace"""
    n = _lib.load().mgx_rel_attn_decode_multi_workspace(B, T, Lmax, d)
    return torch.empty(n, dtype=torch.uint8, device=device) if n else None


def rel_attn_decode_multi(qkv_new, kcache, vcache, E, pos_dev, ctx, workspace, T):
    """the decode attention of T consecutive positions of every row: qkv_new bf16 [B * T, 3d], row b * T + i at position
    pos_dev[b] + i; kcache / vcache bf16 [B, h, Lmax, 64] receive the new rows below Lmax; ctx bf16 [B * T, d]; pos_dev int32 [B]
    on the device (each < Lmax: checked by the kernel, which then appends nothing)"""
    what = "rel_attn_decode_multi"
    T = _check_lookahead_T(what, T)
    if _check_kv_cache(kcache, vcache, None, None, what):
        raise ValueError(f"{what}: the caches must be bf16 (the draft-and-verify attention has no 8-bit form)")
    B, heads, Lmax, _ = kcache.shape
    d = heads * 64
    _check_tensor(what, "qkv_new", qkv_new, torch.bfloat16, shape=(B * T, 3 * d))
    _check_tensor(what, "ctx", ctx, torch.bfloat16, shape=(B * T, d))
    _check_tensor(what, "E", E, torch.bfloat16, shape=("M", 64))
    _step_pos(what, pos_dev, B, True)
    _need_cuda(qkv_new, kcache, vcache, E, pos_dev, ctx, workspace)
    check(_lib.load().mgx_rel_attn_decode_multi(ptr(qkv_new), ptr(kcache), ptr(vcache), ptr(E), ptr(pos_dev), ptr(ctx), ptr(workspace),
                                                0 if workspace is None else workspace.numel(), B, T, Lmax, d, E.shape[0],
                                                stream_ptr()), "mgx_rel_attn_decode_multi")
    return ctx


def lookahead_accept(logits, V, pos_dev, draft, limit, tok, out_tokens, done, *, probs_all=None, stats=None, temperature=1.0,
                     top_k=0, top_p=1.0, seed=0, allow_table=None, row0=0, base=None):
    """in place of the sampler of a draft-and-verify step: logits bf16 [B * T, ld]; position i of row b is drawn as
    sample_topk_topp draws it with (seed, base + pos + i, row0 + b) and the grammar row of draft[b, i]; the prefix of n draws whose
    guesses were right (at most up to column limit[b]) goes to out_tokens, the last of them to tok, pos_dev += n, the
    distributions to probs_all f32 [B, columns, V] and (1, n) to stats int32 [B, 2]; a row already at its limit sets done[b]"""
    what = "lookahead_accept"
    B = tok.numel()
    _check_tensor(what, "draft", draft, torch.int32, shape=(B, "T"))
    T = _check_lookahead_T(what, draft.shape[1])
    ld = logits.shape[-1]
    _check_tensor(what, "logits", logits, torch.bfloat16, entries=B * T * ld)
    pos = _step_pos(what, pos_dev, B, True, base, with_base=True)
    for name, t in (("limit", limit), ("tok", tok), ("done", done)):
        _check_tensor(what, name, t, torch.int32, entries=B)
    _check_tensor(what, "stats", stats, torch.int32, entries=2 * B, optional=True)
    _check_tensor(what, "out_tokens", out_tokens, torch.int32, shape=(B, "out_ld"))
    _check_tensor(what, "probs_all", probs_all, torch.float32, shape=(B, "columns", int(V)), optional=True)
    _check_allow_table(allow_table, V, "lookahead_accept")
    _need_cuda(logits, pos_dev, base, draft, limit, tok, out_tokens, probs_all, done, stats, allow_table)
    check(_lib.load().mgx_lookahead_accept(ptr(logits), int(V), ld, float(temperature), int(top_k), float(top_p), int(seed), pos[0],
                                           pos[1], ptr(draft), ptr(limit), ptr(tok), ptr(out_tokens), out_tokens.shape[1],
                                           ptr(probs_all), 0 if probs_all is None else probs_all.shape[1], ptr(done), ptr(stats), B, T,
                                           int(row0), ptr(allow_table), stream_ptr()), "mgx_lookahead_accept")
    return tok


# ---- held-note state on the decode path (ABI 28; contracts in include/mgx.h) -----------------------------------------
NOTE_WORDS = _lib.DEFINES["MGX_NOTE_WORDS"]               # int32 words of a row's state
NOTE_BITS = 32 * NOTE_WORDS                               # the bits a rule may name; max_on = NOTE_BITS is no cap


def _check_note_state(what, rule, state):
    """the held-note state: rule int32 [V], state int32 [B, NOTE_WORDS], both contiguous.  Returns B"""
    _check_tensor(what, "rule", rule, torch.int32, shape=("V",))
    _check_tensor(what, "state", state, torch.int32, shape=("B", NOTE_WORDS))
    return state.shape[0]


def notes_mask(logits, V, rule, state, max_on=NOTE_BITS):
    """in place, before the sampler: logits bf16 [B, ld] get -inf at every id v < V whose rule sets a bit that state[b] holds
    already -- or any bit, once the row holds ``max_on`` -- and at every id whose rule clears a bit the row does not hold;
    rule-0 ids and columns >= V stay bit for bit"""
    B = _check_note_state("notes_mask", rule, state)
    ld = logits.shape[-1]
    _check_tensor("notes_mask", "logits", logits, torch.bfloat16, entries=B * ld)
    if not 0 < int(V) <= min(ld, rule.numel()):
        raise ValueError(f"notes_mask: V must lie in 1 .. min(ld, the entries of rule) = {min(ld, rule.numel())}, got {V}")
    if not 1 <= int(max_on) <= NOTE_BITS:
        raise ValueError(f"notes_mask: max_on must lie in 1 .. {NOTE_BITS} ({NOTE_BITS}: no cap), got {max_on}")
    _need_cuda(logits, rule, state)
    check(_lib.load().mgx_notes_mask(ptr(logits), int(V), ld, ptr(rule), ptr(state), int(max_on), B, stream_ptr()), "mgx_notes_mask")
    return logits


def notes_account(next_tok, rule, state, V=None):
    """after the sampler: applies rule[next_tok[b]] to state[b] -- sets or clears the bit, whatever it was; a token outside
    0 .. V-1 (``V`` None: the entries of rule) and rule 0 leave the row alone"""
    B = _check_note_state("notes_account", rule, state)
    _check_tensor("notes_account", "next_tok", next_tok, torch.int32, shape=(B,))
    V = rule.numel() if V is None else int(V)
    if not 0 < V <= rule.numel():
        raise ValueError(f"notes_account: V must lie in 1 .. the entries of rule = {rule.numel()}, got {V}")
    _need_cuda(next_tok, rule, state)
    check(_lib.load().mgx_notes_account(ptr(next_tok), ptr(rule), ptr(state), V, B, stream_ptr()), "mgx_notes_account")
    return state


def notes_keep(first_tok, next_tok, out_tokens, pos_dev, rule, state, max_on=NOTE_BITS, V=None, *, ragged=False, base=None):
    """between the step's two draws and the accounts: a row whose first draw first_tok[b] -- made before notes_mask -- is legal
    under state[b] and ``max_on`` keeps it: next_tok[b] and out_tokens[b, base + pos] (the column the second draw was written
    to; ``out_tokens`` None: no column) receive it.  ``ragged`` / ``base`` as in sample_topk_topp"""
    B = _check_note_state("notes_keep", rule, state)
    pos = _step_pos("notes_keep", pos_dev, B, ragged, base, with_base=True)
    for name, t in (("first_tok", first_tok), ("next_tok", next_tok)):
        _check_tensor("notes_keep", name, t, torch.int32, shape=(B,))
    _check_tensor("notes_keep", "out_tokens", out_tokens, torch.int32, shape=(B, "out_ld"), optional=True)
    V = rule.numel() if V is None else int(V)
    if not 0 < V <= rule.numel():
        raise ValueError(f"notes_keep: V must lie in 1 .. the entries of rule = {rule.numel()}, got {V}")
    if not 1 <= int(max_on) <= NOTE_BITS:
        raise ValueError(f"notes_keep: max_on must lie in 1 .. {NOTE_BITS} ({NOTE_BITS}: no cap), got {max_on}")
    _need_cuda(first_tok, next_tok, out_tokens, pos_dev, base, rule, state)
    check(_lib.load().mgx_notes_keep(ptr(first_tok), ptr(next_tok), ptr(out_tokens), 0 if out_tokens is None else out_tokens.shape[1],
                                     *pos, ptr(rule), ptr(state), int(max_on), V, B, stream_ptr()), "mgx_notes_keep")
    return next_tok


# ---- train-time augmentation on the device (ABI 29; contract in include/mgx.h) ---------------------------------------
def crop_augment(corpus, start, avail, x, y, pad_token, *, perm=None, shift_row=None, stretch_q=None, ts0=0, n_ts=0, n_out=None,
                 time_major=False):
    """one crop per row out of ``corpus`` (16-bit ids, 1-D, on the device), stretched in time and transposed, written as the
    model's pair: with n = the ids that count per row, ``x`` and ``y`` int32 [B, n - 1] (the stream and the stream moved on by
    one), or ``x`` [B, n] alone with ``y`` None; ``time_major``: [n - 1, B] / [n, B] instead.  start int64 [B] and avail int32
    [B]: where a row's crop begins and how far its piece goes on from there.  perm int32 [S, V] with shift_row int32 [B] (the
    table's row per crop), stretch_q int32 [B] in per-mille with the codec's time run (ts0, n_ts): each optional.  Rows that run
    out of source end in pad_token; n_out int32 [B] (optional) receives the ids written per row.  Returns (x, y)"""
    what = "crop_augment"
    _check_tensor(what, "corpus", corpus, (torch.uint16, torch.int16), shape=("n",), at_least=1)
    _check_tensor(what, "x", x, torch.int32, shape=("rows", "columns"))
    _check_tensor(what, "y", y, torch.int32, shape=tuple(x.shape), optional=True)
    T, B = (x.shape[0], x.shape[1]) if time_major else (x.shape[1], x.shape[0])
    n = T + (1 if y is not None else 0)
    if B < 1 or T < 1:
        raise ValueError(f"crop_augment: x must hold at least one row and one column, got {tuple(x.shape)}")
    _check_tensor(what, "start", start, torch.int64, shape=(B,))
    _check_tensor(what, "avail", avail, torch.int32, shape=(B,))
    for name, t in (("shift_row", shift_row), ("stretch_q", stretch_q), ("n_out", n_out)):
        _check_tensor(what, name, t, torch.int32, shape=(B,), optional=True)
    if (perm is None) != (shift_row is None):
        raise ValueError("crop_augment: perm and shift_row go together: give both or neither")
    S, V = 0, 1
    if perm is not None:
        _check_tensor(what, "perm", perm, torch.int32, shape=("S", "V"), at_least=1)
        S, V = perm.shape
    if stretch_q is not None and not (int(ts0) >= 0 and int(n_ts) >= 1 and int(ts0) + int(n_ts) <= 65536):
        raise ValueError(f"crop_augment: a stretch needs the codec's time run inside the 16-bit ids, got ts0={ts0}, n_ts={n_ts}")
    stride_b, stride_t = (1, B) if time_major else (T, 1)
    _need_cuda(corpus, start, avail, x, y, perm, shift_row, stretch_q, n_out)
    check(_lib.load().mgx_crop_augment(ptr(corpus), corpus.numel(), ptr(start), ptr(avail), ptr(perm), S, V, ptr(shift_row),
                                       ptr(stretch_q), int(ts0), int(n_ts), ptr(x), ptr(y), stride_b, stride_t, ptr(n_out),
                                       int(pad_token), B, n, stream_ptr()), "mgx_crop_augment")
    return x, y


# ---- beam search on the decode path (ABI 22; contracts in include/mgx.h) ---------------------------------------------
def beam_select(logits, V, score, tok, parent, pos_rows, hist_tok, hist_parent, temperature=1.0, allow_table=None,
                stochastic=False, seed=0, advance=True):
    """the K best expansions of every prompt's K beams: logits bf16 [B*K, ld], score f32 [B, K] (in/out, -inf = dead beam),
    tok / parent / pos_rows int32 [B*K], hist_tok / hist_parent int32 [B*K, out_ld] (column pos + 1 is written)"""
    what = "beam_select"
    _check_tensor(what, "score", score, torch.float32, shape=("B", "K"))
    B, K = score.shape
    ld = logits.shape[-1]
    _check_tensor(what, "logits", logits, torch.bfloat16, entries=B * K * ld)
    for name, t in (("tok", tok), ("parent", parent), ("pos_rows", pos_rows)):
        _check_tensor(what, name, t, torch.int32, shape=(B * K,))
    _check_tensor(what, "hist_tok", hist_tok, torch.int32, shape=(B * K, "out_ld"))
    _check_tensor(what, "hist_parent", hist_parent, torch.int32, shape=tuple(hist_tok.shape))
    _check_allow_table(allow_table, V, "beam_select")
    _need_cuda(logits, score, tok, parent, pos_rows, hist_tok, hist_parent, allow_table)
    check(_lib.load().mgx_beam_select(ptr(logits), int(V), ld, float(temperature), ptr(score), ptr(tok), ptr(parent), ptr(pos_rows),
                                      ptr(hist_tok), ptr(hist_parent), hist_tok.shape[1], B, K, 1 if advance else 0,
                                      ptr(allow_table), 1 if stochastic else 0, int(seed), stream_ptr()), "mgx_beam_select")
    return tok


def kv_beam_reorder(dst, src, parent, pos_rows, K):
    """dst[r, h, :n_r] = src[(r // K) * K + parent[r], h, :n_r] with n_r = pos_rows[r], for one cache tensor [R, h, Lmax, 64]
    (bf16, or the 8-bit codes) or [R, h, Lmax] (f32: the 8-bit cache's scales); dst and src are two buffers of one shape"""
    what = "kv_beam_reorder"
    _check_tensor(what, "dst", dst, None, shape=("R", "h", "Lmax", 64) if dst.dim() == 4 else ("R", "h", "Lmax"))
    _check_tensor(what, "src", src, dst.dtype, shape=tuple(dst.shape))
    R, heads, Lmax = dst.shape[:3]
    row_bytes = dst.element_size() * (dst.shape[3] if dst.dim() == 4 else 1)
    if row_bytes not in (128, 64, 4):
        raise ValueError(f"kv_beam_reorder: rows of 64 bf16 values, 64 8-bit codes or one f32 scale, got {dst.dtype} {tuple(dst.shape)}")
    _check_tensor(what, "parent", parent, torch.int32, shape=(R,))
    _check_tensor(what, "pos_rows", pos_rows, torch.int32, shape=(R,))
    if R % int(K):
        raise ValueError(f"kv_beam_reorder: {R} rows are no multiple of the beam size {K}")
    _need_cuda(dst, src, parent, pos_rows)
    check(_lib.load().mgx_kv_beam_reorder(ptr(dst), ptr(src), ptr(parent), ptr(pos_rows), R, int(K), heads, Lmax, row_bytes,
                                          stream_ptr()), "mgx_kv_beam_reorder")
    return dst


def beam_backtrack(hist_tok, hist_parent, c0_rows, out, K, steps):
    """out[r, c0_r : c0_r + steps] = the tokens of final beam r, walked back through hist_parent (all int32 [R, out_ld])"""
    what = "beam_backtrack"
    _check_tensor(what, "out", out, torch.int32, shape=("R", "out_ld"))
    R = out.shape[0]
    _check_tensor(what, "hist_tok", hist_tok, torch.int32, shape=tuple(out.shape))
    _check_tensor(what, "hist_parent", hist_parent, torch.int32, shape=tuple(out.shape))
    _check_tensor(what, "c0_rows", c0_rows, torch.int32, shape=(R,))
    if R % int(K):
        raise ValueError(f"beam_backtrack: {R} rows are no multiple of the beam size {K}")
    _need_cuda(hist_tok, hist_parent, c0_rows, out)
    check(_lib.load().mgx_beam_backtrack(ptr(hist_tok), ptr(hist_parent), ptr(c0_rows), ptr(out), out.shape[1], R, int(K), int(steps),
                                         stream_ptr()), "mgx_beam_backtrack")
    return out


# ---- scoring (ABI 24; contracts in include/mgx.h) --------------------------------------------------------------------
def _score_outputs(rows, dev, want_lse):
    return (torch.empty(rows, dtype=torch.float32, device=dev), torch.empty(rows, dtype=torch.float32, device=dev) if want_lse else None,
            torch.empty(rows, dtype=torch.int32, device=dev))


def token_logprob(logits, target, temperature=1.0, prev=None, allow_table=None, want_lse=True):
    """log p(target) of every row of logits bf16 [..., V]: a view whose rows are evenly spaced in memory (columns contiguous, e.g.
    [B, Lp, V] cut out of [B, Lp, Vp]).  target (and prev, with allow_table uint32/int32 [V, ceil(V/32)]) int32, one per row.
    Returns (logp f32 [rows], lse f32 [rows] or None, hit int32 [rows])"""
    if logits.dim() < 1 or logits.dtype != BF16:
        raise ValueError(f"token_logprob: logits must be bf16 [..., V], got {logits.dtype} {tuple(logits.shape)}")
    V = logits.shape[-1]
    rows = logits.numel() // V if V else 0
    if V < 1 or rows < 1:
        raise ValueError(f"token_logprob: logits must hold at least one row of at least one column, got {tuple(logits.shape)}")
    # the leading dimensions must collapse into ONE row stride (dimensions of one entry have no say)
    lg, ld = logits, V
    dims = [(lg.shape[i], lg.stride(i)) for i in range(lg.dim() - 1) if lg.shape[i] != 1]
    if dims:
        ld = dims[-1][1]
    if (V > 1 and lg.stride(-1) != 1) or ld < V or any(dims[i][1] != dims[i + 1][1] * dims[i + 1][0] for i in range(len(dims) - 1)):
        raise ValueError(f"token_logprob: the rows of logits must be evenly spaced and their columns contiguous "
                         f"(shape {tuple(lg.shape)}, strides {lg.stride()})")
    _check_tensor("token_logprob", "target", target, torch.int32, entries=rows)
    _check_tensor("token_logprob", "prev", prev, torch.int32, entries=rows, optional=True)
    if (prev is None) != (allow_table is None):
        raise ValueError("token_logprob: prev and allow_table are given together or not at all")
    _check_allow_table(allow_table, V, "token_logprob")
    if not lg.is_cuda:                                        # a strided view: _need_cuda would ask for a contiguous one
        raise _lib.MgxError("mgx ops need CUDA/HIP tensors (no CPU fallback); got a CPU tensor")
    _need_cuda(target, prev, allow_table)
    logp, lse, hit = _score_outputs(rows, lg.device, want_lse)
    check(_lib.load().mgx_token_logprob(ptr(lg), V, int(ld), ptr(target), ptr(prev), ptr(allow_table), float(temperature), ptr(logp),
                                        ptr(lse), ptr(hit), rows, stream_ptr()), "mgx_token_logprob")
    return logp, lse, hit


def linear_logprob(a, w, bias, target, temperature=1.0, want_lse=True):
    """log p(target) under softmax((a w^T + bias) / temperature) without storing the logits: a bf16 [M, K], w bf16 [V, K], bias f32
    [V] or None, target int32 [M].  Returns (logp f32 [M], lse f32 [M] or None, hit int32 [M])"""
    what = "linear_logprob"
    _check_tensor(what, "a", a, BF16, shape=("M", "K"))
    M, K = a.shape
    _check_tensor(what, "w", w, BF16, shape=("V", K))
    V = w.shape[0]
    _check_tensor(what, "bias", bias, torch.float32, shape=(V,), optional=True)
    _check_tensor(what, "target", target, torch.int32, entries=M)
    _need_cuda(a, w, bias, target)
    logp, lse, hit = _score_outputs(M, a.device, want_lse)
    check(_lib.load().mgx_linear_logprob(ptr(a), ptr(w), ptr(bias), ptr(target), float(temperature), ptr(logp), ptr(lse), ptr(hit), M, V,
                                         K, stream_ptr()), "mgx_linear_logprob")
    return logp, lse, hit


def score_reduce(logp, hit):
    """per-row totals of logp f32 [B, L] and hit int32 [B, L]: (sum f64 [B] over the entries with hit >= 0, their count int32 [B],
    the count of hit == 1 int32 [B])"""
    _check_tensor("score_reduce", "logp", logp, torch.float32, shape=("B", "L"))
    _check_tensor("score_reduce", "hit", hit, torch.int32, shape=tuple(logp.shape))
    _need_cuda(logp, hit)
    B, L = logp.shape
    total = torch.empty(B, dtype=torch.float64, device=logp.device)
    count = torch.empty(B, dtype=torch.int32, device=logp.device)
    hits = torch.empty(B, dtype=torch.int32, device=logp.device)
    check(_lib.load().mgx_score_reduce(ptr(logp), ptr(hit), ptr(total), ptr(count), ptr(hits), B, L, stream_ptr()), "mgx_score_reduce")
    return total, count, hits


# --------------------------------------------------------------------------------------------------
# autograd glue
#
# Master (fp32) parameters are passed to each Function only to anchor the autograd graph: their
# gradients are NOT returned (None) but accumulated by the kernels straight into the fp32 views of
# the model's flat gradient buffer (``g*`` arguments).  ``done`` is an optional callable invoked at
# the end of backward (the data-parallel bucket hook, see dp.py).
# --------------------------------------------------------------------------------------------------
class _EmbedPE(torch.autograd.Function):
    """K1: dropout(emb[x]*sqrt(d) + PE)                       layers.py:226-229"""

    @staticmethod
    def forward(ctx, tok, table, pe, p_drop, seed, gtable, done):
        ctx.save_for_backward(tok)
        ctx.cfg = (p_drop, seed, gtable, done)
        return embed_pe_fwd(tok, table, pe, p_drop, seed)

    @staticmethod
    def backward(ctx, dout):
        (tok,) = ctx.saved_tensors
        p_drop, seed, gtable, done = ctx.cfg
        embed_bwd(tok, dout.contiguous(), gtable, p_drop, seed)
        if done is not None:
            done()
        join_side_stream(tok.device)      # last node of the backward: every gradient is complete in this stream's order
        return None, None, None, None, None, None, None


class _Linear(torch.autograd.Function):
    """K2/K5/K7/K8: y = act(x @ W^T + b) and its backward, all libmgx MFMA kernels:
    forward NT GEMM with fused bias/ReLU; dx = dy @ W (NN, transposed LDS reads); dW += dy^T @ x and
    db += colsum(dy) accumulate in fp32 straight into the flat gradient buffer (TN, split-M atomics).
    ``x_is_relu``: x is the output of a fused-ReLU layer, so dx is masked by (x > 0) in the dX
    epilogue -- that producer (act=1) then receives an already-masked gradient."""

    @staticmethod
    def forward(ctx, x, w_master, w_shadow, bias, act, gw, gb, done, x_is_relu):
        y = linear_fwd(x, w_shadow, bias, act)
        ctx.save_for_backward(x, w_shadow)
        ctx.cfg = (gw, gb, done, x_is_relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_shadow = ctx.saved_tensors
        gw, gb, done, x_is_relu = ctx.cfg
        dy = dy.contiguous()
        dx = linear_dx(dy, w_shadow, x if x_is_relu else None)
        linear_dw(dy, x, gw, gb)
        if done is not None:
            done()
        return dx, None, None, None, None, None, None, None, None


class LayerParams:
    """Views one encoder layer's kernels need (bf16 shadow weights, fp32 biases / LayerNorm parameters and
    the fp32 gradient slots they accumulate into); built once per model by network.MusicTransformer."""
    __slots__ = ("wqkv", "bqkv", "gqkv", "gbqkv", "E", "gE", "wfc", "bfc", "gwfc", "gbfc", "g1", "b1", "gg1", "gb1",
                 "wpre", "bpre", "gwpre", "gbpre", "wsuf", "bsuf", "gwsuf", "gbsuf", "g2", "b2", "gg2", "gb2")


class _EncoderLayer(torch.autograd.Function):
    """One whole post-LN block (layers.py:152-161) as a single autograd node: 7 kernels forward, 14 backward.
    Doing the block in one node lets the gradient that arrives over each residual connection join the
    branch's input gradient inside the dX GEMM epilogue (``addend``) instead of a separate elementwise pass,
    and frees each intermediate as soon as its last consumer has run."""

    @staticmethod
    def forward(ctx, h, lp, padbits, p_drop, seed, done, wsink):
        qkv = linear_fwd(h, lp.wqkv, lp.bqkv, 0)
        att, lse = rel_attn_fwd(qkv, lp.E, padbits)
        if wsink is not None:
            wsink.append(rel_attn_weights(qkv, lp.E, padbits, lse))
        a = linear_fwd(att, lp.wfc, lp.bfc, 0)
        o1, mean1, rstd1 = add_ln_fwd(a, h, lp.g1, lp.b1, 1e-6, p_drop, seed + 1)
        f1 = linear_fwd(o1, lp.wpre, lp.bpre, 1)
        f2 = linear_fwd(f1, lp.wsuf, lp.bsuf, 0)
        out, mean2, rstd2 = add_ln_fwd(f2, o1, lp.g2, lp.b2, 1e-6, p_drop, seed + 2)
        ctx.save_for_backward(h, qkv, att, lse, a, o1, f1, f2, mean1, rstd1, mean2, rstd2)
        ctx.cfg = (lp, padbits, p_drop, seed, done)
        return out

    @staticmethod
    def backward(ctx, dout):
        h, qkv, att, lse, a, o1, f1, f2, mean1, rstd1, mean2, rstd2 = ctx.saved_tensors
        lp, padbits, p_drop, seed, done = ctx.cfg
        # LN2 <- FFN_suf <- ReLU <- FFN_pre, residual o1
        df2, dres2 = add_ln_bwd(dout.contiguous(), f2, o1, lp.g2, mean2, rstd2, lp.gg2, lp.gb2, p_drop, seed + 2, lp.gbsuf)
        df1 = linear_dx(df2, lp.wsuf, f1)
        do1 = linear_dx(df1, lp.wpre, None, dres2)
        del dres2
        # LN1 <- fc <- attention <- QKV, residual h
        da, dres1 = add_ln_bwd(do1, a, h, lp.g1, mean1, rstd1, lp.gg1, lp.gb1, p_drop, seed + 1, lp.gbfc)
        del do1
        datt = linear_dx(da, lp.wfc)
        plan = None if torch.cuda.is_current_stream_capturing() else stream_plan(h.device)
        if plan is None or plan.side is None:
            dqkv = rel_attn_bwd(qkv, lp.E, padbits, att, datt, lse, lp.gE)
            del datt
            dh = linear_dx(dqkv, lp.wqkv, None, dres1)
            # the block's four weight gradients (and the two bias gradients that are not LayerNorm by-products) in one launch
            linear_dw_grouped([(dqkv, h, lp.gqkv, lp.gbqkv), (da, att, lp.gwfc, None), (df1, o1, lp.gwpre, lp.gbpre),
                               (df2, f1, lp.gwsuf, None)])
            if done is not None:
                done()
            return dh, None, None, None, None, None, None
        # Two streams (configure_streams): dE and the weight gradients feed only the optimiser (and the bucket's all-reduce), and
        # both run at the HBM rate -- they go to the CU-masked side stream, behind an event recorded once dK/dV (the dS tiles) and
        # dQ (dqkv complete) are issued, while this stream carries on with the dX of the QKV projection and the next block's
        # backward, whose heavy kernels are MFMA-bound.  The bucket callback runs in the side stream's context: the all-reduce
        # it issues is ordered behind the gradients written there (everything this stream wrote into the bucket -- the
        # LayerNorm and bias column sums -- precedes the event).
        main, side = torch.cuda.current_stream(), plan.side.stream
        B, L, _ = qkv.shape
        ws = torch.empty(_lib.load().mgx_rel_attn_bwd_workspace(B, L, qkv.shape[2] // 3), dtype=torch.uint8, device=qkv.device)
        de_side, dw_side = bool(plan.work & 1), bool(plan.work & 2)
        dqkv = rel_attn_bwd(qkv, lp.E, padbits, att, datt, lse, lp.gE, parts=(1 | 4 | 2) if de_side else 15, workspace=ws)
        ready = torch.cuda.Event()
        ready.record(main)
        dh = linear_dx(dqkv, lp.wqkv, None, dres1)
        group = [(dqkv, h, lp.gqkv, lp.gbqkv), (da, att, lp.gwfc, None), (df1, o1, lp.gwpre, lp.gbpre), (df2, f1, lp.gwsuf, None)]
        if not dw_side:
            linear_dw_grouped(group)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            if de_side:
                rel_attn_bwd(qkv, lp.E, padbits, att, datt, lse, lp.gE, parts=8, dqkv=dqkv, workspace=ws)
            if dw_side:
                linear_dw_grouped(group)
            if done is not None:
                if not dw_side:                            # the weight gradients were issued on the other stream, after `ready`
                    again = torch.cuda.Event()
                    again.record(main)
                    side.wait_event(again)
                done()
            plan.last = torch.cuda.Event()
            plan.last.record(side)
        # allocated on this stream, read on the other: the caching allocator must not hand the blocks out again before the side
        # stream is through with them
        for t in (qkv, att, datt, lse, ws, dqkv, h, da, df1, o1, df2, f1, padbits):
            if t is not None:
                t.record_stream(side)
        return dh, None, None, None, None, None, None


def encoder_layer(h, lp, padbits, p_drop, seed, done=None, wsink=None):
    return _EncoderLayer.apply(h, lp, padbits, p_drop, seed, done, wsink)


class _SmoothCE(torch.autograd.Function):
    """K9+K10: smoothed CE (mean over non-pad) with accuracy/argmax side outputs.   criterion.py:43-67"""

    @staticmethod
    def forward(ctx, logits, target, V, eps_ls, pad):
        stats, argmax, row_lse = smooth_ce_fwd(logits, target, V, eps_ls, pad)
        ctx.save_for_backward(logits, target, stats, row_lse)
        ctx.cfg = (V, eps_ls, pad)
        ctx.mark_non_differentiable(stats, argmax)
        loss = stats[0] / stats[1]
        return loss, stats, argmax

    @staticmethod
    def backward(ctx, gloss, _gs, _ga):
        logits, target, stats, row_lse = ctx.saved_tensors
        V, eps_ls, pad = ctx.cfg
        # gloss is a 0-d device tensor: the kernel reads it on the device (no host sync, no second pass over dlogits)
        dl = smooth_ce_bwd(logits, target, stats, row_lse, V, eps_ls, pad, 1.0, gloss.detach().to(torch.float32).contiguous())
        return dl, None, None, None, None


def embed_pe(tok, table, pe, p_drop=0.0, seed=0, gtable=None, done=None):
    return _EmbedPE.apply(tok, table, pe, float(p_drop), int(seed), gtable, done)


# --------------------------------------------------------------------------------------------------
# Stand-alone autograd nodes: the layer-level call surface of the reference (layers.py:64-109,152-161,
# 223-233 -- ``rga([q,k,v], mask)``, ``EncoderLayer(x, mask)``, ``Encoder(x, mask)``).  Unlike the nodes
# above they take ordinary fp32 Parameters, round them to bf16 per call and RETURN their gradients, so a
# layer works on its own with any torch optimizer.  Same kernels; the model's training path keeps using the
# flat-buffer nodes above (no per-call rounding, gradients accumulated in place).
# --------------------------------------------------------------------------------------------------
class _LinearStd(torch.autograd.Function):
    """y = act(x @ W^T + b) with returned gradients.  A reduction length that is no multiple of the GEMMs' granule of 64 (the FFN's
    second projection at d_model = 64 * odd: K = d / 2) is zero-padded here, per call; the model's flat-buffer path pads once,
    inside its buffers (network._flat_order)."""

    @staticmethod
    def forward(ctx, x, weight, bias, act):
        w16 = weight.detach().to(BF16).contiguous()
        K = w16.shape[1]
        Kp = (K + 63) // 64 * 64
        if Kp != K:
            w16 = torch.nn.functional.pad(w16, (0, Kp - K))
            x = torch.nn.functional.pad(x, (0, Kp - K))
        y = linear_fwd(x.contiguous(), w16, None if bias is None else bias.detach().float().contiguous(), act)
        ctx.save_for_backward(x, w16, y if act else None)
        ctx.meta = (weight.dtype, bias is not None, bias.dtype if bias is not None else None, K)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w16, y = ctx.saved_tensors
        wdt, has_b, bdt, K = ctx.meta
        dy = dy.contiguous()
        gw = torch.zeros(w16.shape, dtype=torch.float32, device=dy.device)
        gb = torch.zeros(w16.shape[0], dtype=torch.float32, device=dy.device) if has_b else None
        if y is not None:                           # ReLU output: mask the incoming gradient once, for dx and dW alike
            dy = torch.where(y > 0, dy, torch.zeros_like(dy))
        dx = linear_dx(dy, w16)
        linear_dw(dy, x, gw, gb)
        if w16.shape[1] != K:
            dx, gw = dx[..., :K], gw[:, :K]
        return dx, gw.to(wdt), (gb.to(bdt) if has_b else None), None


class _RelAttnStd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, E, padbits):
        e16 = E.detach().to(BF16).contiguous()
        att, lse = rel_attn_fwd(qkv, e16, padbits)
        ctx.save_for_backward(qkv, e16, att, lse)
        ctx.padbits, ctx.edt = padbits, E.dtype
        ctx.mark_non_differentiable(lse)
        return att, lse

    @staticmethod
    def backward(ctx, datt, _dlse):
        qkv, e16, att, lse = ctx.saved_tensors
        dE = torch.zeros(e16.shape, dtype=torch.float32, device=qkv.device)
        dqkv = rel_attn_bwd(qkv, e16, ctx.padbits, att, datt.contiguous(), lse, dE)
        return dqkv, dE.to(ctx.edt), None


class _AddLNStd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps, p_drop, seed):
        g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        out, mean, rstd = add_ln_fwd(x, res, g32, b32, eps, p_drop, seed)
        ctx.save_for_backward(x, res, g32, mean, rstd)
        ctx.meta = (p_drop, seed, gamma.dtype, beta.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, res, g32, mean, rstd = ctx.saved_tensors
        p_drop, seed, gdt, bdt = ctx.meta
        dg, db = torch.zeros_like(g32), torch.zeros_like(g32)
        dx, dres = add_ln_bwd(dout.contiguous(), x, res, g32, mean, rstd, dg, db, p_drop, seed)
        return dx, dres, dg.to(gdt), db.to(bdt), None, None, None


def linear_std(x, weight, bias=None, act=0):
    return _LinearStd.apply(x, weight, bias, int(act))


def rel_attn_std(qkv, E, padbits):
    return _RelAttnStd.apply(qkv, E, padbits)


def add_ln_std(x, res, gamma, beta, eps=1e-6, p_drop=0.0, seed=0):
    return _AddLNStd.apply(x, res, gamma, beta, float(eps), float(p_drop), int(seed))


def linear(x, w_master, w_shadow, bias, act, gw, gb, done=None, x_is_relu=False):
    return _Linear.apply(x, w_master, w_shadow, bias, int(act), gw, gb, done, bool(x_is_relu))


def smooth_ce(logits, target, V, eps_ls, pad):
    """returns (loss scalar tensor, stats f32[4], argmax int32[rows])"""
    return _SmoothCE.apply(logits, target, int(V), float(eps_ls), int(pad))
