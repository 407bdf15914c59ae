"""Host side of ``MusicTransformer.score``: the argument checks, the window schedule of sequences longer than the model's
window, and the figures reported from the totals.  Nothing here touches a device (the CPU tests import it alone); the driver
that runs the kernels is ``score`` at the end, called by ``network.MusicTransformer.score``.

Event i of row b is SCORED iff i >= max(1, from_pos[b]), i < lengths[b] (when lengths are given) and x[b, i] != pad_token;
column 0 never is -- the model has no start token.  An unscored event has logp 0 and hit -1 and reaches the kernels as target -1.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple

LOGIT_PATHS = ("auto", "fp32", "bf16")
FUSED_KMAX = 1024                 # mgx_linear_logprob: 32 rows x 1024 x 2 B of LDS


def default_stride(W: int) -> int:
    return max(1, W // 2)


def score_schedule(n: int, W: int, stride: Optional[int] = None) -> List[Tuple[int, int, int]]:
    """the windows that score a sequence of ``n`` events with a model window of ``W``: [(start, width, first_scored)], window k
    covering events start .. start + width - 1 (renumbered from position 0, as a training crop is) and scoring its own columns
    first_scored .. width - 1.  start_k = min(k * stride, n - W) until start_k == n - W; window 0 scores columns 1 .. W - 1, window
    k > 0 from the previous window's end up to its own.  Every event 1 .. n - 1 is scored exactly once, and outside window 0
    with at least W - stride events of context.  n <= W: one window."""
    if W < 2:
        raise ValueError(f"the window must hold at least 2 events, got {W}")
    stride = default_stride(W) if stride is None else int(stride)
    if not 1 <= stride <= W - 1:
        raise ValueError(f"stride must lie in 1 .. window - 1 = {W - 1}, got {stride}")
    if n <= W:
        return [(0, max(int(n), 0), 1)]
    out, k, end = [], 0, 1
    while True:
        start = min(k * stride, n - W)
        out.append((start, W, end - start))
        end = start + W
        if start == n - W:
            return out
        k += 1


def resolve_logits(logits: str, grammar, d: int) -> str:
    if logits not in LOGIT_PATHS:
        raise ValueError(f"logits must be one of {LOGIT_PATHS}, got {logits!r}")
    if logits == "fp32" and grammar is not None:
        raise ValueError("grammar is applied to stored logits: logits='fp32' (the fused projection) takes none; use 'bf16' or 'auto'")
    if logits == "fp32" and d > FUSED_KMAX:
        raise ValueError(f"logits='fp32' needs d <= {FUSED_KMAX} (the fused projection holds 32 rows in LDS), got d = {d}")
    if logits == "auto":
        return "bf16" if (grammar is not None or d > FUSED_KMAX) else "fp32"
    return logits


def check_args(max_seq: int, d: int, B: int, L: int, lengths=None, from_pos=None, temperature: float = 1.0, grammar=None,
               logits: str = "auto", window: Optional[int] = None, stride: Optional[int] = None):
    """every refusal of MusicTransformer.score (ValueError), on the host.  Returns (path: 'fp32' or 'bf16'; W; stride; lens: the
    per-row lengths as ints or None; from_pos: per-row ints)"""
    path = resolve_logits(logits, grammar, d)
    if not temperature > 0:
        raise ValueError(f"temperature must be > 0, got {temperature}")
    W = max_seq if window is None else int(window)
    if not 2 <= W <= max_seq:
        raise ValueError(f"window must lie in 2 .. max_seq ({max_seq}), got {window}")
    stride = default_stride(W) if stride is None else int(stride)
    if not 1 <= stride <= W - 1:
        raise ValueError(f"stride must lie in 1 .. window - 1 = {W - 1}, got {stride}")
    if B < 1 or L < 1:
        raise ValueError(f"x must be [B, L] with B, L >= 1, got [{B}, {L}]")
    lens = None
    if lengths is not None:
        lens = [int(v) for v in _as_list(lengths)]
        if len(lens) != B:
            raise ValueError(f"lengths has {len(lens)} entries for a batch of {B} rows")
        if any(not 0 <= v <= L for v in lens):
            raise ValueError(f"lengths must lie in 0 .. {L} (the width of x), got {lens}")
    if from_pos is None:
        fp = [0] * B
    else:
        fp = [int(v) for v in _as_list(from_pos)]
        if len(fp) == 1:
            fp = fp * B
        if len(fp) != B:
            raise ValueError(f"from_pos has {len(fp)} entries for a batch of {B} rows")
        if any(v < 0 for v in fp):
            raise ValueError(f"from_pos must be >= 0, got {fp}")
    return path, W, stride, lens, fp


def _as_list(v):
    if hasattr(v, "tolist"):
        v = v.tolist()
    return list(v) if isinstance(v, (list, tuple)) else [v]


def plan_windows(ns: List[int], L: int, W: int, stride: int):
    """the windows of a batch whose rows hold ns[b] events (of a matrix [B, L]): a list of (row, start, width, first_scored)
    sorted by width (windows are batched by width) and, per (row, column), the (window, column) that scores it -- window -1
    where nothing does"""
    wins = []
    for b, n in enumerate(ns):
        if n >= 2:
            wins += [(b, s, w, f) for (s, w, f) in score_schedule(n, W, stride)]
    wins.sort(key=lambda t: (-t[2], t[0], t[1]))
    src = [[(-1, 0)] * L for _ in ns]
    for k, (b, s, w, f) in enumerate(wins):
        for j in range(f, w):
            src[b][s + j] = (k, j)
    return wins, src


def figures(total: float, count: int, hits: int) -> dict:
    """events, nats / bits per event, perplexity and top-1 accuracy of a total log-probability"""
    if count <= 0:
        return dict(events=0, nats_per_event=float("nan"), bits_per_event=float("nan"), perplexity=float("nan"), accuracy=float("nan"))
    nats = -total / count
    return dict(events=int(count), nats_per_event=nats, bits_per_event=nats / math.log(2.0),
                perplexity=math.exp(nats) if nats < 700 else float("inf"), accuracy=hits / count)


# ----------------------------------------------------------------------------------------------------------------------
# the driver (needs torch and a device)
# ----------------------------------------------------------------------------------------------------------------------
def _score_block(model, tok, tgt, temperature, table, path):
    """one forward of tok int32 [N, n] (n <= max_seq) -> (logp f32, hit int32) [N, n]: column i holds the score of tgt[:, i] given
    tok[:, :i]; tgt < 0 is unscored"""
    import torch
    from . import ops
    N, n = tok.shape
    n_pad = (n + 31) // 32 * 32     # the forward pads to the kernels' 32-row tile and hands back all its rows
    # the row of position i predicts event i + 1
    nxt = torch.full((N, n_pad), -1, dtype=torch.int32, device=tok.device)
    nxt[:, : n - 1] = tgt[:, 1:]
    if path == "fp32":
        h = model._hidden(tok)                                # [N, n_pad, d]
        st = model.store()
        Vp, d = model.vocab_padded, model.embedding_dim
        lp, _, hit = ops.linear_logprob(h.reshape(N * n_pad, d), st.padded_view("fc.weight", Vp, d)[: model.vocab_size],
                                        st.padded_view("fc.bias", Vp, None, "param")[: model.vocab_size], nxt.view(-1), temperature)
    else:
        logits = model._logits_padded(tok)[:, :, : model.vocab_size]      # [N, n_pad, V], a view of [N, n_pad, Vp]
        prev = None
        if table is not None:
            prev = torch.full((N, n_pad), model.pad_token, dtype=torch.int32, device=tok.device)
            prev[:, :n] = tok
        lp, _, hit = ops.token_logprob(logits, nxt, temperature, prev=prev, allow_table=table)
    lp, hit = lp.view(N, n_pad), hit.view(N, n_pad)
    logp = torch.cat([torch.zeros(N, 1, dtype=torch.float32, device=tok.device), lp[:, : n - 1]], 1)
    hits = torch.cat([torch.full((N, 1), -1, dtype=torch.int32, device=tok.device), hit[:, : n - 1]], 1)
    return logp, hits


def score(model, x, lengths=None, from_pos=None, temperature=1.0, grammar=None, logits="auto", window=None, stride=None):
    """MusicTransformer.score (see there); the model is in eval mode"""
    import numpy as np
    import torch
    from . import ops
    if x.dim() != 2:
        raise ValueError(f"x must be [B, L], got {tuple(x.shape)}")
    B, L = x.shape
    path, W, stride, lens, fp = check_args(model.max_seq, model.embedding_dim, B, L, lengths, from_pos, temperature, grammar, logits,
                                           window, stride)
    dev = x.device
    table = ops.grammar_table(grammar, dev)
    tok = x.to(torch.int32).contiguous()
    col = torch.arange(L, device=dev, dtype=torch.int32)[None, :]
    first = torch.tensor([max(1, v) for v in fp], dtype=torch.int32).to(dev)[:, None]
    scored = (col >= first) & (tok != model.pad_token)
    if lens is not None:
        scored &= col < torch.tensor(lens, dtype=torch.int32).to(dev)[:, None]
    tgt = torch.where(scored, tok, torch.full_like(tok, -1))
    ns = lens if lens is not None else [L] * B
    if L <= W:
        logp, hit = _score_block(model, tok, tgt, temperature, table, path)
    else:
        wins, src = plan_windows(ns, L, W, stride)
        Wm = min(W, L)
        outs_lp, outs_hit = [], []
        for k0 in range(0, len(wins), B):                     # batches of at most B windows, widest first
            part = wins[k0:k0 + B]
            wd = part[0][2]
            rows = torch.tensor([p[0] for p in part], dtype=torch.int64).to(dev)[:, None]
            start = torch.tensor([p[1] for p in part], dtype=torch.int64).to(dev)[:, None]
            width = torch.tensor([p[2] for p in part], dtype=torch.int64).to(dev)[:, None]
            fsc = torch.tensor([p[3] for p in part], dtype=torch.int64).to(dev)[:, None]
            j = torch.arange(wd, device=dev, dtype=torch.int64)[None, :]
            cols = (start + j).clamp(max=L - 1)
            inside = j < width
            wtok = torch.where(inside, tok[rows, cols], torch.full((), model.pad_token, dtype=torch.int32, device=dev))
            wtgt = torch.where(inside & (j >= fsc), tgt[rows, cols], torch.full((), -1, dtype=torch.int32, device=dev))
            lp, ht = _score_block(model, wtok.contiguous(), wtgt.contiguous(), temperature, table, path)
            if wd < Wm:
                lp = torch.nn.functional.pad(lp, (0, Wm - wd), value=0.0)
                ht = torch.nn.functional.pad(ht, (0, Wm - wd), value=-1)
            outs_lp.append(lp)
            outs_hit.append(ht)
        # every (row, column) takes the value of the window that scores it; the rest take an unscored entry
        outs_lp.append(torch.zeros(1, Wm, dtype=torch.float32, device=dev))
        outs_hit.append(torch.full((1, Wm), -1, dtype=torch.int32, device=dev))
        all_lp, all_hit = torch.cat(outs_lp, 0), torch.cat(outs_hit, 0)
        s = np.asarray(src, dtype=np.int64).reshape(B, L, 2)
        sw = torch.from_numpy(np.where(s[..., 0] < 0, len(wins), s[..., 0])).to(dev)
        sc = torch.from_numpy(s[..., 1].copy()).to(dev)
        logp, hit = all_lp[sw, sc].contiguous(), all_hit[sw, sc].contiguous()
    total, count, hits = ops.score_reduce(logp, hit)
    return dict(logp=logp, hit=hit, sum=total, count=count, hits=hits)
