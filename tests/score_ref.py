"""fp64 / numpy references of the three scoring contracts of include/mgx.h (ABI 24), written from the header, and their fp32
twins: a plain helper module of the scoring tests, CPU only.  A twin is the same formula in fp32 with its sum taken in the
reverse order -- not a reference, a second evaluation whose distance from the fp64 one is what fp32 does to the formula."""
import numpy as np
import torch

from oracle import decode_ref as D
from oracle import train_ref as T

NEG = -np.inf


def inv_temperature(temperature) -> float:
    """the header's (1 / temperature): an f32 quantity ('all arithmetic is f32'), as fp64"""
    return float(np.float32(1.0) / np.float32(temperature))


def allowed_rows(allow_table, prev, logits):
    """bool [rows, V]: the ids a row's log-softmax runs over.  None -> all.  A table row that leaves no finite logit (the
    NaN-ignoring maximum over its ids is -inf) is ignored for that row"""
    x = np.asarray(logits, dtype=np.float64)
    if allow_table is None:
        return np.ones(x.shape, bool)
    ok = D.allowed_mask(allow_table, prev, x.shape[1])
    with np.errstate(invalid="ignore"):
        mx = np.fmax.reduce(np.where(ok, x, NEG), axis=1, initial=NEG)
    return np.where((mx == NEG)[:, None], True, ok)


def _finish(x, ok, raw, target, lse):
    """logp, hit from x [rows, V] (fp64 or fp32), the allowed mask, the raw values hit compares, and lse"""
    rows, V = x.shape
    t = np.asarray(target).astype(np.int64)
    scored = (t >= 0) & (t < V)
    tc = np.clip(t, 0, V - 1)
    r = np.arange(rows)
    with np.errstate(invalid="ignore"):
        xt = np.where(ok[r, tc], x[r, tc], NEG)
        logp = np.where(scored, xt - lse, 0.0)
        masked = np.where(ok & ~np.isnan(raw), raw, NEG)      # a NaN never wins; -0 == +0 in any comparison
    first = np.argmax(masked == masked.max(1, keepdims=True), axis=1)          # the smallest id at the maximum
    hit = np.where(scored, ((first == tc) & ok[r, tc]).astype(np.int64), -1)
    return logp, hit


def lse_rows(x, ok, dtype=np.float64, reverse=False):
    """logsumexp over the allowed ids; NaN for a row that holds a NaN or +inf among them, or nothing above -inf"""
    x = np.where(ok, x, dtype(NEG)).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        bad = (np.isnan(x) | (x == np.inf)).any(1) | ~(np.fmax.reduce(x, axis=1, initial=NEG) > NEG)
        m = np.fmax.reduce(x, axis=1, initial=NEG).astype(dtype)
        e = np.exp((x - m[:, None]).astype(dtype)).astype(dtype)
        if reverse:
            e = e[:, ::-1]
        s = np.cumsum(e, axis=1, dtype=dtype)[:, -1] if dtype == np.float32 else e.sum(1)        # cumsum: one add after another
        lse = (m + np.log(s).astype(dtype)).astype(dtype)
    return np.where(bad, dtype(np.nan), lse)


def token_logprob(logits, target, temperature=1.0, allow_table=None, prev=None, dtype=np.float64, reverse=False):
    """mgx_token_logprob on logits [rows, V] (the V real columns; the exact values the kernel reads) -> dict(logp, lse, hit, xt)"""
    raw = np.asarray(T._d(logits))
    ok = allowed_rows(allow_table, prev, raw)
    x = (raw.astype(dtype) * dtype(inv_temperature(temperature))).astype(dtype)
    lse = lse_rows(x, ok, dtype, reverse)
    logp, hit = _finish(x, ok, raw, target, lse)
    t = np.clip(np.asarray(target).astype(np.int64), 0, raw.shape[1] - 1)
    return dict(logp=logp, lse=lse, hit=hit, xt=x[np.arange(len(t)), t].astype(np.float64))


def token_floor(logits, target, temperature, allow_table, prev, ref):
    """per row: |fp32 twin with the sum reversed - ref| + ulp32(max(|x_t|, |lse|)), for logp and for lse"""
    tw = token_logprob(logits, target, temperature, allow_table, prev, np.float32, True)
    with np.errstate(invalid="ignore"):
        ulp = np.asarray(T.ulp32(np.nan_to_num(np.maximum(np.abs(ref["xt"]), np.abs(ref["lse"])), nan=0.0, posinf=0.0, neginf=0.0)))
        f_lp = np.nan_to_num(np.abs(tw["logp"].astype(np.float64) - ref["logp"]), nan=0.0, posinf=0.0) + ulp
        f_lse = np.nan_to_num(np.abs(tw["lse"].astype(np.float64) - ref["lse"]), nan=0.0, posinf=0.0) + ulp
    return f_lp, f_lse


def linear_logprob(a, w, bias, target, temperature=1.0):
    """mgx_linear_logprob in fp64 -> dict(logp, lse, hit, xt, x [M, V], S [M, V]: sum_k |a_k w_vk| + |bias_v|, scaled as x is,
    gap [M]: the distance of the two largest x of a row)"""
    c, S = T.proj(a, w, bias)
    inv = inv_temperature(temperature)
    x, S = np.asarray(c) * inv, np.asarray(S) * inv
    ok = np.ones(x.shape, bool)
    lse = lse_rows(x, ok)
    logp, hit = _finish(x, ok, x, target, lse)
    t = np.clip(np.asarray(target).astype(np.int64), 0, x.shape[1] - 1)
    r = np.arange(x.shape[0])
    top = np.sort(x, axis=1)
    gap = top[:, -1] - top[:, -2] if x.shape[1] > 1 else np.full(x.shape[0], np.inf)
    return dict(logp=logp, lse=lse, hit=hit, xt=x[r, t], x=x, S=S, St=S[r, t], gap=gap)


def linear_floor(ref):
    """per row: EPS32 (S_t + max_v S_v) + |fp32 twin lse reversed - ref lse| + ulp32(max(|x_t|, |lse|))"""
    x32 = ref["x"].astype(np.float32)
    tw = lse_rows(x32, np.ones(x32.shape, bool), np.float32, True).astype(np.float64)
    ulp = np.asarray(T.ulp32(np.maximum(np.abs(ref["xt"]), np.abs(ref["lse"]))))
    return T.EPS32 * (ref["St"] + ref["S"].max(1)) + np.abs(tw - ref["lse"]) + ulp


def score_reduce(logp, hit):
    """mgx_score_reduce: (sum fp64 [B] as a sorted (by magnitude) fp64 sum, count, hits, sum |logp| over the counted entries)"""
    logp, hit = np.asarray(logp, dtype=np.float64), np.asarray(hit)
    sums, mags = [], []
    for b in range(logp.shape[0]):
        v = logp[b][hit[b] >= 0]
        with np.errstate(invalid="ignore"):
            sums.append(np.sum(v[np.argsort(np.abs(v))]) if len(v) else 0.0)
            mags.append(np.abs(v).sum() if len(v) else 0.0)
    return np.array(sums), (hit >= 0).sum(1), (hit == 1).sum(1), np.array(mags)


def log_softmax_torch(logits, temperature, ok):
    """torch.log_softmax in fp64 over the allowed ids: what the definitions above must agree with"""
    x = torch.as_tensor(np.asarray(logits, dtype=np.float64)) * inv_temperature(temperature)
    x = torch.where(torch.as_tensor(ok), x, torch.full((), NEG, dtype=torch.float64))
    return torch.log_softmax(x, -1).numpy()
