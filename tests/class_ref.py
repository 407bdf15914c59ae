"""NumPy fp64 restatement of mgx_class_logits (include/mgx.h, ABI 33): per-class temperature, top-k and top-p as two-stage
sampling.  ``warp`` gives ln p' per row, unrounded, with the margins of its own filter decisions -- how far every cut is from
falling elsewhere, so a test can keep to inputs on which f32 and fp64 must agree about the kept set; ``expected_probs`` gives what
the decode files from a plain softmax.  Imported by basename, like repeat_ref / budget_ref."""
import numpy as np
import torch

NEG_INF = float("-inf")


def _lse(a):
    m = a.max()
    return m + np.log(np.exp(a - m).sum())


def allowed_bits(table, prev, V):
    """row ``prev`` (clamped to 0 .. V-1) of the grammar table uint32 [V, ceil(V/32)] as booleans [V]"""
    row = np.asarray(table).view(np.uint32)[min(max(int(prev), 0), V - 1)]
    v = np.arange(V)
    return ((row[v >> 5] >> (v & 31).astype(np.uint32)) & 1).astype(bool)


def warp_row(x, cls, inv_temp, top_k, top_p, temperature, allowed=None):
    """one row.  x float64 [V] (the bf16 logits' values), cls int [V]; allowed: booleans [V] or None.  -> (ln p' float64 [V] with
    -inf at the ids that are not kept, or None where the row is left as it is; margins: one per filtered class)"""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    cls = np.asarray(cls)[:V]
    fin = x > NEG_INF
    A = fin & allowed if allowed is not None else fin
    if allowed is not None and not A.any():
        A = fin                                               # the sampler's fallback: a grammar row that leaves nothing is ignored
    if not A.any():
        return None, []
    out = np.full(V, NEG_INF)
    lse_all = _lse(x[A] / temperature)
    margins = []
    for c in np.unique(cls):
        ids = np.flatnonzero(A & (cls == c))
        if ids.size == 0:
            continue
        ln_pc = _lse(x[ids] / temperature) - lse_all
        z = x[ids] * float(inv_temp[c])
        q = np.exp(z - _lse(z))
        k, p = int(top_k[c]), float(top_p[c])
        tau, margin = 0.0, np.inf
        if 0 < k < ids.size:
            tau = np.sort(q)[::-1][k - 1]                     # the largest tau with #{q >= tau} >= k
        base = q[q >= tau].sum()
        if p < 1:
            need = p * base
            for t in np.sort(np.unique(q[q >= tau]))[::-1]:   # the largest tau with mass{q >= tau} >= need
                if q[q >= t].sum() >= need:
                    tau = t
                    break
            margin = min(margin, (q[q >= tau].sum() - need) / need, (need - q[q > tau].sum()) / need)
        keep = q >= tau
        if not keep.all():
            margin = min(margin, (q[keep].min() - q[~keep].max()) / q[keep].min())
        if (0 < k < ids.size) or p < 1:
            margins.append(margin)
        out[ids[keep]] = ln_pc + z[keep] - _lse(z[keep])
    return out, margins


def warp(x, V, cls, inv_temp, top_k, top_p, temperature, tok=None, table=None):
    """x float64 [B, >= V].  -> (ln p' float64 [B, V]; touched: booleans [B], False where a row is left bit for bit (its ln p' row
    is NaN); margins: a flat list over the filtered (row, class) pairs)"""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    out, touched, margins = np.full((B, V), np.nan), np.zeros(B, dtype=bool), []
    for b in range(B):
        allowed = None if table is None else allowed_bits(table, tok[b], V)
        r, m = warp_row(x[b, :V], cls, inv_temp, top_k, top_p, temperature, allowed)
        if r is not None:
            out[b], touched[b] = r, True
        margins += m
    return out, touched, margins


def bf16_values(a):
    """float64 values rounded to bf16 (nearest-even), as float64"""
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).to(torch.float32).to(torch.bfloat16).to(torch.float64).numpy()


def filed(lnp):
    """what the sampler at temperature 1 files for a row of ln p': softmax(bf16(ln p')), float64"""
    y = bf16_values(lnp)
    e = np.exp(y - y[np.isfinite(y)].max())
    return e / e.sum()


def expected_probs(p_plain, cls, inv_temp, top_k, top_p, temperature, allowed=None, with_lnp=False):
    """p' from a plain softmax p (float64 [V], at the call's temperature, 0 at masked ids): P_c = sum_c p, inside a class
    q ~ p^(temperature * inv_temp[c]), the filters, then softmax(bf16(ln p')).  -> float64 [V] (with_lnp: and ln p', unrounded)"""
    p = np.asarray(p_plain, dtype=np.float64)
    with np.errstate(divide="ignore"):
        x = temperature * np.log(p)                           # logits that give p at the call's temperature
    lnp, _ = warp_row(x, cls, inv_temp, top_k, top_p, temperature, allowed)
    return (filed(lnp), lnp) if with_lnp else filed(lnp)


def prob_bound(lnp, f32_term=3e-4, halves=2, centre=None):
    """the kernel's logit bound turned into probabilities.  The kernel's value is within half a bf16 spacing + f32_term of ln p',
    and bf16(ln p') within half a spacing, so a filed logit differs from bf16(ln p') by at most
    e_v = halves |ln p'_v| 2^-8 + f32_term with halves = 2 -- and from ln p' itself (``centre`` = exp(ln p'), the unquantised
    distribution) with halves = 1.  The softmax's ratio to the centre (default ``filed(lnp)``) then lies in
    [exp(-e_v) / sum_u p_u exp(e_u), exp(e_v + sum_u p_u e_u)].  -> float64 [V], 0 where p' is 0"""
    lnp = np.asarray(lnp, dtype=np.float64)
    p, fin = filed(lnp) if centre is None else np.asarray(centre, dtype=np.float64), np.isfinite(lnp)
    e = np.where(fin, np.abs(np.where(fin, lnp, 0.0)) * halves * 2.0 ** -8 + f32_term, 0.0)
    up = np.exp(e + (p * e).sum()) - 1
    down = 1 - np.exp(-e) / (p * np.exp(e)).sum()
    return p * np.maximum(up, down)
