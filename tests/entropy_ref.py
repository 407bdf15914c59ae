"""NumPy fp64 restatement of mgx_entropy_mask and mgx_entropy_account (include/mgx.h, ABI 34): min-p, locally typical sampling and
the Mirostat v2 cut as three sequential stages of one pure mask, and the surprise / threshold update after the draw.  ``mask_row``
gives the kept set with the margins of its own decisions -- how far every cut is from falling elsewhere, so a test can keep to
inputs on which f32 and fp64 must agree about the kept set.  Imported by basename, like class_ref / budget_ref."""
import numpy as np

from class_ref import allowed_bits, bf16_values  # noqa: F401 (re-exported: the tests take them from here)

NEG_INF = float("-inf")
LN2 = np.log(2.0)


def _lse(a):
    m = a.max()
    return m + np.log(np.exp(a - m).sum())


def live_set(x, allowed=None):
    """A: the finite ids the grammar allows; a grammar row that leaves nothing is ignored"""
    fin = np.asarray(x, dtype=np.float64) > NEG_INF
    A = fin & allowed if allowed is not None else fin
    return fin if allowed is not None and not A.any() else A


def mask_row(x, temperature, min_p=0.0, typical_p=1.0, mu=None, allowed=None):
    """one row.  x float64 [V] (the bf16 logits' values); allowed: booleans [V] or None; mu: the row's threshold in bits or None.
    -> (kept: booleans [V], or None where the row is left as it is; lse; margins: a dict with the entries of the stages that ran --
    "mirostat": min |s_v - mu| in bits, "min_p": min |z_v - zmax - ln min_p| in nats, "typical_over": (mass kept - typical_p) /
    typical_p, "typical_under": (typical_p - mass strictly inside) / typical_p, "typical_gap": the gap in d between the last kept
    and the first dropped value)"""
    x = np.asarray(x, dtype=np.float64)
    A = live_set(x, allowed)
    if not A.any():
        return None, 0.0, {}
    with np.errstate(invalid="ignore"):
        z = x * (1.0 / temperature)
    lse = _lse(z[A])
    margins = {}
    keep = A.copy()
    if mu is not None:
        s = np.where(A, (lse - np.where(A, z, 0.0)) / LN2, np.inf)
        margins["mirostat"] = np.abs(s[A] - mu).min()
        s1 = A & (s <= mu)
        keep = s1 if s1.any() else A & (z == z[A].max())
    if min_p > 0:
        rel = np.where(keep, z, 0.0) - z[keep].max() - np.log(min_p)
        margins["min_p"] = np.abs(rel[keep]).min()
        keep = keep & (rel >= 0)
    if typical_p < 1:
        ids = np.flatnonzero(keep)
        lnq = z[ids] - _lse(z[ids])
        q = np.exp(lnq)
        H = -(q * lnq).sum()
        d = np.abs(-lnq - H)
        for delta in np.unique(d):                            # ascending: the smallest delta with mass{d <= delta} >= typical_p
            if q[d <= delta].sum() >= typical_p:
                break
        inside = d <= delta
        margins["typical_over"] = (q[inside].sum() - typical_p) / typical_p
        margins["typical_under"] = (typical_p - q[d < delta].sum()) / typical_p
        margins["typical_gap"] = d[~inside].min() - delta if (~inside).any() else np.inf
        keep = np.zeros_like(keep)
        keep[ids[inside]] = True
    return keep, lse, margins


def mask(x, V, temperature, min_p=0.0, typical_p=1.0, mu=None, tok=None, table=None):
    """x float64 [B, >= V]; mu: float [B] or None.  -> (kept booleans [B, V]; touched booleans [B], False where a row is left bit
    for bit; lse float64 [B], 0 there; margins: one dict per row)"""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    kept, touched, lse, margins = np.zeros((B, V), dtype=bool), np.zeros(B, dtype=bool), np.zeros(B), []
    for b in range(B):
        allowed = None if table is None else allowed_bits(table, tok[b], V)
        k, l, m = mask_row(x[b, :V], temperature, min_p, typical_p, None if mu is None else float(mu[b]), allowed)
        if k is not None:
            kept[b], touched[b], lse[b] = k, True, l
        margins.append(m)
    return kept, touched, lse, margins


def smallest(margins):
    """the smallest margin of a dict or of a list of dicts (inf where no stage ran)"""
    ms = [margins] if isinstance(margins, dict) else margins
    return min([v for m in ms for v in m.values()], default=np.inf)


def kept_from_probs(p, min_p=0.0, typical_p=1.0, mu=None):
    """the kept set of a row whose distribution, at the sampler's temperature and under its grammar, is p (float64 [V], 0 at masked
    ids): ln p are logits that give it at temperature 1.  -> (kept, margins)"""
    with np.errstate(divide="ignore"):
        x = np.log(np.asarray(p, dtype=np.float64))
    kept, _, margins = mask_row(x, 1.0, min_p, typical_p, mu)
    return kept, margins


def surprise(x_tok, lse, temperature):
    """the surprise in bits of a token whose logit is x_tok under a row of log-sum-exp lse"""
    return (lse - x_tok * (1.0 / temperature)) / LN2


def account(next_tok, x, V, temperature, lse, mu, tau, eta):
    """after the draw.  x float64 [B, >= V], lse / mu float64 [B] (mu may be None).  -> (s float64 [B], NaN where nothing is
    accounted: a token outside 0 .. V-1 or a logit that is not finite; mu' float64 [B] or None)"""
    B = len(next_tok)
    s = np.full(B, np.nan)
    mu2 = None if mu is None else np.asarray(mu, dtype=np.float64).copy()
    for b, t in enumerate(next_tok):
        if not 0 <= t < V or not np.isfinite(x[b, t]):
            continue
        s[b] = surprise(x[b, t], lse[b], temperature)
        if mu2 is not None:
            mu2[b] = mu2[b] - eta * (s[b] - tau)
    return s, mu2
