"""fp64 / numpy references of the three beam-search contracts of include/mgx.h (ABI 22), written from the header: a plain
helper module of the beam tests, CPU only.  Rows r = b * K + k: beam k of prompt b."""
import numpy as np

from oracle import decode_ref as D

NEG = -np.inf


def gumbel(seed, t, B, K, V, dtype=np.float64):
    """g [B, K, V] = -log(-log(min(u, 1 - 2^-24))), u the sampler's uniform of (seed, t_b, (b K + k) 1024 + v).  ``dtype``
    np.float32: the same formula in fp32 from the same u (exact in fp32) -- not a reference, a second evaluation whose distance
    from the fp64 one is what fp32 does to the formula"""
    rows = (np.arange(B * K)[:, None] * 1024 + np.arange(V)[None, :]).reshape(B, K, V)
    u = D.u01(seed, np.broadcast_to(np.asarray(t).reshape(B, 1, 1), rows.shape), rows).astype(dtype)
    u = np.minimum(u, dtype(1.0) - dtype(2.0 ** -24))
    return -np.log(-np.log(u))


def select(logits, temperature, score, tok, t, allow_table=None, stochastic=False, seed=0):
    """mgx_beam_select for logits [B*K, V] (the V real columns; the exact values the kernel reads), score [B, K], tok [B*K],
    t [B] (the prompts' positions).  Returns a dict: cand, key fp64 [B, K, V]; tok, parent int [B, K] and score fp64 [B, K] as
    the contract writes them; flat [B] lists of the chosen flat indices k V + v in slot order (fewer than K where fewer finite
    candidates exist); gap [B]: the smallest key distance between a chosen and a finite not-chosen candidate (inf where there
    is none), not counting STRUCTURAL ties of the deterministic order: two ids of one beam with the same logit have the same
    key in any arithmetic, so the index decides between them exactly"""
    score = np.asarray(score, dtype=np.float64)
    B, K = score.shape
    x = np.asarray(logits, dtype=np.float64).reshape(B * K, -1) * (1.0 / float(temperature))
    V = x.shape[1]
    raw = np.asarray(logits, dtype=np.float64).reshape(B, K * V)
    if allow_table is not None:
        xm = np.where(D.allowed_mask(allow_table, tok, V), x, NEG)
        ignored = ~np.isfinite(xm.max(-1))                   # a grammar row that leaves no finite logit is ignored
        x = np.where(ignored[:, None], x, xm)
    mx = x.max(-1, keepdims=True)
    logp = x - (mx + np.log(np.exp(x - mx).sum(-1, keepdims=True)))
    cand = (score.reshape(B * K, 1) + logp).reshape(B, K, V)
    cand[~np.isfinite(score)] = NEG                          # dead beams
    key = cand + gumbel(seed, t, B, K, V) if stochastic else cand.copy()
    key[cand == NEG] = NEG
    out = dict(cand=cand, key=key, tok=np.zeros((B, K), np.int64), parent=np.zeros((B, K), np.int64),
               score=np.full((B, K), NEG), flat=[], gap=np.full(B, np.inf))
    tok_in = np.asarray(tok).reshape(B, K)
    for b in range(B):
        kf = key[b].reshape(-1)
        order = np.lexsort((np.arange(K * V), -kf))          # descending key, equal keys by the smaller flat index
        order = order[np.isfinite(cand[b].reshape(-1)[order])]
        chosen = order[:K]
        out["flat"].append(chosen.tolist())
        if len(order) > K:
            rest = order[K:]
            diff = kf[chosen][:, None] - kf[rest][None, :]
            if not stochastic:                               # a structural tie is decided exactly, by the index
                same = (chosen[:, None] // V == rest[None, :] // V) & (raw[b][chosen][:, None] == raw[b][rest][None, :])
                diff = np.where(same, np.inf, diff)
            out["gap"][b] = diff.min()
        for j in range(K):
            f = chosen[j] if j < len(chosen) else None
            if f is not None:
                out["tok"][b, j], out["parent"][b, j], out["score"][b, j] = f % V, f // V, cand[b].reshape(-1)[f]
            elif j > 0:                                      # fewer than K finite candidates: a dead copy of slot 0
                out["tok"][b, j], out["parent"][b, j] = out["tok"][b, 0], out["parent"][b, 0]
            else:                                            # none at all
                out["tok"][b, j], out["parent"][b, j] = tok_in[b, 0], 0
    return out


def reorder(dst, src, parent, n, K):
    """mgx_kv_beam_reorder on arrays [R, h, Lmax, ...]: returns dst with rows < n_r of every (r, h) taken from the parent"""
    res = np.array(dst, copy=True)
    for r in range(res.shape[0]):
        res[r, :, :n[r]] = src[r // K * K + parent[r], :, :n[r]]
    return res


def backtrack(hist_tok, hist_parent, c0, steps, K, out):
    """mgx_beam_backtrack: returns ``out`` with columns c0_r .. c0_r + steps - 1 of every row walked back through the parents"""
    res = np.array(out, copy=True)
    for r in range(res.shape[0]):
        first, cur = r // K * K, r % K
        for s in range(steps - 1, -1, -1):
            res[r, c0[r] + s] = hist_tok[first + cur, c0[r] + s]
            cur = hist_parent[first + cur, c0[r] + s]
    return res


def search(logits_of, K, V, steps, temperature=1.0, allow_table=None, stochastic=False, seed=0, first_tok=0):
    """a whole search of ONE prompt through select and backtrack, as the driver runs it: ``logits_of(prefix)`` gives the V
    logits after the tuple of generated tokens ``prefix``.  Returns (sequences int [K, steps], scores fp64 [K])"""
    score = np.full((1, K), NEG)
    score[0, 0] = 0.0                                        # one live beam
    tok = np.full(K, first_tok, np.int64)
    ht, hp = np.zeros((K, steps), np.int64), np.zeros((K, steps), np.int64)
    for s in range(steps):
        prefixes = backtrack(ht, hp, np.zeros(K, int), s, K, np.zeros((K, steps), np.int64))[:, :s]
        logits = np.stack([logits_of(tuple(int(v) for v in p)) for p in prefixes])
        sel = select(logits, temperature, score, tok, np.array([s]), allow_table, stochastic, seed)
        score, tok = sel["score"], sel["tok"][0]
        ht[:, s], hp[:, s] = sel["tok"][0], sel["parent"][0]
    return backtrack(ht, hp, np.zeros(K, int), steps, K, np.zeros((K, steps), np.int64)), score[0]
