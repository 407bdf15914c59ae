"""numpy reference of mgx_crop_augment (include/mgx.h, ABI 29), written from the header as a plain token loop with a running
time -- no scans, no tiles.  Everything is integer, so every comparison against it is exact.  Imported by basename, like
budget_ref / notes_ref."""
import numpy as np


def stretch_row(src, q, ts0, n_ts, limit=None):
    """the ids one row emits for the source tokens ``src`` at q per-mille (a q outside 500 .. 2000 counts as 1000), as a list;
    ``limit``: stop once that many are out.  Also returns the time units emitted, S_last"""
    q = int(q) if 500 <= int(q) <= 2000 else 1000
    out, T, S_prev = [], 0, 0
    for v in (int(t) for t in src):
        if limit is not None and len(out) >= limit:
            break
        if ts0 <= v < ts0 + n_ts:
            T += v - ts0 + 1
            S = (T * q + 500) // 1000
            delta, S_prev = S - S_prev, S
            out += [ts0 + n_ts - 1] * (delta // n_ts)
            if delta % n_ts > 0:
                out.append(ts0 + delta % n_ts - 1)
        else:
            out.append(v)
    return out, S_prev


def crop_augment(corpus, start, avail, n, pad_token, *, perm=None, shift_row=None, stretch_q=None, ts0=0, n_ts=0, with_y=True):
    """-> (x, y, n_out) as [B, n - 1], [B, n - 1], [B] (``with_y``) or ([B, n], None, [B]): row-major whatever strides the
    kernel is asked to write with.  corpus: 1-D array of ids; perm int [S, V] or None"""
    corpus = np.asarray(corpus).astype(np.int64).reshape(-1)
    B, N = len(start), len(corpus)
    out = np.full((B, n), int(pad_token), dtype=np.int64)
    n_out = np.zeros(B, dtype=np.int64)
    for b in range(B):
        st, av = int(start[b]), int(avail[b])
        if st < 0 or av < 0 or st >= N:
            n_src = 0
        else:
            n_src = min(2 * n if stretch_q is not None else n, av, N - st)
        src = corpus[st:st + n_src] if n_src > 0 else corpus[:0]
        if stretch_q is not None:
            ids, _ = stretch_row(src, stretch_q[b], ts0, n_ts, limit=n)
        else:
            ids = [int(v) for v in src]
        ids = ids[:n]
        if perm is not None:
            S, V = perm.shape
            s = int(shift_row[b])
            if 0 <= s < S:
                ids = [int(perm[s, v]) if 0 <= v < V else v for v in ids]
        out[b, :len(ids)] = ids
        n_out[b] = len(ids)
    if with_y:
        return out[:, :-1].copy(), out[:, 1:].copy(), n_out
    return out, None, n_out
