"""mgx_repeat_penalty (ABI 31) restated in numpy from the text of include/mgx.h: the counts over the window, the ids an n-gram rule
bans, the amounts, and the one f32 subtraction with one nearest-even rounding to bf16, on uint16 bit patterns.  Imported by
basename, like budget_ref / notes_ref.  Plain loops: the rows of the tests are short."""
import numpy as np


def step_col(pos, base, per_row, b):
    """c = base + t of row b ("Step positions")"""
    i = b if per_row else 0
    return int(pos[i]) + (0 if base is None else int(base[i]))


def counts(row, c, V, window):
    """cnt[v], 0 <= v < V: the columns j of ``row``, max(0, c - window + 1) <= j <= c, that hold v; other ids count for nothing"""
    cnt = np.zeros(V, dtype=np.int64)
    for j in range(max(0, c - window + 1), c + 1):
        if 0 <= row[j] < V:
            cnt[row[j]] += 1
    return cnt


def banned(row, c, V, n, span):
    """the set of ids the no-repeat-n rule bans at column c: the followers, inside 0..V-1, of every earlier occurrence of the
    context row[c-k+1 .. c], k = n - 1, that begins at or after lo = max(0, c - span + 1) (span 0: column 0)"""
    k = n - 1
    lo = max(0, c - span + 1) if span else 0
    out = set()
    if c - k + 1 < lo:
        return out
    ctx = [int(v) for v in row[c - k + 1:c + 1]]
    for e in range(lo + k - 1, c):
        if [int(v) for v in row[e - k + 1:e + 1]] == ctx and 0 <= row[e + 1] < V:
            out.add(int(row[e + 1]))
    return out


def bf16_bits_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_bits(x):
    """nearest-even; a NaN stays a NaN (quiet bit set)"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    return np.where(np.isnan(x), ((u >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), r)


def amounts(row, c, V, subject, pen, window, ngram, span, ban):
    """{v: a[v]} for the ids of a row that have an amount"""
    out = {}
    if window > 0:
        cnt = counts(row, c, V, window)
        for v in range(V):
            if cnt[v] > 0 and subject[v] != 0:
                out[v] = np.float32(pen[cnt[v]])
    if ngram >= 2:
        for v in banned(row, c, V, ngram, span):
            out[v] = np.float32(ban)                     # ban, not the sum
    return out


def penalise(bits, V, out, pos, base, per_row, subject, pen, window, ngram, span, ban):
    """the logits' bits uint16 [B, ld] after the call; nothing else changes"""
    res = np.array(bits, dtype=np.uint16, copy=True)
    out = np.asarray(out)
    for b in range(res.shape[0]):
        c = step_col(pos, base, per_row, b)
        if c < 0 or c >= out.shape[1]:
            continue
        for v, a in amounts(out[b], c, V, subject, pen, window, ngram, span, ban).items():
            x = bf16_bits_to_f32(res[b, v:v + 1])
            with np.errstate(invalid="ignore"):
                res[b, v] = f32_to_bf16_bits((x - np.float32(a)).astype(np.float32))[0]
    return res


def first_bite(rows, starts, steps, V, subject, pen, window, ngram, span, ban, finite=None):
    """for every row: the first step s (0-based; the step whose input token sits at column starts[b] - 1 + s) at which some id
    gets a non-zero amount -- an id with a finite logit, where ``finite(b, s)`` gives the boolean [V] of that step; None if no
    step of the row does"""
    res = []
    for b, row in enumerate(rows):
        hit = None
        for s in range(steps):
            am = amounts(row, starts[b] - 1 + s, V, subject, pen, window, ngram, span, ban)
            if any(a != 0 and (finite is None or finite(b, s)[v]) for v, a in am.items()):
                hit = s
                break
        res.append(hit)
    return res


def repeats(seq, n, span=0):
    """does some n-gram end twice inside one span: is there a column c whose n-gram seq[c-n+1 .. c] also ends at an earlier
    column e + 1 with the occurrence beginning at or after max(0, c - span) (span 0: anywhere before)?  This is what the
    no-repeat-n rule with this span forbids the step at column c - 1 to produce"""
    seq = [int(v) for v in seq]
    for c in range(n - 1, len(seq)):
        lo = max(0, c - span) if span else 0
        for e in range(lo + n - 1, c):
            if seq[e - n + 1:e + 1] == seq[c - n + 1:c + 1]:
                return True
    return False
