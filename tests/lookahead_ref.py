"""Plain-Python reference of the draft and the accept rule of draft-and-verify decode (include/mgx.h, ABI 32), written from the
header's definitions -- loops over lists, nothing shared with the kernels.  Imported by basename, like beam_ref / repeat_ref."""


def draft_row(row, s, tok, T, pad, ngram=3, guide=None):
    """draft[b, 0..T-1] of one row: ``row`` its columns of out_tokens, ``s`` the column of the step's input token ``tok``"""
    out = [tok]
    if guide is not None:
        return out + [guide[s + i] if 0 <= s and s + i < len(guide) else pad for i in range(1, T)]
    if not 1 <= s < len(row):
        return out + [pad] * (T - 1)
    for n in range(ngram, 0, -1):
        if s - n + 1 < 0:
            continue
        js = [j for j in range(n - 1, s) if row[j - n + 1:j + 1] == row[s - n + 1:s + 1]]
        if js:
            x = list(row[:s + 1])
            period = s - js[-1]
            for c in range(s + 1, s + T):
                x.append(x[c - period])                   # the match, extended periodically where it runs into the present
            return out + x[s + 1:s + T]
    return out + [pad] * (T - 1)


def pos_rows(t, T, Lmax):
    return [max(0, min(t + i, Lmax - 1)) for i in range(T)]


def accept_row(draft, ys, s, limit):
    """-> (n, a): ``ys`` the T draws; a = the guesses that were the tokens drawn, n = the tokens the row keeps (<= 0: finished)"""
    a = 0
    while a < len(draft) - 1 and draft[a + 1] == ys[a]:
        a += 1
    return min(a + 1, limit - s), a


def accept(out, tok, pos, draft, ys, limit, done, stats, base=None):
    """the accept rule on lists, in place: out [B][out_ld], tok / pos / limit / done [B], draft / ys [B][T], stats [B][2]"""
    for b in range(len(tok)):
        s = pos[b] + (base[b] if base else 0)
        n, _ = accept_row(draft[b], ys[b], s, limit[b])
        if n <= 0:
            done[b] = 1
            continue
        for i in range(n):
            out[b][s + 1 + i] = ys[b][i]
        tok[b] = ys[b][n - 1]
        pos[b] += n
        stats[b][0] += 1
        stats[b][1] += n
