"""mgx_repeat_penalty (ABI 31) against the numpy restatement of its header contract (tests/repeat_ref.py).  Per id the kernel does at
most one f32 subtraction and one rounding to bf16, so every check is exact: the logits' BITS after the call -- the columns at and
beyond V and the guard bands included -- and every input, which the call only reads.  The cases are the edges at which this
kernel can go wrong: the first columns of a row, the window's two ends, an occurrence at the span's edge, the longest n-gram,
ids outside the vocabulary in the history.  The chained test plays six steps of a scripted token stream, the host doing the
sampler's write and its advance between the calls, once with a re-anchor of the positions in the middle."""
import numpy as np
import pytest
import torch

import kernel_checks as KC
import repeat_ref
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)

pytestmark = pytest.mark.gpu

OUT_LD = 48
BAN = 1e4


def banded(a, dtype=torch.int32):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return KC.Banded(t.to(dtype), KC.BAND, KC.PATTERN)


def logits_for(rng, B, V, ld):
    """bf16 [B, ld]: N(0, 4) with ~10 % -inf among the logits and NaN in the columns >= V; -> (tensor, its bits uint16)"""
    x = torch.from_numpy(rng.normal(size=(B, ld)) * 4.0).to(torch.bfloat16)
    x[torch.from_numpy(rng.random((B, ld)) < 0.1)] = float("-inf")
    x[:, V:] = float("nan")
    return x, x.view(torch.int16).numpy().view(np.uint16).copy()


def pen_for(window, rng=None):
    """pen [window + 1]: distinct values, so an entry read from the wrong place shows; pen[0] would show too (it is never read)"""
    p = 0.25 + 0.125 * np.arange(window + 1, dtype=np.float64) + (0 if rng is None else rng.random(window + 1) * 0.01)
    p[0] = 777.0
    return p.astype(np.float32)


def run(V, hist, pos, base, per_row, subject, window, ngram, span, case, seed=0, ban=BAN, pen=None, B=None):
    """one call on fresh logits; exact against the reference; bands and inputs intact.  -> (bits before, bits wanted)"""
    hist = np.asarray(hist, dtype=np.int32)
    B = hist.shape[0] if B is None else B
    ld = (V + 63) // 64 * 64
    rng = np.random.default_rng(seed)
    x, bits = logits_for(rng, B, V, ld)
    if window:
        pen = pen_for(window) if pen is None else pen
        subject = np.asarray(subject, dtype=np.int32)
    else:
        pen = subject = None
    pos, base = np.asarray(pos, dtype=np.int32), None if base is None else np.asarray(base, dtype=np.int32)
    lg, h, p = banded(x, torch.bfloat16), banded(hist), banded(pos)
    bs = None if base is None else banded(base)
    sj = None if subject is None else banded(subject)
    pn = None if pen is None else banded(pen, torch.float32)
    KC.ops().repeat_penalty(lg.t, V, h.t, p.t, None if sj is None else sj.t, None if pn is None else pn.t, window, ngram, span, ban,
                            ragged=bool(per_row), base=None if bs is None else bs.t)
    torch.cuda.synchronize()
    want = repeat_ref.penalise(bits, V, hist, pos, base, per_row, subject, pen, window, ngram, span, ban)
    KC.check_equal("repeat", KC.bits16(lg.t).to(torch.int32), torch.from_numpy(want.view(np.int16).astype(np.int32)), case)
    assert (want[:, V:] == bits[:, V:]).all(), case                          # the reference itself: columns >= V stay
    for b_ in (lg, h, p, bs, sj, pn):
        assert b_ is None or b_.bands_intact(), case
    for b_, a in ((h, hist), (p, pos), (bs, base), (sj, subject)):           # the inputs are read only
        assert b_ is None or (b_.t.cpu().numpy() == a).all(), case
    assert pn is None or (pn.t.cpu().numpy() == pen).all(), case
    return bits, want


CONFIGS = [(8, 3, 0), (8, 0, 0), (0, 3, 0), (5, 2, 6), (47, 4, 12), (48, 2, 0)]      # (window, ngram, span)


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("per_row", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 337, 1024])
def test_random_histories(V, B, per_row, with_base):
    """histories over a 4-id alphabet -- two ids of the vocabulary, one beyond it, one negative -- at every edge column"""
    alphabet = np.array([0, V - 1, V + 3, -5], dtype=np.int32)
    changed = 0
    for ci, (window, n, span) in enumerate(CONFIGS):
        cols = sorted({0, 1, max(n - 2, 0), max(n - 1, 0), max(window - 1, 0), min(window, OUT_LD - 1), OUT_LD - 1, OUT_LD})
        for k, c in enumerate(cols):
            seed = ((V * 4 + B) * 4 + per_row * 2 + with_base) * 1000 + ci * 50 + k
            rng = np.random.default_rng(seed)
            hist = alphabet[rng.choice(4, (B, OUT_LD), p=[0.4, 0.4, 0.1, 0.1])]
            subject = (rng.random(V) < 0.7).astype(np.int32)
            subject[0] = 1
            rows = B if per_row else 1
            cs = np.array([cols[(k + r) % len(cols)] for r in range(rows)])   # ragged rows sit at different edges
            base = rng.integers(0, 5, rows) if with_base else None
            pos = cs - (base if with_base else 0)                             # a negative position with a base is still column c
            case = f"V={V} B={B} per_row={per_row} base={with_base} window={window} n={n} span={span} c={cs.tolist()}"
            bits, want = run(V, hist, pos, base, per_row, subject, window, n, span, case, seed)
            for b in range(B):
                if cs[b if per_row else 0] == OUT_LD:
                    assert (want[b] == bits[b]).all(), case                   # the reference itself: a row outside is untouched
            changed += int((want != bits).sum())
    assert changed > 0                                                        # the parametrisation penalises something


def _filler(B=1, out_ld=OUT_LD):
    return np.full((B, out_ld), -1, dtype=np.int32)


def changed_ids(bits, want, V):
    return [sorted(np.flatnonzero(bits[b, :V] != want[b, :V]).tolist()) for b in range(bits.shape[0])]


def finite_logits(V, B=1, seed=0):
    """run() draws the logits from ``seed``: the ids of every row that are not -inf there"""
    _, bits = logits_for(np.random.default_rng(seed), B, V, (V + 63) // 64 * 64)
    return [set(np.flatnonzero(bits[b, :V] != 0xFF80).tolist()) for b in range(B)]


def pick(V, k, seed=0, B=1):
    """k ids whose logit is finite in every row under ``seed`` (so a missing change is a finding, not a -inf)"""
    ids = sorted(set.intersection(*finite_logits(V, B, seed)))
    assert len(ids) >= k
    return ids[:k]


def test_the_two_ends_of_the_window():
    V, window, c = 65, 8, 20
    a, b = pick(V, 2)
    hist = _filler()
    hist[0, c - window], hist[0, c - window + 1] = a, b                       # a: just outside, not counted; b: the oldest counted
    bits, want = run(V, hist, [c], None, 0, np.ones(V), window, 0, 0, "window ends")
    assert changed_ids(bits, want, V) == [[b]]
    hist = _filler()
    hist[0, c], hist[0, c + 1] = a, b                                         # the newest counted column is c itself; c + 1 is not read
    bits, want = run(V, hist, [c], None, 0, np.ones(V), window, 0, 0, "window newest")
    assert changed_ids(bits, want, V) == [[a]]
    hist = _filler()
    hist[0, 0] = a                                                            # c < window: the window is cut at column 0
    bits, want = run(V, hist, [3], None, 0, np.ones(V), window, 0, 0, "window cut at 0")
    assert changed_ids(bits, want, V) == [[a]]


@pytest.mark.parametrize("window", [1, 8, 48])
def test_a_row_of_one_id_reads_the_last_entry_of_pen(window):
    V = 65
    a, = pick(V, 1)
    hist = np.full((1, OUT_LD), a, dtype=np.int32)
    pen = pen_for(window)
    bits, want = run(V, hist, [OUT_LD - 1], None, 0, np.ones(V), window, 0, 0, f"one id window={window}", pen=pen)
    assert changed_ids(bits, want, V) == [[a]]
    x = repeat_ref.bf16_bits_to_f32(bits[0, a:a + 1])
    assert want[0, a] == repeat_ref.f32_to_bf16_bits(x - pen[window])[0]       # the reference itself: cnt == window


def test_ngram_edges():
    V = 65
    a, b, f, g = pick(V, 4)
    # the follower at column c: "a a a" with n = 2 -- the occurrence e = c - 1 is followed by column c itself
    hist = _filler()
    hist[0, 10:13] = a
    bits, want = run(V, hist, [12], None, 0, None, 0, 2, 0, "follower at c")
    assert changed_ids(bits, want, V) == [[a]]
    # an occurrence cut by the span: the context "a b" at 30..31, its earlier occurrence at 20..21 followed by f
    hist = _filler()
    hist[0, 20:23] = [a, b, f]
    hist[0, 30:32] = [a, b]
    bits, want = run(V, hist, [31], None, 0, None, 0, 3, 11, "span cuts")         # lo = 21: the occurrence begins before it
    assert changed_ids(bits, want, V) == [[]]
    bits, want = run(V, hist, [31], None, 0, None, 0, 3, 12, "span holds")        # lo = 20
    assert changed_ids(bits, want, V) == [[f]]
    bits, want = run(V, hist, [31], None, 0, None, 0, 3, 0, "whole row")
    assert changed_ids(bits, want, V) == [[f]]
    # n = 2 with two followers; a follower id >= V bans nothing; the comparison is on raw values (V + 3 is a context like any other)
    hist = _filler()
    hist[0, :7] = [V + 3, f, a, V + 3, g, V + 3, V + 9]
    hist[0, 7] = V + 3
    bits, want = run(V, hist, [7], None, 0, None, 0, 2, 0, "raw context")
    assert changed_ids(bits, want, V) == [sorted([f, g])]                         # and V + 9, a follower too, is out of range
    # c = n - 2: a context exists, no candidate end; c = n - 1: the first candidate
    hist = np.full((1, OUT_LD), a, dtype=np.int32)
    for n in (2, 3, 5):
        bits, want = run(V, hist, [n - 2], None, 0, None, 0, n, 0, f"c = n - 2, n={n}")
        assert changed_ids(bits, want, V) == [[]]
        bits, want = run(V, hist, [n - 1], None, 0, None, 0, n, 0, f"c = n - 1, n={n}")
        assert changed_ids(bits, want, V) == [[a]]


def test_the_longest_ngram():
    V, n, out_ld = 65, 64, 160
    ids = pick(V, 4, B=2)
    rng = np.random.default_rng(5)
    hist = np.array(ids, dtype=np.int32)[rng.integers(0, 4, (2, out_ld))]
    hist[:, 80:143] = hist[:, 10:73]                                          # 63 columns recur; c = 142; the follower sits at 73
    hist[0, 73], hist[1, 73] = ids[0], ids[1]
    hist[1, 100] = hist[1, 30] + 1000                                         # row 1: one column of the 63 differs -- no ban
    bits, want = run(V, hist, [142], None, 0, None, 0, n, 0, "n=64")
    assert changed_ids(bits, want, V) == [[ids[0]], []]
    bits, want = run(V, hist, [142], None, 0, None, 0, n, 133, "n=64 span holds")  # lo = 10
    assert changed_ids(bits, want, V) == [[ids[0]], []]
    bits, want = run(V, hist, [142], None, 0, None, 0, n, 132, "n=64 span cuts")
    assert changed_ids(bits, want, V) == [[], []]


def test_banned_and_counted_gets_the_ban_not_the_sum():
    V = 65
    a, b = pick(V, 2)
    hist = _filler()
    hist[0, 10:14] = [a, b, b, a]                                             # c = 13: "a" was followed by b; b is counted twice
    pen = pen_for(8)
    bits, want = run(V, hist, [13], None, 0, np.ones(V), 8, 2, 0, "banned and counted", pen=pen)
    assert changed_ids(bits, want, V) == [sorted([a, b])]
    xb = repeat_ref.bf16_bits_to_f32(bits[0, b:b + 1])
    assert want[0, b] == repeat_ref.f32_to_bf16_bits(xb - np.float32(BAN))[0]
    xa = repeat_ref.bf16_bits_to_f32(bits[0, a:a + 1])
    assert want[0, a] == repeat_ref.f32_to_bf16_bits(xa - pen[2])[0]
    # a small ban, so that ban and ban + pen differ after the rounding too
    bits, want = run(V, hist, [13], None, 0, np.ones(V), 8, 2, 0, "banned and counted, ban 2", ban=2.0, pen=pen)
    assert want[0, b] == repeat_ref.f32_to_bf16_bits(xb - np.float32(2.0))[0]
    assert want[0, b] != repeat_ref.f32_to_bf16_bits(xb - np.float32(2.0) - pen[2])[0]


def test_inert_by_design():
    V = 65
    rng = np.random.default_rng(3)
    hist = np.array([0, 5, 9, 64], dtype=np.int32)[rng.integers(0, 4, (3, OUT_LD))]
    bits, want = run(V, hist, [40], None, 0, np.zeros(V), 16, 0, 0, "subject all zero")
    assert (bits == want).all()
    bits, want = run(V, hist, [OUT_LD], None, 0, np.ones(V), 16, 2, 0, "c = out_ld")
    assert (bits == want).all()
    bits, want = run(V, hist, [-1, 5, OUT_LD + 7], None, 1, np.ones(V), 16, 2, 0, "rows outside")
    assert (bits[0] == want[0]).all() and (bits[2] == want[2]).all() and (bits[1] != want[1]).any()
    bits, want = run(V, hist, [40], None, 0, None, 0, 2, 0, "window 0, NULL tables")
    assert (bits != want).any()
    bits, want = run(V, hist, [40], None, 0, np.ones(V), 16, 0, 0, "ngram 0")
    assert (bits != want).any()


@pytest.mark.parametrize("per_row", [0, 1])
def test_six_chained_steps_and_a_reanchor(per_row):
    """a scripted stream: the host writes every token where the sampler would (column base + pos + 1) and advances the position;
    every step's logits are fresh.  The second run re-anchors half way (base += h, pos -= h): the columns, so the amounts, are
    the same"""
    V, B, steps, h = 65, 3, 6, 4
    window, n, span = 4, 2, 0
    rng = np.random.default_rng(21 + per_row)
    ids = np.array(pick(V, 3), dtype=np.int32)
    script = ids[rng.integers(0, 3, (B, steps))]
    rows = B if per_row else 1
    start = (rng.integers(4, 9, rows) if per_row else np.array([6])).astype(np.int32)      # the column of the first input token
    hist0 = _filler(B)
    for b in range(B):
        s = start[b if per_row else 0]
        hist0[b, :s + 1] = ids[rng.integers(0, 3, s + 1)]                                   # a prompt
    subject, pen = np.ones(V, dtype=np.int32), pen_for(window)
    results = []
    for reanchor in (False, True):
        hist, pos, base = banded(hist0), banded(start), banded(np.zeros(rows, dtype=np.int32))
        sj, pn = banded(subject), banded(pen, torch.float32)
        ref_hist, outs = hist0.copy(), []
        for s in range(steps):
            if reanchor and s == 3:
                base.t.add_(h)
                pos.t.sub_(h)
            x, bits = logits_for(np.random.default_rng(100 + s), B, V, 128)
            lg = banded(x, torch.bfloat16)
            KC.ops().repeat_penalty(lg.t, V, hist.t, pos.t, sj.t, pn.t, window, n, span, BAN, ragged=bool(per_row), base=base.t)
            c = start + s
            want = repeat_ref.penalise(bits, V, ref_hist, c, None, per_row, subject, pen, window, n, span, BAN)
            KC.check_equal("chain", KC.bits16(lg.t).to(torch.int32), torch.from_numpy(want.view(np.int16).astype(np.int32)),
                           f"per_row={per_row} reanchor={reanchor} step {s}")
            assert lg.bands_intact()
            outs.append((bits, want))
            cols = torch.from_numpy(np.broadcast_to(c + 1, (B,)).astype(np.int64)).to(hist.t.device)
            hist.t[torch.arange(B, device=hist.t.device), cols] = torch.from_numpy(script[:, s].copy()).to(hist.t.device)      # the sampler's write
            ref_hist[np.arange(B), np.broadcast_to(c + 1, (B,))] = script[:, s]
            pos.t.add_(1)                                                                   # and its advance
        torch.cuda.synchronize()
        assert (hist.t.cpu().numpy() == ref_hist).all() and hist.bands_intact() and pos.bands_intact() and base.bands_intact()
        assert (base.t.cpu().numpy() + pos.t.cpu().numpy() == start + steps).all()
        results.append(outs)
    assert all((a[1] == b[1]).all() for a, b in zip(*results))                              # identical amounts across the re-anchor
    assert sum(int((bits != want).sum()) for bits, want in results[0]) > steps              # the chain penalises and bans
    last_bits, last_want = results[0][-1]
    fin = last_bits[:, :V] != 0xFF80                                                        # -inf stays -inf
    assert (np.abs(repeat_ref.bf16_bits_to_f32(last_want[:, :V][fin]).astype(np.float64)
                   - repeat_ref.bf16_bits_to_f32(last_bits[:, :V][fin]).astype(np.float64)) > 5000).any()   # some id is banned


def test_error_codes():
    lib, _, _, _ = KC.raw()
    V, B = 65, 2
    lg = banded(torch.zeros(B, 128), torch.bfloat16)
    hist, pos = banded(np.zeros((B, OUT_LD), dtype=np.int32)), banded(np.zeros(1, dtype=np.int32))
    sj, pn = banded(np.ones(V, dtype=np.int32)), banded(np.zeros(9, dtype=np.float32), torch.float32)
    before = KC.bits16(lg.t).clone()

    def call(**kw):
        a = dict(dict(logits=KC.P(lg), V=V, ld=128, out=KC.P(hist), out_ld=OUT_LD, pos=KC.P(pos), base=None, per_row=0, subject=KC.P(sj),
                      pen=KC.P(pn), window=8, ngram=3, span=0, ban=BAN, B=B), **kw)
        return lib.mgx_repeat_penalty(a["logits"], a["V"], a["ld"], a["out"], a["out_ld"], a["pos"], a["base"], a["per_row"],
                                      a["subject"], a["pen"], a["window"], a["ngram"], a["span"], a["ban"], a["B"], KC.raw()[3]())
    NULL, SHAPE = -2, -1
    for kw in (dict(logits=None), dict(out=None), dict(pos=None), dict(subject=None), dict(pen=None)):
        assert call(**kw) == NULL, kw
    for kw in (dict(B=0), dict(V=0), dict(V=1025, ld=1088), dict(ld=64), dict(out_ld=0), dict(window=-1), dict(window=4097),
               dict(ngram=1), dict(ngram=65), dict(ngram=-3), dict(span=2), dict(span=-1), dict(window=0, ngram=0),
               dict(window=0, ngram=0, subject=None, pen=None), dict(ban=0.0), dict(ban=-1.0), dict(ban=float("inf")),
               dict(ban=float("nan"))):
        assert call(**kw) == SHAPE, kw
        assert b"mgx_repeat_penalty" in lib.mgx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(KC.bits16(lg.t), before)                               # a refused call launches nothing
    # what the clauses allow: NULL tables with window 0; any ban with ngram 0; a span with ngram 0; window at its cap is a shape
    # question only for pen (not read beyond cnt <= c + 1 entries here: c = 0 counts one column)
    assert call(window=0, subject=None, pen=None) == 0
    assert call(ngram=0, ban=float("nan")) == 0
    assert call(ngram=0, span=1) == 0
    assert call(ngram=64, span=64) == 0 and call(ngram=2, span=2) == 0
    torch.cuda.synchronize()
    for b_ in (lg, hist, pos, sj, pn):
        assert b_.bands_intact()
