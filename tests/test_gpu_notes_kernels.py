"""The three held-note kernels (ABI 28) against the numpy restatement of their header contracts (tests/notes_ref.py).  All are
integer work, so every check is exact: the logits' BITS after mgx_notes_mask -- the columns at and beyond V and the guard bands
included -- all of mgx_notes_account's state, and mgx_notes_keep's tokens and output matrix.  The chained test plays six steps, the host doing the sampler's draw between
the two calls (legal draws from the masked logits, and two scripted ones that ignore the mask), and must arrive at
notes_ref.fold's set."""
import numpy as np
import pytest
import torch

import kernel_checks as KC
import notes_ref
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)

pytestmark = pytest.mark.gpu

# bits 0, 31, 32, 63, 64 and 127 (the edges of the four words) with both of their ids, rule-0 ids, and values outside
# -128 .. 128, which count as 0.  Entries 0, 3 and 5 are clear-rules: with the shifts below id 0 is one, so V = 1 masks too
RULES = [-1, 1, 32, -32, 33, -33, 64, -64, 65, -65, 128, -128, 0, 6, -6, 0, 200, -200, 2 ** 31 - 1, -2 ** 31]
SHIFTS = (0, 3, 5)
EDGES = [0, 31, 32, 63, 64, 95, 96, 127]


def banded(a, dtype=torch.int32):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return KC.Banded(t.to(dtype), KC.BAND, KC.PATTERN)


def row_sets(rng):
    """B = 3 rows each: empty / all 128 bits / random; then the single bits at every word edge, and one more random row.  Every
    set holds a row without any given bit"""
    rand = [set(np.flatnonzero(rng.random(128) < p).tolist()) for p in (0.3, 0.04)]
    single = [{k} for k in EDGES]
    return [[set(), set(range(128)), rand[0]], single[0:3], single[3:6], single[6:8] + [rand[1]]]


@pytest.mark.parametrize("V", [1, 63, 64, 65, 309, 1024])
def test_mask(V):
    ld = (V + 63) // 64 * 64                                                  # V = 64 and 1024 leave no column beyond V: the band follows
    B = 3
    cap_alone = False
    for shift in SHIFTS:
        rule = np.array([RULES[(v + shift) % len(RULES)] for v in range(V)], dtype=np.int32)
        rng = np.random.default_rng(1000 * V + shift)
        for si, rows in enumerate(row_sets(rng)):
            state = np.stack([notes_ref.words(s) for s in rows])
            pc = len(rows[2])                                                 # the caps: around the last row's count, 1 and none
            for max_on in sorted({min(max(m, 1), 128) for m in (1, pc - 1, pc, pc + 1, 128)}):
                x = torch.from_numpy(rng.normal(size=(B, ld)) * 4.0).to(torch.bfloat16)
                x[:, V:] = float("nan")
                x[torch.from_numpy(rng.random((B, ld)) < 0.1)] = float("-inf")     # logits that already hold -inf
                x[:, 0] = 1.0                                                  # (not id 0: at V = 1 it is what the case masks)
                bits = x.view(torch.int16).numpy().view(np.uint16)
                lg, r, st = banded(x, torch.bfloat16), banded(rule), banded(state)
                KC.ops().notes_mask(lg.t, V, r.t, st.t, max_on)
                torch.cuda.synchronize()
                want = notes_ref.mask(bits, V, rule, state, max_on)
                case = f"V={V} ld={ld} shift={shift} rows={si} counts={[len(s) for s in rows]} max_on={max_on}"
                KC.check_equal("mask", KC.bits16(lg.t).to(torch.int32), torch.from_numpy(want.view(np.int16).astype(np.int32)), case)
                assert (want[:, V:] == bits[:, V:]).all()                      # the reference itself: columns >= V stay,
                assert (want[:, :V][:, (rule == 0) | (np.abs(rule.astype(np.int64)) > 128)] ==
                        bits[:, :V][:, (rule == 0) | (np.abs(rule.astype(np.int64)) > 128)]).all()     # and the rule-0 ids
                assert (want != bits).any(), case                              # the case masks something
                cap_alone |= bool((want != notes_ref.mask(bits, V, rule, state, 128)).any())
                for b in (lg, r, st):
                    assert b.bands_intact(), case
                assert r.t.cpu().tolist() == rule.tolist() and (st.t.cpu().numpy() == state).all(), case      # read only
    assert cap_alone or V == 1                                                # some case masks on the cap alone (V = 1 has no set-rule)


def account_case(B, seed):
    """rows cycle through: a set of a clear bit; a set of a set bit; a clear of a set bit; a clear of a clear bit; a rule-0
    token; token -1; a token >= V (whose entry of the longer table would set a bit).  The other 127 bits are random"""
    rng = np.random.default_rng(seed)
    rule = np.array([1, -1, 32, -32, 33, -33, 128, -128, 0, 64, -64, 0, 3, -3], dtype=np.int32)
    Vc = 12                                                                   # the last two entries lie beyond V
    keys = [(0, 1, 0), (2, 3, 31), (4, 5, 32), (6, 7, 127), (9, 10, 63)]      # (the id that sets, the id that clears, the bit)
    tok = np.zeros(B, dtype=np.int32)
    state = np.zeros((B, 4), dtype=np.int32)
    for b in range(B):
        kind = b % 7
        on, off, k = keys[(b // 7) % len(keys)]
        held = set(np.flatnonzero(rng.random(128) < 0.3).tolist()) - {k}
        if kind in (1, 2):
            held.add(k)
        tok[b] = (on, on, off, off, (8, 11)[b // 7 % 2], -1, (12, 13, 10 ** 6)[b // 7 % 3])[kind]
        state[b] = notes_ref.words(held)
    return tok, rule, state, Vc


@pytest.mark.parametrize("B", [1, 5, 257])
def test_account(B):
    tok, rule, state, Vc = account_case(B, seed=B)
    t, r, st = banded(tok), banded(rule), banded(state)
    KC.ops().notes_account(t.t, r.t, st.t, Vc)
    torch.cuda.synchronize()
    want = notes_ref.account(tok, rule, state, Vc)
    case = f"B={B}"
    KC.check_equal("account state", st.t, torch.from_numpy(want.astype(np.int64)), case)
    KC.check_equal("account next_tok", t.t, torch.from_numpy(tok.astype(np.int64)), case)
    KC.check_equal("account rule", r.t, torch.from_numpy(rule.astype(np.int64)), case)
    for b in (t, r, st):
        assert b.bands_intact(), case
    changed = (want != state).any(1)
    assert changed[0] and changed[np.arange(B) % 7 == 2].all()                # sets of clear bits and clears of set bits change a row,
    assert not changed[np.isin(np.arange(B) % 7, (1, 3, 4, 5, 6))].any()      # nothing else does


def keep_case(B, per_row, with_base, seed, out_ld=16):
    """rows cycle through first draws that are: a rule-0 id; a set of a clear bit below the cap; a set of a set bit; a set of a
    clear bit AT the cap; a clear of a set bit; a clear of a clear bit; -1; an id >= V; legal with its column outside the row"""
    rng = np.random.default_rng(seed)
    rule = np.array([1, -1, 32, -32, 33, -33, 128, -128, 0, 64, -64, 0, 3, -3], dtype=np.int32)
    Vc, max_on = 12, 5
    keys = [(0, 1, 0), (2, 3, 31), (4, 5, 32), (6, 7, 127), (9, 10, 63)]
    first = np.zeros(B, dtype=np.int32)
    state = np.zeros((B, 4), dtype=np.int32)
    kind = np.arange(B) % 9
    for b in range(B):
        on, off, k = keys[(b // 9) % len(keys)]
        others = [x for x in rng.permutation(128) if x != k]
        n = max_on if kind[b] == 3 else int(rng.integers(0, max_on - 1))      # below the cap also after k is added
        held = set(int(x) for x in others[:n])
        if kind[b] in (2, 4):
            held.add(k)
        first[b] = (8, on, on, on, off, off, -1, (12, 13, 10 ** 6)[b // 9 % 3], 11)[kind[b]]
        state[b] = notes_ref.words(held)
    n = B if per_row else 1
    base = rng.integers(0, 4, n).astype(np.int32) if with_base else None
    pos = rng.integers(1, out_ld - 4, n).astype(np.int32)
    if per_row:                                                               # kind 8: column out_ld, outside the row
        pos = np.where(kind == 8, out_ld - (base if with_base else 0), pos).astype(np.int32)
    return dict(first=first, next_tok=rng.integers(0, Vc, B).astype(np.int32) + 100, out=rng.integers(0, Vc, (B, out_ld)).astype(np.int32) + 100,
                pos=pos, base=base, rule=rule, state=state), Vc, max_on


@pytest.mark.parametrize("with_out", [True, False])
@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("per_row", [0, 1])
@pytest.mark.parametrize("B", [1, 9, 257])
def test_keep(B, per_row, with_base, with_out):
    c, Vc, max_on = keep_case(B, per_row, with_base, seed=B * 8 + per_row * 4 + with_base * 2 + with_out)
    dev = {k: None if v is None else banded(v) for k, v in c.items()}
    KC.ops().notes_keep(dev["first"].t, dev["next_tok"].t, dev["out"].t if with_out else None, dev["pos"].t, dev["rule"].t,
                        dev["state"].t, max_on, Vc, ragged=bool(per_row), base=None if not with_base else dev["base"].t)
    torch.cuda.synchronize()
    tok, out = notes_ref.keep(c["first"], c["next_tok"], c["out"] if with_out else None, c["pos"], c["base"], per_row, c["rule"],
                              c["state"], max_on, Vc)
    case = f"B={B} per_row={per_row} base={with_base} out={with_out}"
    want = dict(c, next_tok=tok, out=out if with_out else c["out"])
    for name, w in want.items():
        if w is None:
            continue
        KC.check_equal("keep " + name, dev[name].t, torch.from_numpy(np.asarray(w, dtype=np.int64)), case)
        assert dev[name].bands_intact(), (case, name)
    kept = tok != c["next_tok"]
    kind = np.arange(B) % 9
    assert kept[np.isin(kind, (0, 1, 4, 8))].all() and not kept[np.isin(kind, (2, 3, 5, 6, 7))].any(), case
    if with_out and B >= 9:
        assert (out != c["out"]).any() and ((out != c["out"]).sum(1) <= 1).all()


def test_six_chained_steps_arrive_at_the_fold():
    """mask -> the host's draw -> account, six times.  At steps 0, 1, 3 and 5 the host draws the largest masked logit (a legal
    id by construction); at steps 2 and 4 it writes a scripted id whatever the mask says -- a double note_on, an orphan
    note_off -- which account must fold all the same.  Every step's mask is compared with the reference on the host's own fold"""
    V, ld, B, max_on = 12, 64, 4, 3
    rule = np.array([1, -1, 32, -32, 33, -33, 128, -128, 0, 64, -64, 0], dtype=np.int32)
    start = [set(), {0, 31}, {32, 127, 63}, {5}]                             # row 2 starts at the cap; bit 5 has no id at all
    scripted = {2: [0, 0, 1, 7], 4: [3, 8, 4, -1]}
    rng = np.random.default_rng(17)
    r, st, tok = banded(rule), banded(np.stack([notes_ref.words(s) for s in start])), banded(np.zeros(B, dtype=np.int32))
    held = [set(s) for s in start]
    drawn = [[] for _ in range(B)]
    illegal = 0
    for s in range(6):
        x = torch.from_numpy(rng.normal(size=(B, ld)) * 4.0).to(torch.bfloat16)
        x[:, V:] = float("nan")
        bits = x.view(torch.int16).numpy().view(np.uint16)
        lg = banded(x, torch.bfloat16)
        KC.ops().notes_mask(lg.t, V, r.t, st.t, max_on)
        torch.cuda.synchronize()
        want = notes_ref.mask(bits, V, rule, np.stack([notes_ref.words(h) for h in held]), max_on)
        KC.check_equal("chain mask", KC.bits16(lg.t).to(torch.int32), torch.from_numpy(want.view(np.int16).astype(np.int32)), f"step {s}")
        assert lg.bands_intact()
        if s in scripted:
            draw = np.array(scripted[s], dtype=np.int32)
            illegal += sum(0 <= t < V and notes_ref.banned_id(rule, t, held[b], max_on) for b, t in enumerate(draw))
        else:
            draw = lg.t[:, :V].float().argmax(1).cpu().numpy().astype(np.int32)
            assert not any(notes_ref.banned_id(rule, t, held[b], max_on) for b, t in enumerate(draw)), f"step {s}"
        tok.t.copy_(torch.from_numpy(draw))
        KC.ops().notes_account(tok.t, r.t, st.t, V)
        for b in range(B):
            held[b] = notes_ref.apply(rule, V, held[b], int(draw[b]))
            drawn[b].append(int(draw[b]))
    torch.cuda.synchronize()
    assert illegal >= 2                                                       # the scripted draws did break rules
    got = st.t.cpu().numpy()
    for b in range(B):
        assert notes_ref.bits_of(got[b]) == notes_ref.fold(rule, V, drawn[b], start[b]) == held[b], (b, drawn[b])
    assert 5 in notes_ref.bits_of(got[3])                                     # a bit no id names is never touched
    for t_ in (r, st, tok):
        assert t_.bands_intact()
