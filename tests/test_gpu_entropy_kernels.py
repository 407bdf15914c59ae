"""mgx_entropy_mask and mgx_entropy_account (ABI 34) against the fp64 restatement of their header contracts (tests/entropy_ref.py).

The mask is a pure mask, so its check is exact: the logits after the call are, bit for bit, the logits before it with 0xFF80 at
the ids of the live set that the reference drops.  The inputs are redrawn until every margin the reference reports for its own
cuts is >= 1e-3 (asserted on the inputs alone, on the CPU) -- bits for the Mirostat cut, nats for min-p, relative mass and nats of
d for the typical set -- far above the f32 error of the quantities compared (1e-5, below), so the two cannot disagree about a
kept set there.  Exact ties at a cut have a case of their own.

The bound on lse_out, |got - lse| <= 1e-5 + 2^-21 max_A |z|:  z = x * (1 / temperature) carries two f32 roundings (the reciprocal
and the product), 2^-23 |z|, which moves lse by at most that.  A term e^(z - m): the difference and its scaling by log2(e) inside
the fast exponential are rounded at 2^-24 |z - m| each and the hardware exponential is good to 2^-23, so a term's relative error is
1.5e-7 |z - m| + 1.2e-7; weighted by the terms themselves, sum_v p_v |z_v - m| <= ln 1024 = 6.93, the sum is off by 1.2e-6
relative.  Summing: 16 adds per lane, 4 across the row of 16 lanes and 3 across the rows, 23 roundings, 1.4e-6.  The logarithm of a
sum in [1, 1024]: 2 ulp of at most 6.93, 1e-6.  The last add, m + ln(sum): 2^-24 |lse|.  Together 3.6e-6 + 2^-22 max |z|; the test
allows 1e-5 + 2^-21 max |z|, twice the second term for the rows whose |lse| exceeds max |z| by ln 1024.

The account's bounds, with z = x * (1 / temperature) and s = (lse - z) / ln 2 on f32 inputs:  |got - s| <= 2^-22 (|z| log2(e) + |s|)
-- the two roundings of z (2^-23 |z|, divided by ln 2), the rounding of the difference and of the quotient and the f32 value of
ln 2 (2^-24 |s| each, 2^-22 |s| allowed) -- and |got - mu'| <= eta (that bound) + 2^-22 eta |s - tau| + 2^-24 |mu'|: the rounding
of s - tau, of eta itself, of the product and of the last subtraction.  Buffers sit inside guard bands; everything a call only
reads is compared afterwards."""
import numpy as np
import pytest
import torch

import entropy_ref
import kernel_checks as KC
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)

pytestmark = pytest.mark.gpu

SEEN = {}
_report = KC.report_fixture(SEEN, "largest error / bound = {:.3g}")
MARGIN = 1e-3
T_CALL = 0.9
NEG = np.int16(np.uint16(0xFF80).view(np.int16))
SETTINGS = {"mirostat": dict(mu=4.0), "min_p": dict(min_p=0.02), "typical": dict(typical_p=0.5),
            "all": dict(mu=4.0, min_p=0.05, typical_p=0.5)}


def banded(a, dtype):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return KC.Banded(t.to(dtype), KC.BAND, KC.PATTERN)


def table_for(rng, V, tok):
    """a random grammar table (bit v of row t, ~70 % set) whose row of tok[3] -- where there is one -- allows nothing"""
    W = (V + 31) // 32
    bits = rng.random((V, W * 32)) < 0.7
    bits[:, V:] = False
    if len(tok) > 3:
        bits[min(max(tok[3], 0), V - 1)] = False
    return (bits.reshape(V, W, 32) * (1 << np.arange(32, dtype=np.uint64))).sum(-1).astype(np.uint32)


def draw_rows(rng, B, V, ld, tok, table, min_p=0.0, typical_p=1.0, mu=None):
    """bf16-valued logits ~ N(0, 3^2) with ~10 % -inf, float64 [B, ld] (NaN beyond V), every row redrawn until the reference's
    margins on it are >= MARGIN.  In a batch of five, row 1 is all -inf, row 3's grammar row is empty (table_for) and row 4's
    grammar row allows only ids that are -inf"""
    x = np.full((B, ld), np.nan)
    for b in range(B):
        allowed = None if table is None else entropy_ref.allowed_bits(table, tok[b], V)
        for _ in range(500):
            r = entropy_ref.bf16_values(rng.normal(size=V) * 3.0)
            r[rng.random(V) < 0.1] = -np.inf
            if B == 5 and b == 1:
                r[:] = -np.inf
            if B == 5 and b == 4 and allowed is not None:
                r[allowed] = -np.inf
            _, _, margins = entropy_ref.mask_row(r, T_CALL, min_p, typical_p, mu, allowed)
            if entropy_ref.smallest(margins) >= MARGIN:
                break
        else:
            raise AssertionError("no row with wide margins in 500 draws")
        x[b, :V] = r
    return x


def run(x, V, case, temperature=T_CALL, min_p=0.0, typical_p=1.0, mu=None, tok=None, table=None, want_lse=True):
    """one call, checked against the reference; mu: one value for every row or None.  -> the kept set, booleans [B, V]"""
    B, ld = x.shape
    mus = None if mu is None else np.full(B, mu, dtype=np.float32)
    kept, touched, lse, margins = entropy_ref.mask(x, V, temperature, min_p, typical_p, mus, tok, table)
    assert entropy_ref.smallest(margins) >= MARGIN, (case, entropy_ref.smallest(margins))      # on the inputs alone
    before = torch.from_numpy(x).to(torch.bfloat16)
    lg = banded(before, torch.bfloat16)
    mu_b = None if mus is None else banded(mus, torch.float32)
    out = KC.output((B,), torch.float32) if want_lse else None
    tb = None if table is None else banded(table.view(np.int32), torch.int32)
    to = None if table is None else banded(np.asarray(tok, dtype=np.int32), torch.int32)
    KC.ops().entropy_mask(lg.t, V, temperature, min_p, typical_p, mu=None if mu_b is None else mu_b.t,
                          lse_out=None if out is None else out.t, tok=None if to is None else to.t,
                          allow_table=None if tb is None else tb.t)
    torch.cuda.synchronize()
    for b_ in (lg, mu_b, out, tb, to):
        assert b_ is None or b_.bands_intact(), case
    for b_, a in ((mu_b, mus), (to, None if table is None else np.asarray(tok, dtype=np.int32)),
                  (tb, None if table is None else table.view(np.int32))):
        assert b_ is None or (b_.t.cpu().numpy() == a).all(), case            # what the call only reads
    bits0, bits1 = KC.bits16(before).numpy(), KC.bits16(lg.t).numpy()
    live = np.stack([entropy_ref.live_set(x[b, :V], None if table is None else entropy_ref.allowed_bits(table, tok[b], V))
                     for b in range(B)])
    want = bits0.copy()
    want[:, :V][live & ~kept & touched[:, None]] = NEG        # a pure mask: -inf at A \ S3, every other value bit for bit
    bad = np.argwhere(bits1 != want)
    assert bad.size == 0, (case, "the logits differ from the masked input at", bad[:4].tolist())
    assert (kept[touched].any(1)).all(), case
    if want_lse:
        got = out.t.cpu().to(torch.float64)
        assert (got[torch.from_numpy(~touched)] == 0).all(), case
        with np.errstate(invalid="ignore"):
            zmax = np.array([np.abs(x[b, :V][live[b]] / temperature).max() if touched[b] else 0.0 for b in range(B)])
        bound = torch.from_numpy(np.where(touched, 1e-5 + 2.0 ** -21 * zmax, 0.0))
        KC.check_bound("entropy_mask lse", got, torch.from_numpy(lse), bound, case, seen=SEEN)
    return kept


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 337, 1024])
def test_mask_against_the_reference(V, setting):
    cases = masked = 0
    kw = SETTINGS[setting]
    for B in (1, 5):
        for ld in (V, V + 7):
            for grammar in (False, True):
                seed = ((V * 17 + list(SETTINGS).index(setting)) * 2 + (B == 5)) * 4 + (ld > V) * 2 + grammar
                rng = np.random.default_rng(seed)
                tok = rng.integers(0, V, B).tolist()
                if B == 5:
                    tok[0] = V + 5                                            # clamped to the last row of the table
                table = table_for(rng, V, tok) if grammar else None
                x = draw_rows(rng, B, V, ld, tok, table, **kw)
                case = f"{setting} V={V} B={B} ld={ld} grammar={grammar}"
                kept = run(x, V, case, tok=tok if grammar else None, table=table, **kw)
                cases += 1
                masked += int(((x[:, :V] > -np.inf) & ~kept).sum())
    assert cases == 8 and (masked > 0 or V <= 2)


def test_exact_ties_straddling_the_cuts():
    """equal bf16 logits on both sides of each of the three cuts, the tie spanning two lanes (ids 3, 33) and two slots of one lane
    (ids 3, 67): the tied ids are kept together or dropped together"""
    V = 70
    x = np.full((1, V), -np.inf)
    x[0, [0, 3, 33, 67, 34]] = [2.0, 1.0, 1.0, 1.0, 0.5]                     # p = (0.430, 0.158 x 3, 0.096): 1.22, 2.66, 3.38 bits
    tie = [3, 33, 67]

    def ids(**kw):
        return np.flatnonzero(run(x, V, f"ties {kw}", temperature=1.0, **kw)[0]).tolist()
    assert ids(mu=3.0) == [0] + tie and ids(mu=2.0) == [0]                    # the Mirostat cut below and above the tie
    assert ids(min_p=0.3) == [0] + tie and ids(min_p=0.5) == [0]              # the tie is at e^-1 = 0.37 of the maximum
    # typical: H = 1.462 nats, d = 0.618 (id 0), 0.382 (the tie), 0.882 (id 34).  The tie comes first with a mass of 0.474: a mass
    # of 0.3 is reached inside it -- one tied id has 0.158, two have 0.316 -- and all three are kept
    assert ids(typical_p=0.3) == tie and ids(typical_p=0.6) == [0] + tie
    # the tie last: p = (0.491, 0.181, 0.110 x 3), d = 0.674, 0.326, 0.826.  0.5 is reached before the tie, which is dropped as a
    # whole; 0.8 is reached inside it
    x[0, [0, 1, 3, 33, 67, 34]] = [2.0, 1.0, 0.5, 0.5, 0.5, -np.inf]
    assert ids(typical_p=0.5) == [0, 1] and ids(typical_p=0.8) == [0, 1] + tie
    assert ids(mu=3.5, min_p=0.2, typical_p=0.8) == [0, 1] + tie              # all three stages, the tie (3.19 bits) kept by each


def test_inert_parameters_write_only_the_log_sum_exp():
    """mu NULL, min_p 0, typical_p 1: a legal call; run() requires the logits back bit for bit and checks lse_out"""
    rng = np.random.default_rng(11)
    for V, B, ld in ((337, 5, 344), (1024, 1, 1024)):
        tok = rng.integers(0, V, B).tolist()
        table = table_for(rng, V, tok)
        x = draw_rows(rng, B, V, ld, tok, table)
        run(x, V, f"inert V={V}", tok=tok, table=table)
        run(x, V, f"inert V={V}, no lse_out", want_lse=False)                 # and with nothing at all to write


def test_the_mirostat_fallback_keeps_the_arg_max_ties():
    """mu = -1: no id is that unsurprising, so the ids at the maximum stand in -- three of them, over two lanes and two slots"""
    V = 200
    rng = np.random.default_rng(5)
    x = entropy_ref.bf16_values(rng.normal(size=(2, V)) * 3.0)
    x[x > 6.0] = 6.0
    x[0, [7, 71, 150]] = 7.5
    x[1, 199] = 9.0
    kept = run(x, V, "fallback", mu=-1.0)
    assert np.flatnonzero(kept[0]).tolist() == [7, 71, 150] and np.flatnonzero(kept[1]).tolist() == [199]
    kept = run(x, V, "fallback, then min-p and typical", mu=-1.0, min_p=0.5, typical_p=0.5)
    assert np.flatnonzero(kept[0]).tolist() == [7, 71, 150] and np.flatnonzero(kept[1]).tolist() == [199]


# ---- the account ----------------------------------------------------------------------------------------------------------------
def account(case, x, V, next_tok, lse, mu, tau, eta, pos, base, per_row, out_ld, temperature=T_CALL, trace=True):
    """one call of mgx_entropy_account, checked.  pos / base: lists (one entry, or one per row with per_row)"""
    B, ld = x.shape
    s_ref, mu_ref = entropy_ref.account(next_tok, x, V, temperature, lse.astype(np.float64), None if mu is None else mu.astype(np.float64),
                                        tau, eta)
    cols = [(pos[b if per_row else 0] + (base[b if per_row else 0] if base is not None else 0)) for b in range(B)]
    if trace:                                                                 # a column outside the matrix: nothing is written
        for b in range(B):
            if not 0 <= cols[b] < out_ld:
                s_ref[b] = np.nan
                if mu_ref is not None:
                    mu_ref[b] = mu[b]
    lg, nt = banded(torch.from_numpy(x).to(torch.bfloat16), torch.bfloat16), banded(np.asarray(next_tok, dtype=np.int32), torch.int32)
    ls, po = banded(lse, torch.float32), banded(np.asarray(pos, dtype=np.int32), torch.int32)
    ba = None if base is None else banded(np.asarray(base, dtype=np.int32), torch.int32)
    mu_b = None if mu is None else banded(mu, torch.float32)
    out = KC.output((B, out_ld), torch.float32, init=torch.full((B, out_ld), float("nan"))) if trace else None
    before = KC.bits16(lg.t).clone()
    KC.ops().entropy_account(nt.t, lg.t, V, temperature, ls.t, po.t, mu=None if mu_b is None else mu_b.t, tau=tau, eta=eta,
                             surprise_out=None if out is None else out.t, ragged=bool(per_row), base=None if ba is None else ba.t)
    torch.cuda.synchronize()
    for b_ in (lg, nt, ls, po, ba, mu_b, out):
        assert b_ is None or b_.bands_intact(), case
    assert torch.equal(KC.bits16(lg.t), before), case                         # what the call only reads
    for b_, a in ((nt, np.asarray(next_tok, dtype=np.int32)), (ls, lse), (po, np.asarray(pos, dtype=np.int32)),
                  (ba, None if base is None else np.asarray(base, dtype=np.int32))):
        assert b_ is None or (b_.t.cpu().numpy() == a).all(), case
    acc = ~np.isnan(s_ref)
    with np.errstate(invalid="ignore"):
        z = np.array([x[b, next_tok[b]] / temperature if acc[b] else 0.0 for b in range(B)])
    s_bound = np.where(acc, 2.0 ** -22 * (np.abs(z) * np.log2(np.e) + np.abs(np.nan_to_num(s_ref))), 0.0)
    if trace:
        got = out.t.cpu().to(torch.float64).numpy()
        want = np.full((B, out_ld), np.nan)
        for b in range(B):
            if acc[b]:
                want[b, cols[b]] = s_ref[b]
        assert (np.isnan(got) == np.isnan(want)).all(), (case, "the written cells differ", np.argwhere(np.isnan(got) != np.isnan(want))[:4].tolist())
        if acc.any():
            rows = np.flatnonzero(acc)
            KC.check_bound("entropy_account s", torch.from_numpy(got[rows, [cols[b] for b in rows]]), torch.from_numpy(s_ref[rows]),
                           torch.from_numpy(s_bound[rows]), case, seen=SEEN)
    if mu is not None:
        got_mu = mu_b.t.cpu().numpy()
        assert (got_mu[~acc] == mu[~acc]).all(), (case, "a row that accounts nothing moved its mu")
        if acc.any():
            bound = eta * s_bound + 2.0 ** -22 * eta * np.abs(np.nan_to_num(s_ref) - tau) + 2.0 ** -24 * np.abs(mu_ref)
            KC.check_bound("entropy_account mu", torch.from_numpy(got_mu[acc].astype(np.float64)), torch.from_numpy(mu_ref[acc]),
                           torch.from_numpy(bound[acc]), case, seen=SEEN)
    return acc


def test_account_against_the_reference():
    V, ld, B, out_ld = 337, 344, 6, 40
    rng = np.random.default_rng(2)
    x = np.full((B, ld), np.nan)
    x[:, :V] = entropy_ref.bf16_values(rng.normal(size=(B, V)) * 3.0)
    x[:, :V][rng.random((B, V)) < 0.1] = -np.inf
    next_tok = [int(np.flatnonzero(x[b, :V] > -np.inf)[5 * b + 1]) for b in range(B)]
    lse = np.array([entropy_ref._lse(x[b, :V][x[b, :V] > -np.inf] / T_CALL) for b in range(B)]).astype(np.float32)
    mu = (6.0 + rng.normal(size=B)).astype(np.float32)
    tau, eta = 3.0, 0.1
    every = np.ones(B, dtype=bool)
    # the shared counter and one position per row, with and without a base
    assert (account("shared", x, V, next_tok, lse, mu, tau, eta, [7], None, 0, out_ld) == every).all()
    assert (account("shared, base", x, V, next_tok, lse, mu, tau, eta, [7], [21], 0, out_ld) == every).all()
    assert (account("per row", x, V, next_tok, lse, mu, tau, eta, [3, 0, 39, 17, 8, 1], None, 1, out_ld) == every).all()
    assert (account("per row, base", x, V, next_tok, lse, mu, tau, eta, [3, 0, 9, 17, 8, 1], [4, 0, 30, 2, 2, 2], 1, out_ld) == every).all()
    # mu alone, the trace alone
    assert (account("no trace", x, V, next_tok, lse, mu, tau, eta, [7], None, 0, out_ld, trace=False) == every).all()
    assert (account("no mu", x, V, next_tok, lse, None, tau, eta, [7], None, 0, out_ld) == every).all()
    # nothing is written: a token outside 0 .. V-1, a logit that is not finite, a column outside the matrix
    bad = list(next_tok)
    bad[0], bad[2], bad[3], bad[5] = -1, V, V + 3, int(np.flatnonzero(x[5, :V] == -np.inf)[0])
    acc = account("tokens outside", x, V, bad, lse, mu, tau, eta, [7], None, 0, out_ld)
    assert acc.tolist() == [False, True, False, False, True, False]
    acc = account("columns outside", x, V, next_tok, lse, mu, tau, eta, [40, 0, 39, -1, 8, 1], [0, 0, 1, 0, -9, 38], 1, out_ld)
    assert acc.tolist() == [False, True, False, False, False, True]
    acc = account("shared column outside", x, V, next_tok, lse, mu, tau, eta, [out_ld], None, 0, out_ld)
    assert not acc.any()
    # without a trace no column is looked at
    assert (account("no trace, any column", x, V, next_tok, lse, mu, tau, eta, [out_ld + 5], None, 0, out_ld, trace=False) == every).all()
    # other temperatures
    for T in (0.5, 2.0):
        lse_t = np.array([entropy_ref._lse(x[b, :V][x[b, :V] > -np.inf] / T) for b in range(B)]).astype(np.float32)
        assert (account(f"T={T}", x, V, next_tok, lse_t, mu, tau, eta, [7], None, 0, out_ld, temperature=T) == every).all()


def test_mask_then_account_share_the_log_sum_exp():
    """the two calls as a step runs them: the mask files lse, the account reads it -- the surprise of a kept id under the
    distribution before the mask"""
    V, ld, B = 337, 344, 4
    rng = np.random.default_rng(9)
    x = draw_rows(rng, B, V, ld, [0] * B, None, min_p=0.05)
    kept, _, lse, _ = entropy_ref.mask(x, V, T_CALL, min_p=0.05)
    lg = torch.from_numpy(x).to(torch.bfloat16).cuda()
    lse_dev, mu = torch.zeros(B, device="cuda"), torch.full((B,), 6.0, device="cuda")
    ops = KC.ops()
    ops.entropy_mask(lg, V, T_CALL, min_p=0.05, lse_out=lse_dev)
    tok = torch.tensor([int(np.flatnonzero(kept[b])[-1]) for b in range(B)], dtype=torch.int32, device="cuda")
    trace = torch.full((B, 8), float("nan"), device="cuda")
    ops.entropy_account(tok, lg, V, T_CALL, lse_dev, torch.tensor([2], dtype=torch.int32, device="cuda"), mu=mu, tau=3.0, eta=0.5,
                        surprise_out=trace)
    torch.cuda.synchronize()
    want = np.array([entropy_ref.surprise(x[b, int(tok[b])], lse[b], T_CALL) for b in range(B)])
    got = trace[:, 2].cpu().to(torch.float64)
    # the account's bound (module docstring) on top of the mask's bound on lse, which enters s divided by ln 2
    z = np.array([x[b, int(tok[b])] / T_CALL for b in range(B)])
    zmax = np.array([np.abs(x[b, :V][x[b, :V] > -np.inf] / T_CALL).max() for b in range(B)])
    s_bound = (1e-5 + 2.0 ** -21 * zmax) / np.log(2) + 2.0 ** -22 * (np.abs(z) * np.log2(np.e) + np.abs(want))
    KC.check_bound("mask + account", got, torch.from_numpy(want), torch.from_numpy(s_bound), "s", seen=SEEN)
    assert torch.isnan(trace[:, :2]).all() and torch.isnan(trace[:, 3:]).all()
    mu_ref = 6.0 - 0.5 * (want - 3.0)
    KC.check_bound("mask + account", mu.cpu().to(torch.float64), torch.from_numpy(mu_ref),
                   torch.from_numpy(0.5 * s_bound + 2.0 ** -22 * 0.5 * np.abs(want - 3.0) + 2.0 ** -24 * np.abs(mu_ref)), "mu", seen=SEEN)


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_every_error_of_the_contract():
    lib, _, ptr, _ = KC.raw()
    V, ld, B, out_ld = 65, 72, 2, 8
    lg = banded(torch.zeros(B, ld), torch.bfloat16)
    mu, lse = banded(np.full(B, 4.0), torch.float32), banded(np.zeros(B), torch.float32)
    tok, tb = banded(np.zeros(B), torch.int32), banded(np.zeros((V, 3)), torch.int32)
    pos, tr = banded(np.zeros(1), torch.int32), banded(np.zeros((B, out_ld)), torch.float32)
    held = [lg, mu, lse, tok, tb, pos, tr]
    before = [KC.bits(b.t).clone() for b in held]

    def mask(**kw):
        a = dict(dict(logits=ptr(lg.t), V=V, ld=ld, t=1.0, min_p=0.1, typical_p=0.5, mu=ptr(mu.t), lse=ptr(lse.t), tok=None, table=None,
                      B=B), **kw)
        return lib.mgx_entropy_mask(a["logits"], a["V"], a["ld"], a["t"], a["min_p"], a["typical_p"], a["mu"], a["lse"], a["tok"],
                                    a["table"], a["B"], None)
    for kw in (dict(logits=None), dict(tok=ptr(tok.t)), dict(table=ptr(tb.t))):
        assert mask(**kw) == -2, kw                                           # MGX_ERR_NULL
    for kw in (dict(B=0), dict(B=-1), dict(V=0), dict(V=1025, ld=1025), dict(ld=V - 1), dict(t=0.0), dict(t=-0.5), dict(t=float("inf")),
               dict(t=float("nan")), dict(min_p=-0.01), dict(min_p=1.0), dict(min_p=float("nan")), dict(typical_p=0.0),
               dict(typical_p=-0.5), dict(typical_p=1.01), dict(typical_p=float("nan"))):
        assert mask(**kw) == -1, kw                                           # MGX_ERR_SHAPE

    def account(**kw):
        a = dict(dict(tok=ptr(tok.t), logits=ptr(lg.t), V=V, ld=ld, t=1.0, lse=ptr(lse.t), mu=ptr(mu.t), tau=3.0, eta=0.1, out=ptr(tr.t),
                      out_ld=out_ld, pos=ptr(pos.t), base=None, per_row=0, B=B), **kw)
        return lib.mgx_entropy_account(a["tok"], a["logits"], a["V"], a["ld"], a["t"], a["lse"], a["mu"], a["tau"], a["eta"], a["out"],
                                       a["out_ld"], a["pos"], a["base"], a["per_row"], a["B"], None)
    for kw in (dict(tok=None), dict(logits=None), dict(lse=None), dict(pos=None)):
        assert account(**kw) == -2, kw
    for kw in (dict(B=0), dict(V=0), dict(ld=V - 1), dict(t=0.0), dict(t=float("nan")), dict(out_ld=0), dict(out_ld=-3),
               dict(tau=float("nan")), dict(eta=float("inf"))):
        assert account(**kw) == -1, kw
    torch.cuda.synchronize()
    for b, was in zip(held, before):                                          # a refused call launches nothing
        assert torch.equal(KC.bits(b.t), was) and b.bands_intact()
    # the legal corners: everything optional NULL; the grammar given; the account without mu, without a trace
    assert mask(mu=None, lse=None, min_p=0.0, typical_p=1.0) == 0 and mask(tok=ptr(tok.t), table=ptr(tb.t)) == 0
    assert account() == 0 and account(mu=None, tau=float("nan")) == 0 and account(out=None, out_ld=0) == 0
    torch.cuda.synchronize()
    assert all(b.bands_intact() for b in held)
    ops = KC.ops()
    with pytest.raises(ValueError, match="together"):
        ops.entropy_mask(lg.t, V, 1.0, min_p=0.1, tok=tok.t)
    with pytest.raises(ValueError, match="bf16"):
        ops.entropy_mask(lg.t.float(), V, 1.0, min_p=0.1)
    with pytest.raises(ValueError, match="mu"):
        ops.entropy_mask(lg.t, V, 1.0, mu=mu.t[:1])
    with pytest.raises(ValueError, match="lse_out"):
        ops.entropy_mask(lg.t, V, 1.0, lse_out=lse.t.double())
    with pytest.raises(Exception, match="min_p must lie"):                    # the library's own refusal, through the wrapper
        ops.entropy_mask(lg.t, V, 1.0, min_p=1.0)
    with pytest.raises(Exception, match="CUDA/HIP"):
        ops.entropy_mask(lg.t, V, 1.0, mu=mu.t.cpu())
    with pytest.raises(ValueError, match="next_tok"):
        ops.entropy_account(tok.t.long(), lg.t, V, 1.0, lse.t, pos.t)
    with pytest.raises(ValueError, match="lse"):
        ops.entropy_account(tok.t, lg.t, V, 1.0, lse.t[:1], pos.t)
    with pytest.raises(ValueError, match="surprise_out"):
        ops.entropy_account(tok.t, lg.t, V, 1.0, lse.t, pos.t, surprise_out=tr.t.view(-1))
    with pytest.raises(ValueError, match="positions|position"):
        ops.entropy_account(tok.t, lg.t, V, 1.0, lse.t, pos.t, ragged=True)
