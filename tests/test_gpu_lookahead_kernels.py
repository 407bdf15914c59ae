"""The three kernels of draft-and-verify decode (ABI 32), each against its header contract.

Draft.  Integers in, integers out: bit-equal to tests/lookahead_ref.py; inputs and guard bands intact.

Attention.  mgx_rel_attn_decode_multi per element against the fp64 reference of its formula (oracle/decode_ref.py, query i of row b
at position t_b + i over the row's cache rows below t_b and the new rows 0..i), with the check and the constant of
tests/test_gpu_decode_kernels.py for mgx_rel_attn_decode: |ctx - ref| <= 2^-8 |ref| + C_ATTN * F, F the fp32 noise floor of the
formula, C_ATTN = 16.  The cache rows at and above t_b are NaN before the call (the kernel reads the new rows from qkv_new, never
from the cache) and hold exactly the new rows after it; everything else, guard bands included, is bit for bit what it was.  The
causal bound is checked by poison: with large values in the K / V of the new rows >= c and in the cache from t_b on, the ctx of
the queries below c must not change by a bit.

Accept.  The draws must equal mgx_sample_topk_topp's on the same logits, row by row (one call per i on the strided view, same seed,
step and row0); everything else must equal tests/lookahead_ref.py on those draws."""
import numpy as np
import pytest
import torch

import kernel_checks as KC
import lookahead_ref as LR
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)
from oracle import decode_ref as D

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
NAN16 = 0x7FC0
PAD = 336
C_ATTN = 16.0                                       # tests/test_gpu_decode_kernels.py: the constant of mgx_rel_attn_decode
SEEN = {}
_report = KC.report_fixture(SEEN, "largest (|ctx - ref| - 2^-8 |ref|) / F {:.3f}")


def banded(a, dtype=torch.int32):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return KC.Banded(t.to(dtype), KC.BAND, KC.PATTERN)


# =====================================================================================================================
# 1. the draft
# =====================================================================================================================
def run_draft(hist, pos, T, Lmax, case, ngram=3, guide=None, base=None):
    hist = np.asarray(hist, dtype=np.int32)
    B, out_ld = hist.shape
    pos = np.asarray(pos, dtype=np.int32)
    s = pos + (0 if base is None else np.asarray(base, dtype=np.int32))
    tok = np.array([hist[b, s[b]] if 0 <= s[b] < out_ld else 5 for b in range(B)], dtype=np.int32)
    h, p, tk = banded(hist), banded(pos), banded(tok)
    bs = None if base is None else banded(base)
    g = None if guide is None else banded(guide)
    draft, rows = KC.output((B, T), torch.int32), KC.output((B * T,), torch.int32)
    KC.ops().lookahead_draft(tk.t, h.t, p.t, draft.t, rows.t, Lmax, PAD, guide=None if g is None else g.t, ngram=ngram,
                             base=None if bs is None else bs.t)
    torch.cuda.synchronize()
    want = [LR.draft_row(hist[b].tolist(), int(s[b]), int(tok[b]), T, PAD, ngram, None if guide is None else np.asarray(guide)[b].tolist())
            for b in range(B)]
    KC.check_equal("draft", draft.t, torch.tensor(want, dtype=torch.float64), case)
    KC.check_equal("pos_rows", rows.t, torch.tensor([v for b in range(B) for v in LR.pos_rows(int(pos[b]), T, Lmax)],
                                                    dtype=torch.float64), case)
    for b_ in (h, p, tk, bs, g, draft, rows):
        assert b_ is None or b_.bands_intact(), case
    assert (h.t.cpu().numpy() == hist).all() and (p.t.cpu().numpy() == pos).all() and (tk.t.cpu().numpy() == tok).all(), case
    return want


def _row(vals, out_ld=48):
    """the history columns ``vals``, then filler that no id equals (columns above s are never read: distinct junk shows a read)"""
    return list(vals) + [1000 + c for c in range(out_ld - len(vals))]


@pytest.mark.parametrize("T", [2, 8])
def test_draft_named_cases(T):
    rows = [
        ([5], "s = 0"),
        ([1, 2, 3, 4], "no match"),
        ([3, 8, 5, 6, 8], "a match only at n = 1"),
        ([7, 1, 2, 9, 8, 1, 2, 4, 1, 2], "two matches, the later wins"),
        ([4, 6, 6], "a match ending at s - 1: period 1"),
        ([1, 2, 1, 2], "a period shorter than T"),
        ([9, 1, 2, 5, 0, 0, 1, 2, 6, 9, 1, 2], "the longer suffix beats the later shorter one"),
    ]
    hist = [_row(v) for v, _ in rows]
    pos = [len(v) - 1 for v, _ in rows]
    want = run_draft(hist, pos, T, 96, f"named T={T}")
    assert want[0][1:] == [PAD] * (T - 1) and want[1][1:] == [PAD] * (T - 1)
    assert want[2][:2] == [8, 5] and want[3][:2] == [2, 4] and want[4] == [6] * T
    assert want[5] == ([2, 1] * T)[:T] and want[6][:2] == [2, 5]
    # the same rows with a window's base: s = base + t
    run_draft(hist, [pos[0]] + [p_ - 1 for p_ in pos[1:]], T, 96, f"named with base T={T}", base=[0] + [1] * 6)


@pytest.mark.parametrize("T, ngram", [(2, 1), (3, 2), (4, 3), (8, 8)])
def test_draft_random_histories_over_a_small_alphabet(T, ngram):
    """four ids, so every n finds matches somewhere; columns 0, 1, n - 1, n, one past a workgroup's 256 threads, the last"""
    out_ld = 600
    rng = np.random.default_rng(100 * T + ngram)
    cols = sorted({0, 1, ngram - 1, ngram, 17, 255, 256, 257, 513, out_ld - 1})
    hist = rng.integers(0, 4, (len(cols), out_ld)).astype(np.int32)
    for c in range(300, out_ld):                                                      # one row periodic with period 10 at its end
        hist[0, c] = hist[0, c - 10]
    run_draft(hist, cols, T, 580, f"random T={T} ngram={ngram}", ngram=ngram)         # Lmax 580: the last rows' pos_rows clamp
    run_draft(hist, [out_ld - 1] * len(cols), T, out_ld, f"random at the last column T={T} ngram={ngram}", ngram=ngram)


@pytest.mark.parametrize("T", [2, 8])
def test_draft_from_a_guide_and_clamped_positions(T):
    out_ld, B = 40, 4
    rng = np.random.default_rng(T)
    hist = rng.integers(0, 300, (B, out_ld)).astype(np.int32)
    guide = rng.integers(0, 300, (B, 30)).astype(np.int32)                            # shorter than the rows: pads beyond column 29
    want = run_draft(hist, [0, 29 - T, 28, 35], T, 36, f"guide T={T}", guide=guide)
    assert want[2][1:] == [int(guide[2, 29])] + [PAD] * (T - 2) and want[3][1:] == [PAD] * (T - 1)
    assert want[0][1:] == guide[0, 1:T].tolist()


# =====================================================================================================================
# 2. the attention of T consecutive queries
# =====================================================================================================================
class MultiData:
    """caches, the B * T new rows and E of one configuration, on the device and (the same values) on the CPU"""

    def __init__(self, B, d, Lmax, extra, T, seed=0):
        self.B, self.d, self.Lmax, self.T, self.h, self.M = B, d, Lmax, T, d // 64, Lmax + extra
        g = torch.Generator(device=DEV).manual_seed(1000 * seed + Lmax + 10 * T + d)
        rn = lambda *s: torch.randn(*s, device=DEV, generator=g)                                    # noqa: E731
        self.kc = (rn(B, self.h, Lmax, 64) * torch.exp(0.5 * rn(B, self.h, Lmax, 1))).to(BF)       # rows of different magnitude
        self.vc = (rn(B, self.h, Lmax, 64) * torch.exp(0.5 * rn(B, self.h, Lmax, 1))).to(BF)
        self.qkv = rn(B * T, 3 * d).to(BF)
        self.E = (0.3 * rn(self.M, 64)).to(BF)
        self.kc_cpu, self.vc_cpu, self.qkv_cpu, self.E_cpu = (t.cpu() for t in (self.kc, self.vc, self.qkv, self.E))
        ops = KC.ops()
        self.nsplit = ops.rel_attn_decode_multi_splits(B, T, Lmax, d)
        assert self.nsplit == ops.rel_attn_decode_splits(B, Lmax, d)
        self.ws = ops.rel_attn_decode_multi_workspace(B, T, Lmax, d, DEV)
        assert (self.ws is None) == (self.nsplit == 1)

    def new_rows(self, qkv, part):
        """k (part 1) or v (part 2) of the new rows as the cache holds them: [B, T, h, 64]"""
        return qkv[:, part * self.d:(part + 1) * self.d].reshape(self.B, self.T, self.h, 64)

    def run(self, ts, qkv=None, poison="nan", case=""):
        """one call; checks what it wrote and what it left alone; -> ctx bf16 [B, T, h, 64] on the CPU"""
        B, T, h, Lmax, d = self.B, self.T, self.h, self.Lmax, self.d
        qkv = self.qkv if qkv is None else qkv
        t_rows = torch.tensor(ts, device=DEV)
        stale = (torch.arange(Lmax, device=DEV)[None] >= t_rows[:, None])[:, None, :, None]           # rows >= t_b
        caches, wants = [], []
        for cache, part in ((self.kc, 1), (self.vc, 2)):
            if poison == "nan":
                c = cache.view(torch.int16).masked_fill(stale, NAN16).view(BF)
            else:                                                                                  # large values, no NaN
                c = torch.where(stale, torch.full_like(cache, 3.0e4 if part == 2 else 60.0), cache)
            want = c.clone()
            new = self.new_rows(qkv, part)
            for b in range(B):
                for i in range(T):
                    if ts[b] + i < Lmax:
                        want[b, :, ts[b] + i] = new[b, i]
            caches.append(KC.Banded(c.cpu(), KC.BAND, KC.PATTERN))
            wants.append(want.view(torch.int16).cpu())
        E = self.E.clone()
        E.view(torch.int16)[:self.M - 1 - min(max(ts) + T - 1, Lmax - 1)] = NAN16                    # rows no key of this call maps to
        if self.ws is not None:
            self.ws.fill_(0xFF)                                                                    # every stale partial is NaN
        ctx = KC.output((B * T, d), BF)
        pos = KC.Banded(t_rows.to(torch.int32).cpu(), KC.BAND, KC.PATTERN)
        KC.ops().rel_attn_decode_multi(qkv, caches[0].t, caches[1].t, E, pos.t, ctx.t, self.ws, T)
        torch.cuda.synchronize()
        for c, want in zip(caches, wants):
            assert torch.equal(c.t.view(torch.int16).cpu(), want), (case, "the cache holds exactly the new rows")
            assert c.bands_intact(), case
        assert ctx.bands_intact() and pos.bands_intact() and pos.t.cpu().tolist() == list(ts), case
        out = ctx.t.float().cpu()
        assert torch.isfinite(out).all(), (case, "non-finite ctx")
        return out.reshape(B, T, h, 64)

    def check(self, ts, fam):
        B, T, h, d, Lmax = self.B, self.T, self.h, self.d, self.Lmax
        case = f"B={B} d={d} Lmax={Lmax} T={T} splits={self.nsplit} t={list(ts)}"
        ctx = self.run(ts, case=case).double()
        q = self.qkv_cpu[:, :d].reshape(B, T, h, 64)
        nk, nv = self.new_rows(self.qkv_cpu, 1), self.new_rows(self.qkv_cpu, 2)
        for b in range(B):
            t = ts[b]
            for i in range(T):
                if t + i >= Lmax:
                    continue                                                                       # unspecified but finite (checked)
                K = torch.cat([self.kc_cpu[b, :, :t].double(), nk[b, :i + 1].permute(1, 0, 2).double()], 1)
                V = torch.cat([self.vc_cpu[b, :, :t].double(), nv[b, :i + 1].permute(1, 0, 2).double()], 1)
                ref = D.rel_attn_decode(q[b, i], K, V, self.E_cpu, t + i)
                F = D.attn_noise_floor(q[b, i], K, V, self.E_cpu, t + i, ref)[:, None]
                # one key (t + i = 0): ctx is v itself in every evaluation and F is 0 -- the bound is then the rounding alone
                KC.check_floor(fam, ctx[b, i], ref, F.clamp(min=1e-30).expand_as(ref), f"{case} b={b} i={i}", C=C_ATTN, seen=SEEN,
                               rounding=2.0 ** -8)


@pytest.mark.parametrize("T", [2, 3, 8])
@pytest.mark.parametrize("d", [64, 128])
def test_attention_against_fp64_at_the_edges(d, T):
    """B = 3 rows at different positions: the first slots of the first wave, the 64-key stride, the last positions of the cache --
    t = Lmax - T (every query in range) and t = Lmax - 1 (only query 0 is)"""
    Lmax = 96
    data = MultiData(3, d, Lmax, 16, T)
    assert data.nsplit == 1
    for ts in ([0, 8, 63], [1, 62, Lmax - T], [7, 64, Lmax - 1]):
        data.check(ts, "multi")


def test_attention_on_the_split_key_path():
    """a long cache, two key splits: positions whose new rows lie on both sides of a share boundary (t = 60, T = 8: keys 64..67,
    the new rows 4..7, are the second split's), a split that is empty for the first queries, and long rows"""
    T = 8
    data = MultiData(3, 64, 1500, 16, T)
    assert data.nsplit == 2
    for ts in ([60, 56, 1400], [63, 64, 1500 - T], [0, 1023, 1499]):
        data.check(ts, "multi [splits]")


@pytest.mark.parametrize("T, Lmax, B, d", [(8, 96, 3, 128), (3, 96, 3, 64), (8, 1500, 3, 64)])
def test_no_query_sees_a_row_above_its_own(T, Lmax, B, d):
    """large values in K / V of the new rows >= c, and in the cache from t on: the queries below c give the same bits"""
    data = MultiData(B, d, Lmax, 16, T, seed=3)
    ts = [5, 63, 70] if Lmax == 96 else [60, 700, 1400]
    base = data.run(ts, case="clean")
    for c in range(1, T):
        qkv = data.qkv.clone().view(B, T, 3 * d)
        qkv[:, c:, d:2 * d] = 60.0 * torch.sign(qkv[:, c:, :d])                                    # a key every query scores high
        qkv[:, c:, 2 * d:] = 3.0e4
        got = data.run(ts, qkv=qkv.view(B * T, 3 * d), poison="large", case=f"poison from {c}")
        KC.check_equal("causal", got[:, :c], base[:, :c].double(), f"T={T} Lmax={Lmax} rows >= {c} poisoned")
        assert not torch.equal(got[:, c:], base[:, c:])                                            # the poison is one: it shows above


# =====================================================================================================================
# 3. the accept
# =====================================================================================================================
def grammar_table(V, rng):
    tab = rng.integers(0, 2 ** 32, (V, (V + 31) // 32), dtype=np.uint64).astype(np.uint32)
    tab[7] = 0                                                                                     # a row that allows nothing is ignored
    return tab


def sampler_draws(logits, V, T, pos, base, draft, seed, row0, table, **kp):
    """mgx_sample_topk_topp once per i on the strided view of logits [B * T, ld]: -> (ys [B, T], probs [B, T, V])"""
    lib, check, ptr, stream_ptr = KC.raw()
    B, ld = draft.shape[0], logits.shape[1]
    ys = torch.zeros(B, T, dtype=torch.int32, device=DEV)
    probs = torch.zeros(B, T, V, dtype=torch.float32, device=DEV)
    for i in range(T):
        nxt = draft[:, i].contiguous()                                                             # the grammar's previous token
        p_i = torch.zeros(B, V, dtype=torch.float32, device=DEV)
        pos_i = (pos + i).contiguous()
        check(lib.mgx_sample_topk_topp(logits.data_ptr() + 2 * i * ld, V, T * ld, kp.get("temperature", 1.0), kp.get("top_k", 0),
                                       kp.get("top_p", 1.0), seed, ptr(pos_i), ptr(base), 1, ptr(nxt), None, 0, ptr(p_i), B, row0, 0,
                                       ptr(table), stream_ptr()), "mgx_sample_topk_topp")
        ys[:, i], probs[:, i] = nxt, p_i
    torch.cuda.synchronize()
    return ys.cpu(), probs.cpu()


def run_accept(logits, V, pos, draft, limit, out_ld, case, seed=11, row0=0, table=None, base=None, **kp):
    B, T = draft.shape
    logits = logits.to(DEV)
    d_pos, d_draft, d_lim = banded(pos), banded(draft), banded(limit)
    d_base = None if base is None else banded(base)
    tab = None if table is None else torch.from_numpy(table.view(np.int32)).to(DEV)
    ys, probs = sampler_draws(logits, V, T, d_pos.t.clone(), None if d_base is None else d_base.t, d_draft.t, seed, row0, tab, **kp)
    tok0 = draft[:, 0].copy()
    out0 = np.full((B, out_ld), -3, dtype=np.int32)
    d_tok, d_out = banded(tok0), banded(out0)
    d_done, d_stats = banded(np.zeros(B, dtype=np.int32)), banded(np.tile(np.array([[2, 5]], dtype=np.int32), (B, 1)))
    d_probs = KC.Banded(torch.full((B, out_ld, V), -1.0), KC.BAND, KC.PATTERN)
    KC.ops().lookahead_accept(logits, V, d_pos.t, d_draft.t, d_lim.t, d_tok.t, d_out.t, d_done.t, probs_all=d_probs.t, stats=d_stats.t,
                              seed=seed, allow_table=tab, row0=row0, base=None if d_base is None else d_base.t, **kp)
    torch.cuda.synchronize()
    out, tok, p, done, stats = out0.tolist(), tok0.tolist(), list(map(int, pos)), [0] * B, [[2, 5] for _ in range(B)]
    s0 = [int(pos[b]) + (0 if base is None else int(base[b])) for b in range(B)]
    LR.accept(out, tok, p, draft.tolist(), ys.tolist(), list(map(int, limit)), done, stats, None if base is None else list(map(int, base)))
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)                                            # noqa: E731
    KC.check_equal("accept out_tokens", d_out.t, f64(out), case)
    KC.check_equal("accept tok", d_tok.t, f64(tok), case)
    KC.check_equal("accept pos", d_pos.t, f64(p), case)
    KC.check_equal("accept done", d_done.t, f64(done), case)
    KC.check_equal("accept stats", d_stats.t, f64(stats), case)
    want_p = torch.full((B, out_ld, V), -1.0)
    ns = []
    for b in range(B):
        n = p[b] - int(pos[b])
        ns.append(n)
        for i in range(n):
            want_p[b, s0[b] + i] = probs[b, i]
    KC.check_equal("accept probs_all", KC.bits(d_probs.t), KC.bits(want_p).to(torch.float64), case)
    for b_ in (d_pos, d_draft, d_lim, d_base, d_tok, d_out, d_done, d_stats, d_probs):
        assert b_ is None or b_.bands_intact(), case
    assert (d_draft.t.cpu().numpy() == draft).all() and (d_lim.t.cpu().numpy() == limit).all(), case
    return ys.tolist(), ns, done


@pytest.mark.parametrize("kp", [dict(), dict(top_k=20, top_p=0.9, temperature=0.8)], ids=["plain", "top-k top-p"])
@pytest.mark.parametrize("T", [2, 4, 8])
def test_accept_with_certain_draws_hits_exactly_as_often_as_drafted(T, kp):
    """peaked logits: position i draws peak[b, i] whatever the random number.  Rows whose drafts hit 0, 1, T - 2 and T - 1 times,
    a row whose limit cuts an all-correct draft, a row already at its limit; under a grammar table whose row of draft[b, i]
    allows the peak"""
    V, ld, out_ld = 337, 384, 64
    rng = np.random.default_rng(T)
    table = grammar_table(V, rng)
    hits = sorted({0, 1, T - 2, T - 1}) + [T - 1, T - 1]
    B = len(hits)
    allowed = lambda prev: np.flatnonzero((table[prev][np.arange(V) >> 5] >> (np.arange(V) & 31).astype(np.uint32)) & 1)   # noqa: E731
    draft, peak = np.zeros((B, T), dtype=np.int32), np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        draft[b, 0] = 20 + b
        for i in range(T):
            ok = allowed(draft[b, i])
            ok = ok[(ok != PAD) & (ok != 7)]
            peak[b, i] = rng.choice(ok)
            if i + 1 < T:
                draft[b, i + 1] = peak[b, i] if i < hits[b] else (peak[b, i] + 1 + rng.integers(0, 300)) % V     # a miss: never the peak
    x = torch.from_numpy(rng.normal(size=(B * T, ld))).float() - 30.0
    x[torch.arange(B * T), torch.from_numpy(peak.reshape(-1)).long()] = 30.0
    x[:, V:] = float("nan")
    pos = np.array([3, 10, 17, 30, 40, 50][:B] + [50] * (B - 6), dtype=np.int32)[:B]
    limit = np.full(B, 62, dtype=np.int32)
    limit[B - 2] = pos[B - 2] + max(1, T - 2)                                          # cuts the all-correct draft of T
    limit[B - 1] = pos[B - 1]                                                          # already at its limit
    ys, ns, done = run_accept(x.to(BF), V, pos, draft, limit, out_ld, f"certain T={T} {kp}", table=table, **kp)
    assert ys == peak.tolist()                                                         # the draws were certain
    assert ns[:B - 2] == [h + 1 for h in hits[:B - 2]] and ns[B - 2] == max(1, T - 2) and ns[B - 1] == 0
    assert done == [0] * (B - 1) + [1]


@pytest.mark.parametrize("T, V", [(2, 64), (4, 337), (8, 1024)])
def test_accept_on_random_logits_with_a_base_and_row0(T, V):
    """draws that depend on the random number: whatever the sampler draws, the accept draws; drafts over a few ids so that some
    guesses hit by chance, more with top_k = 2"""
    ld, out_ld, B = (V + 63) // 64 * 64, 48, 7
    rng = np.random.default_rng(V + T)
    x = torch.from_numpy(rng.normal(size=(B * T, ld)) * 3.0).float()
    x[:, :V][torch.from_numpy(rng.random((B * T, V)) < 0.05)] = float("-inf")
    x[:, 3] = 14.0                                                                     # ids 3 and 5 carry most of the mass
    x[:, 5] = 13.5
    x[:, V:] = float("nan")
    draft = rng.choice([3, 5], (B, T)).astype(np.int32)
    pos = rng.integers(0, 20, B).astype(np.int32)
    base = rng.integers(0, 6, B).astype(np.int32)
    limit = (pos + base + rng.integers(0, 2 * T, B)).astype(np.int32)
    table = grammar_table(V, rng) if V > 64 else None
    if table is not None:
        table[[3, 5], 0] |= np.uint32((1 << 3) | (1 << 5))                             # the two may follow each other
    total = 0
    for kp in (dict(), dict(top_k=2), dict(top_p=0.7, temperature=1.3)):
        _, ns, _ = run_accept(x.to(BF), V, pos, draft, limit, out_ld, f"random T={T} V={V} {kp}", seed=2 ** 40 + 17, row0=5, table=table,
                              base=base, **kp)
        total += sum(n > 1 for n in ns)
    assert total > 0                                                                   # some step accepted more than one token
