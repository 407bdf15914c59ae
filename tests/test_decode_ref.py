"""oracle/decode_ref.py (the fp64 references of one decode step) against what is already pinned to the reference project's
goldens through oracle/ref_cpu.py, and against independent restatements.  No GPU."""
import math

import numpy as np
import torch

from oracle import decode_ref as D
from oracle import ref_cpu as R


def test_attention_at_position_t_is_row_t_of_the_causal_full_sequence_attention():
    g = torch.Generator().manual_seed(0)
    B, L, d, h = 2, 96, 128, 2
    M = L + 8
    qkv = torch.randn(B, L, 3 * d, generator=g)
    E = 0.3 * torch.randn(M, 64, generator=g)
    x = torch.zeros(B, L, dtype=torch.long)
    ctx, _, _ = R.attn_core(qkv, E, R.look_ahead_mask(x, pad=-1), h)          # fp32, materialised L x L
    heads = lambda c: qkv[..., c * d:(c + 1) * d].reshape(B, L, h, 64).permute(0, 2, 1, 3)      # noqa: E731
    q, K, V = heads(0), heads(1), heads(2)
    for t in (0, 1, 31, 32, 63, 64, L - 2, L - 1):
        ref = D.rel_attn_decode(q[:, :, t], K, V, E, t)                       # [B, h, 64]
        want = ctx[:, t].reshape(B, h, 64).double()
        assert (ref - want).abs().max().item() <= 32 * 2 ** -24 * max(1.0, want.abs().max().item()), t
        one = D.rel_attn_decode(q[1, 0, t], K[1, 0], V[1, 0], E, t)           # a single (b, head)
        assert (one - ref[1, 0]).abs().max().item() <= 1e-13
        # the differently ordered fp32 evaluation stays at fp32 distance, and it is not the fp64 value
        F = D.attn_noise_floor(q[:, :, t], K, V, E, t, ref)
        assert F.shape == (B, h) and F.max().item() <= 2 ** -18
    assert D.attn_noise_floor(q[:, :, L - 1], K, V, E, L - 1, D.rel_attn_decode(q[:, :, L - 1], K, V, E, L - 1)).min() > 0


def test_attention_ignores_keys_after_t_and_unused_rows_of_E():
    g = torch.Generator().manual_seed(1)
    L, M, t = 40, 56, 17
    q, K, V, E = torch.randn(64, generator=g), torch.randn(L, 64, generator=g), torch.randn(L, 64, generator=g), \
        torch.randn(M, 64, generator=g)
    ref = D.rel_attn_decode(q, K, V, E, t)
    K2, V2, E2 = K.clone(), V.clone(), E.clone()
    K2[t + 1:], V2[t + 1:], E2[:M - 1 - t] = float("nan"), float("nan"), float("nan")
    assert torch.equal(D.rel_attn_decode(q, K2, V2, E2, t), ref)
    assert torch.equal(D.rel_attn_decode(torch.zeros(64), K, V, E, t), V[:t + 1].double().mean(0))


def test_embed_is_the_first_stage_of_the_model():
    V, d, nl, L, B = 50, 128, 1, 32, 3
    p = R.init_params(V, d, nl, L, seed=3)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, V - 1, (B, L), generator=g)
    table = p["Decoder.embedding.weight"]
    pe = R.sinusoid_table(L, d).to(torch.float32)
    want = table[x] * math.sqrt(d) + pe[None]                                 # decoder_stack's first two lines
    got = D.embed(x.reshape(-1), table, pe, torch.arange(L).repeat(B)).reshape(B, L, d)
    assert (got - want.double()).abs().max().item() <= 2 ** -22 * want.abs().max().item()
    one = D.embed(x[:, 5], table, pe, 5)                                      # one shared position
    assert torch.equal(one, got[:, 5])
    # and the model's first stage really is that: a one-layer stack run on it gives model_forward's result
    h0, _ = R.decoder_stack(p, x, R.look_ahead_mask(x, V - 1))
    mask = R.look_ahead_mask(x, V - 1)
    h1, _ = R.encoder_layer(p, "Decoder.enc_layers.0.", got.float(), mask, d // 64, 0.0, False)
    assert (h0 - h1).abs().max().item() <= 1e-4


def test_linear_and_add_ln_against_torch():
    g = torch.Generator().manual_seed(4)
    a = torch.randn(5, 64, generator=g).to(torch.bfloat16)
    w = torch.randn(12, 64, generator=g).to(torch.bfloat16)
    b = torch.randn(12, generator=g)
    c, S = D.linear(a, w, b, act=1)
    want = torch.relu(torch.nn.functional.linear(a.double(), w.double(), b.double()))
    assert torch.equal(c, want) and (S >= (c - torch.relu(b.double())).abs() - 1e-12).all()
    assert torch.equal(S, a.double().abs() @ w.double().abs().T)
    x, r = torch.randn(5, 64, generator=g) + 30.0, 0.1 * torch.randn(5, 64, generator=g)
    gam, bet = torch.randn(64, generator=g), torch.randn(64, generator=g)
    want = torch.nn.functional.layer_norm(x.double() + r.double(), (64,), gam.double(), bet.double(), 1e-6)
    assert (D.add_ln(x, r, gam, bet) - want).abs().max().item() <= 1e-9
    const = D.add_ln(torch.full((1, 64), 3.0), torch.zeros(1, 64), gam, bet)
    assert torch.equal(const, bet.double()[None])


def _sort_and_cumsum(p, top_k, top_p):
    """the usual implementation: sort descending, cut at k, cut at the first prefix whose mass reaches top_p * the rest"""
    order = np.argsort(-p, kind="stable")
    n = len(p) if not 0 < top_k < len(p) else top_k
    order = order[:n]
    if top_p < 1:
        cs = np.cumsum(p[order])
        order = order[:int(np.argmax(cs >= top_p * cs[-1])) + 1]
    keep = np.zeros(len(p), dtype=bool)
    keep[order] = True
    return keep


def test_kept_set_equals_sort_and_cumsum_without_ties_and_keeps_ties_together():
    rng = np.random.default_rng(5)
    cases = [(0, 1.0), (1, 1.0), (5, 1.0), (0, 0.9), (0, 1e-6), (40, 0.9), (3, 0.5), (69, 1.0), (70, 1.0), (77, 1.0)]
    p = D.softmax_probs(torch.tensor(2 * rng.normal(size=(64, 70))), 1.0)
    assert all(len(np.unique(r)) == 70 for r in p)
    for k, tp in cases:
        rows, _ = D.kept_set_rows(p, k, tp)
        for i, r in enumerate(p):
            keep = D.kept_set(r, k, tp)
            assert (keep == _sort_and_cumsum(r, k, tp)).all(), (k, tp, i)
            assert (keep == rows[i]).all()
            assert any((keep == a).all() for a in D.kept_set_alternatives(r, k, tp, 0.0, 0.0))
    # ties: the values ranked 4..7 are equal
    x = torch.tensor(2 * rng.normal(size=(32, 70))).to(torch.bfloat16).float()
    srt = x.float().sort(-1, descending=True)
    for i in range(32):
        x[i, srt.indices[i, 3:7]] = x[i, srt.indices[i, 3]].item()
    p = D.softmax_probs(x, 0.5)
    for k, tp in ((5, 1.0), (4, 1.0), (6, 1.0), (0, 0.5), (5, 0.7)):
        rows, _ = D.kept_set_rows(p, k, tp)
        for i, r in enumerate(p):
            keep = D.kept_set(r, k, tp)
            assert (keep == rows[i]).all()
            tied = r == r[srt.indices[i, 3]]
            assert tied.sum() >= 4 and (keep[tied].all() or not keep[tied].any()), (k, tp, i)
            if tp == 1.0:
                assert keep.sum() == 7 and keep[tied].all()               # more than top_k: the tie is kept whole
            # monotone: everything kept is at least as likely as everything dropped
            assert r[keep].min() > r[~keep].max()
    # top_k larger than the ids of non-zero probability, and -inf logits
    x = torch.full((1, 70), float("-inf"))
    x[0, [3, 9, 50]] = torch.tensor([0.0, 1.0, -1.0])
    p = D.softmax_probs(x, 1.7)
    assert abs(p.sum() - 1) < 1e-15 and (p[0] > 0).sum() == 3
    assert D.kept_set(p[0], 10, 1.0).nonzero()[0].tolist() == [3, 9, 50]
    assert D.kept_set(p[0], 2, 1.0).nonzero()[0].tolist() == [3, 9]
    assert D.kept_set_rows(p, 10, 0.99)[0][0].nonzero()[0].tolist() == [3, 9, 50]


def test_softmax_with_a_grammar_row_and_the_empty_row_fallback():
    V = 40
    tab = np.zeros((V, 2), dtype=np.uint32)
    tab[0, 0], tab[1, 1], tab[2, 0] = 0b1010, 1 << (35 - 32), 1 << 7      # row 0: {1, 3}; row 1: {35}; row 2: {7}; row 3: {}
    allowed = D.allowed_mask(tab, [0, 1, 2, 3, -5, 99], V)
    assert allowed[0].nonzero()[0].tolist() == [1, 3] and allowed[1].nonzero()[0].tolist() == [35]
    assert allowed[4].nonzero()[0].tolist() == [1, 3] and not allowed[5].any()       # prev clamped to 0 / V-1
    x = torch.randn(6, V, generator=torch.Generator().manual_seed(6))
    x[2, 7] = float("-inf")                                                # the only allowed id of row 2 has no mass
    p = D.softmax_probs(x, 0.5, allowed)
    free = D.softmax_probs(x, 0.5)
    assert (p[0] > 0).nonzero()[0].tolist() == [1, 3] and p[1, 35] == 1.0
    e = np.exp(2 * x[0, [1, 3]].double().numpy())
    assert np.allclose(p[0, [1, 3]], e / e.sum(), rtol=1e-14)
    for row in (2, 3, 5):                                                  # nothing finite left: the unmasked distribution
        assert (p[row] == free[row]).all()


def test_u01_is_a_uniform_pure_function_of_seed_step_row():
    rows = np.arange(100000)
    u = D.u01(0x123456789ABCDEF, 7, rows)
    assert u.min() > 0 and u.max() < 1
    n = D.u01_bits(0x123456789ABCDEF, 7, rows)
    assert n.max() < 2 ** 24 and (u == u.astype(np.float32)).all()
    exact = (n.astype(np.float64) + 0.5) / 2 ** 24                         # n + 0.5 itself; fp32 holds it below 2^23
    assert (u[n < 2 ** 23] == exact[n < 2 ** 23]).all() and np.abs(u - exact).max() == 2.0 ** -25
    assert abs(u.mean() - 0.5) <= 4 * math.sqrt(1 / 12 / len(rows))
    assert abs((u < 0.25).mean() - 0.25) <= 4 * math.sqrt(0.25 * 0.75 / len(rows))
    base = D.u01_bits(0x1234567889ABCDEF, 7, rows[:1000])
    for seed, step, row in ((0x1234567889ABCDEE, 7, 0), (0x1234567989ABCDEF, 7, 0), (0x1234567889ABCDEF, 8, 0),
                            (0x1234567889ABCDEF, 7, 1)):
        other = D.u01_bits(seed, step, rows[:1000] + row)
        assert (other != base).mean() > 0.99, (hex(seed), step, row)
    # the vectorised twin against plain Python integers (no silent wrap-around in the 64-bit numpy arithmetic)
    def h(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = x * 0x7FEB352D & 0xFFFFFFFF
        x ^= x >> 15
        x = x * 0x846CA68B & 0xFFFFFFFF
        return x ^ x >> 16
    for seed, step, row in ((0, 0, 0), (0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0x1234567889ABCDEF, 8191, 511)):
        x = h((seed & 0xFFFFFFFF) ^ h(step * 0x9E3779B9 + 0x7F4A7C15) ^ h(row + 0x85EBCA6B) ^ h((seed >> 32) + 0xC2B2AE35))
        assert int(D.u01_bits(seed, step, row)) == x >> 8
    assert D.u01(5, 3, 2) == D.u01(5, np.array([3]), np.array([2]))[0]


def test_draw_takes_the_first_id_whose_cdf_reaches_u():
    p = np.array([0.0, 0.2, 0.0, 0.3, 0.5, 0.0])
    assert [D.draw(p, u) for u in (1e-9, 0.2, 0.2 + 1e-9, 0.5, 0.5 + 1e-9, 1 - 1e-9)] == [1, 1, 3, 3, 4, 4]
    assert D.draw(p * 0.5, 0.3) == 3                                       # relative to the kept mass
    assert D.draw(np.array([0.0, 1.0, 0.0]), 0.999999) == 1
