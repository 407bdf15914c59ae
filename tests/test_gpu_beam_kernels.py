"""The three beam-search kernels (ABI 22), each against the fp64 / numpy reference of its header contract (tests/beam_ref.py).

Select.  Per case the kernel's tok / parent / history columns / positions must be mutually consistent and nothing else may be
written; a written score is compared with the REFERENCE candidate of the (parent, token) the kernel chose:
|score - ref| <= R_SEL * max(1, |ref|).  MEASURED on one MI355X over all select cases of this module: the largest ratio was
2.688e-7 = 2.26 * 2^-23 (V = 1024, sixteen beams with scores down to -30); R_SEL = 2^-20 is twice that, rounded up to a power of two.
The chosen set must be the reference's top-K set, except that a candidate may change sides where its reference key lies within
BAND = 2 * R_SEL * max(1, |key|) of the reference's K-th key; the stochastic cases add G_ERR to the band, the fp32 error of
g = -log(-log u).  The kernel never writes g, so its error cannot be read off the device; what is measured instead is the same
formula evaluated in fp32 by numpy from the same u (exact in fp32) against the fp64 one, over EVERY stochastic case of this
module: 5.56e-7 at most (half an ulp of g near 8..11 plus what the inner logarithm hands on).  numpy's logf and the device's are
both good to about an ulp, so either's distance from fp64 is of this size, and G_ERR = 2^-19 is twice the measured figure,
rounded up to a power of two (test_select asserts that the figure of its own cases stays within G_ERR / 2).
A (case, prompt) pair is AMBIGUOUS when the reference's K-th and (K+1)-th keys lie within the band; at most 2 % of the pairs of this module may be, asserted from the reference alone (test_few_pairs_are_ambiguous;
counted: 0 of 702).  Slots must descend in the kernel's own keys: its scores, plus the reference's g when stochastic (to within the
band).  Exact ties -- two byte-identical live beams with equal scores -- must be ordered by the flat index exactly.

Reorder: bit for bit against the gather, poison kept beyond n_r, the source untouched.  Backtrack: equal to the reference walk.
"""
import numpy as np
import pytest
import torch

import beam_ref
import kernel_checks as KC
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
R_SEL = 2.0 ** -20
G_ERR = 2.0 ** -19
POISON = -77777
SEEN = {"r": 0.0, "g": 0.0}                        # the largest ratios this process has seen, printed by the tests

# (B, K, V, ld)
SHAPES = [(1, 1, 90, 128), (5, 3, 65, 128), (3, 4, 337, 384), (2, 16, 1024, 1024), (2, 16, 1023, 1024)]
KINDS = ("gauss4", "shifted", "dominant")
TEMPS = (0.7, 1.0, 1.5)
STATES = ("first", "live", "dead")
OUT_LD = 24


def make_case(shape, kind, state, seed, identical=False):
    """logits bf16 [R, ld] (NaN beyond V), score f32 [B, K], tok, t: on the CPU, from the seed alone"""
    B, K, V, ld = shape
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B * K, V)) * 4.0
    if kind == "shifted":
        x -= 200.0
    elif kind == "dominant":
        x[np.arange(B * K), rng.integers(0, V, B * K)] += 60.0
    if identical:                                                                   # beams 0 and 1 of every prompt: the same row
        x.reshape(B, K, V)[:, 1] = x.reshape(B, K, V)[:, 0]
    logits = torch.full((B * K, ld), float("nan"), dtype=BF)
    logits[:, :V] = torch.from_numpy(x).to(BF)
    score = np.full((B, K), -np.inf, dtype=np.float32)
    if state == "first":
        score[:, 0] = 0.0
    else:
        score[:] = -30.0 * rng.random((B, K)).astype(np.float32)
        if state == "dead" and K > 2:
            score[:, 1:K - 1:2] = -np.inf                                           # dead beams in the middle
    if identical:
        score[:, 1] = score[:, 0]
    tok = rng.integers(0, V, B * K).astype(np.int32)
    t = rng.integers(0, OUT_LD - 1, B).astype(np.int32)
    return logits, score, tok, t


def band_of(key, stochastic):
    return 2 * R_SEL * np.maximum(1.0, np.abs(key)) + (G_ERR if stochastic else 0.0)


def ambiguous_prompts(ref, stochastic):
    """bool [B], from the reference alone: a chosen and a not-chosen key lie within the band (beam_ref.select's gap: ids of one
    beam with one logit value -- bf16 logits near -200 are whole numbers -- tie in any arithmetic and are no ambiguity)"""
    kth = np.array([ref["key"][b].reshape(-1)[f[-1]] if f else 0.0 for b, f in enumerate(ref["flat"])])
    return ref["gap"] <= band_of(kth, stochastic)


def run_select(shape, logits, score, tok, t, temperature, allow=None, stochastic=False, seed=0):
    B, K, V, ld = shape
    d = dict(logits=logits.to(DEV), score=torch.from_numpy(score.copy()).to(DEV), tok=torch.from_numpy(tok.copy()).to(DEV),
             parent=torch.full((B * K,), POISON, dtype=torch.int32, device=DEV),
             pos=torch.from_numpy(np.repeat(t, K)).to(DEV),
             ht=torch.full((B * K, OUT_LD), POISON, dtype=torch.int32, device=DEV),
             hp=torch.full((B * K, OUT_LD), POISON, dtype=torch.int32, device=DEV))
    KC.ops().beam_select(d["logits"], V, d["score"], d["tok"], d["parent"], d["pos"], d["ht"], d["hp"], temperature=temperature,
                       allow_table=None if allow is None else torch.from_numpy(allow.view(np.int32)).to(DEV),
                       stochastic=stochastic, seed=seed)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items() if k != "logits"}


def check_select(shape, got, ref, t, stochastic, seed, what, exact=False, raw=None):
    """every assertion of one case; returns the number of prompts whose chosen set differs (inside the band) from the reference's"""
    B, K, V, ld = shape
    tok, parent, score = got["tok"].reshape(B, K), got["parent"].reshape(B, K), got["score"]
    # consistency: the history column t + 1 and nothing else, the positions advanced
    cols = np.arange(OUT_LD)[None, :] == np.repeat(t, K)[:, None] + 1
    assert np.array_equal(got["ht"][cols].reshape(B, K), tok) and np.array_equal(got["hp"][cols].reshape(B, K), parent), what
    assert np.all(got["ht"][~cols] == POISON) and np.all(got["hp"][~cols] == POISON), what
    assert np.array_equal(got["pos"], np.repeat(t, K) + 1), what
    assert parent.min() >= 0 and parent.max() < K and tok.min() >= 0 and tok.max() < V, what
    g = beam_ref.gumbel(seed, t, B, K, V) if stochastic else None
    raw = raw.reshape(B, K, V)                                                      # the logits, for the ties inside a beam
    moved = 0
    for b in range(B):
        n = len(ref["flat"][b])                                                     # finite candidates chosen: exact, not rounded
        live = np.isfinite(score[b])
        assert live.sum() == n and np.all(live[:n]), (what, b, score[b], n)
        assert np.all(tok[b, n:] == tok[b, 0]) and np.all(parent[b, n:] == parent[b, 0]), (what, b)     # dead copies of slot 0
        flat = (parent[b, :n] * V + tok[b, :n]).tolist()
        assert len(set(flat)) == n, (what, b, flat)
        rc, rk = ref["cand"][b].reshape(-1), ref["key"][b].reshape(-1)
        assert np.all(np.isfinite(rc[flat])), (what, b, flat)                       # -inf is never chosen
        err = np.abs(score[b, :n].astype(np.float64) - rc[flat]) / np.maximum(1.0, np.abs(rc[flat]))
        SEEN["r"] = max(SEEN["r"], float(err.max(initial=0.0)))
        assert np.all(err <= R_SEL), (what, b, err.max())
        if exact:
            assert flat == ref["flat"][b], (what, b, flat, ref["flat"][b])
        elif set(flat) != set(ref["flat"][b]):
            moved += 1
            kth = rk[ref["flat"][b][-1]]
            for f in set(flat) ^ set(ref["flat"][b]):
                assert abs(rk[f] - kth) <= band_of(kth, stochastic), (what, b, f, rk[f], kth)
        if not stochastic:                                                          # structural ties: the smaller id first
            for f in flat:
                twins = np.nonzero(raw[b, f // V, :f % V] == raw[b, f // V, f % V])[0] + f // V * V
                assert set(twins.tolist()) <= set(flat), (what, b, f, twins, flat, ref["flat"][b], score[b].tolist())
        own = score[b, :n].astype(np.float64) + (g[b].reshape(-1)[flat] if stochastic else 0.0)
        slack = band_of(own[:-1], True) if stochastic else 0.0                      # deterministic: the kernel's own scores, exactly
        assert np.all(own[:-1] + slack >= own[1:]), (what, b, own)
    return moved


def select_cases(shape, stochastic):
    i = 0
    for kind in KINDS:
        for temp in TEMPS:
            for state in STATES:
                i += 1
                yield kind, temp, state, 1000 * SHAPES.index(shape) + 10 * i + int(stochastic)


@pytest.mark.parametrize("stochastic", [False, True], ids=["det", "stoch"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_select(shape, stochastic):
    B, K, V, ld = shape
    moved = 0
    for kind, temp, state, seed in select_cases(shape, stochastic):
        logits, score, tok, t = make_case(shape, kind, state, seed)
        ref = beam_ref.select(logits[:, :V].double().numpy(), temp, score, tok, t, None, stochastic, seed)
        got = run_select(shape, logits, score, tok, t, temp, None, stochastic, seed)
        moved += check_select(shape, got, ref, t, stochastic, seed, (shape, kind, temp, state, stochastic),
                              raw=logits[:, :V].double().numpy())
        if stochastic:                                                              # the fp32 error of g, of every case
            g32 = beam_ref.gumbel(seed, t, B, K, V, np.float32).astype(np.float64)
            SEEN["g"] = max(SEEN["g"], float(np.abs(g32 - beam_ref.gumbel(seed, t, B, K, V)).max()))
    assert 2 * SEEN["g"] <= G_ERR, SEEN["g"]
    print(f"\nselect {shape} stochastic={stochastic}: largest |score - ref| / max(1, |ref|) so far {SEEN['r']:.3e} = "
          f"{SEEN['r'] * 2 ** 23:.2f} * 2^-23 (R_SEL {R_SEL:.3e}); fp32 error of g {SEEN['g']:.3e}; {moved} sets moved inside the band")


def test_few_pairs_are_ambiguous():
    """a condition on this module's cases, from the reference alone: at most 2 % of the (case, prompt) pairs"""
    amb = total = 0
    for stochastic in (False, True):
        for shape in SHAPES:
            B, K, V, ld = shape
            for kind, temp, state, seed in select_cases(shape, stochastic):
                logits, score, tok, t = make_case(shape, kind, state, seed)
                ref = beam_ref.select(logits[:, :V].double().numpy(), temp, score, tok, t, None, stochastic, seed)
                a = ambiguous_prompts(ref, stochastic)
                amb, total = amb + int(a.sum()), total + B
    print(f"\nambiguous (case, prompt) pairs: {amb} of {total}")
    assert amb <= 0.02 * total, (amb, total)


@pytest.mark.parametrize("stochastic", [False, True], ids=["det", "stoch"])
def test_select_grammar(stochastic):
    """the sampler's grammar rule per beam: a row that allows nothing is ignored, and a prompt whose live beams allow fewer than
    K ids in total leaves dead slots that copy slot 0"""
    shape = B, K, V, ld = SHAPES[2]
    rng = np.random.default_rng(5)
    allow = (rng.random((V, (V + 31) // 32, 32)) < 0.3)
    allow[7] = False                                                                # allows nothing: ignored
    allow[11] = False
    allow[11].reshape(-1)[[3, 200]] = True                                          # two ids only
    table = (allow.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    for temp in TEMPS:
        logits, score, tok, t = make_case(shape, "gauss4", "live", 77)
        tok = tok.reshape(B, K)
        tok[0, 0] = 7                                                               # prompt 0: one beam with the empty row
        tok[1] = 11                                                                 # prompt 1: one live beam, two allowed ids < K
        score[1, 1:] = -np.inf
        tok[2, 1] = 11
        tok = tok.reshape(-1)
        ref = beam_ref.select(logits[:, :V].double().numpy(), temp, score, tok, t, table, stochastic, 3)
        assert len(ref["flat"][1]) == 2 and sorted(ref["flat"][1]) == [3, 200] and not ambiguous_prompts(ref, stochastic).any()
        got = run_select(shape, logits, score, tok, t, temp, table, stochastic, 3)
        assert check_select(shape, got, ref, t, stochastic, 3, ("grammar", temp, stochastic), raw=logits[:, :V].double().numpy()) == 0
        assert np.all(got["score"][1, 2:] == -np.inf)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[3]], ids=lambda s: "x".join(map(str, s)))
def test_select_exact_ties(shape):
    """beams 0 and 1 byte-identical with equal scores: every key occurs twice, and the flat index decides -- exactly"""
    B, K, V, ld = shape
    for kind, temp in (("gauss4", 1.0), ("shifted", 0.7), ("dominant", 1.5)):
        logits, score, tok, t = make_case(shape, kind, "live", 31, identical=True)
        score[:, 2:] -= 40.0                                                        # the twins lead: their ties fill the beam
        ref = beam_ref.select(logits[:, :V].double().numpy(), temp, score, tok, t)
        for b in range(B):                                                          # a condition on the case: distinct values apart
            keys = np.unique(ref["key"][b][np.isfinite(ref["key"][b])])[::-1][:K + 1]
            assert np.all(-np.diff(keys) > band_of(keys[:-1], False)), (shape, kind, b)
            assert ref["flat"][b][0] < V and any(f + V in ref["flat"][b] for f in ref["flat"][b] if f < V)      # twins are chosen
        got = run_select(shape, logits, score, tok, t, temp)
        check_select(shape, got, ref, t, False, 0, ("ties", shape, kind), exact=True, raw=logits[:, :V].double().numpy())


# =====================================================================================================================
# reorder
# =====================================================================================================================
REORDER_SHAPES = [(6, 3, 1, 40), (32, 4, 3, 300), (8, 4, 8, 1030)]                  # (R, K, h, Lmax)


def _parents(kind, R, K, rng):
    k = np.arange(R) % K
    return {"identity": k, "all-to-one": np.full(R, K - 1), "permutation": (k + 1) % K,
            "random": rng.integers(0, K, R)}[kind].astype(np.int32)


@pytest.mark.parametrize("row_bytes", [128, 64, 4])
@pytest.mark.parametrize("shape", REORDER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reorder(shape, row_bytes):
    R, K, h, Lmax = shape
    rng = np.random.default_rng(R + row_bytes)
    dims = (R, h, Lmax) + ((64,) if row_bytes != 4 else ())
    width = {128: torch.int16, 64: torch.uint8, 4: torch.int32}[row_bytes]         # the bytes of bf16 rows, codes, f32 scales
    view = {128: BF, 64: torch.uint8, 4: torch.float32}[row_bytes]
    src_np = rng.integers(0, 120, dims).astype({128: np.int16, 64: np.uint8, 4: np.int32}[row_bytes])
    src = torch.from_numpy(src_np).to(DEV).view(view)
    assert src.element_size() * (64 if row_bytes != 4 else 1) == row_bytes
    poison = torch.full(dims, 0x55, dtype=width, device=DEV)
    ns = [np.full(R, min(n, Lmax)) for n in (1, 2, 3, 63, 64, 65, Lmax)]
    ns.append(np.repeat(rng.choice([1, 2, 3, 63, 64, 65, Lmax], R // K), K).clip(max=Lmax))        # mixed across prompts
    for n in ns:
        for kind in ("identity", "all-to-one", "permutation", "random"):
            parent = _parents(kind, R, K, rng)
            dst = poison.clone().view(view)
            KC.ops().kv_beam_reorder(dst, src, torch.from_numpy(parent).to(DEV), torch.from_numpy(n.astype(np.int32)).to(DEV), K)
            got = dst.view(width).cpu().numpy()
            want = beam_ref.reorder(poison.cpu().numpy(), src_np, parent, n, K)
            assert np.array_equal(got, want), (shape, row_bytes, kind, n.tolist())
    assert np.array_equal(src.view(width).cpu().numpy(), src_np)                    # the source is never written


def test_reorder_refuses_one_buffer():
    from musicgeneration_amd._lib import MgxError
    x = torch.zeros(4, 1, 8, 64, dtype=BF, device=DEV)
    z = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(MgxError, match="different buffers"):
        KC.ops().kv_beam_reorder(x, x, z, z, 2)


# =====================================================================================================================
# backtrack
# =====================================================================================================================
@pytest.mark.parametrize("R,K,steps", [(4, 4, 1), (12, 4, 7), (32, 8, 40)])
def test_backtrack(R, K, steps):
    rng = np.random.default_rng(R)
    out_ld = steps + 9
    c0 = np.repeat(rng.integers(1, 10, R // K), K).astype(np.int32)                 # ragged: one first column per prompt
    ht = rng.integers(0, 500, (R, out_ld)).astype(np.int32)
    hp = rng.integers(0, K, (R, out_ld)).astype(np.int32)
    out = np.full((R, out_ld), POISON, dtype=np.int32)
    got = torch.from_numpy(out).to(DEV)
    KC.ops().beam_backtrack(torch.from_numpy(ht).to(DEV), torch.from_numpy(hp).to(DEV), torch.from_numpy(c0).to(DEV), got, K, steps)
    want = beam_ref.backtrack(ht, hp, c0, steps, K, out)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want != POISON).sum() == R * steps                                      # the prompt columns are the caller's
