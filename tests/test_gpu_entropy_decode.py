"""generate_cached / generate_timed (entropy_sampling=) (ABI 34) at the model level: the tamed model (d 128, two layers, V 337), four
ragged prompts of 3 .. 9 tokens, 24 events.  tests/entropy_ref.py is the host-side restatement; the plain call of the same seed is
computed once and shared.  The call's temperature is 0.35: at 1 the tamed model's distributions are within 0.3 bits of uniform
(8.2 of 8.4 bits), where a cut relative to the row's own shape has nothing to follow; at 0.35 they have 5 to 7 bits.

First step, exact.  The mask writes -inf and nothing else, so what the sampler files is the plain call's distribution renormalised
over the kept set -- two f32 softmaxes apart, 2e-6 as in tests/test_gpu_class_decode.py -- and the kept set is the reference's,
computed from the plain call's filed distribution, wherever the reference's margins are >= 1e-3.  The parameters are the first of
a short list for which they are, on those four rows: a choice made on the plain call's output alone.

Whole sample.  Every drawn token has filed probability > 0; every id of a filed support has p' >= min_p max p' (1 - 1e-5); with
Mirostat the traced surprise of a drawn token is at most the mu in force (+ 1e-5 bits: the mask and the account evaluate the same
surprise in f32 by two routes, each within 2^-22 (|z| log2 e + |s|) < 5e-6 of it for |z|, |s| <= 10), or the support is the
arg-max ties; the final mu is the host's float32 recurrence over the traced surprises.

The trace against the training forward.  check_rows (tests/decode_fixtures.py) allows |p_decode - p_forward| < eps = 1e-2 for every
id.  The traced surprise is s = -log2 p_decode(token), so s - s_forward = -log2(p_decode / p_forward) with p_decode inside
(p_forward - eps, p_forward + eps):  |s - s_forward| < max(log2(1 + eps / p_forward), -log2(1 - eps / p_forward))
= -log2(1 - eps / p_forward) where p_forward > eps; where p_forward <= eps the tolerance lets p_decode reach 0 and implies no
bound, so such a token is counted and not compared.  Under Mirostat a drawn token has p >= 2^-mu, which keeps most of them above
eps.  This comparison is made where the distribution before the mask is the model's own -- the plain keyword, samples_per_prompt,
generate_timed up to the step at which a row has less left than the dearest id costs (from there on the budget's mask takes ids
out of the log-sum-exp) -- not under a grammar, a penalty, class sampling, the window or the 8-bit cache, whose logits are not the
forward's.  First GPU run: largest |s - s_forward| / bound 0.92 (min-p + typical), 0.25 (Mirostat), 0.77 (two samples per prompt);
the temperature of 0.35 multiplies a bf16 rounding difference of the two chains' logits by 2.9 before it reaches a probability."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import entropy_ref
from decode_fixtures import check_rows, prompt_file, ragged_prior, tame_model
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, N, LENS, SEED, TEMP = 337, 24, [3, 9, 5, 7], 11, 0.35
PAD = V - 1
KW = dict(seed=SEED, prior_lengths=LENS, temperature=TEMP, return_probs=True)
SOFTMAX_F32 = 2e-6
MARGIN = 1e-3
EPS_ROWS = 1e-2                                                               # check_rows' tolerance on a probability
MIN_P, TAU, ETA = 0.1, 4.0, 0.25                                              # the whole-sample setting


def _es(**kw):
    from musicgeneration_amd.decode import EntropySampling
    return EntropySampling(**kw)


@pytest.fixture(scope="module")
def model():
    return tame_model()


@pytest.fixture(scope="module")
def prompts():
    return ragged_prior(LENS, V, torch.Generator().manual_seed(5), fill=0)


@pytest.fixture(scope="module")
def plain(model, prompts):
    """the call without the keyword: (tokens, distributions) on the CPU, left unchanged"""
    toks, probs = model[0].generate_cached(prompts.cuda(), N, **KW)
    torch.cuda.synchronize()
    return toks.cpu(), probs.cpu()


def same_bits(a, b):
    """equal, NaN included"""
    return a.shape == b.shape and torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def test_an_inert_object_is_the_call_without_the_keyword(model, prompts, plain):
    mt = model[0]
    for es in (_es(), _es(min_p=0.0, typical_p=1.0, tau=None, eta=0.3, trace=False)):
        for g in (True, False):
            t, p = mt.generate_cached(prompts.cuda(), N, entropy_sampling=es, use_graph=g, **KW)
            assert torch.equal(t.cpu(), plain[0]) and torch.equal(p.cpu(), plain[1]), g
            assert es.mu is None and es.surprise is None


# ---- first step, exact ----------------------------------------------------------------------------------------------------------
def _ref_kw(kw):
    """the reference's arguments for the first step of a call with EntropySampling(**kw): mu starts at 2 tau"""
    return dict(min_p=kw.get("min_p", 0.0), typical_p=kw.get("typical_p", 1.0), mu=None if kw.get("tau") is None else 2.0 * kw["tau"])


def _choose(plain, candidates):
    """the first setting whose reference margins on the plain call's four first distributions are all >= MARGIN"""
    for kw in candidates:
        smallest = min(entropy_ref.smallest(entropy_ref.kept_from_probs(plain[1][b, P - 1].double().numpy(), **_ref_kw(kw))[1])
                       for b, P in enumerate(LENS))
        if smallest >= MARGIN:
            return kw, smallest
    raise AssertionError("no candidate setting with margins >= 1e-3 on these four rows")


FIRST_STEP = {
    "min_p": [dict(min_p=m) for m in (0.2, 0.15, 0.25, 0.1, 0.3)],
    "typical": [dict(typical_p=t) for t in (0.5, 0.45, 0.55, 0.4, 0.6, 0.35, 0.65)],
    "mirostat": [dict(tau=t) for t in (3.5, 3.4, 3.6, 3.3, 3.7, 3.2, 3.8)],
    "all": [dict(tau=t, min_p=m, typical_p=p) for t in (3.5, 3.4, 3.6, 3.7) for m in (0.1, 0.15) for p in (0.5, 0.6, 0.4)],
}


@pytest.mark.parametrize("name", list(FIRST_STEP))
def test_first_step(model, prompts, plain, name):
    kw, smallest = _choose(plain, FIRST_STEP[name])
    t, p = model[0].generate_cached(prompts.cuda(), N, entropy_sampling=_es(**kw), **KW)
    p = p.cpu().double().numpy()
    worst, cut = 0.0, 0
    for b, P in enumerate(LENS):
        src = plain[1][b, P - 1].double().numpy()
        kept, margins = entropy_ref.kept_from_probs(src, **_ref_kw(kw))
        assert entropy_ref.smallest(margins) >= MARGIN
        assert ((p[b, P - 1] > 0) == kept).all(), (name, b, np.flatnonzero((p[b, P - 1] > 0) != kept)[:8].tolist())
        want = np.where(kept, src, 0.0) / src[kept].sum()
        worst = max(worst, np.abs(p[b, P - 1] - want).max())
        cut += int((src > 0).sum() - kept.sum())
        assert abs(p[b, P - 1].sum() - 1) < 1e-5
    print(f"\nMEASURED first step [{name}] {kw}: smallest reference margin {smallest:.3g}; ids cut {cut}; largest |filed - renormalised "
          f"plain| {worst:.3g} (allowed {SOFTMAX_F32})")
    assert worst <= SOFTMAX_F32 and cut > 0


# ---- whole sample ---------------------------------------------------------------------------------------------------------------
def whole_sample(name, toks, probs, es, lens, steps, *, min_p=0.0, tau=None, eta=None, final_mu=None, table=None):
    """the whole-sample conditions of the module docstring for rows r with prompt lengths lens[r] and steps[r] generated events;
    final_mu: the rows whose final mu must be the recurrence's (default: all)"""
    toks, probs = toks.cpu().numpy(), probs.cpu().numpy()
    trace = None if es.surprise is None else es.surprise.cpu().numpy()
    mu_end = None if es.mu is None else es.mu.cpu().numpy()
    fallbacks = cuts = 0
    for r, P in enumerate(lens):
        n = steps[r]
        mu = np.float32(2.0 * tau) if tau is not None else None
        if trace is not None:
            assert np.isnan(trace[r, :P]).all() and np.isnan(trace[r, P + n:]).all(), (name, r)
            assert not np.isnan(trace[r, P:P + n]).any(), (name, r)
        for c in range(P - 1, P + n - 1):
            row, tok = probs[r, c], int(toks[r, c + 1])
            assert row[tok] > 0, (name, r, c)                                 # nothing drawn from outside the support
            assert abs(row.sum() - 1) < 1e-4, (name, r, c)
            sup = row > 0
            cuts += int((~sup).sum())
            if min_p > 0:
                assert (row[sup] >= min_p * row.max() * (1 - 1e-5)).all(), (name, r, c)
            if table is not None:
                assert not row[~entropy_ref.allowed_bits(table, int(toks[r, c]), V)].any(), (name, r, c)
            if tau is not None:
                s = trace[r, c + 1]
                ties = (row[sup] == row.max()).all()
                assert s <= mu + 1e-5 or ties, (name, r, c, s, mu)
                fallbacks += int(not s <= mu + 1e-5)
                mu = np.float32(mu - np.float32(np.float32(eta) * np.float32(s - np.float32(tau))))     # the kernel's three roundings
        if tau is not None and (final_mu is None or r in final_mu):
            assert abs(mu_end[r] - mu) <= n * 2.0 ** -23 * max(abs(mu), 2 * tau), (name, r, mu_end[r], mu)
    print(f"\n[{name}] ids cut over the sample {cuts}; steps on the arg-max fall-back {fallbacks}"
          + ("" if mu_end is None else f"; final mu {np.round(mu_end, 3).tolist()}"))
    assert cuts > 0, name
    return trace


def against_the_forward(name, mt, toks, trace, lens, steps, per=1):
    """the traced surprises against -log2 of the training forward's probability of the row's own tokens (module docstring)"""
    toks = toks.cpu()
    worst, finite, total = 0.0, 0, 0
    for r, P in enumerate(lens):
        n = steps[r]
        seq = toks[r:r + 1, :P + n]
        with torch.no_grad():
            fwd = torch.softmax(mt(seq.to(torch.int32).cuda())[0].double().cpu()[0] / TEMP, -1).numpy()
        for c in range(P - 1, P + n - 1):
            pf = fwd[c, int(toks[r, c + 1])]
            total += 1
            if pf <= EPS_ROWS:
                continue
            finite += 1
            ratio = abs(trace[r, c + 1] + np.log2(pf)) / -np.log2(1 - EPS_ROWS / pf)
            worst = max(worst, ratio)
            assert ratio <= 1, (name, r, c, trace[r, c + 1], -np.log2(pf))
    print(f"\nMEASURED surprise trace against the forward [{name}]: largest |s - s_forward| / bound {worst:.3f} over {finite} of {total} "
          f"tokens (the others have p_forward <= {EPS_ROWS}, where check_rows' tolerance implies no bound)")
    assert finite > 0, name


def test_whole_sample_min_p_and_typical(model, prompts, plain):
    mt = model[0]
    es = _es(min_p=MIN_P, typical_p=0.7, trace=True)
    toks, probs = mt.generate_cached(prompts.cuda(), N, entropy_sampling=es, **KW)
    check_rows(mt, None, prompts, LENS, 1, N, toks, probs, V, oracle=False, forward=False)      # shapes, prompt, padding
    assert es.mu is None and es.surprise.shape == (4, max(LENS) + N)
    trace = whole_sample("min-p + typical", toks, probs, es, LENS, [N] * 4, min_p=MIN_P)
    against_the_forward("min-p + typical", mt, toks, trace, LENS, [N] * 4)
    assert not torch.equal(toks.cpu(), plain[0])                              # the keyword changes the sample


def test_whole_sample_mirostat(model, prompts):
    mt = model[0]
    es = _es(min_p=MIN_P, tau=TAU, eta=ETA, trace=True)
    toks, probs = mt.generate_cached(prompts.cuda(), N, entropy_sampling=es, **KW)
    check_rows(mt, None, prompts, LENS, 1, N, toks, probs, V, oracle=False, forward=False)
    assert es.mu.shape == (4,) and es.mu.dtype == torch.float32 and es.lse.shape == (4,)
    trace = whole_sample("mirostat", toks, probs, es, LENS, [N] * 4, min_p=MIN_P, tau=TAU, eta=ETA)
    against_the_forward("mirostat", mt, toks, trace, LENS, [N] * 4)
    # the loop without a trace and without min-p: the same state
    bare = _es(tau=TAU, eta=ETA)
    mt.generate_cached(prompts.cuda(), N, entropy_sampling=bare, **KW)
    assert bare.surprise is None and bare.mu.shape == (4,) and torch.isfinite(bare.mu).all()


def test_same_seed_same_tokens_and_graph_replay_is_the_eager_run(model, prompts):
    mt, x = model[0], prompts.cuda()
    kw = dict(min_p=MIN_P, typical_p=0.7, tau=TAU, eta=ETA, trace=True)
    ref = _es(**kw)
    ref_t, ref_p = mt.generate_cached(x, N, entropy_sampling=ref, use_graph=False, **KW)
    for g in (True, False):
        es = _es(**kw)
        t, p = mt.generate_cached(x, N, entropy_sampling=es, use_graph=g, **KW)
        assert torch.equal(t, ref_t) and torch.equal(p, ref_p), g
        assert same_bits(es.mu, ref.mu) and same_bits(es.surprise, ref.surprise), g
    other, _ = mt.generate_cached(x, N, entropy_sampling=_es(**kw), **dict(KW, seed=SEED + 1))
    assert not torch.equal(other, ref_t)
    again = _es(**kw)                                                         # an object serves any number of calls
    mt.generate_cached(x, N, entropy_sampling=again, **KW)
    t2, _ = mt.generate_cached(x, N, entropy_sampling=again, **KW)
    assert torch.equal(t2, ref_t) and same_bits(again.mu, ref.mu)


# ---- composition ----------------------------------------------------------------------------------------------------------------
def test_under_a_grammar_every_token_is_allowed(model):
    from musicgeneration_amd.REMI import REMI_EventSeq
    assert REMI_EventSeq.dim() + 1 == V
    mt, table = model[0], REMI_EventSeq.next_token_table()
    prior = torch.full((4, 1), REMI_EventSeq.feat_ranges()["bar"][0], dtype=torch.long).cuda()
    es = _es(min_p=MIN_P, tau=TAU, eta=ETA, trace=True)
    toks, probs = mt.generate_cached(prior, N, seed=SEED, temperature=TEMP, grammar=table, entropy_sampling=es, return_probs=True)
    plain_t = mt.generate_cached(prior, N, seed=SEED, temperature=TEMP, grammar=table)
    assert not torch.equal(toks, plain_t)
    whole_sample("grammar", toks, probs, es, [1] * 4, [N] * 4, min_p=MIN_P, tau=TAU, eta=ETA, table=table)
    t = toks.cpu().numpy()
    for b in range(4):
        for j in range(N):
            a, v = int(t[b, j]), int(t[b, j + 1])
            assert (int(table[a, v >> 5]) >> (v & 31)) & 1, (b, j, a, v)


@pytest.mark.parametrize("name,kw,per", [
    ("repetition", "rep", 1), ("class sampling", "cls", 1), ("fp8", dict(kv_cache="fp8"), 1), ("window", dict(window=24, hop=8), 1),
    ("two samples per prompt", dict(samples_per_prompt=2), 2)])
def test_composition_meets_the_whole_sample_conditions_and_captured_is_eager(model, prompts, name, kw, per):
    from musicgeneration_amd.decode import ClassSampling, Repetition
    mt = model[0]
    if kw == "rep":
        subject = np.ones(V, dtype=np.int32)
        subject[PAD] = 0
        kw = dict(repetition=Repetition(subject, presence=0.5, frequency=0.25, window=8, ngram=2))
    elif kw == "cls":
        cls = np.zeros(V, dtype=np.int32)
        cls[88:176], cls[176:208], cls[208:336], cls[336] = 1, 2, 3, 4
        kw = dict(class_sampling=ClassSampling(cls, temperature={0: 0.3, 3: 0.5}, top_k={2: 4}))
    got = {}
    for g in (True, False):
        es = _es(min_p=MIN_P, tau=TAU, eta=ETA, trace=True)
        got[g] = (*mt.generate_cached(prompts.cuda(), N, entropy_sampling=es, use_graph=g, **KW, **kw), es)
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1]), name
    assert same_bits(got[True][2].mu, got[False][2].mu) and same_bits(got[True][2].surprise, got[False][2].surprise), name
    toks, probs, es = got[True]
    check_rows(mt, None, prompts, LENS, per, N, toks, probs, V, oracle=False, forward=False)
    lens = [P for P in LENS for _ in range(per)]
    trace = whole_sample(name, toks, probs, es, lens, [N] * len(lens), min_p=MIN_P, tau=TAU, eta=ETA)
    if per > 1:                                                               # the model's own distribution: the forward applies
        against_the_forward(name, mt, toks, trace, lens, [N] * len(lens))
    without = mt.generate_cached(prompts.cuda(), N, **KW, **kw)[0]
    assert not torch.equal(without, toks), name


def test_with_a_time_budget(model, prompts):
    """generate_timed: the account runs before the budget's, so a row's last kept token is in the trace and what an ended row
    goes on sampling is not"""
    mt = model[0]
    cost = np.zeros(V, dtype=np.int32)
    cost[208:336] = np.arange(1, 129)                                         # the time_shift class prices the clock
    budgets = [150, 250, 180, 220]
    got = {}
    for g in (True, False):
        es = _es(min_p=MIN_P, tau=TAU, eta=ETA, trace=True)
        res = mt.generate_timed(prompts.cuda(), budgets, cost, N, seed=SEED, prior_lengths=LENS, poll=8, temperature=TEMP,
                                entropy_sampling=es, return_probs=True, use_graph=g)
        got[g] = (res, es)
    (toks, lengths, info), es = got[True]
    assert torch.equal(got[False][0][0], toks) and torch.equal(got[False][0][1], lengths)
    assert same_bits(got[False][1].surprise, es.surprise)
    steps, spent, done = lengths.cpu().tolist(), info["spent"].cpu().numpy(), info["done"].cpu().numpy()
    print(f"\nlengths {steps}, spent {spent.tolist()} of {budgets}, done {done.tolist()}")
    t = toks.cpu().numpy()
    for b, P in enumerate(LENS):
        assert int(cost[t[b, P:P + steps[b]]].sum()) == spent[b] <= budgets[b] and (t[b, P + steps[b]:] == PAD).all()
    live = [b for b in range(4) if steps[b] == N and not done[b]]             # an ended row's mu went on moving on pad steps
    trace = whole_sample("timed", toks, info["probs"], es, LENS, steps, min_p=MIN_P, tau=TAU, eta=ETA, final_mu=live)
    # the forward applies while the budget's mask cannot bite: up to the first step whose row has less left than the dearest id
    free = [int((budgets[b] - np.concatenate([[0], np.cumsum(cost[t[b, P:P + steps[b]]])])[:steps[b]] >= cost.max()).sum())
            for b, P in enumerate(LENS)]
    assert all(0 < f for f in free), free
    print(f"steps before the budget's mask can bite: {free}")
    against_the_forward("timed", mt, toks, trace, LENS, free)


def test_lookahead_with_min_p_on_the_one_token_calls_own_sample(model, prompts):
    """the stateless part under draft and verify, the guide being the one-token call's own sample with the same keyword: what
    tests/test_gpu_lookahead_decode.py's agreement test asks of the plain pair -- first distributions within 1e-2, at least one row
    identical throughout, and such a row in ceil(N / T) steps"""
    mt, x, T = model[0], prompts.cuda(), 4
    es = _es(min_p=MIN_P)
    one_t, one_p = mt.generate_cached(x, N, entropy_sampling=es, **KW)
    st = {}
    toks, probs = mt.generate_cached(x, N, entropy_sampling=es, lookahead=T, draft=one_t, stats=st, **KW)
    check_rows(mt, None, prompts, LENS, 1, N, toks, probs, V, oracle=False, forward=False)
    whole_sample("lookahead", toks, probs, es, LENS, [N] * 4, min_p=MIN_P)
    for r, P in enumerate(LENS):
        assert (probs[r, P - 1] - one_p[r, P - 1]).abs().max().item() < 1e-2, r
    same = (toks == one_t).all(1).cpu().tolist()
    print(f"\nrows identical to the one-token call's throughout: {sum(same)} of {len(same)}; steps {st['steps']}, "
          f"tokens per step {sum(st['tokens']) / sum(st['steps']):.2f}")
    assert any(same), "no row identical to the one-token call's: choose another seed"
    assert any(ok and s == -(-N // T) for ok, s in zip(same, st["steps"])), st
    eager, _ = mt.generate_cached(x, N, entropy_sampling=es, lookahead=T, draft=one_t, use_graph=False, **KW)
    assert torch.equal(eager, toks)
    with pytest.raises(ValueError, match="sequential"):
        mt.generate_cached(x, N, entropy_sampling=_es(tau=3.0), lookahead=T, **KW)


def test_generate_py_writes_its_files(tmp_path):
    mt, _ = tame_model(d=128, nl=2, L=256, V=309)
    ckpt = str(tmp_path / "tame.pt")
    torch.save({"net": {k: v.cpu() for k, v in mt.state_dict().items()}}, ckpt)
    prompt = str(tmp_path / "prompt.mid")
    prompt_file(prompt, 5, 60)
    out = str(tmp_path / "g") + "/"
    cmd = [sys.executable, "-m", "musicgeneration_amd.generate", "-s", ckpt, "-o", out, "-b", "2", "-l", "60", "--num-layers", "2",
           "--d-model", "128", "-M", "256", "-c", prompt, "-d", str(tmp_path / "none"), "--min-p", "0.05", "--mirostat", "3"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert len(glob.glob(out + "gen-*.mid")) == 2 and r.stdout.count("===> ") == 2
