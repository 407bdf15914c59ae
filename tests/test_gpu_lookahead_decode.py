"""generate_cached(lookahead=T) and generate.py --lookahead: draft-and-verify decode (ABI 32).  The model, its reference parameters
and the per-row check against the training forward (1e-2) and the CPU oracle (2e-2) are those of tests/decode_fixtures.py; the
one-token call of the same seed is computed once and shared (its sample is the guide, and what the result is compared with)."""
import glob

import pytest
import torch

from decode_fixtures import check_rows, ragged_prior, tame_model

pytestmark = pytest.mark.gpu

V, N, T, LENS = 337, 20, 4, [1, 7, 33]
KW = dict(top_p=0.95, seed=9, return_probs=True, prior_lengths=LENS)


@pytest.fixture(scope="module")
def model():
    return tame_model()


@pytest.fixture(scope="module")
def prompts():
    return ragged_prior(LENS, V, torch.Generator().manual_seed(17))


@pytest.fixture(scope="module")
def plain(model, prompts):
    """the one-token call: (tokens, distributions), left unchanged"""
    toks, probs = model[0].generate_cached(prompts.cuda(), N, **KW)
    torch.cuda.synchronize()
    return toks.clone(), probs.clone()


def test_history_drafts_match_the_forward_and_the_oracle_per_row(model, prompts):
    mt, p0 = model
    st = {}
    toks, probs = mt.generate_cached(prompts.cuda(), N, lookahead=T, stats=st, **KW)
    torch.cuda.synchronize()
    check_rows(mt, p0, prompts, LENS, 1, N, toks, probs, V)
    assert st["tokens"] == [N] * 3 and all(N // T <= s <= N for s in st["steps"]) and st["steps_run"] <= N, st


def test_a_guide_matches_the_forward_and_the_oracle_per_row(model, prompts, plain):
    mt, p0 = model
    toks, probs = mt.generate_cached(prompts.cuda(), N, lookahead=T, draft=plain[0], **KW)
    torch.cuda.synchronize()
    check_rows(mt, p0, prompts, LENS, 1, N, toks, probs, V)
    # a guide on the CPU, of another integer type and wider than the result, is the same guide
    wide = torch.nn.functional.pad(plain[0].cpu().long(), (0, 5))
    again, _ = mt.generate_cached(prompts.cuda(), N, lookahead=T, draft=wide, **KW)
    assert torch.equal(again, toks)


def test_agreement_with_the_one_token_call(model, prompts, plain):
    """the guide is the one-token call's own sample for the same seed.  The first sampled distributions agree to 1e-2; at least
    one row is that call's row throughout and then took exactly ceil(n / T) steps.  The share of identical rows and the tokens
    per step are printed, not asserted: a last-bit difference between the two chains may flip a draw"""
    mt, _ = model
    st = {}
    toks, probs = mt.generate_cached(prompts.cuda(), N, lookahead=T, draft=plain[0], stats=st, **KW)
    torch.cuda.synchronize()
    for r, P in enumerate(LENS):
        assert (probs[r, P - 1] - plain[1][r, P - 1]).abs().max().item() < 1e-2, r
    same = (toks == plain[0]).all(1).cpu().tolist()
    print(f"\nrows identical to the one-token call's throughout: {sum(same)} of {len(same)}; steps {st['steps']}, "
          f"tokens per step {sum(st['tokens']) / sum(st['steps']):.2f}")
    assert any(same), "no row identical to the one-token call's: choose another seed"
    assert any(ok and s == -(-N // T) for ok, s in zip(same, st["steps"])), st
    # history drafts on the same seed: the same sample where the chains agree, in more steps
    hist, _ = mt.generate_cached(prompts.cuda(), N, lookahead=T, **KW)
    print(f"rows of the history-draft call identical to the one-token call's: {(hist == plain[0]).all(1).sum().item()} of {len(same)}")


def test_same_seed_same_tokens_and_graph_replay_is_bitwise_the_eager_run(model, prompts):
    mt, _ = model
    x = prompts.cuda()
    kw = dict(KW, lookahead=T)
    ref_t, ref_p = mt.generate_cached(x, N, use_graph=False, **kw)
    for use_graph in (False, True):
        st = {}
        got_t, got_p = mt.generate_cached(x, N, use_graph=use_graph, stats=st, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got_t, ref_t) and torch.equal(got_p, ref_p), use_graph
    other, _ = mt.generate_cached(x, N, **dict(kw, seed=10))
    assert not torch.equal(other, ref_t)
    # equal-length prompts without prior_lengths, T = 2 and 8, no distributions
    y = torch.randint(0, 336, (2, 24), generator=torch.Generator().manual_seed(3)).cuda()
    one = mt.generate_cached(y, 30, top_p=0.9, seed=5)
    for t in (2, 8):
        a = mt.generate_cached(y, 30, top_p=0.9, seed=5, lookahead=t, draft=one)
        b = mt.generate_cached(y, 30, top_p=0.9, seed=5, lookahead=t, draft=one, prior_lengths=[24, 24], use_graph=False)
        assert a.shape == (2, 54) and torch.equal(a, b), t
        assert int(a[:, 24:].max()) < V and torch.equal(a[:, :24], y.to(torch.int32))


def test_a_periodic_prompt_with_history_drafts(model):
    """a prompt that repeats a figure: the drafts are the figure's continuation from the first step on"""
    mt, p0 = model
    lens = [24, 30, 13]
    fig = torch.tensor([60, 3, 64, 3, 67, 7])
    x = torch.stack([fig.repeat(5)[:30]] * 3)
    for b, n in enumerate(lens):
        x[b, n:] = -7
    st = {}
    toks, probs = mt.generate_cached(x.cuda(), N, top_k=8, seed=4, return_probs=True, prior_lengths=lens, lookahead=T, draft_ngram=4,
                                     stats=st)
    torch.cuda.synchronize()
    check_rows(mt, p0, x, lens, 1, N, toks, probs, V)
    assert st["tokens"] == [N] * 3
    print(f"\nperiodic prompt, history drafts: steps {st['steps']} for {N} tokens")


def test_eight_positions_on_the_split_key_path_match_the_oracle():
    from musicgeneration_amd import ops
    L, n, lens, d = 1280, 12, [1100, 40], 64
    assert ops.rel_attn_decode_multi_splits(len(lens), 8, max(lens) + n, d) > 1
    mt, p0 = tame_model(d=d, nl=1, L=L, V=V, seed=21)
    x = ragged_prior(lens, V, torch.Generator().manual_seed(29))
    kw = dict(top_p=0.95, seed=4, return_probs=True, prior_lengths=lens)
    one, _ = mt.generate_cached(x.cuda(), n, **kw)
    st = {}
    toks, probs = mt.generate_cached(x.cuda(), n, lookahead=8, draft=one, stats=st, **kw)
    torch.cuda.synchronize()
    check_rows(mt, p0, x, lens, 1, n, toks, probs, V, forward=False)
    print(f"\nsplit-key path, T = 8, guide: steps {st['steps']} for {n} tokens; rows identical to the one-token call's: "
          f"{(toks == one).all(1).sum().item()} of 2")


def test_without_the_keyword_nothing_changes(model, prompts, plain):
    mt, _ = model
    toks, probs = mt.generate_cached(prompts.cuda(), N, lookahead=None, draft="history", draft_ngram=3, stats=None, **KW)
    assert torch.equal(toks, plain[0]) and torch.equal(probs, plain[1])


def test_generate_cli_writes_its_files(tmp_path, capsys):
    from musicgeneration_amd import generate
    out = str(tmp_path / "gen") + "/"
    torch.manual_seed(0)
    generate.main(["-o", out, "-b", "3", "-l", "24", "--num-layers", "1", "--d-model", "128", "-M", "128", "-d", "", "--top-p", "0.9",
                   "--lookahead", "4", "--draft-ngram", "2"])
    assert len(glob.glob(out + "gen-*.mid")) == 3
    assert "Lookahead:" in capsys.readouterr().out
