"""generate_cached(samples_per_prompt=N) and generate.py --share-prompt: N continuations of every prompt over one shared prompt
K/V cache (ABI 26).  The model, its reference parameters and the per-row check against the training forward (1e-2) and the
CPU oracle (2e-2) are those of tests/decode_fixtures.py."""
import glob
import os

import pytest
import torch

from decode_fixtures import check_rows, prompt_file, ragged_prior, tame_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def test_ragged_prompts_match_the_forward_and_the_oracle_per_row():
    mt, p0 = tame_model()
    V, n, N, lens = 337, 20, 4, [1, 7, 33]
    x = ragged_prior(lens, V, torch.Generator().manual_seed(17))
    toks, probs = mt.generate_cached(x.cuda(), n, top_p=0.95, seed=9, return_probs=True, prior_lengths=lens, samples_per_prompt=N)
    torch.cuda.synchronize()
    check_rows(mt, p0, x, lens, N, n, toks, probs, V)
    # the samples of a prompt are independent draws
    t = toks.cpu().view(len(lens), N, -1)
    for b in range(len(lens)):
        assert len({tuple(row.tolist()) for row in t[b]}) > 1, b


def test_more_than_32_rows_take_the_unfused_chain():
    mt, p0 = tame_model()
    V, n, N, lens = 337, 12, 12, [1, 7, 33]                                        # R = 36 rows
    x = ragged_prior(lens, V, torch.Generator().manual_seed(41))
    toks, probs = mt.generate_cached(x.cuda(), n, top_k=20, seed=2, return_probs=True, prior_lengths=lens, samples_per_prompt=N)
    torch.cuda.synchronize()
    check_rows(mt, p0, x, lens, N, n, toks, probs, V, rows=(0, 11, 12, 17, 24, 35))


def test_a_long_prompt_on_the_split_key_path_matches_the_oracle():
    from musicgeneration_amd import ops
    V, L, n, N, lens = 337, 1280, 8, 3, [1100, 40]
    d = 64
    assert ops.rel_attn_decode_shared_splits(len(lens), N, max(lens) - 1, n, d) > 1
    mt, p0 = tame_model(d=d, nl=1, L=L, V=V, seed=21)
    x = ragged_prior(lens, V, torch.Generator().manual_seed(29))
    toks, probs = mt.generate_cached(x.cuda(), n, top_p=0.95, seed=4, return_probs=True, prior_lengths=lens, samples_per_prompt=N)
    torch.cuda.synchronize()
    check_rows(mt, p0, x, lens, N, n, toks, probs, V, rows=(0, 2, 3, 5), forward=False)


def test_same_seed_same_tokens_and_graph_replay_is_bitwise_the_eager_run():
    mt, _ = tame_model(d=128, nl=2, L=160, V=337, seed=31)
    lens, N = [3, 40, 17], 5
    x = ragged_prior(lens, 337, torch.Generator().manual_seed(8)).cuda()
    kw = dict(top_p=0.95, seed=77, prior_lengths=lens, samples_per_prompt=N)
    ref = mt.generate_cached(x, 60, use_graph=False, **kw)
    for use_graph in (False, True):
        got = mt.generate_cached(x, 60, use_graph=use_graph, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, ref), use_graph
    other = mt.generate_cached(x, 60, use_graph=True, **dict(kw, seed=78))
    assert not torch.equal(other, ref)
    assert len(set(ref[:N, 50].tolist())) > 1                                      # the samples of prompt 0 differ
    # equal-length prompts without prior_lengths: the same rows as with them
    y = torch.randint(0, 336, (2, 24), generator=torch.Generator().manual_seed(3)).cuda()
    a = mt.generate_cached(y, 30, top_p=0.9, seed=5, samples_per_prompt=3)
    b = mt.generate_cached(y, 30, top_p=0.9, seed=5, samples_per_prompt=3, prior_lengths=[24, 24])
    assert a.shape == (6, 54) and torch.equal(a, b)


def test_first_step_agrees_with_the_call_on_repeated_prompts():
    """same seed, the prompts repeated N times through the ragged call: the first sampled step's distributions agree to 1e-2
    (different kernels: not bitwise).  The share of rows whose tokens are identical throughout is printed, not asserted: a
    last-bit difference may flip a draw"""
    mt, _ = tame_model()
    V, n, N, lens = 337, 20, 4, [1, 7, 33]
    x = ragged_prior(lens, V, torch.Generator().manual_seed(17)).cuda()
    kw = dict(top_p=0.95, seed=9, return_probs=True)
    ts, ps = mt.generate_cached(x, n, prior_lengths=lens, samples_per_prompt=N, **kw)
    tr, pr = mt.generate_cached(x.repeat_interleave(N, 0), n, prior_lengths=[v for v in lens for _ in range(N)], **kw)
    assert ts.shape == tr.shape and ps.shape == pr.shape
    for r in range(len(lens) * N):
        P = lens[r // N]
        assert (ps[r, P - 1] - pr[r, P - 1]).abs().max().item() < 1e-2, r
    same = (ts == tr).all(1).float().mean().item()
    print(f"\nrows whose tokens are identical to the repeated call's throughout: {100 * same:.0f} %")


def test_without_the_keyword_nothing_changes():
    mt, _ = tame_model()
    lens = [1, 7, 33]
    x = ragged_prior(lens, 337, torch.Generator().manual_seed(17)).cuda()
    for kw in (dict(prior_lengths=lens), dict()):
        xx = x if kw else x[2:]
        a = mt.generate_cached(xx, 20, top_p=0.95, seed=9, **kw)
        b = mt.generate_cached(xx, 20, top_p=0.95, seed=9, samples_per_prompt=None, **kw)
        assert torch.equal(a, b)


def test_one_token_prompt_with_a_grammar(tmp_path):
    """--grammar: the one-token prompt, pre_rows = 0 -- every key is a row's own; the mask rides in the sampler as always"""
    import numpy as np
    from musicgeneration_amd import generate
    from musicgeneration_amd.REMI import REMI_EventSeq
    from musicgeneration_amd.network import MusicTransformer
    torch.manual_seed(0)
    mt = MusicTransformer(embedding_dim=128, vocab_size=REMI_EventSeq.dim() + 1, num_layer=2, max_seq=128, dropout=0.0).cuda().eval()
    tab = REMI_EventSeq.next_token_table()
    bar = REMI_EventSeq.feat_ranges()['bar'][0]
    out = mt.generate_cached(torch.full((1, 1), bar, device=DEV), 60, top_p=0.95, seed=3, grammar=tab, samples_per_prompt=6).cpu().numpy()
    assert out.shape == (6, 61) and len({tuple(row) for row in out.tolist()}) > 1
    for row in out:
        for a, b in zip(row, row[1:]):
            assert (tab[a, b >> 5] >> np.uint32(b & 31)) & np.uint32(1), (a, b)
    gen = str(tmp_path / "gen") + "/"
    generate.main(["-o", gen, "-b", "3", "-l", "24", "--num-layers", "1", "--d-model", "128", "-M", "128", "-d", "", "--repr", "remi",
                   "--grammar", "--share-prompt"])
    assert len(glob.glob(gen + "gen-*.mid")) == 3


def test_refusals_on_the_device():
    mt, _ = tame_model()
    x = torch.randint(0, 300, (3, 40)).cuda()
    for kw in (dict(samples_per_prompt=17), dict(samples_per_prompt=2, window=64), dict(samples_per_prompt=2, kv_cache="fp8"),
               dict(samples_per_prompt=2, return_cache=True), dict(samples_per_prompt=2, length=57)):
        with pytest.raises(ValueError):
            mt.generate_cached(x, kw.pop("length", 10), **kw)


# ---------------------------------------------------------------------------------------------------------------------
# generate.py --share-prompt
# ---------------------------------------------------------------------------------------------------------------------
def _head(f, want):
    from musicgeneration_amd.sequence import NoteSeq
    got = sorted(NoteSeq.from_midi_file(f).notes, key=lambda n_: (n_.start, n_.pitch))
    last = want[-1][2]
    return [(n_.pitch, round(n_.start, 2)) for n_ in got if n_.start < last - 1e-3], [(p, round(s, 2)) for _, p, s, _ in want[:-1]]


def test_generate_cli_shares_one_prompt_file_between_the_batch(tmp_path, capsys):
    from musicgeneration_amd import generate
    a = str(tmp_path / "a.mid")
    notes = prompt_file(a, 11, 48)
    out = str(tmp_path / "gen") + "/"
    torch.manual_seed(0)
    generate.main(["-o", out, "-b", "4", "-l", "24", "--num-layers", "1", "--d-model", "128", "-M", "128", "-d", "", "--top-p", "0.9",
                   "-c", a, "--share-prompt"])
    assert capsys.readouterr().out.count("Prompt:") == 1
    files = sorted(glob.glob(out + "gen-*.mid"))
    assert [os.path.basename(f) for f in files] == [f"gen-00{i}.mid" for i in range(4)]
    for f in files:
        got, want = _head(f, notes)
        assert got == want, f


def test_generate_cli_shares_each_condition_file_between_its_candidates(tmp_path, capsys):
    from musicgeneration_amd import generate
    a, b = str(tmp_path / "a.mid"), str(tmp_path / "b.mid")
    notes = {a: prompt_file(a, 3, 60), b: prompt_file(b, 11, 48)}
    out = str(tmp_path / "gen") + "/"
    torch.manual_seed(0)
    generate.main(["-o", out, "-b", "5", "-l", "16", "--num-layers", "1", "--d-model", "128", "-M", "128", "-d", "", "--top-p", "0.9",
                   "--condition-files", f"{a},{b}", "--best-of", "3", "--share-prompt"])
    log = capsys.readouterr().out
    assert log.count("Prompt:") == 2 and "Best of 3: log-probabilities" in log
    files = sorted(glob.glob(out + "gen-*.mid"))
    assert [os.path.basename(f) for f in files] == ["gen-000.mid", "gen-001.mid"]      # one per file, -b ignored
    for f, src in zip(files, (a, b)):
        got, want = _head(f, notes[src])
        assert got == want, f
