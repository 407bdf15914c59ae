"""Beam search on the KV-cache decode, the host side: every refusal of decode.check_beam_args and of generate.py's -B / -S (they
run before any device work, so no GPU and no library is needed), and the tests' own reference (tests/beam_ref.py) against a
brute-force enumeration of every sequence."""
import itertools

import numpy as np
import pytest
import torch

import beam_ref
from decode_fixtures import host_model


@pytest.mark.parametrize("length,kw,msg", [
    (10, dict(beam_size=0), "beam_size"),
    (10, dict(beam_size=17), "beam_size"),
    (10, dict(beam_size=-1), "beam_size"),
    (10, dict(beam_size=4, temperature=0.0), "temperature"),
    (10, dict(beam_size=4, temperature=-1.0), "temperature"),
    (0, dict(beam_size=4), "length"),
    (57, dict(beam_size=4), "max_seq"),                                             # P + length > max_seq
    (10, dict(beam_size=4, kv_cache="int4"), "kv_cache"),
    (10, dict(beam_size=4, prior_lengths=[0, 5, 40]), "1 .. 40"),                   # the ragged rules of check_args
    (10, dict(beam_size=4, prior_lengths=[41, 5, 40]), "1 .. 40"),
    (10, dict(beam_size=4, prior_lengths=[1, 5]), "2 entries"),
    (57, dict(beam_size=4, prior_lengths=[1, 5, 40]), "max_seq"),
])
def test_generate_beam_refusals(length, kw, msg):
    x = torch.randint(0, 300, (3, 40))
    with pytest.raises(ValueError, match=msg):
        host_model().generate_beam(x, length, **kw)


def test_beam_size_is_limited_by_the_vocabulary():
    with pytest.raises(ValueError, match="beam_size"):
        host_model(V=8).generate_beam(torch.zeros(1, 4, dtype=torch.long), 4, beam_size=9)


def test_prefill_that_pads_past_max_seq_is_refused():
    x = torch.randint(0, 300, (2, 90))                                              # 89 prefill rows pad to 96 > max_seq 92
    with pytest.raises(ValueError, match="max_seq=92"):
        host_model(L=92).generate_beam(x, 2, beam_size=2, prior_lengths=[90, 3])
    with pytest.raises(ValueError, match="max_seq=92"):
        host_model(L=92).generate_beam(x, 2, beam_size=2)


def test_check_beam_args_accepts_and_returns_the_prompt():
    from musicgeneration_amd import decode
    x = torch.randint(0, 300, (3, 40))
    assert decode.check_beam_args(host_model(), x, 56, 16, 0.5, None, "fp8") == (40, None)
    assert decode.check_beam_args(host_model(), x, 10, 1, 1.0, [3, 9, 5], "bf16") == (40, [3, 9, 5])
    assert decode.check_beam_args(host_model(), x, 10, 1, 1.0, [7, 7, 7], "bf16") == (7, None)


def test_beam_cli_refusals(tmp_path):
    from musicgeneration_amd import generate
    base = ["-o", str(tmp_path / "out"), "-d", "", "-B", "4"]
    for extra, msg in ((["--window", "64"], "--window"), (["--top-k", "5"], "--top-k"), (["--top-p", "0.9"], "--top-p"),
                       (["--reference-mask"], "--reference-mask")):
        with pytest.raises(SystemExit, match="cannot be combined with " + msg):
            generate.main(base + extra)
    with pytest.raises(SystemExit, match="1 .. 16"):
        generate.main(["-o", str(tmp_path / "out"), "-d", "", "-B", "17"])
    with pytest.raises(SystemExit, match="add -B"):
        generate.main(["-o", str(tmp_path / "out"), "-d", "", "-S"])
    o = generate.get_options(["-B", "3", "-S", "--kv-cache", "fp8"])
    assert (o.beam_size, o.stochastic_beam_search) == (3, True)
    generate._check_beam_options(o)                                                 # accepted
    assert generate.get_options([]).beam_size == 0                                  # off by default


# ---------------------------------------------------------------------------------------------------------------------
# the reference against brute force: a "model" whose logits are a table over every prefix
# ---------------------------------------------------------------------------------------------------------------------
def _table_model(V, steps, seed):
    rng = np.random.default_rng(seed)
    table = {p: rng.normal(size=V) * 2.0 for n in range(steps) for p in itertools.product(range(V), repeat=n)}
    return table.__getitem__, table


def _prefix_scores(table, V, steps, temperature):
    """the summed log-probability of EVERY sequence of every length, by enumeration"""
    S = {(): 0.0}
    for n in range(steps):
        for p in itertools.product(range(V), repeat=n):
            x = table[p] / temperature
            logp = x - np.log(np.exp(x).sum())
            for v in range(V):
                S[p + (v,)] = S[p] + logp[v]
    return S


@pytest.mark.parametrize("K,V,steps", [(2, 3, 3), (3, 4, 2)])
@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_reference_search_against_enumeration(K, V, steps, temperature):
    for seed in range(5):
        logits_of, table = _table_model(V, steps, seed)
        S = _prefix_scores(table, V, steps, temperature)
        beams = [()]                                                                # brute force: explicit sequences, sorted
        for _ in range(steps):
            ext = sorted((p + (v,) for p in beams for v in range(V)), key=lambda q: -S[q])
            beams = ext[:K]
        seqs, scores = beam_ref.search(logits_of, K, V, steps, temperature)
        live = np.isfinite(scores)
        assert [tuple(int(v) for v in s) for s in seqs[live]] == beams[:live.sum()], (seed, seqs, beams)
        np.testing.assert_allclose(scores[live], [S[q] for q in beams[:live.sum()]], rtol=0, atol=1e-12)
        assert live.sum() == min(K, V ** steps)
        assert np.all(np.diff(scores[live]) <= 0)                                   # slots in descending order


def test_reference_select_ties_dead_beams_and_grammar():
    V, K = 5, 3
    row = np.array([0.0, 1.0, 1.0, -1.0, 0.5])
    logits = np.stack([row, row, row])
    # two identical live beams with equal scores, one dead: exact ties go to the smaller flat index k V + v
    sel = beam_ref.select(logits, 1.0, np.array([[0.0, 0.0, -np.inf]]), np.zeros(3, int), np.array([0]))
    assert sel["flat"][0] == [1, 2, V + 1]
    assert sel["parent"][0].tolist() == [0, 0, 1] and sel["tok"][0].tolist() == [1, 2, 1]
    # a grammar that allows one id after token 0, nothing after token 1 (ignored), fewer than K candidates in total
    table = np.zeros((V, 1), np.uint32)
    table[0, 0] = 1 << 3
    sel = beam_ref.select(logits, 1.0, np.array([[0.0, -np.inf, -np.inf]]), np.array([0, 0, 0]), np.array([0]), table)
    assert sel["flat"][0] == [3] and sel["score"][0, 0] == 0.0                      # the one allowed id has probability 1
    assert sel["tok"][0].tolist() == [3, 3, 3] and sel["parent"][0].tolist() == [0, 0, 0]
    assert np.all(sel["score"][0, 1:] == -np.inf)
    sel = beam_ref.select(logits, 1.0, np.array([[0.0, -1.0, -np.inf]]), np.array([1, 0, 0]), np.array([0]), table)
    assert sorted(sel["flat"][0]) == [1, 2, V + 3]                                  # beam 0's empty row is ignored: all 5 ids
    # stochastic: the score carried is the unperturbed candidate, and the perturbation is the documented Gumbel draw
    sel = beam_ref.select(logits, 1.0, np.array([[0.0, -0.5, -np.inf]]), np.zeros(3, int), np.array([7]), None, True, 11)
    g = beam_ref.gumbel(11, np.array([7]), 1, K, V)
    assert np.array_equal(sel["key"][0, :2], sel["cand"][0, :2] + g[0, :2])
    for j, f in enumerate(sel["flat"][0]):
        assert sel["score"][0, j] == sel["cand"][0].reshape(-1)[f]
    from oracle import decode_ref as D
    u = min(float(D.u01(11, 7, (0 * K + 1) * 1024 + 4)), 1 - 2.0 ** -24)
    assert g[0, 1, 4] == -np.log(-np.log(u))


def test_reference_reorder_and_backtrack():
    rng = np.random.default_rng(0)
    src, dst = rng.integers(0, 255, (4, 2, 6, 3)), np.full((4, 2, 6, 3), -1)
    res = beam_ref.reorder(dst, src, np.array([1, 1, 0, 0]), np.array([2, 2, 6, 6]), 2)
    assert np.array_equal(res[0, :, :2], src[1, :, :2]) and np.all(res[0, :, 2:] == -1)
    assert np.array_equal(res[2], src[2]) and np.array_equal(res[3], src[2])
    ht = np.array([[9, 1, 3, 5], [9, 2, 4, 6]])                                     # one prompt, K = 2, c0 = 1, 3 steps
    hp = np.array([[9, 0, 1, 1], [9, 0, 0, 0]])
    out = beam_ref.backtrack(ht, hp, np.array([1, 1]), 3, 2, np.full((2, 4), 7))
    assert out.tolist() == [[7, 1, 4, 5], [7, 2, 3, 6]]
