"""KV-cache decode past max_seq (ABI 21): generate_cached(window=, hop=) keeps a window of every row's sequence in the cache
and re-anchors it every ``hop`` tokens -- the oldest tokens dropped, the rest renumbered from position 0 and their K/V rebuilt
by one batched causal pass.  The sampler's base (mgx_sample_topk_topp's base_dev) and mgx_decode_reanchor are what it adds to the C ABI."""
import glob
import os

import numpy as np
import pytest
import torch

from decode_fixtures import ragged_prior, tame_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
V = 337


_MODEL = []


def _shared_model():
    """one model (max_seq 96) for the whole file: no test changes it"""
    if not _MODEL:
        _MODEL.append(tame_model())
    return _MODEL[0]


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _flat(res):
    """every tensor of a generate_cached result, in order"""
    if torch.is_tensor(res):
        return [res]
    return [t for r in res for t in _flat(r)]


def _same(a, b):
    a, b = _flat(a), _flat(b)
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x.view(torch.uint8) if x.dtype == torch.float8_e4m3fn else x,
                                                                       y.view(torch.uint8) if y.dtype == torch.float8_e4m3fn else y)
                                    for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the two entries
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grammar", [False, True])
@pytest.mark.parametrize("per_row", [False, True])
def test_window_sampler_is_the_sampler_at_the_absolute_step(per_row, grammar):
    """pos = t and base = c give, bit for bit, what the sampler without a base gives at position c + t (c = 0: a base of zeros
    is no base, the header's sentence, for the shared counter and for per-row positions); advance moves pos only"""
    from musicgeneration_amd import ops
    g = torch.Generator().manual_seed(11)
    B, out_ld = 6, 1100
    logits = (2 * torch.randn(B, 384, generator=g)).to(BF).to(DEV)
    prev = torch.randint(0, V, (B,), generator=g, dtype=torch.int32).to(DEV)
    table = None
    if grammar:                                                   # token t may be followed by t+1 .. t+40 only
        allow = np.zeros((V, (V + 31) // 32), dtype=np.uint32)
        for t in range(V):
            for v in range(t + 1, t + 41):
                allow[t, (v % V) >> 5] |= np.uint32(1) << np.uint32(v % 32)
        table = torch.from_numpy(allow.view(np.int32)).to(DEV)
    out0 = torch.randint(0, V, (B, out_ld), generator=g, dtype=torch.int32).to(DEV)
    kw = dict(temperature=0.9, top_k=50, top_p=0.95, seed=1234, advance=True, allow_table=table, row0=3)
    for c in (0, 7, 1000):
        last = out_ld - c - 2                                     # the token then goes to the last column
        if per_row:
            cases = [([0, last, 5, 37, last - 1, 1], [c] * B), ([3, 0, last, 9, 2, last], [c, c, c, 0, c + 1, c])]
        else:
            cases = [([0], [c]), ([last], [c]), ([41], [c])]
        for t, base in cases:
            pos, bs = _i32(t), _i32(base)
            nt, out, probs = prev.clone(), out0.clone(), torch.zeros(B, V, device=DEV)
            ops.sample_topk_topp(logits, V, pos, nt, out, probs, ragged=per_row, base=bs, **kw)
            pos1 = _i32([a + b for a, b in zip(t, base)])
            nt1, out1, probs1 = prev.clone(), out0.clone(), torch.zeros(B, V, device=DEV)
            ops.sample_topk_topp(logits, V, pos1, nt1, out1, probs1, ragged=per_row, **kw)
            assert torch.equal(nt, nt1) and torch.equal(out, out1) and torch.equal(probs, probs1), (c, t)
            assert torch.equal(pos, _i32(t) + 1) and torch.equal(bs, _i32(base)), (c, t)
            for b in range(B):
                col = (t[b] + base[b] if per_row else t[0] + base[0]) + 1
                assert out[b, col] == nt[b]
            if c:                                                 # the base does enter the draw
                nt2 = prev.clone()
                ops.sample_topk_topp(logits, V, _i32(t), nt2, None, None, ragged=per_row, **kw)
                assert not torch.equal(nt2, nt), (c, t)
    with pytest.raises(ValueError, match="base"):
        ops.sample_topk_topp(logits, V, _i32([0] * B), prev.clone(), ragged=True, base=_i32([0]), **kw)


@pytest.mark.parametrize("hop", [1, 16])
@pytest.mark.parametrize("per_row", [False, True])
def test_reanchor_kernel_moves_the_window_and_gathers_its_tokens(per_row, hop):
    from musicgeneration_amd import ops
    g = torch.Generator().manual_seed(5)
    B, out_ld, n_pad, pad = 5, 80, 64, 336
    out = torch.randint(0, V - 1, (B, out_ld), generator=g, dtype=torch.int32).to(DEV)
    # rows whose new t is 0; n_pad above every t'
    for t_new, base in [([0, 5, 40, 50, 33], [0, 3, 7, 1, 10])] if per_row else [([40], [7]), ([0], [0]), ([63], [0])]:
        pos_d, base_d = _i32([v + hop for v in t_new]), _i32(base)
        seq = torch.full((B, n_pad), -1, dtype=torch.int32, device=DEV)
        out_before = out.clone()
        ops.decode_reanchor(pos_d, base_d, out, seq, hop, pad, ragged=per_row)
        assert pos_d.tolist() == t_new and base_d.tolist() == [v + hop for v in base]
        assert torch.equal(out, out_before)
        want = torch.full((B, n_pad), pad, dtype=torch.int32, device=DEV)
        for b in range(B):
            t, c = (t_new[b], base[b] + hop) if per_row else (t_new[0], base[0] + hop)
            want[b, :t] = out[b, c:c + t]
        assert torch.equal(seq, want), t_new
    if not per_row:                                               # one shared position
        with pytest.raises(ValueError):
            ops.decode_reanchor(_i32([3, 3]), _i32([0, 0]), out, seq, hop, pad)


# ---------------------------------------------------------------------------------------------------------------------
# 3: a window that is never filled is today's call
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_window_without_a_reanchor_is_bitwise_the_batched_call(kv, use_graph):
    mt, _ = _shared_model()
    B, P, n = 3, 40, 30
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, V - 1, (B, P), generator=g).cuda()
    kw = dict(top_p=0.9, seed=5, use_graph=use_graph, prefill="batched", return_cache=True, kv_cache=kv)
    ref = mt.generate_cached(x, n, **kw)
    for W in (P + n, 96):                                         # the window exactly filled by the last token, and a larger one
        got = mt.generate_cached(x, n, window=W, **kw)
        assert _same(got, ref), W
    # prompts of different lengths: the distributions too
    lens = [9, 20, 30]
    xr = ragged_prior(lens, V, g).cuda()
    kw = dict(top_p=0.9, seed=5, use_graph=use_graph, prior_lengths=lens, return_cache=True, kv_cache=kv)
    assert _same(mt.generate_cached(xr, 40, window=80, **kw), mt.generate_cached(xr, 40, **kw))
    kw.update(return_probs=True)
    (ta, pa), *ca = mt.generate_cached(xr, 40, **kw)
    (tb, pb), *cb = mt.generate_cached(xr, 40, window=70, hop=3, **kw)
    assert torch.equal(ta, tb) and torch.equal(pa, pb) and _same(ca, cb)


# ---------------------------------------------------------------------------------------------------------------------
# 4: every step is the causal forward of its window
# ---------------------------------------------------------------------------------------------------------------------
WINDOWS = [
    ([5, 5], 40, 16, 100),                  # 105 columns > max_seq 96; the re-anchor's 24 rows pad to 32
    ([5, 5], 12, 1, 30),                    # the reference's slide by one token: 22 re-anchors
    ([70, 70], 48, 12, 60),                 # a prompt longer than the window
    ([96, 96], 96, 32, 40),                 # window = max_seq
    ([9, 20, 30], 48, 16, 80),              # prompts of different lengths
]


def _run(mt, lens, W, hop, n, kv, g, **kw):
    x = ragged_prior(lens, V, g)
    ragged = dict(prior_lengths=lens) if min(lens) != max(lens) else {}
    return x, mt.generate_cached(x.cuda(), n, window=W, hop=hop, kv_cache=kv, top_p=0.95, seed=9, **ragged, **kw)


@pytest.mark.parametrize("kv", ["bf16", "fp8"])
@pytest.mark.parametrize("lens,W,hop,n", WINDOWS)
def test_every_step_is_the_causal_forward_of_its_window(lens, W, hop, n, kv):
    """the bounds of test_gpu_ragged_decode.py for the same comparison: 1e-2 against the model's own forward (bf16 cache),
    2e-2 against the fp32 CPU oracle (both caches)"""
    from musicgeneration_amd.decode import window_schedule
    from oracle import ref_cpu as R
    mt, p0 = _shared_model()
    x, (toks, probs) = _run(mt, lens, W, hop, n, kv, torch.Generator().manual_seed(17), return_probs=True)
    torch.cuda.synchronize()
    toks, probs = toks.cpu(), probs.cpu()
    Pmax = max(lens)
    assert toks.shape == (len(lens), Pmax + n) and probs.shape == (len(lens), Pmax + n, V)
    bases, ts, anchors = window_schedule(lens, n, W, hop)
    assert len(anchors) == {(40, 16): 4, (12, 1): 22, (48, 12): 5, (96, 32): 2, (48, 16): 4}[(W, hop)]
    worst_fwd = worst_ref = 0.0
    for b, P in enumerate(lens):
        assert torch.equal(toks[b, :P], x[b, :P].to(torch.int32)), b               # the prompt comes back unchanged
        assert (toks[b, P + n:] == mt.pad_token).all(), b                          # then length samples, then padding
        assert int(toks[b, P:P + n].max()) < V and int(toks[b, P:P + n].min()) >= 0
        assert not probs[b, :P - 1].any() and not probs[b, P + n - 1:].any(), b
        for s in range(n):
            base, t = bases[s][b], ts[s][b]
            win = toks[b:b + 1, base:base + t + 1]
            got = probs[b, P - 1 + s]
            with torch.no_grad():
                ref = torch.softmax(R.model_forward(p0, win.long(), V - 1)[0], -1)[0, t]
                worst_ref = max(worst_ref, (got - ref).abs().max().item())
                if kv == "bf16":
                    fwd = torch.softmax(mt(win.cuda())[0].float(), -1).cpu()[0, t]
                    worst_fwd = max(worst_fwd, (got - fwd).abs().max().item())
    print(f"window {W} hop {hop} lens {lens} {kv}: max |p - forward| {worst_fwd:.3e}, max |p - oracle| {worst_ref:.3e}")
    assert worst_fwd < 1e-2
    assert worst_ref < 2e-2


# ---------------------------------------------------------------------------------------------------------------------
# 5: a re-anchor is a fresh start
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv", ["bf16", "fp8"])
def test_a_reanchor_is_bitwise_a_fresh_start_from_the_window(kv):
    """the first distribution after a re-anchor == what a new call reports for the window's tokens as ragged prompts"""
    from musicgeneration_amd import ops
    from musicgeneration_amd.decode import window_schedule
    mt, _ = _shared_model()
    lens, W, hop, n = WINDOWS[-1]
    _, (toks, probs) = _run(mt, lens, W, hop, n, kv, torch.Generator().manual_seed(17), return_probs=True)
    bases, ts, anchors = window_schedule(lens, n, W, hop)
    assert len(anchors) == 4
    for s in anchors:
        base, t = bases[s], ts[s]
        assert max(t) == W - hop
        # with one split per (b, h) for both cache lengths the two calls add up the same keys in the same order
        assert ops.rel_attn_decode_splits(len(lens), W, 128) == 1 and ops.rel_attn_decode_splits(len(lens), max(t) + 2, 128) == 1
        prior = torch.full((len(lens), max(t) + 1), -3, dtype=torch.int64, device=DEV)
        for b in range(len(lens)):
            prior[b, :t[b] + 1] = toks[b, base[b]:base[b] + t[b] + 1]
        _, fresh = mt.generate_cached(prior, 1, prior_lengths=[v + 1 for v in t], return_probs=True, kv_cache=kv, top_p=0.95, seed=1)
        for b, P in enumerate(lens):
            assert torch.equal(fresh[b, t[b]], probs[b, P - 1 + s]), (s, b)


# ---------------------------------------------------------------------------------------------------------------------
# 6: graph replay, repeatability, and the random numbers of consecutive segments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens,W,hop,n", [WINDOWS[0], WINDOWS[2], WINDOWS[4]])
def test_window_graph_replay_is_bitwise_the_eager_run_and_repeats(lens, W, hop, n):
    from musicgeneration_amd.decode import window_schedule
    mt, _ = _shared_model()
    g = torch.Generator().manual_seed(23)
    x = ragged_prior(lens, V, g).cuda()
    kw = dict(window=W, hop=hop, top_p=0.95)
    if min(lens) != max(lens):
        kw.update(prior_lengths=lens)
    eager = mt.generate_cached(x, n, seed=77, use_graph=False, **kw)
    graph = mt.generate_cached(x, n, seed=77, use_graph=True, **kw)
    again = mt.generate_cached(x, n, seed=77, use_graph=True, **kw)
    other = mt.generate_cached(x, n, seed=78, use_graph=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(graph, eager) and torch.equal(again, graph)
    assert not torch.equal(other, graph)
    # two consecutive segments sample at the same window positions; their draws take base + t, so they are not the same numbers
    _, ts, anchors = window_schedule(lens, n, W, hop)
    a, b = [(a, b) for a, b in zip(anchors, anchors[1:]) if b + hop <= n][-1]       # the last two whole segments
    assert b - a == hop and ts[a] == ts[b]
    for row, P in enumerate(lens):
        assert not torch.equal(graph[row, P + a:P + b], graph[row, P + b:P + b + hop]), row


# ---------------------------------------------------------------------------------------------------------------------
# 7: grammar
# ---------------------------------------------------------------------------------------------------------------------
def test_window_with_a_grammar_keeps_every_pair_allowed():
    from musicgeneration_amd.REMI import REMI_EventSeq
    from musicgeneration_amd.decode import window_schedule
    from musicgeneration_amd.network import MusicTransformer
    torch.manual_seed(0)
    Vr = REMI_EventSeq.dim() + 1
    mt = MusicTransformer(embedding_dim=128, vocab_size=Vr, num_layer=2, max_seq=64, dropout=0.0).cuda().eval()
    tab = REMI_EventSeq.next_token_table()
    bar = REMI_EventSeq.feat_ranges()['bar'][0]
    # grammatical prompts of 1, 2 and 4 events: prefixes of constrained samples
    ref = mt.generate_cached(torch.full((3, 1), bar, device=DEV), 10, top_p=0.95, seed=1, grammar=tab).cpu()
    lens, n = [1, 2, 4], 90
    assert len(window_schedule(lens, n, 32, 8)[2]) == 8                             # 94 columns > max_seq 64
    prior = ref[:, :4].long().clone()
    out = mt.generate_cached(prior.cuda(), n, top_p=0.95, seed=3, grammar=tab, prior_lengths=lens, window=32, hop=8).cpu().numpy()
    for row, P in zip(out, lens):
        seq = row[P - 1:P + n]                                    # the last prompt token and the sampled ones, re-anchors included
        for a, b in zip(seq, seq[1:]):
            assert (tab[a, b >> 5] >> np.uint32(b & 31)) & np.uint32(1), (a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 8: generate.py --window
# ---------------------------------------------------------------------------------------------------------------------
def test_generate_cli_window_lifts_the_length_refusal(tmp_path, capsys):
    from musicgeneration_amd import generate, smf
    files = []
    for name, n_notes, pitch0 in (("a.mid", 3, 60), ("b.mid", 6, 48)):           # 14 and 29 MIDI-like events
        files.append(str(tmp_path / name))
        smf.write_notes(files[-1], [(80, pitch0 + (i % 12), 0.5 * i, 0.5 * i + 0.25) for i in range(n_notes)])
    out = str(tmp_path / "gen") + "/"
    argv = ["-o", out, "-l", "100", "--num-layers", "1", "--d-model", "128", "-M", "96", "-d", "", "--top-p", "0.9",
            "--condition-files", ",".join(files)]
    with pytest.raises(SystemExit, match="exceeds -M 96"):
        generate.main(argv)
    assert not glob.glob(out + "gen-*.mid")
    torch.manual_seed(0)
    generate.main(argv + ["--window", "40", "--hop", "16"])
    assert capsys.readouterr().out.count("Prompt:") == 4
    assert [os.path.basename(f) for f in sorted(glob.glob(out + "gen-*.mid"))] == ["gen-000.mid", "gen-001.mid"]
