"""KV-cache decode over prompts of different lengths (ABI 19): with per_row set the decode kernels read one position per batch row, and
generate_cached(prior_lengths=...) continues right-padded prompts of different lengths in one lockstep batch."""
import glob
import os

import numpy as np
import pytest
import torch

from decode_fixtures import check_rows, one, prompt_file, ragged_prior, tame_model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16


def _positions(B, Lmax, g):
    """per-row positions with rows at t = 0, t < 64 and t near Lmax - 1, the rest random"""
    pos = torch.randint(0, Lmax, (B,), generator=g, dtype=torch.int32)
    pos[0], pos[1], pos[2], pos[3] = 0, 37, Lmax - 1, Lmax - 2
    return pos.to(DEV)


# ---------------------------------------------------------------------------------------------------------------------
# kernel level: row b of a ragged call == row b of the shared-position call at t = pos[b], bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def test_ragged_embed_and_embed_qkv_match_the_shared_position_kernels_rowwise():
    from musicgeneration_amd import ops
    g = torch.Generator().manual_seed(1)
    B, d, V, Lmax = 9, 256, 97, 300
    table = torch.randn(V, d, generator=g).to(DEV)
    pe = torch.randn(Lmax, d, generator=g).to(DEV)
    tok = torch.randint(0, V, (B,), generator=g, dtype=torch.int32).to(DEV)
    pos = _positions(B, Lmax, g)
    wq = (torch.randn(3 * d, d, generator=g) / d ** 0.5).to(BF).to(DEV)
    bq = (0.1 * torch.randn(3 * d, generator=g)).to(DEV)
    wf = ops.FragWeight(wq)
    h = ops.decode_embed(tok, table, pe, pos, torch.empty(B, d, dtype=BF, device=DEV), ragged=True)
    outs = {w_name: ops.decode_embed_linear(tok, table, pe, pos, w, bq, torch.empty(B, d, dtype=BF, device=DEV), ragged=True)
            for w_name, w in (("plain", wq), ("frag", wf))}
    for b in range(B):
        h0 = ops.decode_embed(tok, table, pe, one(pos[b]), torch.empty(B, d, dtype=BF, device=DEV))
        assert torch.equal(h[b], h0[b]), b
        for w_name, w in (("plain", wq), ("frag", wf)):
            q0, hh0 = ops.decode_embed_linear(tok, table, pe, one(pos[b]), w, bq, torch.empty(B, d, dtype=BF, device=DEV))
            q1, hh1 = outs[w_name]
            assert torch.equal(q1[b], q0[b]) and torch.equal(hh1[b], hh0[b]), (w_name, b)
    assert not torch.equal(h[0], h[2])                            # the rows did read different positions
    with pytest.raises(ValueError):
        ops.decode_embed(tok, table, pe, pos[:3], torch.empty(B, d, dtype=BF, device=DEV), ragged=True)


@pytest.mark.parametrize("Lmax,B", [(300, 6), (2048, 6)])
def test_ragged_attention_matches_the_shared_position_kernel_rowwise(Lmax, B):
    """one split (Lmax < 1024) and split-K (Lmax = 2048, short rows leave whole splits empty): the context row and the two
    cache rows the step appends"""
    from musicgeneration_amd import ops
    d, M = 256, Lmax + 16
    if Lmax >= 1024:
        assert ops.rel_attn_decode_splits(B, Lmax, d) > 1
    g = torch.Generator().manual_seed(Lmax)
    pos = _positions(B, Lmax, g)
    qkv = torch.randn(B, 3 * d, generator=g).to(BF).to(DEV)
    kc0 = torch.randn(B, d // 64, Lmax, 64, generator=g).to(BF).to(DEV)
    vc0 = torch.randn(B, d // 64, Lmax, 64, generator=g).to(BF).to(DEV)
    E = (0.3 * torch.randn(M, 64, generator=g)).to(BF).to(DEV)
    ws = ops.rel_attn_decode_workspace(B, Lmax, d, DEV)
    kc, vc = kc0.clone(), vc0.clone()
    ctx = ops.rel_attn_decode(qkv, kc, vc, E, pos, torch.empty(B, d, dtype=BF, device=DEV), ws, ragged=True)
    for b in range(B):
        k1, v1 = kc0.clone(), vc0.clone()
        c1 = ops.rel_attn_decode(qkv, k1, v1, E, one(pos[b]), torch.empty(B, d, dtype=BF, device=DEV), ws)
        assert torch.equal(ctx[b], c1[b]), b
        assert torch.equal(kc[b], k1[b]) and torch.equal(vc[b], v1[b]), b
    assert torch.isfinite(ctx.float()).all()


@pytest.mark.parametrize("grammar", [False, True])
def test_ragged_sampler_and_advance_match_the_shared_position_kernel_rowwise(grammar):
    from musicgeneration_amd import ops
    g = torch.Generator().manual_seed(7)
    B, V, Lmax = 10, 337, 200
    pos = _positions(B, Lmax - 1, g)                              # the token goes to column pos + 1 < Lmax
    logits = (2 * torch.randn(B, 384, generator=g)).to(BF).to(DEV)
    prev = torch.randint(0, V, (B,), generator=g, dtype=torch.int32).to(DEV)
    table = None
    if grammar:                                                   # token t may be followed by t+1 .. t+40 only
        allow = np.zeros((V, (V + 31) // 32), dtype=np.uint32)
        for t in range(V):
            for v in range(t + 1, t + 41):
                allow[t, (v % V) >> 5] |= np.uint32(1) << np.uint32(v % 32)
        table = torch.from_numpy(allow.view(np.int32)).to(DEV)
    out0 = torch.randint(0, V, (B, Lmax), generator=g, dtype=torch.int32).to(DEV)
    nt, out, probs, p = prev.clone(), out0.clone(), torch.zeros(B, V, device=DEV), pos.clone()
    ops.sample_topk_topp(logits, V, p, nt, out, probs, 0.9, 50, 0.95, 1234, advance=True, allow_table=table, row0=3, ragged=True)
    for b in range(B):
        nt1, out1, probs1, p1 = prev.clone(), out0.clone(), torch.zeros(B, V, device=DEV), one(pos[b])
        ops.sample_topk_topp(logits, V, p1, nt1, out1, probs1, 0.9, 50, 0.95, 1234, advance=True, allow_table=table, row0=3)
        assert nt[b] == nt1[b] and torch.equal(out[b], out1[b]) and torch.equal(probs[b], probs1[b]), b
        assert out[b, pos[b] + 1] == nt[b]
    assert torch.equal(p, pos + 1)                                # every row advanced by one
    if grammar:
        for b in range(B):
            assert 1 <= (int(nt[b]) - int(prev[b])) % V <= 40


# ---------------------------------------------------------------------------------------------------------------------
# generate_cached(prior_lengths=...)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("prefill", ["batched", "auto"])
def test_equal_prior_lengths_are_bitwise_the_uniform_call(prefill, use_graph):
    mt, _ = tame_model(L=128)
    V, B, P, n = 337, 3, 40, 30
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, V - 1, (B, P), generator=g).cuda()
    kw = dict(top_p=0.9, seed=5, use_graph=use_graph, prefill=prefill, return_cache=True)
    ta, ka, va = mt.generate_cached(x, n, **kw)
    tb, kb, vb = mt.generate_cached(x, n, prior_lengths=[P] * B, **kw)
    assert torch.equal(ta, tb)
    assert all(torch.equal(a, b) for a, b in zip(ka + va, kb + vb))
    if prefill == "auto":                                         # probabilities need the token prefill of the uniform path
        ra, pa = mt.generate_cached(x, n, top_p=0.9, seed=5, use_graph=use_graph, return_probs=True)
        rb, pb = mt.generate_cached(x, n, top_p=0.9, seed=5, use_graph=use_graph, return_probs=True,
                                    prior_lengths=torch.tensor([P] * B))
        assert torch.equal(ra, rb) and torch.equal(pa, pb)
    # equal lengths below the width of prior: the same call on prior[:, :P], padded to Pmax + length
    wide = torch.cat([x, torch.full((B, 6), 11, device=x.device)], 1)
    tc, kc, vc = mt.generate_cached(wide, n, prior_lengths=[P] * B, **kw)
    assert tc.shape == (B, P + 6 + n) and torch.equal(tc[:, :P + n], ta) and (tc[:, P + n:] == mt.pad_token).all()
    assert all(torch.equal(c[:, :, :P + n], a) and not c[:, :, P + n:].any() for a, c in zip(ka + va, kc + vc))


def test_ragged_prompts_match_the_forward_and_the_oracle_per_row():
    mt, p0 = tame_model()
    V, n = 337, 20
    lens = [1, 5, 33, 70]
    g = torch.Generator().manual_seed(17)
    x = ragged_prior(lens, V, g)
    toks, probs = mt.generate_cached(x.cuda(), n, top_p=0.95, seed=9, return_probs=True, prior_lengths=lens)
    torch.cuda.synchronize()
    check_rows(mt, p0, x, lens, 1, n, toks, probs, V)


@pytest.mark.parametrize("d,nl", [(128, 2), (512, 6)])
def test_ragged_prompts_on_the_split_key_path_match_the_oracle(d, nl):
    from musicgeneration_amd import ops
    V, L, n = 337, 2048, 24
    lens = [1, 33, 700, 1500]
    assert ops.rel_attn_decode_splits(len(lens), max(lens) + n, d) > 1
    mt, p0 = tame_model(d=d, nl=nl, L=L, V=V, seed=21)
    g = torch.Generator().manual_seed(29)
    x = ragged_prior(lens, V, g)
    toks, probs = mt.generate_cached(x.cuda(), n, top_p=0.95, seed=4, return_probs=True, prior_lengths=lens)
    torch.cuda.synchronize()
    check_rows(mt, p0, x, lens, 1, n, toks, probs, V)


def test_ragged_prompts_without_the_fused_step_match_the_forward():
    """B > 32: the step runs the unfused kernels (decode_embed, linear_fwd, add_ln_fwd) with per-row positions"""
    mt, _ = tame_model(L=96)
    V, n, B = 337, 12, 34
    g = torch.Generator().manual_seed(41)
    lens = torch.randint(1, 60, (B,), generator=g).tolist()
    lens[0], lens[1] = 1, 60
    x = ragged_prior(lens, V, g)
    toks, probs = mt.generate_cached(x.cuda(), n, top_k=20, seed=2, return_probs=True, prior_lengths=lens)
    toks, probs = toks.cpu(), probs.cpu()
    for b in (0, 1, 7, 33):
        P = lens[b]
        assert torch.equal(toks[b, :P], x[b, :P].to(torch.int32)) and (toks[b, P + n:] == mt.pad_token).all()
        with torch.no_grad():
            fwd = torch.softmax(mt(toks[b:b + 1, :P + n].cuda())[0].float(), -1).cpu()[0, P - 1:P + n - 1]
        assert (probs[b, P - 1:P + n - 1] - fwd).abs().max().item() < 1e-2, b


def test_ragged_graph_replay_and_row_groups_are_bitwise_the_eager_single_group_run():
    mt, _ = tame_model(d=128, nl=2, L=160, V=337, seed=31)
    g = torch.Generator().manual_seed(8)
    lens = [3, 1, 40, 17, 64, 2, 9]
    x = ragged_prior(lens, 337, g).cuda()
    ref = mt.generate_cached(x, 90, top_p=0.95, seed=77, use_graph=False, prior_lengths=lens)
    for use_graph in (False, True):
        for G in (1, 2, 3):
            got = mt.generate_cached(x, 90, top_p=0.95, seed=77, use_graph=use_graph, groups=G, prior_lengths=lens)
            torch.cuda.synchronize()
            assert torch.equal(got, ref), (use_graph, G)
    assert len(set(ref[:, 70].tolist())) > 1
    # the caches a row's decode never reached are zero, as in the uniform case
    _, kc, vc = mt.generate_cached(x, 5, top_p=0.95, seed=77, prior_lengths=lens, return_cache=True)
    for b, P in enumerate(lens):
        assert not kc[0][b, :, P + 4:].any() and kc[0][b, :, P + 3].any(), b


def test_ragged_prompts_with_a_grammar():
    from musicgeneration_amd.REMI import REMI_EventSeq
    from musicgeneration_amd.network import MusicTransformer
    torch.manual_seed(0)
    Vr = REMI_EventSeq.dim() + 1
    mt = MusicTransformer(embedding_dim=128, vocab_size=Vr, num_layer=2, max_seq=128, dropout=0.0).cuda().eval()
    tab = REMI_EventSeq.next_token_table()
    bar = REMI_EventSeq.feat_ranges()['bar'][0]
    # grammatical prompts of 1, 2 and 4 events: prefixes of constrained samples
    ref = mt.generate_cached(torch.full((3, 1), bar, device=DEV), 10, top_p=0.95, seed=1, grammar=tab).cpu()
    lens = [1, 2, 4]
    prior = ref[:, :4].long().clone()
    out = mt.generate_cached(prior.cuda(), 60, top_p=0.95, seed=3, grammar=tab, prior_lengths=lens).cpu().numpy()
    for row, P in zip(out, lens):
        seq = row[P - 1:P + 60]                                   # the last prompt token and the sampled ones
        for a, b in zip(seq, seq[1:]):
            assert (tab[a, b >> 5] >> np.uint32(b & 31)) & np.uint32(1), (a, b)


def test_ragged_refusals_on_the_device():
    mt, _ = tame_model(L=96)
    x = torch.randint(0, 300, (3, 40)).cuda()
    for lens, kw in (([0, 5, 40], {}), ([41, 5, 40], {}), ([1, 5, 40], dict(length=57)), ([1, 5, 40], dict(prefill="token"))):
        with pytest.raises(ValueError):
            mt.generate_cached(x, kw.pop("length", 10), prior_lengths=lens, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# generate.py --condition-files
# ---------------------------------------------------------------------------------------------------------------------
def test_generate_cli_continues_each_condition_file_in_one_batch(tmp_path, capsys):
    from musicgeneration_amd import generate
    from musicgeneration_amd.sequence import NoteSeq
    a, b = str(tmp_path / "a.mid"), str(tmp_path / "b.mid")
    notes = {a: prompt_file(a, 3, 60), b: prompt_file(b, 11, 48)}
    out = str(tmp_path / "gen") + "/"
    torch.manual_seed(0)
    generate.main(["-o", out, "-b", "5", "-l", "24", "--num-layers", "1", "--d-model", "128", "-M", "128", "-d", "",
                   "--top-p", "0.9", "--condition-files", f"{a},{b}"])
    log = capsys.readouterr().out
    assert log.count("Prompt:") == 2
    files = sorted(glob.glob(out + "gen-*.mid"))
    assert [os.path.basename(f) for f in files] == ["gen-000.mid", "gen-001.mid"]      # one per file, -b ignored
    for f, src in zip(files, (a, b)):
        got = sorted(NoteSeq.from_midi_file(f).notes, key=lambda n_: (n_.start, n_.pitch))
        want = notes[src]
        last = want[-1][2]
        head = [(n_.pitch, round(n_.start, 2)) for n_ in got if n_.start < last - 1e-3]
        assert head == [(p, round(s, 2)) for _, p, s, _ in want[:-1]], f
