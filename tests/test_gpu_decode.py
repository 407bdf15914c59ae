"""Decode path (A12): cached single-query relative attention + fused sampler vs the causal training forward."""
import math

import numpy as np
import pytest
import torch

from decode_fixtures import tame_model

pytestmark = pytest.mark.gpu


def test_cached_decode_matches_causal_forward_and_oracle():
    from oracle import ref_cpu as R
    mt, p0 = tame_model()
    V, L, B = 337, 96, 3
    g = torch.Generator().manual_seed(11)
    x = torch.randint(0, V - 1, (B, L), generator=g)
    toks, probs = mt.generate_cached(x.cuda(), 0, return_probs=True)
    torch.cuda.synchronize()
    assert (toks.cpu() == x).all()
    with torch.no_grad():
        fwd = torch.softmax(mt(x.to(torch.int32).cuda())[0].float(), -1).cpu()
        ref = torch.softmax(R.model_forward(p0, x, V - 1)[0], -1)
    assert (probs.cpu() - fwd).abs().max().item() < 1e-2          # same kernels' arithmetic, different order
    assert (probs.cpu() - ref).abs().max().item() < 2e-2          # vs the fp32 oracle (causal semantics)
    assert abs(probs.sum(-1).cpu() - 1).max().item() < 1e-4


@pytest.mark.parametrize("d,nl,B", [(128, 2, 2), (512, 6, 2)])
def test_split_key_cached_decode_matches_the_oracle_at_length_2048(d, nl, B):
    """The long-cache decode path (keys split over workgroups + merge, Lmax >= 1024) against the fp32 ORACLE, not only
    against this repo's own training forward: every one of the 2048 teacher-forced next-token distributions, for the small
    model and for the cfg2/cfg5-shaped one (d 512, 6 layers)."""
    from musicgeneration_amd import ops
    from oracle import ref_cpu as R
    V, L = 337, 2048
    assert ops.rel_attn_decode_splits(B, L, d) > 1
    mt, p0 = tame_model(d=d, nl=nl, L=L, V=V, seed=21)
    g = torch.Generator().manual_seed(23)
    x = torch.randint(0, V - 1, (B, L), generator=g)
    toks, probs = mt.generate_cached(x.cuda(), 0, return_probs=True)
    torch.cuda.synchronize()
    assert (toks.cpu() == x).all()
    with torch.no_grad():
        ref = torch.softmax(R.model_forward(p0, x, V - 1)[0], -1)
    err = (probs.cpu() - ref).abs().amax(-1)                       # [B, L]
    assert err.max().item() < 2e-2, (err.max().item(), int(err.argmax()))
    assert err[:, 1024:].mean().item() < 3e-3                      # and not merely under the cap at the long-cache end
    assert (probs.cpu().argmax(-1) == ref.argmax(-1)).float().mean().item() >= 0.97


def test_sampler_distribution_and_filters():
    from musicgeneration_amd import ops
    dev = torch.device("cuda")
    V, B = 337, 4096
    g = torch.Generator().manual_seed(3)
    row = torch.randn(V, generator=g) * 2
    logits = row.to(torch.bfloat16).repeat(B, 1).contiguous().to(dev)
    p_ref = torch.softmax(row.to(torch.bfloat16).float(), -1)
    pos = torch.zeros(1, dtype=torch.int32, device=dev)
    nxt = torch.empty(B, dtype=torch.int32, device=dev)
    probs = torch.empty(B, V, device=dev)
    ops.sample_topk_topp(logits, V, pos, nxt, None, probs, seed=7, advance=True)
    torch.cuda.synchronize()
    assert pos.item() == 1
    assert (probs[0].cpu() - p_ref).abs().max().item() < 1e-6
    cnt = torch.bincount(nxt.cpu().long(), minlength=V).float() / B
    assert (cnt - p_ref).abs().max().item() < 4 * math.sqrt(p_ref.max().item() / B) + 2e-3   # ~4 sigma
    # same (seed, step, row) -> same draw; another step -> another stream
    nxt2 = torch.empty_like(nxt)
    pos.zero_()
    ops.sample_topk_topp(logits, V, pos, nxt2, None, None, seed=7, advance=False)
    assert (nxt2 == nxt).all()
    # top-k: only the k most likely ids appear; top-p: the smallest prefix reaching p
    k = 5
    ops.sample_topk_topp(logits, V, pos, nxt, None, None, top_k=k, seed=9, advance=False)
    topk_ids = set(p_ref.topk(k).indices.tolist())
    assert set(nxt.cpu().tolist()) <= topk_ids and len(set(nxt.cpu().tolist())) == k
    sp, si = p_ref.sort(descending=True)
    n_keep = int((sp.cumsum(0) < 0.9).sum().item()) + 1
    ops.sample_topk_topp(logits, V, pos, nxt, None, None, top_p=0.9, seed=10, advance=False)
    assert set(nxt.cpu().tolist()) <= set(si[:n_keep].tolist())
    assert len(set(nxt.cpu().tolist())) >= n_keep - 2
    # temperature -> 0 is greedy
    ops.sample_topk_topp(logits, V, pos, nxt, None, None, temperature=1e-3, seed=11, advance=False)
    best = set((p_ref == p_ref.max()).nonzero().flatten().tolist())     # bf16 logits may tie at the top
    assert set(nxt.cpu().tolist()) <= best


def test_graph_replay_equals_eager_decode():
    mt, _ = tame_model(L=64)
    prior = torch.tensor([[24, 28, 31], [5, 6, 7]], device="cuda")
    a = mt.generate_cached(prior, 40, top_p=0.9, seed=123, use_graph=True).cpu()
    b = mt.generate_cached(prior, 40, top_p=0.9, seed=123, use_graph=False).cpu()
    assert a.shape == (2, 43) and (a[:, :3] == prior.cpu()).all()
    assert (a == b).all()                       # sampling is a pure function of (seed, position, row)
    c = mt.generate_cached(prior, 40, top_p=0.9, seed=124, use_graph=True).cpu()
    assert not (a == c).all()
    assert int(a.max()) < 337 and int(a.min()) >= 0
    with pytest.raises(ValueError):
        mt.generate_cached(prior, 100)          # beyond max_seq: no silent sliding window


def test_gru_step_matches_reference_golden(golden_dir):
    """Event_Melody_RNN (A13): gen_forward chain, init_to_hidden and teacher-forced logits vs golden G8."""
    import os
    from musicgeneration_amd.melody_rnn import Event_Melody_RNN
    g = dict(np.load(os.path.join(golden_dir, "g8_gru.npz")))
    net = Event_Melody_RNN(init_dim=8, event_dim=40, hidden_dim=64, rnn_layers=2, dropout=0.0)
    net.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p.")})   # reference keys
    net = net.cuda().eval()
    init = torch.from_numpy(g["init"]).cuda()
    hid = net.init_to_hidden(init)
    np.testing.assert_allclose(hid.detach().cpu().numpy(), g["hid0"], rtol=1e-4, atol=1e-5)
    for s in range(3):
        o, hid = net.gen_forward(torch.from_numpy(g[f"step{s}_event"]).cuda(), hid)
        assert np.abs(o.cpu().numpy() - g[f"step{s}_logits"]).max() < 2e-2
        assert np.abs(hid.cpu().numpy() - g[f"step{s}_hidden"]).max() < 2e-2
    tl = net.Train(init, torch.from_numpy(g["train_events"]).cuda())
    assert tl.shape == g["train_logits"].shape
    assert np.abs(tl.detach().cpu().numpy() - g["train_logits"]).max() < 3e-2


def test_gru_generate_graph_equals_eager():
    from musicgeneration_amd.melody_rnn import Event_Melody_RNN
    torch.manual_seed(0)
    net = Event_Melody_RNN(init_dim=32, event_dim=308, hidden_dim=512, rnn_layers=3, dropout=0.3).cuda().eval()
    init = torch.randn(4, 32, device="cuda")
    a = net.generate(init, 40, greedy=0.5, temperature=1.2, seed=5, use_graph=True)
    b = net.generate(init, 40, greedy=0.5, temperature=1.2, seed=5, use_graph=False)
    assert a.shape == (40, 4) and (a == b).all() and int(a.max()) < 308
    sm = net.generate(init, 3, greedy=0.0, output_type='softmax')
    assert sm.shape == (3, 4, 308) and abs(sm.sum(-1) - 1).max().item() < 1e-4


@pytest.mark.parametrize("B,T,H,nl", [(4, 12, 64, 2), (40, 9, 128, 3)])
def test_gru_train_backward_matches_oracle_autograd(B, T, H, nl):
    """Event_Melody_RNN.Train (A13 / F4): teacher-forced logits and EVERY parameter gradient (embedding, GRU weights and
    biases of all layers, output projection, init->hidden projection) of the backward-through-time kernels vs autograd
    through the oracle's fp32 restatement.  bf16 operands: logits to 3e-2, gradients by cosine >= 0.995."""
    from musicgeneration_amd.melody_rnn import Event_Melody_RNN
    from oracle import ref_cpu as R
    torch.manual_seed(3)
    V, init_dim = 52, 8
    net = Event_Melody_RNN(init_dim=init_dim, event_dim=V, hidden_dim=H, rnn_layers=nl, dropout=0.0)
    p_ref = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    init = torch.randn(B, init_dim)
    events = torch.randint(0, V, (T, B))
    target = torch.randint(0, V, (T + 1, B))
    ref = R.gru_train_logits(p_ref, init, events, nl, H, V - 1)
    torch.nn.functional.cross_entropy(ref.reshape(-1, V), target.reshape(-1)).backward()
    net = net.cuda().train()
    out = net.Train(init.cuda(), events.cuda())
    assert out.shape == ref.shape and out.requires_grad
    assert (out.detach().cpu() - ref.detach()).abs().max().item() < 3e-2
    torch.nn.functional.cross_entropy(out.reshape(-1, V), target.cuda().reshape(-1)).backward()
    for name, prm in net.named_parameters():
        assert prm.grad is not None, name
        got, want = prm.grad.detach().cpu().flatten().double(), p_ref[name].grad.flatten().double()
        cos = float(got @ want / (got.norm() * want.norm() + 1e-30))
        assert cos > 0.995, f"{name}: cos {cos}"
        assert abs(float(got.norm() / (want.norm() + 1e-30)) - 1) < 5e-2, name
    # the reference's optimizer line works on it (Event_MelodyRNN/train.py): one Adam step changes every parameter
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    before = [q.detach().clone() for q in net.parameters()]
    opt.step()
    assert all((a != b).any() for a, b in zip(before, [q.detach() for q in net.parameters()]))


def test_gru_train_dropout_is_consistent():
    """nn.GRU's inter-layer dropout: eval mode ignores it (two calls agree bit for bit), training mode applies it, a pinned
    ``dropout_seed`` repeats the mask and another seed draws another, and the gradients through the dropped path are finite.
    That the backward uses the forward's mask is checked where the masks are known, against the oracle under the same masks:
    tests/test_gpu_dropout_model.py::test_gru_training_with_inter_layer_dropout_matches_the_masked_oracle."""
    from musicgeneration_amd.melody_rnn import Event_Melody_RNN
    torch.manual_seed(5)
    net = Event_Melody_RNN(init_dim=8, event_dim=40, hidden_dim=64, rnn_layers=2, dropout=0.5).cuda()
    init, events = torch.randn(3, 8, device="cuda"), torch.randint(0, 40, (6, 3), device="cuda")
    net.eval()
    a, b = net.Train(init, events), net.Train(init, events)
    assert torch.equal(a, b)
    net.train()
    c = net.Train(init, events)
    assert not torch.allclose(c, a, atol=1e-3)                       # dropout active
    c.float().pow(2).sum().backward()
    assert all(torch.isfinite(q.grad).all() for q in net.parameters())
    with torch.no_grad():
        d, e, f = (net.Train(init, events, dropout_seed=s) for s in (11, 11, 12))
    assert torch.equal(d, e) and not torch.allclose(d, f, atol=1e-3)



def test_sampler_grammar_mask_and_constrained_generation():
    """F3: the sampling kernel honours the allow table (only allowed successors of the previous token are drawn, an empty
    row falls back to the unmasked distribution), and a graph-captured REMI generation obeys the grammar at every step."""
    from musicgeneration_amd import ops
    from musicgeneration_amd.network import MusicTransformer
    from musicgeneration_amd.REMI import REMI_EventSeq
    dev = torch.device("cuda")
    V, B = 70, 16
    W = (V + 31) // 32
    allow = np.zeros((V, W), dtype=np.uint32)
    for t in range(V):                                   # token t may be followed by t+1 or t+2 (mod V); row 5 allows nothing
        for v in ((t + 1) % V, (t + 2) % V):
            allow[t, v >> 5] |= np.uint32(1 << (v & 31))
    allow[5] = 0
    table = torch.from_numpy(allow.view(np.int32)).to(dev)
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(B, 72, generator=g).to(torch.bfloat16).to(dev)
    prev = torch.arange(B, dtype=torch.int32, device=dev)
    pos = torch.zeros(1, dtype=torch.int32, device=dev)
    for seed in range(20):
        tok = prev.clone()
        ops.sample_topk_topp(logits, V, pos, tok, None, None, 1.0, 0, 1.0, seed, advance=False, allow_table=table)
        nxt, pv = tok.cpu().numpy(), prev.cpu().numpy()
        for b in range(B):
            if pv[b] != 5:
                assert nxt[b] in ((pv[b] + 1) % V, (pv[b] + 2) % V)
            else:
                assert 0 <= nxt[b] < V
    with pytest.raises(ValueError):
        ops.sample_topk_topp(logits, V, pos, prev.clone(), allow_table=table[:, :1].contiguous())
    # end to end: REMI grammar through the graph-captured decode loop
    torch.manual_seed(0)
    Vr = REMI_EventSeq.dim() + 1
    mt = MusicTransformer(embedding_dim=128, vocab_size=Vr, num_layer=2, max_seq=128, dropout=0.0).cuda().eval()
    tab = REMI_EventSeq.next_token_table()
    bar = REMI_EventSeq.feat_ranges()['bar'][0]
    prior = torch.full((4, 1), bar, dtype=torch.long, device=dev)
    out = mt.generate_cached(prior, 100, top_p=0.95, seed=3, grammar=tab).cpu().numpy()
    assert out.shape == (4, 101)
    for row in out:
        for a, b in zip(row, row[1:]):
            assert (tab[a, b >> 5] >> np.uint32(b & 31)) & np.uint32(1), (a, b)
    free = mt.generate_cached(prior, 100, top_p=0.95, seed=3).cpu().numpy()
    viol = sum(1 for row in free for a, b in zip(row, row[1:]) if not (tab[a, b >> 5] >> np.uint32(b & 31)) & np.uint32(1))
    assert viol > 0                                   # an untrained model breaks the grammar without the mask


def test_gru_beam_search_is_exact_when_the_beam_is_wide_enough():
    """F4: a beam of V^(steps-1) keeps every prefix, so the search is exhaustive and must return the arg-max over ALL
    V^steps sequences of the sequence log-probability (scored independently by stepping gen_forward over every sequence
    from the same initial hidden state); a narrower beam can never beat that optimum; beam 1 is greedy decoding."""
    import itertools
    from musicgeneration_amd.melody_rnn import Event_Melody_RNN
    torch.manual_seed(2)
    V, steps, B = 5, 3, 3
    net = Event_Melody_RNN(init_dim=8, event_dim=V, hidden_dim=64, rnn_layers=2, dropout=0.0).cuda().eval()
    for q in net.parameters():
        q.data.mul_(3.0)                                  # peaked distributions: well separated sequence scores
    init = torch.randn(B, 8, device="cuda")
    hid0 = net.init_to_hidden(init).detach()                                       # [layers, B, H]
    allseq = torch.tensor(list(itertools.product(range(V), repeat=steps)), device="cuda")       # [n, steps]
    n = allseq.shape[0]
    total = torch.zeros(B, n, device="cuda")
    for b in range(B):
        hid = hid0[:, b:b + 1].repeat(1, n, 1).contiguous()
        ev = net.get_primary_event(n)
        for t in range(steps):
            logits, hid = net.gen_forward(ev, hid)
            total[b] += torch.log_softmax(logits[0], -1).gather(-1, allseq[:, t:t + 1]).squeeze(-1)
            ev = allseq[:, t][None, :]
    exact = allseq[total.argmax(-1)]                                                             # [B, steps]
    wide = net.beam_search(init, steps, beam_size=V)            # clamps at event_dim: exhaustive needs V^(steps-1) > V,
    # so run the exhaustive case on 2 steps (beam V = V^(2-1)) and the bound on 3 steps
    two = net.beam_search(init, 2, beam_size=V).t()
    tot2 = torch.zeros(B, V * V, device="cuda")
    seq2 = torch.tensor(list(itertools.product(range(V), repeat=2)), device="cuda")
    for b in range(B):
        hid = hid0[:, b:b + 1].repeat(1, V * V, 1).contiguous()
        ev = net.get_primary_event(V * V)
        for t in range(2):
            logits, hid = net.gen_forward(ev, hid)
            tot2[b] += torch.log_softmax(logits[0], -1).gather(-1, seq2[:, t:t + 1]).squeeze(-1)
            ev = seq2[:, t][None, :]
    assert torch.equal(two, seq2[tot2.argmax(-1)])                                               # exhaustive == exact
    got = wide.t()
    for b in range(B):
        idx = (allseq == got[b]).all(-1).nonzero()[0, 0]
        assert total[b, idx] <= total[b].max() + 1e-3                                            # never beats the optimum
        assert total[b, idx] >= total[b, (allseq == net.beam_search(init, steps, 1).t()[b]).all(-1).nonzero()[0, 0]] - 1e-3
    assert torch.equal(net.beam_search(init, steps, beam_size=1), net.generate(init, steps, greedy=1.0, use_graph=False))
    # stochastic variant returns valid sequences and is seed-deterministic
    s1 = net.beam_search(init, steps, beam_size=3, stochastic=True, seed=4)
    s2 = net.beam_search(init, steps, beam_size=3, stochastic=True, seed=4)
    assert torch.equal(s1, s2) and s1.shape == (steps, B) and int(s1.max()) < V


def test_cfg5_sized_cached_decode_matches_training_forward():
    """BASELINE cfg5's size (seq_len 8192, batch 32, cfg2-shaped model): the KV-cache decode path, teacher-forced over the
    whole sequence, gives the same next-token distributions as the training forward on the same prefix -- checked at
    positions 1, 4095 and 8191 (cache of 1, 4096 and 8192 rows) for every batch row."""
    mt, _ = tame_model(d=512, nl=6, L=8192, V=337, seed=5)
    V, L, B = 337, 8192, 32
    g = torch.Generator().manual_seed(55)
    x = torch.randint(0, V - 1, (B, L), generator=g).cuda()
    toks, probs = mt.generate_cached(x, 0, return_probs=True)
    torch.cuda.synchronize()
    assert (toks == x).all()
    with torch.no_grad():
        logits = mt(x.to(torch.int32))[0]
    for pos in (1, 4095, 8191):
        fwd = torch.softmax(logits[:, pos].float(), -1)
        got = probs[:, pos]
        assert torch.isfinite(got).all() and abs(got.sum(-1) - 1).max().item() < 1e-3
        assert (got - fwd).abs().max().item() < 1e-2, pos
        assert (got.argmax(-1) == fwd.argmax(-1)).float().mean().item() >= 0.9, pos


def test_gru_train_packed_lengths_matches_torch_packed_gru():
    """Event_Melody_RNN.Train(init, X, lengths) -- the reference's `sequence` mode (network.py:63-84, train.py:263-287):
    against torch's own pack_padded_sequence -> nn.GRU -> pad_packed_sequence -> output_fc on the CPU in fp32, with the
    same weights: valid steps match, steps past a row's end hold output_fc(0), the flattened rows pair with SeqBatchify's
    labels, and every parameter gradient of the label loss agrees."""
    from musicgeneration_amd.data import SeqBatchify, flatten_padded_sequences
    from musicgeneration_amd.melody_rnn import Event_Melody_RNN
    torch.manual_seed(8)
    V, init_dim, H, nl = 52, 8, 64, 2
    net = Event_Melody_RNN(init_dim=init_dim, event_dim=V, hidden_dim=H, rnn_layers=nl, dropout=0.0)
    g = np.random.RandomState(8)
    seqs = [g.randint(0, V - 1, size=n) for n in (11, 7, 11, 3, 9)]
    X, Y, lengths = SeqBatchify(seqs)
    B, Tmax = X.shape
    init = torch.randn(B, init_dim)
    # ---- torch reference (CPU, fp32), same parameters
    ref = Event_Melody_RNN(init_dim=init_dim, event_dim=V, hidden_dim=H, rnn_layers=nl, dropout=0.0)
    ref.load_state_dict(net.state_dict())
    gru = torch.nn.GRU(V, H, num_layers=nl)
    gru.load_state_dict({k[len("rnn."):]: v for k, v in ref.state_dict().items() if k.startswith("rnn.")})
    for p in list(gru.parameters()) + [ref.event_embedding.weight, ref.output_fc.weight, ref.output_fc.bias,
                                       ref.inithid_fc.weight, ref.inithid_fc.bias]:
        p.requires_grad_(True)
    hid0 = torch.tanh(torch.nn.functional.linear(init, ref.inithid_fc.weight, ref.inithid_fc.bias)).view(nl, B, H)
    prim = torch.full((1, B), ref.primary_event, dtype=torch.long)
    out1, hid1 = gru(ref.event_embedding(prim), hid0)
    emb = ref.event_embedding(torch.from_numpy(X.astype(np.int64)).t())                 # [Tmax, B, E]
    packed = torch.nn.utils.rnn.pack_padded_sequence(emb, torch.as_tensor(lengths), batch_first=False)
    outp, _ = gru(packed, hid1)
    outp, _ = torch.nn.utils.rnn.pad_packed_sequence(outp, total_length=Tmax)              # zero past each row's end
    want = torch.nn.functional.linear(torch.cat([out1, outp], 0), ref.output_fc.weight, ref.output_fc.bias).transpose(0, 1)
    # ---- the kernels
    net = net.cuda().train()
    got = net.Train(init.cuda(), torch.from_numpy(X.astype(np.int64)).cuda(), lengths)
    assert got.shape == want.shape == (B, Tmax + 1, V)
    assert (got.detach().cpu() - want.detach()).abs().max().item() < 3e-2
    for i, n in enumerate(lengths):                       # steps past the end: exactly output_fc(0) = the bias
        if n < Tmax:
            assert torch.equal(got[i, n + 1:].detach().cpu(), net.output_fc.bias.detach().cpu().to(got.dtype).expand(Tmax - n, V))
    # loss as the reference's sequence mode pairs it: row t of sample i (after consuming X[i, :t]) predicts X[i, t] ...
    # the label vector of SeqBatchify is X[i, 1:len_i]: logits after the primary event and X[i, 0..t-1] -> steps 1..len-1
    lab = torch.from_numpy(Y.astype(np.int64))
    lw = flatten_padded_sequences(want[:, 1:], lengths)
    lg = flatten_padded_sequences(got[:, 1:], lengths)
    assert lw.shape == lg.shape == (int(sum(lengths) - B), V) and lab.numel() == lw.shape[0]
    torch.nn.functional.cross_entropy(lw, lab).backward()
    torch.nn.functional.cross_entropy(lg, lab.cuda()).backward()
    refg = {"event_embedding.weight": ref.event_embedding.weight.grad, "output_fc.weight": ref.output_fc.weight.grad,
            "output_fc.bias": ref.output_fc.bias.grad, "inithid_fc.weight": ref.inithid_fc.weight.grad}
    refg.update({"rnn." + k: v.grad for k, v in gru.named_parameters()})
    for name, prm in net.named_parameters():
        if name not in refg:
            continue
        a, b = prm.grad.detach().cpu().flatten().double(), refg[name].flatten().double()
        cos = float(a @ b / (a.norm() * b.norm() + 1e-30))
        assert cos > 0.99, f"{name}: cos {cos}"
    with pytest.raises(ValueError):
        net.Train(init.cuda(), torch.from_numpy(X.astype(np.int64)).t().cuda(), lengths)     # time-major + lengths: refused


@pytest.mark.parametrize("P", [33, 80, 96])
def test_batched_prefill_fills_the_same_caches_as_token_by_token(P):
    """A prompt goes through the full-sequence kernels in one pass (prefill='batched'): every layer's K/V cache rows and
    the first sampled distribution must agree with teacher-forcing the prompt one decode step at a time."""
    mt, _ = tame_model(L=128)
    V, B = 337, 2
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, V - 1, (B, P), generator=g).cuda()
    (ta, pa), ka, va = mt.generate_cached(x, 1, top_k=1, return_probs=True, prefill="token", return_cache=True)
    tb, kb, vb = mt.generate_cached(x, 1, top_k=1, prefill="batched", return_cache=True)
    torch.cuda.synchronize()
    for i in range(len(ka)):
        for a, b, nm in ((ka[i], kb[i], "K"), (va[i], vb[i], "V")):
            a, b = a[:, :, :P].float(), b[:, :, :P].float()          # caches are [B, h, total, 64]
            rel = (a - b).abs().max().item() / a.abs().max().item()
            assert rel < 2e-2, f"layer {i} {nm} cache: relative difference {rel:.3e}"
    # the token sampled after the prompt: greedy, so equal unless the top two probabilities are within kernel noise
    p_last = pa[:, P - 1]
    top2 = p_last.topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > 2e-2
    assert (ta[:, P][clear] == tb[:, P][clear]).all()
    assert (ta[:, :P] == tb[:, :P]).all()
    with pytest.raises(ValueError):
        mt.generate_cached(x, 1, return_probs=True, prefill="batched")


def test_decode_embed_linear_matches_the_two_kernels_it_replaces():
    """mgx_decode_embed_linear (ABI 12) == mgx_decode_embed -> mgx_linear_fwd: the embedding rows bit for bit, the projection
    to one bf16 rounding of the output."""
    from musicgeneration_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(31)
    bf = torch.bfloat16
    for (B, d) in ((32, 512), (5, 256)):
        V = 97
        table = torch.randn(V, d, generator=g).to(dev)
        pe = torch.randn(64, d, generator=g).to(dev)
        tok = torch.randint(0, V, (B,), generator=g, dtype=torch.int32).to(dev)
        pos = torch.tensor([17], dtype=torch.int32, device=dev)
        wq = (torch.randn(3 * d, d, generator=g) / d ** 0.5).to(bf).to(dev)
        bq = (0.1 * torch.randn(3 * d, generator=g)).to(dev)
        h1 = torch.empty(B, d, dtype=bf, device=dev)
        q1, _ = ops.decode_embed_linear(tok, table, pe, pos, wq, bq, h1)
        h0 = ops.decode_embed(tok, table, pe, pos, torch.empty(B, d, dtype=bf, device=dev))
        q0 = ops.linear_fwd(h0, wq, bq, 0)
        torch.cuda.synchronize()
        assert torch.equal(h1, h0)
        assert (q1.float() - q0.float()).abs().max().item() <= 2 ** -7 * q0.float().abs().max().item()


def test_cfg5_sized_graph_replay_equals_eager_greedy():
    """The CAPTURED decode step at BASELINE cfg5's size (cache of 8192 rows -> split-K attention + merge, batch 32): greedy
    (top_k = 1) continuation of a 7,900-token prompt for 64 tokens by graph replay equals the eager launches token for token
    -- the graph path at size is asserted, not only shape-checked.  (The prompt is prefilled in one batched pass both
    times, so the two runs start from identical caches.)"""
    mt, _ = tame_model(d=512, nl=6, L=8192, V=337, seed=5)
    V, B, P, n = 337, 32, 7900, 64
    g = torch.Generator().manual_seed(56)
    prompt = torch.randint(0, V - 1, (B, P), generator=g).cuda()
    a = mt.generate_cached(prompt, n, top_k=1, seed=3, use_graph=True, prefill="batched")
    b = mt.generate_cached(prompt, n, top_k=1, seed=3, use_graph=False, prefill="batched")
    torch.cuda.synchronize()
    assert a.shape == (B, P + n) and (a[:, :P] == prompt).all()
    same = (a[:, P:] == b[:, P:]).float().mean().item()
    # greedy tokens are a deterministic function of the logits; the only run-to-run noise is none (no atomics on this path)
    assert same == 1.0, same


@pytest.mark.parametrize("B,H", [(100, 512), (5, 64), (33, 128), (130, 64)])
def test_gru_fused_step_kernels_match_the_two_kernel_path(B, H):
    """mgx_gru_step_fwd / mgx_gru_step_bwd (recurrent projection + cell in one launch) against the kernels they replace
    (mgx_linear_fwd / mgx_linear_dx + mgx_gru_cell_fwd / _bwd): the same bf16 rounding points, so they agree to the
    fp32 summation order of the projection (one bf16 ulp where a rounding flips)."""
    from musicgeneration_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(B * 7 + H)
    bf = torch.bfloat16
    whh = (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(bf).to(dev)
    bhh = (torch.randn(3 * H, generator=g) * 0.1).to(dev)
    gi = torch.randn(B, 3 * H, generator=g).to(bf).to(dev)
    h_prev = (torch.randn(B, H, generator=g) * 0.5).to(dev)
    hp_bf = h_prev.to(bf)
    # forward
    gh_ref = ops.linear_fwd(hp_bf, whh, bhh, 0)
    hn_ref, y_ref = torch.empty_like(h_prev), torch.empty_like(hp_bf)
    ops.gru_cell_fwd(gi, gh_ref, h_prev, hn_ref, y_ref)
    hn, y, gh = torch.empty_like(h_prev), torch.empty_like(hp_bf), torch.empty_like(gi)
    ops.gru_step_fwd(gi, hp_bf, h_prev, ops.pack_frag(whh), bhh, hn, y, gh)
    torch.cuda.synchronize()
    assert (gh.float() - gh_ref.float()).abs().max().item() <= 2 ** -7 * gh_ref.float().abs().max().item()
    assert (hn - hn_ref).abs().max().item() <= 2e-2
    assert ((hn - hn_ref).norm() / hn_ref.norm()).item() < 2e-3
    # backward (a middle step: every input present) and the final d_h0 step
    dgh_next = (torch.randn(B, 3 * H, generator=g) * 0.1).to(bf).to(dev)
    dh_dir = (torch.randn(B, H, generator=g) * 0.1).to(dev)
    dy = (torch.randn(B, H, generator=g) * 0.1).to(bf).to(dev)
    d_rec = ops.linear_dx(dgh_next, whh)
    dgi_r, dgh_r, dd_r = torch.empty_like(gi), torch.empty_like(gi), torch.empty_like(h_prev)
    ops.gru_cell_bwd(gi, gh_ref, h_prev, dh_dir, d_rec, dy, dgi_r, dgh_r, dd_r)
    dgi, dgh, dd, d0 = torch.empty_like(gi), torch.empty_like(gi), torch.empty_like(h_prev), torch.empty_like(h_prev)
    whh_t = ops.pack_frag(whh.t())
    ops.gru_step_bwd(gi, gh_ref, h_prev, dh_dir, dgh_next, whh_t, dy, dgi, dgh, dd)
    ops.gru_step_bwd(None, None, None, dh_dir, dgh_next, whh_t, None, None, None, d0, final=True)
    torch.cuda.synchronize()
    for got, ref in ((dgi, dgi_r), (dgh, dgh_r), (dd, dd_r), (d0, dh_dir + d_rec.float())):
        got, ref = got.float(), ref.float()
        assert ((got - ref).norm() / ref.norm()).item() < 4e-3
        assert (got - ref).abs().max().item() <= 2e-2 * ref.abs().max().item()
    # first backward step of a sequence: no d_rec, no dh_direct
    ops.gru_cell_bwd(gi, gh_ref, h_prev, None, None, dy, dgi_r, dgh_r, dd_r)
    ops.gru_step_bwd(gi, gh_ref, h_prev, None, None, whh_t, dy, dgi, dgh, dd)
    torch.cuda.synchronize()
    for got, ref in ((dgi, dgi_r), (dgh, dgh_r), (dd, dd_r)):      # pure cell arithmetic: equal up to fma contraction
        assert (got.float() - ref.float()).abs().max().item() <= 2 ** -7 * ref.float().abs().max().item()
        assert ((got.float() - ref.float()).norm() / ref.float().norm()).item() < 1e-3


def test_gru_train_graph_replay_equals_eager_and_survives_an_optimizer_step(monkeypatch):
    """Train's time loops replayed from hipGraphs give the same logits and gradients as the eager launches, and the graphs
    stay valid after the parameters change (the bf16 operand copies are refreshed in place).  Forwards of the same shape before
    the backward of an earlier one -- ``(loss1 + loss2).backward()``, an evaluation in between -- get their own sequence buffers
    (the patterns the reference's nn.GRU allows): gradients equal the sum of two separate backward passes."""
    from musicgeneration_amd.melody_rnn import Event_Melody_RNN
    torch.manual_seed(3)
    V, H, B, T = 40, 64, 6, 9
    net = Event_Melody_RNN(init_dim=8, event_dim=V, hidden_dim=H, rnn_layers=2, dropout=0.0).cuda()
    init = torch.randn(B, 8, device="cuda")
    ev = torch.randint(0, V, (T, B), device="cuda")

    def grads():
        net.zero_grad()
        out = net.Train(init, ev)
        (out.float() ** 2).mean().backward()
        return out.detach().clone(), [p.grad.detach().clone() for p in net.parameters()]

    monkeypatch.setenv("MGX_GRU_GRAPH", "0")
    net._train_ws = {}
    out_e, g_e = grads()
    monkeypatch.setenv("MGX_GRU_GRAPH", "1")
    net._train_ws = {}
    grads()                                                  # call 1 captures
    out_g, g_g = grads()                                     # call 2 replays
    assert torch.equal(out_e, out_g)
    for a, b in zip(g_e, g_g):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-7)     # dW kernels add M-splits with fp32 atomics: order varies
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.01)
    out_g2, _ = grads()                                      # replayed graphs read the refreshed operand copies
    monkeypatch.setenv("MGX_GRU_GRAPH", "0")
    net._train_ws = {}
    out_e2, _ = grads()
    assert torch.equal(out_e2, out_g2) and not torch.equal(out_e2, out_e)
    monkeypatch.setenv("MGX_GRU_GRAPH", "1")
    net._train_ws = {}
    ev2 = torch.randint(0, V, (T, B), device="cuda")
    sep = []
    for e_ in (ev, ev2):
        net.zero_grad()
        (net.Train(init, e_).float() ** 2).mean().backward()
        sep.append([p.grad.detach().clone() for p in net.parameters()])
    net.zero_grad()
    o1 = net.Train(init, ev)
    with torch.no_grad():
        ev_out = net.Train(init, ev2)                        # an evaluation between forward and backward: leases nothing
    o2 = net.Train(init, ev2)                                # a second grad-enabled forward of the same shape: another buffer set
    o3 = net.Train(init, ev)                                 # ... a third ...
    o4 = net.Train(init, ev2)                                # ... and a fourth (beyond the kept sets: throw-away buffers, eager)
    assert torch.equal(ev_out, o2.detach()) and torch.equal(o1.detach(), o3.detach()) and torch.equal(o2.detach(), o4.detach())
    ((o1.float() ** 2).mean() + (o2.float() ** 2).mean()).backward()
    for gsum, a, b in zip([p.grad for p in net.parameters()], sep[0], sep[1]):
        assert torch.allclose(gsum, a + b, rtol=1e-4, atol=1e-6)
    assert len(net._train_ws[(T + 1, B)]) == 3
    del o3, o4                                               # never back-propagated: freeing the graph hands the buffers back
    assert sum(w["busy"] for w in net._train_ws[(T + 1, B)]) == 0
    with pytest.raises(RuntimeError, match="twice"):
        out = net.Train(init, ev)
        loss = out.sum()
        loss.backward(retain_graph=True)
        loss.backward()


@pytest.mark.parametrize("B,H,Kx", [(32, 512, 320), (5, 64, 64), (40, 128, 192)])
def test_gru_fused_sampling_step_matches_the_three_kernel_path(B, H, Kx):
    """mgx_gru_step_x_fwd (both projections + the cell, one launch) against mgx_linear_fwd x 2 + mgx_gru_gates."""
    from musicgeneration_amd import ops
    from musicgeneration_amd._lib import check, ptr, stream_ptr, load
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(B + H + Kx)
    bf = torch.bfloat16
    wih = (torch.randn(3 * H, Kx, generator=g) / Kx ** 0.5).to(bf).to(dev)
    whh = (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(bf).to(dev)
    bih, bhh = (torch.randn(3 * H, generator=g) * 0.1).to(dev), (torch.randn(3 * H, generator=g) * 0.1).to(dev)
    x = torch.randn(B, Kx, generator=g).to(bf).to(dev)
    h = (torch.randn(B, H, generator=g) * 0.5).to(dev)
    hb = h.to(bf)
    h_ref, hb_ref = h.clone(), hb.clone()
    gi, gh = ops.linear_fwd(x, wih, bih, 0), ops.linear_fwd(hb_ref, whh, bhh, 0)
    check(load().mgx_gru_gates(ptr(gi), ptr(gh), ptr(h_ref), ptr(hb_ref), B, H, stream_ptr()), "mgx_gru_gates")
    hn, y = torch.empty_like(h), torch.empty_like(hb)
    ops.gru_step_x_fwd(x, ops.pack_frag(wih), bih, hb, h, ops.pack_frag(whh), bhh, hn, y)
    torch.cuda.synchronize()
    assert (hn - h_ref).abs().max().item() <= 2e-2
    assert ((hn - h_ref).norm() / h_ref.norm()).item() < 2e-3
    assert (y.float() - hb_ref.float()).abs().max().item() <= 3e-2
    with pytest.raises(ops._lib.MgxError):
        ops.gru_step_x_fwd(x, ops.pack_frag(wih), bih, hb, h, ops.pack_frag(whh), bhh, h, y)      # in place is refused


@pytest.mark.parametrize("use_graph", [False, True])
def test_decode_row_groups_on_streams_give_the_same_tokens(use_graph):
    """generate_cached(groups=G): the batch as G independent sub-batches on forked streams (joined per step, one graph).  Rows
    never interact and the sampler draws by (seed, step, GLOBAL row), so every grouping returns the same tokens -- bitwise
    below the split-key length (the number of key splits depends on the sub-batch size, the per-row arithmetic otherwise
    not).  A ragged grouping (B=7 in 3 groups) is part of the sweep."""
    mt, _ = tame_model(d=128, nl=2, L=160, V=337, seed=31)
    g = torch.Generator().manual_seed(5)
    for B, groups in ((8, (2, 4)), (7, (3,))):
        prior = torch.randint(0, 336, (B, 3), generator=g).cuda()
        ref = mt.generate_cached(prior, 150, top_p=0.95, seed=77, use_graph=use_graph, groups=1)
        for G in groups:
            got = mt.generate_cached(prior, 150, top_p=0.95, seed=77, use_graph=use_graph, groups=G)
            torch.cuda.synchronize()
            assert torch.equal(got, ref), (B, G)
    assert len(set(ref[:, -1].tolist())) > 1                       # rows are not copies of each other


@pytest.mark.parametrize("d,L", [(192, 70), (64, 40)])
def test_cached_decode_at_odd_head_counts_and_lengths_matches_the_oracle(d, L):
    """round 6: the KV-cache decode engine on a model whose FFN width is zero-padded inside the flat buffers (d = 192: 3 heads, FFN
    96; d = 64: one head, FFN 32) and whose max_seq is no multiple of 32 -- the per-token distributions of a teacher-forced sequence
    against the training forward (same kernels' arithmetic) and the fp32 oracle, then a batched-prefill run giving the same tokens as the
    token-by-token prefill"""
    from musicgeneration_amd.network import MusicTransformer
    from oracle import ref_cpu as R
    V, nl, B = 90, 2, 3
    p0 = R.init_params(V, d, nl, L, seed=9)
    for k in p0:
        if k.endswith("embedding.weight") or k.endswith("rga.E"):
            p0[k] = p0[k] * 0.2
    mt = MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=nl, max_seq=L, dropout=0.0)
    mt.load_state_dict(p0)
    mt = mt.cuda().eval()
    g = torch.Generator().manual_seed(12)
    x = torch.randint(0, V - 1, (B, L), generator=g)
    toks, probs = mt.generate_cached(x.cuda(), 0, return_probs=True)
    torch.cuda.synchronize()
    assert (toks.cpu() == x).all()
    with torch.no_grad():
        fwd = torch.softmax(mt(x.to(torch.int32).cuda())[0].float(), -1).cpu()
        ref = torch.softmax(R.model_forward(p0, x, V - 1)[0], -1)
    assert (probs.cpu() - fwd).abs().max().item() < 1e-2
    assert (probs.cpu() - ref).abs().max().item() < 2e-2
    P = L - 20
    a = mt.generate_cached(x[:, :P].cuda(), 20, top_k=1, seed=3, prefill="token")
    assert tuple(a.shape) == (B, L) and int(a.max()) < V
    if (P - 1 + 31) // 32 * 32 <= L:
        b = mt.generate_cached(x[:, :P].cuda(), 20, top_k=1, seed=3, prefill="batched")
        # greedy continuation: the two prefill paths fill the caches through different GEMM kernels (bf16 rounding), so a near-tie may
        # flip late in the sequence; the first sampled tokens agree
        assert (a[:, :P + 4] == b[:, :P + 4]).all()
