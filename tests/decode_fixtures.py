"""What a model-level test of the KV-cache decode needs: the tamed model with its reference parameters, ragged prompts, the per-row
check of a generate_cached result against the training forward and the CPU oracle, and the prompt files of the generate.py
tests.  Imported by basename, like beam_ref / clip_ref / score_ref."""
import torch


def tame_model(d=128, nl=2, L=96, V=337, seed=0):
    """-> (the model on the device, in eval mode; its parameters as the oracle takes them)"""
    from musicgeneration_amd.network import MusicTransformer
    from oracle import ref_cpu as R
    p0 = R.init_params(V, d, nl, L, seed=seed)
    # tame the random-init logits (N(0,1)*sqrt(d) embeddings give near one-hot attention, the worst case for
    # bf16): decode-vs-forward parity is about the kernels, not about that fixture
    p0["Decoder.embedding.weight"] = p0["Decoder.embedding.weight"] * 0.1
    for k in list(p0):
        if k.endswith("rga.E"):
            p0[k] = p0[k] * 0.2
    mt = MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=nl, max_seq=L, dropout=0.0)
    mt.load_state_dict(p0)
    return mt.cuda().eval(), p0


def host_model(L=96, V=337, d=128):
    """a one-layer model that stays on the CPU, for the argument checks: any device work on it would raise"""
    from musicgeneration_amd.network import MusicTransformer
    return MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=1, max_seq=L, dropout=0.0)


def ragged_prior(lens, V, g, fill=-7):
    B, Pmax = len(lens), max(lens)
    x = torch.randint(0, V - 1, (B, Pmax), generator=g)
    for b, n in enumerate(lens):
        x[b, n:] = fill                                           # ignored: anything may sit in the padding
    return x


def one(t):
    return torch.tensor([int(t)], dtype=torch.int32, device="cuda:0")


def check_rows(mt, p0, x, lens, N, n, toks, probs, V, rows=None, oracle=True, forward=True):
    """row b * N + k: its prompt, n samples, pad_token; its distributions against the forward and the oracle on its own tokens"""
    from oracle import ref_cpu as R
    toks, probs = toks.cpu(), probs.cpu()
    Pmax = x.shape[1]
    assert toks.shape == (len(lens) * N, Pmax + n) and probs.shape == (len(lens) * N, Pmax + n, V)
    for r in (range(len(lens) * N) if rows is None else rows):
        P = lens[r // N]
        assert torch.equal(toks[r, :P], x[r // N, :P].to(torch.int32)), r          # the prompt comes back unchanged
        assert (toks[r, P + n:] == mt.pad_token).all(), r                          # then n samples, then padding
        assert int(toks[r, P:P + n].max()) < V
        seq = toks[r:r + 1, :P + n].long()
        span = slice(P - 1, P + n - 1)                                             # the distributions after P-1 .. P+n-2
        assert not probs[r, :P - 1].any() and not probs[r, P + n - 1:].any(), r
        got = probs[r, span]
        with torch.no_grad():
            if forward:
                fwd = torch.softmax(mt(seq.to(torch.int32).cuda())[0].float(), -1).cpu()[0, span]
                assert (got - fwd).abs().max().item() < 1e-2, r
            if oracle:
                ref = torch.softmax(R.model_forward(p0, seq, V - 1)[0], -1)[0, span]
                assert (got - ref).abs().max().item() < 2e-2, r


def prompt_file(path, n_notes, pitch0):
    from musicgeneration_amd import smf
    notes = [(80, pitch0 + (i % 12), 0.5 * i, 0.5 * i + 0.25) for i in range(n_notes)]
    smf.write_notes(path, notes)
    return notes
