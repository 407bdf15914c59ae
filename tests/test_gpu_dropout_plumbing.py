"""Which dropout seed reaches which kernel call.  The kernels' mask is a pure function of (seed, element index) and is checked bit
for bit against its integer twin elsewhere; what decides whether a model trains under the masks it is meant to is the Python
above them.  Here the four entry points that take (p_drop, seed) -- ops.embed_pe_fwd, ops.add_ln_fwd, ops.embed_bwd,
ops.add_ln_bwd -- are wrapped to record what they are handed, and a forward and backward of MusicTransformer (the flat path), of
the stand-alone Encoder and of one EncoderLayer must show:
  * within one forward, 2 * layers + 1 sites (embedding, LayerNorm 1 and 2 of every layer) with 2 * layers + 1 different seeds;
  * over three training forwards, no seed twice;
  * every backward call with the (p, seed) of its forward call;
  * p = 0 everywhere in eval mode.
The seed arithmetic alone, over many more calls and ranks, is tests/test_host_logic.py::test_dropout_site_seeds_never_collide_...;
the values a step computes under these masks are tests/test_gpu_dropout_model.py."""
import inspect

import pytest
import torch

from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401

pytestmark = pytest.mark.gpu

D, L, B, V, RATE = 64, 32, 2, 30, 0.2


@pytest.fixture
def calls(monkeypatch):
    """name -> [(p_drop, seed)] of every call of the four entry points, in call order"""
    from musicgeneration_amd import ops
    log = {n: [] for n in ("embed_pe_fwd", "add_ln_fwd", "embed_bwd", "add_ln_bwd")}
    for name in log:
        orig = getattr(ops, name)
        sig = inspect.signature(orig)

        def spy(*a, _orig=orig, _sig=sig, _name=name, **k):
            b = _sig.bind(*a, **k)
            b.apply_defaults()
            log[_name].append((float(b.arguments["p_drop"]), int(b.arguments["seed"])))
            return _orig(*a, **k)
        monkeypatch.setattr(ops, name, spy)
    return log


def _clear(log):
    for v in log.values():
        v.clear()


def _check_one_step(log, nl, embed):
    """one forward + backward is in the log: -> the forward's site seeds"""
    fwd = ([] if not embed else log["embed_pe_fwd"]) + log["add_ln_fwd"]
    assert len(log["add_ln_fwd"]) == 2 * nl and len(log["embed_pe_fwd"]) == (1 if embed else 0)
    assert all(p == pytest.approx(RATE) for p, _ in fwd), fwd
    seeds = [s for _, s in fwd]
    assert len(set(seeds)) == len(seeds), f"two sites of one forward share a seed: {seeds}"
    # the backward runs the sites in reverse, each under its forward's (p, seed)
    assert log["add_ln_bwd"] == log["add_ln_fwd"][::-1]
    assert log["embed_bwd"] == log["embed_pe_fwd"]
    return seeds


def _tokens():
    g = torch.Generator().manual_seed(0)
    return torch.randint(0, V - 1, (B, L), generator=g).cuda()


def _look_ahead(tok):
    from musicgeneration_amd import utils
    return utils.get_masked_with_pad_tensor(L, tok.cpu(), tok.cpu(), V - 1)[2].cuda()


@pytest.mark.parametrize("nl", (1, 2, 17))
def test_music_transformer_gives_every_site_of_every_step_its_own_seed(calls, nl):
    from musicgeneration_amd.network import MusicTransformer
    torch.manual_seed(0)
    mt = MusicTransformer(embedding_dim=D, vocab_size=V, num_layer=nl, max_seq=L, dropout=RATE).cuda().train()
    x = _tokens()
    every = []
    for step in range(3):
        _clear(calls)
        mt(x).float().square().mean().backward()
        seeds = _check_one_step(calls, nl, embed=True)
        # the plan: embedding s, layer i LayerNorm 1 s + 4 i + 1, LayerNorm 2 s + 4 i + 2
        s = seeds[0]
        assert seeds[1:] == [s + 4 * i + k for i in range(nl) for k in (1, 2)]
        every += seeds
    assert len(set(every)) == len(every), "a later step reuses a seed of an earlier one"
    _clear(calls)
    mt.eval()
    with torch.no_grad():
        mt(x)
    assert len(calls["add_ln_fwd"]) == 2 * nl and all(p == 0.0 for v in calls.values() for p, _ in v)


def test_stand_alone_encoder_gives_every_layer_its_own_seeds(calls):
    from musicgeneration_amd.layers import Encoder
    torch.manual_seed(0)
    nl = 3
    enc = Encoder(num_layers=nl, d_model=D, input_vocab_size=V, rate=RATE, max_len=L).cuda().train()
    x = _tokens()
    lam = _look_ahead(x)
    every = []
    for step in range(3):
        _clear(calls)
        hid, _ = enc(x, lam)
        hid.square().mean().backward()
        every += _check_one_step(calls, nl, embed=True)
    assert len(set(every)) == len(every), "a later step reuses a seed of an earlier one"
    _clear(calls)
    enc.eval()
    with torch.no_grad():
        enc(x, lam)
    assert len(calls["add_ln_fwd"]) == 2 * nl and all(p == 0.0 for v in calls.values() for p, _ in v)


def test_a_lone_encoder_layer_still_draws_its_own_seeds(calls):
    from musicgeneration_amd.layers import EncoderLayer
    torch.manual_seed(0)
    layer = EncoderLayer(D, rate=RATE, h=1, max_seq=L).cuda().train()
    tok = _tokens()
    lam = _look_ahead(tok)
    x = torch.randn(B, L, D, device="cuda", requires_grad=True)
    every = []
    for step in range(3):
        _clear(calls)
        out, _ = layer(x, lam)
        out.square().mean().backward()
        every += _check_one_step(calls, 1, embed=False)
    assert len(set(every)) == len(every)
    _clear(calls)
    layer.eval()
    with torch.no_grad():
        layer(x, lam)
    assert len(calls["add_ln_fwd"]) == 2 and all(p == 0.0 for v in calls.values() for p, _ in v)
