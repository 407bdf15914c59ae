"""decode.decode_session: every KV-cache decode driver leaves ``model.training`` as it found it, also when it is left by an
exception.  The exception here is a Python one raised on the host in place of a kernel launch; nothing goes wrong on the device."""
import pytest
import torch

pytestmark = pytest.mark.gpu

V, B, P, LENGTH = 337, 2, 4, 3
DRIVERS = {
    "cached": lambda mt, x: mt.generate_cached(x, LENGTH, seed=1),
    "window": lambda mt, x: mt.generate_cached(x, LENGTH, seed=1, window=16),
    "shared": lambda mt, x: mt.generate_cached(x, LENGTH, seed=1, samples_per_prompt=2),
    "beam": lambda mt, x: mt.generate_beam(x, LENGTH, beam_size=2),
}


@pytest.fixture(scope="module")
def model():
    from musicgeneration_amd.network import MusicTransformer
    torch.manual_seed(0)
    return MusicTransformer(embedding_dim=128, vocab_size=V, num_layer=2, max_seq=64, dropout=0.0).cuda()


@pytest.fixture(scope="module")
def prior():
    return torch.randint(0, V - 1, (B, P), generator=torch.Generator().manual_seed(0)).cuda()


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("driver", list(DRIVERS))
def test_the_mode_is_as_it_was_after_the_call(model, prior, driver, training):
    model.train(training)
    res = DRIVERS[driver](model, prior)
    torch.cuda.synchronize()
    toks = res[0] if driver == "beam" else res
    assert toks.shape == (B * 2 if driver == "shared" else B, P + LENGTH)
    assert model.training is training


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("driver", list(DRIVERS))
def test_the_mode_is_as_it_was_after_an_exception(model, prior, driver, training, monkeypatch):
    from musicgeneration_amd import ops
    calls = []

    def refuse(*args, **kw):
        calls.append(1)
        raise RuntimeError("raised on the host before the launch")
    monkeypatch.setattr(ops, "beam_select" if driver == "beam" else "sample_topk_topp", refuse)
    model.train(training)
    with pytest.raises(RuntimeError, match="raised on the host before the launch"):
        DRIVERS[driver](model, prior)
    torch.cuda.synchronize()
    assert calls == [1]                                                      # the driver stopped at the first step
    assert model.training is training
