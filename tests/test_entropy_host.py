"""Host side of entropy-aware sampling (decode.EntropySampling, generate.py's --min-p / --typical-p / --mirostat flags, ABI 34): the
fp64 reference (tests/entropy_ref.py) on hand-made rows; every refusal, which runs before any device work and so without a GPU;
what the check returns; and the header's declarations."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import entropy_ref
from decode_fixtures import host_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 337


def _es(**kw):
    from musicgeneration_amd import decode
    return decode.EntropySampling(**dict(dict(min_p=0.05), **kw))


# ---- the reference on hand-made rows --------------------------------------------------------------------------------------------
def _kept(p, **kw):
    kept, _, margins = entropy_ref.mask_row(np.log(np.asarray(p, dtype=np.float64)), 1.0, **kw)
    return np.flatnonzero(kept).tolist(), margins


def test_reference_stages_are_sequential():
    """p = (0.4, 0.06 x 10): on one common p the typical set at 0.5 is the ten small ids and min-p 0.2 keeps id 0 -- an empty
    intersection.  In sequence min-p leaves id 0, and the typical set of one id is that id"""
    p = [0.4] + [0.06] * 10
    assert _kept(p, typical_p=0.5)[0] == list(range(1, 11))
    assert _kept(p, min_p=0.2)[0] == [0]
    kept, margins = _kept(p, min_p=0.2, typical_p=0.5)
    assert kept == [0]
    assert abs(margins["min_p"] - abs(np.log(0.06 / 0.4) - np.log(0.2))) < 1e-12
    assert margins["typical_gap"] == np.inf and abs(margins["typical_over"] - 1.0) < 1e-12
    assert abs(margins["typical_under"] - 1.0) < 1e-12


def test_reference_min_p():
    p = np.array([0.5, 0.25, 0.1, 0.1, 0.04, 0.01])
    assert _kept(p, min_p=0.3)[0] == [0, 1]
    assert _kept(p, min_p=0.15)[0] == [0, 1, 2, 3]
    kept, margins = _kept(p, min_p=0.05)
    assert kept == [0, 1, 2, 3, 4] and abs(margins["min_p"] - np.log(0.04 / 0.025)) < 1e-12      # the cut is at 0.025
    x = np.log(p) * 2.0                                                       # the cut is on the distribution at the temperature
    kept, lse, _ = entropy_ref.mask_row(x, 2.0, min_p=0.15)
    assert np.flatnonzero(kept).tolist() == [0, 1, 2, 3] and abs(lse) < 1e-12


def test_reference_typical():
    """surprises 1, 2, 3, 3 bits: H = 1.75 bits, d = (0.75, 0.25, 1.25, 1.25) bits -- id 1 first, then id 0, then the tie"""
    p = [0.5, 0.25, 0.125, 0.125]
    assert _kept(p, typical_p=0.2)[0] == [1]
    kept, margins = _kept(p, typical_p=0.5)
    assert kept == [0, 1]
    assert abs(margins["typical_over"] - 0.5) < 1e-12 and abs(margins["typical_under"] - 0.5) < 1e-12
    assert abs(margins["typical_gap"] - 0.5 * np.log(2)) < 1e-12
    assert _kept(p, typical_p=0.8)[0] == [0, 1, 2, 3]                         # equal d: the tie is kept together
    assert _kept(p, typical_p=1.0) == ([0, 1, 2, 3], {})


def test_reference_mirostat_and_its_fallback():
    p = [0.5, 0.25, 0.125, 0.125]
    kept, margins = _kept(p, mu=2.5)
    assert kept == [0, 1] and abs(margins["mirostat"] - 0.5) < 1e-12
    assert _kept(p, mu=3.5)[0] == [0, 1, 2, 3]
    assert _kept(p, mu=0.5)[0] == [0]                                         # nothing is that unsurprising: the arg-max
    assert _kept([0.3, 0.3, 0.2, 0.2], mu=-1.0)[0] == [0, 1]                  # ... and its ties
    # after the cut, min-p and typical work on the survivors: q = (2/3, 1/3) over ids 0, 1
    assert _kept(p, mu=2.5, min_p=0.6)[0] == [0]
    assert _kept(p, mu=2.5, typical_p=0.5)[0] == [0]


def test_reference_grammar_fallback_and_empty_rows():
    x = np.array([[1.0, 2.0, -np.inf, 0.5], [-np.inf] * 4])
    table = np.zeros((4, 1), dtype=np.uint32)
    table[0, 0], table[1, 0] = 0b1011, 0b0100                                 # after 0: ids 0, 1, 3; after 1: id 2 only (which is -inf)
    kept, touched, lse, _ = entropy_ref.mask(x, 4, 1.0, min_p=0.3, tok=[0, 0], table=table)
    assert touched.tolist() == [True, False] and kept[0].tolist() == [True, True, False, False] and lse[1] == 0
    assert abs(lse[0] - np.log(np.exp(1.0) + np.exp(2.0) + np.exp(0.5))) < 1e-12
    kept, _, _, _ = entropy_ref.mask(x[:1], 4, 1.0, min_p=0.2, tok=[1], table=table)
    assert kept[0].tolist() == [True, True, False, True]                      # nothing allowed is live: the table is ignored
    kept, _, _, _ = entropy_ref.mask(x[:1], 4, 1.0, min_p=0.3, tok=[9], table=table)      # clamped to row 3, which is empty
    assert kept[0].tolist() == [True, True, False, False]


def test_reference_account():
    x = np.log(np.array([[0.5, 0.25, 0.125, 0.125]] * 4))
    x[3, 2] = -np.inf
    s, mu = entropy_ref.account([1, 3, 7, 2], x, 4, 1.0, np.zeros(4), np.full(4, 6.0), 3.0, 0.5)
    assert np.allclose(s[:2], [2.0, 3.0]) and np.isnan(s[2:]).all()
    assert np.allclose(mu, [6.5, 6.0, 6.0, 6.0])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,msg", [
    (dict(min_p=-0.1), "min_p"), (dict(min_p=1.0), "min_p"), (dict(min_p=float("nan")), "min_p"), (dict(min_p="0.1"), "min_p"),
    (dict(min_p=True), "min_p"),
    (dict(typical_p=0.0), "typical_p"), (dict(typical_p=1.5), "typical_p"), (dict(typical_p=float("nan")), "typical_p"),
    (dict(typical_p=None), "typical_p"),
    (dict(tau=0.0), "tau"), (dict(tau=-3.0), "tau"), (dict(tau=float("inf")), "tau"), (dict(tau="3"), "tau"),
    (dict(tau=3.0, eta=0.0), "eta"), (dict(eta=1.5), "eta"), (dict(eta=float("nan")), "eta"), (dict(eta=None), "eta"),
    (dict(trace=1), "trace"), (dict(trace="yes"), "trace"),
])
def test_entropy_sampling_refuses(kw, msg):
    from musicgeneration_amd import decode
    with pytest.raises(ValueError, match=msg):
        decode.check_entropy_args(host_model(), _es(**kw), 1.0)
    x = torch.randint(0, 300, (3, 40))                                        # a CPU tensor and a CPU model: nothing reaches a device
    with pytest.raises(ValueError, match=msg):
        host_model().generate_cached(x, 10, entropy_sampling=_es(**kw))
    with pytest.raises(ValueError, match=msg):
        host_model().generate_cached(x, 10, entropy_sampling=_es(**kw), lookahead=4)
    with pytest.raises(ValueError, match=msg):
        host_model().generate_cached(x, 10, entropy_sampling=_es(**kw), samples_per_prompt=2)
    with pytest.raises(ValueError, match=msg):
        host_model().generate_timed(x, 5, np.zeros(V, dtype=np.int32), 10, entropy_sampling=_es(**kw))


@pytest.mark.parametrize("t", [0.0, -1.0, float("nan"), float("inf"), None])
def test_entropy_sampling_refuses_the_calls_temperature(t):
    from musicgeneration_amd import decode
    with pytest.raises(ValueError, match="temperature"):
        decode.check_entropy_args(host_model(), _es(), t)
    with pytest.raises(ValueError, match="temperature"):
        host_model().generate_cached(torch.randint(0, 300, (3, 40)), 10, temperature=t, entropy_sampling=_es())


def test_entropy_sampling_refuses_other_options_and_objects():
    from musicgeneration_amd import decode
    from musicgeneration_amd.sequence import EventSeq
    m, x = host_model(), torch.randint(0, 300, (3, 40))
    for kw in (dict(groups=2), dict(masked_groups=True)):
        with pytest.raises(ValueError, match="groups.*later work"):
            decode.check_entropy_args(m, _es(), 1.0, **kw)
        with pytest.raises(ValueError, match="groups.*later work"):
            m.generate_cached(x, 10, entropy_sampling=_es(), **kw)
    rules = EventSeq.note_rules(V)
    for kw in (dict(note_rules=rules), dict(note_rules=rules, max_polyphony=4)):
        with pytest.raises(ValueError, match="note_rules.*draws twice.*later work"):
            decode.check_entropy_args(m, _es(), 1.0, **kw)
        with pytest.raises(ValueError, match="note_rules.*later work"):
            m.generate_cached(x, 10, entropy_sampling=_es(), **kw)
        with pytest.raises(ValueError, match="note_rules.*later work"):
            m.generate_timed(x, 5, np.zeros(V, dtype=np.int32), 10, entropy_sampling=_es(), **kw)
    # under draft and verify only the stateless part: the state is sequential
    for kw in (dict(tau=3.0), dict(trace=True), dict(min_p=0.0, tau=3.0, trace=True)):
        with pytest.raises(ValueError, match="lookahead.*sequential.*later work"):
            decode.check_entropy_args(m, _es(**kw), 1.0, lookahead=4)
        with pytest.raises(ValueError, match="lookahead.*sequential.*later work"):
            m.generate_cached(x, 10, entropy_sampling=_es(**kw), lookahead=4)
    assert decode.check_entropy_args(m, _es(typical_p=0.5), 1.0, lookahead=4) is not None
    with pytest.raises(ValueError, match="EntropySampling"):
        decode.check_entropy_args(m, dict(min_p=0.1), 1.0)
    with pytest.raises(ValueError, match="generate_timed is not combined with lookahead"):
        m.generate_timed(x, 5, np.zeros(V, dtype=np.int32), 10, entropy_sampling=_es(), lookahead=4)
    assert decode.check_entropy_args(m, None, 1.0) is None
    assert decode.check_entropy_args(m, _es(), 1.0, groups=1) is not None
    with pytest.raises(TypeError):                                            # the drivers that do not take it
        m.generate_beam(torch.randint(0, 300, (1, 4)), 4, 2, entropy_sampling=_es())
    with pytest.raises(TypeError):
        m.generate(torch.randint(0, 300, (1, 4)), 4, entropy_sampling=_es())


def test_what_the_check_returns():
    from musicgeneration_amd import decode
    m = host_model()
    es = _es(min_p=np.float32(0.25), typical_p=0.5, tau=3, eta=np.float64(0.2), trace=np.bool_(True))
    own = decode.check_entropy_args(m, es, 1.25)
    assert own is not es and not own.inert and own.accounting
    assert (own.min_p, own.typical_p, own.tau, own.eta, own.trace) == (0.25, 0.5, 3.0, 0.2, True)
    assert all(type(v) is float for v in (own.min_p, own.typical_p, own.tau, own.eta)) and type(own.trace) is bool
    assert own.mu is None and own.lse is None and own.surprise is None        # staged by the driver, on its device
    assert es.mu is None and es.surprise is None                              # the caller's object is not touched
    # inert: min_p 0, typical_p 1, no tau, no trace -- whatever eta says: the unchanged step
    for kw in (dict(min_p=0.0), dict(min_p=0, typical_p=1), dict(min_p=0.0, typical_p=1.0, tau=None, eta=0.5, trace=False)):
        assert _es(**kw).inert and decode.check_entropy_args(m, _es(**kw), 1.0) is None, kw
    assert decode.EntropySampling().inert
    for kw in (dict(min_p=1e-6), dict(min_p=0.0, typical_p=0.999), dict(min_p=0.0, tau=3.0), dict(min_p=0.0, trace=True)):
        own = decode.check_entropy_args(m, _es(**kw), 1.0)
        assert own is not None and own.accounting == ("tau" in kw or "trace" in kw), kw


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_cli_flags_and_refusals(tmp_path, monkeypatch):
    from musicgeneration_amd import generate

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(generate, "MusicTransformer", no_model)
    base = ["-o", str(tmp_path / "out"), "-d", ""]
    flags = (["--min-p", "0.05"], ["--typical-p", "0.9"], ["--mirostat", "3"])
    for f in flags:
        for other, word in ((["-B", "2"], "-B/--beam-size"), (["--reference-mask"], "--reference-mask"),
                            (["--well-formed"], "--well-formed"), (["--max-polyphony", "4"], "--max-polyphony")):
            with pytest.raises(SystemExit, match="cannot be combined") as e:
                generate.main(base + f + other)
            assert word in str(e.value) and f[0] in str(e.value)
        with pytest.raises(AssertionError, match="a model was built"):        # the flag alone selects the KV-cache decode
            generate.main(base + f + ["--kv-cache", "fp8"])
    with pytest.raises(SystemExit, match="draws twice.*later work"):
        generate.main(base + flags[0] + ["--well-formed"])
    with pytest.raises(SystemExit, match="--mirostat cannot be combined with --lookahead.*sequential.*later work"):
        generate.main(base + ["--mirostat", "3", "--lookahead", "4"])
    with pytest.raises(SystemExit, match="--mirostat cannot be combined with --lookahead"):
        generate.main(base + ["--min-p", "0.05", "--mirostat", "3", "--lookahead", "4"])
    with pytest.raises(AssertionError, match="a model was built"):            # the stateless part goes with --lookahead
        generate.main(base + ["--min-p", "0.05", "--typical-p", "0.9", "--lookahead", "4"])
    for args in (["--mirostat-eta", "0.2"], ["--min-p", "0.05", "--mirostat-eta", "0.2"]):
        with pytest.raises(SystemExit, match="--mirostat-eta.*add --mirostat"):
            generate.main(base + args)
    for args, word in ((["--min-p", "1"], "--min-p"), (["--min-p", "-0.1"], "--min-p"), (["--min-p", "nan"], "--min-p"),
                       (["--typical-p", "0"], "--typical-p"), (["--typical-p", "1.2"], "--typical-p"),
                       (["--typical-p", "nan"], "--typical-p"), (["--mirostat", "0"], "--mirostat must"),
                       (["--mirostat", "-1"], "--mirostat must"), (["--mirostat", "inf"], "--mirostat must"),
                       (["--mirostat", "3", "--mirostat-eta", "0"], "--mirostat-eta"),
                       (["--mirostat", "3", "--mirostat-eta", "1.5"], "--mirostat-eta")):
        with pytest.raises(SystemExit, match=word):
            generate.main(base + args)
    o = generate.get_options([])
    assert (o.min_p, o.typical_p, o.mirostat, o.mirostat_eta) == (0.0, 1.0, None, None)
    assert generate._check_entropy(o, False) == {}                            # off by default
    es = generate._check_entropy(generate.get_options(["--min-p", "0.05", "--mirostat", "3"]), False)["entropy_sampling"]
    assert (es.min_p, es.typical_p, es.tau, es.eta, es.trace) == (0.05, 1.0, 3.0, 0.1, False)
    es = generate._check_entropy(generate.get_options(["--typical-p", "0.9", "--mirostat", "2.5", "--mirostat-eta", "0.3"]),
                                 False)["entropy_sampling"]
    assert (es.min_p, es.typical_p, es.tau, es.eta) == (0.0, 0.9, 2.5, 0.3)


# ---- the header -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_and_abi_34():
    from musicgeneration_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert int(re.search(r"^#define MGX_ABI_VERSION (\d+)", hdr, re.M).group(1)) >= 34 and _lib.EXPECTED_ABI >= 34
    assert "34: entropy-aware sampling" in hdr and "network.py:52-77" in hdr[hdr.index("Entropy-aware sampling (ABI 34)"):][:400]
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.FUNCTIONS["mgx_entropy_mask"] == (i, [vp, i, i, f, f, f, vp, vp, vp, vp, i, vp])
    assert _lib.FUNCTIONS["mgx_entropy_account"] == (i, [vp, vp, i, i, f, vp, vp, f, f, vp, i, vp, vp, i, i, vp])
    decl = re.search(r"int mgx_entropy_account\(([^;]*)\);", hdr).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    assert names == ["next_tok", "logits", "V", "ld", "temperature", "lse", "mu", "tau", "eta", "surprise_out", "out_ld", "pos_dev",
                     "base_dev", "per_row", "B", "stream"]                    # the header's one order: pos_dev, base_dev, per_row
    decl = re.search(r"int mgx_entropy_mask\(([^;]*)\);", hdr).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    assert names == ["logits", "V", "ld", "temperature", "min_p", "typical_p", "mu", "lse_out", "tok", "allow_table", "B", "stream"]
    lib = _lib.load()
    one = vp(16)                                                              # every refusal returns before anything is launched

    def mask(logits=one, V=5, ld=8, t=1.0, min_p=0.1, typical_p=0.5, mu=None, lse=None, tok=None, table=None, B=1):
        return lib.mgx_entropy_mask(logits, V, ld, t, min_p, typical_p, mu, lse, tok, table, B, None)
    for kw in (dict(logits=None), dict(tok=one), dict(table=one)):
        assert mask(**kw) == -2, kw
    for kw in (dict(B=0), dict(V=0), dict(V=1025, ld=1025), dict(V=9), dict(t=0.0), dict(t=-1.0), dict(t=float("inf")),
               dict(t=float("nan")), dict(min_p=-0.1), dict(min_p=1.0), dict(min_p=float("nan")), dict(typical_p=0.0),
               dict(typical_p=1.1), dict(typical_p=float("nan"))):
        assert mask(**kw) == -1, kw
    assert mask(V=9) == -1 and b"ld>=V" in lib.mgx_last_error()

    def account(tok=one, logits=one, V=5, ld=8, t=1.0, lse=one, mu=None, tau=3.0, eta=0.1, out=None, out_ld=0, pos=one, base=None,
                per_row=0, B=1):
        return lib.mgx_entropy_account(tok, logits, V, ld, t, lse, mu, tau, eta, out, out_ld, pos, base, per_row, B, None)
    for kw in (dict(tok=None), dict(logits=None), dict(lse=None), dict(pos=None)):
        assert account(**kw) == -2, kw
    for kw in (dict(B=0), dict(V=0), dict(V=9), dict(t=0.0), dict(t=float("nan")), dict(out=one, out_ld=0),
               dict(mu=one, tau=float("nan")), dict(mu=one, eta=float("inf"))):
        assert account(**kw) == -1, kw
