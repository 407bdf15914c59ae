"""Host side of repetition control (decode.Repetition, generate.py's repetition flags, ABI 31): tests/repeat_ref.py against a second,
brute-force formulation; every refusal, which runs before any device work and so without a GPU; the penalty table; the codecs'
subject tables; the flags; and the header's declaration."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import repeat_ref
from decode_fixtures import host_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 337


def _brute(row, c, Vb, subject, pen, window, n, span, ban):
    """the amounts of one row, formulated the other way round: every id asks for itself.  v is banned iff appending v to the
    history up to column c makes the n-gram that now ends the row occur a second time, wholly inside the last ``span`` columns of
    the history; v is counted by looking at the window backwards from c"""
    hist = [int(t) for t in row[:c + 1]]
    am = {}
    for v in range(Vb):
        hit = False
        if n >= 2 and len(hist) >= n - 1:
            ext = hist + [v]
            tail = ext[len(ext) - n:]
            first = (max(0, len(hist) - span) if span else 0)
            hit = len(hist) - first >= n - 1 and any(ext[s:s + n] == tail for s in range(first, len(hist) - n + 1))
        if hit:
            am[v] = np.float32(ban)
            continue
        k = sum(1 for back in range(window) if c - back >= 0 and hist[c - back] == v)
        if window > 0 and k > 0 and subject[v] != 0:
            am[v] = np.float32(pen[k])
    return am


def test_reference_against_a_second_formulation():
    """random short rows over a 3-id alphabet (so that contexts recur, occurrences overlap and runs like aaaa occur), with ids
    outside 0..V-1 among them"""
    rng = np.random.default_rng(11)
    alphabet = np.array([0, 2, 5, -3])                                        # V = 4: id 5 and the negative id are out of range
    Vb, checked, bans, counted = 4, 0, 0, 0
    for trial in range(300):
        L = int(rng.integers(1, 14))
        row = alphabet[rng.choice(4, L, p=[0.4, 0.4, 0.1, 0.1])]
        if trial % 5 == 0:
            row[:] = row[0]                                                    # a run of one id
        window = int(rng.integers(0, 6))
        n = int(rng.choice([0, 2, 3, 4]))
        span = 0 if n == 0 or rng.random() < 0.4 else int(rng.integers(n, n + 6))
        subject = rng.integers(0, 2, Vb)
        pen = np.concatenate([[0.0], rng.random(window) + 0.5]).astype(np.float32)
        for c in range(L):
            want = _brute(row, c, Vb, subject, pen, window, n, span, 100.0)
            got = repeat_ref.amounts(row, c, Vb, subject, pen, window, n, span, 100.0)
            assert got == want, (row.tolist(), c, window, n, span, got, want)
            checked += 1
            bans += sum(1 for a in want.values() if a == 100.0)
            counted += sum(1 for a in want.values() if a != 100.0)
    assert checked > 1500 and bans > 200 and counted > 200


def test_reference_by_hand():
    row = [1, 2, 1, 2, 3, 1, 2, 9]
    assert repeat_ref.banned(row, 6, 4, 3, 0) == {1, 3}                       # "1 2" was followed by 1 and by 3
    assert repeat_ref.banned(row, 6, 4, 3, 5) == {3}                          # lo = 2: the occurrence at 0..1 begins before it
    assert repeat_ref.banned(row, 6, 4, 3, 4) == set()                        # lo = 3: the one at 2..3 too
    assert repeat_ref.banned(row, 6, 4, 2, 0) == {1, 3}                       # "2" -> 1, 3
    assert repeat_ref.banned(row, 6, 3, 2, 0) == {1}                          # V = 3: the follower 3 is out of range
    assert repeat_ref.banned([7, 7, 7, 7], 3, 8, 3, 0) == {7}                 # overlapping occurrences; the follower at column c
    assert repeat_ref.banned([7, 7], 1, 8, 3, 0) == set()                     # c = n - 2 = 1: a context, no earlier occurrence
    assert repeat_ref.banned([7], 0, 8, 3, 0) == set()                        # c < n - 2: no context
    assert repeat_ref.counts(row, 6, 4, 3).tolist() == [0, 1, 1, 1]           # columns 4..6
    assert repeat_ref.counts(row, 7, 4, 64).tolist() == [0, 3, 3, 1]          # the 9 counts for nothing
    assert repeat_ref.repeats([1, 2, 3, 1, 2], 2) and not repeat_ref.repeats([1, 2, 3, 2, 1], 2)
    assert repeat_ref.repeats([1, 2, 3, 4, 1, 2], 2, 5) and not repeat_ref.repeats([1, 2, 3, 4, 1, 2], 2, 4)
    one, ninf = 0x3F80, 0xFF80                                                # 1.0 and -inf
    bits = np.array([[one, one, ninf, one, 0x7FC0]], dtype=np.uint16)
    pen = np.array([0, 0.5, 1.0], dtype=np.float32)
    got = repeat_ref.penalise(bits, 4, [[0, 0, 2, 3, 1]], [3], None, 0, [1, 1, 1, 0], pen, 2, 2, 0, 1e4)
    # c = 3, window 2: columns 2..3 hold 2 and 3 (3 is no subject); n = 2: the context "3" has not occurred before
    assert got.tolist() == [[one, one, ninf, one, 0x7FC0]]
    got = repeat_ref.penalise(bits, 4, [[0, 0, 0, 3, 1]], [2], None, 0, [1, 1, 1, 0], pen, 2, 2, 0, 1e4)
    # c = 2, window 2: id 0 twice -> pen[2]; n = 2: "0" was followed by 0 -> ban, not the sum: 1 - 1e4 = -9999 -> bf16 -9984
    assert got.tolist() == [[0xC61C, one, ninf, one, 0x7FC0]]
    got = repeat_ref.penalise(bits, 4, [[0, 1, 0, 3, 1]], [1], [1], 0, [1, 1, 1, 0], pen, 2, 0, 0, 1e4)
    assert got.tolist() == [[0x3F00, 0x3F00, ninf, one, 0x7FC0]]              # c = 2: ids 0 and 1 once: 1 - 0.5
    assert (repeat_ref.penalise(bits, 4, [[0, 1, 0, 3, 1]], [5], None, 0, [1, 1, 1, 0], pen, 2, 0, 0, 1e4) == bits).all()   # c = out_ld


def _rep(**kw):
    from musicgeneration_amd import decode
    sub = np.zeros(V, dtype=np.int32)
    sub[:88] = 1
    kw = dict(dict(subject=sub, presence=0.5, frequency=0.1), **kw)
    return decode.Repetition(**kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(subject=np.ones(V - 1, dtype=np.int32)), r"\[vocab_size\]"),
    (dict(subject=np.ones((V, 1), dtype=np.int32)), r"\[vocab_size\]"),
    (dict(subject=np.zeros(V)), "integers"),
    (dict(subject=np.ones(V, dtype=np.int32)), "pad_token"),
    (dict(presence=-0.1), "presence"),
    (dict(presence=float("nan")), "presence"),
    (dict(frequency=float("inf")), "frequency"),
    (dict(frequency=-1), "frequency"),
    (dict(window=0), "window"),
    (dict(window=4097), "window"),
    (dict(window=2.5), "window"),
    (dict(ngram=1), "ngram"),
    (dict(ngram=65), "ngram"),
    (dict(ngram=-2), "ngram"),
    (dict(ngram=4, span=3), "span"),
    (dict(span=-1), "span"),
    (dict(ngram=2, ban=0.0), "ban"),
    (dict(ban=1e4 + 1), "ban"),
    (dict(ban=float("nan")), "ban"),
    (dict(presence=1.0, frequency=200.0, window=50), "presence \\+ frequency"),
])
def test_repetition_refuses(kw, msg):
    from musicgeneration_amd import decode
    with pytest.raises(ValueError, match=msg):
        decode.check_repeat_args(host_model(), _rep(**kw))
    x = torch.randint(0, 300, (3, 40))                                        # a CPU tensor and a CPU model: nothing reaches a device
    with pytest.raises(ValueError, match=msg):
        host_model().generate_cached(x, 10, repetition=_rep(**kw))
    cost = np.zeros(V, dtype=np.int32)
    with pytest.raises(ValueError, match=msg):
        host_model().generate_timed(x, 5, cost, 10, repetition=_rep(**kw))


def test_repetition_refuses_the_experiment_flags_and_other_objects():
    from musicgeneration_amd import decode
    m = host_model()
    for kw in (dict(groups=2), dict(masked_groups=True)):
        with pytest.raises(ValueError, match="groups"):
            decode.check_repeat_args(m, _rep(), **kw)
        with pytest.raises(ValueError, match="groups"):
            m.generate_cached(torch.randint(0, 300, (3, 40)), 10, repetition=_rep(), **kw)
    with pytest.raises(ValueError, match="Repetition"):
        decode.check_repeat_args(m, dict(presence=1.0))
    assert decode.check_repeat_args(m, None) is None
    assert decode.check_repeat_args(m, _rep(), groups=1) is not None
    with pytest.raises(TypeError):                                            # the drivers that do not take it
        m.generate_beam(torch.randint(0, 300, (1, 4)), 4, 2, repetition=_rep())
    with pytest.raises(TypeError):
        m.generate(torch.randint(0, 300, (1, 4)), 4, repetition=_rep())


def test_what_the_check_returns():
    from musicgeneration_amd import decode
    m = host_model()
    r = decode.check_repeat_args(m, _rep(subject=torch.arange(V) % 2 * (torch.arange(V) < V - 1), ngram=3, span=3, ban=50))
    assert r.subject_host.dtype == np.int32 and r.subject_host.sum() == (V - 1) // 2 and r.counting and not r.inert
    assert (r.window, r.ngram, r.span, r.ban) == (64, 3, 3, 50.0)
    assert decode.check_repeat_args(m, _rep(presence=0, frequency=0)) is None             # inert: the unchanged step
    r = decode.check_repeat_args(m, _rep(presence=0, frequency=0, ngram=2))
    assert not r.counting and not r.inert
    assert decode.check_repeat_args(m, _rep(presence=0.0, frequency=1e4 / 64)) is not None  # exactly the cap


def test_pen_table():
    p = _rep(presence=0.3, frequency=0.1, window=5).pen_table()
    assert p.dtype == np.float32 and p.shape == (6,) and p[0] == 0
    for c in range(1, 6):
        assert p[c] == np.float32(np.float64(0.3) + np.float64(0.1) * c)
    p = _rep(presence=0.0, frequency=2.0, window=3).pen_table()
    assert p.tolist() == [0.0, 2.0, 4.0, 6.0]
    p = _rep(presence=1.5, frequency=0.0, window=2).pen_table()
    assert p.tolist() == [0.0, 1.5, 1.5]


def test_repeat_subject_tables():
    from musicgeneration_amd.MuMIDI import MuMIDI_EventSeq
    from musicgeneration_amd.REMI import REMI_EventSeq
    from musicgeneration_amd.sequence import EventSeq
    for Codec in (EventSeq, REMI_EventSeq, MuMIDI_EventSeq):
        on, dim = Codec.feat_ranges()["note_on"], Codec.dim()
        for Vm in (dim, dim + 1, dim + 50):
            s = Codec.repeat_subject(Vm)
            assert s.dtype == np.int32 and s.shape == (Vm,)
            want = np.zeros(Vm, dtype=np.int32)
            want[list(on)] = 1
            assert (s == want).all() and s.sum() == len(on) and not s[dim:].any()
        assert (Codec.repeat_subject() == Codec.repeat_subject(dim)).all()
        with pytest.raises(ValueError, match="vocab_size"):
            Codec.repeat_subject(dim - 1)
    assert EventSeq.repeat_subject().sum() == 88 and REMI_EventSeq.repeat_subject().sum() == 127
    assert MuMIDI_EventSeq.repeat_subject().sum() == 256 and MuMIDI_EventSeq.repeat_subject()[0] == 0     # the drum hits; not `empty`


def test_cli_flags_and_refusals(tmp_path, monkeypatch):
    from musicgeneration_amd import generate

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(generate, "MusicTransformer", no_model)
    base = ["-o", str(tmp_path / "out"), "-d", ""]
    flags = (["--presence-penalty", "0.5"], ["--frequency-penalty", "0.2"], ["--repeat-window", "32"], ["--repeat-ids", "all"],
             ["--no-repeat-ngram", "4"], ["--no-repeat-ngram", "4", "--ngram-span", "16"])
    for f in flags:
        for other, word in ((["-B", "2"], "-B/--beam-size"), (["--reference-mask"], "--reference-mask")):
            with pytest.raises(SystemExit, match="cannot be combined") as e:
                generate.main(base + f + other)
            assert word in str(e.value) and f[0] in str(e.value)
        assert generate._check_repeat(generate.get_options(f)) is True
    for args, word in ((["--presence-penalty", "-1"], "--presence-penalty"), (["--frequency-penalty", "nan"], "--frequency-penalty"),
                       (["--repeat-window", "0"], "--repeat-window"), (["--repeat-window", "5000"], "--repeat-window"),
                       (["--no-repeat-ngram", "1"], "--no-repeat-ngram"), (["--no-repeat-ngram", "65"], "--no-repeat-ngram"),
                       (["--no-repeat-ngram", "4", "--ngram-span", "3"], "--ngram-span"),
                       (["--frequency-penalty", "200", "--repeat-window", "100"], "1e4")):
        with pytest.raises(SystemExit, match=word):
            generate.main(base + args)
    o = generate.get_options([])
    assert (o.presence_penalty, o.frequency_penalty, o.repeat_window, o.repeat_ids, o.no_repeat_ngram, o.ngram_span) == \
        (0.0, 0.0, 64, "pitch", 0, 0)
    assert generate._check_repeat(o) is False                                  # off by default
    assert "unpenalised" in [op for op in generate_parser_options(generate) if op.dest == "presence_penalty"][0].help

    class M:                                                                   # what _repeat_args reads of a model
        vocab_size, pad_token = 337, 336
    o = generate.get_options(["--repr", "remi", "--frequency-penalty", "0.25", "--no-repeat-ngram", "6", "--ngram-span", "40"])
    r = generate._repeat_args(o, M)["repetition"]
    assert (r.presence, r.frequency, r.window, r.ngram, r.span, r.ban) == (0.0, 0.25, 64, 6, 40, 1e4)
    assert np.asarray(r.subject_host).sum() == 127
    r = generate._repeat_args(generate.get_options(["--repeat-ids", "all", "--presence-penalty", "1"]), M)["repetition"]
    assert np.asarray(r.subject_host).sum() == 336 and r.subject_host[336] == 0 and r.presence == 1.0
    # --kv-cache fp8 alone is refused (the default sampler keeps no cache); a repetition flag selects the KV-cache decode
    with pytest.raises(SystemExit, match="KV-cache decode only"):
        generate.main(base + ["--kv-cache", "fp8"])
    with pytest.raises(AssertionError, match="a model was built"):
        generate.main(base + ["--kv-cache", "fp8", "--no-repeat-ngram", "3"])


def generate_parser_options(generate):
    """the optparse options of generate.py (get_options builds the parser inside: read them off a parse of --help's parser)"""
    import optparse
    seen = []
    orig = optparse.OptionParser.parse_args

    def spy(self, *a, **k):
        seen.extend(self.option_list)
        return orig(self, *a, **k)
    optparse.OptionParser.parse_args = spy
    try:
        generate.get_options([])
    finally:
        optparse.OptionParser.parse_args = orig
    return seen


def test_header_declares_the_call_and_abi_31():
    from musicgeneration_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert int(re.search(r"^#define MGX_ABI_VERSION (\d+)", hdr, re.M).group(1)) >= 31 and _lib.EXPECTED_ABI >= 31
    assert "31: repetition control" in hdr
    assert _lib.DEFINES["MGX_REPEAT_MAX_WINDOW"] == 4096 == ops.REPEAT_MAX_WINDOW
    assert _lib.DEFINES["MGX_REPEAT_MAX_NGRAM"] == 64 == ops.REPEAT_MAX_NGRAM
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.FUNCTIONS["mgx_repeat_penalty"] == (i, [vp, i, i, vp, i, vp, vp, i, vp, vp, i, i, i, f, i, vp])
    lib = _lib.load()
    one = vp(16)
    assert lib.mgx_repeat_penalty(None, 5, 8, one, 8, one, None, 0, one, one, 4, 0, 0, 1e4, 1, None) == -2
    assert lib.mgx_repeat_penalty(one, 5, 8, one, 8, one, None, 0, None, one, 4, 0, 0, 1e4, 1, None) == -2
    assert lib.mgx_repeat_penalty(one, 9, 8, one, 8, one, None, 0, one, one, 4, 0, 0, 1e4, 1, None) == -1
    assert b"ld>=V" in lib.mgx_last_error()
    assert lib.mgx_repeat_penalty(one, 5, 8, one, 8, one, None, 0, None, None, 0, 0, 0, 1e4, 1, None) == -1     # nothing to do
