"""Host side of the held-note constraints (generate_cached(note_rules=, max_polyphony=), generate.py --well-formed /
--max-polyphony / --release, ABI 28): the codec's rule table, the fold and the release against plain Python loops, every refusal
(they run before any device work, so on a CPU model), tests/notes_ref.py against rows worked by hand, and the header."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import notes_ref
from decode_fixtures import host_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 309                                                                       # the MIDI-like codec's 308 ids and the pad id


def _rules(**at):
    from musicgeneration_amd.sequence import EventSeq
    r = EventSeq.note_rules(V)
    for k, v in at.items():
        r[int(k[1:])] = v
    return r


def _loop_held(ids):
    """the fold as a plain loop over the codec's ranges"""
    from musicgeneration_amd.sequence import EventSeq
    on, off = EventSeq.feat_ranges()["note_on"], EventSeq.feat_ranges()["note_off"]
    held = set()
    for t in ids:
        t = int(t)
        if t in on:
            held.add(t - on.start)
        elif t in off:
            held.discard(t - off.start)
    return sorted(held)


def test_note_rules_follow_the_codec_ranges():
    from musicgeneration_amd.sequence import EventSeq
    ranges = EventSeq.feat_ranges()
    for Vm in (308, 309, 390):
        r = EventSeq.note_rules(Vm)
        assert r.dtype == np.int32 and r.shape == (Vm,)
        for k, v in enumerate(ranges["note_on"]):
            assert r[v] == k + 1
        for k, v in enumerate(ranges["note_off"]):
            assert r[v] == -(k + 1)
        for name in ("velocity", "time_shift"):
            assert not r[ranges[name].start:ranges[name].stop].any()
        assert not r[EventSeq.dim():].any() and np.abs(r).max() == 88
    assert (EventSeq.note_rules() == EventSeq.note_rules(308)).all()
    with pytest.raises(ValueError, match="vocab_size"):
        EventSeq.note_rules(300)


def test_note_rules_refuse_a_small_vocabulary_as_time_cost_does():
    from musicgeneration_amd.sequence import EventSeq
    msgs = []
    for f in (EventSeq.note_rules, EventSeq.time_cost):
        with pytest.raises(ValueError) as e:
            f(7)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]


def test_held_after_and_release_against_a_plain_loop():
    from musicgeneration_amd.sequence import EventSeq
    rng = np.random.default_rng(3)
    off0 = EventSeq.feat_ranges()["note_off"].start
    doubles = orphans = 0
    for case in range(40):
        n = int(rng.integers(0, 120))
        # few keys, so that double note_ons and orphan note_offs are common; some velocity / time ids and ids beyond dim()
        ids = np.where(rng.random(n) < 0.7, rng.integers(0, 6, n) + off0 * rng.integers(0, 2, n), rng.integers(176, 312, n))
        held = set()
        for t in ids:
            doubles += int(t < 88 and t in held)
            orphans += int(88 <= t < 176 and t - 88 not in held)
            held = held | {int(t)} if t < 88 else held - {int(t) - 88}
        want = _loop_held(ids)
        got = EventSeq.held_after(ids)
        assert got.tolist() == want, case
        assert sorted(notes_ref.fold(EventSeq.note_rules(312), 312, ids)) == want
        rel = EventSeq.release(ids)
        assert rel.dtype == EventSeq(()).to_array().dtype == np.uint16
        assert rel[:n].tolist() == ids.tolist() and rel[n:].tolist() == [off0 + k for k in want]
        assert EventSeq.held_after(rel).size == 0
    assert doubles > 20 and orphans > 20
    assert EventSeq.held_after([]).size == 0 and EventSeq.release([]).size == 0
    assert EventSeq.held_after(torch.tensor([5, 5, 93, 7])).tolist() == [7]


def test_released_well_formed_stream_has_no_fallback_length(monkeypatch):
    from musicgeneration_amd import sequence
    from musicgeneration_amd.sequence import EventSeq
    FALLBACK = 12345.0                                                        # a length no time_shift sum of the stream reaches
    monkeypatch.setattr(sequence, "DEFAULT_NOTE_LENGTH", FALLBACK)
    rng = np.random.default_rng(9)
    rule = EventSeq.note_rules()
    held, ids = set(), []
    while len(ids) < 300:                                                     # a well-formed stream that stops with notes held
        t = int(rng.integers(0, 308))
        if not notes_ref.banned_id(rule, t, held, 128):
            ids.append(t)
            held = notes_ref.apply(rule, 308, held, t)
    for t in (3, 250, 40):                                                    # at least two held at the end
        if not notes_ref.banned_id(rule, t, held, 128):
            ids.append(t)
            held = notes_ref.apply(rule, 308, held, t)
    assert len(held) >= 2 and notes_ref.first_break(rule, 308, ids) is None and sorted(held) == EventSeq.held_after(ids).tolist()
    ons = sum(1 for t in ids if t < 88)

    def fallen_back(a):
        notes = EventSeq.from_array(a).to_note_seq().notes
        assert len(notes) == ons
        return sum(1 for n in notes if n.end - n.start == FALLBACK)
    assert fallen_back(np.array(ids)) == len(held)                            # without the release the held notes fall back
    assert fallen_back(EventSeq.release(ids)) == 0
    # an ill-formed stream keeps a fallback note whatever is appended: the double note_on's first note is never closed
    assert fallen_back(EventSeq.release(ids + [200, 200])) == 0 and \
        sum(1 for n in EventSeq.from_array(EventSeq.release([5, 250, 5])).to_note_seq().notes if n.end - n.start == FALLBACK) == 1


X = torch.randint(0, 300, (3, 40))                                            # a CPU tensor and a CPU model: nothing reaches a device


@pytest.mark.parametrize("kw,msg", [
    (dict(note_rules=None, max_polyphony=3), "needs note_rules"),
    (dict(max_polyphony=0), r"1 \.\. 128"),
    (dict(max_polyphony=129), r"1 \.\. 128"),
    (dict(max_polyphony=2.5), r"1 \.\. 128"),
    (dict(note_rules=np.zeros(V - 1, dtype=np.int32)), r"\[vocab_size\]"),
    (dict(note_rules=np.zeros((V, 1), dtype=np.int32)), r"\[vocab_size\]"),
    (dict(note_rules=np.zeros(V)), "integers"),
    (dict(note_rules=_rules(**{f"i{V - 1}": 5, "i4": -5})), "pad_token"),
    (dict(note_rules=_rules(i200=129, i201=-129)), "-128 .. 128"),
    (dict(note_rules=_rules(i200=100)), "sets it and one that clears it"),
    (dict(note_rules=_rules(i200=-100)), "sets it and one that clears it"),
    (dict(note_rules=_rules(i3=0)), "sets it and one that clears it"),
    (dict(grammar=torch.ones(V, V, dtype=torch.bool)), "grammar"),
    (dict(groups=2), "groups"),
    (dict(masked_groups=True), "groups"),
    (dict(return_cache=True), "return_cache"),
    (dict(kv_cache="int4"), "kv_cache"),                                      # what generate_cached refuses is refused too
])
def test_generate_cached_refuses(kw, msg):
    kw = dict(dict(note_rules=_rules()), **kw)
    with pytest.raises(ValueError, match=msg):
        host_model(V=V).generate_cached(X, 10, **kw)


def test_generate_timed_and_generate_beam_refuse():
    from musicgeneration_amd.sequence import EventSeq
    m = host_model(V=V)
    cost = EventSeq.time_cost(V)
    for kw, msg in ((dict(max_polyphony=3), "needs note_rules"), (dict(note_rules=_rules(), max_polyphony=200), r"1 \.\. 128"),
                    (dict(note_rules=_rules(i200=100)), "clears it"),
                    (dict(note_rules=_rules(), grammar=torch.ones(V, V, dtype=torch.bool)), "grammar"),
                    (dict(note_rules=_rules(), groups=2), "groups"), (dict(note_rules=_rules(), return_cache=True), "return_cache")):
        with pytest.raises(ValueError, match=msg):
            m.generate_timed(X, 100, cost, 10, **kw)
    for kw in (dict(note_rules=_rules()), dict(max_polyphony=2)):
        with pytest.raises(ValueError, match="generate_beam"):
            m.generate_beam(X, 10, 2, **kw)


def test_check_note_args_accepts_what_it_documents():
    from musicgeneration_amd import decode, ops
    m = host_model(V=V)
    assert decode.check_note_args(m, None, None) is None
    for rules in (_rules(), _rules().astype(np.int64), torch.from_numpy(_rules()), _rules().tolist()):
        ns = decode.check_note_args(m, rules, None)
        assert ns.rule_host.dtype == np.int32 and (ns.rule_host == _rules()).all() and ns.max_on == ops.NOTE_BITS == 128
    assert decode.check_note_args(m, _rules(), 1).max_on == 1 and decode.check_note_args(m, _rules(), 128).max_on == 128
    both = _rules(i300=128, i301=-128)                                        # bit 127, the last one
    assert decode.check_note_args(m, both, 7).max_on == 7
    # the staged fold, without a device: words of an ill-formed prompt
    w = decode.NoteState.fold(both, [300, 0, 0, 88 + 5, 31, 32, 88 + 31, 63, 301, 300])
    assert notes_ref.bits_of(w.view(np.int32)) == {0, 32, 63, 127}


def test_references_by_hand():
    rule = np.array([1, -1, 33, -33, 128, -128, 0, 2, -2, 500, -500], dtype=np.int32)
    ninf, keep = 0xFF80, 0x3F80
    st = np.stack([notes_ref.words(s) for s in ({0}, set(), {0, 32, 127}, {1})])
    assert st[2].view(np.uint32).tolist() == [1, 1, 0, 1 << 31]
    bits = np.full((4, 16), keep, dtype=np.uint16)
    got = notes_ref.mask(bits, 11, rule, st, 2)
    want = np.full((4, 16), keep, dtype=np.uint16)
    want[0, [0, 3, 5, 8]] = ninf                                              # bit 0 held: its note_on; the note_offs of clear bits
    want[1, [1, 3, 5, 8]] = ninf                                              # nothing held: every note_off
    want[2, [0, 2, 4, 7, 8]] = ninf                                           # three held >= 2: every note_on, and bit 1's note_off
    want[3, [1, 3, 5, 7]] = ninf                                              # bit 1 held, below the cap
    assert (got == want).all()                                                # ids 6, 9, 10 and columns >= 11 untouched
    got = notes_ref.account([0, 0, 1, 1, 4, 6, -1, 11, 9], rule, np.stack([st[0], st[1], st[0], st[1]] + [st[1]] * 5), 11)
    assert [sorted(notes_ref.bits_of(w)) for w in got] == [[0], [0], [], [], [127], [], [], [], []]
    # keep: rows 0 / 1 draw id 0 first (bit 0 held: banned; nothing held: legal), row 2 a rule-0 id at the cap, row 3 id -1
    tok, out = notes_ref.keep([0, 0, 6, -1], [7, 7, 7, 7], np.full((4, 3), 9), [1], [1], 0, rule, st, 2, 11)
    assert tok.tolist() == [7, 0, 6, 7] and out.tolist() == [[9, 9, 9], [9, 9, 0], [9, 9, 6], [9, 9, 9]]
    tok, out = notes_ref.keep([0, 0], [7, 7], np.full((2, 3), 9), [0, 3], None, 1, rule, st[1:3], 5, 11)
    assert tok.tolist() == [0, 7] and out.tolist() == [[0, 9, 9], [9, 9, 9]]       # row 1 holds bit 0; a column outside is not written
    assert notes_ref.first_break(rule, 11, [0, 2, 6, 1, 3]) is None
    assert notes_ref.first_break(rule, 11, [0, 2, 0]) == 2 and notes_ref.first_break(rule, 11, [0, 8]) == 1
    assert notes_ref.first_break(rule, 11, [0, 2, 4], max_on=2) == 2 and notes_ref.first_break(rule, 11, [1], held={0}) is None


def test_header_declares_the_two_calls_and_abi_28():
    from musicgeneration_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert int(re.search(r"^#define MGX_ABI_VERSION (\d+)", hdr, re.M).group(1)) >= 28 and _lib.EXPECTED_ABI >= 28
    assert "28: per-row held-note state" in hdr
    assert _lib.DEFINES["MGX_NOTE_WORDS"] == 4 == ops.NOTE_WORDS == notes_ref.NOTE_WORDS
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.FUNCTIONS["mgx_notes_mask"] == (i, [vp, i, i, vp, vp, i, i, vp])
    assert _lib.FUNCTIONS["mgx_notes_account"] == (i, [vp, vp, vp, i, i, vp])
    assert _lib.FUNCTIONS["mgx_notes_keep"] == (i, [vp, vp, vp, i, vp, vp, i, vp, vp, i, i, i, vp])
    lib = _lib.load()
    one = vp(16)
    assert lib.mgx_notes_mask(None, 5, 8, one, one, 3, 1, None) == -2
    assert lib.mgx_notes_mask(one, 9, 8, one, one, 3, 1, None) == -1 and b"ld>=V" in lib.mgx_last_error()
    assert lib.mgx_notes_mask(one, 5, 8, one, one, 0, 1, None) == -1 and b"max_on" in lib.mgx_last_error()
    assert lib.mgx_notes_mask(one, 5, 8, one, one, 129, 1, None) == -1
    assert lib.mgx_notes_mask(one, 5, 8, one, one, 3, 0, None) == -1
    assert lib.mgx_notes_account(one, None, one, 5, 1, None) == -2
    assert lib.mgx_notes_account(one, one, one, 5, 0, None) == -1
    assert lib.mgx_notes_keep(one, one, None, 0, None, None, 0, one, one, 3, 5, 1, None) == -2
    assert lib.mgx_notes_keep(one, one, one, 0, one, None, 0, one, one, 3, 5, 1, None) == -1
    assert lib.mgx_notes_keep(one, one, None, 0, one, None, 0, one, one, 0, 5, 1, None) == -1 and b"max_on" in lib.mgx_last_error()


def test_cli_refusals_come_before_any_model(tmp_path, monkeypatch):
    from musicgeneration_amd import generate

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(generate, "MusicTransformer", no_model)
    base = ["-o", str(tmp_path / "out"), "-d", ""]
    for args, word in ((["--well-formed", "-B", "4"], "-B/--beam-size"), (["--max-polyphony", "3", "-B", "2"], "-B/--beam-size"),
                       (["--release", "-B", "2"], "-B/--beam-size"), (["--well-formed", "--reference-mask"], "--reference-mask")):
        with pytest.raises(SystemExit, match="cannot be combined") as e:
            generate.main(base + args)
        assert word in str(e.value)
    for args, word in ((["--well-formed", "--repr", "remi"], "--repr midi_like"), (["--release", "--repr", "mumidi"], "--repr midi_like"),
                       (["--well-formed", "--repr", "remi", "--grammar"], "--repr midi_like"),
                       (["--max-polyphony", "0"], r"1 \.\. 128"), (["--max-polyphony", "129"], r"1 \.\. 128")):
        with pytest.raises(SystemExit, match=word):
            generate.main(base + args)
    o = generate.get_options(["--well-formed", "--grammar"])                  # (--grammar itself wants another --repr)
    with pytest.raises(SystemExit, match="--grammar"):
        generate._check_notes(o)
    o = generate.get_options([])
    assert not o.well_formed and o.max_polyphony is None and not o.release and generate._check_notes(o) is False
    assert generate._check_notes(generate.get_options(["--max-polyphony", "4"])) is True          # implies --well-formed
    assert generate._check_notes(generate.get_options(["--release"])) is False
