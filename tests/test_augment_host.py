"""Host side of the train-time augmentation (ABI 29; no GPU): the codecs' transposition tables against the reference's function
(fixture g13) and against their stated properties, EventSeq.stretch_ids, the crop plan of data.DeviceData against the host
feeder's draws, the numpy reference of the kernel against the header's own claims, and every refusal of the constructor and of
the two command lines."""
import os
import random
import re

import numpy as np
import pytest
import torch

import augment_ref
from musicgeneration_amd import _lib, melody_train, train
from musicgeneration_amd.data import Data, DeviceData, check_stretch
from musicgeneration_amd.MuMIDI import MuMIDI_EventSeq
from musicgeneration_amd.REMI import REMI_EventSeq
from musicgeneration_amd.sequence import EventSeq

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALL_OFFSETS = list(range(-11, 12))


# ---- the tables ------------------------------------------------------------------------------------------------------------------
def test_midi_like_table_is_the_reference_s_transposition():
    g = np.load(os.path.join(GOLDEN, "g13_transposition.npz"))
    assert g["offsets"].tolist() == list(range(-6, 7)) and g["table"].shape == (13, EventSeq.dim())
    table = EventSeq.transpose_table(g["offsets"])
    assert table.dtype == np.int32 and np.array_equal(table, g["table"])
    wide = EventSeq.transpose_table(g["offsets"], EventSeq.dim() + 1)         # with a model's pad id: it maps to itself
    assert np.array_equal(wide[:, :-1], g["table"]) and (wide[:, -1] == EventSeq.dim()).all()


def pitch_runs_move(table, run, offsets):
    """slot k of the run goes to k + offset, or comes back by one octave; the pitch class moves by offset mod 12"""
    k = np.arange(len(run))
    for s, off in enumerate(offsets):
        to = table[s, run.start:run.stop] - run.start
        assert ((to >= 0) & (to < len(run))).all()
        assert ((to - k) % 12 == off % 12).all()
        inside = (k + off >= 0) & (k + off < len(run))
        assert (to[inside] == (k + off)[inside]).all()
        assert (to[k + off >= len(run)] == (k + off - 12)[k + off >= len(run)]).all()
        assert (to[k + off < 0] == (k + off + 12)[k + off < 0]).all()


def chords_rotate(table, run, offsets):
    c = np.arange(len(run) - 1)
    for s, off in enumerate(offsets):
        to = table[s, run.start:run.stop] - run.start
        assert (to[:-1] // 12 == c // 12).all() and (to[:-1] % 12 == (c % 12 + off) % 12).all()
        assert to[-1] == len(run) - 1                                          # N:N


def fixed_elsewhere(table, moving):
    V = table.shape[1]
    still = np.setdiff1d(np.arange(V), np.concatenate([np.arange(r.start, r.stop) for r in moving]))
    assert (table[:, still] == still).all()


@pytest.mark.parametrize("extra", [0, 1])
def test_midi_like_table_properties(extra):
    r = EventSeq.feat_ranges()
    table = EventSeq.transpose_table(ALL_OFFSETS, EventSeq.dim() + extra)
    assert table.shape == (23, 308 + extra)
    pitch_runs_move(table, r["note_on"], ALL_OFFSETS)
    pitch_runs_move(table, r["note_off"], ALL_OFFSETS)
    on, off = table[:, r["note_on"].start:r["note_on"].stop], table[:, r["note_off"].start:r["note_off"].stop]
    assert (off - r["note_off"].start == on - r["note_on"].start).all()        # note_on and note_off of a key move alike
    fixed_elsewhere(table, [r["note_on"], r["note_off"]])
    assert (table[ALL_OFFSETS.index(0)] == np.arange(308 + extra)).all()
    assert table[ALL_OFFSETS.index(3), 86] == table[ALL_OFFSETS.index(3), 74] == 77      # the wrap sends two keys to one


def test_remi_table_properties():
    r = REMI_EventSeq.feat_ranges()
    table = REMI_EventSeq.transpose_table(ALL_OFFSETS, REMI_EventSeq.dim() + 1)
    assert table.shape == (23, 337) and table.dtype == np.int32
    pitch_runs_move(table, r["note_on"], ALL_OFFSETS)
    chords_rotate(table, r["chord"], ALL_OFFSETS)
    fixed_elsewhere(table, [r["note_on"], r["chord"]])
    assert (table[ALL_OFFSETS.index(0)] == np.arange(337)).all()
    from musicgeneration_amd.REMI import chord_map
    c0 = r["chord"].start
    assert table[ALL_OFFSETS.index(2), c0 + chord_map["B:min"]] == c0 + chord_map["C#:min"]
    assert table[ALL_OFFSETS.index(-1), c0 + chord_map["C:dom"]] == c0 + chord_map["B:dom"]


def test_mumidi_table_properties():
    r = MuMIDI_EventSeq.feat_ranges()
    table = MuMIDI_EventSeq.transpose_table(ALL_OFFSETS, MuMIDI_EventSeq.dim() + 1)
    assert table.shape == (23, 486)
    on = r["note_on"]
    pitches, drums = range(on.start, on.start + 128), range(on.start + 128, on.stop)
    assert len(drums) == 128
    pitch_runs_move(table, pitches, ALL_OFFSETS)
    assert (table[:, drums.start:drums.stop] == np.arange(drums.start, drums.stop)).all()
    chords_rotate(table, r["chord"], ALL_OFFSETS)
    fixed_elsewhere(table, [pitches, r["chord"]])
    assert (table[ALL_OFFSETS.index(0)] == np.arange(486)).all()


@pytest.mark.parametrize("codec", [EventSeq, REMI_EventSeq, MuMIDI_EventSeq])
def test_table_refusals(codec):
    for bad in ([12], [-12], [0, 13], []):
        with pytest.raises(ValueError, match="offsets"):
            codec.transpose_table(bad)
    with pytest.raises(ValueError, match="vocab_size"):
        codec.transpose_table([1], codec.dim() - 1)


def test_stretch_ids(monkeypatch):
    assert EventSeq.stretch_ids() == (208, 100) and EventSeq.stretch_ids(309) == (208, 100)
    cost = EventSeq.time_cost()
    assert (cost[208:308] == np.arange(1, 101)).all()
    monkeypatch.setattr(EventSeq, "time_shift_bins", 0.02 * np.arange(1, 101))           # bins of 2, 4, ... units
    with pytest.raises(ValueError, match="linear"):
        EventSeq.stretch_ids()
    monkeypatch.setattr(EventSeq, "time_shift_bins", np.concatenate([0.01 * np.arange(1, 100), [1.5]]))
    with pytest.raises(ValueError, match="linear"):
        EventSeq.stretch_ids()
    assert not hasattr(REMI_EventSeq, "stretch_ids") and not hasattr(MuMIDI_EventSeq, "stretch_ids")


# ---- the plan --------------------------------------------------------------------------------------------------------------------
def write_files(root, lengths, seed=0):
    rng = np.random.default_rng(seed)
    for i, n in enumerate(lengths):
        torch.save(rng.integers(0, 308, n).astype(np.uint16), os.path.join(root, f"f{i:02d}.data"))


def pair(root, max_seq, seed, **aug):
    return Data(root, max_seq, rng=random.Random(seed)), DeviceData(Data(root, max_seq, rng=random.Random(seed)), "cpu", 308, **aug)


def slices(dev, files, starts, length):
    corpus = dev.corpus.view(torch.int16).numpy().view(np.uint16)
    at = dev.offsets_host[files] + starts
    assert ((dev.lengths_host[files] - starts) >= length + 1).all()
    return np.stack([corpus[a:a + length] for a in at]), np.stack([corpus[a + 1:a + length + 1] for a in at])


def test_the_plan_names_the_host_feeder_s_crops(tmp_path):
    write_files(str(tmp_path), [70 + 3 * i for i in range(30)])
    host, dev = pair(str(tmp_path), 32, seed=11)
    assert dev.corpus.dtype == torch.uint16 and dev.corpus.numel() == int(dev.lengths_host.sum())
    assert dev.offsets.tolist() == dev.offsets_host.tolist() and dev.lengths.tolist() == dev.lengths_host.tolist()
    assert len(dev.files) == len(host.file_dict["train"]) == 24
    for B, L in ((4, 32), (24, 40), (1, 68), (5, 33)):
        hx, hy = host.slide_seq2seq_batch(B, L)
        files, starts = dev.plan(B, L)
        assert files.dtype == starts.dtype == np.int64 and len(set(files.tolist())) == B
        x, y = slices(dev, files, starts, L)
        assert np.array_equal(x, hx.astype(np.int64)) and np.array_equal(y, hy.astype(np.int64))


def test_the_other_splits_upload_their_own_files(tmp_path):
    write_files(str(tmp_path), [60] * 20)
    data = Data(str(tmp_path), 32, rng=random.Random(1))
    dev = DeviceData(data, "cpu", 308, mode="valid")
    assert dev.files == data.file_dict["valid"] and len(dev.files) == 2
    with pytest.raises(ValueError, match="mode"):
        DeviceData(data, "cpu", 308, mode="all")


def test_too_short_files_raise_as_on_the_host_and_spend_the_same_draws(tmp_path):
    """files of exactly length (IndexError), length + 1 (ValueError: an empty randrange) and longer ones, mixed: batch after
    batch both feeders raise the same or return the same crops -- the draws made before a raise are spent alike"""
    L = 40
    write_files(str(tmp_path), [L, L + 1, L + 2, 90, L, 77, L + 1, 60, 55, 120] * 3)
    host, dev = pair(str(tmp_path), L, seed=3)
    seen = set()
    for _ in range(40):
        try:
            want = host.slide_seq2seq_batch(3, L)
        except (IndexError, ValueError) as e:
            seen.add(type(e))
            with pytest.raises(type(e)):
                dev.plan(3, L)
            continue
        seen.add(None)
        files, starts = dev.plan(3, L)
        x, y = slices(dev, files, starts, L)
        assert np.array_equal(x, want[0].astype(np.int64)) and np.array_equal(y, want[1].astype(np.int64))
    assert seen == {IndexError, ValueError, None}
    with pytest.raises(ValueError):                            # more rows than files: random.sample's refusal, as on the host
        dev.plan(25, L)


def test_augmentation_never_moves_the_crops(tmp_path):
    write_files(str(tmp_path), [80 + i for i in range(20)])
    _, plain = pair(str(tmp_path), 32, seed=5)
    _, aug = pair(str(tmp_path), 32, seed=5, transpose=[-2, 0, 2], stretch=[0.9, 1.1], aug_rng=random.Random(1))
    assert plain.perm is None and plain.stretch_q is None and plain.draw_augmentation(4) == (None, None)
    assert aug.perm.shape == (3, 309) and aug.perm.dtype == torch.int32 and aug.stretch_q == [900, 1100] and (aug.ts0, aug.n_ts) == (208, 100)
    for _ in range(5):
        a, b = plain.plan(6, 32), aug.plan(6, 32)
        shift, q = aug.draw_augmentation(6)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert len(shift) == len(q) == 6 and set(shift) <= {0, 1, 2} and set(q) <= {900, 1100}
    twin = random.Random(1)                                    # row after row: the shift, then the factor
    _, again = pair(str(tmp_path), 32, seed=5, transpose=[-2, 0, 2], stretch=[0.9, 1.1], aug_rng=random.Random(1))
    shift, q = again.draw_augmentation(3)
    want = [(twin.randrange(3), [900, 1100][twin.randrange(2)]) for _ in range(3)]
    assert list(zip(shift, q)) == want


def test_constructor_refusals(tmp_path):
    write_files(str(tmp_path), [80] * 10)
    data = Data(str(tmp_path), 32, rng=random.Random(0))
    for bad in ([0.49], [2.01], [], [1.0, 3.0], "fast", [None]):
        with pytest.raises(ValueError, match="stretch"):
            DeviceData(data, "cpu", 308, stretch=bad)
    with pytest.raises(ValueError, match="offsets"):
        DeviceData(data, "cpu", 308, transpose=[12])
    with pytest.raises(ValueError, match="offsets"):
        DeviceData(data, "cpu", 308, transpose=[])
    for codec in (REMI_EventSeq, MuMIDI_EventSeq):
        with pytest.raises(ValueError, match="time stretch needs the MIDI-like codec"):
            DeviceData(data, "cpu", codec.dim(), stretch=[1.0], codec=codec)
        assert DeviceData(data, "cpu", codec.dim(), transpose=[1], codec=codec).perm.shape == (1, codec.dim() + 1)
    assert check_stretch([0.5, 0.9996, 2.0]) == [500, 1000, 2000]
    x = torch.zeros(2, 4, dtype=torch.int32)
    from musicgeneration_amd import ops
    with pytest.raises(_lib.MgxError, match="no CPU fallback"):               # the feeder itself needs the device
        ops.crop_augment(torch.zeros(8, dtype=torch.uint16), torch.zeros(2, dtype=torch.int64), x[:, 0].contiguous(), x, None, 0)


# ---- the reference of the kernel against the header's own claims ---------------------------------------------------------------
TS0, N_TS = 208, 100


def units(ids):
    ids = np.asarray(ids)
    return int(np.where((ids >= TS0) & (ids < TS0 + N_TS), ids - TS0 + 1, 0).sum())


def test_reference_worked_example_of_the_header():
    out, total = augment_ref.stretch_row([TS0 + 99] * 6, 1005, TS0, N_TS)
    assert [v - TS0 + 1 for v in out] == [100, 1, 100, 100, 1, 100, 100, 1, 100] and total == 603


def test_reference_q_1000_is_the_identity_and_time_is_rounded_once():
    rng = np.random.default_rng(0)
    for trial in range(200):
        src = rng.integers(0, 312, int(rng.integers(1, 80)))
        if trial % 3 == 0:
            src = rng.integers(TS0, TS0 + N_TS, len(src))
        out, total = augment_ref.stretch_row(src, 1000, TS0, N_TS)
        assert out == src.tolist() and total == units(src)
        for q in (500, 501, 999, 1001, 1005, 1500, 2000, int(rng.integers(500, 2001))):
            out, total = augment_ref.stretch_row(src, q, TS0, N_TS)
            assert total == (units(src) * q + 500) // 1000 == units(out)          # no drift: the emitted ids last S_last units
            keep = [v for v in src.tolist() if not TS0 <= v < TS0 + N_TS]
            assert [v for v in out if not TS0 <= v < TS0 + N_TS] == keep             # everything else, in order, as it is
        for q in (0, 499, 2001, -1000):                                            # outside the range: 1000
            assert augment_ref.stretch_row(src, q, TS0, N_TS)[0] == src.tolist()


def test_reference_length_bounds_at_their_tight_cases():
    n = 50
    out, _ = augment_ref.stretch_row([TS0] * (2 * n), 500, TS0, N_TS)          # 1-unit shifts at q = 500: exactly n from 2 n
    assert len(out) == n
    assert len(augment_ref.stretch_row([TS0] * (2 * n - 1), 500, TS0, N_TS)[0]) == n      # (the odd token rounds up)
    assert len(augment_ref.stretch_row([TS0] * (2 * n - 2), 500, TS0, N_TS)[0]) == n - 1
    assert len(augment_ref.stretch_row([TS0] * n, 1000, TS0, N_TS)[0]) == n     # q >= 1000: every token emits
    assert len(augment_ref.stretch_row([TS0] * 600, 999, TS0, N_TS)[0]) == 599  # ... and just below it one, in time, does not
    rng = np.random.default_rng(1)
    for trial in range(300):
        q = int(rng.choice([500, 501, 600, 999, 1000, 1001, 2000]))
        kind = trial % 3
        src = [TS0] * (2 * n) if kind == 0 else rng.integers(TS0, TS0 + 3, 2 * n) if kind == 1 else rng.integers(200, 215, 2 * n)
        assert len(augment_ref.stretch_row(src, q, TS0, N_TS)[0]) >= n
        for i in range(2 * n - 1):                              # any two consecutive tokens emit at least one id
            before = len(augment_ref.stretch_row(src[:i], q, TS0, N_TS)[0]) if i % 10 == 0 else None
            if before is not None:
                assert len(augment_ref.stretch_row(src[:i + 2], q, TS0, N_TS)[0]) >= before + 1
        if q >= 1000:
            assert len(augment_ref.stretch_row(src[:n], q, TS0, N_TS)[0]) >= n


def test_reference_rows_pads_and_clamps():
    corpus = np.arange(100, 130)
    start, avail = np.array([0, 25, -1, 3, 30, 28]), np.array([30, 5, 9, -2, 4, 99])
    x, y, n_out = augment_ref.crop_augment(corpus, start, avail, 6, 7)
    assert n_out.tolist() == [6, 5, 0, 0, 0, 2]
    assert x.tolist()[0] == [100, 101, 102, 103, 104] and y.tolist()[0] == [101, 102, 103, 104, 105]
    assert x.tolist()[1] == [125, 126, 127, 128, 129] and y.tolist()[1] == [126, 127, 128, 129, 7]
    assert x.tolist()[5] == [128, 129, 7, 7, 7] and (x[2:5] == 7).all()
    perm = np.arange(130)[None, ::-1].copy()
    x2, _, _ = augment_ref.crop_augment(corpus, start, avail, 6, 7, perm=perm, shift_row=[0, 1, 0, 0, 0, -1], with_y=False)
    assert x2.tolist()[0] == [29, 28, 27, 26, 25, 24] and x2.tolist()[1] == [125, 126, 127, 128, 129, 7]
    assert x2.tolist()[5] == [128, 129, 7, 7, 7, 7]            # the pad is not looked up


# ---- header and command lines ----------------------------------------------------------------------------------------------------
def test_header_declares_the_call_and_abi_29():
    hdr = open(_lib.HEADER).read()
    assert "mgx_crop_augment" in _lib.FUNCTIONS and len(_lib.FUNCTIONS["mgx_crop_augment"][1]) == 20
    assert int(re.search(r"^#define MGX_ABI_VERSION (\d+)", hdr, re.M).group(1)) >= 29 and _lib.EXPECTED_ABI >= 29


def test_train_flags():
    base = train.get_options([])
    assert base.transpose == 0 and base.stretch is None and base.device_feeder is False
    assert train.augment_args(base) is None                    # no new flag: the host feeder
    got = train.augment_args(train.get_options(["--device-feeder"]))
    assert got["transpose"] is None and got["stretch"] is None and got["codec"] is EventSeq
    got = train.augment_args(train.get_options(["--transpose", "3", "--stretch", "0.95,1.0,1.05"]))
    assert got["transpose"] == [-3, -2, -1, 0, 1, 2, 3] and got["stretch"] == [0.95, 1.0, 1.05]
    assert train.augment_args(train.get_options(["--transpose", "11", "--repr", "remi"]))["codec"] is REMI_EventSeq
    assert train.augment_args(train.get_options(["--transpose", "1", "--repr", "mumidi"]))["codec"] is MuMIDI_EventSeq
    for bad, why in ((["--transpose", "12"], "0 .. 11"), (["--transpose", "-1"], "0 .. 11"),
                     (["--stretch", "1.0", "--repr", "remi"], "needs --repr midi_like"),
                     (["--stretch", "1.0", "--repr", "mumidi"], "tempo"),
                     (["--stretch", "0.4"], "0.5 .. 2.0"), (["--stretch", "1.0,2.5"], "0.5 .. 2.0"),
                     (["--stretch", "a,b"], "separated by commas"), (["--stretch", ""], "separated by commas")):
        with pytest.raises(ValueError, match=why):
            train.main(bad)                                    # refused before anything asks for a device


def test_melody_train_flags():
    assert melody_train.get_options(["-t"]).use_transposition is True and melody_train.get_options([]).use_transposition is False
    with pytest.raises(ValueError, match="--mode sequence"):
        melody_train.main(["-t", "--mode", "sequence"])
    assert list(melody_train.Transposer.TRANSPOSE_OFFSETS) == list(range(-6, 6))
