"""Token-id layout shared by the three event codecs (sequence.EventSeq, REMI_EventSeq, MuMIDI_EventSeq).

A codec's vocabulary is an ordered list of (feature name, number of slots); ids are handed out feature after feature
with no gaps.  The reference spells the same arithmetic out once per codec (utils/sequence.py:204-221, utils/REMI.py:434-474,
utils/MuMIDI.py:352-405); here it lives in one place and the codecs only state their layouts."""
from __future__ import annotations

import collections
from itertools import accumulate
from typing import Callable, Iterable, Optional, Sequence, Tuple

import numpy as np


def slots(layout: Iterable[Tuple[str, int]]) -> "collections.OrderedDict[str, int]":
    """feature -> number of ids, in vocabulary order"""
    return collections.OrderedDict(layout)


def id_ranges(layout: Iterable[Tuple[str, int]]) -> "collections.OrderedDict[str, range]":
    """feature -> range of its ids (consecutive features are adjacent)"""
    names, sizes = zip(*layout)
    ends = list(accumulate(sizes))
    return collections.OrderedDict((n, range(e - s, e)) for n, s, e in zip(names, sizes, ends))


def id_table(ranges: "collections.OrderedDict[str, range]",
             label: Optional[Callable[[str, int], str]] = None) -> "collections.OrderedDict[int, Tuple[str, int]]":
    """id -> (feature name, value inside the feature); ``label(feature, value)`` may substitute the reported name"""
    table = collections.OrderedDict()
    for name, ids in ranges.items():
        table.update((i, (label(name, v) if label else name, v)) for v, i in enumerate(ids))
    return table


def word_dtype(vocab_size: int):
    """ids are stored as uint8 while they fit, uint16 beyond (the reference's on-disk choice)"""
    return np.uint8 if vocab_size <= 256 else np.uint16


def encode(pairs: Sequence[Tuple[range, int]], vocab_size: int) -> np.ndarray:
    """[(feature id range, value)] -> id array.  ``range.__getitem__`` raises IndexError for a value the feature has no
    slot for -- the reference's behaviour (e.g. REMI note_velocity >= 4), kept on purpose."""
    return np.array([ids[v] for ids, v in pairs], dtype=word_dtype(vocab_size))


# ---- transposition tables (train-time augmentation: data.DeviceData, ops.crop_augment) -----------------------------------------
MAX_TRANSPOSE = 11                                         # semitones: beyond an octave the wrap below is no transposition


def transpose_table(dim: int, offsets, vocab_size=None, pitch_runs=(), chord_run: Optional[range] = None) -> np.ndarray:
    """int32 [len(offsets), V]: row s maps every id to its id under a transposition by offsets[s] semitones.

    ``pitch_runs``: id ranges whose slot k is a pitch -- slot k goes to k + offset, and a slot that would leave the run comes
    back by an octave (-12 above, +12 below: utils/shared.py:36-68 of the reference).  ``chord_run``: ids quality * 12 + root
    followed by one 'no chord' id -- the root goes to (root + offset) mod 12, the last id stays.  Every other id, and the ids a
    model adds beyond ``dim`` (its pad id), map to themselves."""
    V = dim if vocab_size is None else int(vocab_size)
    if V < dim:
        raise ValueError(f"vocab_size ({V}) is below the codec's {dim} ids")
    offsets = [int(o) for o in offsets]
    if not offsets or any(abs(o) > MAX_TRANSPOSE for o in offsets):
        raise ValueError(f"transposition offsets must be a non-empty list of semitones in -{MAX_TRANSPOSE} .. {MAX_TRANSPOSE}, got {offsets}")
    table = np.tile(np.arange(V, dtype=np.int32), (len(offsets), 1))
    for s, off in enumerate(offsets):
        for run in pitch_runs:
            if len(run) < 2 * 12:
                raise ValueError("a pitch run shorter than two octaves cannot wrap by one")
            k = np.arange(len(run)) + off
            k = np.where(k >= len(run), k - 12, np.where(k < 0, k + 12, k))
            table[s, run.start:run.stop] = run.start + k
        if chord_run is not None:
            c = np.arange(len(chord_run) - 1)
            table[s, chord_run.start:chord_run.stop - 1] = chord_run.start + (c // 12) * 12 + (c % 12 + off) % 12
    return table


def repeat_subject(dim, note_on, vocab_size=None):
    """the ids that repetition control counts, int32 [vocab_size]: 1 on the run ``note_on``, 0 elsewhere and on the ids a model
    adds beyond ``dim`` (its pad id)"""
    V = dim if vocab_size is None else int(vocab_size)
    if V < dim:
        raise ValueError(f"vocab_size ({V}) is below the codec's {dim} ids")
    subject = np.zeros(V, dtype=np.int32)
    subject[note_on.start:note_on.stop] = 1
    return subject


def event_classes(ranges, vocab_size=None):
    """the classes of per-class sampling (``decode.ClassSampling``): (names, classes int32 [vocab_size]).  The layout's features in
    id order, one class each, then a last class 'other' for the ids a model adds beyond the codec's (its pad id)"""
    dim = sum(len(r) for r in ranges.values())
    V = dim if vocab_size is None else int(vocab_size)
    if V < dim:
        raise ValueError(f"vocab_size ({V}) is below the codec's {dim} ids")
    names = list(ranges) + ['other']
    classes = np.full(V, len(names) - 1, dtype=np.int32)
    for c, ids in enumerate(ranges.values()):
        classes[ids.start:ids.stop] = c
    return names, classes
