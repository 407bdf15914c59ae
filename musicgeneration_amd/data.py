"""Mirror of mg/model/MusicTransformer/data.py: ``Data(dir_path, max_length)`` with
``batch / slide_seq2seq_batch / seq2seq_batch / smallest_encoder_batch`` and ``file_dict``.

File format: each ``*.data`` file is ``torch.save(np.ndarray[uint8|uint16, T])`` written
by the reference's preprocess_*.py.  The reference unpickles every sampled file on every step
(data.py:96-107); here every file is loaded ONCE into host memory at construction (so the GPU is
not starved), and each rank may use its own ``random.Random`` stream (data-parallel sharding).
MuMIDI files hold a dict {'melody','arrangement'}; the reference's filter drops them
(len(dict) == 2 < max_length) -- pass ``field='melody'`` to train on one of the two arrays."""
from __future__ import annotations

import random
from typing import Dict, List, Optional

import numpy as np
import torch

from . import utils


def _load_array(fname, field=None):
    obj = torch.load(fname, weights_only=False)
    if isinstance(obj, dict):
        if field is None:
            return None, len(obj)
        obj = obj[field]
    arr = np.asarray(obj)
    return arr, len(arr)


class Data:
    def __init__(self, dir_path, max_length, field: Optional[str] = None, rng: Optional[random.Random] = None,
                 min_length: Optional[int] = None):
        """``min_length`` (extra): keep only files with at least this many events.  The reference keeps
        ``len >= max_length`` (data.py:33-40) although ``slide_seq2seq_batch`` crops ``max_length + 1`` events with
        ``randrange(0, len - (max_length+1))``: a file of exactly ``max_length`` events raises IndexError at sampling
        time and one of ``max_length + 1`` raises ValueError (empty range).  Data-parallel training passes
        ``min_length = max_length + 2`` so that no rank can ever skip a micro-batch on its own (every rank must
        issue the same collectives)."""
        self.files = list(utils.find_files_by_extensions(dir_path, ['.data']))
        self.field = field
        self.min_length = min_length
        self._rng = rng if rng is not None else random
        self._cache: Dict[str, np.ndarray] = {}
        n = len(self.files)
        self.file_dict = {
            'train': self.file_filter(self.files[:int(n * 0.8)], max_length),
            'valid': self.file_filter(self.files[int(n * 0.8): int(n * 0.9)], max_length),
            'test': self.file_filter(self.files[int(n * 0.9):], max_length),
        }
        self._seq_file_name_idx = 0
        self._seq_idx = 0

    def __repr__(self):
        return (f"<class Data has train: {len(self.file_dict['train'])}, val: {len(self.file_dict['valid'])},"
                f"test: {len(self.file_dict['test'])} files>")

    def file_filter(self, files, max_length):
        """keep files with len(data) >= max_length (data.py:33-40); arrays stay cached in RAM"""
        kept = []
        for fname in files:
            arr, n = _load_array(fname, self.field)
            if arr is not None and max(max_length, self.min_length or 0) <= n:
                self._cache[fname] = arr
                kept.append(fname)
        return kept

    def check_vocab(self, vocab_size):
        """Raise if any kept file holds a token id outside [0, vocab_size): the reference's nn.Embedding / one_hot raise
        on such input (a dataset / --repr mismatch), the HIP kernels would clamp silently.  Host-side, once per dataset."""
        for fname, arr in self._cache.items():
            if len(arr) and (int(arr.max()) >= vocab_size or int(arr.min()) < 0):
                raise ValueError(f"{fname}: token id {int(arr.max())} outside the vocabulary [0, {vocab_size}) "
                                 f"(dataset written for another event representation?)")

    def array(self, fname) -> np.ndarray:
        """the whole event array of a kept file (held in RAM since construction)"""
        return self._get_seq(fname)

    def _get_seq(self, fname, max_length=None):
        """random crop of max_length events (data.py:96-107); IndexError when the file is too short"""
        data = self._cache.get(fname)
        if data is None:
            data, _ = _load_array(fname, self.field)
            self._cache[fname] = data
        if max_length is not None:
            if max_length <= len(data):
                start = self._rng.randrange(0, len(data) - max_length)
                data = data[start:start + max_length]
            else:
                raise IndexError
        return data

    def batch(self, batch_size, length, mode='train'):
        batch_files = self._rng.sample(self.file_dict[mode], k=batch_size)
        batch_data = [self._get_seq(file, length) for file in batch_files]
        return np.array(batch_data, dtype=np.int16)

    def seq2seq_batch(self, batch_size, length, mode='train'):
        data = self.batch(batch_size, length * 2, mode)
        return data[:, :length], data[:, length:]

    def smallest_encoder_batch(self, batch_size, length, mode='train'):
        data = self.batch(batch_size, length * 2, mode)
        return data[:, :length // 100], data[:, length // 100:length // 100 + length]

    def slide_seq2seq_batch(self, batch_size, length, mode='train'):
        data = self.batch(batch_size, length + 1, mode)
        return data[:, :-1], data[:, 1:]


def check_stretch(stretch):
    """a list of time-stretch factors in 0.5 .. 2.0 -> their rounded per-mille; ValueError otherwise"""
    try:
        qs = [int(round(1000 * float(f))) for f in stretch]
    except (TypeError, ValueError):
        raise ValueError(f"stretch must be a list of factors in 0.5 .. 2.0, got {stretch!r}") from None
    if not qs or any(not 500 <= q <= 2000 for q in qs):
        raise ValueError(f"stretch must be a non-empty list of factors in 0.5 .. 2.0, got {list(stretch)}")
    return qs


class DeviceData:
    """The feeder of ``Data.slide_seq2seq_batch`` with the tokens on the device: the kept files of one split of ``data`` are
    uploaded ONCE as one flat 16-bit corpus, and a batch is one small staged copy (four per-row numbers) and one kernel
    (ops.crop_augment) that cuts the crops, stretches their time, transposes them and writes x and y.

    Which files and which starts: drawn from ``data``'s own random stream exactly as ``Data.batch`` draws them (``plan``), so
    without augmentation a batch holds the tokens the host feeder returns for the same seed.  The augmentation draws come from
    ``aug_rng``, a second stream: turning augmentation on never moves the crops.
      transpose: a list of semitone offsets (|offset| <= 11); per row one of them, uniformly; the codec's table is built once.
      stretch:   a list of factors in 0.5 .. 2.0, kept as rounded per-mille; per row one of them, uniformly.  Needs a codec whose
                 time ids are one linear run (``codec.stretch_ids``): the MIDI-like one.
      corpus (uint16), offsets and lengths (int64, per file of the split, also as ``offsets_host`` / ``lengths_host``): on the device.
      codec:     the event codec of the files (default ``sequence.EventSeq``); vocab_size: the model's (default: pad_token + 1
                 or the codec's ids, whichever is larger)."""

    def __init__(self, data: Data, device, pad_token, mode='train', transpose=None, stretch=None, aug_rng=None, codec=None,
                 vocab_size=None):
        if codec is None:
            from .sequence import EventSeq as codec
        if mode not in data.file_dict:
            raise ValueError(f"mode must be one of {sorted(data.file_dict)}, got {mode!r}")
        self.data, self.mode, self.device, self.pad_token = data, mode, torch.device(device), int(pad_token)
        V = max(codec.dim(), self.pad_token + 1) if vocab_size is None else int(vocab_size)
        self.offsets_semitones = None if transpose is None else [int(o) for o in transpose]
        table = None if transpose is None else codec.transpose_table(self.offsets_semitones, V)      # refuses |offset| > 11
        self.stretch_q, self.ts0, self.n_ts = None, 0, 0
        if stretch is not None:
            self.stretch_q = check_stretch(stretch)
            if not hasattr(codec, 'stretch_ids'):
                raise ValueError(f"{codec.__name__} carries time in bar, position and tempo tokens, not in a run of time-shift "
                                 "ids: a time stretch needs the MIDI-like codec")
            self.ts0, self.n_ts = codec.stretch_ids(V)
        self.aug_rng = aug_rng if aug_rng is not None else random.Random(0)
        self.files = list(data.file_dict[mode])
        arrays = [np.asarray(data.array(f)).reshape(-1) for f in self.files]
        for f, a in zip(self.files, arrays):
            if len(a) and (int(a.max()) > 65535 or int(a.min()) < 0):
                raise ValueError(f"{f}: token ids outside 0 .. 65535 do not fit the 16-bit corpus")
        self.lengths_host = np.array([len(a) for a in arrays], dtype=np.int64)
        self.offsets_host = np.concatenate([[0], np.cumsum(self.lengths_host)[:-1]]).astype(np.int64) if arrays else np.zeros(0, np.int64)
        flat = np.concatenate(arrays).astype(np.uint16) if arrays else np.zeros(0, np.uint16)
        self.corpus = torch.from_numpy(flat).to(self.device)
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self.lengths = torch.from_numpy(self.lengths_host).to(self.device)
        self.perm = None if table is None else torch.from_numpy(table).to(self.device)

    def plan(self, batch_size, length):
        """host only: the crops of the next batch, (file indices into the split, starts inside the files), int64 [batch_size]
        each -- ``Data.batch``'s draws from ``data``'s random stream: one ``sample`` of the files, then per file in order one
        ``randrange(0, len - (length + 1))``.  A file shorter than length + 1 raises IndexError, one of exactly length + 1
        ValueError, as there (and as there, the draws made before it are spent)"""
        rng = self.data._rng
        files = rng.sample(range(len(self.files)), k=batch_size)
        need = length + 1
        starts = []
        for f in files:
            n = int(self.lengths_host[f])
            if need > n:
                raise IndexError
            starts.append(rng.randrange(0, n - need))
        return np.array(files, dtype=np.int64), np.array(starts, dtype=np.int64)

    def draw_augmentation(self, batch_size):
        """host only: per row the table row of its transposition and its stretch in per-mille, from ``aug_rng`` (row after
        row: the shift, then the factor); None for an augmentation that is off"""
        shift = [] if self.perm is not None else None
        q = [] if self.stretch_q is not None else None
        for _ in range(batch_size):
            if shift is not None:
                shift.append(self.aug_rng.randrange(len(self.offsets_semitones)))
            if q is not None:
                q.append(self.stretch_q[self.aug_rng.randrange(len(self.stretch_q))])
        return shift, q

    def slide_seq2seq_batch(self, batch_size, length, crops=None):
        """-> (x, y) int32 [batch_size, length] on the device: ``Data.slide_seq2seq_batch`` of the split, augmented.
        ``crops``: what ``plan(batch_size, length)`` returned, for a caller that handles a failed draw apart from the launch"""
        from . import ops
        files, starts = self.plan(batch_size, length) if crops is None else crops
        shift, q = self.draw_augmentation(batch_size)
        B = batch_size
        # the four per-row arrays in one pinned buffer (int32 words: start as int64 first) and one copy
        stage = torch.empty(5 * B, dtype=torch.int32, pin_memory=self.device.type == 'cuda')
        host = stage.numpy()
        host[:2 * B].view(np.int64)[:] = self.offsets_host[files] + starts
        host[2 * B:3 * B] = self.lengths_host[files] - starts
        host[3 * B:4 * B] = 0 if shift is None else shift
        host[4 * B:] = 1000 if q is None else q
        dev = stage.to(self.device, non_blocking=True)
        x = torch.empty(B, length, dtype=torch.int32, device=self.device)
        y = torch.empty_like(x)
        ops.crop_augment(self.corpus, dev[:2 * B].view(torch.int64), dev[2 * B:3 * B], x, y, self.pad_token, perm=self.perm,
                         shift_row=None if shift is None else dev[3 * B:4 * B],
                         stretch_q=None if q is None else dev[4 * B:], ts0=self.ts0, n_ts=self.n_ts)
        return x, y


# --------------------------------------------------------------------------------------------------
# GRU feeder: mirror of mg/model/utils/data.py:23-47 (SeqBatchify, MyDataset) and :49-123 (Event_Dataset)
# --------------------------------------------------------------------------------------------------
def flatten_padded_sequences(outs, lengths):
    """[B, mx, V] batch-first outputs -> the rows that have a label, concatenated: outs[i, :lengths[i]-1] for every i
    (utils/data.py:14-21); pairs with SeqBatchify's Y."""
    if lengths is None:
        return outs.contiguous().view(-1, outs.shape[-1])
    return torch.cat([outs[i, :int(lengths[i]) - 1] for i in range(outs.shape[0])], 0)


def SeqBatchify(inputs):
    """sort by length (desc), zero-pad to the longest -> (X int16 [B,Tmax], Y = concat of X[i,1:len_i], lengths)"""
    inputs = sorted(inputs, key=lambda i: len(i), reverse=True)
    lengths = np.array([len(item) for item in inputs])
    mx_length = np.max(lengths)
    X = np.zeros((len(inputs), mx_length), dtype=np.int16)
    for i in range(len(inputs)):
        X[i, :lengths[i]] = np.array(inputs[i])
    Y = np.concatenate([np.array(X[i])[1:lengths[i]] for i in range(len(inputs))])
    return X, Y, lengths


class MyDataset(torch.utils.data.Dataset):
    def __init__(self, seqs):
        self.seqs = seqs

    def __getitem__(self, index):
        return self.seqs[index]

    def __len__(self):
        return len(self.seqs)


class Event_Dataset:
    """All ``*.data`` arrays with len >= limlen, held in RAM; window index + time-major collate."""

    def __init__(self, root, limlen=None, verbose=False):
        import os
        assert os.path.isdir(root), root
        self.root = root
        self.samples = []
        self.seqlens = []
        for path in utils.find_files_by_extensions(root, ['.data']):
            eventseq, n = _load_array(path)
            if eventseq is not None and n >= (limlen or 0):
                self.samples.append(eventseq)
                self.seqlens.append(n)
        self.avglen = np.mean(self.seqlens) if self.seqlens else 0.0

    def count(self, v):
        a = sorted(self.seqlens)
        x = int(np.searchsorted(a, v, side='left'))
        return 100 * x / len(a)

    def batches(self, batch_size, window_size, stride_size):
        """list of (file index, (start, end)) windows            utils/data.py:74-78"""
        return [(i, (j, j + window_size))
                for i, seqlen in enumerate(self.seqlens)
                for j in range(0, seqlen - window_size, stride_size)]

    def SegBatchify(self, data):
        """collate -> np [T, B] (time-major)                      utils/data.py:104-114"""
        return np.stack([self.samples[i][start:end] for i, (start, end) in data], axis=1)

    Batchify = SegBatchify

    def __repr__(self):
        return (f'Dataset(root="{self.root}", samples={len(self.samples)}, avglen={self.avglen})')
