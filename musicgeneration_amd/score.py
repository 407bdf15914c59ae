"""Evaluate a checkpoint on whole pieces: the negative log-likelihood per event (nats, bits, perplexity) and the top-1 accuracy
of every file of a split, each scored in full -- pieces longer than the model's window in overlapping windows
(``MusicTransformer.score``, ``scoring.score_schedule``).  ``python -m musicgeneration_amd.score -s ckpt -d data_dir --split test``.

The reference has no such tool: its evaluation (train.py:150-170, generate.py:60-80) scores two random windows with the
label-smoothed loss (criterion.py:43-67); this is that log-softmax without the smoothing, over every event of every file."""
from __future__ import annotations

import json
import optparse
import os

import numpy as np
import torch

from . import config, scoring, utils
from .data import Data
from .network import MusicTransformer
from .train import vocab_of


def get_options(argv=None):
    parser = optparse.OptionParser()
    parser.add_option('-s', '--load_path', dest='load_path', type='string', default=None)
    parser.add_option('-d', '--dataset', dest='data_path', type='string', default=config.pickle_dir)
    parser.add_option('--split', dest='split', type='choice', choices=['valid', 'test'], default='test')
    parser.add_option('-M', '--max_seq', dest='max_seq', type='int', default=config.max_seq)
    parser.add_option('--d-model', dest='d_model', type='int', default=config.embedding_dim)
    parser.add_option('--num-layers', dest='num_layers', type='int', default=config.num_layers)
    parser.add_option('--repr', dest='repr', type='string', default='midi_like')
    parser.add_option('--field', dest='field', type='string', default=None, help="MuMIDI files: 'melody' or 'arrangement'")
    parser.add_option('-b', '--batch-size', dest='batch_size', type='int', default=8, help='files scored per call')
    parser.add_option('--stride', dest='stride', type='int', default=0, help='events between window starts (0 = default, W // 2)')
    parser.add_option('--window', dest='window', type='int', default=0, help='events per window, 2 .. -M (0 = -M)')
    parser.add_option('--logits', dest='logits', type='choice', choices=['fp32', 'bf16'], default='fp32',
                      help='fp32: log-sum-exp from the fp32 accumulators of the vocabulary projection; bf16: from the stored bf16 logits')
    parser.add_option('--json', dest='json', type='string', default=None, help='write the figures per file to this file')
    parser.add_option('--midi', dest='midi', type='string', default=None,
                      help='comma-separated MIDI files to score in place of a split (through the MIDI-like codec, as generate.py -c)')
    parser.add_option('--ema', dest='ema', action='store_true', default=False,
                      help="score the checkpoint's 'net_ema' (train.py --ema-decay), not its 'net'")
    return parser.parse_args(argv)[0]


def _pieces(o, vocab):
    """[(name, int array)] -- the --midi files, or every file of the split; ids outside the vocabulary are refused"""
    if o.midi:
        if o.repr != 'midi_like':
            raise SystemExit('--midi scores MIDI-like (EventSeq) events: use --repr midi_like')
        from .sequence import EventSeq, NoteSeq
        out = []
        for f in [f for f in o.midi.split(',') if f]:
            a = np.asarray(EventSeq.from_note_seq(NoteSeq.from_midi_file(f)).to_array())
            if len(a) < 2:
                raise SystemExit(f'{f}: fewer than 2 events in the MIDI-like pitch range')
            out.append((f, a))
        return out
    if not (o.data_path and os.path.isdir(o.data_path)):
        raise SystemExit(f'-d {o.data_path!r} is no directory')
    ds = Data(o.data_path, 2, field=o.field)                 # every file of at least 2 events, whole
    try:
        ds.check_vocab(vocab)
    except ValueError as e:
        raise SystemExit(str(e))
    return [(f, np.asarray(ds.array(f))) for f in ds.file_dict[o.split]]


def main(argv=None):
    o = get_options(argv)
    vocab = vocab_of(o.repr)
    W = o.window or o.max_seq
    try:                                                      # the window arguments, before any model or device work
        scoring.check_args(o.max_seq, o.d_model, 1, 2, logits=o.logits, window=W, stride=o.stride or None)
    except ValueError as e:
        raise SystemExit(str(e))
    if o.batch_size < 1:
        raise SystemExit(f'-b must be at least 1, got {o.batch_size}')
    net = utils.load_net(o.load_path, o.ema)
    pieces = _pieces(o, vocab)
    if not pieces:
        raise SystemExit(f'no file to score in the {o.split} split of {o.data_path}')
    device = torch.device('cuda:0')
    mt = MusicTransformer(embedding_dim=o.d_model, vocab_size=vocab, num_layer=o.num_layers, max_seq=o.max_seq, dropout=0)
    if net is not None:
        mt.load_state_dict(net)
    mt.to(device).eval()
    per_file, total, count, hits = [], 0.0, 0, 0
    for i in range(0, len(pieces), o.batch_size):
        part = pieces[i:i + o.batch_size]
        lens = [len(a) for _, a in part]
        x = np.full((len(part), max(lens)), vocab - 1, dtype=np.int64)
        for r, (_, a) in enumerate(part):
            x[r, :len(a)] = a
        res = mt.score(torch.from_numpy(x).to(device), lengths=lens, logits=o.logits, window=W, stride=o.stride or None)
        for (name, _), s, c, h in zip(part, res['sum'].tolist(), res['count'].tolist(), res['hits'].tolist()):
            per_file.append(dict(file=name, **scoring.figures(s, c, h)))
            total, count, hits = total + s, count + c, hits + h
    mt.check_no_leading_pads()
    fig = scoring.figures(total, count, hits)
    print('Score >>>> files: {}, events: {}, nats/event: {:.6f}, bits/event: {:.6f}, perplexity: {:.4f}, accuracy: {:.4f}'.format(
        len(per_file), fig['events'], fig['nats_per_event'], fig['bits_per_event'], fig['perplexity'], fig['accuracy']))
    if o.json:
        with open(o.json, 'w') as f:
            json.dump(dict(split=None if o.midi else o.split, window=W, stride=o.stride or scoring.default_stride(W), logits=o.logits,
                           total=dict(files=len(per_file), **fig), files=per_file), f, indent=1)
    return fig


if __name__ == '__main__':
    main()
