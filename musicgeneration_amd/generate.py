"""Drop-in for mg/model/MusicTransformer/generate.py:18-123: load a checkpoint, print a 2-sample test
loss/accuracy, sample ``--max-length`` events from a prior and write them out.
MIDI-like and REMI samples are written as .mid files (pretty_midi if installed, else the built-in SMF writer,
smf.py; REMI / MuMIDI through their write_midi on the same writer)."""
from __future__ import annotations

import optparse
import os

import numpy as np
import torch

from . import config, utils
from .criterion import SmoothCrossEntropyLoss
from .data import Data
from .metrics import CategoricalAccuracy, LogitsBucketting, MetricsSet
from .network import MusicTransformer
from .train import vocab_of


def get_options(argv=None):
    parser = optparse.OptionParser()
    parser.add_option('-b', '--batch-size', dest='batch_size', type='int', default=8)
    parser.add_option('-s', '--load_path', dest='load_path', type='string', default=None)
    parser.add_option('-o', '--output-dir', dest='output_dir', type='string', default='./output/generate/')
    parser.add_option('-d', '--dataset', dest='data_path', type='string', default=config.pickle_dir)
    parser.add_option('-l', '--max-length', dest='max_len', type='int', default=config.length)
    parser.add_option('-T', '--temperature', dest='temperature', type='float', default=1.0)
    parser.add_option('--top-k', dest='top_k', type='int', default=0)
    parser.add_option('--top-p', dest='top_p', type='float', default=1.0)
    parser.add_option('--num-layers', dest='num_layers', type='int', default=config.num_layers)
    parser.add_option('--d-model', dest='d_model', type='int', default=config.embedding_dim)
    parser.add_option('--repr', dest='repr', type='string', default='midi_like')
    parser.add_option('--grammar', dest='grammar', action='store_true', default=False,
                      help='constrain sampling to the REMI / MuMIDI event grammar (KV-cache decode, mask inside the sampler)')
    parser.add_option('--reference-mask', dest='reference_mask', action='store_true', default=False,
                      help="sample exactly as the reference's generate() does: Decoder(window, mask=None), i.e. no look-ahead "
                           'mask at sampling time (network.py:60); default: the training-time causal semantics')
    parser.add_option('-M', '--max_seq', dest='max_seq', type='int', default=config.max_seq)
    parser.add_option('-c', '--condition-file', dest='condition_file', type='string', default=getattr(config, 'condition_file', None),
                      help='MIDI file to continue (the reference reads config.condition_file, generate.py:101-105): its '
                           'first 500 MIDI-like events become the prior of every sample')
    parser.add_option('--condition-files', dest='condition_files', type='string', default=None,
                      help='comma-separated MIDI files to continue in one batch: each file is one sample (-b is ignored), '
                           'its first 500 MIDI-like events that sample\'s prompt (KV-cache decode over prompts of different '
                           'lengths)')
    parser.add_option('--kv-cache', dest='kv_cache', type='choice', choices=['bf16', 'fp8'], default='bf16',
                      help='K/V cache of the KV-cache decode (--grammar, --condition-files, --window): bf16 (default) or fp8, '
                           'e4m3fn codes with one scale per row -- half the bytes per key, samples differ from bf16')
    parser.add_option('--window', dest='window', type='int', default=0,
                      help='generate past -M with the KV-cache decode: a window of at most W tokens that is re-anchored (oldest '
                           'tokens dropped, positions renumbered from 0, K/V rebuilt in one pass) every --hop tokens; 0 = off. '
                           "--window 499 --hop 1 is the reference's threshold_len = 500 window")
    parser.add_option('--hop', dest='hop', type='int', default=0,
                      help='tokens dropped per re-anchor of --window (0 = default, max(1, W // 8))')
    parser.add_option('-B', '--beam-size', dest='beam_size', type='int', default=0,
                      help='beam search over the KV-cache decode with this many beams per sample (1 .. 16; 1 = greedy); 0 = off, '
                           'sample.  Each of the -b samples is searched with its own beam and the best beam is written')
    parser.add_option('-S', '--stochastic-beam-search', dest='stochastic_beam_search', action='store_true', default=False,
                      help='with -B: choose the surviving beams by Gumbel-perturbed scores')
    parser.add_option('--best-of', dest='best_of', type='int', default=1,
                      help='draw N candidates per sample (a batch of b * N rows, every prompt repeated N times), score every '
                           'continuation with the model at temperature 1 (MusicTransformer.score) and write the most likely one')
    parser.add_option('--share-prompt', dest='share_prompt', action='store_true', default=False,
                      help='KV-cache decode of the samples of one prompt over ONE copy of its K/V: with -c FILE (or --grammar) the '
                           '-b x --best-of samples (16 at most) share the prompt, with --condition-files the --best-of N candidates '
                           'of every file do (the prompt is prefilled once, not once per sample)')
    parser.add_option('--seconds', dest='seconds', type='float', default=None,
                      help='generate S seconds of music after the prompt (--repr midi_like; KV-cache decode with a per-sample clock '
                           'on the device): every sample ends exactly on S, in 0.01 s units, and -l becomes the cap on its events')
    parser.add_option('--bars', dest='bars', type='int', default=None,
                      help='generate N bars (--repr remi): every sample ends where its N-th new bar token would begin, and -l '
                           'becomes the cap on its events.  With --grammar: exactly N bars after the one-bar prompt')
    parser.add_option('--well-formed', dest='well_formed', action='store_true', default=False,
                      help='keep every sample a well-formed note stream (--repr midi_like; KV-cache decode with the set of held '
                           'notes per sample on the device): no note_off of a silent pitch, no note_on of a sounding one, '
                           'counted from what the prompt leaves sounding')
    parser.add_option('--max-polyphony', dest='max_polyphony', type='int', default=None,
                      help='at most K notes sounding at once (1 .. 128): no note_on while K are held.  Implies --well-formed')
    parser.add_option('--release', dest='release', action='store_true', default=False,
                      help='close the notes a sample still holds where it ends: their note_off events are appended before the '
                           'MIDI file is written (--repr midi_like; with --seconds: after the events the sample kept)')
    parser.add_option('--presence-penalty', dest='presence_penalty', type='float', default=0.0,
                      help='repetition control (KV-cache decode): subtract X from the logit of every --repeat-ids event that occurs '
                           'among the last --repeat-window events of the sample, the prompt included.  With --best-of the '
                           'candidates are ranked by their unpenalised score')
    parser.add_option('--frequency-penalty', dest='frequency_penalty', type='float', default=0.0,
                      help='subtract X times the number of its occurrences among the last --repeat-window events')
    parser.add_option('--repeat-window', dest='repeat_window', type='int', default=64,
                      help='the events the two penalties look back over (1 .. 4096; default 64)')
    parser.add_option('--repeat-ids', dest='repeat_ids', type='choice', choices=['pitch', 'all'], default='pitch',
                      help="the events the two penalties apply to: 'pitch' (default), the note_on events of the --repr -- a penalty "
                           "on time events would distort the rhythm -- or 'all', every event but the pad")
    parser.add_option('--no-repeat-ngram', dest='no_repeat_ngram', type='int', default=0,
                      help='no run of N events (2 .. 64) occurs twice: an event that would complete a run the sample holds already '
                           'loses 1e4 from its logit (it is still drawn where --grammar, --seconds or --well-formed leave nothing else)')
    parser.add_option('--ngram-span', dest='ngram_span', type='int', default=0,
                      help='the events --no-repeat-ngram looks back over (>= N); 0 (default): the whole sequence so far')
    parser.add_option('--lookahead', dest='lookahead', type='int', default=0,
                      help='draft and verify (KV-cache decode): T positions per step and sample (2 .. 8; 0 = off).  A step guesses '
                           'the next T - 1 events from the sample\'s own history and keeps the guesses the sampler would have drawn: '
                           'the same sample for a seed, 1 to T events per step')
    parser.add_option('--draft-ngram', dest='draft_ngram', type='int', default=3,
                      help='with --lookahead: the longest run of last events whose earlier occurrence is continued (1 .. 8; default 3)')
    parser.add_option('--class-temperature', dest='class_temperature', type='string', default=None,
                      help='per-class sampling (KV-cache decode): NAME=T,NAME=T -- the events of class NAME (the event types of the '
                           "--repr, e.g. time_shift=0.8,note_on=1.2) are drawn at temperature T inside their class; a class's total "
                           'probability stays what -t gives it.  With --best-of the candidates are ranked by the model\'s own score')
    parser.add_option('--class-top-k', dest='class_top_k', type='string', default=None,
                      help='NAME=K,...: the events of class NAME come from the K most likely of that class (e.g. velocity=4)')
    parser.add_option('--class-top-p', dest='class_top_p', type='string', default=None,
                      help='NAME=P,...: the events of class NAME come from the nucleus of mass P of that class (e.g. chord=0.9)')
    parser.add_option('--min-p', dest='min_p', type='float', default=0.0,
                      help='entropy-aware sampling (KV-cache decode): keep the events with at least this share of the most likely '
                           "event's probability (0 .. 1; 0 = off) -- a cut that widens where the model is unsure and narrows where "
                           'it is certain.  With --best-of the candidates are ranked by the model\'s own score')
    parser.add_option('--typical-p', dest='typical_p', type='float', default=1.0,
                      help="locally typical sampling: keep the events whose surprise lies closest to the step's entropy, up to this "
                           'mass (0 .. 1; 1 = off)')
    parser.add_option('--mirostat', dest='mirostat', type='float', default=None,
                      help='Mirostat v2: hold the surprise of the sampled events near TAU bits with a feedback loop per sample '
                           '(e.g. 3; not with --lookahead)')
    parser.add_option('--mirostat-eta', dest='mirostat_eta', type='float', default=None,
                      help="with --mirostat: the loop's learning rate (0 .. 1; default 0.1)")
    parser.add_option('--ema', dest='ema', action='store_true', default=False,
                      help="sample from the checkpoint's 'net_ema' (train.py --ema-decay), not from 'net'")
    return parser.parse_args(argv)[0]


def _check_beam_options(o):
    """-B / -S against the options a search does not offer, before any model or device work"""
    if o.stochastic_beam_search and not o.beam_size:
        raise SystemExit('-S/--stochastic-beam-search chooses the beams of a search: add -B K')
    if not o.beam_size:
        return
    if not 1 <= o.beam_size <= 16:
        raise SystemExit(f'-B/--beam-size must lie in 1 .. 16 (0 = off), got {o.beam_size}')
    if o.window:
        raise SystemExit('-B/--beam-size cannot be combined with --window (a search keeps every beam\'s whole cache)')
    if o.top_k:
        raise SystemExit('-B/--beam-size cannot be combined with --top-k (a search ranks all events; top-k filters a sampler)')
    if o.top_p != 1.0:
        raise SystemExit('-B/--beam-size cannot be combined with --top-p (a search ranks all events; top-p filters a sampler)')
    if o.reference_mask:
        raise SystemExit('-B/--beam-size cannot be combined with --reference-mask (the KV-cache decode is causal)')


def _check_best_of(o):
    """--best-of against -B, before any model or device work"""
    if o.best_of < 1:
        raise SystemExit(f'--best-of must be at least 1, got {o.best_of}')
    if o.best_of > 1 and o.beam_size:
        raise SystemExit('--best-of cannot be combined with -B/--beam-size (a search returns its best beam; --best-of ranks samples)')


def _check_share_prompt(o):
    """--share-prompt against what the shared prompt cache leaves out, before any model or device work"""
    if not o.share_prompt:
        return
    for on, what, why in ((o.window, '--window', "a re-anchor would rebuild every sample's own window"),
                          (o.kv_cache != 'bf16', '--kv-cache ' + o.kv_cache, 'the shared prompt cache is bf16'),
                          (o.beam_size, '-B/--beam-size', 'a search reorders whole cache rows between its beams'),
                          (o.reference_mask, '--reference-mask', 'the KV-cache decode is causal')):
        if on:
            raise SystemExit(f'--share-prompt cannot be combined with {what} ({why})')
    if o.condition_files is None and o.condition_file is None and not o.grammar:
        raise SystemExit('--share-prompt shares a prompt between its samples: add -c FILE, --condition-files or --grammar')
    n = o.best_of if o.condition_files is not None else o.batch_size * o.best_of
    if not 1 <= n <= 16:
        raise SystemExit(f'--share-prompt decodes at most 16 samples per prompt, got {n}'
                         + (' (--best-of)' if o.condition_files is not None else ' (-b x --best-of)'))


def _check_timed(o):
    """--seconds / --bars against the options a length budget does not offer, before any model or device work.  Returns the
    keyword arguments of generate_timed that the flag sets (None without either)"""
    if o.seconds is None and o.bars is None:
        return None
    if o.seconds is not None and o.bars is not None:
        raise SystemExit('--seconds and --bars are two budgets for one clock: give one')
    flag, need = ('--seconds', 'midi_like') if o.seconds is not None else ('--bars', 'remi')
    if o.repr != need:
        raise SystemExit(f'{flag} prices the events of --repr {need}, got --repr {o.repr}')
    for on, what, why in ((o.beam_size, '-B/--beam-size', 'a beam has no clock of its own'),
                          (o.share_prompt, '--share-prompt', 'the shared prompt cache is another decode driver'),
                          (o.best_of > 1, '--best-of', 'candidates of different lengths are not ranked against each other'),
                          (o.reference_mask, '--reference-mask', 'the KV-cache decode is causal')):
        if on:
            raise SystemExit(f'{flag} cannot be combined with {what} ({why})')
    from .sequence import TIME_UNITS_PER_SECOND
    budget = int(round(TIME_UNITS_PER_SECOND * o.seconds)) if o.seconds is not None else o.bars
    if budget < 0:
        raise SystemExit(f'{flag} must be >= 0, got {o.seconds if o.seconds is not None else o.bars}')
    return dict(budget=budget, inclusive=o.seconds is not None)


def _check_notes(o):
    """--well-formed / --max-polyphony / --release against the options they do not go with, before any model or device work.
    Returns whether sampling is constrained (--max-polyphony implies --well-formed)"""
    well = o.well_formed or o.max_polyphony is not None
    if not well and not o.release:
        return False
    flag = '--max-polyphony' if o.max_polyphony is not None else '--well-formed' if o.well_formed else '--release'
    if o.repr != 'midi_like':
        raise SystemExit(f'{flag} follows the note_on / note_off events of --repr midi_like, got --repr {o.repr}')
    for on, what, why in ((o.beam_size, '-B/--beam-size', "a beam's held notes would have to follow its parent: not built"),
                          (o.grammar, '--grammar', 'the two masks together can leave a sample no event'),
                          (well and o.reference_mask, '--reference-mask', 'the KV-cache decode is causal')):
        if on:
            raise SystemExit(f'{flag} cannot be combined with {what} ({why})')
    if o.max_polyphony is not None and not 1 <= o.max_polyphony <= 128:
        raise SystemExit(f'--max-polyphony must lie in 1 .. 128, got {o.max_polyphony}')
    return well


def _check_repeat(o):
    """--presence-penalty / --frequency-penalty / --repeat-window / --repeat-ids / --no-repeat-ngram / --ngram-span against the
    options they do not go with and their own ranges, before any model or device work.  Returns whether any of them is given"""
    d = get_options([])
    names = ('presence_penalty', 'frequency_penalty', 'repeat_window', 'repeat_ids', 'no_repeat_ngram', 'ngram_span')
    given = [n for n in names if getattr(o, n) != getattr(d, n)]
    if not given:
        return False
    flag = '--' + given[0].replace('_', '-')
    for on, what, why in ((o.beam_size, '-B/--beam-size', 'a search ranks whole beams by likelihood: not built'),
                          (o.reference_mask, '--reference-mask', 'the KV-cache decode is causal')):
        if on:
            raise SystemExit(f'{flag} cannot be combined with {what} ({why})')
    from .ops import REPEAT_MAX_NGRAM, REPEAT_MAX_WINDOW
    for name in ('presence_penalty', 'frequency_penalty'):
        v = getattr(o, name)
        if not (np.isfinite(v) and v >= 0):
            raise SystemExit(f"--{name.replace('_', '-')} must be a finite number >= 0, got {v}")
    if not 1 <= o.repeat_window <= REPEAT_MAX_WINDOW:
        raise SystemExit(f'--repeat-window must lie in 1 .. {REPEAT_MAX_WINDOW}, got {o.repeat_window}')
    if o.no_repeat_ngram and not 2 <= o.no_repeat_ngram <= REPEAT_MAX_NGRAM:
        raise SystemExit(f'--no-repeat-ngram must lie in 2 .. {REPEAT_MAX_NGRAM} (0 = off), got {o.no_repeat_ngram}')
    if o.ngram_span and o.ngram_span < max(o.no_repeat_ngram, 1):
        raise SystemExit(f'--ngram-span must be 0 (the whole sequence) or >= --no-repeat-ngram {o.no_repeat_ngram}, got {o.ngram_span}')
    if o.presence_penalty + o.frequency_penalty * o.repeat_window > 1e4:
        raise SystemExit('--presence-penalty + --frequency-penalty x --repeat-window must not exceed 1e4, got '
                         f'{o.presence_penalty + o.frequency_penalty * o.repeat_window:g}')
    return True


def _check_lookahead(o, timed, well, repeat):
    """--lookahead / --draft-ngram against the options draft and verify does not offer, before any model or device work"""
    if not o.lookahead:
        if o.draft_ngram != 3:
            raise SystemExit('--draft-ngram is the history match of --lookahead: add --lookahead T')
        return
    for on, what, why in ((o.beam_size, '-B/--beam-size', 'a search has no single draw per position to verify a guess against'),
                          (o.share_prompt, '--share-prompt', 'the shared prompt cache is another decode driver'),
                          (o.window, '--window', 'a re-anchor would have to fall between two accepted events'),
                          (o.kv_cache != 'bf16', '--kv-cache ' + o.kv_cache, 'the T-query attention has no 8-bit form'),
                          (timed, '--seconds / --bars', "a budget's state is sequential"),
                          (well, '--well-formed / --max-polyphony', 'the held-note state is sequential'),
                          (repeat, 'the repetition flags', 'the penalty of an event counts the event before it'),
                          (o.reference_mask, '--reference-mask', 'the KV-cache decode is causal')):
        if on:
            raise SystemExit(f'--lookahead cannot be combined with {what} ({why})')
    if not 2 <= o.lookahead <= 8:
        raise SystemExit(f'--lookahead must lie in 2 .. 8 (0 = off), got {o.lookahead}')
    if not 1 <= o.draft_ngram <= 8:
        raise SystemExit(f'--draft-ngram must lie in 1 .. 8, got {o.draft_ngram}')


def _codec(o):
    """the codec class of --repr"""
    if o.repr == 'remi':
        from .REMI import REMI_EventSeq as Codec
    elif o.repr == 'mumidi':
        from .MuMIDI import MuMIDI_EventSeq as Codec
    else:
        from .sequence import EventSeq as Codec
    return Codec


def _check_class(o, well):
    """--class-temperature / --class-top-k / --class-top-p against the options they do not go with, the class names of the --repr
    and their own ranges, before any model or device work.  Returns the three {class index: value} dicts (None without a flag)"""
    flags = (('--class-temperature', o.class_temperature, float, lambda v: np.isfinite(v) and v > 0, 'a finite number > 0'),
             ('--class-top-k', o.class_top_k, int, lambda v: v >= 0, 'an integer >= 0'),
             ('--class-top-p', o.class_top_p, float, lambda v: 0 < v <= 1, 'a number in (0, 1]'))
    given = [f for f, text, *_ in flags if text is not None]
    if not given:
        return None
    for on, what, why in ((o.beam_size, '-B/--beam-size', 'a search ranks whole beams by likelihood: not built'),
                          (o.reference_mask, '--reference-mask', 'the KV-cache decode is causal'),
                          (well, '--well-formed / --max-polyphony', 'that step draws twice and an in-place rewrite of the logits '
                                                                    'cannot serve both: later work')):
        if on:
            raise SystemExit(f'{given[0]} cannot be combined with {what} ({why})')
    names = _codec(o).event_classes()[0]
    out = []
    for flag, text, conv, valid, what in flags:
        vals = {}
        for item in (text or '').split(','):
            if not item:
                continue
            name, eq, v = item.partition('=')
            if not eq or name not in names:
                raise SystemExit(f"{flag}: '{item}' is not NAME=VALUE with a class of --repr {o.repr}: the classes are "
                                 + ', '.join(names))
            try:
                val = conv(v)
            except ValueError:
                val = None
            if val is None or not valid(val):
                raise SystemExit(f'{flag}: {name} must be {what}, got {v!r}')
            vals[names.index(name)] = val
        out.append(vals)
    return tuple(out)


def _class_args(o, mt, classes):
    """the keyword argument of generate_cached / generate_timed that the --class-* flags set"""
    from .decode import ClassSampling
    return dict(class_sampling=ClassSampling(_codec(o).event_classes(mt.vocab_size)[1], *classes))


def _check_entropy(o, well):
    """--min-p / --typical-p / --mirostat / --mirostat-eta against the options they do not go with and their own ranges, before
    any model or device work.  Returns the keyword argument of generate_cached / generate_timed they set ({} without a flag)"""
    given = [f for f, on in (('--min-p', o.min_p != 0), ('--typical-p', o.typical_p != 1), ('--mirostat', o.mirostat is not None))
             if on]
    if not given:
        if o.mirostat_eta is not None:
            raise SystemExit("--mirostat-eta is the learning rate of --mirostat's loop: add --mirostat TAU")
        return {}
    for on, what, why in ((o.beam_size, '-B/--beam-size', 'a search ranks whole beams by likelihood: not built'),
                          (o.reference_mask, '--reference-mask', 'the KV-cache decode is causal'),
                          (well, '--well-formed / --max-polyphony', 'that step draws twice and one mask cannot serve both draws: '
                                                                    'later work')):
        if on:
            raise SystemExit(f'{given[0]} cannot be combined with {what} ({why})')
    if not (np.isfinite(o.min_p) and 0 <= o.min_p < 1):
        raise SystemExit(f'--min-p must lie in 0 .. 1 (0 = off, 1 excluded), got {o.min_p}')
    if not (np.isfinite(o.typical_p) and 0 < o.typical_p <= 1):
        raise SystemExit(f'--typical-p must lie in 0 .. 1 (1 = off, 0 excluded), got {o.typical_p}')
    if o.mirostat is None and o.mirostat_eta is not None:
        raise SystemExit("--mirostat-eta is the learning rate of --mirostat's loop: add --mirostat TAU")
    if o.mirostat is not None:
        if not (np.isfinite(o.mirostat) and o.mirostat > 0):
            raise SystemExit(f'--mirostat must be a number of bits > 0, got {o.mirostat}')
        if o.mirostat_eta is not None and not (np.isfinite(o.mirostat_eta) and 0 < o.mirostat_eta <= 1):
            raise SystemExit(f'--mirostat-eta must lie in 0 .. 1 (0 excluded), got {o.mirostat_eta}')
        if o.lookahead:
            raise SystemExit('--mirostat cannot be combined with --lookahead (the loop is sequential: the cut of an event depends '
                             'on the event drawn before it: later work)')
    from .decode import EntropySampling
    return dict(entropy_sampling=EntropySampling(o.min_p, o.typical_p, o.mirostat, 0.1 if o.mirostat_eta is None else o.mirostat_eta))


def _repeat_args(o, mt):
    """the keyword argument of generate_cached / generate_timed that the repetition flags set"""
    from .decode import Repetition
    if o.repeat_ids == 'all':
        subject = np.ones(mt.vocab_size, dtype=np.int32)
        subject[mt.pad_token] = 0
    else:
        subject = _codec(o).repeat_subject(mt.vocab_size)
    return dict(repetition=Repetition(subject, o.presence_penalty, o.frequency_penalty, o.repeat_window, o.no_repeat_ngram,
                                      o.ngram_span))


def _note_args(o, mt):
    """the keyword arguments of generate_cached / generate_timed that --well-formed / --max-polyphony set"""
    from .sequence import EventSeq
    return dict(note_rules=EventSeq.note_rules(mt.vocab_size), max_polyphony=o.max_polyphony)


def _timed(o, mt, timed, prior, lens=None, **kw):
    """--seconds / --bars: the samples through generate_timed, each trimmed to its prompt and the events it kept"""
    if o.seconds is not None:
        from .sequence import EventSeq
        cost, unit = EventSeq.time_cost(mt.vocab_size), 'x 0.01 s'
    else:
        from .REMI import REMI_EventSeq
        cost, unit = REMI_EventSeq.bar_cost(mt.vocab_size), 'bars'
    tokens, lengths, info = mt.generate_timed(prior, timed['budget'], cost, o.max_len, inclusive=timed['inclusive'],
                                              temperature=o.temperature, top_k=o.top_k, top_p=o.top_p, prior_lengths=lens,
                                              kv_cache=o.kv_cache, window=o.window or None, hop=o.hop or None, **kw)
    tokens, lengths, done, spent = tokens.cpu().numpy(), lengths.tolist(), info['done'].tolist(), info['spent'].tolist()
    lens = lens or [prior.shape[1]] * len(lengths)
    print('Budget {} {}: {} steps for at most {} events'.format(timed['budget'], unit, info['steps_run'], o.max_len))
    for i, (n, ended) in enumerate(zip(lengths, done)):
        if not ended:
            print('Sample {}: reached -l {} events first ({} of {} {})'.format(i, o.max_len, spent[i], timed['budget'], unit))
    return [row[:p + n] for row, p, n in zip(tokens, lens, lengths)]


def _best_of(o, mt, res, prompt_lens, grammar=None):
    """--best-of N: rows b * N + k of ``res`` are the N candidates of sample b.  Scores every continuation (the events from the
    row's prompt length on) in one ``score`` call at temperature 1 and returns the best row of every group"""
    N = o.best_of
    if N == 1:
        return res
    x = torch.from_numpy(np.asarray(res)).to(torch.device('cuda:0'))
    lengths = [n + o.max_len for n in prompt_lens]
    out = mt.score(x, lengths=lengths, from_pos=prompt_lens, temperature=1.0, grammar=grammar)
    sums = out['sum'].view(-1, N).cpu()
    best = sums.argmax(1)
    print('Best of {}: log-probabilities {}'.format(N, [round(float(sums[i, k]), 3) for i, k in enumerate(best.tolist())]))
    return np.asarray(res)[[i * N + k for i, k in enumerate(best.tolist())]]


def _ragged_priors(o):
    """--condition-files: one MIDI-like prompt per file, right-padded into [B, Pmax]; returns (prior, lengths)"""
    if o.condition_file is not None or o.grammar or o.reference_mask:
        raise SystemExit('--condition-files cannot be combined with -c, --grammar or --reference-mask')
    if o.repr != 'midi_like':
        raise SystemExit('--condition-files continues MIDI-like (EventSeq) prompts: use --repr midi_like')
    from .sequence import EventSeq, NoteSeq
    files = [f for f in o.condition_files.split(',') if f]
    if not files:
        raise SystemExit('--condition-files: no file given')
    ids = []
    for f in files:
        a = EventSeq.from_note_seq(NoteSeq.from_midi_file(f)).to_array()[:500]
        if len(a) == 0:
            raise SystemExit(f'{f}: no notes in the MIDI-like pitch range')
        ids.append(a)
        print('Prompt: {} events from {}'.format(len(a), f))
    lens = [len(a) for a in ids]
    if not o.window and max(lens) + o.max_len > o.max_seq:
        raise SystemExit(f'--condition-files: the longest prompt ({max(lens)} events) + -l {o.max_len} exceeds -M {o.max_seq}')
    pad = vocab_of(o.repr) - 1
    prior = np.full((len(ids), max(lens)), pad, dtype=np.int64)
    for i, a in enumerate(ids):
        prior[i, :len(a)] = a
    return torch.from_numpy(prior), lens


def main(argv=None):
    o = get_options(argv)
    _check_best_of(o)
    _check_beam_options(o)
    _check_share_prompt(o)
    timed = _check_timed(o)
    well = _check_notes(o)
    repeat = _check_repeat(o)
    _check_lookahead(o, timed, well, repeat)
    classes = _check_class(o, well)
    entropy = _check_entropy(o, well)
    if o.hop and not o.window:
        raise SystemExit('--hop is the stride of --window: add --window W')
    if o.window and o.reference_mask:
        raise SystemExit('--reference-mask cannot be combined with --window (the KV-cache decode is causal)')
    if o.kv_cache != 'bf16' and not (o.grammar or o.condition_files is not None or o.window or o.beam_size or timed or well
                                     or repeat or classes or entropy):
        raise SystemExit(f'--kv-cache {o.kv_cache} applies to the KV-cache decode only: add --grammar or --condition-files '
                         '(or -B K; the default sampler recomputes the window and keeps no cache)')
    # with --window every branch below samples through the KV-cache decode and its re-anchored window
    cached = dict(kv_cache=o.kv_cache, window=o.window or None, hop=o.hop or None)
    look = {}                                             # --lookahead: what every step accepted, printed when the call is done
    if o.lookahead:
        cached.update(lookahead=o.lookahead, draft_ngram=o.draft_ngram, stats=look)
    ragged = _ragged_priors(o) if o.condition_files is not None else None     # checked before any model or device work
    net = utils.load_net(o.load_path, o.ema)
    device = torch.device('cuda:0')
    vocab = vocab_of(o.repr)
    mt = MusicTransformer(embedding_dim=o.d_model, vocab_size=vocab, num_layer=o.num_layers, max_seq=o.max_seq,
                          dropout=0)
    if net is not None:
        mt.load_state_dict(net)
    mt.to(device).eval()
    if o.data_path and os.path.isdir(o.data_path):
        ds = Data(o.data_path, o.max_seq)
        if len(ds.file_dict['test']) >= 2:
            ms = MetricsSet({'accuracy': CategoricalAccuracy(), 'loss': SmoothCrossEntropyLoss(config.label_smooth, vocab, vocab - 1),
                             'bucket': LogitsBucketting(vocab)})
            x, y = ds.slide_seq2seq_batch(2, o.max_seq, 'test')
            with torch.no_grad():
                pred, _ = mt(torch.from_numpy(x).to(device, dtype=torch.int))
                m = ms(pred, torch.from_numpy(y).to(device, dtype=torch.int))
            print('Test >>>> Loss: {:6.6}, Accuracy: {}'.format(m['loss'], m['accuracy']))
    mt.test()
    notes = _note_args(o, mt) if well else {}             # --well-formed: every sampling call below is the KV-cache decode
    if repeat:                                            # so it is with the repetition flags; their keyword travels with the notes'
        notes.update(_repeat_args(o, mt))
    if classes:                                           # and with the --class-* flags
        notes.update(_class_args(o, mt, classes))
    notes.update(entropy)                                 # and with --min-p / --typical-p / --mirostat

    def search(prior, **kw):                              # -B: the best beam of every sample
        res, scores = mt.generate_beam(prior, o.max_len, o.beam_size, temperature=o.temperature, stochastic=o.stochastic_beam_search,
                                       kv_cache=o.kv_cache, **kw)
        print('Beam search ({} beams): log-probabilities {}'.format(o.beam_size, [round(v, 3) for v in scores.tolist()]))
        return res.cpu().numpy()
    if ragged is not None:
        prior, lens = ragged
        if timed:
            _write(o, _timed(o, mt, timed, prior.to(device), lens, **notes))
            return
        if o.share_prompt:                                 # the N candidates of a file over one copy of its prompt
            res = mt.generate_cached(prior.to(device), o.max_len, temperature=o.temperature, top_k=o.top_k, top_p=o.top_p,
                                     prior_lengths=lens, samples_per_prompt=o.best_of, **notes).cpu().numpy()
            res = _best_of(o, mt, res, [n for n in lens for _ in range(o.best_of)])
            _write(o, [row[:n + o.max_len] for row, n in zip(res, lens)])
            return
        if o.best_of > 1:                                  # every prompt N times, side by side
            prior, lens = prior.repeat_interleave(o.best_of, 0), [n for n in lens for _ in range(o.best_of)]
        if o.beam_size:
            _write(o, [row[:n + o.max_len] for row, n in zip(search(prior.to(device), prior_lengths=lens), lens)])
            return
        res = mt.generate_cached(prior.to(device), o.max_len, temperature=o.temperature, top_k=o.top_k, top_p=o.top_p,
                                 prior_lengths=lens, **cached, **notes).cpu().numpy()
        res, lens = _best_of(o, mt, res, lens), lens[::o.best_of]
        res = [row[:n + o.max_len] for row, n in zip(res, lens)]             # without the pad tail
        _report_lookahead(look)
        _write(o, res)
        return
    rows = o.batch_size * o.best_of                        # --best-of N: N candidates per sample, side by side
    prior = torch.tensor([[24, 28, 31]] * rows, dtype=torch.long, device=device)
    if o.condition_file is not None:
        # generate.py:101-105: MIDI -> notes -> MIDI-like events -> the first 500 indices, repeated for the batch
        if o.repr != 'midi_like':
            raise SystemExit('--condition-file continues a MIDI-like (EventSeq) prompt: use --repr midi_like')
        from .sequence import EventSeq, NoteSeq
        ids = EventSeq.from_note_seq(NoteSeq.from_midi_file(o.condition_file)).to_array()[:500]
        if len(ids) == 0:
            raise SystemExit(f'{o.condition_file}: no notes in the MIDI-like pitch range')
        prior = torch.from_numpy(np.array([ids] * (1 if o.share_prompt else rows), dtype=np.int64)).to(device)
        print('Prompt: {} events from {}'.format(len(ids), o.condition_file))
    if o.grammar:
        if o.repr == 'remi':
            from .REMI import REMI_EventSeq as Codec
        elif o.repr == 'mumidi':
            from .MuMIDI import MuMIDI_EventSeq as Codec
        else:
            raise SystemExit('--grammar is defined for --repr remi and --repr mumidi')
        bar = Codec.feat_ranges()['bar'][0]
        prior = torch.full((1 if o.share_prompt else rows, 1), bar, dtype=torch.long, device=device)
        if o.share_prompt:                                 # the one-token prompt: nothing to share yet, every key is a row's own
            cached = dict(samples_per_prompt=rows)
        if o.beam_size:
            _write(o, search(prior, grammar=Codec.next_token_table()))
            return
        if timed:
            _write(o, _timed(o, mt, timed, prior, grammar=Codec.next_token_table(), **notes))
            return
        res = mt.generate_cached(prior, o.max_len, temperature=o.temperature, top_k=o.top_k, top_p=o.top_p,
                                 grammar=Codec.next_token_table(), **cached, **notes).cpu().numpy()
        res = _best_of(o, mt, res, [1] * rows, Codec.next_token_table())
    elif o.beam_size:
        res = search(prior)
    elif timed:
        _write(o, _timed(o, mt, timed, prior, **notes))
        return
    elif o.share_prompt:                                   # -c FILE: one prompt, -b x --best-of samples
        res = mt.generate_cached(prior, o.max_len, temperature=o.temperature, top_k=o.top_k, top_p=o.top_p,
                                 samples_per_prompt=rows, **notes).cpu().numpy()
    elif o.window or well or repeat or o.lookahead or classes or entropy:
        res = mt.generate_cached(prior, o.max_len, temperature=o.temperature, top_k=o.top_k, top_p=o.top_p, **cached,
                                 **notes).cpu().numpy()
    else:
        res = mt.generate(prior, o.max_len, temperature=o.temperature, top_k=o.top_k, top_p=o.top_p,
                          reference_mask=o.reference_mask).cpu().numpy()
    if not o.grammar:
        res = _best_of(o, mt, res, [prior.shape[1]] * rows)
    _report_lookahead(look)
    _write(o, res)


def _report_lookahead(look):
    if look:
        print('Lookahead: {} steps, {:.2f} events per step and sample'.format(look['steps_run'], sum(look['tokens']) / max(1, sum(look['steps']))))


def _write(o, res):
    os.makedirs(o.output_dir, exist_ok=True)
    for i, seq in enumerate(res):
        name = os.path.join(o.output_dir, f'gen-{i:03d}')
        if o.repr == 'midi_like':
            if o.release:                                 # the note_off of every note the sample still holds
                from .sequence import EventSeq
                seq = EventSeq.release(seq)
            n = utils.event_indeces_to_midi_file(seq, name + '.mid')
            print('===> {} ({} notes)'.format(name + '.mid', n))
        elif o.repr == 'remi':
            from .REMI import REMI_EventSeq
            ids = [int(v) for v in seq if int(v) < REMI_EventSeq.dim()]            # drop pad ids
            notes, _, _ = REMI_EventSeq.write_midi(REMI_EventSeq.to_event(ids), name + '.mid')
            print('===> {} ({} notes)'.format(name + '.mid', len(notes)))
        elif o.repr == 'mumidi':
            from .MuMIDI import MuMIDI_EventSeq
            ids = [int(v) for v in seq if int(v) < MuMIDI_EventSeq.dim()]          # drop pad ids
            notes, _, _ = MuMIDI_EventSeq.write_midi(MuMIDI_EventSeq.from_array(ids), name + '.mid')
            print('===> {} ({} notes)'.format(name + '.mid', sum(len(v) for v in notes.values())))
        else:
            np.save(name + '.npy', seq.astype(np.uint16))
            print('===> {} (event indices)'.format(name + '.npy'))


if __name__ == '__main__':
    main()
