"""generate_cached(note_rules=, max_polyphony=) (ABI 28) at the model level, on the tamed model (d 128, two layers, V 309: the
MIDI-like codec's ids and the pad id), four ragged prompts of 3 .. 9 tokens and at most 40 events.

Exact prefix.  The sampler draws by (seed, step, global row) and rows never interact, so a constrained row is the unconstrained
row of the same seed up to, but excluding, the first step at which that one breaks a rule; there it holds another id, a legal one; a row that never breaks a rule is identical
throughout.  The rule table is a sparse one chosen from the unconstrained run (_plan), so that one row breaks within three
steps, one strictly inside and one never.

The sampler draws by inverse CDF, so this holds because the step draws twice (include/mgx.h, mgx_notes_keep): once from the
logits before the note mask, with the call's seed, and once from the masked ones; a legal first draw is the row's token.

Validity and bite, distributions, the prompt's state, a time budget on top, and the shared prompt cache follow, with
EventSeq.note_rules and tests/notes_ref.py as the host-side fold."""
import numpy as np
import pytest
import torch

import notes_ref
from decode_fixtures import ragged_prior, tame_model
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
V = 309
PAD = V - 1
LENS = [3, 9, 5, 7]
N = 40
SEED = 11

_MODEL = []


def _model():
    """one model (max_seq 96) with its reference parameters for the whole file: no test changes it"""
    if not _MODEL:
        _MODEL.extend(tame_model(d=128, nl=2, L=96, V=V))
    return _MODEL[0]


def _prior(lens=LENS):
    return ragged_prior(lens, V, torch.Generator().manual_seed(5), fill=0)


def _codec_rules():
    from musicgeneration_amd.sequence import EventSeq
    return EventSeq.note_rules(V)


def _breaks(rule, prior, lens, toks, n, max_on=128):
    """per row: the 0-based step at which its continuation first breaks a rule, from its own prompt's state (None: never)"""
    return [notes_ref.first_break(rule, V, toks[b, P:P + n], notes_ref.fold(rule, V, prior[b, :P]), max_on) for b, P in enumerate(lens)]


def _plan(ref, prior, lens):
    """a sparse rule table for the unconstrained run ``ref``: three bits whose set and clear ids are drawn, with a fixed
    generator, from the ids the continuations hold, until one row first breaks a rule within its first three steps, one
    strictly inside and one never.  Asserts that such a table exists"""
    pool = np.unique(np.concatenate([ref[b, P:P + N] for b, P in enumerate(lens)]))
    pool = pool[pool != PAD]
    rng = np.random.default_rng(0)
    for _ in range(4000):
        ids = rng.choice(pool, 6, replace=False)
        rule = np.zeros(V, dtype=np.int32)
        rule[ids[:3]], rule[ids[3:]] = (1, 32, 128), (-1, -32, -128)          # bits 0, 31 and 127
        br = _breaks(rule, prior, lens, ref, N)
        if any(b is not None and b <= 2 for b in br) and any(b is not None and 3 <= b < N - 1 for b in br) and None in br:
            print(f"rule ids: set {ids[:3].tolist()} clear {ids[3:].tolist()}, first breaks at steps {br}")
            return rule, br
    raise AssertionError("no sparse table gives an early, an inside and a never-breaking row: pick another SEED")


def _check_prefix(mt, prior, lens, **kw):
    """the constrained run, captured and eager, against the unconstrained run of the same arguments"""
    x = prior.to(DEV)
    pl = dict(prior_lengths=lens) if lens is not None else {}
    lens = lens or [prior.shape[1]] * prior.shape[0]
    ref = mt.generate_cached(x, N, seed=SEED, **pl, **kw).cpu().numpy()
    rule, br = _plan(ref, prior.numpy(), lens)
    got = {g: mt.generate_cached(x, N, seed=SEED, note_rules=rule, use_graph=g, **pl, **kw).cpu() for g in (True, False)}
    assert torch.equal(got[True], got[False])                                 # the captured and the eager run are identical
    toks = got[True].numpy()
    assert toks.shape == ref.shape and toks.dtype == np.int32
    parts = [int(np.argmax(toks[b, P:P + N] != ref[b, P:P + N])) if (toks[b, P:P + N] != ref[b, P:P + N]).any() else None
             for b, P in enumerate(lens)]
    print(f"the constrained rows first differ from the unconstrained ones at steps {parts}")
    for b, P in enumerate(lens):
        held0 = notes_ref.fold(rule, V, prior[b, :P].numpy())
        if br[b] is None:
            assert (toks[b] == ref[b]).all(), b
            continue
        s = br[b]
        assert (toks[b, :P + s] == ref[b, :P + s]).all(), (b, s)              # equal up to, but excluding, the breaking step
        held = notes_ref.fold(rule, V, toks[b, P:P + s], held0)
        assert toks[b, P + s] != ref[b, P + s] and not notes_ref.banned_id(rule, toks[b, P + s], held, 128), (b, s)
        assert notes_ref.first_break(rule, V, toks[b, P:P + N], held0) is None, b      # and well-formed from there on
        assert (toks[b, P + N:] == PAD).all()


def test_rows_equal_the_unconstrained_rows_up_to_their_first_break():
    _check_prefix(_model(), _prior(), LENS)


def test_prefix_with_top_k_top_p_and_temperature():
    _check_prefix(_model(), _prior(), LENS, top_k=40, top_p=0.9, temperature=1.3)


def test_prefix_on_the_8_bit_cache():
    _check_prefix(_model(), _prior(), LENS, kv_cache="fp8")


def test_prefix_across_the_re_anchored_window():
    from musicgeneration_amd.decode import window_schedule
    assert len(window_schedule(LENS, N, 24, 8)[2]) >= 2                       # the run re-anchors; the state ignores positions
    _check_prefix(_model(), _prior(), LENS, window=24, hop=8)


def test_prefix_on_equal_prompts_and_the_shared_counter():
    """prompts of one length: the shared position counter, prefilled token by token -- those prompt steps stay unconstrained"""
    _check_prefix(_model(), _prior()[:, :3], None)
    _check_prefix(_model(), _prior()[:, :3], None, prefill="token")


def test_every_row_is_well_formed_under_the_cap_and_the_unconstrained_run_is_not():
    mt, prior, rule = _model(), _prior(), _codec_rules()
    ref = mt.generate_cached(prior.to(DEV), N, seed=SEED, prior_lengths=LENS).cpu().numpy()
    br = _breaks(rule, prior.numpy(), LENS, ref, N, max_on=3)
    print(f"the unconstrained rows first break a rule at steps {br}")
    assert all(b is not None for b in br), "an unconstrained row breaks no rule, the test would pass vacuously: pick another SEED"
    toks = mt.generate_cached(prior.to(DEV), N, seed=SEED, prior_lengths=LENS, note_rules=rule, max_polyphony=3).cpu().numpy()
    ons = 0
    for b, P in enumerate(LENS):
        held = notes_ref.fold(rule, V, prior[b, :P].numpy())
        for s, t in enumerate(toks[b, P:P + N]):
            assert 0 <= t < V and not notes_ref.banned_id(rule, t, held, 128), (b, s, int(t), sorted(held))     # well-formed,
            if rule[t] > 0:
                assert len(held) < 3, (b, s, sorted(held))                    # and no note is turned on while three are held
                ons += 1
            held = notes_ref.apply(rule, V, held, int(t))
        assert (toks[b, :P] == prior[b, :P].numpy()).all()
    assert ons > 0


def _masked_softmax(logits, ban):
    z = logits.clone().double()
    z[ban] = float("-inf")
    return torch.softmax(z, -1)


def test_distributions_are_zero_on_banned_ids_and_the_masked_softmax_elsewhere():
    from oracle import ref_cpu as R
    mt, prior, rule = _model(), _prior(), _codec_rules()
    p0, n = _MODEL[1], 12
    toks, probs = mt.generate_cached(prior.to(DEV), n, seed=SEED, prior_lengths=LENS, note_rules=rule, max_polyphony=3,
                                     return_probs=True)
    toks, probs = toks.cpu(), probs.cpu()
    assert probs.shape == (4, max(LENS) + n, V)
    for b, P in enumerate(LENS):
        seq = toks[b:b + 1, :P + n].long()
        with torch.no_grad():
            fwd = mt(seq.to(torch.int32).cuda())[0].float().cpu()[0]
            ora = R.model_forward(p0, seq, PAD)[0][0]
        held = notes_ref.fold(rule, V, prior[b, :P].numpy())
        assert not probs[b, :P - 1].any() and not probs[b, P + n - 1:].any(), b
        for s in range(n):                                                    # the distribution after column P - 1 + s
            ban = torch.from_numpy(notes_ref.banned(rule, V, held, 3))
            got = probs[b, P - 1 + s]
            assert ban.any() and not got[ban].any(), (b, s)                    # exactly 0 on what the host-folded state bans
            assert abs(got.sum().item() - 1) < 1e-3
            assert (got - _masked_softmax(fwd[P - 1 + s], ban)).abs().max().item() < 1e-2, (b, s)
            assert (got - _masked_softmax(ora[P - 1 + s], ban)).abs().max().item() < 2e-2, (b, s)
            assert got[toks[b, P + s]] > 0
            held = notes_ref.apply(rule, V, held, int(toks[b, P + s]))


def test_the_prompt_s_state_is_folded_ill_formed_or_not():
    """a prompt that leaves keys 10 and 20 held, with a double note_on (10) and an orphan note_off (30): step one may not turn
    10 or 20 on, may turn them off, and no other key off.  A second row with the cap already exceeded may turn nothing on"""
    mt, rule = _model(), _codec_rules()
    on, off = 0, 88
    rows = [[on + 10, on + 10, on + 20, off + 30, on + 40, off + 40, 250],
            [on + 1, on + 2, on + 3, on + 4, 250, off + 4, 251]]              # three held under a cap of 2 (four after five ids)
    prior = torch.tensor(rows)
    from musicgeneration_amd.sequence import EventSeq
    assert EventSeq.held_after(rows[0]).tolist() == [10, 20] and EventSeq.held_after(rows[1]).tolist() == [1, 2, 3]
    for kw in (dict(), dict(prior_lengths=[7, 5])):                           # the shared counter (token prefill); ragged (batched)
        toks, probs = mt.generate_cached(prior.to(DEV), 4, seed=SEED, note_rules=rule, max_polyphony=2, return_probs=True, **kw)
        P0, P1 = (7, 5) if kw else (7, 7)
        p = probs[0, P0 - 1].cpu().numpy()
        assert p[on + 10] == 0 and p[on + 20] == 0 and p[off + 10] > 0 and p[off + 20] > 0
        assert not p[off:off + 88][np.setdiff1d(np.arange(88), [10, 20])].any()
        assert not p[on:on + 88].any()                                        # two held: the cap of 2 is reached
        assert p[176:308].all()                                               # velocity and time_shift are never touched
        q = probs[1, P1 - 1].cpu().numpy()
        held1 = [1, 2, 3] if P1 == 7 else [1, 2, 3, 4]
        assert not q[on:on + 88].any() and (q[off:off + 88] > 0).nonzero()[0].tolist() == held1
        if not kw:                                                            # the teacher-forced prompt steps were not constrained
            assert probs[0, 0].cpu().numpy()[on + 10] > 0 and probs[0, 2].cpu().numpy()[off + 30] > 0


def test_with_a_time_budget_rows_land_and_stay_well_formed():
    from musicgeneration_amd.sequence import EventSeq
    mt, prior, rule, cost = _model(), _prior(), _codec_rules(), EventSeq.time_cost(V)
    budgets = [150, 250, 180, 220]
    toks, lengths, info = mt.generate_timed(prior.to(DEV), budgets, cost, N, seed=SEED, prior_lengths=LENS, note_rules=rule,
                                            max_polyphony=3, poll=8)
    eager = mt.generate_timed(prior.to(DEV), budgets, cost, N, seed=SEED, prior_lengths=LENS, note_rules=rule, max_polyphony=3,
                              poll=8, use_graph=False)
    assert torch.equal(eager[0], toks) and torch.equal(eager[1], lengths)
    toks, lengths, spent, done = (t.cpu().numpy() for t in (toks, lengths, info["spent"], info["done"]))
    print(f"lengths {lengths.tolist()}, spent {spent.tolist()} of {budgets}, done {done.tolist()}, steps {info['steps_run']}")
    for b, P in enumerate(LENS):
        n = int(lengths[b])
        kept = toks[b, P:P + n]
        assert int(cost[kept].sum()) == spent[b] <= budgets[b]                # no row overshoots
        assert spent[b] == budgets[b] if done[b] else n == N                  # a finished row has spent exactly its budget
        assert (toks[b, P + n:] == PAD).all()                                 # an ended row steps on pad_token: its state is frozen
        assert notes_ref.first_break(rule, V, kept, notes_ref.fold(rule, V, prior[b, :P].numpy()), 3) is None, b
    assert done.any()


def test_samples_per_prompt_start_from_their_prompt_s_state():
    mt, rule = _model(), _codec_rules()
    lens = [5, 9]
    prior = _prior(lens)
    kw = dict(seed=SEED, note_rules=rule, max_polyphony=3)
    shared = mt.generate_cached(prior.to(DEV), 24, prior_lengths=lens, samples_per_prompt=2, **kw).cpu()
    repeated = mt.generate_cached(prior.repeat_interleave(2, 0).to(DEV), 24, prior_lengths=[5, 5, 9, 9], **kw).cpu()
    for r in range(4):
        P = lens[r // 2]
        held0 = notes_ref.fold(rule, V, prior[r // 2, :P].numpy())
        assert notes_ref.first_break(rule, V, shared[r, P:P + 24].numpy(), held0, 3) is None, r
    assert not torch.equal(shared[0], shared[1])                              # two samples, not one twice
    assert torch.equal(shared, repeated)
