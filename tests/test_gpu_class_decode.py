"""generate_cached / generate_timed (class_sampling=) (ABI 33) at the model level: the tamed model (d 128, two layers, V 337), four
ragged prompts of 3 .. 9 tokens, 24 events, MIDI-like-shaped classes over the 337 ids.  tests/class_ref.py is the host-side
restatement; the plain call of the same seed is computed once and shared.

Bounds.  A filed distribution is softmax of the bf16 logits the kernel wrote, each within half a bf16 spacing + 3e-4 of ln p'
(tests/test_gpu_class_kernels.py); class_ref.prob_bound turns that into a bound per probability.  On the first step the plain
call's logits are bitwise the class call's, so its filed distribution p is exact input: the comparison allows prob_bound + 2e-6
(two f32 softmaxes).  Over a whole sample the comparison is with the TRAINING forward on the row's own tokens, which differs from
the decode chain by bf16 rounding (check_rows allows 1e-2 for the unwarped comparison) and which the class temperatures amplify
by up to the largest ratio, 2: see test_whole_sample_against_the_forward for the measured figure."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import class_ref
from decode_fixtures import check_rows, prompt_file, ragged_prior, tame_model
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, N, LENS, SEED, TEMP = 337, 24, [3, 9, 5, 7], 11, 1.1
PAD = V - 1
KW = dict(seed=SEED, prior_lengths=LENS, temperature=TEMP, return_probs=True)
CLS = np.zeros(V, dtype=np.int32)                                             # note_on, note_off, velocity, time_shift, other
CLS[88:176], CLS[176:208], CLS[208:336], CLS[336] = 1, 2, 3, 4
RATIOS = [2.0, 0.5, 1.5, 0.75, 1.0]                                           # temperature * inv_temp[c]
TEMPS = [TEMP / r for r in RATIOS]
SOFTMAX_F32 = 2e-6


def _cs(temperature=None, top_k=None, top_p=None, classes=CLS):
    from musicgeneration_amd.decode import ClassSampling
    return ClassSampling(classes, temperature, top_k, top_p)


def _arrays(cs, temperature=TEMP):
    """(inv_temp, top_k, top_p) as the checked copy stages them"""
    from musicgeneration_amd import decode
    own = decode.check_class_args(_HOST, cs, temperature)
    return ([1.0 / (temperature if t is None else t) for t in own.temperature], own.top_k, own.top_p)


class _Host:
    vocab_size, pad_token = V, PAD


_HOST = _Host()


@pytest.fixture(scope="module")
def model():
    return tame_model()


@pytest.fixture(scope="module")
def prompts():
    return ragged_prior(LENS, V, torch.Generator().manual_seed(5), fill=0)


@pytest.fixture(scope="module")
def plain(model, prompts):
    """the call without the keyword: (tokens, distributions) on the CPU, left unchanged"""
    toks, probs = model[0].generate_cached(prompts.cuda(), N, **KW)
    torch.cuda.synchronize()
    return toks.cpu(), probs.cpu()


def test_an_all_plain_object_is_the_call_without_the_keyword(model, prompts, plain):
    mt = model[0]
    for cs in (_cs(), _cs(temperature=[TEMP] * 5, top_k=[0] * 5, top_p={2: 1.0})):
        for g in (True, False):
            t, p = mt.generate_cached(prompts.cuda(), N, class_sampling=cs, use_graph=g, **KW)
            assert torch.equal(t.cpu(), plain[0]) and torch.equal(p.cpu(), plain[1]), g


def _first_step(model, prompts, plain, cs, name):
    """the class call's first filed distribution of every row against expected_probs of the plain call's"""
    t, p = model[0].generate_cached(prompts.cuda(), N, class_sampling=cs, **KW)
    p = p.cpu().double().numpy()
    inv_temp, top_k, top_p = _arrays(cs)
    worst, margins = 0.0, []
    for b, P in enumerate(LENS):
        src = plain[1][b, P - 1].double().numpy()
        want, lnp = class_ref.expected_probs(src, CLS, inv_temp, top_k, top_p, TEMP, with_lnp=True)
        margins += class_ref.warp_row(TEMP * np.log(np.maximum(src, 1e-300)), CLS, inv_temp, top_k, top_p, TEMP)[1]
        assert ((p[b, P - 1] > 0) == (want > 0)).all(), (name, b)
        bound = class_ref.prob_bound(lnp) + SOFTMAX_F32
        ratio = (np.abs(p[b, P - 1] - want) / bound).max()
        worst = max(worst, ratio)
        assert ratio <= 1, (name, b, ratio)
        assert abs(p[b, P - 1].sum() - 1) < 1e-5
    print(f"\nMEASURED first step [{name}]: largest error / bound {worst:.3f}; smallest filter margin "
          f"{min(margins) if margins else float('inf'):.3g}")
    return t.cpu(), p


def test_unit_ratios_launch_the_kernel_and_agree_with_the_plain_call(model, prompts, plain):
    """every inv_temp = 1 / temperature and a top-k that can cut nothing: not inert, so the kernel runs; what is filed is the plain
    distribution up to the quantisation of ln p -- a relative error of at most |ln p| 2^-8 (+ 3e-4), prob_bound with one half
    spacing around the plain distribution itself"""
    from musicgeneration_amd import decode
    cs = _cs(top_k={0: 1024})
    assert decode.check_class_args(model[0], cs, TEMP) is not None
    t, p = model[0].generate_cached(prompts.cuda(), N, class_sampling=cs, **KW)
    p, worst, differs = p.cpu().double().numpy(), 0.0, False
    for b, P in enumerate(LENS):
        src = plain[1][b, P - 1].double().numpy()
        with np.errstate(divide="ignore"):
            bound = class_ref.prob_bound(np.log(src), halves=1, centre=src) + SOFTMAX_F32
        ratio = (np.abs(p[b, P - 1] - src) / bound).max()
        worst = max(worst, ratio)
        assert ratio <= 1, (b, ratio)
        differs |= bool((p[b, P - 1] != src).any())
    print(f"\nMEASURED unit ratios: largest error / bound {worst:.3f}")
    assert differs                                                            # quantised: the launch was made


def test_first_step_temperatures_only(model, prompts, plain):
    _first_step(model, prompts, plain, _cs(temperature=TEMPS), "temperatures")


def test_first_step_temperatures_and_filters(model, prompts, plain):
    t, p = _first_step(model, prompts, plain, _cs(temperature=TEMPS, top_k={2: 4, 0: 20}, top_p={3: 0.8, 0: 0.9}), "filters")
    for b, P in enumerate(LENS):
        assert 1 <= (p[b, P - 1][CLS == 2] > 0).sum() < 32 and (p[b, P - 1][CLS == 3] > 0).sum() < 128
        assert (p[b, P - 1][CLS == 1] > 0).all()                              # an unfiltered class keeps every id


WHOLE_SAMPLE_RECORDED = 1.22e-3                                               # see the docstring below


def test_whole_sample_against_the_forward(model, prompts):
    """temperatures only, ratios in [0.5, 2]: per row, every filed distribution against expected_probs of the training forward's
    softmax on the row's own tokens.  The bound is measured: the largest |difference| of the first GPU run, 1.22e-3, is recorded
    in WHOLE_SAMPLE_RECORDED and the test allows twice that.  (check_rows allows 1e-2 for the unwarped comparison; a figure above
    2e-2 * the largest ratio, 4e-2, would need an explanation, not a looser bound: the measured one is 30 times below it.)"""
    mt = model[0]
    cs = _cs(temperature=TEMPS)
    inv_temp, top_k, top_p = _arrays(cs)
    toks, probs = mt.generate_cached(prompts.cuda(), N, class_sampling=cs, **KW)
    check_rows(mt, None, prompts, LENS, 1, N, toks, probs, V, oracle=False, forward=False)      # shapes, prompt, padding
    toks, probs = toks.cpu(), probs.cpu().double().numpy()
    worst = 0.0
    for b, P in enumerate(LENS):
        seq = toks[b:b + 1, :P + N]
        with torch.no_grad():
            fwd = torch.softmax(mt(seq.to(torch.int32).cuda())[0].double().cpu()[0] / TEMP, -1).numpy()
        for c in range(P - 1, P + N - 1):
            want = class_ref.expected_probs(fwd[c], CLS, inv_temp, top_k, top_p, TEMP)
            worst = max(worst, np.abs(probs[b, c] - want).max())
            assert probs[b, c, toks[b, c + 1]] > 0
    print(f"\nMEASURED whole sample: largest |filed - expected| {worst:.3g} (recorded {WHOLE_SAMPLE_RECORDED})")
    assert worst <= 2e-2 * max(RATIOS)
    assert WHOLE_SAMPLE_RECORDED is not None and worst <= 2 * WHOLE_SAMPLE_RECORDED


def _cut_to(probs_row, k):
    """what top-k k leaves of a class in a filed distribution: at least one id, at most k -- or more only where the surplus is an
    exact tie with the k-th (the sampler's tie rule: tied ids get bitwise equal ln p', hence bitwise equal filed probabilities).
    -> the number of nonzero ids"""
    nz = np.sort(probs_row[probs_row > 0])[::-1]
    assert len(nz) >= 1
    assert len(nz) <= k or nz[k - 1] == nz[-1], nz
    return len(nz)


def test_top_k_1_on_one_class_leaves_it_one_id_at_every_step(model, prompts):
    """at every step the filed distribution has one nonzero id in the class.  The tamed model's bf16 logits do tie exactly at a
    class's top now and then (first GPU run: row 1, step 19, two velocity ids), and the contract keeps ties together: such a
    step has several ids of bitwise equal probability, which _cut_to accepts and nothing else.  They must stay the exception"""
    toks, probs = model[0].generate_cached(prompts.cuda(), N, class_sampling=_cs(top_k={2: 1}), **KW)
    probs = probs.cpu().numpy()
    single = steps = 0
    for b, P in enumerate(LENS):
        for c in range(P - 1, P + N - 1):
            single += _cut_to(probs[b, c][CLS == 2], 1) == 1
            steps += 1
            assert (probs[b, c][CLS != 2] > 0).all()
    print(f"\nsteps with exactly one id in the class: {single} of {steps}")
    assert single >= 0.9 * steps


def test_graph_replay_is_the_eager_run_and_the_seed_decides(model, prompts, plain):
    mt, x = model[0], prompts.cuda()
    cs = _cs(temperature=TEMPS, top_k={2: 4}, top_p={3: 0.8})
    ref_t, ref_p = mt.generate_cached(x, N, class_sampling=cs, use_graph=False, **KW)
    for g in (True, False):
        t, p = mt.generate_cached(x, N, class_sampling=cs, use_graph=g, **KW)
        assert torch.equal(t, ref_t) and torch.equal(p, ref_p), g
    assert not torch.equal(ref_t.cpu(), plain[0])                             # the keyword changes the sample
    other, _ = mt.generate_cached(x, N, class_sampling=cs, **dict(KW, seed=SEED + 1))
    assert not torch.equal(other, ref_t)


def test_under_a_grammar_every_token_is_allowed(model):
    from musicgeneration_amd.REMI import REMI_EventSeq
    assert REMI_EventSeq.dim() + 1 == V
    mt, table = model[0], REMI_EventSeq.next_token_table()
    names, classes = REMI_EventSeq.event_classes(V)
    cs = _cs({names.index("position"): 0.7, names.index("note_on"): 1.4}, {names.index("note_velocity"): 2},
             {names.index("chord"): 0.9}, classes=classes)
    prior = torch.full((4, 1), REMI_EventSeq.feat_ranges()["bar"][0], dtype=torch.long).cuda()
    toks, probs = mt.generate_cached(prior, N, seed=SEED, grammar=table, class_sampling=cs, return_probs=True)
    plain_t = mt.generate_cached(prior, N, seed=SEED, grammar=table)
    assert not torch.equal(toks, plain_t)
    toks, probs = toks.cpu().numpy(), probs.cpu().numpy()
    vel = classes == names.index("note_velocity")
    for b in range(4):
        for j in range(N):
            t, v = int(toks[b, j]), int(toks[b, j + 1])
            assert (int(table[t, v >> 5]) >> (v & 31)) & 1, (b, j, t, v)
            allowed = class_ref.allowed_bits(table, t, V)
            assert not probs[b, j][~allowed].any(), (b, j)
            assert not (probs[b, j][vel] > 0).any() or _cut_to(probs[b, j][vel], 2) < vel.sum(), (b, j)


def test_with_a_time_budget_rows_end_exactly_on_their_budgets(model, prompts):
    mt = model[0]
    cost = np.zeros(V, dtype=np.int32)
    cost[208:336] = np.arange(1, 129)                                         # the time_shift class prices the clock
    budgets = [150, 250, 180, 220]
    kw = dict(seed=SEED, prior_lengths=LENS, poll=8, temperature=TEMP, class_sampling=_cs(temperature=TEMPS, top_k={3: 40}))
    toks, lengths, info = mt.generate_timed(prompts.cuda(), budgets, cost, N, **kw)
    eager = mt.generate_timed(prompts.cuda(), budgets, cost, N, use_graph=False, **kw)
    assert torch.equal(eager[0], toks) and torch.equal(eager[1], lengths)
    toks, lengths, spent, done = (t.cpu().numpy() for t in (toks, lengths, info["spent"], info["done"]))
    print(f"\nlengths {lengths.tolist()}, spent {spent.tolist()} of {budgets}, done {done.tolist()}")
    for b, P in enumerate(LENS):
        n = int(lengths[b])
        assert int(cost[toks[b, P:P + n]].sum()) == spent[b] <= budgets[b]    # no row overshoots
        assert spent[b] == budgets[b] if done[b] else n == N                  # a finished row has spent exactly its budget
        assert (toks[b, P + n:] == PAD).all()
    assert done.any()


@pytest.mark.parametrize("name,kw,per", [
    ("repetition", "rep", 1), ("fp8", dict(kv_cache="fp8"), 1), ("window", dict(window=24, hop=8), 1),
    ("two samples per prompt", dict(samples_per_prompt=2), 2)])
def test_composition_keeps_the_shape_and_padding_and_captured_is_eager(model, prompts, name, kw, per):
    from musicgeneration_amd.decode import Repetition
    mt = model[0]
    if kw == "rep":
        subject = np.ones(V, dtype=np.int32)
        subject[PAD] = 0
        kw = dict(repetition=Repetition(subject, presence=0.5, frequency=0.25, window=8, ngram=2))
    cs = _cs(temperature=TEMPS, top_k={2: 4}, top_p={3: 0.8})
    got = {g: mt.generate_cached(prompts.cuda(), N, class_sampling=cs, use_graph=g, **KW, **kw) for g in (True, False)}
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1]), name
    toks, probs = got[True]
    check_rows(mt, None, prompts, LENS, per, N, toks, probs, V, oracle=False, forward=False)
    probs = probs.cpu().numpy()
    for r in range(len(LENS) * per):
        P = LENS[r // per]
        for c in range(P - 1, P + N - 1):
            assert _cut_to(probs[r, c][CLS == 2], 4) < 32 and abs(probs[r, c].sum() - 1) < 1e-4, (name, r, c)
    without = mt.generate_cached(prompts.cuda(), N, **KW, **kw)[0]
    assert not torch.equal(without, toks), name


def test_lookahead_on_the_one_token_calls_own_sample(model, prompts):
    """the guide is the one-token class call's own sample.  First distributions agree to 1e-2; at least one row is identical
    throughout; the share is printed, not asserted: a last-bit difference between the two chains may flip a draw"""
    mt, x = model[0], prompts.cuda()
    cs = _cs(temperature=TEMPS, top_k={2: 4}, top_p={3: 0.8})
    one_t, one_p = mt.generate_cached(x, N, class_sampling=cs, **KW)
    st = {}
    toks, probs = mt.generate_cached(x, N, class_sampling=cs, lookahead=4, draft=one_t, stats=st, **KW)
    check_rows(mt, None, prompts, LENS, 1, N, toks, probs, V, oracle=False, forward=False)
    for r, P in enumerate(LENS):
        assert (probs[r, P - 1] - one_p[r, P - 1]).abs().max().item() < 1e-2, r
    same = (toks == one_t).all(1).cpu().tolist()
    print(f"\nrows identical to the one-token class call's throughout: {sum(same)} of {len(same)}; steps {st['steps']}, "
          f"tokens per step {sum(st['tokens']) / sum(st['steps']):.2f}")
    assert any(same), "no row identical to the one-token call's: choose another seed"
    eager, _ = mt.generate_cached(x, N, class_sampling=cs, lookahead=4, draft=one_t, use_graph=False, **KW)
    assert torch.equal(eager, toks)


def test_generate_py_writes_its_files(tmp_path):
    mt, _ = tame_model(d=128, nl=2, L=256, V=309)
    ckpt = str(tmp_path / "tame.pt")
    torch.save({"net": {k: v.cpu() for k, v in mt.state_dict().items()}}, ckpt)
    prompt = str(tmp_path / "prompt.mid")
    prompt_file(prompt, 5, 60)
    out = str(tmp_path / "g") + "/"
    cmd = [sys.executable, "-m", "musicgeneration_amd.generate", "-s", ckpt, "-o", out, "-b", "2", "-l", "60", "--num-layers", "2",
           "--d-model", "128", "-M", "256", "-c", prompt, "-d", str(tmp_path / "none"), "--class-temperature",
           "time_shift=0.8,note_on=1.2", "--class-top-k", "velocity=4", "--class-top-p", "note_off=0.9"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert len(glob.glob(out + "gen-*.mid")) == 2 and r.stdout.count("===> ") == 2
