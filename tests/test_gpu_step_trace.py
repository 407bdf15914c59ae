"""A real training step of MusicTransformer on the GPU, recorded launch by launch (tests/step_trace.py: record) and checked stage by
stage against the fp64 reference of each stage on the inputs the GPU itself produced (check_step): the joining code of
ops._EncoderLayer, _EmbedPE, _Linear, _SmoothCE and MusicTransformer._hidden / _logits_padded / _params_for_padded_E -- the residual
gradient joined in a dX epilogue, the ReLU mask, the bias gradients emitted by the LayerNorm backward, the grouped dW launch, the two
streams, every padding of the vocabulary, the FFN width and the rows, the zero rows in front of E and their fold-back -- at the
bounds the kernels already have, element by element, with every element of the flat gradient buffer and every parameter accounted
for.  tests/test_gpu_model.py and tests/test_gpu_dropout_model.py compare whole tensors with the reference project's run; this
module compares nothing end to end.

Every case runs two micro-batches without zero_grad (the second call's slots start nonzero, and it draws its own dropout seed,
recorded by wrapping _next_seed) from the tamed initialiser of tests/dropout_fixtures.py (embedding and E x 0.25):
  base      V 60  d 128 nl 2 L 64  (max_seq 64)  B 3 p 0    trailing pads in one row: a fully padded key tile
  padded    V 337 d 192 nl 2 L 40  (max_seq 64)  B 3 p 0.1  Vp = 384, FFN 96 -> 128 (the column-padded view), Lp = 64: masks over Lp rows
  short-E   V 60  d 128 nl 2 L 40  (max_seq 40)  B 2 p 0    Lp > max_seq: zero rows in front of E and pe, the fold-back
  asm-dkv   V 60  d 256 nl 1 L 128 (max_seq 128) B 2 p 0.1  L % 128 == 0: the 64-key dK/dV loop; interior and trailing pads
  two-stream, det: the base case under ops.configure_streams (side_work 1, 2, 3) and in deterministic mode (one stream, side_work 3)
Each case asserts from the reference alone that its data reaches what it names (every case has a fully padded key tile in row 1).
In deterministic mode the dE stage is held this way: where the CPU twin of the mode's fixed-point
arithmetic (step_trace.dE_bound_covers_fixed_point) is itself beyond attn_bwd_bounds -- the first micro-batch, whose slot starts from
zero -- the GPU's figure is reported, not asserted (1.546 at an entry of 5e-8, error 3.4e-10, a third of the quantum 2^-30); the
bound is unchanged, the stage is asserted wherever the twin is within it, and the mode's gradients are held bit for bit to each other
across stream plans.  The controls re-run check_step on the same GPU
outputs with planted mistakes 1, 3, 5 and 6 (step_trace.MISTAKES) applied to the roles: each must fail at its stage.  No bound here
is new or tuned: profiles/r33_step_trace_tests.txt has the largest ratio per family and case beside the per-kernel modules' figures.
Every test prints its ratios before it asserts (pytest -s)."""
import pytest
import torch

import dropout_fixtures as DF
import kernel_checks as KC
import step_trace as ST
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)
from oracle import train_ref as T

pytestmark = pytest.mark.gpu

F64 = torch.float64
SEEN = {}
_report = KC.report_fixture(SEEN, "largest ratio {:.3f}")   # GEMM, ATTN: error / bound; LNF, LNB, CE, EMB, ADAM: floors F, against their C
CASES = {"base": dict(V=60, d=128, nl=2, L=64, max_seq=64, B=3, p=0.0, pads={1: ((), 30)}),
         "padded": dict(V=337, d=192, nl=2, L=40, max_seq=64, B=3, p=0.1, pads={1: ((), 31)}),
         "short-E": dict(V=60, d=128, nl=2, L=40, max_seq=40, B=2, p=0.0, pads={1: ((), 31)}),
         "asm-dkv": dict(V=60, d=256, nl=1, L=128, max_seq=128, B=2, p=0.1, pads={0: ((17, 70), None), 1: ((), 90)})}
SIDE_CUS = 64
_memo = {}


def _run(name, monkeypatch, two_stream=0, det=False):
    """two micro-batches of case `name`, recorded -> (the Steps, the model): run once per (case, streams, mode)"""
    key = (name, two_stream, det)
    if key in _memo:
        return _memo[key]
    from musicgeneration_amd import ops
    from musicgeneration_amd.criterion import SmoothCrossEntropyLoss
    from musicgeneration_amd.network import MusicTransformer
    c = CASES[name]
    V, d, nl, L, max_seq, B, p = (c[k] for k in ("V", "d", "nl", "L", "max_seq", "B", "p"))
    p0, _ = DF._params_from_oracle_init((V, d, nl, max_seq, B), seed=3, scale=0.25)
    torch.manual_seed(DF.MODEL_SEED)
    mt = MusicTransformer(embedding_dim=d, vocab_size=V, num_layer=nl, max_seq=max_seq, dropout=p)
    mt.load_state_dict({k: v.clone() for k, v in p0.items()})
    mt = mt.cuda().train()
    seeds, draw = [], mt._next_seed
    mt._next_seed = lambda: seeds.append(draw()) or seeds[-1]
    lossf = SmoothCrossEntropyLoss(ST.EPS_LS, V, V - 1)
    st = mt.store()
    lay = ST.Layout(mt)
    assert lay.numel == st.numel and lay.reserved == st.reserved and lay.offsets == {n: o for n, (o, _) in st.offsets.items()}
    steps = []
    if det:
        ops.set_deterministic(True)
    try:
        plan = ops.configure_streams(SIDE_CUS, 0, side_work=two_stream) if two_stream else None
        try:
            with torch.cuda.stream(ops.main_stream()):
                for x, y in ST.batches(V, B, L, c["pads"], seed=5):
                    torch.cuda.synchronize()
                    g0 = st.grad.detach().cpu().clone()
                    with ST.record(monkeypatch, st.grad) as trace:
                        loss = lossf(mt(x.to(torch.int32).cuda()), y.to(torch.int32).cuda())
                        loss.backward()
                        ops.join_side_stream()
                        torch.cuda.synchronize()
                    s = ST.new_step(mt, (st.param.detach().cpu().clone(), st.shadow.detach().cpu().clone()), V, d, nl, L, max_seq, B, p, x, y,
                                    seeds[-1], g0, two_stream, det)
                    s.trace, s.g1 = trace.finish(), st.grad.detach().cpu().clone()
                    steps.append(s)
        finally:
            if plan is not None:
                ops.configure_streams(0, 0)
    finally:
        if det:
            torch.cuda.synchronize()
            ops.set_deterministic(False)
    assert len(seeds) == 2 and seeds[0] != seeds[1]
    _memo[key] = (steps, mt)
    return _memo[key]


def _reaches(name, s, r):
    """from the reference alone, on the recorded inputs: the data exercises what the case names"""
    D = ST.dims(s)
    tokp = r.tokp.long()
    pm = tokp == D.pad_token
    for l in range(s.nl):
        w = ST.weights(s, l)
        pre, _ = T.linear_fwd(r.o1[l].reshape(-1, s.d), w.wpre[:D.H], w.bpre[:D.H], 0)
        real = pre[~pm.reshape(-1)]
        assert (real > 0).any() and (real < 0).any() and (real > 0).any(1).float().mean() > 0.9, f"{name}: FFN pre-activations of one sign in layer {l}"
    assert pm.reshape(s.B, D.Lp // 32, 32).all(-1).any(), f"{name}: no fully padded key tile"          # (every case)
    if name == "asm-dkv":
        assert D.Lp % 128 == 0 and any((pm[b] & ~pm[b].roll(-1))[:-1].any() for b in range(s.B)), f"{name}: no interior pad"
    if name in ("padded", "short-E"):
        assert D.Lp > s.L
    if name == "padded":
        assert D.Vp == 384 and D.Hp == 128 and D.H == 96
    if s.p > 0:
        sites = [s.seed] + [x for l in range(s.nl) for x in ST.seeds_of(s, l)]
        assert len(set(sites)) == len(sites)
        for seed in sites:
            m = ST.mult_of(s, seed).reshape(s.B, D.Lp, s.d)
            for rows in (m[:, :s.L], m[:, s.L:]) if D.Lp > s.L else (m,):
                assert (rows == 0).any() and (rows > 1).any(), f"{name}: dropout site {seed - s.seed} drops or keeps nothing"
    if name == "short-E":
        assert D.extra == 24
        fa = T.rel_attn_fwd(r.qkv[0], ST.weights(s, 0).E, pm, D.heads, D.Lp)
        i, j = torch.arange(D.Lp)[:, None], torch.arange(D.Lp)[None, :]
        far = (i - j >= 32) & (i < s.L)
        assert (fa.P[:, :, far] > 2.0 ** -20).any(), f"{name}: no real query attends over a distance >= 32"


def _check(name, monkeypatch, two_stream=0, det=False):
    steps, _ = _run(name, monkeypatch, two_stream, det)
    tag = name + (f" side_work={two_stream}" if two_stream else "") + (" det" if det else "")
    for call, s in enumerate(steps):
        seen = {}
        try:
            r = ST.check_step(s, seen, f"{tag} call {call}")
        finally:
            for fam, (ratio, case) in seen.items():
                if ratio > SEEN.get((fam, tag), (-1.0, None))[0]:
                    SEEN[(fam, tag)] = (ratio, case)
        _reaches(name, s, r)
        assert (s.g0 != 0).any() == (call > 0) and (s.g1 != s.g0).any()
    return steps


@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_of_a_traced_step_is_within_its_kernels_bound(name, monkeypatch):
    _check(name, monkeypatch)


@pytest.mark.parametrize("side_work", (1, 2, 3))
def test_every_stage_of_a_two_stream_step(side_work, monkeypatch):
    _check("base", monkeypatch, two_stream=side_work)


@pytest.mark.parametrize("side_work", (0, 3))
def test_every_stage_in_deterministic_mode(side_work, monkeypatch):
    _check("base", monkeypatch, two_stream=side_work, det=True)


def test_deterministic_mode_gives_the_same_gradient_bits_on_one_stream_and_two(monkeypatch):
    """the mode's promise, on the recorded buffers: dE and the weight gradients issued on the side stream end bit for bit where the
    one-stream step's do -- the hold on dE in this mode, whose distance from fp64 is reported and not asserted (step_trace.py)"""
    one, two = _run("base", monkeypatch, 0, True)[0], _run("base", monkeypatch, 3, True)[0]
    for call, (a, b) in enumerate(zip(one, two)):
        assert KC.bits(a.g0).equal(KC.bits(b.g0)) and KC.bits(a.g1).equal(KC.bits(b.g1)), f"call {call}"


@pytest.mark.parametrize("name,mistake", [(n, m) for n in CASES for m in (1, 3, 5, 6)
                                          if (m not in (5, 6) or CASES[n]["p"] > 0) and (m != 6 or CASES[n]["L"] % 32)])
def test_planted_mistakes_fail_at_their_stage_on_the_gpus_own_outputs(name, mistake, monkeypatch):
    """no extra launches: the recorded step with one role replaced by what the mis-joined launch would have written"""
    steps, _ = _run(name, monkeypatch)
    s = steps[1]
    with pytest.raises(AssertionError) as e:
        ST.check_step(ST.plant(s, mistake), {}, f"{name} planted {mistake}")
    assert ST.FAILS_AT[mistake] in str(e.value), (ST.MISTAKES[mistake], str(e.value)[:300])


def test_an_optimizer_step_leaves_the_padding_zero_and_follows_adam(monkeypatch):
    """one FusedAdam.step() after the padded case: param, m, v and shadow stay exactly zero in every padded tail and gap, and the
    parameters follow T.adam_step on the recorded gradient buffer within C_ADAM floors"""
    from musicgeneration_amd.optim import FusedAdam
    steps, mt = _run("padded", monkeypatch)
    s, st, lay = steps[-1], mt.store(), steps[-1].layout
    lr, b1, b2, eps = 1e-3, 0.9, 0.98, 1e-9
    opt = FusedAdam(mt, lr=lr, betas=(b1, b2), eps=eps)
    p0, g = st.param.detach().cpu().clone(), st.grad.detach().cpu().clone()
    assert KC.bits(g).equal(KC.bits(s.g1))
    opt.step()
    torch.cuda.synchronize()
    got = {"param": st.param.detach().cpu(), "m": opt.m.cpu(), "v": opt.v.cpu(), "shadow": st.shadow.detach().cpu()}
    own = torch.zeros(lay.numel, dtype=torch.bool)
    for n in lay.names:
        lay.view(own, n).fill_(True)
    assert 0 < (~own).sum() and (~own)[lay.offsets["fc.weight"] + 337 * 192:lay.offsets["fc.weight"] + 384 * 192].all()
    for what, buf in got.items():
        KC.check_equal("ADAM", buf[~own], 0.0, f"padded: {what} in the padded tails and the gaps")
    zeros = torch.zeros(lay.numel)
    ref = T.adam_step(p0, g, zeros, zeros, lr, b1, b2, eps, 1, 1.0)
    F = T.adam_floor(p0, g, zeros, zeros, lr, b1, b2, eps, 1, 1.0, ref)
    for what, rf, f in zip(("param", "m", "v"), ref, F):
        seen = {}
        try:
            KC.check_floor("ADAM", got[what][own], rf[own], f[own], f"padded {what} after one step", C=KC.C_ADAM, seen=seen)
        finally:
            if seen["ADAM"][0] > SEEN.get(("ADAM", "padded"), (-1.0, None))[0]:
                SEEN[("ADAM", "padded")] = seen["ADAM"]
    assert KC.bits16(got["shadow"]).equal(KC.bits16(got["param"].to(torch.bfloat16))), "shadow is not the bf16 rounding of param"
    assert (got["param"] != p0)[own].any()
