"""mgx_adam_step_groups (include/mgx.h, K11c) against its contract: bit identity with mgx_adam_step / mgx_adam_step_clipped for one
group (1, 0) without an EMA, the fp64 reference of tests/adamw_ref.py with groups, decay, frozen chunks, shadow and EMA, frozen and
skipped chunks bit for bit, guard bands around every buffer, and the return codes.

Sizes: a tail only (1), one vector plus tail (5), two chunks with a tail (67), 3 chunks plus a tail in a fourth (3 * 64 + 7), and
two sizes beyond the 2048 x 256 x 4 elements of one grid pass (2^21 + 67, 2^21 + 64 + 3): the second grid-stride pass and the tail.

Bounds
  p, m, v   C_ADAM = 16 noise floors (kernel_checks.C_ADAM, the constant the parent's Adam is held to) of adamw_ref's floors: those
            of oracle.train_ref.adam_floor at the rate lr s, p's extended by one ulp of p where the group decays.
  shadow    exactly the bf16 rounding of the p the kernel stored.
  ema       C_EMA = 4 of adamw_ref's floor (the roundings of the two products and of the sum, plus (1 - d) times p's floor):
            measured 0.621 on the MI355X over the cases of this module (the largest ratio, at n = 2^21 + 67, step 1, decay
            0.1); 4 x that is 2.5, the next power of two 4.
  frozen / skipped / one group (1, 0)   bit equality."""
import functools
import math

import pytest
import torch

import adamw_ref
import kernel_checks as KC
from kernel_checks import bits, nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
GUARD = 8                                           # elements on each side of every buffer
GS = 0.37                                           # a gradient scale that is no power of two
HYPER = (1e-3, 0.9, 0.98, 1e-9)
BIG = 2 ** 21                                       # elements of one grid pass: 2048 blocks x 256 threads x 4
C_EMA = 4.0
SEEN = {}
_report = KC.report_fixture(SEEN, "largest ratio {:.3f}")


def guarded(data, dtype=None):
    """n elements on the device between GUARD sentinel elements (a multiple of 16 bytes: .t keeps the alignment the kernel asks for)"""
    data = torch.as_tensor(data).to(dtype or torch.as_tensor(data).dtype)
    return KC.Banded(data, GUARD * data.element_size(), -12345.0 if data.dtype.is_floating_point else 0xA5)


def chunks_of(n):
    return (n + 63) // 64


@functools.lru_cache(maxsize=None)
def gradient(n, seed=0):
    """fp32 Gaussian gradients [n], shared by the tests and never modified"""
    return torch.randn(n, generator=torch.Generator().manual_seed(7919 * seed + n % 997))


class State:
    """p, m, v, shadow, ema of one optimiser, each inside guard elements"""

    def __init__(self, n, seed, shadow=True, ema=True):
        gen = torch.Generator().manual_seed(seed)
        self.p = guarded(torch.randn(n, generator=gen))
        self.m = guarded(0.1 * torch.randn(n, generator=gen))
        self.v = guarded(torch.rand(n, generator=gen))
        self.shadow = guarded(self.p.t.cpu().to(BF)) if shadow else None
        self.ema = guarded(self.p.t.cpu() + 0.01 * torch.randn(n, generator=gen)) if ema else None

    def buffers(self):
        return [(k, b) for k, b in (("p", self.p), ("m", self.m), ("v", self.v), ("shadow", self.shadow), ("ema", self.ema)) if b]

    def snapshot(self):
        return {k: bits(b.buf).clone() for k, b in self.buffers()}

    def bands_intact(self):
        return all(b.bands_intact() for _, b in self.buffers())

    def args(self, g):
        return (self.p.t, g, self.m.t, self.v.t, self.shadow.t if self.shadow else None, self.ema.t if self.ema else None)


class Groups:
    """the chunk table and the two per-group tables on the device, inside guard bytes / elements"""

    def __init__(self, table, pairs):
        self.table, self.pairs = list(table), list(pairs)
        self.group_of = guarded(torch.tensor(self.table, dtype=torch.uint8))
        self.lr_scale = guarded(torch.tensor([s for s, _ in pairs], dtype=torch.float32))
        self.weight_decay = guarded(torch.tensor([w for _, w in pairs], dtype=torch.float32))

    def args(self):
        return (self.group_of.t, self.lr_scale.t, self.weight_decay.t)

    def bands_intact(self):
        return self.group_of.bands_intact() and self.lr_scale.bands_intact() and self.weight_decay.bands_intact()


def clip_buffers():
    ws, state = KC.ops().clip_buffers(DEV)
    return ws, state


# =====================================================================================================================
# 1. one group (1, 0), no EMA: the bits of mgx_adam_step and of mgx_adam_step_clipped
# =====================================================================================================================
@pytest.mark.parametrize("n", (1, 5, 67, BIG + 67))
@pytest.mark.parametrize("with_shadow", (True, False))
@pytest.mark.parametrize("mode", ("plain", "guard", "clip"))
def test_one_neutral_group_without_an_ema_is_the_existing_kernels_bit_for_bit(n, with_shadow, mode):
    ops = KC.ops()
    a, b = State(n, n, with_shadow, ema=False), State(n, n, with_shadow, ema=False)
    one = Groups([0] * chunks_of(n), [(1.0, 0.0)])
    ws, state = clip_buffers()
    for step in (1, 2, 3):
        g = guarded(gradient(n, step))
        if mode == "plain":
            ops.adam_step_groups(*a.args(g.t), *HYPER, step, GS, None, *one.args())
            ops.adam_step(*b.args(g.t)[:5], *HYPER, step, GS)
        else:
            max_norm = math.inf if mode == "guard" else 0.25 * float(gradient(n, step).double().norm()) * GS + 1e-3
            ops.grad_norm(g.t, GS, max_norm, ws, state)
            st = ops.read_clip_state(state)
            assert st["skipped_last"] == 0 and (mode == "guard" or st["clipped"] == step)
            ops.adam_step_groups(*a.args(g.t), *HYPER, step, 123.0, state, *one.args())       # gscale is ignored with a state
            ops.adam_step_clipped(*b.args(g.t)[:5], *HYPER, step, state)
        sa, sb = a.snapshot(), b.snapshot()
        for k in sa:
            assert sa[k].equal(sb[k]), f"n={n} step={step} {mode}: {k} differs from the existing kernel"
        assert a.bands_intact() and g.bands_intact() and one.bands_intact()
        assert g.t.cpu().equal(gradient(n, step))


# =====================================================================================================================
# 2. groups, decay, a frozen group, shadow and EMA against fp64, the state carried over three steps
# =====================================================================================================================
PAIRS = [(1.0, 0.1), (0.0, 0.5), (0.25, 0.0)]


def table_for(n):
    if n == 3 * 64 + 7:
        return [0, 1, 2, 2]                         # one chunk per group, the tail in a fourth chunk of group 2
    return [c % 3 for c in range(chunks_of(n))]     # group boundaries inside a wave's four chunks


@pytest.mark.parametrize("n", (3 * 64 + 7, BIG + 64 + 3))
def test_groups_decay_shadow_and_ema_against_fp64_with_the_state_carried_across_steps(n):
    ops = KC.ops()
    a = State(n, n + 1)
    grp = Groups(table_for(n), PAIRS)
    assert len(grp.table) == chunks_of(n)
    frozen = adamw_ref.element_groups(grp.table, n) == 1
    for step, decay in ((1, 0.1), (2, 0.999), (3, 0.5)):
        g_cpu = gradient(n, 10 + step)
        g = guarded(g_cpu)
        before = {k: b.t.cpu().clone() for k, b in a.buffers()}
        ops.adam_step_groups(*a.args(g.t), *HYPER, step, GS, None, *grp.args(), decay)
        r = adamw_ref.step(before["p"], g_cpu, before["m"], before["v"], before["ema"], *HYPER, step, GS, grp.table,
                           [s for s, _ in PAIRS], [w for _, w in PAIRS], decay)
        assert r["live"].equal(~frozen)
        case = f"n={n} step={step} decay={decay}"
        for k in ("p", "m", "v"):
            KC.check_floor("ADAMW", getattr(a, k).t, r[k], r["F_" + k], f"{case} {k}", C=KC.C_ADAM, seen=SEEN)
        KC.check_floor("EMA", a.ema.t, r["ema"], r["F_ema"], f"{case} ema", C=C_EMA, seen=SEEN)
        assert bits(a.shadow.t).equal(bits(a.p.t.to(BF))), case + ": shadow is not the bf16 rounding of p"
        for k, b in a.buffers():                     # the frozen group: bits, not a bound
            assert bits(b.t)[frozen].equal(bits(before[k])[frozen]), f"{case}: frozen elements of {k} changed"
            if k != "shadow":                        # (a step of lr may leave every bf16 rounding where it was)
                assert not bits(b.t)[~frozen].equal(bits(before[k])[~frozen]), f"{case}: {k} did not move"
        assert a.bands_intact() and g.bands_intact() and grp.bands_intact()


# =====================================================================================================================
# 3. frozen chunks: lr_scale 0, and a group byte outside the tables
# =====================================================================================================================
@pytest.mark.parametrize("n", (5 * 64 + 3, BIG + 64 + 3))
def test_frozen_chunks_keep_the_bits_of_all_five_buffers_while_their_neighbours_move(n):
    ops = KC.ops()
    a = State(n, n + 2)
    pairs = [(1.0, 0.1), (0.0, 0.5)]
    # chunk 1: frozen by its scale; chunk 3: a byte >= n_groups (2, and 255); the last chunk (the tail's): frozen too
    table = [0] * chunks_of(n)
    table[1], table[3], table[-1] = 1, 2, 255
    if n > BIG:
        table[BIG // 64 - 1], table[BIG // 64] = 1, 200          # either side of the first grid pass's end
    grp = Groups(table, pairs)
    elem = adamw_ref.element_groups(table, n)
    frozen = elem != 0
    before = a.snapshot()
    lead = {k: b.lead for k, b in a.buffers()}
    g = guarded(gradient(n, 3))
    ops.adam_step_groups(*a.args(g.t), *HYPER, 1, GS, None, *grp.args(), 0.9)
    after = a.snapshot()
    for k in before:
        x, y = after[k][lead[k]:lead[k] + n], before[k][lead[k]:lead[k] + n]
        assert x[frozen].equal(y[frozen]), f"n={n}: frozen elements of {k} changed"
        moved = x != y
        for c in sorted({0, 2, 4, len(table) - 2} | ({BIG // 64 - 2, BIG // 64 + 1} if n > BIG else set())):
            if table[c] == 0 and k != "shadow":       # (a step of lr may leave a chunk's bf16 roundings where they were)
                assert moved[c * 64:(c + 1) * 64].any(), f"n={n}: chunk {c} of {k} did not move"
    assert a.bands_intact() and g.bands_intact() and grp.bands_intact()
    assert torch.isfinite(a.p.t).all()


# =====================================================================================================================
# 4. the skipped step
# =====================================================================================================================
@pytest.mark.parametrize("n", (5, 3 * 64 + 7, BIG + 67))
def test_a_non_finite_gradient_skips_the_step_for_all_five_buffers_and_is_counted(n):
    ops = KC.ops()
    a = State(n, n + 3)
    grp = Groups(table_for(n), PAIRS)
    ws, state = clip_buffers()
    bad = gradient(n, 4).clone()
    bad[n // 2] = math.nan
    g = guarded(bad)
    before = a.snapshot()
    ops.grad_norm(g.t, GS, 1.0, ws, state)
    ops.adam_step_groups(*a.args(g.t), *HYPER, 1, GS, state, *grp.args(), 0.9)
    st = ops.read_clip_state(state)
    assert st["skipped_last"] == 1 and st["skipped"] == 1
    after = a.snapshot()
    for k in before:
        assert after[k].equal(before[k]), f"n={n}: {k} changed in a skipped step"
    # the next finite gradient updates, the EMA included
    g = guarded(gradient(n, 5))
    ops.grad_norm(g.t, GS, 1.0, ws, state)
    ops.adam_step_groups(*a.args(g.t), *HYPER, 2, GS, state, *grp.args(), 0.9)
    st = ops.read_clip_state(state)
    assert st["skipped_last"] == 0 and st["skipped"] == 1
    after = a.snapshot()
    live = adamw_ref.element_groups(grp.table, n) != 1
    if live.any():
        for k in ("p", "m", "v", "ema"):
            assert not after[k].equal(before[k]), f"n={n}: {k} did not move after the recovery"
        assert bits(a.shadow.t).equal(bits(a.p.t.to(BF)))
    assert a.bands_intact() and g.bands_intact() and grp.bands_intact()


# =====================================================================================================================
# 5. argument errors: the documented status, and no launch
# =====================================================================================================================
def test_argument_errors_return_the_documented_status_without_launching():
    lib, _, ptr, stream_ptr = KC.raw()
    n = 3 * 64 + 8
    a = State(n, 9)
    grp = Groups(table_for(3 * 64 + 7), PAIRS)
    g = guarded(gradient(n, 6))
    ws, state = clip_buffers()
    before = a.snapshot()
    P, G, M, V, S, E = (ptr(t) for t in a.args(g.t))
    T_, L, W, ST = ptr(grp.group_of.t), ptr(grp.lr_scale.t), ptr(grp.weight_decay.t), ptr(state)
    NULL, SHAPE = -2, -1

    def call(p=P, g_=G, m=M, v=V, s=S, e=E, n_=n, step=1, st=None, t=T_, l=L, w=W, k=3, d=0.9):
        return lib.mgx_adam_step_groups(p, g_, m, v, s, e, n_, *HYPER, step, GS, st, t, l, w, k, d, stream_ptr())

    calls = [
        (NULL, lambda: call(p=None)), (NULL, lambda: call(g_=None)), (NULL, lambda: call(m=None)), (NULL, lambda: call(v=None)),
        (NULL, lambda: call(t=None)), (NULL, lambda: call(l=None)), (NULL, lambda: call(w=None)),
        (SHAPE, lambda: call(n_=0)), (SHAPE, lambda: call(step=0)), (SHAPE, lambda: call(k=0)), (SHAPE, lambda: call(k=257)),
        (SHAPE, lambda: call(k=-1)), (SHAPE, lambda: call(d=1.0)), (SHAPE, lambda: call(d=-0.5)), (SHAPE, lambda: call(d=math.nan)),
        (SHAPE, lambda: call(p=P + 4, n_=n - 1)), (SHAPE, lambda: call(g_=G + 4, n_=n - 1)), (SHAPE, lambda: call(m=M + 8, n_=n - 2)),
        (SHAPE, lambda: call(v=V + 4, n_=n - 1)), (SHAPE, lambda: call(e=E + 4, n_=n - 1)), (SHAPE, lambda: call(s=S + 2, n_=n - 1)),
        (SHAPE, lambda: call(st=ST + 4)),
    ]
    for i, (want, c) in enumerate(calls):
        rc = c()
        assert rc == want, (i, rc, lib.mgx_last_error())
        assert lib.mgx_last_error(), i
    torch.cuda.synchronize()
    after = a.snapshot()
    for k in before:
        assert after[k].equal(before[k]), k
    # without an EMA the decay is not looked at; shadow and ema may both be NULL
    assert call(s=None, e=None, d=1.0) == 0
    assert call(k=256) == 0                                        # the largest table count (only three entries are read: the bytes are < 3)
    torch.cuda.synchronize()
    assert a.bands_intact() and grp.bands_intact()
    ops = KC.ops()
    with pytest.raises(ValueError):
        ops.adam_step_groups(*a.args(g.t), *HYPER, 1, GS, None, grp.group_of.t[:2], grp.lr_scale.t, grp.weight_decay.t)
    with pytest.raises(ValueError):
        ops.adam_step_groups(*a.args(g.t), *HYPER, 1, GS, None, grp.group_of.t, grp.lr_scale.t[:2], grp.weight_decay.t)
    with pytest.raises(ValueError):
        ops.adam_step_groups(*a.args(g.t), *HYPER, 1, GS, state[:2], *grp.args())
