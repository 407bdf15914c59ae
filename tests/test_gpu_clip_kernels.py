"""mgx_grad_norm and mgx_adam_step_clipped (include/mgx.h, K11b) against the fp64 reference of their contract (tests/clip_ref.py),
at the sizes where such kernels go wrong: a tail only, one vector, vector plus tail, a partly filled last block, the first n at
which a thread takes a second grid-stride iteration, several iterations plus a tail.

Bounds, none of them measured:
  norm     |got - ref| <= n 2^-52 ref.  The kernel forms every square exactly (fp32 x fp32 in fp64) and adds non-negative fp64 terms:
           any order is within (n - 1) 2^-53 of the exact sum, the reference (math.fsum) is the exact sum rounded once, the
           square root halves a relative error and the two roundings of sqrt and of the product with |gscale| add 2^-52.
  scale    BIT equality with the reference's (float)(gscale * coef), demanded only where the host has checked that the
           reference's fp64 value is farther than n 2^-51 (relative) from a point where its fp32 rounding changes -- and, when
           max_norm / (norm + 1e-6) is near 1, that it is farther than that from 1; the seed is re-drawn otherwise.
  Adam     max_norm = inf: bit equality with mgx_adam_step.  Clipped: the C_ADAM = 16 bound of tests/test_gpu_rowwise_kernels.py
           against oracle.train_ref with gscale = the bit-checked scale.
  skipped  p, m, v, shadow keep their bits.
Every buffer carries guard elements on both sides, the workspace beyond the blocks written and the memory behind the state too:
all are compared bit for bit after every call."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import clip_ref
import kernel_checks as KC
from kernel_checks import bits, nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)
from oracle import train_ref as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
F64 = torch.float64
PARTS = 1024
SIZES = (1, 3, 4, 5, 1023, 1025, 4 * 256 * 1024 + 4, 2 ** 21 + 3)
GUARD = 8                                           # elements on each side of every buffer
GS = 0.37                                           # a gradient scale that is no power of two
SEEN = {}


def blocks_of(n):
    return min(max((n // 4 + 255) // 256, 1), PARTS)


def guarded(data, dtype=None):
    """a device buffer of n elements with GUARD sentinel elements before and after it; .t is the view the kernels get (16-byte
    aligned for fp32 and fp64, 8-byte for bf16: GUARD elements are a multiple of 16 bytes), .buf the whole allocation"""
    data = torch.from_numpy(data.copy()) if isinstance(data, np.ndarray) else torch.as_tensor(data)
    data = data.to(dtype or data.dtype)
    b = KC.Banded(data, GUARD * data.element_size(), -12345.0 if data.dtype.is_floating_point else -12345)
    assert b.t.data_ptr() % (16 if data.dtype != BF else 8) == 0
    return b


class Clip:
    """workspace and state of mgx_grad_norm, both with sentinels: the workspace entirely (entries beyond `blocks` must keep them),
    the state in the 32 bytes that follow it"""

    def __init__(self):
        self.ws_full = torch.full((PARTS + GUARD,), -777.0, dtype=F64, device=DEV)
        self.ws = self.ws_full[:PARTS]
        self.st_full = torch.zeros(8, dtype=torch.int64, device=DEV)
        self.st_full[4:] = 0x5A5A5A5A5A5A5A5A
        self.state = self.st_full[:4]

    def run(self, g, gscale, max_norm):
        n = g.numel()
        KC.ops().grad_norm(g, gscale, max_norm, self.ws, self.state)
        ws = self.ws_full.cpu()
        b = blocks_of(n)
        assert (ws[b:] == -777.0).all(), f"n={n}: workspace written beyond its {b} blocks"
        assert (self.st_full[4:].cpu() == 0x5A5A5A5A5A5A5A5A).all(), "memory behind the state written"
        return KC.ops().read_clip_state(self.state)

    def state_bytes(self):
        return self.state.cpu().numpy().tobytes()

    def scale_bytes(self):
        return self.state_bytes()[8:12]


@functools.lru_cache(maxsize=None)
def gaussian(n, seed=0):
    """-> fp32 Gaussian gradients [n] as a read-only numpy array (shared by the tests: never modified)"""
    g = torch.randn(n, generator=torch.Generator().manual_seed(1000 * seed + n % 997)).numpy()
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def ref_norm(n, seed, factor):
    return clip_ref.norm(gaussian(n, seed) * np.float32(factor), 1.0)


# =====================================================================================================================
# 1. the norm
# =====================================================================================================================
@pytest.mark.parametrize("n", SIZES)
def test_norm_against_fp64_for_ordinary_huge_and_tiny_gradients(n):
    clip = Clip()
    for factor in (1.0, 1e25, 1e-30):
        g = gaussian(n) * np.float32(factor)
        ref = ref_norm(n, 0, factor)
        for gscale in (1.0, -0.5):
            gd = guarded(g)
            st = clip.run(gd.t, gscale, math.inf)
            want = ref * abs(gscale)
            err = abs(st["norm"] - want)
            print(f"[NORM] n={n} factor={factor:g} gscale={gscale}: got {st['norm']!r} ref {want!r} err/ref {err / want:.3e} bound {n * 2.0 ** -52:.3e}")
            assert err <= n * 2.0 ** -52 * want
            assert gd.bands_intact() and bits(gd.t).equal(bits(torch.from_numpy(g)))
            # max_norm = inf: measure only -- scale is gscale bit for bit, nothing is clipped or skipped
            assert clip.scale_bytes() == np.float32(gscale).tobytes() and st["skipped_last"] == 0 and st["clipped"] == 0 and st["skipped"] == 0


@pytest.mark.parametrize("n", SIZES)
def test_all_zero_gradients_have_norm_zero_and_no_nan(n):
    clip = Clip()
    gd = guarded(torch.zeros(n))
    for max_norm in (math.inf, 1.0):
        st = clip.run(gd.t, GS, max_norm)
        assert st["norm"] == 0.0 and clip.scale_bytes() == np.float32(GS).tobytes()
        assert st["skipped_last"] == 0 and st["clipped"] == 0 and st["skipped"] == 0


# =====================================================================================================================
# 2. scale: bit equality where the host says the rounding cannot flip
# =====================================================================================================================
@functools.lru_cache(maxsize=None)
def scale_cases(n):
    """-> (g, [(max_norm, reference step)]) for max_norm below, (as fp32) equal to and above the norm, and inf -- from the first seed
    at which every case is decidable: the reference's gscale * coef farther than n 2^-51 from an fp32 rounding boundary, and
    max_norm / (norm + 1e-6) farther than that from 1 (the clamp, and the `coef < 1` that n_clipped counts)"""
    margin = n * 2.0 ** -51
    for seed in range(1, 50):
        g = gaussian(n, seed)
        nrm = clip_ref.norm(g, GS)
        cases, ok = [], True
        for max_norm in (clip_ref.f32(0.25 * nrm), clip_ref.f32(nrm), clip_ref.f32(3.0 * nrm), math.inf):
            ref = clip_ref.step(g, GS, max_norm, nrm)
            raw = clip_ref.coef_raw(nrm, max_norm)
            ok &= clip_ref.f32_boundary_distance(clip_ref.f32(GS) * ref["coef"]) > margin and abs(raw - 1.0) > margin
            cases.append((max_norm, ref))
        if ok:
            return g, tuple(cases)
    raise AssertionError("no decidable seed")


@pytest.mark.parametrize("n", SIZES)
def test_scale_is_the_references_fp32_bit_for_bit_and_the_counter_counts_the_clipped_calls(n):
    g, cases = scale_cases(n)
    assert [r["clipped"] for _, r in cases][0] and not cases[2][1]["clipped"] and not cases[3][1]["clipped"]
    clip = Clip()
    gd = guarded(g)
    clipped = 0
    for max_norm, ref in list(cases) + list(cases)[::-1]:
        st = clip.run(gd.t, GS, max_norm)
        clipped += ref["clipped"]
        got = np.frombuffer(clip.scale_bytes(), np.float32)[0]
        print(f"[SCALE] n={n} max_norm={max_norm!r}: scale {got!r} ref {ref['scale']!r} coef {ref['coef']!r}")
        assert clip.scale_bytes() == ref["scale"].tobytes()
        assert abs(st["norm"] - ref["norm"]) <= n * 2.0 ** -52 * ref["norm"]
        assert st["clipped"] == clipped and st["skipped"] == 0 and st["skipped_last"] == 0
    assert gd.bands_intact()


def test_two_runs_give_the_same_state_bytes():
    n = 2 ** 21 + 3
    g = guarded(gaussian(n))
    a, b = Clip(), Clip()
    a.run(g.t, GS, 1.0)
    b.run(g.t, GS, 1.0)
    assert a.state_bytes() == b.state_bytes() and len(a.state_bytes()) == 32
    assert bits(a.ws[:blocks_of(n)]).equal(bits(b.ws[:blocks_of(n)]))


# =====================================================================================================================
# 3. the clipped Adam
# =====================================================================================================================
class AdamState:
    def __init__(self, n, seed, with_shadow):
        gen = torch.Generator().manual_seed(seed)
        self.p = guarded(torch.randn(n, generator=gen))
        self.m = guarded(0.1 * torch.randn(n, generator=gen))
        self.v = guarded(torch.rand(n, generator=gen))
        self.shadow = guarded(self.p.t.cpu().to(BF)) if with_shadow else None
        self.gen = gen

    def tensors(self):
        return [self.p, self.m, self.v] + ([self.shadow] if self.shadow else [])

    def snapshot(self):
        return [bits(x.buf).clone() for x in self.tensors()]

    def bands_intact(self):
        return all(x.bands_intact() for x in self.tensors())


HYPER = (1e-3, 0.9, 0.98, 1e-9)


@pytest.mark.parametrize("n", (1031, 4 * 2 ** 20 + 5))
@pytest.mark.parametrize("with_shadow", (True, False))
def test_without_a_clip_the_update_is_adam_steps_bit_for_bit(n, with_shadow):
    """max_norm = inf: scale == gscale, and the kernel is the same per-element code"""
    ops = KC.ops()
    a, b = AdamState(n, n, with_shadow), AdamState(n, n, with_shadow)
    clip = Clip()
    for step in (1, 2, 1000):
        g = guarded(torch.randn(n, generator=a.gen))
        st = clip.run(g.t, GS, math.inf)
        assert st["skipped_last"] == 0
        ops.adam_step_clipped(a.p.t, g.t, a.m.t, a.v.t, a.shadow.t if with_shadow else None, *HYPER, step, clip.state)
        ops.adam_step(b.p.t, g.t, b.m.t, b.v.t, b.shadow.t if with_shadow else None, *HYPER, step, GS)
        for x, y, name in zip(a.snapshot(), b.snapshot(), "pmvs"):
            assert x.equal(y), f"n={n} step={step}: {name} differs from mgx_adam_step"
        assert a.bands_intact() and g.bands_intact()


def check_f32(got, ref, F, case):
    assert got.dtype == torch.float32
    KC.check_floor("ADAM", got, ref, F, case, C=KC.C_ADAM, seen=SEEN)


@pytest.mark.parametrize("n", (1031, 2 ** 21 + 3))
@pytest.mark.parametrize("with_shadow", (True, False))
def test_clipped_update_against_fp64_with_the_state_carried_across_steps(n, with_shadow):
    ops = KC.ops()
    g_np, cases = scale_cases(n)
    max_norm, ref = cases[0]                                    # a quarter of the norm: clipped, scale decidable
    a = AdamState(n, n + 1, with_shadow)
    clip = Clip()
    g = guarded(g_np)
    grad = torch.from_numpy(g_np.copy())
    for k, step in enumerate((1, 2, 3)):
        st = clip.run(g.t, GS, max_norm)
        assert clip.scale_bytes() == ref["scale"].tobytes() and st["clipped"] == k + 1
        scale = float(ref["scale"])
        p0, m0, v0 = a.p.t.cpu(), a.m.t.cpu(), a.v.t.cpu()
        ops.adam_step_clipped(a.p.t, g.t, a.m.t, a.v.t, a.shadow.t if with_shadow else None, *HYPER, step, clip.state)
        r = T.adam_step(p0, grad, m0, v0, *HYPER, step, scale)
        F = T.adam_floor(p0, grad, m0, v0, *HYPER, step, scale, r)
        case = f"n={n} step={step} shadow={with_shadow}"
        check_f32(a.p.t, r[0], F[0], case + " p")
        check_f32(a.m.t, r[1], F[1], case + " m")
        check_f32(a.v.t, r[2], F[2], case + " v")
        if with_shadow:
            assert bits(a.shadow.t).equal(bits(a.p.t.to(BF))), case + ": shadow is not the bf16 rounding of p"
        assert a.bands_intact() and g.bands_intact()


# =====================================================================================================================
# 4. the skipped step
# =====================================================================================================================
@pytest.mark.parametrize("n", (7, 1027, 2 ** 21 + 3))
def test_a_non_finite_gradient_skips_the_step_and_the_next_finite_one_updates(n):
    ops = KC.ops()
    a = AdamState(n, n + 2, True)
    clip = Clip()
    clean = gaussian(n)
    n4 = n // 4 * 4
    skipped, step = 0, 0
    for where in (0, n4 - 1, n - 1):                             # element 0, the last element of the vector part, the tail
        for bad in (math.inf, -math.inf, math.nan):
            g_np = clean.copy()
            g_np[where] = bad
            g = guarded(g_np)
            before = a.snapshot()
            st = clip.run(g.t, GS, 1.0)
            skipped += 1
            step += 1
            assert st["skipped_last"] == 1 and st["skipped"] == skipped and st["scale"] == 0.0 and not math.isfinite(st["norm"]), (where, bad, st)
            ops.adam_step_clipped(a.p.t, g.t, a.m.t, a.v.t, a.shadow.t, *HYPER, step, clip.state)
            for x, y, name in zip(a.snapshot(), before, "pmvs"):
                assert x.equal(y), f"n={n} where={where} bad={bad}: {name} changed in a skipped step"
            assert g.bands_intact()
        # the next call with finite gradients clears the flag and updates
        g = guarded(clean)
        before = a.snapshot()
        st = clip.run(g.t, GS, 1.0)
        step += 1
        assert st["skipped_last"] == 0 and st["skipped"] == skipped and math.isfinite(st["norm"])
        ops.adam_step_clipped(a.p.t, g.t, a.m.t, a.v.t, a.shadow.t, *HYPER, step, clip.state)
        moved = [not x.equal(y) for x, y in zip(a.snapshot()[:3], before[:3])]
        assert all(moved), moved                                  # p, m and v; the shadow follows p
        assert bits(a.shadow.t).equal(bits(a.p.t.to(BF)))
        assert a.bands_intact() and torch.isfinite(a.p.t).all()


# =====================================================================================================================
# 5. argument errors: the documented status, and no launch (the state keeps its bytes)
# =====================================================================================================================
def test_argument_errors_return_the_documented_status_without_launching():
    lib, _, ptr, stream_ptr = KC.raw()
    n = 1031
    g, p, m, v = (guarded(torch.randn(n)) for _ in range(4))
    clip = Clip()
    clip.run(g.t, GS, 1.0)
    before_state, before_ws = clip.st_full.cpu().clone(), bits(clip.ws_full).clone()
    before = [bits(x.buf).clone() for x in (p, m, v)]
    G, W, S = ptr(g.t), ptr(clip.ws), ptr(clip.state)
    fl = ctypes.c_float
    NULL, SHAPE = -2, -1
    calls = [
        (NULL, lambda: lib.mgx_grad_norm(None, n, 1.0, 1.0, W, S, stream_ptr())),
        (NULL, lambda: lib.mgx_grad_norm(G, n, 1.0, 1.0, None, S, stream_ptr())),
        (NULL, lambda: lib.mgx_grad_norm(G, n, 1.0, 1.0, W, None, stream_ptr())),
        (SHAPE, lambda: lib.mgx_grad_norm(G, 0, 1.0, 1.0, W, S, stream_ptr())),
        (SHAPE, lambda: lib.mgx_grad_norm(G + 4, n - 1, 1.0, 1.0, W, S, stream_ptr())),          # g not 16-byte aligned
        (SHAPE, lambda: lib.mgx_grad_norm(G, n, 1.0, 1.0, W + 4, S, stream_ptr())),
        (SHAPE, lambda: lib.mgx_grad_norm(G, n, 1.0, 1.0, W, S + 4, stream_ptr())),
        (SHAPE, lambda: lib.mgx_grad_norm(G, n, 1.0, 0.0, W, S, stream_ptr())),
        (SHAPE, lambda: lib.mgx_grad_norm(G, n, 1.0, -1.0, W, S, stream_ptr())),
        (SHAPE, lambda: lib.mgx_grad_norm(G, n, 1.0, fl(-math.inf), W, S, stream_ptr())),
        (SHAPE, lambda: lib.mgx_grad_norm(G, n, 1.0, fl(math.nan), W, S, stream_ptr())),
        (NULL, lambda: lib.mgx_adam_step_clipped(ptr(p.t), G, ptr(m.t), ptr(v.t), None, n, *HYPER, 1, None, stream_ptr())),
        (NULL, lambda: lib.mgx_adam_step_clipped(None, G, ptr(m.t), ptr(v.t), None, n, *HYPER, 1, S, stream_ptr())),
        (SHAPE, lambda: lib.mgx_adam_step_clipped(ptr(p.t) + 4, G, ptr(m.t), ptr(v.t), None, n - 1, *HYPER, 1, S, stream_ptr())),
        (SHAPE, lambda: lib.mgx_adam_step_clipped(ptr(p.t), G, ptr(m.t), ptr(v.t), None, n, *HYPER, 1, S + 4, stream_ptr())),
        (SHAPE, lambda: lib.mgx_adam_step_clipped(ptr(p.t), G, ptr(m.t), ptr(v.t), None, n, *HYPER, 0, S, stream_ptr())),
        (SHAPE, lambda: lib.mgx_adam_step_clipped(ptr(p.t), G, ptr(m.t), ptr(v.t), None, 0, *HYPER, 1, S, stream_ptr())),
    ]
    for i, (want, call) in enumerate(calls):
        rc = call()
        assert rc == want, (i, rc, lib.mgx_last_error())
        assert lib.mgx_last_error(), i
    torch.cuda.synchronize()
    assert clip.st_full.cpu().equal(before_state) and bits(clip.ws_full).equal(before_ws)
    for x, y in zip((p, m, v), before):
        assert bits(x.buf).equal(y)
    ops = KC.ops()
    with pytest.raises(ValueError):
        ops.grad_norm(g.t, 1.0, 1.0, clip.ws[:8], clip.state)                # workspace too small
    with pytest.raises(ValueError):
        ops.grad_norm(g.t, 1.0, 1.0, clip.ws, clip.state[:2])                # state too small
