"""What a test module of raw kernels needs, in one form: the library handles, the fixtures that report the measured ratios and
that end the session after a GPU error, the element-by-element checks against an fp64 reference (floor, bound, equal), buffers
inside guard bands, and a few small helpers.  Imported by basename, like beam_ref / clip_ref / score_ref.

Every check records the largest ratio it has seen per family in the `seen` dict of the calling module, which prints them when it
is done (report_fixture); the constants, the bounds and the references stay in the modules."""
import os

import numpy as np
import pytest
import torch

BF, F64 = torch.bfloat16, torch.float64
BAND = 512                                          # bytes before and after every buffer of operand() / output()
PATTERN = b"\x5a"
C_ADAM = 16.0                                       # noise floors an Adam update may be off by: C["ADAM"] of tests/test_gpu_rowwise_kernels.py
                                                    # (measured there), which the two clip modules check the clipped step with as well
# noise floors a row-wise kernel may be off by, per family (LayerNorm forward / backward, cross entropy, embedding): measured by
# tests/test_gpu_rowwise_kernels.py on its edge cases (its docstring has the figures); tests/step_trace.py holds a traced step to them
C_ROWWISE = {"LNF": 8.0, "LNB": 4.0, "CE": 8.0, "EMB": 4.0}


def raw(product_only=False):
    """-> (lib, check, ptr, stream_ptr); product_only: the module is about libmgx.so as built, not an experiment build"""
    from musicgeneration_amd import _lib
    if product_only:
        assert "MGX_LIB_PATH" not in os.environ, "this module is about the product library"
    return _lib.load(), _lib.check, _lib.ptr, _lib.stream_ptr


def ops():
    from musicgeneration_amd import ops as o
    return o


def report_fixture(seen, label):
    """the module-scoped fixture that prints, after the module's last test, `MEASURED <family>: <label> at <case>` for every
    family in `seen`; label is a format of the ratio, e.g. "largest ratio {:.3f}"; a (family, kind) key prints as family [kind]"""
    @pytest.fixture(scope="module", autouse=True)
    def _report():
        yield
        for key, (r, case) in sorted(seen.items()):
            fam = key if isinstance(key, str) else f"{key[0]} [{key[1]}]"
            print(f"\nMEASURED {fam}: {label.format(r)} at {case}", end="")
        print()
    return _report


@pytest.fixture(autouse=True)
def nothing_more_after_a_gpu_error():
    """a HIP error is sticky and the device may be shared: the session ends instead of launching the remaining cases on it"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU error, nothing more is launched: {e}", returncode=3)


# ---- checks ---------------------------------------------------------------------------------------------------------------------
def _note(seen, key, worst, case, line):
    if worst > seen.get(key, (-1.0, None))[0]:
        seen[key] = (worst, case)
    print(line)


def check_floor(fam, got, ref, F, case, *, C, seen, rounding=0.0, extra=None):
    """|got - ref| <= rounding |ref| + extra + C F, element by element; got finite, F > 0 (a floor per row is broadcast over the
    trailing dimensions); records the largest (|err| - rounding |ref| - extra) / F"""
    got = got.detach().cpu().to(F64).reshape(ref.shape)
    assert torch.isfinite(got).all(), (fam, case, "non-finite output", torch.nonzero(~torch.isfinite(got))[:4].tolist())
    F = torch.as_tensor(F, dtype=F64)
    while F.dim() < ref.dim():
        F = F.unsqueeze(-1)
    F = F.expand(ref.shape)
    assert (F > 0).all(), (fam, case, "a floor is not positive")
    ratio = ((got - ref).abs() - rounding * ref.abs() - (0.0 if extra is None else extra)) / F
    worst = ratio.max().item()
    _note(seen, fam, worst, case, f"[{fam}] {case}: ratio {worst:.3f}")
    if worst > C:
        i = tuple(int(v) for v in np.unravel_index(int(ratio.argmax()), ratio.shape))
        raise AssertionError(f"{fam} {case}: element {i} got {got[i].item()!r} ref {ref[i].item()!r} F {F[i].item():.3e} ratio {worst:.2f} > {C}")


def check_floor_rows(fam, got, ref, F, case, *, C, seen):
    """check_floor on numpy rows whose reference may hold -inf and NaN: those entries must match exactly, the finite ones lie
    within C F"""
    got, ref, F = (np.asarray(a, dtype=np.float64) for a in (got, ref, F))
    fin = np.isfinite(ref)
    assert (np.isnan(got) == np.isnan(ref)).all(), (fam, case, "NaN rows differ")
    assert (got[~fin & ~np.isnan(ref)] == ref[~fin & ~np.isnan(ref)]).all(), (fam, case, "infinite entries differ")
    if fin.any():                                   # the entries already compared count as exact: error 0 over a floor of 1
        check_floor(fam, *(torch.from_numpy(np.where(fin, a, v)) for a, v in ((got, 0.0), (ref, 0.0), (F, 1.0))), case, C=C, seen=seen)


def check_bound(fam, got, ref, bound, case, *, seen, key=None):
    """|got - ref| <= bound, element by element (bound 0: equal); got, ref and bound finite, bound >= 0; records the largest
    error / bound under `key` (the family unless given)"""
    got = got.detach().cpu().to(F64)
    assert torch.isfinite(got).all(), (fam, case, "non-finite output", torch.nonzero(~torch.isfinite(got))[:4].tolist())
    assert torch.isfinite(ref).all() and torch.isfinite(bound).all() and (bound >= 0).all(), (fam, case, "the reference or its bound is not a number")
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = ratio.max().item()
    _note(seen, fam if key is None else key, worst, case, f"[{fam}] {case}: error / bound {worst:.3g}")
    if not (worst <= 1.0 and (err <= bound).all()):             # (the comparison itself: a bound below 1e-300 is clamped in the ratio)
        i = tuple(int(v) for v in torch.nonzero((ratio == ratio.max()) | ~(err <= bound))[0])
        raise AssertionError(f"{fam} {case}: element {i} got {got[i].item()!r} ref {ref[i].item()!r} bound {bound[i].item():.3e} ratio {worst:.3f}")


def check_equal(fam, got, want, case):
    """the values are equal (-0 == +0), element by element; want may be a scalar"""
    got = got.detach().cpu().to(F64)
    bad = torch.nonzero(~(got == want))
    assert bad.numel() == 0, (f"{fam} {case}: {bad.shape[0]} elements differ, first {bad[:4].tolist()} got "
                              f"{[got[tuple(i)].item() for i in bad[:4]]} want {[torch.as_tensor(want).expand_as(got)[tuple(i)].item() for i in bad[:4]]}")
    print(f"[{fam}] {case}: exact")


# ---- the analytic bounds of the training GEMMs on Gaussian data (tests/test_gpu_gemm_kernels.py derives them) -----------------------
def gemm_fwd_bound(pre, S, R):
    """bf16 output of a forward GEMM: 2^-8 |ref| (its rounding) + R 2^-23 S (an fp32 sum of R terms in any order; R = reduction
    length, + 1 with a bias)"""
    return 2.0 ** -8 * pre.abs() + R * 2.0 ** -23 * S


def gemm_dx_bound(pm, S, N, add=None):
    """dX of reduction length N, pm the masked product -> (ref, bound): 2^-8 |pm| + N 2^-23 S, and with an addend the two-rounding
    form on ref = pm + addend: 2^-8 |ref| + (1 + 2^-8) (2^-8 |pm| + N 2^-23 S)"""
    first = 2.0 ** -8 * pm.abs() + N * 2.0 ** -23 * S
    if add is None:
        return pm, first
    ref = pm + add.to(F64)
    return ref, 2.0 ** -8 * ref.abs() + (1 + 2.0 ** -8) * first


def gemm_dw_bound(S, M):
    """fp32 gW / gb: M terms and the slot's start value, any order: (M + 1) 2^-23 S, S the sum of |terms|, |start| included"""
    return (M + 1) * 2.0 ** -23 * S


# ---- guard bands ----------------------------------------------------------------------------------------------------------------
class Banded:
    """a CPU tensor placed on the device inside a larger allocation: `band` bytes of `fill` before and after it.  fill is a
    value of the tensor's type (NaN: a read outside an operand poisons the result) or one byte, repeated (b"\\x5a").  .t is the
    interior, .buf the whole allocation"""

    def __init__(self, t, band, fill, device="cuda:0"):
        t = t.contiguous()
        es = t.element_size()
        assert band % es == 0
        self.band, self.lead, self.n = band, band // es, t.numel()
        self.buf = torch.empty(self.n + 2 * self.lead, dtype=t.dtype, device=device)
        if isinstance(fill, bytes):
            self.buf.view(torch.uint8).fill_(fill[0])
        else:
            self.buf.fill_(fill)
        self.t = self.buf[self.lead:self.lead + self.n].view(t.shape)
        self.t.copy_(t)
        assert self.t.data_ptr() - self.buf.data_ptr() == band      # a multiple of 256 bytes leaves the alignment as it was
        self.bands = self._bands()

    def _bands(self):
        b = self.buf.view(torch.uint8)
        return torch.cat([b[:self.band], b[self.band + self.n * self.buf.element_size():]]).cpu()

    def bands_intact(self):
        """both bands hold the bytes they were filled with"""
        return torch.equal(self._bands(), self.bands)


def operand(t, device="cuda:0"):
    return None if t is None else Banded(t, BAND, float("nan"), device)


def output(shape, dtype, init=None, device="cuda:0"):
    """an output inside pattern bands; its interior starts as `init` (gW / gb accumulate) or as the pattern (every element must be
    written: 0x5A5A is 1.5e16 in bf16)"""
    if init is not None:
        return Banded(init.to(dtype), BAND, PATTERN, device)
    o = Banded(torch.zeros(shape, dtype=dtype), BAND, PATTERN, device)
    o.t.view(torch.uint8).fill_(PATTERN[0])
    return o


def P(b):
    return None if b is None else b.t.data_ptr()


class Stream:
    """the stream a case launches on: the default stream (the whole device) or the CU-masked stream of `cus` CUs"""

    def __init__(self, cus=0):
        self.ms = ops().masked_stream(cus) if cus else None

    def __enter__(self):
        torch.cuda.synchronize()
        if self.ms is not None:
            self.ctx = torch.cuda.stream(self.ms.stream)
            self.ctx.__enter__()
            assert raw()[3]() == self.ms.ptr
        return self

    def __exit__(self, *exc):
        if self.ms is not None:
            self.ctx.__exit__(*exc)
        torch.cuda.synchronize()


class Det:
    """deterministic mode for the calls inside, on the masked stream `ms` too"""

    def __init__(self, on, ms=None):
        self.on, self.ms = on, ms

    def __enter__(self):
        if self.on:
            ops().set_deterministic(True)
            if self.ms is not None:
                ops()._det_register_stream(self.ms)

    def __exit__(self, *exc):
        if self.on:
            torch.cuda.synchronize()
            ops().set_deterministic(False)


# ---- small helpers --------------------------------------------------------------------------------------------------------------
def bits(t):
    """the tensor's bits as integers of its width, on the CPU (integer tensors as they are)"""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16) if t.dtype == BF else t.view(torch.int64) if t.dtype == F64 else t


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)))


def weights(N, K, seed):
    g = gen(N, K, seed)
    return (torch.randn(N, K, generator=g) / K ** 0.5).to(BF), torch.randn(N, generator=g)


def cos(a, b):
    a, b = a.float().flatten().cpu(), b.float().flatten().cpu()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


def rel(a, b):
    a, b = a.float().flatten().cpu(), b.float().flatten().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()
