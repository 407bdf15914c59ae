"""tests/kernel_checks.py judges every kernel: its checks and guard bands on synthetic tensors, on the CPU."""
import math

import numpy as np
import pytest
import torch

import kernel_checks as KC

F64 = torch.float64
REF = torch.tensor([[1.0, -2.0, 4.0], [8.0, 16.0, -32.0]], dtype=F64)


def floor_case(ratio, C=4.0, rounding=0.0, extra=None, F=None):
    """got whose element [1, 2] lies at `ratio` floors beyond the rounding and extra terms, all others exact"""
    F = torch.full(REF.shape, 0.5, dtype=F64) if F is None else F
    Fe = torch.as_tensor(F, dtype=F64)
    Fe = (Fe.unsqueeze(-1) if Fe.dim() < REF.dim() else Fe).expand(REF.shape)
    got = REF.clone()
    got[1, 2] += rounding * REF[1, 2].abs() + (0.0 if extra is None else extra[1, 2]) + ratio * Fe[1, 2]
    seen = {}
    KC.check_floor("FAM", got, REF, F, "case", C=C, seen=seen, rounding=rounding, extra=extra)
    return seen


@pytest.mark.parametrize("rounding", (0.0, 2.0 ** -8))
@pytest.mark.parametrize("extra", (None, torch.full((2, 3), 0.25, dtype=F64)))
@pytest.mark.parametrize("F", (None, torch.tensor([0.5, 2.0])), ids=("F-per-element", "F-per-row"))
def test_check_floor_passes_just_under_C_and_raises_just_over(rounding, extra, F):
    seen = floor_case(4.0 * (1 - 1e-9), rounding=rounding, extra=extra, F=F)
    assert seen["FAM"][1] == "case" and abs(seen["FAM"][0] - 4.0) < 1e-6
    with pytest.raises(AssertionError, match=r"element \(1, 2\)"):
        floor_case(4.0 * (1 + 1e-9), rounding=rounding, extra=extra, F=F)


def test_check_floor_keeps_the_worst_ratio_and_its_case():
    seen = {}
    for case, d in (("small", 0.5), ("large", 1.5), ("middle", 1.0)):
        KC.check_floor("FAM", REF + d, REF, 1.0, case, C=4.0, seen=seen)
    assert seen == {"FAM": (1.5, "large")}


@pytest.mark.parametrize("bad", (float("nan"), float("inf"), -float("inf")))
def test_check_floor_raises_on_a_non_finite_output(bad):
    got = REF.clone()
    got[0, 1] = bad
    with pytest.raises(AssertionError, match="non-finite"):
        KC.check_floor("FAM", got, REF, 1.0, "case", C=4.0, seen={})


def test_check_floor_raises_on_a_floor_of_zero():
    F = torch.ones(2, 3, dtype=F64)
    F[1, 0] = 0.0
    with pytest.raises(AssertionError, match="floor"):
        KC.check_floor("FAM", REF, REF, F, "case", C=4.0, seen={})


def test_check_floor_rows_wants_minus_inf_and_nan_matched_exactly():
    ref = np.array([1.0, -np.inf, np.nan, 3.0])
    F = np.array([0.5, 0.0, 0.0, 0.5])                        # no floor is asked of the entries compared exactly
    seen = {}
    KC.check_floor_rows("FAM", ref + np.array([1.0, 0, 0, 0]), ref, F, "case", C=4.0, seen=seen)
    assert seen == {"FAM": (2.0, "case")}
    with pytest.raises(AssertionError, match=r"element \(3,\)"):
        KC.check_floor_rows("FAM", ref + np.array([0, 0, 0, 2.5]), ref, F, "case", C=4.0, seen={})
    for i, v in ((1, -1e30), (1, np.inf), (2, 0.0), (0, np.nan)):
        got = ref.copy()
        got[i] = v
        with pytest.raises(AssertionError, match="differ"):
            KC.check_floor_rows("FAM", got, ref, F, "case", C=4.0, seen={})
    KC.check_floor_rows("FAM", ref[1:3], ref[1:3], F[1:3], "case", C=4.0, seen=seen)      # nothing finite: nothing recorded
    assert seen == {"FAM": (2.0, "case")}


def test_check_bound_holds_at_the_bound_and_fails_one_ulp_above():
    bound = torch.tensor([[0.5, 0.0, 3.0], [1e-3, 7.0, 0.1]], dtype=F64)
    seen = {}
    KC.check_bound("FAM", REF + bound, REF, REF + bound - REF, "at", seen=seen)              # err == bound in fp64, by construction
    KC.check_bound("FAM", REF - bound * 0.5, REF, bound, "half", seen=seen, key=("FAM", "kind"))
    assert seen == {"FAM": (1.0, "at"), ("FAM", "kind"): (0.5, "half")}
    got = REF.clone()
    got[1, 1] = 16.0 + 7.0
    KC.check_bound("FAM", got, REF, bound, "at", seen=seen)
    got[1, 1] = math.nextafter(16.0 + 7.0, math.inf)
    assert got[1, 1] - REF[1, 1] > 7.0
    with pytest.raises(AssertionError, match=r"element \(1, 1\)"):
        KC.check_bound("FAM", got, REF, bound, "above", seen=seen)
    zero, tiny = torch.zeros(3, dtype=F64), torch.full((3,), 1e-310, dtype=F64)             # a bound below the clamp of the printed ratio
    KC.check_bound("FAM", tiny, zero, tiny, "denormal", seen={})
    with pytest.raises(AssertionError):
        KC.check_bound("FAM", 2 * tiny, zero, tiny, "denormal", seen={})


def test_check_bound_of_zero_demands_equality():
    zero = torch.zeros(2, 3, dtype=F64)
    KC.check_bound("FAM", REF, REF, zero, "equal", seen={})
    got = REF.clone()
    got[0, 0] = math.nextafter(1.0, 2.0)
    with pytest.raises(AssertionError, match=r"element \(0, 0\)"):
        KC.check_bound("FAM", got, REF, zero, "off by an ulp", seen={})


@pytest.mark.parametrize("which,bad", (("ref", float("nan")), ("ref", float("inf")), ("bound", float("nan")), ("bound", float("inf")),
                                       ("bound", -1.0), ("got", float("nan")), ("got", -float("inf"))))
def test_check_bound_refuses_an_output_a_reference_or_a_bound_that_is_not_a_number(which, bad):
    t = {"got": REF.clone(), "ref": REF.clone(), "bound": torch.ones(2, 3, dtype=F64)}
    t[which][1, 0] = bad
    with pytest.raises(AssertionError, match="non-finite" if which == "got" else "not a number"):
        KC.check_bound("FAM", t["got"], t["ref"], t["bound"], "case", seen={})


def test_check_equal_compares_values():
    KC.check_equal("FAM", torch.tensor([0.0, -0.0, 2.0]), torch.tensor([-0.0, 0.0, 2.0], dtype=F64), "zeros")
    KC.check_equal("FAM", torch.zeros(3), 0.0, "scalar")
    with pytest.raises(AssertionError, match="1 elements differ"):
        KC.check_equal("FAM", torch.tensor([0.0, 1.0]), 0.0, "scalar")
    with pytest.raises(AssertionError):
        KC.check_equal("FAM", torch.tensor([float("nan")]), torch.tensor([float("nan")], dtype=F64), "NaN is equal to nothing")


BANDS = [(torch.bfloat16, 512, b"\x5a"), (torch.float32, 512, float("nan")), (torch.float32, 32, 777.0), (torch.int32, 32, 777),
         (torch.float64, 64, -12345.0), (torch.bfloat16, 16, -12345.0)]


@pytest.mark.parametrize("dtype,band,fill", BANDS, ids=[f"{str(d)[6:]}-{b}-{f!r}" for d, b, f in BANDS])
def test_banded_notices_one_flipped_byte_in_either_band(dtype, band, fill):
    t = torch.arange(15).reshape(3, 5).to(dtype)
    b = KC.Banded(t, band, fill, device="cpu")
    assert b.t.shape == t.shape and torch.equal(b.t, t)
    assert b.t.data_ptr() - b.buf.data_ptr() == band and b.buf.numel() * t.element_size() == 2 * band + 15 * t.element_size()
    raw = b.buf.view(torch.uint8)
    if isinstance(fill, bytes):
        assert (raw[:band] == fill[0]).all() and (raw[-band:] == fill[0]).all()
    elif fill == fill:
        assert (b.buf[:b.lead] == fill).all() and (b.buf[-b.lead:] == fill).all()
    else:
        assert torch.isnan(b.buf[:b.lead]).all() and torch.isnan(b.buf[-b.lead:]).all()
    assert b.bands_intact()
    b.t.fill_(3)                                                # the interior is the call's to write
    assert b.bands_intact()
    for at in (0, band - 1, raw.numel() - band, raw.numel() - 1):
        raw[at] ^= 1
        assert not b.bands_intact(), at
        raw[at] ^= 1
        assert b.bands_intact()


def test_output_starts_as_the_pattern_and_operand_lies_in_nan():
    o = KC.output((4, 6), torch.bfloat16, device="cpu")
    assert (o.buf.view(torch.uint8) == 0x5A).all() and o.t.shape == (4, 6) and o.bands_intact()
    assert o.t.data_ptr() - o.buf.data_ptr() == KC.BAND == 512
    init = torch.arange(6.0)
    a = KC.output(None, torch.float32, init, device="cpu")
    assert torch.equal(a.t, init) and (a.buf.view(torch.uint8)[:512] == 0x5A).all() and KC.P(a) == a.t.data_ptr()
    x = KC.operand(init, device="cpu")
    assert torch.equal(x.t, init) and torch.isnan(x.buf[:128]).all() and torch.isnan(x.buf[-128:]).all()
    assert KC.operand(None) is None and KC.P(None) is None


def test_bits_and_the_norm_helpers():
    assert KC.bits(torch.tensor([1.0])).item() == 0x3F800000 and KC.bits(torch.tensor([1.0], dtype=torch.bfloat16)).item() == 0x3F80
    assert KC.bits(torch.tensor([1.0], dtype=F64)).item() == 0x3FF << 52 and KC.bits(torch.tensor([7])).item() == 7
    assert KC.bits16(torch.tensor([-0.0], dtype=torch.bfloat16)).item() == -0x8000
    a = torch.tensor([3.0, 4.0])
    assert abs(KC.cos(a, 2 * a) - 1.0) < 1e-6 and KC.cos(a, torch.tensor([-4.0, 3.0])) == 0.0 and abs(KC.rel(1.5 * a, a) - 0.5) < 1e-6
    assert torch.equal(torch.randn(3, generator=KC.gen(2, 5)), torch.randn(3, generator=KC.gen(2, 5)))
    w, b = KC.weights(6, 4, 1)
    assert w.shape == (6, 4) and w.dtype == torch.bfloat16 and b.shape == (6,) and b.dtype == torch.float32
