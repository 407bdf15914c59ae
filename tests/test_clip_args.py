"""Host side of gradient clipping (no GPU): the argument check of FusedAdam(max_norm=...) / train.py --clip-norm, and the fp64
reference of the kernels' contract (tests/clip_ref.py) against torch.nn.utils.clip_grad_norm_ run in fp64 on the CPU."""
import math

import numpy as np
import pytest
import torch

import clip_ref


def test_check_clip_args_accepts_positive_numbers_and_inf():
    from musicgeneration_amd.optim import check_clip_args
    for ok in (1, 0.5, 1e-30, 1e30, float("inf"), np.float32(2.0), np.float64(3.0)):
        got = check_clip_args(ok)
        assert isinstance(got, float) and got == float(ok)


@pytest.mark.parametrize("bad", (0, 0.0, -0.0, -1.0, float("-inf"), float("nan"), "1.0", None, True, [1.0], 1 + 0j))
def test_check_clip_args_rejects_everything_else(bad):
    from musicgeneration_amd.optim import check_clip_args
    with pytest.raises(ValueError, match="max_norm"):
        check_clip_args(bad)


def test_train_cli_parses_clip_norm():
    from musicgeneration_amd import train
    assert train.get_options([]).clip_norm == 0.0                      # off by default
    assert train.get_options(["--clip-norm", "0.5"]).clip_norm == 0.5
    assert math.isinf(train.get_options(["--clip-norm", "inf"]).clip_norm)


def _torch_clip(g64, splits, max_norm):
    """clip_grad_norm_ in fp64 over the flat vector split into a few tensors -> (returned norm, the gradients afterwards, flat)"""
    parts = [torch.nn.Parameter(torch.zeros(k, dtype=torch.float64)) for k in splits]
    off = 0
    for p, k in zip(parts, splits):
        p.grad = torch.from_numpy(g64[off:off + k].copy())
        off += k
    total = torch.nn.utils.clip_grad_norm_(parts, max_norm)
    return total.item(), torch.cat([p.grad for p in parts]).numpy()


@pytest.mark.parametrize("n,splits", ((1, (1,)), (5, (2, 3)), (1031, (7, 1000, 24)), (40000, (1, 39000, 999))))
@pytest.mark.parametrize("gscale", (1.0, 0.25))
def test_reference_is_torchs_clip_grad_norm(n, splits, gscale):
    """torch measures the gradients it is given: hand it g * gscale (exact in fp64 for a power of two), compare norm, coefficient
    and the scaled gradients -- with max_norm below the norm (clipped), far below, and above it (nothing is scaled)"""
    rng = np.random.default_rng(n)
    g = rng.standard_normal(n).astype(np.float32)
    g64 = g.astype(np.float64) * gscale
    nrm = clip_ref.norm(g, gscale)
    for max_norm in (0.5 * nrm, 1e-3 * nrm, 2.0 * nrm + 1.0):
        max_norm = clip_ref.f32(max_norm)
        total, after = _torch_clip(g64, splits, max_norm)
        ref = clip_ref.step(g, gscale, max_norm)
        assert abs(total - ref["norm"]) <= n * 2.0 ** -52 * ref["norm"]
        assert not ref["skipped"] and ref["clipped"] == (max_norm < nrm)
        # torch multiplies by clamp(max_norm / (norm + 1e-6), max=1): the reference's coef, up to the norm's rounding
        want = g64 * ref["coef"]
        assert np.abs(after - want).max() <= (n + 4) * 2.0 ** -52 * np.abs(want).max()
        if max_norm > nrm:
            assert ref["coef"] == 1.0 and ref["scale"] == np.float32(gscale) and np.array_equal(after, g64)
        else:
            assert abs(float(ref["scale"]) - gscale * ref["coef"]) <= 2.0 ** -24 * gscale * ref["coef"]      # one fp32 rounding


def test_reference_with_infinite_max_norm_never_clips():
    g = np.array([3e30, -4e30, 1e-30], np.float32)
    ref = clip_ref.step(g, 0.37, float("inf"))
    assert ref["coef"] == 1.0 and not ref["clipped"] and not ref["skipped"]
    assert ref["scale"].tobytes() == np.float32(0.37).tobytes()
    assert abs(ref["norm"] - 5e30 * clip_ref.f32(0.37)) <= 1e-6 * ref["norm"]       # no overflow: the squares are fp64
    assert clip_ref.norm(np.zeros(9, np.float32), 0.5) == 0.0
    z = clip_ref.step(np.zeros(9, np.float32), 0.5, 1.0)
    assert z["norm"] == 0.0 and z["coef"] == 1.0 and z["scale"] == np.float32(0.5)


@pytest.mark.parametrize("bad", (float("inf"), float("-inf"), float("nan")))
@pytest.mark.parametrize("where", (0, 3, 6))
def test_reference_skips_a_step_with_a_non_finite_gradient(bad, where):
    g = np.arange(1, 8, dtype=np.float32)
    g[where] = bad
    ref = clip_ref.step(g, 0.5, 1.0)
    assert ref["skipped"] and not ref["clipped"] and not math.isfinite(ref["norm"])
    assert ref["scale"].tobytes() == np.float32(0.0).tobytes()
    g[where] = 1.0
    assert not clip_ref.step(g, 0.5, 1.0)["skipped"]


def test_fp32_boundary_distance():
    """the host-side condition of the GPU test's bit-equality demand on `scale`"""
    one = np.float32(1.0)
    up = float(np.nextafter(one, np.float32(2.0)))
    assert clip_ref.f32_boundary_distance(1.0) == pytest.approx(2.0 ** -25, rel=1e-6)       # the nearer midpoint is below 1
    mid = (1.0 + up) / 2.0
    assert clip_ref.f32_boundary_distance(mid) == 0.0
    assert clip_ref.f32_boundary_distance(mid * (1 + 2.0 ** -40)) == pytest.approx(2.0 ** -40, rel=1e-3)
    assert clip_ref.f32_boundary_distance(0.0) == float("inf")
