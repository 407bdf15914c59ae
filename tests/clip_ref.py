"""fp64 references of the gradient-clipping contract of include/mgx.h (mgx_grad_norm, mgx_adam_step_clipped), written from the
header and used by tests/test_clip_args.py (against torch.nn.utils.clip_grad_norm_ on the CPU) and the GPU tests.

  norm  = sqrt(sum g[i]^2) * |gscale|                 every square and the sum in fp64; the sum here is math.fsum: EXACT, rounded once
  coef  = min(1, max_norm / (norm + 1e-6))            torch's clip_grad_norm_
  scale = (float32)(gscale * coef)                    rounded once
  a non-finite norm (some g[i] is +-inf or NaN)  ->  the step is skipped: scale = 0

gscale and max_norm cross the C ABI as fp32, so both are rounded to fp32 first."""
import math

import numpy as np

EPS = 1e-6


def f32(x) -> float:
    """x as the fp32 the C ABI passes, held in a Python float (fp64)"""
    return float(np.float32(x))


def sum_squares(g) -> float:
    g = np.asarray(g, dtype=np.float32).astype(np.float64).reshape(-1)
    if not np.isfinite(g).all():
        return float(np.sum(g * g))          # +inf or NaN: fsum raises on some of these
    return math.fsum(g * g)                  # the products are exact in fp64; fsum adds them exactly


def norm(g, gscale=1.0) -> float:
    return math.sqrt(sum_squares(g)) * abs(f32(gscale))


def coef_raw(nrm: float, max_norm) -> float:
    """max_norm / (norm + 1e-6) before the clamp at 1"""
    m = f32(max_norm)
    return m / (nrm + EPS) if math.isfinite(m) else float("inf")


def coef(nrm: float, max_norm) -> float:
    return min(1.0, coef_raw(nrm, max_norm))


def step(g, gscale, max_norm, nrm=None) -> dict:
    """what one mgx_grad_norm call leaves: {"norm", "coef", "scale" (np.float32), "skipped", "clipped"}; nrm: norm(g, gscale) where
    the caller has it already"""
    nrm = norm(g, gscale) if nrm is None else nrm
    if not math.isfinite(nrm):
        return {"norm": nrm, "coef": None, "scale": np.float32(0.0), "skipped": True, "clipped": False}
    c = coef(nrm, max_norm)
    return {"norm": nrm, "coef": c, "scale": np.float32(np.float64(f32(gscale)) * np.float64(c)), "skipped": False, "clipped": c < 1.0}


def f32_boundary_distance(x: float) -> float:
    """relative distance of the fp64 value x from the nearest point where its rounding to fp32 changes (the midpoints between
    x's fp32 neighbours); inf for x = 0"""
    if x == 0.0:
        return float("inf")
    r = np.float32(x)
    lo, hi = np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf))
    mids = ((float(r) + float(lo)) / 2.0, (float(r) + float(hi)) / 2.0)
    return min(abs(x - m) for m in mids) / abs(x)
