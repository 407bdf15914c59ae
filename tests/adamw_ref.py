"""fp64 reference of mgx_adam_step_groups (include/mgx.h, K11c), written from the header on top of oracle.train_ref's Adam, and
the noise floors its outputs are held to.  Imported by basename, like clip_ref.

Per element of a 64-element chunk of group k, s = lr_scale[k], w = weight_decay[k] (all scalars as the fp32 the C ABI passes):
  s == 0 or k >= n_groups   frozen: p, m, v, ema keep their values
  else                      pd = p (1 - lr s w);  (p', m', v') = Adam(pd, g, m, v) at the rate f32(lr s);
                            ema' = d ema + (1 - d) p'

Floors (what fp32 arithmetic in the kernel's order may differ by from the fp64 value, before the constant C of the test):
  p    train_ref.adam_floor on pd at the rate lr s, plus -- where w > 0 -- one ulp of p: the rounding unit of the decay multiply
       (the product's own rounding, and the factor 1 - lr s w, which is rounded at 1)
  m, v train_ref.adam_floor unchanged
  ema  ulp(d ema) + ulp((1 - d) p') + ulp(ema'), the roundings of the two products and of the sum, plus (1 - d) times p's floor:
       the kernel averages the p it stored, not the reference's"""
import numpy as np
import torch

from oracle import train_ref as T

F64 = torch.float64
CHUNK = 64


def f32(x) -> float:
    return float(np.float32(x))


def element_groups(group_of, n):
    """the chunk table (one entry per 64 elements) -> the group of every element, int64 [n]"""
    return torch.as_tensor(group_of, dtype=torch.int64).repeat_interleave(CHUNK)[:n]


def step(p, g, m, v, ema, lr, beta1, beta2, eps, step_no, gscale, group_of, lr_scale, weight_decay, ema_decay):
    """-> {"p", "m", "v", "ema" (None without one), "F_p", "F_m", "F_v", "F_ema", "live" (bool [n]: not frozen)}, fp64 [n];
    frozen elements keep their inputs and carry a floor of one ulp (they are compared bit for bit elsewhere)"""
    p, g, m, v = (torch.as_tensor(t).to(F64).reshape(-1) for t in (p, g, m, v))
    n = p.numel()
    grp = element_groups(group_of, n)
    out = {"p": p.clone(), "m": m.clone(), "v": v.clone(), "F_p": T.ulp32(p), "F_m": T.ulp32(m), "F_v": T.ulp32(v)}
    live = torch.zeros(n, dtype=torch.bool)
    for k, (s, w) in enumerate(zip(lr_scale, weight_decay)):
        s, w = f32(s), f32(w)
        sel = grp == k
        if s == 0.0 or not sel.any():
            continue
        live |= sel
        rate = f32(f32(lr) * s)                                          # the product of two fp32 is exact in fp64: rounded once, as the kernel's
        pd = p[sel] * (1.0 - rate * w)
        r = T.adam_step(pd, g[sel], m[sel], v[sel], rate, beta1, beta2, eps, step_no, gscale)
        F = T.adam_floor(pd, g[sel], m[sel], v[sel], rate, beta1, beta2, eps, step_no, gscale, r)
        out["p"][sel], out["m"][sel], out["v"][sel] = r[0], r[1], r[2]
        out["F_p"][sel] = F[0] + (T.ulp32(p[sel]) if w > 0.0 else 0.0)
        out["F_m"][sel], out["F_v"][sel] = F[1], F[2]
    out["live"] = live
    out["ema"] = out["F_ema"] = None
    if ema is not None:
        e = torch.as_tensor(ema).to(F64).reshape(-1)
        d = f32(ema_decay)
        new = torch.where(live, d * e + (1.0 - d) * out["p"], e)
        out["ema"] = new
        out["F_ema"] = T.ulp32(d * e) + T.ulp32((1.0 - d) * out["p"]) + T.ulp32(new) + (1.0 - d) * out["F_p"]
    return out


def ema_recurrence(start, params, ema_decay, schedule):
    """the EMA after the recorded parameter vectors ``params`` (one per update, fp32-representable), from ``start``:
    e <- d_u e + (1 - d_u) p_u with d_u = f32(schedule(ema_decay, u)), in fp64 -> (ema, accumulated rounding floor of an fp32
    evaluation: three roundings per update, each carried on with weight <= 1)"""
    e = torch.as_tensor(start).to(F64)
    F = torch.zeros_like(e)
    for u, p in enumerate(params):
        d = f32(schedule(ema_decay, u))
        p = torch.as_tensor(p).to(F64)
        new = d * e + (1.0 - d) * p
        F = d * F + T.ulp32(d * e) + T.ulp32((1.0 - d) * p) + T.ulp32(new)
        e = new
    return e, F
