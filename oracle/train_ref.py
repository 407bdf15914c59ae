"""ORACLE -- test infrastructure only.  NOT part of the product path.

fp64 references for the training kernels of ``csrc/rowwise_ops.hip`` (embedding + PE, residual + LayerNorm, smoothed cross
entropy, Adam, bf16 cast, pad bitmap) and ``csrc/gru_train.hip`` (GRU cell, fused steps, bf16 dropout, row scatter), each a
plain restatement of what ``include/mgx.h`` promises for the entry point it names and of the closed formula in the kernel's
comment.  CPU only, numpy / torch only.  Inputs are the exact values the kernels read (bf16 / f32 tensors); every function
widens them to fp64 first, so the only error left in a result is fp64's own.  Scalars a kernel receives as ``float`` (eps,
betas, lr, p_drop) are taken at their fp32 value.

Noise floors.  Every formula can also be evaluated in fp32 with its sums taken in reverse order (``fp32_reversed=True``):
not a reference but a second, differently ordered fp32 evaluation.  Its distance from the fp64 value, plus one fp32 ulp of
the result, is the floor F of a family.  Two refinements, so that F says what fp32 does to the formula and not what one
lucky element did:
  * the ulp is taken at the largest addend of the result's last sum (``scale``): where the addends cancel the result's own
    ulp says nothing about the rounding the sum has already suffered;
  * for the row-wise families (LayerNorm, CE, embedding, GRU cell) F is the maximum over the row, as
    ``decode_ref.attn_noise_floor`` takes it over a head's 64 outputs: single elements of a second fp32 evaluation land on
    the fp64 value by chance.
  * the LayerNorm forward is checked in stages (``add_ln_out``): its output against the formula on the mean / rstd it saved.
For sums over rows or tokens (dgamma, dbeta, dxsum, dtable, stats[0], scatter) the floor is 2^-24 * sum |terms| (+ that ulp).

The dropout mask is a pure integer function of (seed, element index): ``make_drop`` / ``hash32`` / ``drop_mult8`` are its
integer twin and return the exact multiplier (0 or the fp32 constant ``scale``) of every element.

The training attention (``csrc/rel_attn_*.hip``) has its references here too: ``rel_attn_fwd`` / ``rel_attn_bwd``, the per-element
bounds ``attn_fwd_bounds`` / ``attn_weights_bound`` / ``attn_bwd_bounds`` and the seeded inputs of ``tests/test_gpu_attn_kernels.py``
(Gaussian, far, the two selectors with an exact answer, the pad patterns), each asserting its preconditions from the reference.

``tests/test_train_ref.py`` ties these to independent fp64 computations (torch's own layer_norm / GRUCell / Adam / autograd,
``oracle.ref_cpu.smooth_ce``); ``tests/test_gpu_rowwise_kernels.py`` and ``tests/test_gpu_gru_kernels.py`` compare the
kernels with them element by element.
"""
from __future__ import annotations

import math

import numpy as np
import torch

F64 = torch.float64
F32 = torch.float32
BF = torch.bfloat16
EPS32 = 2.0 ** -24
M32 = 0xFFFFFFFF


def _d(t) -> torch.Tensor:
    return torch.as_tensor(t).to(F64)


def _f32(v) -> float:
    """the value a C ``float`` parameter holds"""
    return float(np.float32(v))


def ulp32(x) -> torch.Tensor:
    """one fp32 ulp at |x| (never zero: the smallest subnormal at 0), as fp64"""
    a = torch.clamp(_d(x).abs(), max=1e38).to(F32)
    return torch.nextafter(a, torch.full_like(a, float("inf"))).to(F64) - a.to(F64)


def bf16_round(t) -> torch.Tensor:
    """the bf16 value (RNE) of an fp32-representable quantity, as fp64"""
    return torch.as_tensor(t).to(F32).to(BF).to(F64)


def sum_floor(terms, dim, ref) -> torch.Tensor:
    """floor of an fp32 sum over ``dim``: 2^-24 * sum |terms| + one ulp of the result"""
    return EPS32 * _d(terms).abs().sum(dim) + ulp32(ref)


# ---------------------------------------------------------------------------------------------------------------------
# dropout: integer twin of make_drop / hash32 / drop_mult8 (csrc/mgx_common.hpp)
# ---------------------------------------------------------------------------------------------------------------------
def make_drop(p, seed):
    """-> (thr16, mix, scale): drop iff a 16-bit random < thr16; scale = fp32(1 / (1 - thr16 / 65536))"""
    p = _f32(p)
    if p <= 0.0:
        return 0, 0, np.float32(1.0)
    thr = min(int(p * 65536.0 + 0.5), 65535)
    scale = np.float32(1.0 / (1.0 - thr / 65536.0))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = seed & M32, seed >> 32
    mix = (lo * 0x9E3779B9 + (hi ^ 0x85EBCA6B) * 0xC2B2AE35 + 0x27D4EB2F) & M32
    return thr, mix, scale


def hash32(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & M32
    x = x ^ (x >> 16)
    return x


def drop_mult8(cfg, g) -> np.ndarray:
    """multipliers of the 8 consecutive elements of every group in g (g = element index // 8, taken mod 2^32) -> f32 [len(g), 8]"""
    thr, mix, scale = cfg
    g = np.asarray(g, dtype=np.uint64).reshape(-1) & M32
    out = np.empty((g.size, 8), dtype=np.float32)
    for k in range(4):
        r = hash32(((g * 4 + k) & M32) ^ mix)
        out[:, 2 * k] = np.where((r & 0xFFFF) < thr, np.float32(0), scale)
        out[:, 2 * k + 1] = np.where((r >> 16) < thr, np.float32(0), scale)
    return out


def drop_mult(p, seed, n, chunk=1 << 22) -> torch.Tensor:
    """the multiplier of elements 0..n-1 (n % 8 == 0) of a buffer -> f32 tensor [n]"""
    assert n % 8 == 0
    cfg = make_drop(p, seed)
    if cfg[0] == 0:
        return torch.ones(n, dtype=F32)
    out = np.empty(n, dtype=np.float32)
    for g0 in range(0, n // 8, chunk):
        g1 = min(n // 8, g0 + chunk)
        out[8 * g0:8 * g1] = drop_mult8(cfg, np.arange(g0, g1, dtype=np.uint64)).reshape(-1)
    return torch.from_numpy(out)


def _mult(mult, like, dt):
    return torch.ones((), dtype=dt) if mult is None else torch.as_tensor(mult).to(dt).reshape(like.shape)


# ---------------------------------------------------------------------------------------------------------------------
# K6: residual + LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def add_ln_fwd(x, res, gamma, beta, eps, mult=None, *, fp32_reversed=False):
    """mgx_add_ln_fwd: z = x * mult + res; mean, rstd = 1 / sqrt(biased var + eps) (centred two-pass form); out = (z - mean)
    * rstd * gamma + beta -> (mean [rows], rstd [rows], out [rows, d])"""
    dt = F32 if fp32_reversed else F64
    x, res, gamma, beta = (torch.as_tensor(t).to(dt) for t in (x, res, gamma, beta))
    m = _mult(mult, x, dt)
    z = x * m + res
    if fp32_reversed:
        z, gamma, beta = z.flip(-1), gamma.flip(-1), beta.flip(-1)
    d = z.shape[-1]
    mean = z.sum(-1, keepdim=True) / d
    c = z - mean
    rstd = 1.0 / torch.sqrt((c * c).sum(-1, keepdim=True) / d + torch.tensor(_f32(eps), dtype=dt))
    out = c * rstd * gamma + beta
    if fp32_reversed:
        out = out.flip(-1)
    return mean[:, 0], rstd[:, 0], out


def add_ln_out(x, res, gamma, beta, mean, rstd, mult=None, *, fp32=False):
    """the last stage of mgx_add_ln_fwd on the mean / rstd the call SAVED: out = (x * mult + res - mean) * rstd * gamma + beta.
    The saved mean is an fp32 value, up to an ulp from the true one, and on a row far from zero that ulp, times rstd * |gamma|,
    is most of the distance between out and the fp64 LayerNorm; checked in stages -- mean and rstd against fp64, out against
    this -- no bound has to carry it."""
    dt = F32 if fp32 else F64
    x, res, gamma, beta, mean, rstd = (torch.as_tensor(t).to(dt) for t in (x, res, gamma, beta, mean, rstd))
    return (x * _mult(mult, x, dt) + res - mean[:, None]) * rstd[:, None] * gamma + beta


def add_ln_fwd_floor(x, res, gamma, beta, eps, mult, ref):
    """-> (F_mean, F_rstd), each [rows]"""
    mean, rstd, _ = ref
    m32, r32, _ = add_ln_fwd(x, res, gamma, beta, eps, mult, fp32_reversed=True)
    z = _d(x) * _mult(mult, _d(x), F64) + _d(res)
    return (m32.to(F64) - mean).abs() + ulp32(z.abs().mean(-1)), (r32.to(F64) - rstd).abs() + ulp32(rstd)


def add_ln_out_floor(x, res, gamma, beta, mean, rstd, mult, ref):
    """-> F [rows] of add_ln_out"""
    o32 = add_ln_out(x, res, gamma, beta, mean, rstd, mult, fp32=True)
    scale = ((ref - _d(beta)).abs() + _d(beta).abs()).amax(-1)
    return (o32.to(F64) - ref).abs().amax(-1) + ulp32(scale)


def add_ln_bwd(dout, x, res, gamma, mean, rstd, mult=None, *, fp32_reversed=False):
    """mgx_add_ln_bwd, with the mean / rstd the call is GIVEN (they are inputs of the backward): xhat = (x * mult + res - mean)
    * rstd, g = dout * gamma, dres = rstd * (g - mean(g) - xhat * mean(g * xhat)), dx = dres * mult; the column sums dgamma =
    sum dout * xhat, dbeta = sum dout, dxsum = sum dx (of the unrounded dx: the kernel sums its bf16 dx, tests compare that with
    the sum of the dx it wrote) -> (dres, dx, dgamma, dbeta, dxsum)"""
    dt = F32 if fp32_reversed else F64
    dout, x, res, gamma, mean, rstd = (torch.as_tensor(t).to(dt) for t in (dout, x, res, gamma, mean, rstd))
    m = _mult(mult, x, dt)
    xh = (x * m + res - mean[:, None]) * rstd[:, None]
    g = dout * gamma
    d = x.shape[-1]
    if fp32_reversed:
        c1, c2 = g.flip(-1).sum(-1, keepdim=True) / d, (g * xh).flip(-1).sum(-1, keepdim=True) / d
    else:
        c1, c2 = g.sum(-1, keepdim=True) / d, (g * xh).sum(-1, keepdim=True) / d
    dres = rstd[:, None] * (g - c1 - xh * c2)
    dx = dres * m
    rows = (lambda t: t.flip(0)) if fp32_reversed else (lambda t: t)
    return dres, dx, rows(dout * xh).sum(0), rows(dout).sum(0), rows(dx).sum(0)


def add_ln_bwd_floor(dout, x, res, gamma, mean, rstd, mult, ref):
    """-> (F_row [rows] for dres and dx, F_dgamma [d], F_dbeta [d])"""
    dres, dx, dgamma, dbeta, _ = ref
    r32 = add_ln_bwd(dout, x, res, gamma, mean, rstd, mult, fp32_reversed=True)
    m = _mult(mult, _d(x), F64)
    xh = (_d(x) * m + _d(res) - _d(mean)[:, None]) * _d(rstd)[:, None]
    g = _d(dout) * _d(gamma)
    d = xh.shape[-1]
    scale = _d(rstd) * (g.abs().amax(-1) + g.sum(-1).abs() / d + (xh.abs() * ((g * xh).sum(-1, keepdim=True).abs() / d)).amax(-1))
    scale = scale * m.abs().amax().clamp(min=1.0)
    f_row = torch.maximum((r32[0].to(F64) - dres).abs().amax(-1), (r32[1].to(F64) - dx).abs().amax(-1)) + ulp32(scale)
    return f_row, sum_floor(_d(dout) * xh, 0, dgamma), sum_floor(dout, 0, dbeta)


# ---------------------------------------------------------------------------------------------------------------------
# K9 + K10: label-smoothed cross entropy, arg-max, accuracy
# ---------------------------------------------------------------------------------------------------------------------
def smooth_ce_fwd(logits, target, V, eps_ls, pad, *, fp32_reversed=False):
    """mgx_smooth_ce_fwd on the V real columns: lse [rows]; arg-max [rows] (the FIRST index of the maximum); per-row loss =
    lse - (1 - eps) x_t - (eps / V) sum_v x_v; stats [4] = (sum of loss over target != pad, #target != pad,
    #(argmax == target) over ALL rows, rows) -> (lse, argmax int64, stats, loss)"""
    dt = F32 if fp32_reversed else F64
    x = torch.as_tensor(logits)[:, :V].to(dt)
    t = torch.as_tensor(target).long()
    rows = x.shape[0]
    am = torch.from_numpy(np.argmax(x.to(F64).numpy(), axis=1))            # numpy: first occurrence
    inside = (t >= 0) & (t < V)
    xt = torch.where(inside, x[torch.arange(rows), t.clamp(0, V - 1)], torch.zeros((), dtype=dt))
    if fp32_reversed:
        x = x.flip(-1)
    mx = x.amax(-1)
    lse = mx + torch.log(torch.exp(x - mx[:, None]).sum(-1))
    e = torch.tensor(_f32(eps_ls), dtype=dt)
    loss = lse - (1.0 - e) * xt - (e / V) * x.sum(-1)
    keep = t != pad
    stats = torch.stack([(loss.flip(0) if fp32_reversed else loss)[keep.flip(0) if fp32_reversed else keep].sum().to(F64),
                         keep.sum().to(F64), (am == t).sum().to(F64), torch.tensor(float(rows), dtype=F64)])
    return lse, am, stats, loss


def smooth_ce_fwd_floor(logits, target, V, eps_ls, pad, ref):
    """-> (F_lse [rows], F_loss_sum scalar)"""
    lse, _, stats, _ = ref
    l32, _, _, _ = smooth_ce_fwd(logits, target, V, eps_ls, pad, fp32_reversed=True)
    x = _d(torch.as_tensor(logits)[:, :V])
    t = torch.as_tensor(target).long()
    inside = (t >= 0) & (t < V)
    xt = torch.where(inside, x[torch.arange(x.shape[0]), t.clamp(0, V - 1)], torch.zeros((), dtype=F64))
    e = _f32(eps_ls)
    terms = (lse.abs() + (1.0 - e) * xt.abs() + (e / V) * x.abs().sum(-1))[t != pad]
    return (l32.to(F64) - lse).abs() + ulp32(torch.maximum(lse.abs(), x.abs().amax(-1))), EPS32 * terms.sum() + ulp32(stats[0])


def smooth_ce_bwd(logits, target, cnt, row_lse, V, ld, eps_ls, pad, g, *, fp32=False):
    """mgx_smooth_ce_bwd with the lse and the count the call is GIVEN: dlogits [rows, ld] = g / cnt * (exp(x - lse) - eps / V
    - (1 - eps) [v == target]) on the V real columns of the rows with target != pad, 0 everywhere else (an all-pad batch, cnt =
    0, is all zeros)"""
    dt = F32 if fp32 else F64
    x = torch.as_tensor(logits)[:, :V].to(dt)
    t = torch.as_tensor(target).long()
    rows = x.shape[0]
    out = torch.zeros(rows, ld, dtype=dt)
    keep = t != pad
    if float(cnt) == 0.0 or not bool(keep.any()):
        return out
    e = torch.tensor(_f32(eps_ls), dtype=dt)
    sc = torch.tensor(g, dtype=dt) / torch.tensor(float(cnt), dtype=dt)
    onehot = (torch.arange(V)[None, :] == t[:, None]).to(dt)
    grad = sc * (torch.exp(x - torch.as_tensor(row_lse).to(dt)[:, None]) - e / V - onehot * (1.0 - e))
    out[:, :V] = torch.where(keep[:, None], grad, torch.zeros((), dtype=dt))
    return out


def smooth_ce_bwd_floor(logits, target, cnt, row_lse, V, ld, eps_ls, pad, g, ref):
    """-> F [rows]"""
    g32 = smooth_ce_bwd(logits, target, cnt, row_lse, V, ld, eps_ls, pad, g, fp32=True)
    if float(cnt) == 0.0:
        return ulp32(torch.zeros(ref.shape[0], dtype=F64))
    x = _d(torch.as_tensor(logits)[:, :V])
    scale = abs(g / float(cnt)) * (torch.exp(x - _d(row_lse)[:, None]).amax(-1) + 1.0)
    return (g32.to(F64) - ref).abs().amax(-1) + ulp32(scale)


# ---------------------------------------------------------------------------------------------------------------------
# K11: Adam
# ---------------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, gscale=1.0, *, fp32=False):
    """mgx_adam_step = torch.optim.Adam's update on g * gscale: m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
    p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps) -> (p, m, v, upd) with upd the subtracted term"""
    dt = F32 if fp32 else F64
    p, g, m, v = (torch.as_tensor(t).to(dt) for t in (p, g, m, v))
    S = (lambda a: torch.tensor(_f32(a), dtype=dt))
    lr, b1, b2, eps, gs = S(lr), S(beta1), S(beta2), S(eps), S(gscale)
    gk = g * gs
    m = b1 * m + (1.0 - b1) * gk
    v = b2 * v + (1.0 - b2) * gk * gk
    bc1 = 1.0 - b1 ** step
    bc2s = torch.sqrt(1.0 - b2 ** step)
    upd = (lr / bc1) * m / (torch.sqrt(v) / bc2s + eps)
    return p - upd, m, v, upd


def adam_floor(p, g, m, v, lr, beta1, beta2, eps, step, gscale, ref):
    """-> (F_p, F_m, F_v) per element"""
    r32 = adam_step(p, g, m, v, lr, beta1, beta2, eps, step, gscale, fp32=True)
    gk = _d(g) * _f32(gscale)
    b1, b2 = _f32(beta1), _f32(beta2)
    return ((r32[0].to(F64) - ref[0]).abs() + ulp32(torch.maximum(_d(p).abs(), ref[3].abs())),
            (r32[1].to(F64) - ref[1]).abs() + ulp32(torch.maximum(b1 * _d(m).abs(), (1 - b1) * gk.abs())),
            (r32[2].to(F64) - ref[2]).abs() + ulp32(torch.maximum(b2 * _d(v).abs(), (1 - b2) * gk * gk)))


# ---------------------------------------------------------------------------------------------------------------------
# K1: embedding * sqrt(d) + PE, and its backward; the row scatter
# ---------------------------------------------------------------------------------------------------------------------
def embed_pe_fwd(tok, table, pe, L, mult=None, *, fp32=False):
    """mgx_embed_pe_fwd: out[r] = (table[tok[r]] * sqrt(d) + pe[r % L]) * mult[r] -> [rows, d]"""
    dt = F32 if fp32 else F64
    tok = torch.as_tensor(tok).long().reshape(-1)
    d = table.shape[1]
    s = torch.tensor(_f32(math.sqrt(d)) if fp32 else math.sqrt(d), dtype=dt)
    out = torch.as_tensor(table).to(dt)[tok] * s + torch.as_tensor(pe).to(dt)[torch.arange(tok.numel()) % L]
    return out * _mult(mult, out, dt)


def embed_pe_fwd_floor(tok, table, pe, L, mult, ref):
    """-> F [rows]"""
    tok = torch.as_tensor(tok).long().reshape(-1)
    d = table.shape[1]
    o32 = embed_pe_fwd(tok, table, pe, L, mult, fp32=True)
    scale = (_d(table)[tok].abs() * math.sqrt(d) + _d(pe)[torch.arange(tok.numel()) % L].abs()).amax(-1)
    scale = scale * _mult(mult, ref, F64).abs().amax().clamp(min=1.0)
    return (o32.to(F64) - ref).abs().amax(-1) + ulp32(scale)


def scatter_add_rows(idx, src, V, cols):
    """mgx_scatter_add_rows: update [V, cols] with row idx[r] += src[r, :cols]; indices outside [0, V) are ignored
    -> (update, sum of |terms|)"""
    idx = torch.as_tensor(idx).long().reshape(-1)
    s = _d(src)[:, :cols]
    ok = (idx >= 0) & (idx < V)
    upd = torch.zeros(V, cols, dtype=F64).index_add_(0, idx[ok], s[ok])
    return upd, torch.zeros(V, cols, dtype=F64).index_add_(0, idx[ok], s[ok].abs())


def embed_bwd(tok, dout, V, mult=None):
    """mgx_embed_bwd: update of dtable [V, d] = sqrt(d) * sum_{r: tok[r] == v} mult[r] * dout[r] -> (update, sum of |terms|)"""
    dout = _d(dout).reshape(-1, dout.shape[-1])
    d = dout.shape[1]
    upd, S = scatter_add_rows(torch.as_tensor(tok).reshape(-1), dout * _mult(mult, dout, F64), V, d)
    return upd * math.sqrt(d), S * math.sqrt(d)


# ---------------------------------------------------------------------------------------------------------------------
# K13b: GRU cell (torch.nn.GRU, gate order r, z, n) and the projections of the fused steps
# ---------------------------------------------------------------------------------------------------------------------
def _gates(gi, gh, dt):
    gi, gh = torch.as_tensor(gi).to(dt), torch.as_tensor(gh).to(dt)
    H = gi.shape[-1] // 3
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    hn = gh[:, 2 * H:]
    n = torch.tanh(gi[:, 2 * H:] + r * hn)
    return r, z, n, hn


def gru_cell_fwd(gi, gh, h_prev, *, fp32=False):
    """mgx_gru_cell_fwd: r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h -> h' [B, H]"""
    dt = F32 if fp32 else F64
    r, z, n, _ = _gates(gi, gh, dt)
    return (1.0 - z) * n + z * torch.as_tensor(h_prev).to(dt)


def gru_cell_fwd_floor(gi, gh, h_prev, ref):
    """-> F [B]"""
    _, z, n, _ = _gates(gi, gh, F64)
    scale = torch.maximum(((1 - z) * n).abs(), (z * _d(h_prev)).abs()).amax(-1)
    return (gru_cell_fwd(gi, gh, h_prev, fp32=True).to(F64) - ref).abs().amax(-1) + ulp32(scale)


def gru_cell_coef(gi, gh, h_prev):
    """the coefficients of dh in the cell backward: dgi = dgh = dh * (c_r, c_z, c_n) except dgh_n = dh * c_n * r;
    dh_prev_direct = dh * z -> dict of fp64 [B, H]"""
    r, z, n, hn = _gates(gi, gh, F64)
    c_n = (1 - z) * (1 - n * n)
    return {"r": c_n * hn * r * (1 - r), "z": (_d(h_prev) - n) * z * (1 - z), "n": c_n, "nr": c_n * r, "h": z}


def gru_cell_bwd(gi, gh, h_prev, dh, *, fp32=False):
    """mgx_gru_cell_bwd for a given total dh (= dh_direct + d_rec + dy, each optional) -> (dgi [B, 3H], dgh [B, 3H],
    dh_prev_direct [B, H])"""
    dt = F32 if fp32 else F64
    r, z, n, hn = _gates(gi, gh, dt)
    dh = torch.as_tensor(dh).to(dt)
    dn = dh * (1.0 - z) * (1.0 - n * n)
    dz = dh * (torch.as_tensor(h_prev).to(dt) - n) * z * (1.0 - z)
    dr = dn * hn * r * (1.0 - r)
    return torch.cat([dr, dz, dn], 1), torch.cat([dr, dz, dn * r], 1), dh * z


def gru_cell_bwd_floor(gi, gh, h_prev, dh, ref):
    """-> F [B], one floor for the three outputs of a batch row"""
    r32 = gru_cell_bwd(gi, gh, h_prev, dh, fp32=True)
    f = torch.stack([(a.to(F64) - b).abs().amax(-1) for a, b in zip(r32, ref)]).amax(0)
    return f + ulp32(torch.stack([b.abs().amax(-1) for b in ref]).amax(0))


def proj(a, w, bias=None):
    """a [M, K] @ w [N, K]^T + bias in fp64 -> (c [M, N], S = sum_k |a_k w_k| + |bias|): the recurrent and input projections of
    the fused steps (gh = h_bf16 W_hh^T + b_hh, gi = x W_ih^T + b_ih) and, with w = W_hh^T, d_rec = dgh_next W_hh.  mgx.h rounds
    each of them to bf16 before the cell reads it: ``bf16_round``."""
    a, w = _d(a), _d(w)
    c, S = a @ w.T, a.abs() @ w.abs().T
    if bias is not None:
        c, S = c + _d(bias), S + _d(bias).abs()
    return c, S


def relu(v) -> torch.Tensor:
    """max(v, 0) that keeps a NaN a NaN (IEEE 754-2019 maximum); -0 and -inf give +0"""
    v = _d(v)
    return torch.where(v > 0, v, torch.where(torch.isnan(v), v, torch.zeros((), dtype=F64)))


def linear_fwd(a, w, bias=None, act=0):
    """mgx_linear_fwd before its one rounding: act(a [M, K] @ w [N, K]^T + bias) in fp64 -> (v [M, N], S = sum_k |a_k w_k| +
    |bias|).  The kernel's output is ``bf16_round(v)`` (mgx.h: bias and ReLU in fp32, then one RNE rounding)."""
    c, S = proj(a, w, bias)
    return (relu(c) if act else c), S


def linear_dx(dy, w, relu_y=None, addend=None):
    """mgx_linear_dx: p = dy [M, N] @ w [N, K] in fp64, unrounded, S = sum_n |dy_n w_n|, and the value mgx.h promises for p:
    the product rounded to bf16, zeroed where not relu_y > 0 (an IEEE comparison: NaN and -0 zero it), the addend added in fp32,
    rounded once more -> (p, S, final).  ``final`` is the kernel's output to the bit wherever p and the sum are
    fp32-representable (integer data); otherwise the tests bound the distance from ``masked p + addend``."""
    p, S = proj(dy, _d(w).T)
    v = bf16_round(p)
    if relu_y is not None:
        v = torch.where(_d(relu_y) > 0, v, torch.zeros((), dtype=F64))
    if addend is not None:
        v = bf16_round(v + _d(addend))
    return p, S, v


def linear_dw(dy, x, gw0=None, gb0=None):
    """mgx_linear_dw / mgx_linear_dw_grouped: gW [N, K] = gw0 + dy [M, N]^T @ x [M, K], gb [N] = gb0 + column sums of dy, in fp64
    -> (gW, gb, S_W, S_b) with S the sum of |terms|, |gw0| / |gb0| included"""
    dy, x = _d(dy), _d(x)
    gW, SW = dy.T @ x, dy.abs().T @ x.abs()
    gb, Sb = dy.sum(0), dy.abs().sum(0)
    if gw0 is not None:
        gW, SW = gW + _d(gw0), SW + _d(gw0).abs()
    if gb0 is not None:
        gb, Sb = gb + _d(gb0), Sb + _d(gb0).abs()
    return gW, gb, SW, Sb


def on_bf16_tie(v) -> torch.Tensor:
    """where an fp32-representable value lies exactly half way between two bf16 values (the low 16 bits of its fp32 image are
    0x8000): RNE and every other rounding rule differ there"""
    v = _d(v)
    f = v.to(F32)
    assert (f.to(F64) == v)[torch.isfinite(v)].all(), "not fp32-representable"
    return (f.view(torch.int32) & 0xFFFF) == 0x8000


def dw_mchunk(M, tiles, target):
    """Python twin of dw_mchunk (csrc/linear_tile128.hip): rows per M-split of the 128 x 128 weight-gradient kernels"""
    splits = (target + tiles - 1) // tiles
    return ((M + splits - 1) // splits + 63) // 64 * 64


def dw_tile_plan(M, shapes, grouped):
    """-> (mchunk, exact path?, reduction tiles per split nm) of mgx_linear_dw (one weight, ``grouped`` False) or of the grouped
    128 x 128 kernel for weights [(N, K), ..]: target 256 workgroups below 32 tiles, 384 from there, 480 for a group"""
    tiles = sum(((N + 127) // 128) * ((K + 127) // 128) for N, K in shapes)
    mchunk = dw_mchunk(M, tiles, 480 if grouped else (384 if tiles >= 32 else 256))
    return mchunk, M % mchunk == 0, (min(M, mchunk) + 63) // 64


def proj_floor(a, w, bias, ref, S):
    """fp32 product with the reduction reversed against fp64, + 2^-24 S (the classical unit of an fp32 accumulation)"""
    a32, w32 = torch.as_tensor(a).to(F32).flip(-1), torch.as_tensor(w).to(F32).flip(-1)
    c32 = a32 @ w32.T
    if bias is not None:
        c32 = c32 + torch.as_tensor(bias).to(F32)
    return (c32.to(F64) - ref).abs() + EPS32 * S + ulp32(ref)


# ---------------------------------------------------------------------------------------------------------------------
# inputs the GPU tests build (on the CPU, so that tests/test_train_ref.py can assert their preconditions without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
LN_KINDS = ("zero-mean", "far", "const", "scales")


def ln_case(kind, rows, d, seed=0):
    """x, res bf16 [rows, d] of one LayerNorm case:
      zero-mean  x, res ~ N(0, 1)
      far        rows far from zero: x is a per-row offset of 16 .. 60 (an integer: exact in bf16), res a detail of std 0.25
                 whose elements below 2^-10 are zero, so that x + res, and 2 x + res (dropout at p = 0.5), are exact in fp32
                 (7 + 17 bits)
      const      every row a constant (variance 0: rstd = 1 / sqrt(eps), out = beta)
      scales     rows of very different scale in one call: row r is N(0, 1) * 2^(-12 + 3 (r % 9))"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * rows + d)
    rn = lambda *s: torch.randn(*s, generator=g)                                                    # noqa: E731
    if kind == "zero-mean":
        x, res = rn(rows, d), rn(rows, d)
    elif kind == "far":
        off = torch.randint(16, 61, (rows, 1), generator=g).float() * torch.where(torch.arange(rows)[:, None] % 2 == 0, 1.0, -1.0)
        x = off.expand(rows, d).clone()
        res = (0.25 * rn(rows, d)).to(BF).float()
        res = torch.where(res.abs() < 2.0 ** -10, torch.zeros(()), res)
    elif kind == "const":
        c = torch.randint(-40, 41, (rows, 1), generator=g).float() * 0.25
        x, res = c.expand(rows, d).clone(), torch.zeros(rows, d)
    elif kind == "scales":
        s = 2.0 ** (-12.0 + 3.0 * (torch.arange(rows) % 9).float())[:, None]
        x, res = rn(rows, d) * s, rn(rows, d) * s
    else:
        raise ValueError(kind)
    return x.to(BF), res.to(BF)


def ce_logits(kind, rows, V, ld, seed=0, fill=0.0):
    """logits bf16 [rows, ld]; columns >= V hold ``fill`` (NaN / +inf in the padding tests):
      gauss   N(0, 2)            pm80    every logit +80 or -80            equal   all-equal rows (arg-max 0)
      last    N(0, 1) with the row maximum in column V - 1"""
    g = torch.Generator().manual_seed(1000 * seed + 13 * rows + V)
    if kind == "gauss":
        x = 2.0 * torch.randn(rows, V, generator=g)
    elif kind == "pm80":
        x = torch.where(torch.rand(rows, V, generator=g) < 0.5, 80.0, -80.0)
    elif kind == "equal":
        x = torch.randint(-3, 4, (rows, 1), generator=g).float().expand(rows, V).clone()
    elif kind == "last":
        x = torch.randn(rows, V, generator=g)
        x[:, V - 1] = 6.0
    else:
        raise ValueError(kind)
    out = torch.full((rows, ld), float(fill))
    out[:, :V] = x
    return out.to(BF)


def ce_targets(rows, V, pad, seed=0):
    """random targets with the edge columns planted in the first rows: 0, V - 1, 511, 512 (where they exist) and ``pad``"""
    g = torch.Generator().manual_seed(seed + rows + V)
    t = torch.randint(0, V, (rows,), generator=g)
    plant = [0, V - 1, pad] + [c for c in (511, 512) if c < V]
    for i, c in enumerate(plant[:rows]):
        t[i] = c
    if rows > 8:
        t[torch.rand(rows, generator=g) < 0.1] = pad
    return t.to(torch.int32)


# ---- the training GEMMs (tests/test_gpu_gemm_kernels.py) ------------------------------------------------------------------------
GEMM_KINDS = ("exact", "gauss", "far")
EXACT_OPERAND, EXACT_BIAS, EXACT_ADDEND, EXACT_GRAD = 7, 2000, 128, 1000      # magnitudes of the integer data


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) % (2 ** 31))


def _ints(g, lim, *shape):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def gemm_operands(kind, M, N, R, seed=0):
    """a [M, R], b [N, R] (both reduction-contiguous; bf16) of one product c[m, n] = sum_r a[m, r] b[n, r]:
      exact  integers of magnitude <= 7 (exact in bf16; any partial sum in any order is an integer below 2^24 as long as S is:
             fp32 accumulation is then exact whatever its order).  Planted (R >= 6): a[0] = 7 on r < 6, else 0; b[0] = 7 on r < 5,
             6 at r = 5 -> c[0, 0] = 287, between the bf16 neighbours 286 and 288: a tie, and >= 256
      gauss  a ~ N(0, 1), b ~ N(0, 1 / R)
      far    rows far from zero: a[m] = an offset of +-16 .. 60 plus N(0, 1/16); b[n] = u_n * (+1, -1, +1, ..) plus N(0, 1/400),
             so the offsets cancel in the sum and S >> |c|"""
    g = _gen(M, N, R, seed, GEMM_KINDS.index(kind))
    if kind == "exact":
        a, b = _ints(g, EXACT_OPERAND, M, R), _ints(g, EXACT_OPERAND, N, R)
        if R >= 6:
            a[0], b[0] = 0.0, 0.0
            a[0, :6], b[0, :5], b[0, 5] = 7.0, 7.0, 6.0
    elif kind == "gauss":
        a, b = torch.randn(M, R, generator=g), torch.randn(N, R, generator=g) / R ** 0.5
    elif kind == "far":
        off = torch.randint(16, 61, (M, 1), generator=g).float() * torch.where(torch.arange(M)[:, None] % 2 == 0, 1.0, -1.0)
        a = off + 0.25 * torch.randn(M, R, generator=g)
        alt = torch.where(torch.arange(R) % 2 == 0, 1.0, -1.0)
        b = torch.randn(N, 1, generator=g) * alt + 0.05 * torch.randn(N, R, generator=g)
    else:
        raise ValueError(kind)
    return a.to(BF), b.to(BF)


def gemm_bias(kind, N, seed=0):
    """f32 [N]: integers of magnitude <= 2000 (0 in column 0, which holds the planted tie), or N(0, 1)"""
    g = _gen(N, seed, 11)
    if kind == "exact":
        b = _ints(g, EXACT_BIAS, N)
        b[0] = 0.0
        return b
    return torch.randn(N, generator=g)


def gemm_addend(kind, M, K, seed=0):
    """bf16 [M, K]: integers of magnitude <= 128 (1 at [0, 0]: the planted 287 rounds to 288 and 288 + 1 is a tie again), or N(0, 1)"""
    g = _gen(M, K, seed, 12)
    if kind == "exact":
        a = _ints(g, EXACT_ADDEND, M, K)
        a[0, 0] = 1.0
        return a.to(BF)
    return torch.randn(M, K, generator=g).to(BF)


def gemm_grad0(kind, *shape, seed=0):
    """f32 start value of a gW / gb slot: integers of magnitude <= 1000, or N(0, 1)"""
    g = _gen(*shape, seed, 13)
    return _ints(g, EXACT_GRAD, *shape) if kind == "exact" else torch.randn(*shape, generator=g)


MASK_SPECIALS = (0x0000, 0x8000, 0x0001, 0x0080, 0xBC00, 0x7F80, 0xFF80, 0x7FC0, 0xFFC0)
MASK_KEPT = (False, False, True, True, False, True, False, False, False)


def relu_mask(M, K, seed=0):
    """bf16 [M, K] mask operand of mgx_linear_dx: N(0, 1) with a quarter of the elements exactly +0 (what a ReLU really leaves),
    [0, 0] = 1 (the planted tie is kept) and, from [0, 1] on, MASK_SPECIALS: +0, -0, the smallest subnormal, the smallest
    normal, a small negative, +inf, -inf, NaN of both signs (K >= 16; kept iff > 0 as an IEEE comparison: MASK_KEPT)"""
    g = _gen(M, K, seed, 14)
    y = torch.randn(M, K, generator=g)
    y = torch.where(torch.rand(M, K, generator=g) < 0.25, torch.zeros(()), y).to(BF)
    y[0, 0] = 1.0
    if K >= 16:
        y.view(torch.int16)[0, 1:1 + len(MASK_SPECIALS)] = torch.tensor(MASK_SPECIALS, dtype=torch.int32).to(torch.int16)
    return y


# ---------------------------------------------------------------------------------------------------------------------
# K3 + K4: the training attention (tests/test_gpu_attn_kernels.py)
# ---------------------------------------------------------------------------------------------------------------------
TINY = 2.0 ** -124                                  # fp32 / bf16 underflow: a result below the smallest normal 2^-126 may be flushed to 0; four such steps
U_BF = 2.0 ** -8                                    # unit roundoff of bf16 (8 significant bits) under RNE (pack_bf16x2): 1 + 2^-8 rounds to 1


class Ref(dict):
    """a dict whose entries read and write as attributes; hashed and compared by identity (a key of a cache)"""
    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    __setattr__ = dict.__setitem__
    __hash__ = object.__hash__
    __eq__ = object.__eq__


def _attn_operands(qkv, E, heads, M):
    """-> qs = q / 8, k, v [B, h, L, 64]; Eg [L, L, 64] with Eg[i, j] = Er[i - j] = E[M - 1 - (i - j)] for j <= i and 0 above the
    diagonal; low [L, L] = (j <= i)"""
    qkv, E = _d(qkv), _d(E)
    B, L, d3 = qkv.shape
    d = d3 // 3
    assert d == 64 * heads and tuple(E.shape) == (M, 64) and M >= L
    hd = lambda t: t.reshape(B, L, heads, 64).permute(0, 2, 1, 3)                                    # noqa: E731
    i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
    low = j <= i
    Er = E[M - L:].flip(0)
    Eg = Er[(i - j).clamp(min=0)] * low[..., None]
    return hd(qkv[..., :d]) / 8.0, hd(qkv[..., d:2 * d]), hd(qkv[..., 2 * d:]), Eg, low


def _merge(t):
    """[B, h, L, 64] -> [B, L, h * 64]"""
    B, h, L, c = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, L, h * c)


def _heads(t, heads):
    B, L = t.shape[:2]
    return _d(t).reshape(B, L, heads, 64).permute(0, 2, 1, 3)


def _attn_logits(qkv, E, pad_mask, heads, M, causal, Lk):
    qs, k, v, Eg, low = _attn_operands(qkv, E, heads, M)
    B, L = qs.shape[0], qs.shape[2]
    S = qs @ k.transpose(-1, -2) + torch.einsum("bhic,ijc->bhij", qs, Eg)
    A = qs.abs() @ k.abs().transpose(-1, -2) + torch.einsum("bhic,ijc->bhij", qs.abs(), Eg.abs())
    # R: what the logit's rounding is proportional to.  Every kernel forms it from eight MFMA instructions of 16 columns each, D = C +
    # sum of 16 exact products, 17 addends in an order of the hardware's own: at most 17 2^-24 (sum |products| + |C|) each.  Over the
    # instructions the sums of |products| add up to A; the C operands are the partial sums of the relative term over 16, 32, 48 columns
    # (pE), of the content term likewise (pK), and -- where the four K instructions continue the accumulator of the four Er ones
    # (forward, dK/dV, recompute dQ) -- the whole relative term SE four times; the recompute dE kernel adds two chains: |S| once
    SE = torch.einsum("bhic,ijc->bhij", qs, Eg)
    R = A + 4 * SE.abs() + S.abs()
    for c in (16, 32, 48):
        R = R + (qs[..., :c] @ k[..., :c].transpose(-1, -2)).abs() + torch.einsum("bhic,ijc->bhij", qs[..., :c], Eg[..., :c]).abs()
    A = Ref(A=A, R=R)
    if causal:
        assert Lk is None
        vis = low[None, None].expand(B, 1, L, L)
        if pad_mask is not None:
            vis = vis & ~torch.as_tensor(pad_mask).bool()[:, None, None, :]
    else:
        assert pad_mask is None
        vis = (torch.arange(L) < (L if Lk is None else Lk))[None, None, None, :].expand(B, 1, L, L)
    assert vis.any(-1).all(), "a row without a visible key is outside the contract"
    return qs, k, v, Eg, S, A, vis


def rel_attn_fwd(qkv, E, pad_mask, heads, M, causal=True, Lk=None):
    """mgx_rel_attn_fwd (causal: keys j <= i that are not padded; pad_mask bool [B, L], True = padded key) and
    mgx_rel_attn_fwd_nomask (causal=False: keys j < Lk, the relative term for j <= i only), per (b, h) in fp64:
      S [B, h, L, L]  qs_i . k_j + qs_i . Er[i - j], qs = q / 8 (unmasked values)      vis  the visible (i, j)
      lse [B, h, L]   log sum_visible exp S          P = exp(S - lse) on visible, 0 elsewhere      ctx [B, L, d] = P v
      A [B, h, L, L]  sum_c |qs_ic| (|k_jc| + |Er[i - j]_c|); R: A + the |C| operands of the eight MFMAs (_attn_logits)                           PV [B, L, d] = sum_j P_ij |v_jc|
      V1 [B, L, d]    sum over the visible j of |v_jc| (the weight of an underflowed P)"""
    qs, k, v, Eg, S, AR, vis = _attn_logits(qkv, E, pad_mask, heads, M, causal, Lk)
    A, R = AR.A, AR.R
    Sm = torch.where(vis, S, torch.full((), -float("inf"), dtype=F64))
    lse = torch.logsumexp(Sm, -1)
    P = torch.exp(Sm - lse[..., None])
    return Ref(S=S, vis=vis, lse=lse, P=P, ctx=_merge(P @ v), A=A, R=R, PV=_merge(P @ v.abs()), V1=_merge(vis.to(F64) @ v.abs()), L=S.shape[-1])


def attn_weights(ref, lse_in):
    """mgx_rel_attn_weights on the lse it is handed: exp(S - lse_in) on visible entries, 0 elsewhere -> [B, h, L, L]"""
    return torch.where(ref.vis, torch.exp(ref.S - _d(lse_in)[..., None]), torch.zeros((), dtype=F64))


def _skew_sum(W, X):
    """sum_{b, h, i} W[b, h, i, i - dl] X[b, h, i, c] -> [L, 64] by relative distance dl (W is zero above the diagonal)"""
    L = W.shape[-1]
    i, dl = torch.arange(L)[:, None], torch.arange(L)[None, :]
    Wk = torch.gather(W, -1, (i - dl).clamp(min=0).expand(W.shape)) * (dl <= i)
    return torch.einsum("bhid,bhic->dc", Wk, X)


def rel_attn_bwd(qkv, E, pad_mask, ctx_in, lse_in, dctx, heads, M, causal=True, Lk=None):
    """mgx_rel_attn_bwd / _parts: the formula block of csrc/rel_attn_bwd.hip on the values the kernels are HANDED -- ctx_in and
    lse_in are inputs and are not recomputed:
      P = exp(S - lse_in) on visible entries     dP = dO v^T     delta = rowsum(dO o ctx_in)     dS = P o (dP - delta)
      dq = (sum_j dS_ij (k_j + Er[i - j])) / 8    dk_j = sum_i dS_ij qs_i    dv_j = sum_i P_ij dO_i    dEr[dl] = sum_{b,h,i} dS[i, i - dl] qs_i
    -> dqkv [B, L, 3d], dE [M, 64] (the UPDATE: rows < M - L are zero), and what the bounds need: S, A, P, dS, dP - delta (dPd),
    qs, k, Eg, dO per head, DV[i, j] = sum_c |dO_ic| |v_jc|, DC[i] = sum_c |dO_ic| |ctx_in_ic|"""
    qs, k, v, Eg, S, AR, vis = _attn_logits(qkv, E, pad_mask, heads, M, causal, Lk)     # (causal=False: the CPU tie alone)
    A, R = AR.A, AR.R
    L = S.shape[-1]
    dO, O = _heads(dctx, heads), _heads(ctx_in, heads)
    lse_in = _d(lse_in)
    P = torch.where(vis, torch.exp(S - lse_in[..., None]), torch.zeros((), dtype=F64))
    dPd = dO @ v.transpose(-1, -2) - (dO * O).sum(-1, keepdim=True)
    dS = P * dPd
    dq = (dS @ k + torch.einsum("bhij,ijc->bhic", dS, Eg)) / 8.0
    dk, dv = dS.transpose(-1, -2) @ qs, P.transpose(-1, -2) @ dO
    dE = torch.zeros(M, 64, dtype=F64)
    dE[M - L:] = _skew_sum(dS, qs).flip(0)
    return Ref(dqkv=torch.cat([_merge(dq), _merge(dk), _merge(dv)], -1), dE=dE, S=S, A=A, R=R, P=P, dS=dS, dPd=dPd, qs=qs, k=k, Eg=Eg, dO=dO, vis=vis,
               lse=lse_in, DV=dO.abs() @ v.abs().transpose(-1, -2), DC=(dO.abs() * O.abs()).sum(-1), L=L, M=M)


LOGIT_U = 17 * EPS32                                # per MFMA instruction: 17 addends (16 exact bf16 products and C), any order


def attn_eps(R, S, lse, vis_or_P):
    """the relative error of P_ij as the kernels form it: eps_ij = expm1(17 2^-24 R_ij + 2^-22 (|S_ij| + |lse_i|)) + 2^-21, 0 on
    entries that are not visible (R: _attn_logits; tests/test_gpu_attn_kernels.py derives the rest)"""
    e = torch.expm1(LOGIT_U * R + 2.0 ** -22 * (S.abs() + lse.abs()[..., None])) + 2.0 ** -21
    return torch.where(vis_or_P, e, torch.zeros((), dtype=F64))


def attn_fwd_bounds(ref):
    """-> per-element bounds (ctx [B, L, d], lse [B, h, L], eps [B, h, L, L]) of the forward"""
    L = ref.L
    eps = attn_eps(ref.R, ref.S, ref.lse, ref.vis)
    eps_i = eps.amax(-1)                                                     # [B, h, L]
    rel = U_BF + 2 * eps_i + (L + 2) * EPS32
    rel = rel[..., None].expand(*eps_i.shape, 64)
    ctx = 2.0 ** -8 * ref.ctx.abs() + (1 + 2.0 ** -8) * (_merge(rel) * ref.PV + TINY * ref.V1)
    # lse: log-sum-exp moves by a weighted mean of the logits' errors (mean value theorem), the weights a softmax at a point between
    # the exact and the computed logits: within exp(2 max error) of P.  The row sum l is added up five deep inside a tile (exp_tile's
    # four chains), once per tile, once across the lane halves, and is rescaled: L / 32 + 8 roundings.  __logf and the last add: 2 ulp
    Rv = torch.where(ref.vis, ref.R, torch.zeros((), dtype=F64))
    lse = LOGIT_U * (ref.P * Rv).sum(-1) * torch.exp(2 * LOGIT_U * Rv.amax(-1)) + (L // 32 + 8) * EPS32 + 2 * ulp32(ref.lse)
    return ctx, lse, eps


def attn_weights_bound(ref, lse_in, W):
    return (attn_eps(ref.R, ref.S, _d(lse_in), ref.vis) + 2.0 ** -23) * W + TINY * ref.vis


def attn_bwd_bounds(r, B_total, dE0=None):
    """-> per-element bounds (dqkv [B, L, 3d], dE [M, 64]) of the backward from its reference ``r``; dE0 the start value of dE"""
    L, M = r.L, r.M
    heads = r.qs.shape[1]
    eps = attn_eps(r.R, r.S, r.lse, r.P > 0)
    g = r.P * (eps * r.dPd.abs() + 66 * EPS32 * (r.DV + r.DC[..., None])) + U_BF * r.dS.abs() + TINY * r.vis * (r.dPd.abs() + 1)
    G = g + L * EPS32 * r.dS.abs()
    W = (eps + U_BF + L * EPS32) * r.P + TINY * r.vis
    bq = (G @ r.k.abs() + torch.einsum("bhij,ijc->bhic", G, r.Eg.abs())) / 8.0
    bk, bv = G.transpose(-1, -2) @ r.qs.abs(), W.transpose(-1, -2) @ r.dO.abs()
    b = 2.0 ** -8 * r.dqkv.abs() + (1 + 2.0 ** -8) * torch.cat([_merge(bq), _merge(bk), _merge(bv)], -1)
    start = torch.zeros(M, 64, dtype=F64) if dE0 is None else _d(dE0)
    bE = torch.zeros(M, 64, dtype=F64)
    bE[M - L:] = _skew_sum(g + B_total * heads * L * EPS32 * r.dS.abs(), r.qs.abs()).flip(0)
    bE[M - L:] += ulp32(torch.maximum(start.abs(), (start + r.dE).abs()))[M - L:]
    return b, bE


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
ATTN_PADS = ("none", "trailing", "interior", "tile", "second", "bits")


def attn_pads(name, B, L, seed=0):
    """bool [B, L] (True = padded key) or None.  Position 0 is always real, so every row sees a key.
      trailing  the last 1 .. L/2 keys of every batch row            interior  four single keys per row
      tile      a whole 32-key tile (keys 32 .. 63; at L = 32 the upper half of the only tile) of batch row 0, one key elsewhere
      second    every second key (1, 3, 5, ..)
      bits      bit 31 of a word (key 31, and key L - 1) and bit 0 of a word (key 32 and key L - 32, where L >= 64)"""
    if name == "none":
        return None
    g = _gen(B, L, seed, 21 + ATTN_PADS.index(name))
    m = torch.zeros(B, L, dtype=torch.bool)
    if name == "trailing":
        for b in range(B):
            m[b, L - int(torch.randint(1, L // 2 + 1, (1,), generator=g)):] = True
    elif name == "interior":
        for b in range(B):
            m[b, torch.randint(1, L, (4,), generator=g)] = True
    elif name == "tile":
        m[0, (32 if L >= 64 else 16):(64 if L >= 64 else 32)] = True
        m[1:, L // 2] = True
    elif name == "second":
        m[:, 1::2] = True
    elif name == "bits":
        m[:, 31] = True
        m[:, L - 1] = True
        if L >= 64:
            m[:, 32] = True
            m[:, L - 32] = True
    else:
        raise ValueError(name)
    assert not m[:, 0].any() and m.any()
    return m


def pack_padbits(mask):
    """the bitmap of mgx_pad_bitmap: int32 [B, L / 32] holding uint32 words, bit (j & 31) of word j >> 5 set iff key j is padded"""
    B, L = mask.shape
    w = (mask.reshape(B, L // 32, 32).numpy().astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return torch.from_numpy(w.view(np.int32).copy())


def attn_gauss(B, L, heads, M, seed=0):
    """the scales of tests/test_gpu_kernels.py: qkv 0.8, E 0.5, dctx 1.0, all bf16 -> (qkv, E, dctx)"""
    g = _gen(B, L, heads, M, seed, 31)
    d = 64 * heads
    return ((torch.randn(B, L, 3 * d, generator=g) * 0.8).to(BF), (torch.randn(M, 64, generator=g) * 0.5).to(BF),
            torch.randn(B, L, d, generator=g).to(BF))


def attn_far(B, L, heads, M, seed=0):
    """Gaussian data of scale 0.3 in which query row L - 20 of (batch row 0, head 0) is 4.0 in every column and so is key 40
    (L < 160) or 70 (key tile 1 or 2): that logit is 64 * 16 / 8 = 128 + the relative term.  The forward's lazy softmax reference
    then lags by far more than 40 nats when the sweep reaches that tile (its redo and rescale branch; the kernel's threshold is a
    tile sum of 1e24, 55.3 nats); at L >= 160 the tile lies in the branch-free main loop of the last query block.  Without pads.
    The jump is asserted from the reference -> (qkv, E, dctx, (i, j))"""
    assert L >= 96
    g = _gen(B, L, heads, M, seed, 32)
    d = 64 * heads
    qkv, E = (torch.randn(B, L, 3 * d, generator=g) * 0.3).to(BF), (torch.randn(M, 64, generator=g) * 0.3).to(BF)
    i, j = L - 20, (40 if L < 160 else 70)
    qkv[0, i, :64] = 4.0
    qkv[0, j, d:d + 64] = 4.0
    S = rel_attn_fwd(qkv, E, None, heads, M).S[0, 0, i]
    t = j // 32
    assert t >= 1 and 32 * (t + 1) <= (i // 128) * 128 or L < 160
    jump = (S[32 * t:32 * t + 32].max() - S[:32 * t].max()).item()
    assert jump > 60.0 and S[j] == S[:i + 1].max(), jump
    return qkv, E, torch.randn(B, L, d, generator=g).to(BF), (i, j)


SEL_MARGIN = 256.0                                   # nats: exp2(-256 log2 e) = 2^-369 is 0 in fp32 (smallest subnormal 2^-149)
SEL_REL_DELTAS = (0, 1, 31, 32, 33, 127, 128, -1)    # -1 stands for L - 1


def _small_ints(g, lim, *shape):
    """non-zero-mean small integers of magnitude <= lim"""
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def _selector_check(qkv, E, dctx, pad_mask, heads, M, sel, rows, causal=True, Lk=None):
    """from the reference alone: on the rows ``rows`` [B, L] the softmax is one-hot on key sel [B, L] by SEL_MARGIN nats; the values
    and the sums of the exact answer are integers that bf16 / fp32 hold exactly -> the exact answer (ctx, dv) as fp64"""
    B, L = sel.shape
    d = 64 * heads
    ref = rel_attn_fwd(qkv, E, pad_mask, heads, M, causal, Lk)
    Sm = torch.where(ref.vis, ref.S, torch.full((), -float("inf"), dtype=F64))
    top = Sm.gather(-1, sel[:, None, :, None].expand(B, heads, L, 1))[..., 0]
    rest = Sm.scatter(-1, sel[:, None, :, None].expand(B, heads, L, 1), -float("inf")).amax(-1)
    ok = rows[:, None, :].expand(B, heads, L)
    assert ok.any() and (top - rest)[ok].min() >= SEL_MARGIN, "the margin does not hold"
    v, dO = _d(qkv[..., 2 * d:]), _d(dctx)
    assert (v == v.round()).all() and (dO == dO.round()).all()
    ctx = torch.gather(v, 1, sel[..., None].expand(B, L, d))
    dv = torch.zeros(B, L, d, dtype=F64).scatter_add_(1, sel[..., None].expand(B, L, d), dO * rows[..., None])
    absum = torch.zeros(B, L, d, dtype=F64).scatter_add_(1, sel[..., None].expand(B, L, d), dO.abs() * rows[..., None])
    assert (bf16_round(dv) == dv).all() and absum.max() < 2 ** 8, "an integer sum is not exact in bf16"
    assert (dO.abs().sum(-1).max() * v.abs().max()) * 64 < 2 ** 24                      # delta, dP: exact in fp32 in any order
    real = torch.ones(B, L, dtype=torch.bool) if pad_mask is None else ~torch.as_tensor(pad_mask)
    if not causal:
        real = real & (torch.arange(L) < (Lk or L))[None, :]
    tiles = [(sel[rows] // 32 == t).any().item() for t in range(L // 32) if real[:, 32 * t:32 * t + 32].any()]
    return ref, ctx, dv, all(tiles)


def attn_selector_rel(B, L, heads, M, delta0, pad_mask, seed=0):
    """the RELATIVE selector: k = 0, q_i = 8 u for one fixed +-1 vector u, E zero except row M - 1 - delta0 = c u with c =
    4 (exact in bf16): S[i, i - delta0] = 64 c = 256 and every other logit is 0, so row i >= delta0 attends to key i - delta0 alone
    (unless that key is padded; rows i < delta0, and rows whose key is padded, attend uniformly and are held to the bounds alone).  v and dO are integers of magnitude <= 8 and <= 3.
    -> (qkv, E, dctx, sel [B, L], rows bool [B, L] = the rows with the exact answer, exact ctx, exact dv)"""
    g = _gen(B, L, heads, M, delta0, seed, 33)
    d = 64 * heads
    u = torch.where(torch.rand(64, generator=g) < 0.5, 1.0, -1.0)         # one E serves every head: one u
    qkv = torch.zeros(B, L, 3 * d)
    qkv[..., :d] = 8.0 * u.repeat(heads)
    qkv[..., 2 * d:] = _small_ints(g, 8, B, L, d)
    E = torch.zeros(M, 64)
    c = 4.0
    E[M - 1 - delta0] = c * u
    dctx = _small_ints(g, 3, B, L, d)
    i = torch.arange(L)[None, :].expand(B, L)
    sel = (i - delta0).clamp(min=0)
    rows = i >= delta0
    if pad_mask is not None:
        rows = rows & ~torch.gather(pad_mask, 1, sel)
    qkv, E, dctx = qkv.to(BF), E.to(BF), dctx.to(BF)
    assert E[M - 1 - delta0, 0].abs().item() == c
    ref, ctx, dv, _ = _selector_check(qkv, E, dctx, pad_mask, heads, M, sel, rows)
    return qkv, E, dctx, sel, rows, ctx, dv


def attn_code(idx):
    """+-1 [.., 64]: bit (c % 9) of the index decides column c, so two different indices below 512 differ in >= 7 columns"""
    bits = (torch.as_tensor(idx)[..., None] >> (torch.arange(64) % 9)) & 1
    return (1.0 - 2.0 * bits).float()


def attn_selector_content(B, L, heads, M, pad_mask, seed=0, causal=True, Lk=None):
    """the CONTENT selector: E = 0, k_j = c code(j) with c = 148 (exact in bf16), q_i = code(t(i)): S[i, j] = c (64 - 2 #differing
    columns) / 8 is 1184 at j = t(i) and at most 1184 - 259 elsewhere.  t(i) is a seeded choice among the real keys the row may see
    (j <= i; j < Lk without the causal mask) that also crosses tile and 128-row block boundaries; rows 32 t + 31 take a key of tile t,
    so that every tile that has a real key is selected.  Every row is one-hot: dq, dk and dE are exactly 0.
    -> (qkv, E, dctx, sel, rows (all True), exact ctx, exact dv)"""
    assert L < 512
    g = _gen(B, L, heads, M, seed, 34, int(causal), Lk or 0)
    d = 64 * heads
    c = 148.0
    real = torch.ones(B, L, dtype=torch.bool) if pad_mask is None else ~pad_mask
    sel = torch.zeros(B, L, dtype=torch.long)
    for b in range(B):
        for i in range(L):
            hi = (i + 1) if causal else (Lk or L)
            cand = torch.nonzero(real[b, :hi])[:, 0]
            if i % 32 == 31:
                own = cand[(cand >= i - 31) & (cand <= i)]
                cand = own if own.numel() else cand
            sel[b, i] = cand[int(torch.randint(0, cand.numel(), (1,), generator=g))]
    qkv = torch.zeros(B, L, 3 * d)
    qkv[..., :d] = attn_code(sel).repeat(1, 1, heads)
    qkv[..., d:2 * d] = c * attn_code(torch.arange(L)).repeat(1, heads)
    qkv[..., 2 * d:] = _small_ints(g, 8, B, L, d)
    E, dctx = torch.zeros(M, 64), _small_ints(g, 3, B, L, d)
    qkv, E, dctx = qkv.to(BF), E.to(BF), dctx.to(BF)
    assert (qkv[0, 1, d:2 * d].float().abs() == c).all()
    rows = torch.ones(B, L, dtype=torch.bool)
    if not causal:
        rows = rows & (torch.arange(L) < (Lk or L))[None, :]
    ref, ctx, dv, every_tile = _selector_check(qkv, E, dctx, pad_mask, heads, M, sel, rows, causal, Lk)
    assert every_tile, "a key tile with a real key is never selected"
    if causal and L >= 160:
        assert ((sel // 128) < (torch.arange(L)[None, :] // 128)).any(), "no row selects a key of an earlier 128-row block"
    return qkv, E, dctx, sel, rows, ctx, dv
