"""ORACLE -- test infrastructure only.  NOT part of the product path.

fp64 references for ONE step of the KV-cache decode, each a plain restatement of what ``include/mgx.h`` promises for the
entry point it names (written from the header, not from the kernels).  CPU only, numpy / torch only.  Inputs are the exact
values the kernels read (bf16 / f32 tensors); every function widens them to fp64 first, so the only error left in a result
is fp64's own.

``tests/test_decode_ref.py`` ties these to what is already pinned to the reference project's goldens (``oracle.ref_cpu``);
``tests/test_gpu_decode_kernels.py`` compares the kernels with them element by element.
"""
from __future__ import annotations

import math

import numpy as np
import torch

F64 = torch.float64


def _d(t) -> torch.Tensor:
    return torch.as_tensor(t).to(F64)


# ---------------------------------------------------------------------------------------------------------------------
# embedding, projection, LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def embed(tok, table, pe, pos) -> torch.Tensor:
    """mgx_decode_embed: table[tok] * sqrt(d) + pe[pos], fp64 [rows, d].  ``pos``: one int or one per row."""
    tok = torch.as_tensor(tok).long().reshape(-1)
    pos = torch.as_tensor(pos).long().reshape(-1).expand(tok.numel()) if torch.as_tensor(pos).numel() == 1 \
        else torch.as_tensor(pos).long().reshape(-1)
    d = table.shape[1]
    return _d(table)[tok] * math.sqrt(d) + _d(pe)[pos]


def linear(a, w, bias=None, act=0):
    """mgx_linear_fwd and its decode-size forms: act(a @ w^T + bias) in fp64 -> (c [M,N], S [M,N]) with
    S = sum_k |a_k w_k|, the quantity the classical bound of an fp32 accumulation is stated in."""
    a, w = _d(a), _d(w)
    c = a @ w.T
    if bias is not None:
        c = c + _d(bias)
    if act == 1:
        c = torch.relu(c)
    return c, a.abs() @ w.abs().T


def add_ln(x, res, gamma, beta, eps=1e-6) -> torch.Tensor:
    """LayerNorm(x + res) * gamma + beta over the last dimension (biased variance, centred two-pass form), fp64"""
    z = _d(x) + _d(res)
    mean = z.mean(-1, keepdim=True)
    var = ((z - mean) ** 2).mean(-1, keepdim=True)
    return (z - mean) / torch.sqrt(var + eps) * _d(gamma) + _d(beta)


# ---------------------------------------------------------------------------------------------------------------------
# attention of one decode step
# ---------------------------------------------------------------------------------------------------------------------
def rel_attn_decode(q, K, V, E, t, M=None, *, fp32_reversed=False) -> torch.Tensor:
    """mgx_rel_attn_decode for (b, head)s that share one position t:
        ctx = softmax_j((q.k_j + q.E[M-1-(t-j)]) / 8) v_j,   j = 0..t
    q [..., 64], K / V [..., >= t+1, 64] (row t already holds this step's k_t / v_t), E [M, 64].  fp64.
    ``fp32_reversed``: the same formula in fp32 with the keys taken in reverse order -- not a reference but a second,
    differently ordered fp32 evaluation whose distance from the fp64 value is the fp32 noise floor of the formula itself."""
    M = E.shape[0] if M is None else M
    dt = torch.float32 if fp32_reversed else F64
    q, K, V = (torch.as_tensor(x).to(dt) for x in (q, K[..., :t + 1, :], V[..., :t + 1, :]))
    Er = torch.as_tensor(E).to(dt)[M - 1 - t:M]                         # row j of this slice is E[M-1-(t-j)]
    if fp32_reversed:
        K, V, Er = K.flip(-2), V.flip(-2), Er.flip(-2)
    s = (torch.einsum("...jd,...d->...j", K, q) + torch.einsum("jd,...d->...j", Er, q)) / 8.0
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return torch.einsum("...j,...jd->...d", p, V) / p.sum(-1, keepdim=True)


def attn_noise_floor(q, K, V, E, t, ref, M=None) -> torch.Tensor:
    """F: max over a head's 64 outputs of |fp32 reversed-order evaluation - fp64 reference| -> [...]"""
    return (rel_attn_decode(q, K, V, E, t, M, fp32_reversed=True).to(F64) - ref).abs().amax(-1)


# ---------------------------------------------------------------------------------------------------------------------
# the 8-bit cache (ABI 20): OCP e4m3fn codes, one f32 scale per row of 64
# ---------------------------------------------------------------------------------------------------------------------
def quant_twin(x):
    """torch twin of the cache's quantizer (include/mgx.h): x [..., 64] -> (codes uint8 [..., 64], scales f32 [...]); inv is
    an IEEE f32 division (``448.0 / t`` would be t.reciprocal() * 448)"""
    xf = x.float()
    amax = xf.abs().amax(-1)
    zero = amax == 0
    inv = torch.tensor(448.0, device=amax.device) / torch.where(zero, torch.ones_like(amax), amax)
    codes = (xf * inv[..., None]).to(torch.float8_e4m3fn).view(torch.uint8).clone()
    codes[zero] = 0
    return codes, amax / 448.0


def dequant(codes, scale):
    return codes.view(torch.float8_e4m3fn).float() * scale[..., None].float()


def dequant64(codes, scale) -> torch.Tensor:
    """float(code) * scale without the fp32 rounding of the product (4 + 24 significant bits)"""
    return codes.view(torch.float8_e4m3fn).to(F64) * scale[..., None].to(F64)


# ---------------------------------------------------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------------------------------------------------
def allowed_mask(allow_table, prev, V) -> np.ndarray:
    """bool [rows, V]: bit v of grammar row prev[r] (prev clamped to 0..V-1, as the header's 'token next_tok holds')"""
    tab = np.asarray(allow_table).astype(np.uint32).reshape(V, (V + 31) // 32)
    prev = np.clip(np.asarray(prev).astype(np.int64), 0, V - 1)
    v = np.arange(V)
    return ((tab[prev][:, v >> 5] >> (v & 31).astype(np.uint32)) & 1).astype(bool)


def softmax_probs(logits, temperature, allowed=None, dtype=np.float64) -> np.ndarray:
    """softmax(logits / temperature) per row in fp64, logits [rows, V] (the V real columns only).  ``allowed`` bool [rows, V]:
    disallowed logits are -inf; a row that is left without a finite logit (the grammar row is empty, or allows only tokens
    whose logit is -inf) falls back to the unmasked logits.  ``dtype=np.float32``: the same formula in fp32 throughout -- not a
    reference, a second evaluation whose distance from the fp64 one is what fp32 does to the formula."""
    x = np.asarray(_d(logits)).astype(dtype) * dtype(dtype(1.0) / dtype(temperature))
    if allowed is not None:
        xm = np.where(allowed, x, dtype(-np.inf))
        dead = ~np.isfinite(xm.max(-1))
        x = np.where(dead[:, None], x, xm)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True, dtype=dtype)


def kept_set(p, top_k, top_p) -> np.ndarray:
    """bool [V]: the ids mgx_sample_topk_topp may draw from, by the header's definition.  top-k: {p >= tau_k} for the largest
    tau_k with count(p >= tau_k) >= top_k (top_k <= 0 or >= V: all).  Then top-p: {p >= tau} for the largest tau with
    mass(p >= tau) >= top_p * mass(p >= tau_k) (top_p >= 1: no further cut).  Values equal to a threshold are all kept: ties
    stay together.  Ids of probability 0 are never drawn and are left out."""
    p = np.asarray(p, dtype=np.float64)
    V = p.shape[0]
    keep = p > 0
    vals = np.unique(p)[::-1]                                              # distinct values, descending
    if 0 < top_k < V:
        tau = next(v for v in vals if (p >= v).sum() >= top_k)
        keep &= p >= tau
    if top_p < 1:
        need = top_p * p[keep].sum()
        tau = next((v for v in vals if p[keep & (p >= v)].sum() >= need), 0.0)
        keep &= p >= tau
    return keep


def _hash32(x):
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def u01_bits(seed, step, row) -> np.ndarray:
    """the 24-bit integer n of the draw: u = (n + 0.5) / 2^24 (integer twin of the sampler's counter-based hash)"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    step = np.asarray(step, dtype=np.uint64) & 0xFFFFFFFF
    row = np.asarray(row, dtype=np.uint64) & 0xFFFFFFFF
    x = (np.uint64(seed & 0xFFFFFFFF) ^ _hash32((step * 0x9E3779B9 + 0x7F4A7C15) & 0xFFFFFFFF)
         ^ _hash32((row + 0x85EBCA6B) & 0xFFFFFFFF) ^ _hash32(((seed >> 32) + 0xC2B2AE35) & 0xFFFFFFFF))
    return _hash32(x) >> 8


def u01(seed, step, row) -> np.ndarray:
    """u, a pure function of (seed, step, row): (n + 0.5) / 2^24 with the sum taken in fp32 as the sampler takes it.  For
    n < 2^23 that is exact; above, n + 0.5 needs 25 bits and rounds to the even neighbour, so u is a multiple of 2^-24 there
    (and 1.0 for the single value n = 2^24 - 1, where the draw falls through to the last kept id).  Returned as fp64."""
    n = u01_bits(seed, step, row).astype(np.float32)
    return ((n + np.float32(0.5)) * np.float32(1.0 / 16777216.0)).astype(np.float64)


def draw(p_kept, u) -> int:
    """first id, in id order, with p > 0 whose inclusive CDF reaches u * total"""
    p_kept = np.asarray(p_kept, dtype=np.float64)
    cdf = np.cumsum(p_kept)
    hit = np.nonzero((p_kept > 0) & (cdf >= u * cdf[-1]))[0]
    return int(hit[0]) if hit.size else int(np.nonzero(p_kept > 0)[0][-1])


def kept_set_rows(p, top_k, top_p):
    """kept_set for every row of p [B, V] at once -> (keep bool [B, V], info).  info holds what a caller needs to tell how close
    a row's decisions were: ``tau_k`` [B] (0 without top-k), ``mass`` [B] = mass(p >= tau_k), and ``gap`` [B] = the smallest
    |mass(p >= v) - top_p * mass| over the distinct values v >= tau_k (inf without top-p)."""
    p = np.asarray(p, dtype=np.float64)
    B, V = p.shape
    ps = -np.sort(-p, axis=1)                                              # descending
    keep = p > 0
    tau_k = ps[:, top_k - 1].copy() if 0 < top_k < V else np.zeros(B)
    keep &= p >= tau_k[:, None]
    in_k = ps >= tau_k[:, None]
    cum = np.cumsum(np.where(in_k, ps, 0.0), axis=1)
    mass = cum[:, -1].copy()
    gap = np.full(B, np.inf)
    if top_p < 1:
        need = top_p * mass
        last = np.ones((B, V), dtype=bool)                                 # last member of its group of equal values
        last[:, :-1] = ps[:, :-1] != ps[:, 1:]
        G = np.where(last, cum, np.inf)
        G = np.minimum.accumulate(G[:, ::-1], axis=1)[:, ::-1]             # mass(p >= ps[i]): the whole tie group counts
        first = (G >= need[:, None]).argmax(1)
        keep &= p >= ps[np.arange(B), first][:, None]
        gap = np.where(in_k, np.abs(G - need[:, None]), np.inf).min(1)
    return keep, {"tau_k": tau_k, "mass": mass, "gap": gap}


def kept_set_alternatives(p, top_k, top_p, r, band):
    """every kept set a sampler may arrive at for ONE row when each probability it sees is off by at most r (relative) and each
    mass it compares by at most ``band`` (absolute): a list of bool [V] masks, kept_set(p, top_k, top_p) among them"""
    p = np.asarray(p, dtype=np.float64)
    V = p.shape[0]
    vals = np.unique(p[p > 0])[::-1]
    if 0 < top_k < V:
        ref = next((v for v in vals if (p >= v).sum() >= top_k), 0.0)
        taus_k = [v for v in vals if abs(v - ref) <= r * ref] or [ref]
    else:
        taus_k = [0.0]
    out = []
    for tk in taus_k:
        k1 = (p > 0) & (p >= tk)
        if top_p >= 1:
            out.append(k1)
            continue
        need = top_p * p[k1].sum()
        above = 0.0                                                        # mass of the values above v
        for v in vals[vals >= tk]:
            at = p[k1 & (p >= v)].sum()
            if at >= need - band and above < need + band:
                out.append(k1 & (p >= v))
            above = at
    return out
