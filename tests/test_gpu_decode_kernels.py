"""The kernels of one KV-cache decode step, each against the fp64 reference of its header contract (oracle/decode_ref.py),
element by element, at the shapes and positions where such kernels go wrong: every split count of the attention and the
positions on either side of a share boundary, poisoned memory wherever the call must not look, fragment-ordered weights with
partial last tiles, LayerNorm rows far from zero, and the sampler's draw row by row.

No bound here is a max-norm bound and none was calibrated against another kernel.

Attention.  |ctx - ref| <= 2^-8 |ref| + C_ATTN * F per element: 2^-8 |ref| is the bf16 rounding of the output (half an ulp is
2^-9), F the fp32 noise floor of the reference formula itself (decode_ref.attn_noise_floor: the formula in fp32 with the keys
in reverse order, against fp64, maximum over the head's 64 outputs).  C_ATTN is the margin for the kernel's exp2 and merge
tree.  MEASURED on one MI355X over all cases of this module: the largest (|ctx - ref| - 2^-8 |ref|) / F was 6.11 (the
8-bit cache with every logit near -200; 5.62 for the bf16 cache, 1.17 on Gaussian data); C_ATTN = 16 is twice that, rounded
up to a power of two.

Sampler.  |probs_out - softmax_fp64| <= R_PROB * ref + 1e-12.  MEASURED: the largest relative error was 1.167e-6 = 2^-19.71
(the fast exp of arguments down to -30); R_PROB = 2^-18 is twice that rounded up to a power of two.  The drawn token must be
the reference's draw from the reference's probabilities and an integer twin of the hash.  A row is ambiguous, and may take
either side, when its draw or its kept set is decided within a band of a boundary: R_PROB for the comparison of two single
probabilities (top-k), and for a compared mass (a CDF prefix, the mass above a top-p threshold) the distance of an fp32
evaluation of the same softmax and prefix sums from the fp64 one, plus 32 * 2^-24 for the order of the sampler's own sums
(sampler_reference says why the mass band is not R_PROB * total).  At most 2 % of the rows of any case may be ambiguous,
asserted from the reference and the hash alone; measured: none in 74 of the 80 cases, 1.2 % at most (V = 1024).
"""
import math

import numpy as np
import pytest
import torch

import kernel_checks as KC
from kernel_checks import nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)
from oracle import decode_ref as D

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
NAN16 = 0x7FC0                                     # a bf16 NaN; as a byte pattern 0xFF.. is a NaN in f32 too

C_ATTN = 16.0
R_PROB = 2.0 ** -18
SEEN = {"c": 0.0, "r": 0.0}                        # the largest ratios this process has seen, printed by the tests


# =====================================================================================================================
# 1. attention
# =====================================================================================================================
# name: (B, d, Lmax, M - Lmax, key splits per (b, head))
ATTN_CONFIGS = {
    "one-short": (3, 192, 300, 16, 1),
    "one-long": (32, 2048, 1024, 0, 1),            # B * heads = 1024 workgroups: one of them walks the whole cache
    "two": (2, 64, 1500, 16, 2),                   # Lmax not a multiple of 64
    "four": (2, 192, 2048, 0, 4),
    "eight": (2, 512, 4096, 16, 8),
}
CFG5 = (32, 512, 8192, 0, 4)                       # the benchmarked decode: shares of 2048 keys


def positions(n, Lmax):
    """the positions of a configuration with n key splits: the first waves' slots, the 64-key stride, and both sides of every
    share boundary (t + 1 a multiple of 64 n: a split goes from empty to one key) for k = 1, 2 and the largest k"""
    ps = [0, 1, 7, 8, 9, 15, 16, 17, 62, 63, 64, 65, 127, 128, Lmax - 2, Lmax - 1]
    kmax = (Lmax - 1) // (64 * n)
    for k in {1, 2, kmax}:
        ps += [64 * n * k - 1, 64 * n * k, 64 * n * k + 1]
    return sorted({p for p in ps if 0 <= p < Lmax})


def ragged_batches(ps, B):
    """the positions as rows of batches of B, first against last: one batch holds t = 0 next to t = Lmax - 1"""
    order = [ps[i // 2] if i % 2 == 0 else ps[-1 - i // 2] for i in range(len(ps))]
    order += order[:(-len(order)) % B]
    return [order[i:i + B] for i in range(0, len(order), B)]


class AttnData:
    """caches, q/k/v of the step and E of one configuration, on the device and (the same values) on the CPU"""

    def __init__(self, cfg, fp8, kind="gauss", seed=0):
        self.B, self.d, self.Lmax, extra, self.nsplit = cfg
        self.h, self.M, self.fp8, self.kind = self.d // 64, self.Lmax + extra, fp8, kind
        B, h, Lmax, d = self.B, self.h, self.Lmax, self.d
        g = torch.Generator(device=DEV).manual_seed(1000 * seed + Lmax + B + (7 if fp8 else 0))
        rn = lambda *s: torch.randn(*s, device=DEV, generator=g)                                    # noqa: E731
        K = rn(B, h, Lmax, 64) * torch.exp(0.5 * rn(B, h, Lmax, 1))                 # rows of different magnitude
        V = rn(B, h, Lmax, 64) * torch.exp(0.5 * rn(B, h, Lmax, 1))
        qkv = rn(B, 3 * d)
        q = qkv[:, :d].reshape(B, h, 64)
        alpha = (8.0 * 90.0 / (q * q).sum(-1, keepdim=True))                        # (alpha q).q / 8 = 90
        if kind == "q0":
            qkv[:, :d] = 0
        elif kind == "dom-t":                                                       # the new key dominates
            qkv[:, d:2 * d] = (alpha * q).reshape(B, d)
        elif kind == "dom-0":
            K[:, :, 0] = alpha * q
        elif kind == "dom-last":                                                    # the last split holds the winner, split 0
            K[:, :, Lmax - 2] = alpha * q                                           # the runner-up
            K[:, :, 0] = 0.5 * alpha * q
        elif kind == "neg200":                                                      # every logit near -200
            qkv[:, :d] = 4.0
            qkv[:, d:2 * d] = -6.25 + 0.05 * rn(B, d)
            K = -6.25 + 0.05 * rn(B, h, Lmax, 64)
        self.qkv = qkv.to(BF)
        self.E = (0.3 * rn(self.M, 64)).to(BF)
        if fp8:
            (self.kc, self.ks), (self.vc, self.vs) = D.quant_twin(K.to(BF)), D.quant_twin(V.to(BF))
            self.cpu = [t.cpu() for t in (self.kc, self.ks, self.vc, self.vs)]
        else:
            self.kc, self.vc = K.to(BF), V.to(BF)
            self.cpu = [self.kc.cpu(), None, self.vc.cpu(), None]
        self.qkv_cpu, self.E_cpu = self.qkv.cpu(), self.E.cpu()
        ops = KC.ops()
        assert ops.rel_attn_decode_splits(B, Lmax, d) == self.nsplit, (cfg, ops.rel_attn_decode_splits(B, Lmax, d))
        self.ws = ops.rel_attn_decode_workspace(B, Lmax, d, DEV)
        assert (self.ws is None) == (self.nsplit == 1)

    def new_rows(self, dev):
        """this step's k_t, v_t per (b, head) as the cache holds them: bf16 rows, or (codes, scales)"""
        B, h, d = self.B, self.h, self.d
        k, v = self.qkv_cpu[:, d:2 * d].reshape(B, h, 64), self.qkv_cpu[:, 2 * d:].reshape(B, h, 64)
        # the quantizer's twin runs on the CPU (IEEE division; a device-side torch division by a scalar need not be one)
        rows = (D.quant_twin(k), D.quant_twin(v)) if self.fp8 else ((k, None), (v, None))
        return [tuple(None if x is None else x.to(DEV) for x in r) for r in rows] if dev else rows

    def rows64(self, b, t):
        """K, V of batch row b as the step at position t sees them: fp64 [h, t+1, 64], rows < t from the cache, row t new"""
        out = []
        (nk, nks), (nv, nvs) = self.new_rows(False)
        for cache, scale, new, nscale in ((self.cpu[0], self.cpu[1], nk, nks), (self.cpu[2], self.cpu[3], nv, nvs)):
            if self.fp8:
                old = D.dequant64(cache[b, :, :t], scale[b, :, :t])
                cur = D.dequant64(new[b], nscale[b])
            else:
                old, cur = cache[b, :, :t].double(), new[b].double()
            out.append(torch.cat([old, cur[:, None]], 1))
        return out

    def run(self, ts, ragged):
        """one call with every poison in place; returns ctx on the CPU after checking what the call wrote and left alone"""
        ops = KC.ops()
        B, h, Lmax, d, M = self.B, self.h, self.Lmax, self.d, self.M
        t_rows = torch.tensor(ts if ragged else [ts] * B, device=DEV)
        stale = (torch.arange(Lmax, device=DEV)[None] >= t_rows[:, None])[:, None]             # [B, 1, Lmax]: rows >= t
        (nk, nks), (nv, nvs) = self.new_rows(True)
        bidx = torch.arange(B, device=DEV)

        def poisoned(cache, scale, new, nscale):
            if self.fp8:
                c, s = cache.masked_fill(stale[..., None], 0x7F), scale.masked_fill(stale, float("nan"))
                want_c, want_s = c.clone(), s.clone()
                want_c[bidx, :, t_rows], want_s[bidx, :, t_rows] = new, nscale
                return c, s, want_c, want_s.view(torch.int32)
            c = cache.view(torch.int16).masked_fill(stale[..., None], NAN16).view(BF)
            want = c.clone()
            want[bidx, :, t_rows] = new
            return c, None, want.view(torch.int16), None

        kc, ks, want_kc, want_ks = poisoned(self.kc, self.ks if self.fp8 else None, nk, nks)
        vc, vs, want_vc, want_vs = poisoned(self.vc, self.vs if self.fp8 else None, nv, nvs)
        E = self.E.clone()
        E.view(torch.int16)[:M - 1 - int(t_rows.max())] = NAN16                                  # rows no key of this call maps to
        if self.ws is not None:
            self.ws.fill_(0xFF)                                                                 # every stale partial is NaN
        ctx = torch.full((B, d), float("nan"), dtype=BF, device=DEV)
        pos = t_rows.to(torch.int32) if ragged else t_rows[:1].to(torch.int32).contiguous()
        ops.rel_attn_decode(self.qkv, kc, vc, E, pos, ctx, self.ws, ragged=ragged, kscale=ks, vscale=vs)
        torch.cuda.synchronize()
        what = (self.kind, "fp8" if self.fp8 else "bf16", "ragged" if ragged else "uniform", ts)
        # row t is exactly this step's k / v (8-bit: exactly the quantizer's twin), every other row bit for bit what it was
        # (integer views: NaN != NaN)
        if self.fp8:
            assert torch.equal(kc, want_kc) and torch.equal(vc, want_vc), what
            assert torch.equal(ks.view(torch.int32), want_ks) and torch.equal(vs.view(torch.int32), want_vs), what
        else:
            assert torch.equal(kc.view(torch.int16), want_kc) and torch.equal(vc.view(torch.int16), want_vc), what
        return ctx.float().cpu()

    def check(self, ts, ragged):
        B, h = self.B, self.h
        ctx = self.run(ts, ragged).double().reshape(B, h, 64)
        what = (self.kind, "fp8" if self.fp8 else "bf16", "ragged" if ragged else "uniform")
        assert torch.isfinite(ctx).all(), (what, ts)
        q = self.qkv_cpu[:, :self.d].reshape(B, h, 64)
        for b in range(B):
            t = ts[b] if ragged else ts
            K, V = self.rows64(b, t)
            ref = D.rel_attn_decode(q[b], K, V, self.E_cpu, t)
            F = D.attn_noise_floor(q[b], K, V, self.E_cpu, t, ref)[:, None]
            err = (ctx[b] - ref).abs()
            over = (err - 2.0 ** -8 * ref.abs()).clamp(min=0)
            SEEN["c"] = max(SEEN["c"], float((over / F)[(F > 0).expand_as(over)].max()) if (F > 0).any() else 0.0)
            bad = err > 2.0 ** -8 * ref.abs() + C_ATTN * F
            assert not bad.any(), (what, "b", b, "t", t, "head, dim", bad.nonzero()[:4].tolist(), "err", err[bad][:4].tolist(),
                                   "ref", ref[bad][:4].tolist(), "F", F.flatten().tolist())


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("name", list(ATTN_CONFIGS))
def test_attention_at_every_split_count_and_share_boundary(name, fp8):
    """Gaussian data; the uniform entry point takes the positions one per call, the ragged one as rows of a few batches"""
    data = AttnData(ATTN_CONFIGS[name], fp8)
    ps = positions(data.nsplit, data.Lmax)
    n = data.nsplit
    assert {64 * n - 1, 64 * n, 64 * n + 1, data.Lmax - 1, 0} <= set(ps)
    for t in ps:
        data.check(t, ragged=False)
    batches = ragged_batches(ps, data.B)
    assert 0 in batches[0] and data.Lmax - 1 in batches[0]
    for ts in batches:
        data.check(ts, ragged=True)
    print(f"\n{name} fp8={fp8}: {len(ps)} positions, largest (err - 2^-8|ref|) / F so far {SEEN['c']:.3f}")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_attention_at_the_benchmarked_shape(fp8):
    """cfg5's own shape: batch 32, 8 heads, 8192 cache rows, 4 splits of 2048 keys -- one ragged batch over the positions and
    two uniform calls"""
    data = AttnData(CFG5, fp8)
    assert data.nsplit == 4 and ((data.Lmax + 3) // 4 + 63) // 64 * 64 == 2048
    ps = positions(4, data.Lmax)
    (ts,) = ragged_batches(ps, data.B)
    assert len(ps) <= data.B and 0 in ts and data.Lmax - 1 in ts
    data.check(ts, ragged=True)
    for t in (4 * 64 * 31, data.Lmax - 1):
        data.check(t, ragged=False)
    print(f"\ncfg5 shape fp8={fp8}: largest (err - 2^-8|ref|) / F so far {SEEN['c']:.3f}")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("kind", ["q0", "dom-t", "dom-0", "dom-last", "neg200"])
@pytest.mark.parametrize("name", ["one-short", "two", "four", "eight"])
def test_attention_value_cases(name, kind, fp8):
    """q = 0 (the plain mean of v_0..v_t); one key 60 or more above all others at j = t, at j = 0, and in the last split with
    the runner-up in split 0 (every rescale branch of the epilogue and of the merge); every logit near -200"""
    data = AttnData(ATTN_CONFIGS[name], fp8, kind, seed=1)
    B, h, d, Lmax = data.B, data.h, data.d, data.Lmax
    t = Lmax - 1
    # the case is what it claims to be, from the reference's own logits at t = Lmax - 1
    q = data.qkv_cpu[:, :d].reshape(B, h, 64).double()
    for b in range(B):
        K, V = data.rows64(b, t)
        s = (torch.einsum("hjd,hd->hj", K, q[b]) + torch.einsum("jd,hd->hj", data.E_cpu.double()[data.M - 1 - t:], q[b])) / 8
        top = s.topk(2, -1)
        if kind == "q0":
            assert (s == 0).all() and (D.rel_attn_decode(q[b], K, V, data.E_cpu, t) - V.mean(1)).abs().max() <= 1e-12
        elif kind == "neg200":
            assert s.max() < -150 and s.min() > -250
        else:
            want = {"dom-t": t, "dom-0": 0, "dom-last": Lmax - 2}[kind]
            third = s.sort(-1).values[:, -3]
            assert (top.indices[:, 0] == want).all() and (top.values[:, 0] - third >= 60).all(), (b, top)
            if kind == "dom-last":                     # the runner-up sits in split 0, well above the rest
                assert (top.indices[:, 1] == 0).all() and (top.values[:, 0] - top.values[:, 1] >= 30).all()
                assert (top.values[:, 1] - third >= 20).all()
            else:
                assert (top.values[:, 0] - top.values[:, 1] >= 60).all()
    ps = positions(data.nsplit, Lmax)
    for t in ps:
        data.check(t, ragged=False)
    for ts in ragged_batches(ps, B):
        data.check(ts, ragged=True)
    print(f"\n{name} {kind} fp8={fp8}: largest (err - 2^-8|ref|) / F so far {SEEN['c']:.3f}")


# =====================================================================================================================
# 2. decode-size projections
# =====================================================================================================================
MS, NS, KS = (1, 5, 31, 32), (4, 40, 96, 340, 1536), (64, 192, 512, 1024, 2048)


def shapes(ks):
    """every (M, N, K), with act / bias / weight layout cycling so that each value of each occurs with each M, N and K"""
    out, i = [], 0
    for K in ks:
        for N in NS:
            for M in MS:
                out.append((M, N, K, i % 2, (i // 2) % 2 == 0, (i // 4) % 2 == 0))
                i += 3
    return out


def _randw(N, K, g):
    return (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF)


def _weight(w, frag):
    ops = KC.ops()
    return ops.FragWeight(w.to(DEV)) if frag else w.to(DEV)


def check_c(c, a_used, w, bias, act, what):
    """C against the fp64 product of the values the kernel multiplied: 2^-8 |ref| (output rounding) + K 2^-23 S (fp32
    accumulation in any order, S = sum_k |a_k w_k|)"""
    ref, S = D.linear(a_used, w, bias, act)
    err = (c.double() - ref).abs()
    bad = err > 2.0 ** -8 * ref.abs() + w.shape[1] * 2.0 ** -23 * S
    assert not bad.any(), (what, bad.nonzero()[:4].tolist(), err[bad][:4].tolist(), ref[bad][:4].tolist())


def check_rows(z, ref, what):
    """a bf16 row output (H, Z) that feeds the next residual: 2^-8 |ref| + 2^-20"""
    err = (z.double() - ref).abs()
    bad = err > 2.0 ** -8 * ref.abs() + 2.0 ** -20
    assert torch.isfinite(z).all() and not bad.any(), (what, bad.nonzero()[:4].tolist(), err[bad][:4].tolist(), ref[bad][:4].tolist())


def test_skinny_projection_against_fp64():
    ops = KC.ops()
    g = torch.Generator().manual_seed(11)
    for M, N, K, act, has_bias, frag in shapes(KS):
        a, w = torch.randn(M, K, generator=g).to(BF), _randw(N, K, g)
        bias = torch.randn(N, generator=g) if has_bias else None
        c = ops.linear_fwd(a.to(DEV), _weight(w, frag), None if bias is None else bias.to(DEV), act)
        torch.cuda.synchronize()
        assert c.shape == (M, N)
        check_c(c.float().cpu(), a, w, bias, act, ("skinny", M, N, K, act, has_bias, frag))
        if frag:                                           # and the other layout on the same operands: both are checked
            c2 = ops.linear_fwd(a.to(DEV), w.to(DEV), None if bias is None else bias.to(DEV), act)
            check_c(c2.float().cpu(), a, w, bias, act, ("skinny row-major", M, N, K, act, has_bias))


def _unit_rows(M, K):
    """k(m): all four wave slices of K, both 8-column halves of a 16-column step, the first, a middle and the last step"""
    kq = K // 4
    steps = [0, kq // 16 - 1, (kq // 16) // 2]
    return [(m % 4) * kq + steps[(m // 8) % 3] * 16 + ((m // 4) % 2) * 8 + (m * 5 + m // 8) % 8 for m in range(M)]


def _coded_weight(N, K):
    """W[n][k] = 16 (n mod 16) + (k mod 16): at most 8 bits, exact in bf16; a fragment read from the wrong place shows"""
    return ((torch.arange(N)[:, None] % 16) * 16 + torch.arange(K)[None] % 16).to(BF)


@pytest.mark.parametrize("K", KS)
def test_fragment_order_is_exact_on_unit_vectors(K):
    """row m of A is the unit vector e_k(m), W a small integer code of (n mod 16, k mod 16): C[m][n] = W[n][k(m)] exactly"""
    ops = KC.ops()
    M = 32
    ks = _unit_rows(M, K)
    kq = K // 4
    assert {k // kq for k in ks} == {0, 1, 2, 3} and {(k % 16) // 8 for k in ks} == {0, 1}
    assert {(k % kq) // 16 for k in ks} >= {0, kq // 16 - 1} and len(set(ks)) == M
    a = torch.zeros(M, K)
    a[torch.arange(M), ks] = 1.0
    for N in NS:
        w = _coded_weight(N, K)
        want = w.float()[:, ks].T
        for frag in (True, False):
            c = ops.linear_fwd(a.to(BF).to(DEV), _weight(w, frag), None, 0)
            assert torch.equal(c.float().cpu(), want), ("skinny", N, K, frag)
        # the fused embedding: table rows e_k / sqrt(K) (exact when K is a square), pe = 0 -> H = e_k
        if math.isqrt(K) ** 2 == K:
            V = M
            table = (a / math.sqrt(K)).to(DEV)
            pe = torch.zeros(3, K, device=DEV)
            tok = torch.arange(M, dtype=torch.int32, device=DEV)
            for frag in (True, False):
                for ragged in (False, True):
                    pos = torch.full((M,), 2, dtype=torch.int32, device=DEV) if ragged else torch.tensor([2], dtype=torch.int32, device=DEV)
                    hout = torch.empty(M, K, dtype=BF, device=DEV)
                    c, _ = ops.decode_embed_linear(tok, table, pe, pos, _weight(w, frag), None, hout, ragged=ragged)
                    assert torch.equal(hout.float().cpu(), a) and torch.equal(c.float().cpu(), want), ("embed", N, K, frag, ragged)


def _ln_rows(M, K, g):
    """X, RES rows: centred Gaussian rows, and rows far from zero -- |mean| / std of 16, 64, 256 and 300, and a constant row.
    The uncentred rows lie on a grid (X multiples of 2^-3 or coarser as bf16 has it, RES multiples of 2^-6 below 2^-3) and are
    used with K a power of two, so that z, its sum and its mean are exact in fp32: what is left is the variance formula."""
    x = torch.randn(M, K, generator=g)
    r = 0.5 * torch.randn(M, K, generator=g)
    kinds = []
    if K & (K - 1) == 0:
        grid = (torch.randint(-8, 9, (M, K), generator=g) / 64.0)
        for m, (mean, std) in zip(range(M), [(4.0, 0.25), (16.0, 0.25), (30.0, 0.1), (60.0, 0.25), (-60.0, 0.25), (3.0, 0.0)]):
            if m == 0 and M > 1:
                continue                                   # row 0 stays Gaussian
            x[m] = mean + std * torch.randn(K, generator=g)
            r[m] = grid[m] if std else 0.0
            kinds.append((m, mean, std))
    return x.to(BF), r.to(BF), kinds


def test_layernorm_projection_against_fp64_with_rows_far_from_zero():
    """Z = LayerNorm(X + RES) and C = act(Z W^T + b): Z against the centred fp64 form, C against the fp64 product of the
    kernel's own Z (checked first, so no input error term is left).  On the rows far from zero Z also agrees with the
    training LayerNorm kernel within one bf16 ulp."""
    ops = KC.ops()
    g = torch.Generator().manual_seed(12)
    seen = set()
    for M, N, K, act, has_bias, frag in shapes(KS[:-1]):
        x, r, kinds = _ln_rows(M, K, g)
        gamma, beta = 1 + 0.25 * torch.randn(K, generator=g), 0.25 * torch.randn(K, generator=g)
        w = _randw(N, K, g) if (M + N) % 3 else (_coded_weight(N, K).float() / 64).to(BF)
        bias = torch.randn(N, generator=g) if has_bias else None
        c, z = ops.linear_ln_fwd(x.to(DEV), r.to(DEV), gamma.to(DEV), beta.to(DEV), _weight(w, frag),
                                 None if bias is None else bias.to(DEV), act)
        torch.cuda.synchronize()
        what = ("ln", M, N, K, act, has_bias, frag)
        z = z.float().cpu()
        zref = D.add_ln(x, r, gamma, beta, 1e-6)
        for m, mean, std in kinds:
            check_rows(z[m:m + 1], zref[m:m + 1], what + ("row", m, "mean", mean, "std", std))
            seen.add((mean, std))
            if std == 0:
                assert torch.equal(z[m], beta.to(BF).float()), what          # variance exactly 0: Z = beta
        check_rows(z, zref, what)
        check_c(c.float().cpu(), z, w, bias, act, what)
        if kinds:
            zt = ops.add_ln_fwd(x.to(DEV), r.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6)[0].float().cpu()
            rows = [m for m, _, _ in kinds]
            # one bf16 ulp of the value; where gamma n + beta cancels, two fp32 evaluations in different orders differ by
            # 2^-24 |gamma n| whatever the result's own ulp is: the absolute term of check_rows covers that
            ulp = 2.0 ** (torch.floor(torch.log2(torch.maximum(z[rows].abs(), zt[rows].abs()).clamp(min=2.0 ** -126))) - 7)
            assert ((z[rows] - zt[rows]).abs() <= ulp + 2.0 ** -20).all(), what
    assert seen == {(4.0, 0.25), (16.0, 0.25), (30.0, 0.1), (60.0, 0.25), (-60.0, 0.25), (3.0, 0.0)}


def test_layernorm_projection_refuses_what_it_cannot_hold():
    ops = KC.ops()
    from musicgeneration_amd._lib import MgxError
    g = torch.Generator().manual_seed(13)
    for M, K in ((33, 512), (4, 96), (4, 1088)):
        x = torch.randn(M, K, generator=g).to(BF).to(DEV)
        gam = torch.ones(K, device=DEV)
        w = _randw(64, K, g).to(DEV)
        for wt in (w, ops.FragWeight(w)):
            with pytest.raises(MgxError, match=r"status -1"):                  # MGX_ERR_SHAPE, before any launch
                ops.linear_ln_fwd(x, x, gam, gam, wt, None, 0)
    torch.cuda.synchronize()


def _embed_inputs(M, K, V, P, g):
    table, pe = torch.randn(V, K, generator=g), torch.randn(P, K, generator=g)
    tok = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    pos = torch.randint(0, P, (M,), generator=g, dtype=torch.int32)
    tok[0], pos[0] = V - 1, P - 1
    if M > 1:
        tok[-1], pos[-1] = 0, 0
    return table, pe, tok, pos


def test_fused_embedding_projection_against_fp64():
    """H = table[tok] sqrt(K) + pe[pos] and C = H W^T + b, shared and per-row positions, both weight layouts"""
    ops = KC.ops()
    g = torch.Generator().manual_seed(14)
    V, P = 53, 41
    for i, (M, N, K, _, has_bias, frag) in enumerate(shapes(KS)):
        table, pe, tok, pos = _embed_inputs(M, K, V, P, g)
        w = _randw(N, K, g)
        bias = torch.randn(N, generator=g) if has_bias else None
        for ragged in (False, True):
            p = pos if ragged else pos[i % M:i % M + 1].clone()
            hout = torch.full((M, K), float("nan"), dtype=BF, device=DEV)
            c, _ = ops.decode_embed_linear(tok.to(DEV), table.to(DEV), pe.to(DEV), p.to(DEV), _weight(w, frag),
                                           None if bias is None else bias.to(DEV), hout, ragged=ragged)
            torch.cuda.synchronize()
            what = ("embed-linear", M, N, K, has_bias, frag, ragged)
            hh = hout.float().cpu()
            check_rows(hh, D.embed(tok, table, pe, p), what)
            check_c(c.float().cpu(), hh, w, bias, 0, what)


def test_decode_embed_against_fp64():
    ops = KC.ops()
    g = torch.Generator().manual_seed(15)
    V, P = 53, 41
    for B in (1, 5, 37):
        for d in (64, 192, 512):
            table, pe, tok, pos = _embed_inputs(B, d, V, P, g)
            for ragged in (False, True):
                for p in ([pos] if ragged else [pos[:1], pos[-1:]]):          # shared position: the last row of pe, and 0
                    out = torch.full((B, d), float("nan"), dtype=BF, device=DEV)
                    ops.decode_embed(tok.to(DEV), table.to(DEV), pe.to(DEV), p.contiguous().to(DEV), out, ragged=ragged)
                    torch.cuda.synchronize()
                    check_rows(out.float().cpu(), D.embed(tok, table, pe, p), ("embed", B, d, ragged))


# =====================================================================================================================
# 3. sampler
# =====================================================================================================================
SAMPLER_V = (1, 2, 63, 64, 65, 337, 1023, 1024)
SAMPLER_T = (0.5, 1.0, 1.7)
SAMPLER_ROWS = 256
ENTRIES = ("plain", "rows", "ragged")


def sampler_kp(V):
    return [(0, 1.0), (1, 1.0), (5, 1.0), (V - 1, 1.0), (V, 1.0), (V + 7, 1.0), (0, 0.9), (0, 1e-6), (40, 0.9), (3, 0.5)]


def sampler_cases():
    """every (V, (top_k, top_p)); temperature, grammar and entry point cycle so that each occurs with each V and each pair"""
    out = []
    for iv, V in enumerate(SAMPLER_V):
        for ik, (k, tp) in enumerate(sampler_kp(V)):
            i = iv * 11 + ik
            out.append((V, SAMPLER_T[i % 3], k, tp, (i // 3) % 2 == 0, ENTRIES[(iv + ik) % 3]))
    return out


def grammar_table(V, g):
    """row v allows: v % 4 == 0 a random half, 1 three ids (fewer than most top_k), 2 exactly one, 3 nothing"""
    allow = np.zeros((V, V), dtype=bool)
    for v in range(V):
        if v % 4 == 0:
            allow[v] = torch.rand(V, generator=g).numpy() < 0.5
        elif v % 4 == 1:
            allow[v, torch.randperm(V, generator=g)[:3].numpy()] = True
        elif v % 4 == 2:
            allow[v, int(torch.randint(0, V, (1,), generator=g))] = True
    tab = np.zeros((V, (V + 31) // 32), dtype=np.uint32)
    for w in range((V + 31) // 32):
        bits = allow[:, 32 * w:32 * w + 32]
        tab[:, w] = (bits.astype(np.uint64) << np.arange(bits.shape[1], dtype=np.uint64)).sum(1).astype(np.uint32)
    return tab


def sampler_inputs(V, top_k, grammar, seed, B=SAMPLER_ROWS):
    """bf16 logits [B, ld] of scale 2 with NaN in the padding columns; every fourth row has the values ranked around the k-th
    made equal (a tie across the k-th value), every fourth one -inf in a third of its columns (never in all)"""
    g = torch.Generator().manual_seed(seed)
    ld = (V + 7) // 8 * 8 + 8
    x = (2 * torch.randn(B, V, generator=g)).to(BF).float()
    for i in range(1, B, 4):
        if V >= 4:
            order = x[i].argsort(descending=True)
            j = max(0, min(top_k if top_k > 0 else 4, V - 2) - 2)
            x[i, order[j:j + 3]] = x[i, order[j]].item()
    for i in range(2, B, 4):
        dead = torch.rand(V, generator=g) < 0.33
        dead[int(torch.randint(0, V, (1,), generator=g))] = False
        x[i, dead] = float("-inf")
    logits = torch.full((B, ld), float("nan"))
    logits[:, :V] = x
    prev = torch.randint(0, V, (B,), generator=g, dtype=torch.int32)
    prev[:8] = torch.arange(8, dtype=torch.int32) % V                       # every kind of grammar row occurs
    table = grammar_table(V, g) if grammar else None
    return logits.to(BF), prev, table


def sampler_reference(logits, V, temperature, top_k, top_p, seed, steps, row0, prev, table, r=None):
    """per row: the reference probabilities, the set of tokens the row may draw (one token unless the row is ambiguous), the
    ambiguity flag and the union of the kept sets it may use"""
    r = R_PROB if r is None else r
    B = logits.shape[0]
    allowed = D.allowed_mask(table, prev, V) if table is not None else None
    p = D.softmax_probs(logits[:, :V].float(), np.float32(temperature), allowed)
    keep, info = D.kept_set_rows(p, top_k, top_p)
    u = D.u01(seed, np.broadcast_to(np.asarray(steps), (B,)), row0 + np.arange(B))
    pk = p * keep
    cdf = np.cumsum(pk, 1)
    total = cdf[:, -1]
    # how far a mass the sampler compares (a CDF prefix, the mass above a threshold) may be from the reference's: the element
    # errors enter such a sum with their signs, normalised by their own total, so the sum is not r * total off but what an
    # fp32 evaluation of the same softmax and prefix sums is off (taken per row from one), plus 32 * 2^-24 for the order of the
    # sampler's own lane-prefix and wave sums.  r stays the bound of a single element (the top-k comparison of two values).
    p32 = D.softmax_probs(logits[:, :V].float(), np.float32(temperature), allowed, dtype=np.float32)
    d32 = np.abs(np.cumsum(p32 * keep, 1, dtype=np.float32) - cdf).max(1) / total
    rel = d32 + 32 * 2.0 ** -24
    target = u * total
    near_cdf = (np.where(keep, np.abs(cdf - target[:, None]), np.inf).min(1) <= rel * total)
    tk = info["tau_k"][:, None]
    near_k = ((np.abs(p - tk) <= r * tk) & (p != tk) & (p > 0)).any(1)
    near_p = info["gap"] <= rel * info["mass"]
    amb = near_cdf | near_k | near_p
    tokens, kept_union = [], keep.copy()
    for i in range(B):
        if not amb[i]:
            tokens.append({D.draw(pk[i], u[i])})
            continue
        ok = set()
        for alt in D.kept_set_alternatives(p[i], top_k, top_p, r, rel[i] * info["mass"][i]):
            kept_union[i] |= alt
            pa = p[i] * alt
            ca = np.cumsum(pa)
            band, tg = rel[i] * ca[-1], u[i] * ca[-1]
            ok |= set(np.nonzero(alt & (ca >= tg - band) & (ca - pa < tg + band))[0].tolist())
        tokens.append(ok)
    return p, tokens, amb, kept_union


def run_sampler(entry, logits, V, temperature, top_k, top_p, seed, pos, prev, table, row0=0, advance=True, out_ld=64):
    """one call on the device -> (tokens, out_tokens, probs_out, pos after the call), all on the CPU"""
    ops = KC.ops()
    from musicgeneration_amd import _lib
    B = logits.shape[0]
    lg, pos_d, nt = logits.to(DEV), pos.to(DEV), prev.clone().to(DEV)
    out = torch.full((B, out_ld), -1, dtype=torch.int32, device=DEV)
    probs = torch.full((B, V), float("nan"), device=DEV)
    tab = None if table is None else torch.from_numpy(table.view(np.int32).copy()).to(DEV)
    if entry == "plain":                                   # the C entry itself: a shared counter, no base, row0 = 0
        assert row0 == 0
        _lib.check(_lib.load().mgx_sample_topk_topp(lg.data_ptr(), V, lg.shape[1], float(temperature), int(top_k), float(top_p),
                                                    int(seed), pos_d.data_ptr(), None, 0, nt.data_ptr(), out.data_ptr(), out_ld,
                                                    probs.data_ptr(), B, 0, 1 if advance else 0,
                                                    None if tab is None else tab.data_ptr(), _lib.stream_ptr()),
                   "mgx_sample_topk_topp")
    else:
        ops.sample_topk_topp(lg, V, pos_d, nt, out, probs, temperature, top_k, top_p, seed, advance, tab, row0,
                             ragged=entry == "ragged")
    torch.cuda.synchronize()
    return nt.cpu().numpy(), out.cpu().numpy(), probs.double().cpu().numpy(), pos_d.cpu()


def _positions_for(entry, B, g):
    return torch.randint(0, 50, (B,), generator=g, dtype=torch.int32) if entry == "ragged" else \
        torch.randint(0, 50, (1,), generator=g, dtype=torch.int32)


def _case_seed(i):
    return (0x9E3779B97F4A7C15 * (i + 1) + 0x1234567) & 0xFFFFFFFFFFFFFFFF      # both halves of the seed in use


@pytest.mark.parametrize("case", range(len(sampler_cases())), ids=lambda i: "V{}-T{}-k{}-p{}-g{:d}-{}".format(*sampler_cases()[i]))
def test_sampler_draws_the_reference_token_in_every_row(case):
    V, temperature, top_k, top_p, grammar, entry = sampler_cases()[case]
    B, seed = SAMPLER_ROWS, _case_seed(case)
    logits, prev, table = sampler_inputs(V, top_k, grammar, case)
    pos = _positions_for(entry, B, torch.Generator().manual_seed(case))
    p, tokens, amb, kept = sampler_reference(logits, V, temperature, top_k, top_p, seed, pos.numpy(), 0, prev.numpy(), table)
    assert amb.mean() <= 0.02, ("ambiguous rows", amb.mean())
    tok, out, probs, pos_after = run_sampler(entry, logits, V, temperature, top_k, top_p, seed, pos, prev, table)
    # probs_out: the unfiltered softmax
    err = np.abs(probs - p)
    big = p > 1e-9
    SEEN["r"] = max(SEEN["r"], float(((err - 1e-12) / np.where(big, p, 1.0))[big].max()))
    print(f"\nambiguous rows {amb.mean():.4f}; largest relative error of probs_out so far {SEEN['r']:.3e} = 2^{math.log2(max(SEEN['r'], 1e-30)):.2f}")
    assert np.isfinite(probs).all() and (err <= R_PROB * p + 1e-12).all(), (err / np.maximum(p, 1e-300)).max()
    # the token, row by row
    assert ((tok >= 0) & (tok < V)).all()
    assert kept[np.arange(B), tok].all(), ("outside the kept set", np.nonzero(~kept[np.arange(B), tok])[0][:8])
    wrong = [i for i in range(B) if int(tok[i]) not in tokens[i]]
    assert not wrong, (wrong[:8], [int(tok[i]) for i in wrong[:8]], [tokens[i] for i in wrong[:8]], amb[wrong[:8]])
    # where it went, and the positions
    steps = np.broadcast_to(pos.numpy(), (B,))
    want_out = np.full_like(out, -1)
    want_out[np.arange(B), steps + 1] = tok
    assert (out == want_out).all()
    assert torch.equal(pos_after, pos + 1)                                     # uniform: +1 once; ragged: every row


@pytest.mark.parametrize("entry", ["rows", "ragged"])
def test_sampler_sub_batches_draw_what_the_whole_batch_draws(entry):
    V, temperature, top_k, top_p = 337, 1.0, 40, 0.9
    B, seed = SAMPLER_ROWS, _case_seed(1000)
    logits, prev, table = sampler_inputs(V, top_k, True, 1000)
    pos = _positions_for(entry, B, torch.Generator().manual_seed(5))
    whole, out, _, after = run_sampler(entry, logits, V, temperature, top_k, top_p, seed, pos, prev, table, advance=False)
    assert torch.equal(after, pos)                                             # advance = 0: untouched
    halves = []
    for row0 in (0, B // 2):
        sl = slice(row0, row0 + B // 2)
        halves.append(run_sampler(entry, logits[sl], V, temperature, top_k, top_p, seed, pos[sl] if entry == "ragged" else pos,
                                  prev[sl], table, row0=row0, advance=False)[0])
    assert (np.concatenate(halves) == whole).all()
    wrong0 = run_sampler(entry, logits[B // 2:], V, temperature, top_k, top_p, seed, pos[B // 2:] if entry == "ragged" else pos,
                         prev[B // 2:], table, row0=0, advance=False)[0]
    assert (wrong0 != whole[B // 2:]).mean() > 0.1                              # the row offset is part of the draw
    # and the whole batch is the reference's
    _, tokens, amb, _ = sampler_reference(logits, V, temperature, top_k, top_p, seed, pos.numpy(), 0, prev.numpy(), table)
    assert amb.mean() <= 0.02 and all(int(whole[i]) in tokens[i] for i in range(B))


def test_sampler_draw_on_an_exact_cdf_boundary():
    """1024 equal logits: every probability is 2^-10, every prefix sum and the total are exact in fp32, so nothing rounds and
    no band applies.  For u >= 0.5 the sampler's u is a multiple of 2^-24 and can sit exactly ON a CDF boundary k 2^-10: the
    draw is then the id whose inclusive CDF equals u (the FIRST id that reaches it), not the next one.  The (step, row)
    pairs that give such a u are found with the hash's integer twin."""
    ops = KC.ops()
    V, B, seed = 1024, 16, _case_seed(2000)
    steps = np.arange(400000)
    pos, want = [], []
    for b in range(B):
        u = D.u01(seed, steps, b)
        hit = np.nonzero((u * 1024 == np.floor(u * 1024)) & (u < 1))[0]
        assert hit.size, b
        pos.append(int(steps[hit[b % hit.size]]))
        want.append(int(u[hit[b % hit.size]] * 1024) - 1)
    assert min(want) >= 511 and len(set(want)) > B // 2
    logits = torch.full((B, V + 8), 1.5, dtype=BF, device=DEV)
    pos_d = torch.tensor(pos, dtype=torch.int32, device=DEV)
    nt = torch.zeros(B, dtype=torch.int32, device=DEV)
    probs = torch.empty(B, V, device=DEV)
    ops.sample_topk_topp(logits, V, pos_d, nt, None, probs, 1.0, 0, 1.0, seed, False, None, 0, ragged=True)
    torch.cuda.synchronize()
    assert (probs == 2.0 ** -10).all()
    assert nt.cpu().tolist() == want
    assert [D.draw(np.full(V, 2.0 ** -10), D.u01(seed, s, b)) for b, s in enumerate(pos)] == want
