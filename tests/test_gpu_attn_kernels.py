"""The training attention kernels of the product library -- the forward (csrc/rel_attn_fwd.hip: mgx_rel_attn_fwd, _fwd_nomask,
_weights), the pre-pass (rel_attn_bwd.hip), the 32-key and the 64-key dK/dV kernels (rel_attn_dkv32.hip, rel_attn_dkv64.hip with its
generated sweep), the readers of the stored dS tiles (rel_attn_dq_lite.hip, rel_attn_de_tiles.hip) and the recompute kernels
(rel_attn_bwd_recompute.hip) -- against the fp64 references of oracle/train_ref.py (rel_attn_fwd / rel_attn_bwd), element by element,
inside guard bands, through the raw C ABI.  Until now tests/test_gpu_kernels.py was their only check: max-norm, cosine and rel-L2
against an fp32 oracle on Gaussian data, which one query row attending to the wrong key, a relative index off by one at a tile
boundary, a pad bit of the neighbouring word or one lost 32 x 32 dS tile all pass.

No bound here is a max-norm bound and none was measured on a kernel (oracle/train_ref.py: attn_eps, attn_fwd_bounds,
attn_weights_bound, attn_bwd_bounds).  u = 2^-8: the conversions to bf16 are RNE (pack_bf16x2) and bf16 has 8 significant bits: the
spacing at 1 is 2^-7, so rounding to nearest loses up to half of it, 2^-8 / (1 + 2^-8) of the value (1 + 2^-8 rounds to 1); it is
the same unit as the 2^-8 |ref| of an output's own rounding (oracle/train_ref.py: U_BF).  Notation of rel_attn_bwd.hip: qs = q / 8,
Er[dl] = E[M - 1 - dl], S = qs . k_j + qs . Er[i - j], A_ij = sum_c |qs_ic| (|k_jc| + |Er[i - j]_c|), all sums from the reference.
  eps_ij  relative error of P_ij = exp2(S log2e - lse log2e):  expm1(17 2^-24 R_ij + 2^-22 (|S_ij| + |lse_i|)) + 2^-21
            17 2^-24 R    the logit: eight MFMA instructions (mfma(qf[ks], e[ks], .), then mfma(frag_R(kt, ..), qf[ks], .) on the same
                          accumulator; the recompute dE kernel adds two chains of four), each D = C + 16 products of bf16 values,
                          which are exact in fp32: 17 addends in the hardware's own order, error <= 17 2^-24 (sum |products| + |C|).
                          R_ij = A_ij + the |C| operands, taken from the reference: the partial sums of the relative and of the
                          content term over 16, 32, 48 columns, 4 |relative term| (it is C of the four K instructions) and |S|.
                          (The bound first written here, 130 2^-24 A for 128 terms in ANY order, was 40 to 70 times the error of lse
                          and weights on Gaussian data: it charged every one of 128 roundings with the whole absolute sum.)
            2^-22 (|S| + |lse|)   the fma S * LOG2E - lse2 (fwd: exp_tile; dkv32: c * 0.125 LOG2E + nl; weights: fmaf(sv, LOG2E,
                          -lse2w)): LOG2E and the pre-pass's nlse2 = -lse * LOG2E are each rounded once, the fma once; an absolute
                          error e of the exponent is a relative error expm1(e ln 2) < expm1(e) of P
            2^-21         v_exp_f32 (__builtin_amdgcn_exp2f), 1 ulp, and its argument's own last bit
  eps_i   max_j eps_ij over the visible keys of row i
  ctx     2^-8 |ref| + (1 + 2^-8) (u + 2 eps_i + (L + 2) 2^-24) sum_j P_ij |v_jc|
            2^-8 |ref|  store_rows_lds packs O / l to bf16: u of the value stored, which lies within the rest of the bound of ref: the
                        factor 1 + 2^-8 on the rest
            u           P is packed to bf16 (exp_tile: pf) before the O^T += V^T P^T product
            2 eps_i     the numerator's P_ij and the row sum l (fp32 sum of the unrounded p) each carry eps
            (L + 2)     fp32 accumulation of <= L terms in O and in l, the rescale by alpha and the division
  lse     17 2^-24 sum_j P_ij R_ij exp(2 * 17 2^-24 max_j R_ij) + (L / 32 + 8) 2^-24 + 2 ulp32(lse)
            log-sum-exp moves by a weighted mean of the logits' errors, the weights a softmax between the exact and the computed
            logits (mean value theorem): within exp(2 max error) of P.  The row sum l: five adds deep inside a tile (exp_tile's four
            chains), one add per tile (l_run += lsum), one across the lane halves, the rescale by alpha.  m_ref + __logf(l_tot): 2 ulp
  weights (eps_ij + 2^-23) P_ij; entries that are masked, inside a visited tile, are exactly 0
  dS      g_ij = P_ij [eps_ij |dP_ij - delta_i| + 66 2^-24 (sum_c |dO_ic| |v_jc| + sum_c |dO_ic| |ctx_ic|)] + u |dS_ij|
            dP - delta is one fp32 MFMA accumulation of 64 products that STARTS from -delta (dkv32: `dp`), delta the pre-pass's
            fp32 sum of 64 products (attn_delta_kernel): 66 2^-24 of the absolute sums; dS = p * dp is then packed to bf16
            (acc_to_frag(ds)): u |dS|; it is those bf16 tiles that dq_lite and de_tiles read
  dv      2^-8 |ref| + (1 + 2^-8) sum_i (eps_ij + u + L 2^-24) P_ij |dO_ic|          P packed to bf16 (acc_to_frag(c)), L-term fp32 sum
  dk      2^-8 |ref| + (1 + 2^-8) sum_i (g_ij + L 2^-24 |dS_ij|) |qs_ic|
  dq      the same with |k_jc| + |Er[i - j]_c| in place of |qs_ic|, summed over j, scaled by 1 / 8
  dE      sum_{b,h,i} (g + B h L 2^-24 |dS|) |qs| + ulp32(max(|start|, |start + update|))      fp32, accumulated into the start value
  underflow   fp32 and bf16 share the exponent range: a P, a product p * dp or a packed value below the smallest normal 2^-126 may be
              flushed to 0 whatever its relative accuracy.  TINY = 2^-124 (four such steps) is added to the error of every visible P
              and (times |dP - delta| + 1) of every dS: the selector data has weights of e^-256, everything else is far above it.
The backward gets ctx_in = bf16(reference ctx), lse_in = fp32(reference lse) and is compared with the formula ON THOSE: a forward
error can neither hide in it nor be blamed on it.  The chained cases feed the kernel's own ctx and lse; their reference is on those.

Data (oracle/train_ref.py; every precondition is asserted there from the reference):
  gauss     qkv 0.8, E 0.5, dctx 1.0, the scales of tests/test_gpu_kernels.py
  far       one logit 128 nats above its row in a later key tile: the forward's redo-and-rescale branch, inside the main loop
  rel       the relative selector: row i attends to key i - delta0 alone, by 256 nats; delta0 in {0, 1, 31, 32, 33, 127, 128, L - 1}
  content   the content selector: row i attends to key t(i) alone, by 259 nats; every tile with a real key is selected
On the selectors every other weight is exactly 0 in fp32 and v, dO are small integers: ctx is the selected v row and dv the integer
sum of the selecting dO rows EXACTLY, dq is exactly 0 on selecting rows, and on content data dk is 0 and dE comes back as it started.
A wrong key, relative index or pad bit is wrong by whole integers.  Both families go through the same bound formulas as well.
Pad patterns (attn_pads): none, trailing, interior, a whole 32-key tile, every second key, bit 0 / bit 31 of a word.

Guard bands: every operand and output lies 512 bytes inside a larger allocation.  Bands of qkv, E, ctx_in, dctx, lse_in hold NaN,
those of padbits have all bits set; ctx, lse, weights, dqkv, dE and the workspace -- exactly the size its query returns -- lie in 0x5A
bands that must come back bit for bit.  Outputs start as the 0x5A pattern (1.5e16 in bf16: an unwritten element fails), dE from a
seeded non-zero value (the call accumulates; rows < M - L must come back bit-identical).

Shapes: L = 32 one tile | 96 a query block with an idle wave, 32-key dK/dV | 128 the smallest 64-key dK/dV | 160 a forward main-loop
tile plus tail, L % 128 == 32 | 256 two 128-key blocks | 288 nine tile diagonals: a ragged last de_tiles group; B = 8 at L = 160 for
the dE groups dealt across XCDs.  Batch groups smaller than B are not reachable at these sizes: the long cases of
tests/test_gpu_kernels.py (test_rel_attn_bwd_matches_oracle_autograd, test_dkv64_matches_the_32_key_kernel_bitwise) and
tests/test_gpu_large_offsets.py (L = 2048, d = 512: B = 128 in groups of 8, B = 127 in 127 groups of one) are the cover for that.
The product library only: no experiment build, no environment variable.  Every test prints its largest (error / bound)
ratio per output before it asserts (pytest -s; profiles/r18_attn_kernel_tests.txt has the figures).
"""
import functools

import pytest
import torch

import kernel_checks as KC
from kernel_checks import BAND, Banded, Det, P, check_equal, nothing_more_after_a_gpu_error, operand, output  # noqa: F401 (the fixture is used by name)
from oracle import train_ref as T

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SEEN = {}
_report = KC.report_fixture(SEEN, "largest error / bound {:.3g}")
PROD, DKV32, RECOMPUTE = 1 | 4 | 2 | 8, 1 | 64 | 2 | 8, 1 | 4 | 32 | 16
PARTS_NAME = {PROD: "bwd", DKV32: "bwd[32-key dK/dV]", RECOMPUTE: "bwd[recompute dQ, dE]"}

# (B, L, heads, M)
SHAPES = ((2, 32, 1, 32), (1, 96, 3, 97), (3, 128, 2, 128), (2, 160, 1, 260), (1, 256, 2, 256), (2, 288, 1, 289))
IDS = [f"L{s[1]}" for s in SHAPES]


class OnesBanded(Banded):
    """padbits: the bands have all bits set (a word taken from beyond the bitmap pads 32 keys)"""

    def __init__(self, t):
        super().__init__(t, BAND, b"\xff")


def check_bound(fam, kind, got, ref, bound, case):
    KC.check_bound(fam, got, ref, bound, case, seen=SEEN, key=(fam, kind))


# ---- cases: inputs, reference and bounds, built once and shared ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_case(kind, B, L, heads, M, pads, extra=None):
    """kind gauss / far / rel (extra = delta0) / content -> T.Ref of inputs, forward reference and bounds, backward reference"""
    pm = T.attn_pads(pads, B, L)
    c = T.Ref(kind=kind, B=B, L=L, heads=heads, d=64 * heads, M=M, pm=pm, rows=None,
              name=f"{kind}{'' if extra is None else extra} B={B} L={L} h={heads} M={M} pads={pads}")
    if kind == "gauss":
        c.qkv, c.E, c.dctx = T.attn_gauss(B, L, heads, M)
    elif kind == "far":
        assert pm is None
        c.qkv, c.E, c.dctx, _ = T.attn_far(B, L, heads, M)
    elif kind == "rel":
        c.qkv, c.E, c.dctx, c.sel, c.rows, c.ctx_exact, c.dv_exact = T.attn_selector_rel(B, L, heads, M, extra, pm)
    elif kind == "content":
        c.qkv, c.E, c.dctx, c.sel, c.rows, c.ctx_exact, c.dv_exact = T.attn_selector_content(B, L, heads, M, pm)
    c.ref = T.rel_attn_fwd(c.qkv, c.E, pm, heads, M)
    c.ctx_bound, c.lse_bound, _ = T.attn_fwd_bounds(c.ref)
    g = torch.Generator().manual_seed(L + M)
    c.dE0 = torch.randint(-9, 10, (M, 64), generator=g).float() if c.rows is not None else torch.randn(M, 64, generator=g)
    assert (c.dE0 != 0).any()
    return c


@functools.lru_cache(maxsize=None)
def bwd_ref(c):
    """the backward reference on ctx_in = bf16(reference ctx), lse_in = fp32(reference lse)"""
    ctx_in, lse_in = c.ref.ctx.to(BF), c.ref.lse.to(F32)
    r = T.rel_attn_bwd(c.qkv, c.E, c.pm, ctx_in, lse_in, c.dctx, c.heads, c.M)
    return ctx_in, lse_in, r, T.attn_bwd_bounds(r, c.B, c.dE0)


def cases_of(kind, shape_index):
    """the cases of one data family at one shape; over the six shapes every family meets every pad pattern"""
    B, L, heads, M = SHAPES[shape_index]
    pads = T.ATTN_PADS
    if kind == "gauss":
        return [make_case("gauss", B, L, heads, M, pads[shape_index]), make_case("gauss", B, L, heads, M, pads[(shape_index + 3) % 6])]
    if kind == "far":
        return [make_case("far", B, L, heads, M, "none")]
    if kind == "content":
        return [make_case("content", B, L, heads, M, p) for p in pads]
    out = []
    for n, d0 in enumerate(T.SEL_REL_DELTAS):
        d0 = L - 1 if d0 < 0 else d0
        if d0 < L and (d0 != L - 1 or n == len(T.SEL_REL_DELTAS) - 1):
            out.append(make_case("rel", B, L, heads, (L, L + 1, L + 100)[(n + shape_index) % 3], pads[(n + shape_index) % 6], d0))
    return out


# ---- forward ----------------------------------------------------------------------------------------------------------------------
def launch_fwd(c, qkv=None, E=None, Lk=None):
    """mgx_rel_attn_fwd (Lk None) or mgx_rel_attn_fwd_nomask inside bands -> ctx bf16 [B, L, d], lse f32 [B, h, L] on the device"""
    lib, chk, _, sp = KC.raw(product_only=True)
    B, L, d, M = c.B, c.L, c.d, c.M
    QKV, EE = operand(c.qkv if qkv is None else qkv), operand(c.E if E is None else E)
    PB = None if c.pm is None or Lk is not None else OnesBanded(T.pack_padbits(c.pm))
    CTX, LSE = output((B, L, d), BF), output((B, c.heads, L), F32)
    need = lib.mgx_rel_attn_fwd_workspace(L)
    WS = output((need,), torch.uint8)
    if Lk is None:
        chk(lib.mgx_rel_attn_fwd(P(QKV), P(EE), P(PB), P(CTX), P(LSE), P(WS), need, B, L, d, M, sp()), c.name)
    else:
        chk(lib.mgx_rel_attn_fwd_nomask(P(QKV), P(EE), P(CTX), P(LSE), P(WS), need, B, L, Lk, d, M, sp()), c.name)
    torch.cuda.synchronize()
    assert CTX.bands_intact() and LSE.bands_intact() and WS.bands_intact(), c.name + ": the call wrote outside ctx / lse / its workspace"
    return CTX.t, LSE.t


@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=IDS)
@pytest.mark.parametrize("kind", ("gauss", "rel", "content"))
def test_forward(kind, shape_index):
    """mgx_rel_attn_fwd: ctx and lse per element; on selector data the selecting rows' ctx is the selected v row exactly"""
    run_forward(kind, shape_index)


@pytest.mark.parametrize("shape_index", range(1, len(SHAPES)), ids=IDS[1:])
def test_forward_redo_and_rescale(shape_index):
    """far data (L >= 96: a later key tile exists): a logit 128 nats above the lazy softmax reference, from L = 160 on inside the
    branch-free main loop; the relative selector's rows with delta0 < 32 < i jump by 256 nats in the same way"""
    run_forward("far", shape_index)


def run_forward(kind, shape_index):
    for c in cases_of(kind, shape_index):
        ctx, lse = launch_fwd(c)
        check_bound("fwd ctx", kind, ctx, c.ref.ctx, c.ctx_bound, c.name)
        check_bound("fwd lse", kind, lse, c.ref.lse, c.lse_bound, c.name)
        if c.rows is not None:
            check_equal("fwd ctx", ctx.cpu().to(F64)[c.rows], c.ctx_exact[c.rows], c.name + " selecting rows")


NOMASK = ((2, 32, 1, 32, 32), (2, 32, 1, 33, 19), (1, 96, 3, 97, 37), (1, 96, 2, 96, 96), (2, 160, 1, 260, 101), (2, 160, 2, 160, 160),
          (1, 288, 1, 289, 261), (2, 288, 1, 288, 225))


@pytest.mark.parametrize("B,L,heads,M,Lk", NOMASK)
def test_forward_nomask(B, L, heads, M, Lk):
    """mgx_rel_attn_fwd_nomask: keys j < Lk (also Lk % 32 != 0 and Lk < L - 32), relative term for j <= i only; rows >= Lk are
    don't-cares of the contract (they must still stay inside ctx and lse).  Gaussian data, and the content selector whose rows also
    select keys j > i"""
    c = T.Ref(B=B, L=L, heads=heads, d=64 * heads, M=M, pm=None, name=f"nomask B={B} L={L} h={heads} M={M} Lk={Lk}")
    for kind in ("gauss", "content"):
        if kind == "gauss":
            qkv, E, _ = T.attn_gauss(B, L, heads, M, seed=1)
        else:
            qkv, E, _, sel, rows, ctx_exact, _ = T.attn_selector_content(B, L, heads, M, None, causal=False, Lk=Lk)
            assert (sel[rows] > torch.arange(L)[None, :].expand(B, L)[rows]).any()
        ref = T.rel_attn_fwd(qkv, E, None, heads, M, causal=False, Lk=Lk)
        cb, lb, _ = T.attn_fwd_bounds(ref)
        ctx, lse = launch_fwd(c, qkv, E, Lk)
        check_bound("nomask ctx", kind, ctx[:, :Lk], ref.ctx[:, :Lk], cb[:, :Lk], c.name)
        check_bound("nomask lse", kind, lse[..., :Lk], ref.lse[..., :Lk], lb[..., :Lk], c.name)
        if kind == "content":
            check_equal("nomask ctx", ctx.cpu().to(F64)[rows], ctx_exact[rows], c.name + " selecting rows")


@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=IDS)
@pytest.mark.parametrize("kind", ("gauss", "rel", "content"))
def test_weights(kind, shape_index):
    """mgx_rel_attn_weights on lse_in = fp32(reference lse): per element into a zero-filled buffer, masked entries exactly 0; into a
    buffer filled with a sentinel, every element of a tile above the diagonal (j >= 32 (i // 32 + 1)) comes back untouched and the
    masked entries of the visited tiles are written as 0"""
    lib, chk, _, sp = KC.raw(product_only=True)
    SENTINEL = 7.25
    for c in cases_of(kind, shape_index)[:3]:
        B, L, d, M, h = c.B, c.L, c.d, c.M, c.heads
        lse_in = c.ref.lse.to(F32)
        want = T.attn_weights(c.ref, lse_in)
        bound = T.attn_weights_bound(c.ref, lse_in, want)
        i, j = torch.arange(L)[:, None], torch.arange(L)[None, :]
        beyond = (j >= 32 * (i // 32 + 1)).expand(B, h, L, L)
        for fill in (0.0, SENTINEL):
            QKV, EE, LSE = operand(c.qkv), operand(c.E), operand(lse_in)
            PB = None if c.pm is None else OnesBanded(T.pack_padbits(c.pm))
            W = output(None, F32, torch.full((B, h, L, L), fill))
            need = lib.mgx_rel_attn_fwd_workspace(L)
            WS = output((need,), torch.uint8)
            chk(lib.mgx_rel_attn_weights(P(QKV), P(EE), P(PB), P(LSE), P(W), P(WS), need, B, L, d, M, sp()), c.name)
            torch.cuda.synchronize()
            assert W.bands_intact() and WS.bands_intact(), c.name + ": the call wrote outside weights / its workspace"
            got = W.t.cpu()
            if fill:
                assert (got[beyond] == SENTINEL).all(), c.name + ": a tile above the diagonal was written"
                got = torch.where(beyond, torch.zeros(()), got)
            check_bound("weights", kind, got, want, bound, c.name + f" fill={fill}")
            if kind == "rel":                                    # S = lse = 256: the exponent's argument is exactly 0
                onehot = torch.zeros(B, L, L, dtype=F64).scatter_(2, c.sel[..., None], 1.0)[:, None].expand(B, h, L, L)
                rows = c.rows[:, None, :].expand(B, h, L)
                check_equal("weights", got.to(F64)[rows], onehot[rows], c.name + " selecting rows")


# ---- backward ---------------------------------------------------------------------------------------------------------------------
def launch_bwd(c, ctx_in, lse_in, parts, det=False):
    """mgx_rel_attn_bwd_parts inside bands -> dqkv bf16 [B, L, 3d], dE f32 [M, 64] on the CPU"""
    lib, chk, _, sp = KC.raw(product_only=True)
    B, L, d, M = c.B, c.L, c.d, c.M
    QKV, EE, CTX, DCTX, LSE = operand(c.qkv), operand(c.E), operand(ctx_in), operand(c.dctx), operand(lse_in)
    PB = None if c.pm is None else OnesBanded(T.pack_padbits(c.pm))
    DQKV, DE = output((B, L, 3 * d), BF), output(None, F32, c.dE0)
    need = lib.mgx_rel_attn_bwd_workspace(B, L, d)
    WS = output((need,), torch.uint8)
    with Det(det):
        chk(lib.mgx_rel_attn_bwd_parts(P(QKV), P(EE), P(PB), P(CTX), P(DCTX), P(LSE), P(DQKV), P(DE), P(WS), need, B, L, d, M, parts, sp()),
            c.name)
        torch.cuda.synchronize()
    assert DQKV.bands_intact() and DE.bands_intact() and WS.bands_intact(), c.name + ": the call wrote outside dqkv / dE / its workspace"
    dE = DE.t.cpu()
    assert torch.equal(dE[:M - L].view(torch.int32), c.dE0[:M - L].view(torch.int32)), c.name + ": rows of dE below M - L changed"
    return DQKV.t.cpu(), dE


def check_bwd(c, fam, dqkv, dE, r, bounds, tag=""):
    d, kind, name = c.d, c.kind, c.name + tag
    b, bE = bounds
    for out, lo in (("dq", 0), ("dk", d), ("dv", 2 * d)):
        check_bound(f"{fam} {out}", kind, dqkv[..., lo:lo + d], r.dqkv[..., lo:lo + d], b[..., lo:lo + d], name)
    check_bound(f"{fam} dE", kind, dE, c.dE0.double() + r.dE, bE, name)
    if c.rows is None:
        return
    # the exact answer of the selector data
    got = dqkv.to(F64)
    check_equal(f"{fam} dq", got[..., :d][c.rows], 0.0, name + " selecting rows")
    for bi in range(c.B):
        other = torch.nonzero(~c.rows[bi])
        j0 = int(other.max()) + 1 if other.numel() else 0        # keys from j0 on are visible to selecting rows alone
        check_equal(f"{fam} dk", got[bi, j0:, d:2 * d], 0.0, name + f" b={bi} keys >= {j0}")
        check_equal(f"{fam} dv", got[bi, j0:, 2 * d:], c.dv_exact[bi, j0:], name + f" b={bi} keys >= {j0}")
    if c.rows.all():
        check_equal(f"{fam} dE", dE, c.dE0.double(), name + " start value")


@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=IDS)
@pytest.mark.parametrize("kind", ("gauss", "rel", "content"))
def test_backward(kind, shape_index):
    """mgx_rel_attn_bwd_parts on ctx_in = bf16(reference ctx), lse_in = fp32(reference lse): production (1|4|2|8); where L % 128 == 0
    also the 32-key dK/dV kernel at that shape (1|64|2|8); dQ and dE by recomputation (1|4|32|16)"""
    L = SHAPES[shape_index][1]                                   # bit 4 takes the 64-key asm kernel iff L % 128 == 0 (BwdPlan::dkv64, rel_attn_bwd.hip;
    cases = cases_of(kind, shape_index)                          # tests/test_gpu_kernels.py::test_dkv_falls_back_.. pins that plan): L = 128, 256 here
    for n, c in enumerate(cases):
        ctx_in, lse_in, r, bounds = bwd_ref(c)
        for parts in (PROD, DKV32, RECOMPUTE):
            if parts == DKV32 and L % 128 != 0:
                continue
            if parts != PROD and kind != "gauss" and n % 3 != shape_index % 3:
                continue                                         # the cross-check paths meet a third of the selector cases
            dqkv, dE = launch_bwd(c, ctx_in, lse_in, parts)
            check_bwd(c, PARTS_NAME[parts], dqkv, dE, r, bounds, f" parts={parts}")


@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=IDS)
def test_backward_deterministic(shape_index):
    """production parts in deterministic mode (mgx_set_deterministic): the same bounds, dE included"""
    for c in (cases_of("gauss", shape_index)[0], cases_of("content", shape_index)[shape_index]):
        ctx_in, lse_in, r, bounds = bwd_ref(c)
        dqkv, dE = launch_bwd(c, ctx_in, lse_in, PROD, det=True)
        check_bwd(c, "bwd[deterministic]", dqkv, dE, r, bounds, " deterministic")


@pytest.mark.parametrize("shape_index", range(len(SHAPES)), ids=IDS)
def test_backward_chained(shape_index):
    """forward, then production backward on the kernel's OWN ctx and lse; the reference is evaluated on those"""
    c = cases_of("gauss", shape_index)[1]
    ctx, lse = launch_fwd(c)
    ctx_in, lse_in = ctx.cpu(), lse.cpu()
    r = T.rel_attn_bwd(c.qkv, c.E, c.pm, ctx_in, lse_in, c.dctx, c.heads, c.M)
    dqkv, dE = launch_bwd(c, ctx_in, lse_in, PROD)
    check_bwd(c, "bwd[chained]", dqkv, dE, r, T.attn_bwd_bounds(r, c.B, c.dE0), " chained")


@pytest.mark.parametrize("kind,pads", (("gauss", "trailing"), ("content", "bits")))
def test_backward_eight_batch_rows(kind, pads):
    """B = 8, L = 160, d = 64: the dE groups are dealt across the XCDs, one batch row each; E longer than L"""
    c = make_case(kind, 8, 160, 1, 192, pads)
    ctx, lse = launch_fwd(c)
    check_bound("fwd ctx", kind, ctx, c.ref.ctx, c.ctx_bound, c.name)
    check_bound("fwd lse", kind, lse, c.ref.lse, c.lse_bound, c.name)
    ctx_in, lse_in, r, bounds = bwd_ref(c)
    for parts, det in ((PROD, False), (PROD, True), (RECOMPUTE, False)):
        dqkv, dE = launch_bwd(c, ctx_in, lse_in, parts, det)
        check_bwd(c, PARTS_NAME[parts] + ("[deterministic]" if det else ""), dqkv, dE, r, bounds, f" parts={parts} det={int(det)}")
