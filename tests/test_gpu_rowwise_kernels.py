"""Every entry point of csrc/rowwise_ops.hip (embedding + PE and its backward, pad bitmap, residual + LayerNorm, smoothed cross
entropy, Adam, bf16 cast) against the fp64 reference of its header contract (oracle/train_ref.py), element by element, at the
shapes where such kernels go wrong: partial last 512-column chunks, waves that loop over rows, the clamped prefetch, the scalar
and the vector path of the cross entropy, accumulating outputs that start from nonzero values, rows far from zero.

No bound here is a max-norm bound and none was calibrated against another kernel.
  bf16 output   |got - ref| <= 2^-8 |ref| + C * F      2^-8 |ref| is the output's rounding (half an ulp is 2^-9)
  fp32 output   |got - ref| <= C * F
  integers, masks, the bf16 shadow and cast: exact
F is the family's noise floor (train_ref: the same formula in fp32 with its sums reversed, against fp64, plus one fp32 ulp; for
sums over rows or tokens 2^-24 * sum |terms|).  One C per family absorbs the kernel's summation order and its fast exp / log,
nothing else.  Each is MEASURED on one MI355X as the largest (|err| - rounding term) / F over all cases of this module and set
to twice that, rounded up to a power of two (profiles/r11_rowwise_gru_kernel_tests.txt has the figures and the cases):
  C_LNF  LayerNorm forward     8    measured 2.967 (rstd, rows far from zero, rows 2045, d 2048; mean 1.913, out 0.193)
  C_LNB  LayerNorm backward    4    measured 1.632 (dgamma, rows of very different scale, rows 3, d 2040)
  C_CE   cross entropy         8    measured 3.376 (stats[0], rows 8209, V 513; the sum's atomics arrive in any order: 1.826 in another run)
  C_ADAM Adam                  16   measured 4.626 (p, n 2^21 + 3, step 100000)
  C_EMB  embedding             4    measured 1.810 (dtable, rows 40000, V 5000, d 64, p 0.1)
The LayerNorm forward is checked in stages: mean and rstd against fp64, out against the fp64 formula on the mean and rstd the
kernel saved (one ulp of a mean far from zero, times rstd * |gamma|, is most of a correct kernel's distance from the fp64
LayerNorm and so needs no slack); a constant row must give mean = the constant and out = beta exactly.
Every test prints its largest ratio before it asserts (pytest -s shows them).
"""
import math

import numpy as np
import pytest
import torch

import kernel_checks as KC
from kernel_checks import bits16, nothing_more_after_a_gpu_error  # noqa: F401 (the fixture is used by name)
from oracle import train_ref as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
C = {**KC.C_ROWWISE, "ADAM": KC.C_ADAM}                   # LNF 8, LNB 4, CE 8, EMB 4, ADAM 16: kept in kernel_checks, which tests/step_trace.py reads too
SEEN = {}                                          # family -> (largest ratio this process has seen, its case)
_report = KC.report_fixture(SEEN, "largest ratio {:.3f}")


def check_bf16(fam, got, ref, F, case):
    KC.check_floor(fam, got, ref, F, case, C=C[fam], seen=SEEN, rounding=2.0 ** -8)


def check_f32(fam, got, ref, F, case):
    assert got.dtype == torch.float32
    KC.check_floor(fam, got, ref, F, case, C=C[fam], seen=SEEN)


# =====================================================================================================================
# 1. residual + LayerNorm
# =====================================================================================================================
LN_D = (8, 64, 504, 512, 520, 1024, 1032, 1536, 2040, 2048)       # 1..4 chunks of 512 columns, whole and partial
LN_BIG = {8: 2049, 64: 4100, 504: 6151, 512: 2049, 520: 4100, 1024: 6151, 1032: 2049, 1536: 4100, 2040: 6151, 2048: 2049}


def ln_bwd_raw(dout, x, res, gamma, mean, rstd, dgamma, dbeta, dxsum, p_drop, seed, alias):
    lib, check, ptr, stream_ptr = KC.raw()
    rows, d = x.shape
    dres = torch.empty_like(x)
    dx = dres if alias else torch.empty_like(x)
    ws = torch.empty(lib.mgx_add_ln_bwd_workspace(rows, d), dtype=torch.uint8, device=DEV)
    check(lib.mgx_add_ln_bwd(ptr(dout), ptr(x), ptr(res), ptr(gamma), ptr(mean), ptr(rstd), ptr(dx), ptr(dres), ptr(dgamma),
                             ptr(dbeta), ptr(dxsum), ptr(ws), ws.numel(), rows, d, float(p_drop), int(seed), stream_ptr()),
          "mgx_add_ln_bwd")
    return dx, dres


def run_ln(kind, rows, d, p_drop=0.0, seed=0, init=False, alias=False, want_dxsum=True):
    case = f"{kind} rows={rows} d={d} p={p_drop} init={init} alias={alias}"
    ops = KC.ops()
    x, res = T.ln_case(kind, rows, d, seed)
    g = torch.Generator().manual_seed(seed + d)
    gamma, beta = 1 + 0.5 * torch.randn(d, generator=g), torch.randn(d, generator=g)
    dout = torch.randn(rows, d, generator=g).to(BF)
    mult = T.drop_mult(p_drop, seed, rows * d).reshape(rows, d) if p_drop > 0 else None
    xg, rg, gg, bg, dg = (t.to(DEV) for t in (x, res, gamma, beta, dout))
    out, mean, rstd = ops.add_ln_fwd(xg, rg, gg, bg, 1e-6, p_drop, seed)
    ref = T.add_ln_fwd(x, res, gamma, beta, 1e-6, mult)
    Fm, Fr = T.add_ln_fwd_floor(x, res, gamma, beta, 1e-6, mult, ref)
    check_f32("LNF", mean, ref[0], Fm, case + " mean")
    check_f32("LNF", rstd, ref[1], Fr, case + " rstd")
    # in stages: out against the fp64 formula on the mean / rstd the kernel saved (an ulp of a mean far from zero needs no slack)
    staged = T.add_ln_out(x, res, gamma, beta, mean.cpu(), rstd.cpu(), mult)
    check_bf16("LNF", out, staged, T.add_ln_out_floor(x, res, gamma, beta, mean.cpu(), rstd.cpu(), mult, staged), case + " out")
    if kind == "const":                            # mgx.h: a row of equal elements has mean = that value and out = beta exactly
        assert mean.cpu().equal(x[:, 0].float()), case + ": the mean of a constant row is not the constant"
        assert bits16(out).equal(bits16(beta.to(BF).expand(rows, d))), case + ": a constant row's output is not beta"
    # backward, from the mean / rstd the forward kernel saved
    init_v = [torch.randn(d, generator=g) * (3.0 if init else 0.0) for _ in range(3)]
    dgamma, dbeta, dxsum = (t.clone().to(DEV) for t in init_v)
    dx, dres = ln_bwd_raw(dg, xg, rg, gg, mean, rstd, dgamma, dbeta, dxsum if want_dxsum else None, p_drop, seed, alias)
    mk, rk = mean.cpu(), rstd.cpu()
    rb = T.add_ln_bwd(dout, x, res, gamma, mk, rk, mult)
    Frow, Fg, Fb = T.add_ln_bwd_floor(dout, x, res, gamma, mk, rk, mult, rb)
    check_bf16("LNB", dres, rb[0], Frow, case + " dres")
    check_bf16("LNB", dx, rb[1], Frow, case + " dx")
    if alias:
        assert dx.data_ptr() == dres.data_ptr()
    if mult is not None:
        assert (dx.cpu()[mult == 0] == 0).all(), case + ": a dropped element of dx is not 0"
    for name, got, upd, F, i0 in (("dgamma", dgamma, rb[2], Fg, init_v[0]), ("dbeta", dbeta, rb[3], Fb, init_v[1])):
        tot = i0.double() + upd
        check_f32("LNB", got, tot, F + T.ulp32(torch.maximum(i0.double().abs(), tot.abs())), f"{case} {name}")
    if want_dxsum:                                 # the kernel sums what the consumer reads: its own bf16 dx
        dxk = dx.cpu().double()
        tot = init_v[2].double() + dxk.sum(0)
        check_f32("LNB", dxsum, tot, T.sum_floor(dxk, 0, tot) + T.ulp32(init_v[2].double()), case + " dxsum")
    else:
        assert (dxsum.cpu() == init_v[2]).all()


@pytest.mark.parametrize("kind", T.LN_KINDS)
@pytest.mark.parametrize("d", LN_D)
def test_layernorm_against_fp64_at_every_chunk_count_and_row_count(d, kind):
    """rows 1, 3, 5 (partial last workgroup) and one of 2049 / 4100 / 6151 per width: above 2048 rows the backward's waves loop
    and their prefetch of the row after the last is clamped"""
    big = kind in ("zero-mean", "far") or d in (520, 2048)
    for rows in (1, 3, 5) + ((LN_BIG[d],) if big else (9,)):
        run_ln(kind, rows, d)


@pytest.mark.parametrize("d", (64, 520, 2048))
@pytest.mark.parametrize("kind", ("zero-mean", "far"))
def test_layernorm_backward_accumulates_into_nonzero_gradients_and_may_alias(d, kind):
    for rows in (5, 2049, 511 * 4 + 1):                   # 512 blocks' partials; 2045 rows: 512 blocks, the last one with one row
        run_ln(kind, rows, d, init=True, alias=True)
        run_ln(kind, rows, d, init=True, alias=False, want_dxsum=False)
    run_ln(kind, 4 * 77, d, init=True)                    # 77 blocks: ln_finish's tail loop (nblk not a multiple of 128)
    run_ln(kind, 4 * 200 + 2, d, init=True)               # 201 blocks: one unrolled round + tail


@pytest.mark.parametrize("p_drop", (0.1, 0.5))
@pytest.mark.parametrize("d", (8, 520, 1536, 2048))
def test_layernorm_with_dropout_uses_the_twins_mask_forward_and_backward(d, p_drop):
    for rows, seed in ((3, 1), (4100, (1 << 32) + 9)):
        run_ln("zero-mean", rows, d, p_drop=p_drop, seed=seed, init=True)
        if p_drop == 0.5:                                     # scale = 2: x * scale + res is still exact in fp32 (at p = 0.1 the product
            run_ln("far", rows, d, p_drop=p_drop, seed=seed)  # is not, and z - mean magnifies its rounding: fp32's doing, not a kernel's)


# =====================================================================================================================
# 2. smoothed cross entropy
# =====================================================================================================================
CE_V = (7, 8, 9, 511, 512, 513, 1024, 1025, 2040, 2048, 2049)
EPS_LS = 0.1


def ce_lds(V):
    return sorted({V, (V + 7) // 8 * 8, (V + 127) // 128 * 128})


def ce_fwd_raw(logits, target, stats, V, ld, pad):
    lib, check, ptr, stream_ptr = KC.raw()
    rows = target.numel()
    argmax = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    lse = torch.full((rows,), float("nan"), dtype=torch.float32, device=DEV)
    check(lib.mgx_smooth_ce_fwd(ptr(logits), ptr(target), ptr(stats), ptr(argmax), ptr(lse), rows, V, ld, float(EPS_LS), int(pad),
                                stream_ptr()), "mgx_smooth_ce_fwd")
    return argmax, lse


def on_device(t, off):
    """a device copy of t whose base pointer is ``off`` elements past an aligned allocation"""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (2 * off) % 16
    return v


def run_ce(kind, rows, V, ld, off=0, fill=float("nan"), init=False, gscale=1.0, gdev=None, all_pad=False, seed=0):
    case = f"{kind} rows={rows} V={V} ld={ld} off={off} fill={fill} init={init} g={gscale}/{gdev} all_pad={all_pad}"
    ops = KC.ops()
    pad = V - 2 if V > 2 else 0
    logits = T.ce_logits(kind, rows, V, ld, seed, fill)
    target = torch.full((rows,), pad, dtype=torch.int32) if all_pad else T.ce_targets(rows, V, pad, seed)
    s0 = torch.tensor([2.5, 3.0, 1.0, 4.0] if init else [0.0] * 4)
    lg, tg, stats = on_device(logits, off), target.to(DEV), s0.clone().to(DEV)
    argmax, lse = ce_fwd_raw(lg, tg, stats, V, ld, pad)
    ref = T.smooth_ce_fwd(logits, target, V, EPS_LS, pad)
    Fl, Fs = T.smooth_ce_fwd_floor(logits, target, V, EPS_LS, pad, ref)
    assert (argmax.cpu().long() == ref[1]).all(), f"{case}: arg-max differs at rows {torch.nonzero(argmax.cpu().long() != ref[1])[:4].tolist()}"
    check_f32("CE", lse, ref[0], Fl, case + " lse")
    sk = stats.cpu()
    tot = s0.double() + ref[2]
    assert (sk[1:].double() == tot[1:]).all(), (case, sk, tot)                 # counts: exact
    check_f32("CE", sk[:1], tot[:1], (Fs + T.ulp32(torch.maximum(s0[0].double().abs(), tot[0].abs()))).reshape(1), case + " stats[0]")
    if all_pad:
        assert sk[1] == s0[1] and sk[0] == s0[0]
    # backward, from the lse and the count the forward kernel left
    gd = None if gdev is None else torch.tensor([gdev], dtype=torch.float32, device=DEV)
    dl = ops.smooth_ce_bwd(lg, tg, stats, lse, V, EPS_LS, pad, gscale, gd)
    gtot = float(np.float32(gscale)) * (1.0 if gdev is None else float(np.float32(gdev)))
    cnt = float(sk[1])
    rb = T.smooth_ce_bwd(logits, target, cnt, lse.cpu(), V, ld, EPS_LS, pad, gtot)
    Fb = T.smooth_ce_bwd_floor(logits, target, cnt, lse.cpu(), V, ld, EPS_LS, pad, gtot, rb)
    check_bf16("CE", dl, rb, Fb, case + " dlogits")
    dlc = dl.cpu()
    assert (dlc[:, V:] == 0).all() and (dlc[target == pad] == 0).all(), case + ": padding columns / pad rows of dlogits are not 0"
    return argmax.cpu(), lse.cpu(), sk, dlc


@pytest.mark.parametrize("kind", ("gauss", "pm80", "equal", "last"))
@pytest.mark.parametrize("V", CE_V)
def test_cross_entropy_against_fp64_on_the_vector_and_the_scalar_path(V, kind):
    """every ld of V, V rounded up to 8 and to 128; a base pointer off by one element (the scalar path, as V > 2048 and
    ld % 8 != 0 are); NaN in the padding columns throughout"""
    for ld in ce_lds(V):
        for rows in (1, 17):
            for off in (0, 1):
                run_ce(kind, rows, V, ld, off)


@pytest.mark.parametrize("V", (9, 513, 1024, 2049))
def test_cross_entropy_with_waves_that_loop_over_rows(V):
    """8209 rows: more than the 512 * 16 waves of the forward and the 2048 * 4 of the backward"""
    run_ce("gauss", 8209, V, (V + 7) // 8 * 8, init=True, gscale=0.5, gdev=3.0)


@pytest.mark.parametrize("V,ld", ((7, 8), (513, 520), (513, 640), (1025, 1152), (2049, 2176)))
def test_cross_entropy_ignores_the_padding_columns_bit_for_bit(V, ld):
    for off in (0, 1):
        base = run_ce("gauss", 17, V, ld, off, fill=0.0)
        for fill in (float("nan"), float("inf")):
            other = run_ce("gauss", 17, V, ld, off, fill=fill)
            for a, b in zip(base, other):
                assert KC.bits(a).equal(KC.bits(b)), (V, ld, off, fill)


@pytest.mark.parametrize("V,ld", ((9, 16), (600, 600), (600, 640), (2049, 2049)))
def test_cross_entropy_accumulates_scales_and_handles_an_all_pad_batch(V, ld):
    for gscale, gdev in ((1.0, None), (0.25, None), (0.5, 3.0), (1.0, 0.125)):
        run_ce("gauss", 17, V, ld, init=True, gscale=gscale, gdev=gdev)
    for init in (False, True):                            # every target is pad: dlogits exactly zero, stats[0..1] unchanged
        _, _, _, dl = run_ce("gauss", 17, V, ld, init=init, all_pad=True)
        assert (bits16(dl) == 0).all()


# =====================================================================================================================
# 3. Adam, bf16 cast
# =====================================================================================================================
@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 7, 1031, 2 * 2 ** 20 + 3, 4 * 2 ** 20 + 5))
@pytest.mark.parametrize("with_shadow", (True, False))
def test_adam_against_fp64_with_the_state_carried_across_steps(n, with_shadow):
    """4 * 2^20 + 5 elements: more float4 groups than the 2048 * 256 threads, so the grid loops; n % 4 != 0: the tail"""
    ops = KC.ops()
    lr, b1, b2, eps, gs = 1e-3, 0.9, 0.98, 1e-9, 0.5
    g = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=g).to(DEV)
    m, v = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    shadow = torch.zeros(n, dtype=BF, device=DEV) if with_shadow else None
    for step in (1, 2, 10, 1000, 100000):
        grad = torch.randn(n, generator=g)
        sel = torch.randint(0, 8, (n,), generator=g)
        grad[sel == 0] = 0.0                                  # g = 0
        grad[sel == 1] = 1e-30                                # g^2 underflows in fp32
        grad[sel == 2] = 1e18                                 # large
        if n <= 7:
            grad[-1] = (0.0, 1e-30, 1e18, 1.5, -2.0)[step % 5]
        p0, m0, v0 = p.cpu(), m.cpu(), v.cpu()
        ops.adam_step(p, grad.to(DEV), m, v, shadow, lr, b1, b2, eps, step, gs)
        ref = T.adam_step(p0, grad, m0, v0, lr, b1, b2, eps, step, gs)
        F = T.adam_floor(p0, grad, m0, v0, lr, b1, b2, eps, step, gs, ref)
        case = f"n={n} step={step} shadow={with_shadow}"
        check_f32("ADAM", p, ref[0], F[0], case + " p")
        check_f32("ADAM", m, ref[1], F[1], case + " m")
        check_f32("ADAM", v, ref[2], F[2], case + " v")
        if with_shadow:
            assert bits16(shadow).equal(bits16(p.to(BF))), case + ": shadow is not the bf16 rounding of p"


def test_adam_without_gradient_scale_is_the_plain_update():
    ops = KC.ops()
    for n in (3, 1031):
        g = torch.Generator().manual_seed(n)
        p0, grad, m0, v0 = torch.randn(n, generator=g), torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g), torch.rand(n, generator=g)
        p, m, v = p0.to(DEV), m0.to(DEV), v0.to(DEV)
        ops.adam_step(p, grad.to(DEV), m, v, None, 2e-3, 0.9, 0.999, 1e-8, 7, 1.0)
        ref = T.adam_step(p0, grad, m0, v0, 2e-3, 0.9, 0.999, 1e-8, 7, 1.0)
        F = T.adam_floor(p0, grad, m0, v0, 2e-3, 0.9, 0.999, 1e-8, 7, 1.0, ref)
        for name, got, r, f in zip("pmv", (p, m, v), ref, F):
            check_f32("ADAM", got, r, f, f"gscale=1 n={n} {name}")


@pytest.mark.parametrize("n", (1, 7, 2 ** 19 + 13))
def test_cast_bf16_is_torchs_rounding_bit_for_bit(n):
    """2^19 + 13 elements: more than the 2048 * 256 threads, so the grid loops"""
    ops = KC.ops()
    g = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=g)
    special = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20, 1e-40, -1e-40, 2.0 ** -133,
                            3 * 2.0 ** -134, float("inf"), float("-inf"), float("nan"), 3.3895e38, 0.0, -0.0])
    k = min(n, special.numel())
    p[n - k:] = special[:k]                                   # at the end: the elements of the looping threads when n is large
    if n == 7:
        p[:7] = special[4:11]
    if n == 1:
        p[0] = special[10]
    shadow = torch.zeros(n, dtype=BF, device=DEV)
    ops.cast_bf16(p.to(DEV), shadow)
    want = p.to(BF)
    nan = torch.isnan(p)                                      # torch's own CPU cast gives 0x7FC0 or 0xFFFF for a NaN, by code path:
    assert nan.any() and torch.isnan(shadow.cpu()[nan].float()).all()      # a NaN stays a NaN, whichever
    bad = torch.nonzero((bits16(shadow) != bits16(want)) & ~nan).reshape(-1)
    assert bad.numel() == 0, [(p[i].item(), hex(bits16(shadow)[i].item() & 0xFFFF), hex(bits16(want)[i].item() & 0xFFFF)) for i in bad[:8]]


# =====================================================================================================================
# 4. embedding + PE, its backward, the pad bitmap
# =====================================================================================================================
def pe_table(L, d):
    from oracle import ref_cpu as R
    return R.sinusoid_table(L, d).float()


@pytest.mark.parametrize("p_drop", (0.0, 0.1))
@pytest.mark.parametrize("B,L,d,V", ((3, 32, 8, 11), (2, 64, 520, 337), (4, 2048, 520, 337)))
def test_embedding_forward_against_fp64(B, L, d, V, p_drop):
    """B > 1: row r reads pe[r % L]; 4 * 2048 rows of 65 groups: more than the 2048 * 256 threads, so the grid loops"""
    ops = KC.ops()
    seed = (1 << 33) + 17
    g = torch.Generator().manual_seed(B * L + d)
    tok = torch.randint(0, V, (B, L), generator=g).to(torch.int32)
    tok[0, 0], tok[-1, -1] = V - 1, 0
    table, pe = torch.randn(V, d, generator=g), pe_table(L, d)
    mult = T.drop_mult(p_drop, seed, B * L * d).reshape(B * L, d) if p_drop > 0 else None
    out = ops.embed_pe_fwd(tok.to(DEV), table.to(DEV), pe.to(DEV), p_drop, seed)
    ref = T.embed_pe_fwd(tok, table, pe, L, mult)
    F = T.embed_pe_fwd_floor(tok, table, pe, L, mult, ref)
    check_bf16("EMB", out.reshape(B * L, d), ref, F, f"fwd B={B} L={L} d={d} p={p_drop}")
    if mult is not None:
        assert (out.cpu().reshape(B * L, d)[mult == 0] == 0).all()


# (B, L, V, d, every token the same): rows 192 .. 40000; 16384 rows -> two token ranges, 40000 rows and V = 337 -> four (the atomic
# path); V = 5000 keeps one range of ten 4096-token chunks; d > 512: a second column pass; one token in all 4097 rows fills the hit list
EMB_BWD = ((2, 96, 3, 64, False), (1, 4097, 3, 512, True), (4, 4096, 337, 520, False), (10, 4000, 5000, 64, False),
           (10, 4000, 337, 512, False), (4, 4096, 3, 1024, False))


def run_embed_bwd(B, L, V, d, same, p_drop, det):
    ops = KC.ops()
    seed, rows = 77, B * L
    g = torch.Generator().manual_seed(rows + V + d)
    tok = (torch.ones(B, L, dtype=torch.int64) if same else torch.randint(0, V - 1, (B, L), generator=g)).to(torch.int32)
    assert not (tok == V - 1).any()                           # token V - 1 never occurs
    dout = torch.randn(B, L, d, generator=g).to(BF)
    init = torch.randn(V, d, generator=g)
    mult = T.drop_mult(p_drop, seed, rows * d).reshape(rows, d) if p_drop > 0 else None
    dtable = init.clone().to(DEV)
    ops.embed_bwd(tok.to(DEV), dout.to(DEV), dtable, p_drop, seed)
    upd, S = T.embed_bwd(tok, dout, V, mult)
    tot = init.double() + upd
    F = T.EPS32 * S + T.ulp32(torch.maximum(init.double().abs(), tot.abs()))
    if det:                                                   # every addend is rounded to the mode's quantum 2^-30 (mgx.h) before it is summed
        hits = torch.bincount(tok.reshape(-1).long(), minlength=V).double()
        F = F + hits[:, None] * 2.0 ** -31 * math.sqrt(d)
    check_f32("EMB", dtable, tot, F, f"bwd rows={rows} V={V} d={d} same={same} p={p_drop} det={det}")
    got = dtable.cpu()
    assert got[V - 1].view(torch.int32).equal(init[V - 1].view(torch.int32)), "the row of a token that never occurs was touched"
    if same:
        assert got[0].view(torch.int32).equal(init[0].view(torch.int32)) and got[2:].view(torch.int32).equal(init[2:].view(torch.int32))


@pytest.mark.parametrize("p_drop", (0.0, 0.1))
@pytest.mark.parametrize("B,L,V,d,same", EMB_BWD)
def test_embedding_backward_against_fp64(B, L, V, d, same, p_drop):
    run_embed_bwd(B, L, V, d, same, p_drop, det=False)


@pytest.mark.parametrize("p_drop", (0.0, 0.1))
@pytest.mark.parametrize("B,L,V,d,same", EMB_BWD)
def test_embedding_backward_against_fp64_in_deterministic_mode(B, L, V, d, same, p_drop):
    ops = KC.ops()
    ops.set_deterministic(True, DEV)
    try:
        run_embed_bwd(B, L, V, d, same, p_drop, det=True)
    finally:
        ops.set_deterministic(False)


@pytest.mark.parametrize("B,L", ((1, 32), (3, 32), (1, 96), (2049, 32), (3, 21856)))
def test_pad_bitmap_words_are_exact(B, L):
    """B * L of 32, 96 and 64 k + 32 tokens: a wave whose upper half, or all but its first 32 lanes, lies past the end"""
    ops = KC.ops()
    pad = 5
    g = torch.Generator().manual_seed(B * L)
    tok = torch.randint(0, 9, (B, L), generator=g).to(torch.int32)
    tok[:, 0] = 1                                             # no leading pad
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    bits = ops.pad_bitmap(tok.to(DEV), pad, flag).cpu()
    isp = (tok == pad).numpy().reshape(B, L // 32, 32).astype(np.uint64)
    want = (isp << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    assert bits.shape == (B, L // 32) and (bits.numpy().view(np.uint32) == want).all()
    assert flag.item() == 0


def test_pad_bitmap_flag_is_raised_by_a_real_token_after_a_leading_pad_only():
    ops = KC.ops()
    pad, L = 5, 64
    rows = {"trailing": [1] * 40 + [pad] * 24, "interior": [1, pad, pad, 1] * 16, "all-pad": [pad] * L,
            "leading": [pad] + [1] * 63, "leading-late": [pad] * 63 + [1]}
    for names, want in ((("trailing", "interior", "all-pad"), 0), (("trailing", "leading"), 1), (("all-pad", "leading-late", "interior"), 1),
                        (("leading",), 1), (("all-pad",), 0)):
        tok = torch.tensor([rows[n] for n in names], dtype=torch.int32)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.pad_bitmap(tok.to(DEV), pad, flag)
        assert flag.item() == want, names
    flag = torch.tensor([1], dtype=torch.int32, device=DEV)   # sticky
    ops.pad_bitmap(torch.tensor([rows["trailing"]], dtype=torch.int32).to(DEV), pad, flag)
    assert flag.item() == 1

