"""oracle/train_ref.py (the fp64 references of the row-wise and GRU training kernels) against independent fp64 computations:
torch's own layer_norm / GRUCell / Adam / index_add_ and autograd, oracle.ref_cpu.smooth_ce, and hand-computed words of the
dropout hash; the attention references against oracle.ref_cpu.attn_core in fp64 and its autograd.  Also the preconditions of the
inputs the GPU tests build.  No GPU."""
import math

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from oracle import train_ref as T

F64 = torch.float64
BF = torch.bfloat16


def close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a).to(F64), torch.as_tensor(b).to(F64)
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), (a - b).abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["zero-mean", "far", "scales"])
@pytest.mark.parametrize("rows,d", [(5, 8), (7, 520), (3, 2048)])
def test_layernorm_forward_and_backward_are_torch_layer_norm_and_its_autograd(kind, rows, d):
    x, res = T.ln_case(kind, rows, d)
    g = torch.Generator().manual_seed(d)
    gamma, beta = 1 + 0.5 * torch.randn(d, generator=g), torch.randn(d, generator=g)
    dout = torch.randn(rows, d, generator=g).to(BF)
    mult = T.drop_mult(0.5, 11, rows * d).reshape(rows, d)
    eps = float(np.float32(1e-6))
    xa, ra = x.double().requires_grad_(), res.double().requires_grad_()
    ga, ba = gamma.double().requires_grad_(), beta.double().requires_grad_()
    out = torch.nn.functional.layer_norm(xa * mult.double() + ra, (d,), ga, ba, eps)
    out.backward(dout.double())
    mean, rstd, ref = T.add_ln_fwd(x, res, gamma, beta, 1e-6, mult)
    close(ref, out.detach())
    z = x.double() * mult.double() + res.double()
    close(mean, z.mean(-1))
    close(rstd, 1 / torch.sqrt(z.var(-1, unbiased=False) + eps))
    dres, dx, dgamma, dbeta, dxsum = T.add_ln_bwd(dout, x, res, gamma, mean, rstd, mult)
    close(dres, ra.grad, 1e-10)
    close(dx, xa.grad, 1e-10)
    close(dgamma, ga.grad, 1e-10)
    close(dbeta, ba.grad)
    close(dxsum, xa.grad.sum(0), 1e-10)
    # the floors: positive, and at fp32 distance
    Fm, Fr = T.add_ln_fwd_floor(x, res, gamma, beta, 1e-6, mult, (mean, rstd, ref))
    assert Fm.shape == (rows,) and Fm.min() > 0 and Fr.min() > 0
    # the staged form: on the exact mean / rstd it is the LayerNorm; on fp32-rounded ones its own, nearby, value
    close(T.add_ln_out(x, res, gamma, beta, mean, rstd, mult), ref)
    staged = T.add_ln_out(x, res, gamma, beta, mean.float(), rstd.float(), mult)
    Fo = T.add_ln_out_floor(x, res, gamma, beta, mean.float(), rstd.float(), mult, staged)
    assert Fo.shape == (rows,) and Fo.min() > 0 and (Fo / (staged.abs().amax(-1) + 1)).max() < 2 ** -18
    # half an ulp of the mean through rstd * |gamma|, half an ulp of rstd through |xhat gamma|
    assert ((staged - ref).abs() <= (T.ulp32(mean) * rstd)[:, None] * gamma.double().abs() + 2 ** -23 * (ref - beta.double()).abs() + 1e-13).all()
    Frow, Fg, Fb = T.add_ln_bwd_floor(dout, x, res, gamma, mean, rstd, mult, (dres, dx, dgamma, dbeta, dxsum))
    assert Frow.shape == (rows,) and Fg.shape == (d,) and min(Frow.min(), Fg.min(), Fb.min()) > 0


@pytest.mark.parametrize("rows,d", [(1, 8), (5, 504), (2049, 64), (33, 2048)])
def test_layernorm_case_preconditions(rows, d):
    x, res = T.ln_case("far", rows, d)
    xf, rf = x.float(), res.float()
    assert ((xf + rf).double() == xf.double() + rf.double()).all()           # x + res is exact in fp32
    assert xf.abs().min() >= 16 and xf.abs().max() <= 60 and (xf == xf[:, :1]).all()
    if rows * d >= 2048:
        assert 0.2 < rf.std().item() < 0.3
    m2 = T.drop_mult(0.5, 9, rows * d).reshape(rows, d)      # p = 0.5: scale 2, the dropped-out sum is exact too
    assert ((xf * m2 + rf).double() == xf.double() * m2.double() + rf.double()).all() and set(m2.unique().tolist()) <= {0.0, 2.0}
    x, res = T.ln_case("const", rows, d)
    assert (x == x[:, :1]).all() and (res == 0).all()
    assert (x.float() * 4 == (x.float() * 4).round()).all() and x.float().abs().max() <= 10     # d <= 2048 copies sum exactly in fp32
    mean, rstd, out = T.add_ln_fwd(x, res, torch.ones(d), torch.full((d,), 0.5), 1e-6)
    close(mean, x[:, 0].double())
    close(rstd, torch.full((rows,), 1 / math.sqrt(float(np.float32(1e-6))), dtype=F64))
    assert (out == 0.5).all()
    x, res = T.ln_case("scales", 18, d)
    amax = (x.float() + res.float()).abs().amax(-1)
    assert amax.max() / amax.min() > 2 ** 20


# ---------------------------------------------------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "pm80", "equal", "last"])
@pytest.mark.parametrize("V,ld", [(7, 8), (513, 640), (2049, 2049)])
def test_cross_entropy_is_ref_cpu_smooth_ce_and_its_autograd(kind, V, ld):
    rows, eps_ls, pad = 17, 0.1, V - 2
    logits = T.ce_logits(kind, rows, V, ld, fill=float("nan"))
    target = T.ce_targets(rows, V, pad)
    lse, am, stats, loss = T.smooth_ce_fwd(logits, target, V, eps_ls, pad)
    x = logits[:, :V].double().requires_grad_()
    close(lse, torch.logsumexp(x, -1).detach())
    e = float(np.float32(eps_ls))
    q = torch.full((rows, V), e / V, dtype=F64)
    q[torch.arange(rows), target.long()] += 1 - e
    per = -(q * torch.log_softmax(x, -1)).sum(-1)                            # the definition, not the closed form
    close(loss, per.detach(), 1e-9)
    keep = target != pad
    close(stats, torch.tensor([per[keep].sum().item(), keep.sum().item(), (x.argmax(-1) == target).sum().item(), rows], dtype=F64), 1e-9)
    want = R.smooth_ce(logits[:, :V].float(), target, e, V, pad)              # fp32 inside
    assert abs(stats[0].item() / stats[1].item() - want.item()) <= 1e-5 * max(1.0, abs(want.item()))
    (per[keep].sum() / keep.sum() * 0.25).backward()
    got = T.smooth_ce_bwd(logits, target, stats[1].item(), lse, V, ld, eps_ls, pad, 0.25)
    close(got[:, :V], x.grad, 1e-9)
    assert (got[:, V:] == 0).all() and (got[~keep] == 0).all() and torch.isfinite(got).all()
    xr = logits[:, :V].float().requires_grad_()
    (R.smooth_ce(xr, target, e, V, pad) * 0.25).backward()
    assert (got[:, :V] - xr.grad.double()).abs().max() <= 1e-6
    # first-index arg-max
    if kind == "equal":
        assert (am == 0).all()
    if kind == "last":
        assert (am == V - 1).all()
    if kind == "pm80":
        first = [int(np.nonzero(r == 80)[0][0]) if (r == 80).any() else 0 for r in logits[:, :V].float().numpy()]
        assert am.tolist() == first
    Fl, Fs = T.smooth_ce_fwd_floor(logits, target, V, eps_ls, pad, (lse, am, stats, loss))
    assert Fl.min() > 0 and Fs > 0 and Fl.max() < 2 ** -14
    Fb = T.smooth_ce_bwd_floor(logits, target, stats[1].item(), lse, V, ld, eps_ls, pad, 0.25, got)
    assert Fb.shape == (rows,) and Fb.min() > 0


def test_cross_entropy_all_pad_batch_and_target_preconditions():
    V, pad = 600, 5
    logits = T.ce_logits("gauss", 4, V, V)
    target = torch.full((4,), pad, dtype=torch.int32)
    lse, am, stats, _ = T.smooth_ce_fwd(logits, target, V, 0.1, pad)
    assert stats[0] == 0 and stats[1] == 0 and stats[3] == 4
    assert (T.smooth_ce_bwd(logits, target, 0.0, lse, V, V, 0.1, pad, 1.0) == 0).all()
    t = T.ce_targets(17, V, pad)
    assert {0, V - 1, pad, 511, 512} <= set(t.tolist())
    t = T.ce_targets(8209, 9, 3)
    assert {0, 8, 3} <= set(t.tolist()) and 0.05 < (t == 3).float().mean() < 0.3
    for kind in ("gauss", "pm80", "equal", "last"):
        x = T.ce_logits(kind, 5, 9, 16, fill=float("inf"))
        assert torch.isfinite(x[:, :9]).all() and torch.isinf(x[:, 9:]).all()
        assert (x.float().to(BF) == x).all()


# ---------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------
def test_adam_is_torch_optim_adam_on_float64_parameters():
    g = torch.Generator().manual_seed(0)
    n, lr, b1, b2, eps, gs = 37, 1e-3, 0.9, 0.98, 1e-9, 0.5
    f = lambda a: float(np.float32(a))                                                              # noqa: E731
    p0 = torch.randn(n, generator=g)
    pt = p0.double().clone().requires_grad_()
    opt = torch.optim.Adam([pt], lr=f(lr), betas=(f(b1), f(b2)), eps=f(eps))
    p, m, v = p0.double(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    for step in range(1, 8):
        grad = torch.randn(n, generator=g)
        pt.grad = grad.double() * f(gs)
        opt.step()
        p, m, v, _ = T.adam_step(p, grad, m, v, lr, b1, b2, eps, step, gs)
        close(p, pt.detach(), 1e-13)
    st = opt.state[pt]
    close(m, st["exp_avg"], 1e-13)
    close(v, st["exp_avg_sq"], 1e-13)
    Fp, Fm, Fv = T.adam_floor(p0, grad, m.float(), v.float(), lr, b1, b2, eps, 8, gs,
                              T.adam_step(p0, grad, m.float(), v.float(), lr, b1, b2, eps, 8, gs))
    assert min(Fp.min(), Fm.min(), Fv.min()) > 0 and (Fp / (p0.abs().double() + 1e-3)).max() < 2 ** -18


# ---------------------------------------------------------------------------------------------------------------------
# embedding, scatter
# ---------------------------------------------------------------------------------------------------------------------
def test_embedding_forward_backward_and_scatter_are_index_select_and_index_add():
    g = torch.Generator().manual_seed(3)
    B, L, d, V = 3, 32, 24, 11
    tok = torch.randint(0, V - 1, (B, L), generator=g).to(torch.int32)       # token V - 1 never occurs
    table = torch.randn(V, d, generator=g)
    pe = R.sinusoid_table(L, d).float()
    mult = T.drop_mult(0.1, 5, B * L * d).reshape(B * L, d)
    ta = table.double().requires_grad_()
    out = (ta[tok.long().reshape(-1)] * math.sqrt(d) + pe.double().repeat(B, 1)) * mult.double()
    ref = T.embed_pe_fwd(tok, table, pe, L, mult)
    close(ref, out.detach())
    dout = torch.randn(B * L, d, generator=g).to(BF)
    out.backward(dout.double())
    upd, S = T.embed_bwd(tok, dout, V, mult)
    close(upd, ta.grad)
    assert (upd[V - 1] == 0).all() and (S >= upd.abs() - 1e-12).all()
    assert T.embed_pe_fwd_floor(tok, table, pe, L, mult, ref).min() > 0
    idx = torch.tensor([0, 3, 3, -1, V, 3, 10], dtype=torch.int32)
    src = torch.randn(7, 16, generator=g).to(BF)
    upd, S = T.scatter_add_rows(idx, src, V, 12)
    want = torch.zeros(V, 12, dtype=F64).index_add_(0, torch.tensor([0, 3, 3, 3, 10]), src[[0, 1, 2, 5, 6], :12].double())
    close(upd, want)
    close(S[3], src[[1, 2, 5], :12].double().abs().sum(0))


# ---------------------------------------------------------------------------------------------------------------------
# GRU cell
# ---------------------------------------------------------------------------------------------------------------------
def test_gru_cell_is_torch_grucell_and_its_autograd():
    g = torch.Generator().manual_seed(4)
    B, H, K = 5, 24, 16
    cell = torch.nn.GRUCell(K, H).double()
    x, h = torch.randn(B, K, generator=g).double(), torch.randn(B, H, generator=g).double().requires_grad_()
    gi = (x @ cell.weight_ih.T + cell.bias_ih).detach().requires_grad_()
    gh = (h @ cell.weight_hh.T + cell.bias_hh).detach().requires_grad_()
    want = cell(x, h)
    ref = T.gru_cell_fwd(gi.detach(), gh.detach(), h.detach())
    close(ref, want.detach())
    dh = torch.randn(B, H, generator=g).double()
    # autograd of the cell formula with gi, gh and h as leaves
    r, z, n, _ = T._gates(gi, gh, F64)
    hl = h.detach().requires_grad_()
    ((1 - z) * n + z * hl).backward(dh)
    dgi, dgh, dhp = T.gru_cell_bwd(gi.detach(), gh.detach(), h.detach(), dh)
    close(dgi, gi.grad)
    close(dgh, gh.grad)
    close(dhp, hl.grad)
    # and through torch's own cell: dh/dh_prev = direct + dgh @ W_hh
    want.backward(dh)
    close(dhp + dgh @ cell.weight_hh.detach(), h.grad)
    c = T.gru_cell_coef(gi.detach(), gh.detach(), h.detach())
    close(torch.cat([dh * c["r"], dh * c["z"], dh * c["n"]], 1), dgi)
    close(torch.cat([dh * c["r"], dh * c["z"], dh * c["nr"]], 1), dgh)
    close(dh * c["h"], dhp)
    assert T.gru_cell_fwd_floor(gi.detach(), gh.detach(), h.detach(), ref).min() > 0
    assert T.gru_cell_bwd_floor(gi.detach(), gh.detach(), h.detach(), dh, (dgi, dgh, dhp)).shape == (B,)
    pr, S = T.proj(h.detach(), cell.weight_hh.detach(), cell.bias_hh.detach())
    close(pr, gh.detach())
    assert (S >= pr.abs() - 1e-12).all() and T.proj_floor(h.detach(), cell.weight_hh.detach(), cell.bias_hh.detach(), pr, S).min() > 0
    assert (T.bf16_round(torch.tensor([1.0 + 2 ** -8, 1.0 + 3 * 2 ** -8])) == torch.tensor([1.0, 1.0 + 2 ** -6], dtype=F64)).all()


# ---------------------------------------------------------------------------------------------------------------------
# dropout twin
# ---------------------------------------------------------------------------------------------------------------------
def test_dropout_twin_constants_hash_words_and_keep_rate():
    assert T.make_drop(0.0, 99) == (0, 0, np.float32(1.0))
    thr, mix, scale = T.make_drop(0.1, 0)
    assert (thr, mix) == (6554, 0xF9A08D56) and scale == np.float32(65536.0 / 58982.0) and scale.dtype == np.float32
    assert T.make_drop(0.5, 1) == (32768, 0x97D8070F, np.float32(2.0))
    assert T.make_drop(0.99999, 1234) == (65535, 0xA1094B18, np.float32(65536.0))
    assert T.make_drop(0.5, (1 << 32) + 5)[1] == 0x4E033FBE                   # a seed above 2^32: the high word enters
    assert T.make_drop(0.5, 0x123456789ABCDEF0)[1] == 0x9DD7B08E
    assert T.make_drop(0.5, 5)[1] != T.make_drop(0.5, (1 << 32) + 5)[1]
    words = {0: 0, 1: 0x688990C0, 2: 0xD1132181, 0xFFFFFFFF: 0x6768824A, 0x12345678: 0xF5E71C96}
    assert T.hash32(list(words)).tolist() == list(words.values())
    # element e of group g: 16-bit half (e % 2) of hash32((4 g + e // 2) ^ mix)
    cfg = T.make_drop(0.5, 7)
    m8 = T.drop_mult8(cfg, [0, 5, 2 ** 32 + 5])
    assert (m8[1] == m8[2]).all()                                             # the group index is taken mod 2^32
    for k in range(8):
        r = int(T.hash32([(4 * 5 + k // 2) ^ cfg[1]])[0])
        half = (r >> 16) if k % 2 else (r & 0xFFFF)
        assert m8[1, k] == (0.0 if half < cfg[0] else 2.0)
    for p in (0.1, 0.5, 0.99999):
        m = T.drop_mult(p, 42, 1 << 20)
        thr, _, scale = T.make_drop(p, 42)
        assert set(m.unique().tolist()) <= {0.0, float(scale)}
        keep = (m != 0).float().mean().item()
        assert abs(keep - (1 - thr / 65536)) < 4 * math.sqrt(0.25 / (1 << 20)) + 1e-6, (p, keep)
    assert (T.drop_mult(0.0, 42, 64) == 1).all()
    assert (T.drop_mult(0.5, 42, 1 << 12)[:64] == T.drop_mult(0.5, 42, 64)).all()


# ---------------------------------------------------------------------------------------------------------------------
# the training GEMMs (tests/test_gpu_gemm_kernels.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", T.GEMM_KINDS)
def test_gemm_references_are_autograd_of_relu_linear_in_float64(kind):
    """linear_fwd / linear_dx / linear_dw against torch autograd of relu(F.linear(x, w, b)) on the same values in fp64: the mask of
    the dX is the forward's output, the addend a gradient arriving beside it"""
    M, N, K = 37, 24, 64
    x, w = T.gemm_operands(kind, M, N, K)
    b = T.gemm_bias(kind, N)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    y = torch.relu(torch.nn.functional.linear(xd, wd, bd))
    v, S = T.linear_fwd(x, w, b, 1)
    assert torch.equal(v, y.detach()) and (S >= v.abs()).all()
    lin, _ = T.linear_fwd(x, w, b, 0)
    assert torch.equal(lin, torch.nn.functional.linear(xd, wd, bd).detach())
    dy = T.gemm_addend(kind, M, N, seed=3)                                    # any bf16 [M, N]
    y.backward(dy.double())
    dz = dy.double() * (y.detach() > 0)                                       # the gradient below the ReLU
    # dX of this layer is dz @ w; the kernel applies a mask to its OUTPUT, so check the two pieces separately
    p, Sp, final = T.linear_dx(dz.to(T.BF), w)                                # (dz is bf16-exact: dy or 0)
    assert torch.allclose(p, xd.grad, rtol=1e-13, atol=1e-13) and (Sp >= p.abs() * (1 - 1e-12)).all()
    assert torch.equal(final, T.bf16_round(p))
    mask = T.relu_mask(M, K)
    add = T.gemm_addend(kind, M, K, seed=4)
    _, _, fin2 = T.linear_dx(dz.to(T.BF), w, mask, add)
    want = T.bf16_round(torch.where(mask.double() > 0, T.bf16_round(p), torch.zeros((), dtype=T.F64)) + add.double())
    assert torch.equal(fin2, want)
    gw0, gb0 = T.gemm_grad0(kind, N, K), T.gemm_grad0(kind, N)
    gW, gb, SW, Sb = T.linear_dw(dz.to(T.BF), x, gw0, gb0)
    assert torch.allclose(gW - gw0.double(), wd.grad, rtol=1e-13, atol=1e-12) and torch.allclose(gb - gb0.double(), bd.grad, rtol=1e-13, atol=1e-12)
    assert (SW >= gW.abs() * (1 - 1e-12)).all() and (Sb >= gb.abs() * (1 - 1e-12)).all()


def test_relu_reference_propagates_nan_and_bf16_round_is_torchs_cast_on_ties():
    v = torch.tensor([float("nan"), -float("nan"), float("inf"), -float("inf"), -0.0, 0.0, -3.0, 2.5], dtype=T.F64)
    r = T.relu(v)
    assert torch.isnan(r[:2]).all() and r[2] == float("inf") and (r[3:7] == 0).all() and r[7] == 2.5
    # ties: 257 -> 256 (even mantissa below), 259 -> 260, 287 -> 288, 289 -> 288, -257 -> -256; 2^-133 * 1.5 (a subnormal tie) -> 2^-132
    t = torch.tensor([257.0, 259.0, 287.0, 289.0, -257.0, 1.5 * 2.0 ** -133, 258.0, 0.0], dtype=T.F64)
    assert T.on_bf16_tie(t).tolist() == [True, True, True, True, True, True, False, False]
    assert T.bf16_round(t).tolist() == [256.0, 260.0, 288.0, 288.0, -256.0, 2.0 ** -132, 258.0, 0.0]
    assert torch.equal(T.bf16_round(t), t.float().bfloat16().double())
    # every bf16 tie between 256 and 1024, against round-half-even done in integers
    ints = torch.arange(256, 1024, dtype=T.F64)
    ulp = torch.where(ints < 512, 2.0, 4.0).double()
    q = ints / ulp
    want = torch.where(q - q.floor() == 0.5, 2 * torch.round(q / 2), torch.round(q)) * ulp      # torch.round is half-even on x.5
    assert torch.equal(T.bf16_round(ints), want) and torch.equal(T.on_bf16_tie(ints), q - q.floor() == 0.5)


@pytest.mark.parametrize("M,N,R", ((33, 4, 64), (129, 132, 192), (8, 8, 8), (128, 128, 16384 * 7)))
def test_gemm_builders_preconditions(M, N, R):
    """what tests/test_gpu_gemm_kernels.py assumes of its inputs, from the references alone"""
    a, b = T.gemm_operands("exact", M, N, R)
    bias = T.gemm_bias("exact", N)
    for t, lim in ((a, T.EXACT_OPERAND), (b, T.EXACT_OPERAND), (bias, T.EXACT_BIAS)):
        assert (t.double() == t.double().round()).all() and t.double().abs().max() <= lim
    v, S = T.linear_fwd(a, b, bias, 0)
    assert S.max() < 2 ** 24 and (v == v.round()).all()                       # every partial sum is an integer below 2^24
    assert v[0, 0] == 287 and T.on_bf16_tie(v)[0, 0] and T.bf16_round(v)[0, 0] == 288
    add = T.gemm_addend("exact", M, N)
    assert add.double().abs().max() <= T.EXACT_ADDEND and add[0, 0] == 1 and T.on_bf16_tie(T.bf16_round(v) + add.double())[0, 0]
    g0 = T.gemm_grad0("exact", N, 8)
    assert g0.abs().max() <= T.EXACT_GRAD and (g0 == g0.round()).all() and g0.dtype == torch.float32
    # weight gradient of the same integers over R rows: |gW0| + 49 R stays below 2^24 up to the largest M of the GPU tests
    assert T.EXACT_GRAD + T.EXACT_OPERAND ** 2 * 16384 * 7 < 2 ** 24
    if M * N >= 64 and R <= 512:
        assert (v.abs() >= 256).any() and T.on_bf16_tie(torch.relu(v)).any()
    # far: S >> |ref| for most elements
    a, b = T.gemm_operands("far", M, N, R)
    v, S = T.linear_fwd(a, b, None, 0)
    assert (S / v.abs().clamp(min=1e-300)).median() > 20
    # the mask operand: both sides of zero, exact zeros, and the special values where they are promised
    y = T.relu_mask(M, max(N, 16))
    yd = y.double()
    assert (yd > 0).any() and (yd < 0).any() and (yd == 0).sum() > 0 and y[0, 0] == 1
    sp = y.view(torch.int16)[0, 1:1 + len(T.MASK_SPECIALS)].int() & 0xFFFF
    assert sp.tolist() == list(T.MASK_SPECIALS) and (yd[0, 1:1 + len(T.MASK_KEPT)] > 0).tolist() == list(T.MASK_KEPT)


def test_dw_mchunk_twin_gives_the_intended_reduction_tiles():
    """the table of test_tile_dw_pipeline_remainders: one 128 x 128 tile, M = 16384 nm -> 256 splits of nm reduction tiles on the
    exact path; 8 rows fewer -> the guarded path with as many"""
    for nm in range(1, 8):
        assert T.dw_tile_plan(16384 * nm, [(128, 128)], False) == (64 * nm, True, nm)
        assert T.dw_tile_plan(16384 * nm - 8, [(128, 128)], False) == (64 * nm, False, nm)
    for M in (1, 63, 64, 65):
        assert T.dw_tile_plan(M, [(136, 200)], False) == (64, M == 64, 1)          # (65: a second split of one row)
    assert T.dw_tile_plan(6144, [(8, 8), (72, 200), (136, 8), (128, 128), (64, 64), (256, 128), (8, 200), (136, 200)], True) == (192, True, 3)


# ---------------------------------------------------------------------------------------------------------------------
# the training attention
# ---------------------------------------------------------------------------------------------------------------------
ATTN_TIES = [(2, 32, 1, 32, "none", None), (2, 64, 2, 65, "trailing", None), (1, 96, 3, 196, "interior", None), (2, 160, 1, 160, "tile", None),
             (2, 96, 2, 100, "second", None), (1, 64, 1, 64, "bits", None), (2, 64, 2, 70, "none", 64), (1, 96, 1, 96, "none", 37), (2, 160, 2, 161, "none", 100)]


@pytest.mark.parametrize("B,L,heads,M,pads,Lk", ATTN_TIES)
def test_attention_references_are_attn_core_in_fp64_and_its_autograd(B, L, heads, M, pads, Lk):
    """rel_attn_fwd == oracle.ref_cpu.attn_core run in fp64 (causal with pads; Lk: the non-causal form, keys >= Lk masked); with
    ctx_in, lse_in its own fp64 forward, rel_attn_bwd == fp64 autograd through attn_core"""
    qkv, E, dctx = T.attn_gauss(B, L, heads, M)
    pm = T.attn_pads(pads, B, L)
    causal = Lk is None
    if causal:
        mask = (torch.arange(L)[None, :] > torch.arange(L)[:, None])[None, None]
        if pm is not None:
            mask = mask | pm[:, None, None, :]
    else:
        mask = (torch.arange(L) >= Lk)[None, None, None, :]
    qa, Ea = qkv.double().requires_grad_(), E.double().requires_grad_()
    ctx, w, logits = R.attn_core(qa, Ea, mask, heads)
    (ctx * dctx.double()).sum().backward()
    ref = T.rel_attn_fwd(qkv, E, pm, heads, M, causal, Lk)
    close(ref.ctx, ctx.detach())
    close(ref.P, w.detach())
    close(ref.lse, torch.logsumexp(logits.detach(), -1))
    assert (ref.P[~ref.vis.expand_as(ref.P)] == 0).all() and (ref.A >= ref.S.abs()).all() and (ref.R >= ref.A).all() and (ref.R <= 12 * ref.A + 1e-300).all() and (ref.PV >= ref.ctx.abs()).all()
    r = T.rel_attn_bwd(qkv, E, pm, ref.ctx, ref.lse, dctx, heads, M, causal, Lk)
    close(r.dqkv, qa.grad, 1e-12)
    close(r.dE, Ea.grad, 1e-12)
    assert M == L or (r.dE[:M - L] == 0).all()
    close(T.attn_weights(ref, ref.lse), ref.P)
    if causal:
        b, bE = T.attn_bwd_bounds(r, B)
        cb, lb, eps = T.attn_fwd_bounds(ref)
        assert (b[r.dqkv != 0] > 0).all() and (b >= 0).all() and (bE[M - L:] > 0).all() and (bE[:M - L] == 0).all() and (cb > 0).all() and (lb > 0).all()
        # the bounds are bounds of rounding: a bf16 ulp of the output and a few of its absolute sum, far below the data's own scale
        assert (cb <= 2.0 ** -6 * ref.PV + 1e-300).all() and lb.max() < 2.0 ** -10


def test_attention_backward_reference_takes_ctx_and_lse_as_given():
    """the backward is the kernels' formula on the values handed in: another lse scales P, another ctx moves delta"""
    qkv, E, dctx = T.attn_gauss(1, 32, 1, 32)
    ref = T.rel_attn_fwd(qkv, E, None, 1, 32)
    a = T.rel_attn_bwd(qkv, E, None, ref.ctx, ref.lse, dctx, 1, 32)
    b = T.rel_attn_bwd(qkv, E, None, ref.ctx, ref.lse + math.log(2.0), dctx, 1, 32)
    close(b.P, a.P / 2)
    c = T.rel_attn_bwd(qkv, E, None, torch.zeros_like(ref.ctx), ref.lse, dctx, 1, 32)
    close(c.dS, a.P * (a.dO @ T._heads(qkv[..., 128:], 1).transpose(-1, -2)))


def test_pad_patterns_and_bitmap():
    for L in (32, 96, 160):
        for name in T.ATTN_PADS[1:]:
            m = T.attn_pads(name, 3, L)
            assert m.shape == (3, L) and not m[:, 0].any() and m.any()
            w = T.pack_padbits(m).numpy().view(np.uint32)
            for b, j in ((0, 31), (2, L - 1), (1, L // 2), (0, 1)):
                assert bool((w[b, j >> 5] >> (j & 31)) & 1) == bool(m[b, j])
    m = T.attn_pads("bits", 1, 96)
    assert m[0, 31] and m[0, 32] and m[0, 64] and m[0, 95] and m.sum() == 4
    assert T.attn_pads("tile", 2, 96)[0, 32:64].all() and T.attn_pads("second", 1, 32)[0, 1::2].all()


@pytest.mark.parametrize("L", (32, 96, 160, 288))
def test_selector_data_has_the_exact_answer_it_claims(L):
    """the builders assert margin, exactness and tile cover from the reference; here the references reproduce the exact answer
    and the bounds collapse: about a bf16 ulp of the selected value for ctx, exactly 0 for dq / dk where nothing can contribute"""
    B, heads, M = 2, 2, L + 1
    for pads in T.ATTN_PADS:
        pm = T.attn_pads(pads, B, L)
        qkv, E, dctx, sel, rows, ctx, dv = T.attn_selector_content(B, L, heads, M, pm)
        ref = T.rel_attn_fwd(qkv, E, pm, heads, M)
        assert (ref.ctx - ctx).abs().max() < 1e-100 and rows.all()
        cb, lb, _ = T.attn_fwd_bounds(ref)
        assert (cb <= 2.0 ** -4 * ctx.abs() + 2.0 ** -100).all() and (cb[ctx == 0] < 2.0 ** -100).all()          # (the underflow floor)
        r = T.rel_attn_bwd(qkv, E, pm, ref.ctx.to(BF), ref.lse.float(), dctx, heads, M)
        d = 64 * heads
        # (fp64 keeps exp(-259), fp32 does not)
        assert r.dqkv[..., :2 * d].abs().max() < 1e-100 and r.dE.abs().max() < 1e-100 and (r.dqkv[..., 2 * d:] - dv).abs().max() < 1e-100
        b, bE = T.attn_bwd_bounds(r, B)
        assert b[..., 2 * d:].max() < 0.5 and cb.max() < 0.5       # a whole integer off fails outright
        for d0 in T.SEL_REL_DELTAS:
            d0 = L - 1 if d0 < 0 else d0
            if d0 < L:
                qkv, E, dctx, sel, rows, ctx, dv = T.attn_selector_rel(B, L, heads, M, d0, pm)
                ref = T.rel_attn_fwd(qkv, E, pm, heads, M)
                assert (ref.ctx - ctx)[rows].abs().max() < 1e-100
                r = T.rel_attn_bwd(qkv, E, pm, ref.ctx.to(BF), ref.lse.float(), dctx, heads, M)
                assert r.dqkv[..., :d][rows].abs().max() < 1e-100


def test_far_data_jumps():
    for L in (96, 160, 288):
        qkv, E, dctx, (i, j) = T.attn_far(2, L, 2, L)
        assert j // 32 >= 1 and (L < 160 or j // 32 < (i // 128) * 4)


# ---------------------------------------------------------------------------------------------------------------------
# dropout with injected masks in oracle.ref_cpu (tests/test_gpu_dropout_model.py compares training steps with it)
# ---------------------------------------------------------------------------------------------------------------------
def _tiny_model(dtype=torch.float32, V=20, d=64, nl=2, L=40, B=2):
    p = {k: v.to(dtype) for k, v in R.init_params(V, d, nl, L, seed=4).items()}
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, V - 1, (B, L), generator=g)
    x[1, -3:] = V - 1
    return p, x, (V, d, nl, L, B)


@pytest.mark.parametrize("emulate", (False, True))
def test_all_ones_multipliers_reproduce_the_unmasked_oracle_exactly(emulate):
    p, x, (V, d, nl, L, B) = _tiny_model()
    ones = R.model_drop(0.0, 77, nl, B, L, d)
    assert set(ones) == {"emb"} | {(s, i) for s in ("ln1", "ln2") for i in range(nl)}
    assert all(m.shape == (B, L, d) and (m == 1).all() for m in ones.values())
    R.EMULATE_BF16 = emulate
    try:
        want, _ = R.model_forward(p, x, V - 1)
        got, _ = R.model_forward(p, x, V - 1, drop=ones)
        assert torch.equal(got, want)
        assert torch.equal(R.model_forward(p, x, V - 1, drop={})[0], want)       # a missing site is not dropped
        # `drop` replaces F.dropout: rate / training no longer draw anything
        assert torch.equal(R.model_forward(p, x, V - 1, 0.5, True, drop=ones)[0], want)
    finally:
        R.EMULATE_BF16 = False
    # the GRU: fp32 semantics only (the emulation rounds the masked value to bf16, as the kernel does; see below)
    T_, Bg, H, lay, Vg = 5, 3, 8, 3, 11
    net = torch.nn.GRU(Vg, H, num_layers=lay)
    pg = {"rnn." + k: v.detach() for k, v in net.named_parameters()}
    g = torch.Generator().manual_seed(1)
    pg.update({"event_embedding.weight": torch.randn(Vg, Vg, generator=g), "output_fc.weight": torch.randn(Vg, H, generator=g),
               "output_fc.bias": torch.randn(Vg, generator=g), "inithid_fc.weight": torch.randn(lay * H, 4, generator=g),
               "inithid_fc.bias": torch.randn(lay * H, generator=g)})
    init, ev = torch.randn(Bg, 4, generator=g), torch.randint(0, Vg, (T_, Bg), generator=g)
    want = R.gru_train_logits(pg, init, ev, lay, H, Vg - 1)
    ones = R.gru_drop(0.0, 5, lay, T_ + 1, Bg, H)
    assert set(ones) == {("gru", 0), ("gru", 1)} and all(m.shape == (T_ + 1, Bg, H) for m in ones.values())
    assert torch.equal(R.gru_train_logits(pg, init, ev, lay, H, Vg - 1, drop=ones), want)
    # a real mask: layer l's output is dropped on its way UP only; the recurrence keeps the whole state
    drop = R.gru_drop(0.5, 5, lay, T_ + 1, Bg, H)
    hid = R.gru_init_hidden(pg, init, lay, H)
    seq = torch.cat([torch.full((1, Bg), Vg - 1), ev]).long()
    outs = []
    for t in range(T_ + 1):
        xin, new = pg["event_embedding.weight"][seq[t]], []
        for l in range(lay):
            cell = torch.nn.GRUCell(xin.shape[1], H)
            cell.load_state_dict({k: pg[f"rnn.{k}_l{l}"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")})
            h = cell(xin, hid[l]).detach()
            new.append(h)
            xin = h * drop["gru", l][t] if l < lay - 1 else h
        hid = torch.stack(new)
        outs.append(torch.nn.functional.linear(xin, pg["output_fc.weight"], pg["output_fc.bias"]))
    close(R.gru_train_logits(pg, init, ev, lay, H, Vg - 1, drop=drop), torch.stack(outs), 1e-5)
    R.EMULATE_BF16 = True
    try:                                                    # one bf16 rounding after the multiplier, as mgx_dropout_bf16 stores it
        h0 = R.gru_init_hidden(pg, init, lay, H)
        m = [drop["gru", 0][0], None, None]
        _, a = R.gru_step(pg, seq[:1], h0)
        lo, b = R.gru_step({**pg, "rnn.weight_ih_l1": torch.eye(H).repeat(3, 1), "rnn.bias_ih_l1": torch.zeros(3 * H),
                            "rnn.weight_hh_l1": torch.zeros(3 * H, H), "rnn.bias_hh_l1": torch.zeros(3 * H)}, seq[:1], h0, m)
        assert torch.equal(a[0], b[0])
        # layer 1 with W_ih = [I; I; I] and nothing else: r = z = sigmoid(input), n = tanh(input) -- it shows the input it saw
        seen = (a[0] * m[0]).to(BF).float()
        z = torch.sigmoid(seen)
        assert torch.equal(b[1], (1 - z) * torch.tanh(seen) + z * h0[1])
    finally:
        R.EMULATE_BF16 = False


def test_site_multipliers_index_the_padded_rows_and_carry_the_twins_scale():
    B, L, d = 3, 40, 64
    for p_drop in (0.1, 0.2, 0.5):
        thr, _, scale = T.make_drop(p_drop, 1234)
        m = R.site_mult(p_drop, 1234, B, L, d)
        assert m.shape == (B, L, d) and m.dtype == torch.float32
        assert set(m.unique().tolist()) == {0.0, float(scale)} and float(scale) == float(np.float32(1.0 / (1.0 - thr / 65536.0)))
        full = T.drop_mult(p_drop, 1234, B * 64 * d).view(B, 64, d)                 # Lp = 64 rows per sequence on the device
        assert torch.equal(m, full[:, :L])
        unpadded = R.site_mult(p_drop, 1234, B, L, d, Lp=L)
        assert torch.equal(unpadded, T.drop_mult(p_drop, 1234, B * L * d).view(B, L, d))
        assert torch.equal(unpadded[0], m[0]) and not torch.equal(unpadded[1], m[1])   # the first sequence starts at row 0 either way
    assert float(T.make_drop(0.2, 0)[2]) != 1.25                                    # thr = 13107: not 1 / (1 - p)
    plan = R.model_drop(0.5, 1000, 2, B, L, d)
    for key, off in (("emb", 0), (("ln1", 0), 1), (("ln2", 0), 2), (("ln1", 1), 5), (("ln2", 1), 6)):
        assert torch.equal(plan[key], R.site_mult(0.5, 1000 + off, B, L, d)), key


def test_masked_encoder_layer_is_the_masked_layernorm_between_its_neighbours():
    """fp64 throughout: rga -> add_ln_fwd(.., mult1) -> FFN -> add_ln_fwd(.., mult2), the multiplier on the branch, never on the
    residual; and under the bf16 emulation the multiplier meets the rounded branch output in fp32, with no rounding of its own"""
    p, x, (V, d, nl, L, B) = _tiny_model(F64)
    pre = "Decoder.enc_layers.1."
    g = torch.Generator().manual_seed(2)
    h = torch.randn(B, L, d, generator=g, dtype=F64)
    mask = R.look_ahead_mask(x, V - 1)
    m1, m2 = R.site_mult(0.2, 31, B, L, d), R.site_mult(0.2, 32, B, L, d)
    got, _ = R.encoder_layer(p, pre, h, mask, 1, 0.0, False, drop=(m1, m2))
    a, _ = R.rga_forward(p, pre + "rga.", h, mask, 1)
    flat = lambda t: t.reshape(B * L, d)
    o1 = T.add_ln_fwd(flat(a), flat(h), p[pre + "layernorm1.weight"], p[pre + "layernorm1.bias"], 1e-6, flat(m1))[2]
    f = torch.relu(torch.nn.functional.linear(o1, p[pre + "FFN_pre.weight"], p[pre + "FFN_pre.bias"]))
    f = torch.nn.functional.linear(f, p[pre + "FFN_suf.weight"], p[pre + "FFN_suf.bias"])
    o2 = T.add_ln_fwd(f, o1, p[pre + "layernorm2.weight"], p[pre + "layernorm2.bias"], 1e-6, flat(m2))[2]
    close(flat(got), o2, 1e-9)
    plain, _ = R.encoder_layer(p, pre, h, mask, 1, 0.0, False)
    assert (got - plain).abs().max() > 0.1                                          # the masks matter
    # bf16 emulation, fp32 values
    p32 = {k: v.float() for k, v in p.items()}
    h32 = h.float().to(BF).float()
    R.EMULATE_BF16 = True
    try:
        got, _ = R.encoder_layer(p32, pre, h32, mask, 1, 0.0, False, drop=(m1, m2))
        a, _ = R.rga_forward(p32, pre + "rga.", h32, mask, 1)
        assert torch.equal(a, a.to(BF).float())
        o1 = torch.nn.functional.layer_norm(a * m1 + h32, (d,), p32[pre + "layernorm1.weight"], p32[pre + "layernorm1.bias"], 1e-6).to(BF).float()
        f = torch.relu(R._lin(o1, p32[pre + "FFN_pre.weight"], p32[pre + "FFN_pre.bias"]))
        f = R._lin(f, p32[pre + "FFN_suf.weight"], p32[pre + "FFN_suf.bias"])
        o2 = torch.nn.functional.layer_norm(o1 + f * m2, (d,), p32[pre + "layernorm2.weight"], p32[pre + "layernorm2.bias"], 1e-6).to(BF).float()
        assert torch.equal(got, o2)
        # the embedding: the multiplier inside the single rounding (a model without layers is its embedding stage)
        emb = {"Decoder.embedding.weight": p32["Decoder.embedding.weight"]}
        me = R.site_mult(0.2, 30, B, L, d)
        e, _ = R.decoder_stack(emb, x, mask, drop={"emb": me})
        want = ((emb["Decoder.embedding.weight"][x] * math.sqrt(d) + R.sinusoid_table(L, d).float()[None]) * me).to(BF).float()
        assert torch.equal(e, want)
        twice = (emb["Decoder.embedding.weight"][x] * math.sqrt(d) + R.sinusoid_table(L, d).float()[None]).to(BF).float() * me
        assert not torch.equal(e, twice.to(BF).float())                             # (rounding first, then scaling, is another number)
    finally:
        R.EMULATE_BF16 = False


def test_split_multiplier_node_uses_one_mask_forward_and_the_other_backward():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 16, generator=g, dtype=F64).requires_grad_()
    mf, mb = T.drop_mult(0.5, 1, 64).view(4, 16).double(), T.drop_mult(0.5, 2, 64).view(4, 16).double()
    up = torch.randn(4, 16, generator=g, dtype=F64)
    y = R.SplitMult.apply(x, mf, mb)
    assert torch.equal(y.detach(), x.detach() * mf)
    y.backward(up)
    assert torch.equal(x.grad, up * mb) and not torch.equal(mf, mb)
    # through the oracle: same forward as the plain masks, another gradient
    p, tok, (V, d, nl, L, B) = _tiny_model()
    right = R.model_drop(0.5, 50, nl, B, L, d)
    other = R.model_drop(0.5, 9050, nl, B, L, d)
    grads = []
    for drop in (right, {k: (right[k], other[k]) for k in right}):
        q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        out, _ = R.model_forward(q, tok, V - 1, drop=drop)
        grads.append((out.detach(), torch.autograd.grad(out.square().sum(), q["Decoder.embedding.weight"])[0]))
    assert torch.equal(grads[0][0], grads[1][0]) and not torch.allclose(grads[0][1], grads[1][1], rtol=1e-2)


# ---------------------------------------------------------------------------------------------------------------------
# the masks of the seeds the model really uses are independent
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_drop", (0.1, 0.2, 0.5))
def test_twin_masks_at_the_models_seeds_are_independent(p_drop):
    """The seeds of one training forward of a 3-layer model (network._hidden: embedding s, layer i s + 4 i + 1 and s + 4 i + 2)
    and of the next one (s + 64 ..) differ in a few low bits only.  Keep rate of each mask, and the rate at which two masks agree
    -- every pair of seeds, element against element and against the element 1, 8, 64 and 128 further on, and each mask against
    itself at those shifts -- all within 5 sigma of the binomial's: independent masks agree at q^2 + (1 - q)^2, q = thr / 65536.
    The largest figure is 4.17 sigma at p = 0.5, offsets 2 and 66 (the LayerNorm 2 seeds of layer 0 in consecutive calls) at shift
    1 -- about 2 % likely among these 795 comparisons.  Followed up: a correlation would grow with sqrt(n), but the same pair gives
    -4.17, -3.15, -2.72, -2.83, -2.20 sigma at n = 2^20 .. 2^24; -0.10, 0.17, -1.50, -1.27 at p = 0.1, 0.2, 0.3, 0.7 (n = 2^22); and the
    same offsets from 40 other base seeds have mean -0.23, standard deviation 1.25, the 4.17 here the largest.  A fluctuation of the
    first 2^20 elements of one pair, not a property of seeds 64 apart (40 such pairs at shift 1: mean -0.05, sd 1.14, max 2.29)."""
    n = 1 << 20
    torch.manual_seed(0)
    s = (torch.initial_seed() * 1000003 + 64) & 0x7FFFFFFFFFFFFFFF             # _next_seed's first value
    seeds = [s + o for o in (0, 1, 2, 5, 6, 9, 10, 64, 65, 66)]
    q = T.make_drop(p_drop, 0)[0] / 65536.0
    kept = [T.drop_mult(p_drop, sd, n).numpy() != 0 for sd in seeds]
    worst = 0.0
    for k, sd in zip(kept, seeds):
        z = abs(k.mean() - (1 - q)) / math.sqrt(q * (1 - q) / n)
        worst = max(worst, z)
        assert z <= 5, (p_drop, sd, z)
    a = q * q + (1 - q) * (1 - q)
    for i in range(len(seeds)):
        for j in range(i, len(seeds)):
            for shift in (0, 1, 8, 64, 128):
                if i == j and shift == 0:
                    continue
                m = n - shift
                agree = (kept[i][:m] == kept[j][shift:]).mean()
                z = abs(agree - a) / math.sqrt(a * (1 - a) / m)
                worst = max(worst, z)
                assert z <= 5, (p_drop, seeds[i] - s, seeds[j] - s, shift, z)
    print(f"p {p_drop}: worst {worst:.2f} sigma")


def test_dropout_fixtures_keep_the_references_own_ambiguity_inside_the_bound():
    """tests/test_gpu_dropout_model.py holds training steps to a gradient cosine of 0.999 against the bf16-emulated oracle.  The
    emulation leaves out one rounding of the kernels (the attention probabilities enter P V as bf16); with a rounding of that size
    emulated as well (R.rga_forward's round_p) the oracle's own gradients move, FFN_pre.weight the most.  At the seeds the
    fixtures use (tests/dropout_fixtures.py) no gradient moves by more than 0.75 of its bound, in any comparison the module makes
    (p = 0 and p > 0; first call, second call, their sum).  That says the bound means something AT these seeds; at others the
    move exceeds the bound (the module's docstring has the range)."""
    import dropout_fixtures as DF
    for case in DF.CASES:
        name, r = DF.ambiguity(case)
        assert not R.EMULATE_BF16 and R.rga_forward.__name__ == "rga_forward"
        print(case, "seed", DF.FIXTURE_SEED[case], "largest move / bound %.3f (%s)" % (r, name))
        assert r <= 0.75 and name.endswith("FFN_pre.weight"), (case, name, r)
