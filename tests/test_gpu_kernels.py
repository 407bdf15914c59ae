"""GPU parity tests proper: every HIP kernel, called through the C ABI, against the oracle on the
same seeded inputs.  bf16-IO kernels are compared with the fp32 oracle evaluated on the SAME
bf16-rounded inputs, so the tolerances below only cover in-kernel rounding:
  attention ctx: |err| <= 2e-2 * max|ref| (P and ctx are rounded to bf16), lse: 2e-3 abs
  LayerNorm out: 2e-2 abs (bf16 output of O(1) values), statistics 1e-4
  CE loss: rtol 1e-4 (fp32 math on bf16 logits), dlogits: 1e-2 relative to max
  gradients: cosine >= 0.999 and rel-L2 <= 2e-2."""
import math
import os

import numpy as np
import pytest
import torch

from kernel_checks import cos as _cos, rel as _relerr

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _mask(tok, pad):
    from oracle import ref_cpu as R
    return R.look_ahead_mask(tok, pad)


@pytest.mark.parametrize("B,L,d,M,padcase", [(2, 32, 64, 32, 0), (2, 64, 128, 64, 1), (1, 160, 64, 192, 1),
                                              (2, 256, 128, 256, 0), (1, 512, 512, 512, 1)])
def test_rel_attn_fwd_matches_oracle(B, L, d, M, padcase):
    from musicgeneration_amd import ops
    from oracle import ref_cpu as R
    dev = _dev()
    g = torch.Generator().manual_seed(100 + L + d)
    h = d // 64
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 1.0).to(torch.bfloat16)
    E = (torch.randn(M, 64, generator=g) * 0.5).to(torch.bfloat16)
    pad = 7
    tok = torch.randint(0, 7, (B, L), generator=g, dtype=torch.int32)
    if padcase:
        tok[0, L - 5:] = pad           # trailing pads
        tok[-1, L // 2] = pad          # an isolated padded key in the middle
    ref_ctx, ref_w, ref_logits = R.attn_core(qkv.float(), E.float(), _mask(tok, pad), h)
    ref_lse = torch.logsumexp(ref_logits, -1)
    tok_d = tok.to(dev)
    bits = ops.pad_bitmap(tok_d, pad) if padcase else None
    if padcase:  # bitmap itself is integer work: bit-exact
        exp = (tok == pad).reshape(B, L // 32, 32).to(torch.int64)
        exp = (exp << torch.arange(32)).sum(-1).to(torch.int64)
        got = bits.cpu().to(torch.int64) & 0xFFFFFFFF
        assert (got == exp).all()
    ctx, lse = ops.rel_attn_fwd(qkv.to(dev), E.to(dev), bits)
    torch.cuda.synchronize()
    ctx, lse = ctx.float().cpu(), lse.cpu()
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    tol = 2e-2 * ref_ctx.abs().max().item()
    err = (ctx - ref_ctx).abs().max().item()
    assert err <= tol, f"ctx max err {err} > {tol}"
    assert _relerr(ctx, ref_ctx) < 1e-2
    assert (lse - ref_lse).abs().max().item() < 2e-3 * max(1.0, ref_lse.abs().max().item())


@pytest.mark.parametrize("B,L,Lk,d,M", [(2, 32, 32, 64, 32), (1, 160, 160, 128, 192), (2, 64, 37, 64, 64), (1, 288, 261, 64, 288),
                                        (3, 128, 97, 192, 128)])
def test_rel_attn_fwd_nomask_matches_oracle(B, L, Lk, d, M):
    """mgx_rel_attn_fwd_nomask = the reference's attention with mask=None (its sampling call): bidirectional over the Lk real
    positions, relative term q_i.E[M-1-(i-j)] for j <= i and 0 for j > i; rows >= Lk are padding (ignored)."""
    from musicgeneration_amd import ops
    from oracle import ref_cpu as R
    dev = _dev()
    g = torch.Generator().manual_seed(77 + L + Lk)
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 0.8).to(torch.bfloat16)
    E = (torch.randn(M, 64, generator=g) * 0.5).to(torch.bfloat16)
    # the oracle on the window of Lk positions (E is indexed from its END, so a shorter window only drops distances)
    ref, _, _ = R.attn_core(qkv[:, :Lk].float(), E.float(), None, d // 64)
    ctx = ops.rel_attn_fwd_nomask(qkv.to(dev), E.to(dev), Lk)
    torch.cuda.synchronize()
    got = ctx[:, :Lk].float().cpu()
    assert torch.isfinite(got).all()
    assert (got - ref).abs().max().item() <= 2e-2 * ref.abs().max().item()
    assert ((got - ref).norm() / ref.norm()).item() < 1e-2
    # not the causal result
    causal, _ = ops.rel_attn_fwd(qkv.to(dev), E.to(dev), None)
    assert (causal[:, :Lk].float().cpu() - ref).abs().max().item() > 5e-2 * ref.abs().max().item() or Lk == 1


def test_rel_attn_fwd_softmax_rescale_branch():
    """Force the online-softmax rescale: one late key dominates a row so the running max jumps at a
    later key tile (cdna guide rule 26: a rare data-dependent branch needs its own test)."""
    from musicgeneration_amd import ops
    from oracle import ref_cpu as R
    dev = _dev()
    B, L, d = 1, 128, 64
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 0.3).to(torch.bfloat16)
    qkv[0, 100, :64] = 4.0     # query row 100
    qkv[0, 70, 64:128] = 4.0   # key 70 (third key tile) aligned with it: logit = 64*16/8 = 128
    E = (torch.randn(L, 64, generator=g) * 0.1).to(torch.bfloat16)
    tok = torch.zeros(B, L, dtype=torch.int32)
    ref_ctx, _, _ = R.attn_core(qkv.float(), E.float(), _mask(tok, 9), 1)
    ctx, _ = ops.rel_attn_fwd(qkv.to(dev), E.to(dev), None)
    ctx = ctx.float().cpu()
    assert (ctx - ref_ctx).abs().max().item() <= 2e-2 * ref_ctx.abs().max().item()


def test_rel_attn_fwd_leading_pad_rows_finite():
    """Rows whose every key j<=i is padding are outside the parity contract (reference = rounding
    artefact); the kernel must stay finite and all other rows must still match."""
    from musicgeneration_amd import ops
    from oracle import ref_cpu as R
    dev = _dev()
    B, L, d, pad = 1, 64, 64, 5
    g = torch.Generator().manual_seed(6)
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 0.5).to(torch.bfloat16)
    E = (torch.randn(L, 64, generator=g) * 0.5).to(torch.bfloat16)
    tok = torch.zeros(B, L, dtype=torch.int32)
    tok[0, :3] = pad
    ref_ctx, _, _ = R.attn_core(qkv.float(), E.float(), _mask(tok, pad), 1)
    ctx, lse = ops.rel_attn_fwd(qkv.to(dev), E.to(dev), ops.pad_bitmap(tok.to(dev), pad))
    ctx = ctx.float().cpu()
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    assert (ctx[:, 3:] - ref_ctx[:, 3:]).abs().max().item() <= 2e-2 * ref_ctx.abs().max().item()


@pytest.mark.parametrize("rows,d", [(64, 128), (300, 512), (77, 768)])
def test_add_ln_fwd_bwd(rows, d):
    from musicgeneration_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(rows + d)
    x = torch.randn(rows, d, generator=g).to(torch.bfloat16)
    res = (torch.randn(rows, d, generator=g) * 2).to(torch.bfloat16)
    gamma = torch.randn(d, generator=g) * 0.5 + 1
    beta = torch.randn(d, generator=g) * 0.1
    dout = torch.randn(rows, d, generator=g).to(torch.bfloat16)
    xr, rr = x.float().requires_grad_(True), res.float().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr + rr, (d,), gr, br, 1e-6)
    ref.backward(dout.float())
    out, mean, rstd = ops.add_ln_fwd(x.to(dev), res.to(dev), gamma.to(dev), beta.to(dev), 1e-6)
    dgamma = torch.zeros(d, device=dev)
    dbeta = torch.zeros(d, device=dev)
    dxsum = torch.ones(d, device=dev)
    dx, dres = ops.add_ln_bwd(dout.to(dev), x.to(dev), res.to(dev), gamma.to(dev), mean, rstd, dgamma, dbeta, dxsum=dxsum)
    torch.cuda.synchronize()
    assert _relerr(dxsum.cpu() - 1, dx.float().cpu().sum(0)) < 1e-4       # bias gradient of the producer of x
    assert (out.float().cpu() - ref.detach()).abs().max().item() < 3e-2
    z = x.float() + res.float()
    assert (mean.cpu() - z.mean(-1)).abs().max().item() < 1e-4
    assert _relerr(rstd.cpu(), 1 / torch.sqrt(z.var(-1, unbiased=False) + 1e-6)) < 1e-4
    assert dx.data_ptr() == dres.data_ptr()
    assert _relerr(dres.cpu(), rr.grad) < 1e-2 and _cos(dres.cpu(), rr.grad) > 0.9999
    assert _relerr(dgamma.cpu(), gr.grad) < 2e-3
    assert _relerr(dbeta.cpu(), br.grad) < 2e-3


def test_add_ln_dropout_consistent():
    """dropout mask is a pure function of (seed, index): fwd and bwd must agree, keep rate ~ 1-p."""
    from musicgeneration_amd import ops
    dev = _dev()
    rows, d, p = 256, 512, 0.2
    x = torch.ones(rows, d, dtype=torch.bfloat16, device=dev)
    res = torch.zeros(rows, d, dtype=torch.bfloat16, device=dev)
    gamma = torch.ones(d, device=dev)
    beta = torch.zeros(d, device=dev)
    out, mean, rstd = ops.add_ln_fwd(x, res, gamma, beta, 1e-6, p, seed=1234)
    # z is either 0 or 1/(1-p); after LN the two values are distinguishable by sign
    keep_fwd = out.float() > 0
    rate = keep_fwd.float().mean().item()
    assert abs(rate - (1 - p)) < 0.01, rate
    dgamma = torch.zeros(d, device=dev)
    dbeta = torch.zeros(d, device=dev)
    dout = torch.randn(rows, d, device=dev).to(torch.bfloat16)
    dx, dres = ops.add_ln_bwd(dout, x, res, gamma, mean, rstd, dgamma, dbeta, p, seed=1234)
    torch.cuda.synchronize()
    kept_bwd = dx.float() != 0
    # dropped positions must have exactly zero grad; kept ones dx = dres/(1-p)
    assert (kept_bwd & ~keep_fwd).sum().item() == 0
    sel = keep_fwd & (dres.float().abs() > 1e-3)
    ratio = (dx.float()[sel] / dres.float()[sel])
    assert (ratio - 1 / (1 - p)).abs().max().item() < 0.02
    out2, _, _ = ops.add_ln_fwd(x, res, gamma, beta, 1e-6, p, seed=99)
    assert ((out2.float() > 0) != keep_fwd).any()      # another seed gives another mask


def test_embed_pe_fwd_bwd():
    from musicgeneration_amd import ops
    from oracle import ref_cpu as R
    dev = _dev()
    B, L, d, V = 3, 64, 128, 337
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, V, (B, L), generator=g, dtype=torch.int32)
    table = torch.randn(V, d, generator=g)
    pe = R.sinusoid_table(L, d).float()
    ref = table[tok.long()] * math.sqrt(d) + pe[None]
    out = ops.embed_pe_fwd(tok.to(dev), table.to(dev), pe.to(dev))
    assert (out.float().cpu() - ref).abs().max().item() <= 2 ** -8 * ref.abs().max().item()
    dout = torch.randn(B, L, d, generator=g).to(torch.bfloat16)
    dtable = torch.zeros(V, d, device=dev)
    ops.embed_bwd(tok.to(dev), dout.to(dev), dtable)
    refg = torch.zeros(V, d).index_add_(0, tok.flatten().long(), dout.float().reshape(-1, d)) * math.sqrt(d)
    assert _relerr(dtable.cpu(), refg) < 1e-5


def test_smooth_ce_golden_and_random(golden_dir):
    from musicgeneration_amd import ops
    from oracle import ref_cpu as R
    dev = _dev()
    g = dict(np.load(os.path.join(golden_dir, "g3_smoothce.npz")))
    V, pad, eps = g["logits"].shape[-1], int(g["pad"]), float(g["eps"])
    cases = [(torch.from_numpy(g["logits"]), torch.from_numpy(g["target"]))]
    gen = torch.Generator().manual_seed(8)
    lg = torch.randn(5, 40, 486, generator=gen) * 4
    tg = torch.randint(0, 486, (5, 40), generator=gen)
    tg[:, -3:] = 485
    cases.append((lg, tg))
    for lg, tg in cases:
        V = lg.shape[-1]
        pad = V - 1
        lb = lg.to(torch.bfloat16)
        ref_in = lb.float().requires_grad_(True)
        ref = R.smooth_ce(ref_in, tg, eps, V, pad)
        ref.backward()
        loss, stats, argmax = ops.smooth_ce(lb.to(dev).requires_grad_(True), tg.to(torch.int32).to(dev), V, eps, pad)
        torch.cuda.synchronize()
        assert abs(loss.item() - ref.item()) <= 1e-4 * abs(ref.item())
        assert (argmax.cpu().long() == lb.float().argmax(-1).flatten()).all()
        st = stats.cpu()
        assert st[1].item() == (tg != pad).sum().item() and st[3].item() == tg.numel()
        assert st[2].item() == (lb.float().argmax(-1) == tg).sum().item()
        s2, a2, rl = ops.smooth_ce_fwd(lb.to(dev), tg.to(torch.int32).to(dev), V, eps, pad)
        dl = ops.smooth_ce_bwd(lb.to(dev), tg.to(torch.int32).to(dev), s2, rl, V, eps, pad, 1.0)
        assert _relerr(dl.cpu(), ref_in.grad) < 1e-2
        assert (dl.float().cpu() - ref_in.grad).abs().max().item() <= 1e-2 * ref_in.grad.abs().max().item()
        # the upstream gradient as host constant x device scalar (ABI 16): read inside the kernel, no pass over dlogits
        dl3 = ops.smooth_ce_bwd(lb.to(dev), tg.to(torch.int32).to(dev), s2, rl, V, eps, pad, 0.5, torch.tensor(3.0, device=dev))
        assert _relerr(dl3.cpu(), 1.5 * ref_in.grad) < 1e-2
        # ... which is how autograd's grad_output reaches it
        lg_dev = lb.to(dev).requires_grad_(True)
        loss2, _, _ = ops.smooth_ce(lg_dev, tg.to(torch.int32).to(dev), V, eps, pad)
        (loss2 * 0.25).backward()
        assert _relerr(lg_dev.grad.cpu(), 0.25 * ref_in.grad) < 1e-2


@pytest.mark.parametrize("V,ld", [(337, 384), (486, 512), (1100, 1104), (20, 64)])
def test_smooth_ce_padded_rows_take_the_vector_path_and_agree_with_the_scalar_one(V, ld):
    """the model hands the loss its logits as a [rows, V] view of a [rows, ld] buffer (vocabulary rows padded to the GEMM tile):
    rows of ld % 8 == 0 elements go through the 16-byte-per-lane kernels, a contiguous [rows, V] copy (ld = V, odd) through the
    scalar ones -- same statistics, same arg-max, same gradient, and zeros in the padding columns of dlogits."""
    from musicgeneration_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(V)
    rows, eps, pad = 77, 0.1, V - 1
    base = torch.zeros(rows, ld, dtype=torch.bfloat16)
    base[:, :V] = (torch.randn(rows, V, generator=g) * 3).to(torch.bfloat16)
    base[3, 5:9] = base[3, :V].max() + 1                      # a tie for the maximum: arg-max must be the FIRST index
    tgt = torch.randint(0, V, (rows,), generator=g, dtype=torch.int32)
    tgt[-5:] = pad
    based, tg = base.to(dev), tgt.to(dev)
    flat = based[:, :V].contiguous() if V % 8 else None
    s1, a1, l1 = ops.smooth_ce_fwd(based, tg, V, eps, pad)
    d1 = ops.smooth_ce_bwd(based, tg, s1, l1, V, eps, pad, 1.0)
    ref = base[:, :V].float()
    assert (a1.cpu().long() == ref.argmax(-1)).all() and a1[3].item() == 5
    assert torch.allclose(l1.cpu(), torch.logsumexp(ref, -1), rtol=1e-5, atol=1e-5)
    assert (d1[:, V:] == 0).all()
    if flat is not None:
        s2, a2, l2 = ops.smooth_ce_fwd(flat, tg, V, eps, pad)
        d2 = ops.smooth_ce_bwd(flat, tg, s2, l2, V, eps, pad, 1.0)
        assert torch.equal(a1, a2) and torch.allclose(l1, l2, rtol=1e-6, atol=1e-6)
        assert torch.allclose(s1, s2, rtol=1e-5)
        assert torch.equal(d1[:, :V], d2)


def test_adam_matches_torch():
    from musicgeneration_amd import ops
    dev = _dev()
    n = 10007
    g = torch.Generator().manual_seed(4)
    p0 = torch.randn(n, generator=g)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=0.0, betas=(0.9, 0.98), eps=1e-9)
    npad = (n + 3) // 4 * 4
    p = torch.zeros(npad, device=dev); p[:n] = p0.to(dev)
    m = torch.zeros(npad, device=dev); v = torch.zeros(npad, device=dev)
    sh = torch.zeros(npad, dtype=torch.bfloat16, device=dev)
    for step in range(1, 4):
        grad = torch.randn(n, generator=g) * 0.1
        lr = 1e-3 * step
        ref.grad = grad.clone()
        for gr in opt.param_groups:
            gr["lr"] = lr
        opt.step()
        gd = torch.zeros(npad, device=dev); gd[:n] = grad.to(dev)
        ops.adam_step(p[:n], gd[:n], m[:n], v[:n], sh[:n], lr, 0.9, 0.98, 1e-9, step)
    torch.cuda.synchronize()
    np.testing.assert_allclose(p[:n].cpu().numpy(), ref.detach().numpy(), rtol=2e-5, atol=1e-7)
    assert (sh[:n].float().cpu() - p[:n].cpu()).abs().max().item() <= 2 ** -8 * p.abs().max().item()


@pytest.mark.parametrize("B,L,d,M,padcase", [(1, 32, 64, 32, 0), (2, 64, 128, 64, 1), (1, 160, 64, 192, 0),
                                              (2, 256, 128, 256, 1), (1, 512, 128, 512, 0), (3, 416, 128, 416, 1),
                                              (3, 96, 192, 96, 1), (5, 32, 64, 40, 0),
                                              # long sweeps with L % 128 == 32: every main loop of dq_lite / dK/dV plus their tails,
                                              # nine diagonal groups of de_tiles with a ragged last one
                                              (1, 1056, 64, 1056, 1), (2, 800, 64, 1024, 0),
                                              # B % 8 == 0: the dE groups dealt to the XCDs (one batch row each), a ragged second
                                              # diagonal group, the 32-key dK/dV kernel, E longer than L
                                              (8, 160, 64, 192, 1)])
def test_rel_attn_bwd_matches_oracle_autograd(B, L, d, M, padcase):
    """dq/dk/dv/dE of the backward kernels (dK/dV storing dS, dQ and dE from the stored tiles) vs autograd through the oracle
    (fp32, same bf16 inputs)."""
    from musicgeneration_amd import ops
    from oracle import ref_cpu as R
    dev = _dev()
    g = torch.Generator().manual_seed(200 + L + d)
    h = d // 64
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 0.8).to(torch.bfloat16)
    E = (torch.randn(M, 64, generator=g) * 0.5).to(torch.bfloat16)
    dctx = torch.randn(B, L, d, generator=g).to(torch.bfloat16)
    pad = 7
    tok = torch.randint(0, 7, (B, L), generator=g, dtype=torch.int32)
    if padcase:
        tok[0, L - 5:] = pad
        tok[-1, L // 2] = pad
    qr = qkv.float().requires_grad_(True)
    Er = E.float().requires_grad_(True)
    ref_ctx, _, _ = R.attn_core(qr, Er, _mask(tok, pad), h)
    (ref_ctx * dctx.float()).sum().backward()
    bits = ops.pad_bitmap(tok.to(dev), pad) if padcase else None
    qd, Ed = qkv.to(dev), E.to(dev)
    ctx, lse = ops.rel_attn_fwd(qd, Ed, bits)
    dE = torch.zeros(M, 64, device=dev)
    dqkv = ops.rel_attn_bwd(qd, Ed, bits, ctx, dctx.to(dev), lse, dE)
    torch.cuda.synchronize()
    dqkv, dE = dqkv.float().cpu(), dE.cpu()
    assert torch.isfinite(dqkv).all() and torch.isfinite(dE).all()
    for name, lo in (("dq", 0), ("dk", d), ("dv", 2 * d)):
        got, ref = dqkv[..., lo:lo + d], qr.grad[..., lo:lo + d]
        assert _cos(got, ref) > 0.999, f"{name} cos {_cos(got, ref)}"
        assert _relerr(got, ref) < 2e-2, f"{name} relerr {_relerr(got, ref)}"
    assert _cos(dE, Er.grad) > 0.999, f"dE cos {_cos(dE, Er.grad)}"
    assert _relerr(dE, Er.grad) < 2e-2, f"dE relerr {_relerr(dE, Er.grad)}"
    # rows of E that no (i,j) pair can reach (index < M-L) must stay exactly zero
    if M > L:
        assert (dE[:M - L] == 0).all()
    # two independent dE implementations (from the dS tiles the dK/dV kernel stored vs full recomputation) agree to
    # fp32 summation order: both multiply the same bf16 dS and q values
    dE2 = torch.zeros(M, 64, device=dev)
    dq2 = ops.rel_attn_bwd(qd, Ed, bits, ctx, dctx.to(dev), lse, dE2, parts=1 | 16 | 32)
    torch.cuda.synchronize()
    assert (dE2.cpu() - dE).abs().max().item() <= 1e-4 * max(1.0, dE.abs().max().item())
    # ... and two dQ implementations (from the stored tiles vs the recompute kernel, which forms its own dS): bf16 rounding of dS
    dq2 = dq2[..., :d].float().cpu()
    assert (dq2 - dqkv[..., :d]).abs().max().item() <= 2e-2 * dq2.abs().max().item()
    assert _relerr(dqkv[..., :d], dq2) < 5e-3


def _fuzz_cases():
    """32 seeded draws of (B, L, heads, M, pad pattern): lengths around the kernels' structural boundaries (one key tile, one 128-row
    query block, 128-key blocks of the asm dK/dV kernel, L % 128 != 0 -> the 32-key kernel), 1-5 heads, E longer than L, and pads
    trailing / interior / in whole tiles / in every row"""
    import random
    rng = random.Random(20260)
    Ls = [32, 64, 96, 128, 160, 224, 256, 288, 384, 512]
    out = []
    for i in range(32):
        L = rng.choice(Ls)
        out.append((rng.randint(1, 3), L, rng.randint(1, 5), L + rng.choice([0, 0, 32, 100, 1]), rng.choice(["none", "trail", "interior", "both", "tile", "rows"]), i))
    return out


@pytest.mark.parametrize("B,L,heads,M,pads,seed", _fuzz_cases())
def test_rel_attn_fuzz_forward_and_backward_match_oracle(B, L, heads, M, pads, seed):
    """round 6: randomised shapes and pad patterns through mgx_rel_attn_fwd / mgx_rel_attn_bwd against the oracle's autograd --
    tolerances of the fixed-shape tests above (ctx 2e-2 max|ref|, lse 2e-3, gradients cosine >= 0.999 and rel-L2 <= 2e-2).
    No row may be fully masked (position 0 of every row is a real token: the parity contract)."""
    from musicgeneration_amd import ops
    from oracle import ref_cpu as R
    dev = _dev()
    d = 64 * heads
    g = torch.Generator().manual_seed(7000 + seed)
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 0.8).to(torch.bfloat16)
    E = (torch.randn(M, 64, generator=g) * 0.5).to(torch.bfloat16)
    dctx = torch.randn(B, L, d, generator=g).to(torch.bfloat16)
    pad = 9
    tok = torch.randint(0, 9, (B, L), generator=g, dtype=torch.int32)
    if pads in ("trail", "both"):
        for b in range(B):
            n = int(torch.randint(0, L // 2, (1,), generator=g))
            if n:
                tok[b, L - n:] = pad
    if pads in ("interior", "both"):
        idx = torch.randint(1, L, (B, 4), generator=g)
        for b in range(B):
            tok[b, idx[b]] = pad
    if pads == "tile" and L >= 96:
        tok[0, 32:64] = pad                                # a whole key tile of pads inside the sequence
    if pads == "rows":
        tok[:, 1::2] = pad                                 # every second key of every row
    assert (tok[:, 0] != pad).all()
    qr, Er = qkv.float().requires_grad_(True), E.float().requires_grad_(True)
    ref_ctx, _, ref_logits = R.attn_core(qr, Er, _mask(tok, pad), heads)
    (ref_ctx * dctx.float()).sum().backward()
    bits = ops.pad_bitmap(tok.to(dev), pad) if pads != "none" else None
    qd, Ed = qkv.to(dev), E.to(dev)
    ctx, lse = ops.rel_attn_fwd(qd, Ed, bits)
    dE = torch.zeros(M, 64, device=dev)
    dqkv = ops.rel_attn_bwd(qd, Ed, bits, ctx, dctx.to(dev), lse, dE)
    torch.cuda.synchronize()
    ctxc, lsec, dqkv, dE = ctx.float().cpu(), lse.cpu(), dqkv.float().cpu(), dE.cpu()
    assert torch.isfinite(ctxc).all() and torch.isfinite(dqkv).all() and torch.isfinite(dE).all()
    rc = ref_ctx.detach()
    assert (ctxc - rc).abs().max().item() <= 2e-2 * rc.abs().max().item()
    ref_lse = torch.logsumexp(ref_logits.detach(), -1)
    assert (lsec - ref_lse).abs().max().item() < 2e-3 * max(1.0, ref_lse.abs().max().item())
    for name, lo in (("dq", 0), ("dk", d), ("dv", 2 * d)):
        got, ref = dqkv[..., lo:lo + d], qr.grad[..., lo:lo + d]
        assert _cos(got, ref) > 0.999, f"{name} cos {_cos(got, ref)}"
        assert _relerr(got, ref) < 2e-2, f"{name} relerr {_relerr(got, ref)}"
    assert _cos(dE, Er.grad) > 0.999 and _relerr(dE, Er.grad) < 2e-2
    if M > L:
        assert (dE[:M - L] == 0).all()


@pytest.mark.parametrize("M,N,K,act", [(128, 128, 64, 0), (300, 340, 128, 0), (1000, 1536, 512, 0),
                                        (257, 256, 512, 1), (64, 64, 256, 1), (32, 1536, 512, 0), (7, 308, 320, 1),
                                        (2048, 512, 512, 0), (2304, 384, 64, 1), (4100, 340, 192, 0),
                                        (1, 384, 512, 0), (32, 512, 256, 0)])
def test_linear_fwd(M, N, K, act):
    from musicgeneration_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    bias = torch.randn(N, generator=g)
    ref = a.float() @ w.float().t() + bias
    if act:
        ref = torch.relu(ref)
    out = ops.linear_fwd(a.to(dev), w.to(dev), bias.to(dev), act)
    torch.cuda.synchronize()
    err = (out.float().cpu() - ref).abs().max().item()
    assert err <= 2 ** -7 * ref.abs().max().item() + 1e-3, err
    out2 = ops.linear_fwd(a.to(dev), w.to(dev), None, 0)
    assert _relerr(out2.cpu(), a.float() @ w.float().t()) < 5e-3


@pytest.mark.parametrize("M,N,K,relu", [(128, 128, 128, 0), (300, 384, 512, 0), (1000, 1536, 512, 0),
                                         (257, 512, 256, 1), (2048, 256, 512, 0), (96, 64, 64, 1)])
def test_linear_backward_kernels(M, N, K, relu):
    """dX = dY W (optionally masked by relu(x) > 0) and gW += dY^T X, gb += colsum(dY)."""
    from musicgeneration_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(3 * M + N + K)
    dy = torch.randn(M, N, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    if relu:
        x = torch.relu(x)
    ref_dx = dy.float() @ w.float()
    if relu:
        ref_dx = ref_dx * (x.float() > 0)
    dx = ops.linear_dx(dy.to(dev), w.to(dev), x.to(dev) if relu else None)
    torch.cuda.synchronize()
    assert _relerr(dx.cpu(), ref_dx) < 5e-3
    assert (dx.float().cpu() - ref_dx).abs().max().item() <= 2 ** -7 * ref_dx.abs().max().item() + 1e-3
    # residual-gradient addend joins after the mask
    add = torch.randn(M, K, generator=g).to(torch.bfloat16)
    dx2 = ops.linear_dx(dy.to(dev), w.to(dev), x.to(dev) if relu else None, add.to(dev))
    ref2 = ref_dx + add.float()
    assert (dx2.float().cpu() - ref2).abs().max().item() <= 2 ** -7 * ref2.abs().max().item() + 1e-3
    with pytest.raises(ValueError):
        ops.linear_dx(dy.to(dev), w.to(dev), None, add.to(dev).float())
    gw0 = torch.randn(N, K, generator=g)
    gb0 = torch.randn(N, generator=g)
    gw, gb = gw0.clone().to(dev), gb0.clone().to(dev)
    ops.linear_dw(dy.to(dev), x.to(dev), gw, gb)
    ops.linear_dw(dy.to(dev), x.to(dev), gw, None)            # accumulates: called twice -> 2x
    torch.cuda.synchronize()
    ref_gw = gw0 + 2 * (dy.float().t() @ x.float())
    ref_gb = gb0 + dy.float().sum(0)
    assert _relerr(gw.cpu(), ref_gw) < 1e-4
    assert _relerr(gb.cpu(), ref_gb) < 1e-4


def _gemm_fuzz_cases():
    import random
    rng = random.Random(606)
    out = []
    for i in range(24):
        M = rng.choice([1, 7, 32, 33, 100, 257, 1000, 2048, 4099, 8192, 16384 + 32 * rng.randint(0, 3)])
        N = 8 * rng.randint(1, 96)
        K = 64 * rng.randint(1, 12)
        out.append((M, N, K, rng.randint(0, 1), i))
    return out


@pytest.mark.parametrize("M,N,K,act,seed", _gemm_fuzz_cases())
def test_linear_fuzz_all_three_gemms_match_fp32(M, N, K, act, seed):
    """round 6: randomised (M, N, K) through mgx_linear_fwd / mgx_linear_dx / mgx_linear_dw -- ragged tiles, one row, widths that are
    no multiple of the 128 / 256 tiles, reduction lengths with a tail (dX reduces over N, any multiple of 8) -- against an fp32 product
    of the same bf16 operands on the GPU; tolerances of test_linear_fwd / test_linear_backward_kernels"""
    from musicgeneration_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(9000 + seed)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    ref = a.float() @ w.float().t() + bias
    if act:
        ref = ref.relu()
    out = ops.linear_fwd(a, w, bias, act)
    assert (out.float() - ref).abs().max().item() <= 2 ** -7 * ref.abs().max().item() + 1e-3
    dy = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev)
    y = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    add = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    wd = (torch.randn(N, K, generator=g) / math.sqrt(N)).to(torch.bfloat16).to(dev)
    rdx = dy.float() @ wd.float()
    for relu_y, addend in ((None, None), (y, None), (None, add), (y, add)):
        r = rdx * (relu_y.float() > 0) if relu_y is not None else rdx
        r = r + addend.float() if addend is not None else r
        dx = ops.linear_dx(dy, wd, relu_y, addend)
        assert (dx.float() - r).abs().max().item() <= 2 ** -6 * r.abs().max().item() + 1e-3, (relu_y is not None, addend is not None)
    gw0, gb0 = torch.randn(N, K, generator=g).to(dev), torch.randn(N, generator=g).to(dev)
    gw, gb = gw0.clone(), gb0.clone()
    ops.linear_dw(dy, a, gw, gb)
    torch.cuda.synchronize()
    rw, rb = gw0 + dy.float().t() @ a.float(), gb0 + dy.float().sum(0)
    assert _relerr(gw, rw) < 1e-4 and _relerr(gb, rb) < 1e-4


def test_linear_dw_grouped_matches_separate_launches():
    """one launch for several weight gradients == the per-weight launches (same kernels body, other M-split)"""
    from musicgeneration_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(11)
    M = 1500
    shapes = [(384, 128), (128, 128), (64, 128), (128, 64)]          # (N, K) like QKV / fc / FFN_pre / FFN_suf
    probs, refs = [], []
    for i, (N, K) in enumerate(shapes):
        dy = torch.randn(M, N, generator=g).to(torch.bfloat16).to(dev)
        x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
        gw0 = torch.randn(N, K, generator=g).to(dev)
        gb0 = torch.randn(N, generator=g).to(dev) if i % 2 == 0 else None
        gw, gb = gw0.clone(), (gb0.clone() if gb0 is not None else None)
        probs.append((dy, x, gw, gb))
        refs.append((gw0 + dy.float().t() @ x.float(), None if gb0 is None else gb0 + dy.float().sum(0)))
    ops.linear_dw_grouped(probs)
    torch.cuda.synchronize()
    for (dy, x, gw, gb), (rw, rb) in zip(probs, refs):
        assert _relerr(gw.cpu(), rw.cpu()) < 1e-4
        if gb is not None:
            assert _relerr(gb.cpu(), rb.cpu()) < 1e-4
    with pytest.raises(ValueError):
        ops.linear_dw_grouped([probs[0], (probs[1][0][:100], probs[1][1][:100], probs[1][2], None)])


@pytest.mark.parametrize("M,N,K,act", [(32, 256, 512, 1), (7, 1536, 512, 0), (1, 384, 768, 0), (32, 96, 1024, 1), (5, 40, 64, 0)])
def test_linear_ln_fwd(M, N, K, act):
    """decode fusion: Z = LN(X + RES), C = act(Z W^T + b) vs the two separate kernels and vs fp32 torch"""
    from musicgeneration_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    res = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev)
    gamma = (1 + 0.1 * torch.randn(K, generator=g)).to(dev)
    beta = (0.1 * torch.randn(K, generator=g)).to(dev)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).to(dev)
    bias = torch.randn(N, generator=g).to(dev)
    c, z = ops.linear_ln_fwd(x, res, gamma, beta, w, bias, act)
    z_ref = ops.add_ln_fwd(x, res, gamma, beta, 1e-6)[0]
    c_ref = ops.linear_fwd(z_ref, w, bias, act)
    torch.cuda.synchronize()
    zf = torch.nn.functional.layer_norm(x.float() + res.float(), (K,), gamma, beta, 1e-6)
    assert (z.float() - zf).abs().max().item() <= 2 ** -7 * zf.abs().max().item() + 1e-3
    assert (z.float() - z_ref.float()).abs().max().item() <= 2 ** -6 * zf.abs().max().item()      # <= 1-2 bf16 ulp apart
    cf = zf @ w.float().t() + bias
    if act:
        cf = torch.relu(cf)
    assert (c.float() - cf).abs().max().item() <= 2e-2 * cf.abs().max().item() + 2e-2
    assert (c.float() - c_ref.float()).abs().max().item() <= 2e-2 * cf.abs().max().item() + 2e-2
    with pytest.raises(ops._lib.MgxError):
        ops.linear_ln_fwd(torch.zeros(33, K, dtype=torch.bfloat16, device=dev), torch.zeros(33, K, dtype=torch.bfloat16, device=dev),
                          gamma, beta, w, bias, act)


def test_rel_attn_fwd_redoes_a_main_loop_tile_that_leaves_the_safe_range():
    """The lazy softmax of the forward keeps one reference per query row and redoes a tile against the true maximum when a
    lane's tile sum leaves the safe range (then rescales O and l once).  Every sweep does that on its first tile; here it must
    ALSO happen deep inside the branch-free-looking main loop: key 70 (key tile 2, below the diagonal block of every query block
    from the second on) beats the reference of query row 400 by 128 nats and of row 300 by 64.  Both rows, and every other row
    of those workgroups, must match the oracle."""
    from musicgeneration_amd import ops
    from oracle import ref_cpu as R
    dev = torch.device("cuda")
    B, L, d = 2, 512, 128
    g = torch.Generator().manual_seed(17)
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 0.3).to(torch.bfloat16)
    E = (torch.randn(L, 64, generator=g) * 0.3).to(torch.bfloat16)
    qkv[0, 400, :64] = 4.0          # head 0: query row 400 (query block 3) ...
    qkv[0, 70, d:d + 64] = 4.0      # ... and key 70: logit 64 * 16 / 8 = 128
    qkv[0, 300, :64] = 2.0          # query block 2: 64 nats above its reference
    qkv[1, 200, 64:128] = -4.0      # head 1 of batch row 1: the same key pattern strongly NEGATIVE (no restart there)
    qkv[1, 70, d + 64:d + 128] = 4.0
    tok = torch.zeros(B, L, dtype=torch.int32)
    ref_ctx, _, _ = R.attn_core(qkv.float(), E.float(), R.look_ahead_mask(tok, 9), d // 64)
    ctx, lse = ops.rel_attn_fwd(qkv.to(dev), E.to(dev), None)
    torch.cuda.synchronize()
    ctx = ctx.float().cpu()
    assert torch.isfinite(ctx).all() and torch.isfinite(lse).all()
    assert (ctx - ref_ctx).abs().max().item() <= 2e-2 * ref_ctx.abs().max().item()
    # the dominated rows attend to key 70 alone
    v70 = qkv[0, 70, 2 * d:2 * d + 64].float()
    assert (ctx[0, 400, :64] - v70).abs().max().item() < 2e-2
    assert abs(lse.view(B, d // 64, L)[0, 0, 400].item() - 128.0) < 4.0          # 128 + the relative term of that pair


def test_deterministic_mode_kernels_repeat_and_agree_with_the_default():
    """mgx_set_deterministic: the kernels that end in atomics (dE, single-weight dW / db, embedding gradient, CE statistics), run
    twice on the same inputs, give identical bits; against the default (fp32 atomics) they differ only by summation order and the
    2^-30 quantisation of the partial sums."""
    from musicgeneration_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(77)
    B, L, d, V = 3, 256, 128, 90
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 0.7).to(torch.bfloat16).to(dev)
    E = (torch.randn(L, 64, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    dctx = torch.randn(B, L, d, generator=g).to(torch.bfloat16).to(dev)
    ctx, lse = ops.rel_attn_fwd(qkv, E, None)
    tok = torch.randint(0, V, (B, L), generator=g, dtype=torch.int32).to(dev)
    dout = torch.randn(B, L, d, generator=g).to(torch.bfloat16).to(dev)
    M = 4096
    dy = torch.randn(M, 384, generator=g).to(torch.bfloat16).to(dev)
    x = torch.randn(M, 128, generator=g).to(torch.bfloat16).to(dev)
    logits = (torch.randn(B * L, V, generator=g) * 3).to(torch.bfloat16).to(dev)
    tgt = torch.randint(0, V, (B * L,), generator=g, dtype=torch.int32).to(dev)

    def run():
        dE = torch.zeros(L, 64, device=dev)
        ops.rel_attn_bwd(qkv, E, None, ctx, dctx, lse, dE)
        dtab = torch.zeros(V, d, device=dev)
        ops.embed_bwd(tok, dout, dtab, 0.1, 5)
        gw, gb = torch.zeros(384, 128, device=dev), torch.zeros(384, device=dev)
        ops.linear_dw(dy, x, gw, gb)
        stats, _, _ = ops.smooth_ce_fwd(logits, tgt, V, 0.1, V - 1)
        torch.cuda.synchronize()
        return [t.clone() for t in (dE, dtab, gw, gb, stats)]

    plain = run()
    assert not ops.deterministic()
    ops.set_deterministic(True)
    try:
        assert ops.deterministic()
        d1, d2 = run(), run()
    finally:
        ops.set_deterministic(False)
    assert not ops.deterministic()
    for a, b, p, name in zip(d1, d2, plain, ("dE", "dtable", "gW", "gb", "stats")):
        assert torch.equal(a, b), name
        assert _relerr(a, p) < 1e-5, (name, _relerr(a, p))
        assert (a - p).abs().max().item() <= 1e-5 * p.abs().max().item() + 1e-8, name


def test_deterministic_mode_keeps_a_nan_a_nan():
    """a NaN / Inf / out-of-range partial has no fixed-point image; in deterministic mode it must poison its destination
    (fold -> NaN) instead of silently becoming a finite number -- a diverging run has to stay recognisable from its gradients."""
    from musicgeneration_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    B, L, d, V, M = 2, 128, 128, 50, 2048
    tok = torch.randint(0, V, (B, L), generator=g, dtype=torch.int32)
    tok[0, 3] = 7
    dout = torch.randn(B, L, d, generator=g).to(torch.bfloat16)
    dout[0, 3, 17] = float("nan")                    # -> dtable[7, 17]
    dout[1, 9, 40] = float("inf")                    # -> dtable[tok[1, 9], 40]
    dy = torch.randn(M, 384, generator=g).to(torch.bfloat16)
    x = torch.randn(M, 128, generator=g).to(torch.bfloat16)
    dy[100, 5] = float("nan")                        # -> gW[5, :], gb[5]
    logits = (torch.randn(B * L, V, generator=g) * 3).to(torch.bfloat16)
    logits[11, 3] = float("nan")                     # -> the loss statistic
    tgt = torch.randint(0, V - 1, (B * L,), generator=g, dtype=torch.int32)
    ops.set_deterministic(True)
    try:
        dtab = torch.zeros(V, d, device=dev)
        ops.embed_bwd(tok.to(dev), dout.to(dev), dtab, 0.0, 5)
        gw, gb = torch.zeros(384, 128, device=dev), torch.zeros(384, device=dev)
        ops.linear_dw(dy.to(dev), x.to(dev), gw, gb)
        stats, _, _ = ops.smooth_ce_fwd(logits.to(dev), tgt.to(dev), V, 0.1, V - 1)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(False)
    dtab, gw, gb, stats = dtab.cpu(), gw.cpu(), gb.cpu(), stats.cpu()
    assert torch.isnan(dtab[7, 17]) and torch.isnan(dtab[tok[1, 9], 40])
    assert torch.isfinite(dtab).sum().item() == dtab.numel() - 2          # nothing else was touched
    assert torch.isnan(gw[5]).all() and torch.isnan(gb[5])
    assert torch.isfinite(gw[:5]).all() and torch.isfinite(gw[6:]).all() and torch.isfinite(gb[:5]).all() and torch.isfinite(gb[6:]).all()
    assert torch.isnan(stats[0])                                            # the loss sum


def test_deterministic_mode_poison_is_sticky():
    """a poisoned destination must stay poisoned whatever arrives later.  Until round 6 the poison was a signed max with
    2^62 on the sum word itself, and two later partials of about -1.5e9 (each a legal fixed-point value) carried the word back into
    the valid band: NaN + (-1.5e9) + (-1.5e9) folded to a finite number.  Exactly that: a weight gradient whose 256 M-splits hold one
    NaN partial, two partials of -1.5e9 and 253 zeros for element [0, 0] (mgx_linear_dw: one 128 x 128 tile, 64-row splits)."""
    from musicgeneration_amd import _lib, ops
    dev = _dev()
    M, N, K = 16384, 64, 64
    dy = torch.zeros(M, N, dtype=torch.bfloat16)
    x = torch.zeros(M, K, dtype=torch.bfloat16)
    x[:, 0] = 1.0
    x[:, 1] = 1.0
    dy[0:64, 0] = float("nan")                       # split 0 -> NaN partial
    dy[64:192, 0] = -2.34e7                          # splits 1, 2: 64 rows x -2.34e7 = -1.5e9 each (bf16 holds 2.34e7 to 3 digits)
    dy[0:64, 1] = 3.0                                # a clean column beside it
    ops.set_deterministic(True)
    try:
        gw, gb = torch.zeros(N, K, device=dev), torch.zeros(N, device=dev)
        lib = _lib.load()
        dyd, xd = dy.to(dev), x.to(dev)
        _lib.check(lib.mgx_linear_dw(ops.ptr(dyd), ops.ptr(xd), ops.ptr(gw), ops.ptr(gb), M, N, K, ops.stream_ptr()), "mgx_linear_dw")
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(False)
    gw, gb = gw.cpu(), gb.cpu()
    assert torch.isnan(gw[0, 0]) and torch.isnan(gw[0, 1]) and torch.isnan(gb[0])
    assert gw[1, 0].item() == 192.0 and gw[1, 1].item() == 192.0 and gb[1].item() == 192.0
    assert torch.isfinite(gw[1:]).all() and torch.isfinite(gb[1:]).all()


@pytest.mark.parametrize("B,L,d", [(2, 256, 128), (1, 1024, 64), (3, 512, 192), (2, 2048, 128), (1, 640, 64)])
def test_dkv64_matches_the_32_key_kernel_bitwise(B, L, d):
    """The 64-keys-per-wave dK/dV kernel whose whole sweep is the generated, hand-scheduled asm block (rel_attn_dkv64.hip,
    gen_dkv_asm.py; parts bit 2 where L % 128 == 0) against the HIP 32-key kernel (parts bit 6): the same arithmetic per tile in the
    same accumulation order, so dk, dv and every stored dS tile -- the whole workspace -- must be equal BIT FOR BIT, without and with
    padded keys (the masked bodies then run for every step of the padded key blocks).  L = 640: five key blocks, sweeps of 4..20 tiles
    (every exit point of the six-body loops)."""
    from musicgeneration_amd import ops
    dev = _dev()
    g = torch.Generator().manual_seed(L + d)
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 0.7).to(torch.bfloat16).to(dev)
    E = (torch.randn(L, 64, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    dctx = torch.randn(B, L, d, generator=g).to(torch.bfloat16).to(dev)
    tok = torch.zeros(B, L, dtype=torch.int32)
    tok[0, L - 37:] = 5                                   # trailing pads in batch row 0: its last two key blocks take the masked bodies
    tok[B - 1, L - 150:] = 5
    n = ops._lib.load().mgx_rel_attn_bwd_workspace(B, L, d)
    for bits in (None, ops.pad_bitmap(tok.to(dev), 5)):
        ctx, lse = ops.rel_attn_fwd(qkv, E, bits)
        ws1 = torch.zeros(n, dtype=torch.uint8, device=dev)
        ws2 = torch.zeros(n, dtype=torch.uint8, device=dev)
        dE = torch.zeros(L, 64, device=dev)
        dq1, dq2 = torch.zeros_like(qkv), torch.zeros_like(qkv)
        ops.rel_attn_bwd(qkv, E, bits, ctx, dctx, lse, dE, 1 | 64, dq1, ws1)          # 32-key kernel
        ops.rel_attn_bwd(qkv, E, bits, ctx, dctx, lse, dE, 1 | 4, dq2, ws2)           # 64-key kernel, asm sweep
        torch.cuda.synchronize()
        assert torch.isfinite(dq2.float()).all()
        assert torch.equal(dq1[..., d:], dq2[..., d:]), "dk / dv"
        assert torch.equal(ws1, ws2), "dS tiles"


def test_dkv_falls_back_to_the_32_key_kernel_when_the_sequence_is_not_whole_key_blocks():
    """L % 128 != 0: parts bit 2 runs the 32-key kernel (the 64-key kernel needs whole 128-key blocks) -- same bits as bit 6"""
    from musicgeneration_amd import ops
    dev = _dev()
    B, L, d = 2, 352, 64
    g = torch.Generator().manual_seed(3)
    qkv = (torch.randn(B, L, 3 * d, generator=g) * 0.7).to(torch.bfloat16).to(dev)
    E = (torch.randn(L, 64, generator=g) * 0.5).to(torch.bfloat16).to(dev)
    dctx = torch.randn(B, L, d, generator=g).to(torch.bfloat16).to(dev)
    ctx, lse = ops.rel_attn_fwd(qkv, E, None)
    dE = torch.zeros(L, 64, device=dev)
    a = ops.rel_attn_bwd(qkv, E, None, ctx, dctx, lse, dE, 1 | 4)
    b = ops.rel_attn_bwd(qkv, E, None, ctx, dctx, lse, dE, 1 | 64)
    torch.cuda.synchronize()
    assert torch.equal(a[..., d:], b[..., d:])
    with pytest.raises(Exception):
        ops.rel_attn_bwd(qkv, E, None, ctx, dctx, lse, dE, 4 | 64)                   # both write dk / dv
