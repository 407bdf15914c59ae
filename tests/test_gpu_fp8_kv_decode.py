"""The opt-in 8-bit K/V cache of the KV-cache decode (ABI 20): OCP e4m3fn codes with one f32 scale per (b, h, row).
Kernel level: the quantizer is bit-exact with its torch twin, the attention is attention over the dequantized rows.  Model
level: generate_cached(kv_cache="fp8") against an fp32 model whose K and V pass through the same quantizer, and with every
option of the cached decode."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from decode_fixtures import one, tame_model
from oracle.decode_ref import dequant, quant_twin

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
BF = torch.bfloat16
SENTINEL = 0xA5


def _special_rows(x, g):
    """x [..., 64] f32 rows (flattened view): an all-zero row, one large outlier that pushes the rest into subnormal codes,
    an all-negative row and a power-of-two amax"""
    r = x.reshape(-1, 64)
    r[0] = 0
    r[1] = 1e-3 * torch.randn(64, generator=g)
    r[1, 5] = 7.5
    r[2] = -r[2].abs()
    r[3] = r[3].clamp(-0.99, 0.99)
    r[3, 60] = 1.0
    return x


# ---------------------------------------------------------------------------------------------------------------------
# 1. the quantizer, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def test_kv_store_fp8_is_bit_exact_with_the_torch_twin():
    from musicgeneration_amd import ops
    g = torch.Generator().manual_seed(0)
    B, d, Lrows, n, Lmax = 3, 256, 64, 45, 50
    h = d // 64
    qkv = torch.randn(B, Lrows, 3 * d, generator=g)
    k_spec = qkv[0, :4, d:d + 64]
    k_spec.copy_(_special_rows(k_spec.clone(), g))
    v_spec = qkv[2, 10:14, 2 * d + 64:2 * d + 128]
    v_spec.copy_(_special_rows(v_spec.clone(), g))
    qkv = qkv.to(BF)
    kc = torch.full((B, h, Lmax, 64), SENTINEL, dtype=torch.uint8, device=DEV)
    vc = kc.clone()
    ks = torch.full((B, h, Lmax), -7.0, device=DEV)
    vs = ks.clone()
    ops.kv_store_fp8(qkv.to(DEV).contiguous(), n, kc, vc, ks, vs)
    torch.cuda.synchronize()
    for col, codes, scales in ((1, kc, ks), (2, vc, vs)):
        rows = qkv[:, :n, col * d:(col + 1) * d].reshape(B, n, h, 64).permute(0, 2, 1, 3)
        want_c, want_s = quant_twin(rows)
        got_c, got_s = codes.cpu(), scales.cpu()
        assert torch.equal(got_c[:, :, :n], want_c), (got_c[:, :, :n] != want_c).nonzero()[:5]
        assert torch.equal(got_s[:, :, :n], want_s)
        assert (got_c[:, :, n:] == SENTINEL).all() and (got_s[:, :, n:] == -7.0).all()      # rows >= n untouched
    # the special rows are what they claim to be
    assert not kc[0, 0, 0].any() and ks[0, 0, 0] == 0
    sub = kc[0, 0, 1].cpu() & 0x7F
    assert ((sub >> 3) == 0).logical_and(sub != 0).any()                                  # subnormal codes
    assert ks[0, 0, 3].item() == (torch.tensor(1.0) / 448.0).item()                       # amax 1.0
    assert (kc[0, 0, 2].cpu() >= 0x80).logical_or(kc[0, 0, 2].cpu() == 0).all()           # negative
    ops.kv_store_fp8(qkv.to(DEV).contiguous(), 0, kc, vc, ks, vs)                         # n = 0: nothing


# ---------------------------------------------------------------------------------------------------------------------
# 2. the attention kernel against attention over the dequantized caches
# ---------------------------------------------------------------------------------------------------------------------
def _random_fp8_cache(B, h, Lmax, g):
    x = torch.randn(B, h, Lmax, 64, generator=g)
    x = x * torch.exp(0.5 * torch.randn(B, h, Lmax, 1, generator=g))                      # rows of different magnitude
    return quant_twin(x)


def _attention_over_dequantized(qkv, kc, ks, vc, vs, E, b, t):
    """ctx row b [d] at position t: rows 0..t-1 from the caches, row t quantized from qkv (all f32, CPU)"""
    d = qkv.shape[1] // 3
    h, M = d // 64, E.shape[0]
    out = torch.empty(d)
    for hd in range(h):
        q = qkv[b, hd * 64:(hd + 1) * 64].float()
        kt_c, kt_s = quant_twin(qkv[b, d + hd * 64:d + (hd + 1) * 64])
        vt_c, vt_s = quant_twin(qkv[b, 2 * d + hd * 64:2 * d + (hd + 1) * 64])
        K = torch.cat([dequant(kc[b, hd, :t], ks[b, hd, :t]), dequant(kt_c[None], kt_s[None])], 0)
        Vv = torch.cat([dequant(vc[b, hd, :t], vs[b, hd, :t]), dequant(vt_c[None], vt_s[None])], 0)
        j = torch.arange(t + 1)
        Er = E[M - 1 - (t - j)].float()
        s = (K @ q + Er @ q) / 8.0
        out[hd * 64:(hd + 1) * 64] = torch.softmax(s, 0) @ Vv
    return out


@pytest.mark.parametrize("Lmax,B", [(300, 5), (2048, 4)])
def test_fp8_attention_is_attention_over_the_dequantized_rows(Lmax, B):
    """one split (Lmax < 1024) and split-K; uniform at t = 0, Lmax - 1 and in between, and ragged with per-row t (0 and Lmax-1
    included): the appended row t is the quantizer's, ctx is fp32 attention over the dequantized rows to bf16 output
    rounding, and the ragged kernel equals the uniform one bit for bit, row by row"""
    from musicgeneration_amd import ops
    d = 256
    h, M = d // 64, Lmax + 16
    if Lmax >= 1024:
        assert ops.rel_attn_decode_splits(B, Lmax, d) > 1
    g = torch.Generator().manual_seed(Lmax + B)
    kc0, ks0 = _random_fp8_cache(B, h, Lmax, g)
    vc0, vs0 = _random_fp8_cache(B, h, Lmax, g)
    qkv = (0.5 * torch.randn(B, 3 * d, generator=g)).to(BF)
    qkv[0, d:d + 64] = 0                                                    # an all-zero new K row of (b 0, head 0)
    E = (0.3 * torch.randn(M, 64, generator=g)).to(BF)
    ws = ops.rel_attn_decode_workspace(B, Lmax, d, DEV)
    dev = [t.to(DEV) for t in (kc0, ks0, vc0, vs0)]
    qd, Ed = qkv.to(DEV), E.to(DEV)

    def run(pos, ragged):
        kc, ks, vc, vs = (t.clone() for t in dev)
        ctx = ops.rel_attn_decode(qd, kc, vc, Ed, pos, torch.empty(B, d, dtype=BF, device=DEV), ws, ragged=ragged,
                                  kscale=ks, vscale=vs)
        torch.cuda.synchronize()
        return ctx.cpu(), kc.cpu(), ks.cpu(), vc.cpu(), vs.cpu()

    def check_row(b, t, ctx, kc, ks, vc, vs):
        for col, codes, scales in ((1, kc, ks), (2, vc, vs)):
            want_c, want_s = quant_twin(qkv[b, col * d:(col + 1) * d].reshape(h, 64))
            assert torch.equal(codes[b, :, t], want_c) and torch.equal(scales[b, :, t], want_s), (b, t, col)
        other = torch.ones(Lmax, dtype=torch.bool)
        other[t] = False
        assert torch.equal(kc[b, :, other], kc0[b, :, other]) and torch.equal(vs[b, :, other], vs0[b, :, other])
        ref = _attention_over_dequantized(qkv, kc0, ks0, vc0, vs0, E, b, t)
        err = (ctx[b].float() - ref).abs()
        assert (err <= 2 ** -8 * ref.abs() + 2e-3 * ref.abs().max()).all(), (b, t, err.max().item())

    for t in (0, 97, Lmax - 1):
        ctx, kc, ks, vc, vs = run(one(t), False)
        for b in range(B):
            check_row(b, t, ctx, kc, ks, vc, vs)
    pos = torch.randint(0, Lmax, (B,), generator=g, dtype=torch.int32)
    pos[0], pos[1] = 0, Lmax - 1
    ctx, kc, ks, vc, vs = run(pos.to(DEV), True)
    for b in range(B):
        check_row(b, int(pos[b]), ctx, kc, ks, vc, vs)
        c1, k1, s1, v1, t1 = run(one(pos[b]), False)
        assert torch.equal(ctx[b], c1[b]) and torch.equal(kc[b], k1[b]) and torch.equal(ks[b], s1[b]), b
        assert torch.equal(vc[b], v1[b]) and torch.equal(vs[b], t1[b]), b


# ---------------------------------------------------------------------------------------------------------------------
# 3. model level: against an fp32 model whose K and V pass through the quantizer
# ---------------------------------------------------------------------------------------------------------------------
def _fp8_emulating_probs(p, x, pad):
    """the causal fp32 stack of oracle.ref_cpu with every layer's K and V quantized (per (b, row, head)) before attn_core"""
    from oracle import ref_cpu as R
    B, L = x.shape
    emb = p["Decoder.embedding.weight"]
    d = emb.shape[1]
    h = d // 64
    mask = R.look_ahead_mask(x, pad)
    hc = emb[x.long()] * math.sqrt(d) + R.sinusoid_table(L, d).to(torch.float32)[None]
    for li in range(R.num_layers_of(p)):
        pre = f"Decoder.enc_layers.{li}."
        qkv = torch.cat([R._lin(hc, p[pre + f"rga.W{c}.weight"], p[pre + f"rga.W{c}.bias"]) for c in "qkv"], -1)
        codes, sc = quant_twin(qkv[..., d:].reshape(B, L, 2 * h, 64))
        qkv = torch.cat([qkv[..., :d], dequant(codes, sc).reshape(B, L, 2 * d)], -1)
        ctx, _, _ = R.attn_core(qkv, p[pre + "rga.E"], mask, h)
        a = R._lin(ctx, p[pre + "rga.fc.weight"], p[pre + "rga.fc.bias"])
        o1 = F.layer_norm(a + hc, (d,), p[pre + "layernorm1.weight"], p[pre + "layernorm1.bias"], 1e-6)
        f = R._lin(F.relu(R._lin(o1, p[pre + "FFN_pre.weight"], p[pre + "FFN_pre.bias"])), p[pre + "FFN_suf.weight"],
                   p[pre + "FFN_suf.bias"])
        hc = F.layer_norm(o1 + f, (d,), p[pre + "layernorm2.weight"], p[pre + "layernorm2.bias"], 1e-6)
    return torch.softmax(R._lin(hc, p["fc.weight"], p["fc.bias"]), -1)


@pytest.mark.parametrize("d,nl,L,B", [(128, 2, 96, 3), (512, 6, 2048, 1)])
def test_fp8_cache_decode_matches_an_fp8_emulating_fp32_model(d, nl, L, B):
    from musicgeneration_amd import ops
    from oracle import ref_cpu as R
    V = 337
    if L >= 1024:
        assert ops.rel_attn_decode_splits(B, L, d) > 1
    mt, p0 = tame_model(d=d, nl=nl, L=L, V=V, seed=21)
    g = torch.Generator().manual_seed(23)
    x = torch.randint(0, V - 1, (B, L), generator=g)
    toks, probs = mt.generate_cached(x.cuda(), 0, return_probs=True, kv_cache="fp8")
    _, probs16 = mt.generate_cached(x.cuda(), 0, return_probs=True)
    torch.cuda.synchronize()
    assert (toks.cpu() == x).all()
    probs, probs16 = probs.cpu(), probs16.cpu()
    with torch.no_grad():
        emu = _fp8_emulating_probs(p0, x, V - 1)
        ref = torch.softmax(R.model_forward(p0, x, V - 1)[0], -1)
    err = (probs - emu).abs().max().item()
    agree = (probs.argmax(-1) == emu.argmax(-1)).float().mean().item()
    err32, err32_bf16 = (probs - ref).abs().max().item(), (probs16 - ref).abs().max().item()
    print(f"\nd {d} layers {nl} L {L}: fp8 cache vs fp8-emulating fp32 model: max {err:.3e}, argmax agreement {agree:.4f}; "
          f"vs the unquantized fp32 oracle: fp8 cache {err32:.3e}, bf16 cache {err32_bf16:.3e}")
    assert err < 2e-2 and agree >= 0.97, (err, agree)
    # the quantization error of the cache itself, against the unquantized fp32 oracle, with the bf16 cache's beside it.
    # Measured on one MI355X: 2.4e-4 (bf16 cache 2.0e-4) at d 128 / L 96 and 3.0e-4 (bf16 cache 3.2e-4) at d 512 / L 2048;
    # the bound keeps a margin of three over the larger one
    assert err32 < 1e-3, (err32, err32_bf16)
    assert abs(probs.sum(-1) - 1).max().item() < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 4. the two prefill paths
# ---------------------------------------------------------------------------------------------------------------------
def test_batched_and_token_prefill_fill_the_same_fp8_caches():
    """the batched prefill (ops.kv_store_fp8 on the full-sequence projections) and the token prefill (the decode kernel's
    append) quantize rows that differ by GEMM rounding (2e-2 of a row's largest element at most, the bf16 cache's bound in
    test_gpu_decode.py): the dequantized caches agree to that rounding, plus one fp8 step (2^-3 of the element) where it
    moves an element across an fp8 rounding boundary.  Measured: 1.5 % of the elements of a layer moved by more than 2e-2 of
    the row maximum, the relative norm of the difference stays at bf16 level"""
    mt, _ = tame_model(L=128)
    V, B, P = 337, 2, 70
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, V - 1, (B, P), generator=g).cuda()
    (ta, pa), ka, va, ksa, vsa = mt.generate_cached(x, 1, top_k=1, return_probs=True, prefill="token", return_cache=True,
                                                    kv_cache="fp8")
    tb, kb, vb, ksb, vsb = mt.generate_cached(x, 1, top_k=1, prefill="batched", return_cache=True, kv_cache="fp8")
    torch.cuda.synchronize()
    for i in range(len(ka)):
        for ca, sa, cb, sb, nm in ((ka[i], ksa[i], kb[i], ksb[i], "K"), (va[i], vsa[i], vb[i], vsb[i], "V")):
            a, b = dequant(ca[:, :, :P], sa[:, :, :P]).cpu(), dequant(cb[:, :, :P], sb[:, :, :P]).cpu()
            amax = a.abs().amax(-1, keepdim=True)
            assert ((sa[:, :, :P] - sb[:, :, :P]).abs() <= 2e-2 * sa[:, :, :P]).all(), f"layer {i} {nm} scales"
            diff = (a - b).abs()
            assert (diff <= 2 ** -3 * a.abs().maximum(b.abs()) + 2e-2 * amax).all(), f"layer {i} {nm} cache"
            assert ((a - b).norm() / a.norm()).item() < 2e-2, f"layer {i} {nm} cache: relative norm of the difference"
    p_last = pa[:, P - 1]
    top2 = p_last.topk(2, -1).values
    clear = (top2[:, 0] - top2[:, 1]) > 5e-2
    assert (ta[:, P][clear] == tb[:, P][clear]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. every option of the cached decode
# ---------------------------------------------------------------------------------------------------------------------
def test_fp8_cfg5_sized_graph_replay_equals_eager_greedy():
    """batch 32, d 512, 6 layers, a 1500-event prompt (split-K attention + merge): greedy tokens by graph replay = eager"""
    from musicgeneration_amd import ops
    mt, _ = tame_model(d=512, nl=6, L=2048, V=337, seed=5)
    V, B, P, n = 337, 32, 1500, 48
    assert ops.rel_attn_decode_splits(B, P + n, 512) > 1
    g = torch.Generator().manual_seed(56)
    prompt = torch.randint(0, V - 1, (B, P), generator=g).cuda()
    a = mt.generate_cached(prompt, n, top_k=1, seed=3, use_graph=True, prefill="batched", kv_cache="fp8")
    b = mt.generate_cached(prompt, n, top_k=1, seed=3, use_graph=False, prefill="batched", kv_cache="fp8")
    torch.cuda.synchronize()
    assert a.shape == (B, P + n) and (a[:, :P] == prompt).all()
    assert torch.equal(a, b)


@pytest.mark.parametrize("use_graph", [False, True])
def test_fp8_row_groups_give_the_same_tokens(use_graph):
    mt, _ = tame_model(L=160)
    g = torch.Generator().manual_seed(8)
    x = torch.randint(0, 336, (7, 20), generator=g).cuda()
    ref = mt.generate_cached(x, 100, top_p=0.95, seed=77, use_graph=use_graph, kv_cache="fp8")
    for G in (2, 3):
        got = mt.generate_cached(x, 100, top_p=0.95, seed=77, use_graph=use_graph, groups=G, kv_cache="fp8")
        torch.cuda.synchronize()
        assert torch.equal(got, ref), G
    assert len(set(ref[:, 90].tolist())) > 1


def test_fp8_grammar_is_respected():
    from musicgeneration_amd.REMI import REMI_EventSeq
    from musicgeneration_amd.network import MusicTransformer
    torch.manual_seed(0)
    Vr = REMI_EventSeq.dim() + 1
    mt = MusicTransformer(embedding_dim=128, vocab_size=Vr, num_layer=2, max_seq=128, dropout=0.0).cuda().eval()
    tab = REMI_EventSeq.next_token_table()
    bar = REMI_EventSeq.feat_ranges()['bar'][0]
    out = mt.generate_cached(torch.full((4, 1), bar, device=DEV), 100, top_p=0.95, seed=1, grammar=tab, kv_cache="fp8").cpu().numpy()
    for row in out:
        for a, b in zip(row, row[1:]):
            assert (tab[a, b >> 5] >> np.uint32(b & 31)) & np.uint32(1), (a, b)


@pytest.mark.parametrize("prefill", ["batched", "auto"])
def test_fp8_equal_prior_lengths_are_bitwise_the_uniform_call(prefill):
    mt, _ = tame_model(L=128)
    V, B, P, n = 337, 3, 40, 30
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, V - 1, (B, P), generator=g).cuda()
    kw = dict(top_p=0.9, seed=5, prefill=prefill, return_cache=True, kv_cache="fp8")
    a = mt.generate_cached(x, n, **kw)
    b = mt.generate_cached(x, n, prior_lengths=[P] * B, **kw)
    assert torch.equal(a[0], b[0])
    for la, lb in zip(a[1:], b[1:]):
        assert all(torch.equal(u.view(torch.uint8) if u.dtype == torch.float8_e4m3fn else u,
                               w.view(torch.uint8) if w.dtype == torch.float8_e4m3fn else w) for u, w in zip(la, lb))
    # below the width of prior: padded to Pmax + length, codes and scales with zeros
    wide = torch.cat([x, torch.full((B, 6), 11, device=x.device)], 1)
    c = mt.generate_cached(wide, n, prior_lengths=[P] * B, **kw)
    assert c[0].shape == (B, P + 6 + n) and torch.equal(c[0][:, :P + n], a[0]) and (c[0][:, P + n:] == mt.pad_token).all()
    for la, lc in zip(a[1:], c[1:]):
        for u, w in zip(la, lc):
            assert w.dtype == u.dtype and w.shape[2] == P + 6 + n
            u8 = (lambda t: t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t)
            assert torch.equal(u8(w)[:, :, :P + n], u8(u)) and not u8(w)[:, :, P + n:].any()


def test_fp8_return_cache_shapes_and_ragged_prompts():
    mt, _ = tame_model(L=160)
    V, n = 337, 40
    lens = [3, 1, 40, 17]
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, V - 1, (4, 40), generator=g).cuda()
    B, h, total = 4, 2, 40 + n
    toks, kc, vc, ks, vs = mt.generate_cached(x, n, top_p=0.95, seed=7, return_cache=True, kv_cache="fp8", prior_lengths=lens)
    assert toks.shape == (B, total) and toks.dtype == torch.int32
    assert len(kc) == len(vc) == len(ks) == len(vs) == 2
    for c in kc + vc:
        assert c.dtype == torch.float8_e4m3fn and c.shape == (B, h, total, 64)
    for s in ks + vs:
        assert s.dtype == torch.float32 and s.shape == (B, h, total)
    for b, P in enumerate(lens):                                     # the rows a row's decode never reached are zero
        assert not ks[0][b, :, P + n - 1:].any() and (ks[0][b, :, :P + n - 1] > 0).all(), b
        assert not kc[0][b, :, P + n - 1:].view(torch.uint8).any(), b
        assert (toks[b, P + n:] == mt.pad_token).all() and int(toks[b, P:P + n].max()) < V
    # graph replay = eager on the ragged path too
    eager = mt.generate_cached(x, n, top_p=0.95, seed=7, use_graph=False, kv_cache="fp8", prior_lengths=lens)
    assert torch.equal(eager, toks)
    # return_probs over ragged prompts with the 8-bit cache: distributions, summing to 1 at each row's sampled positions
    t2, pr = mt.generate_cached(x, n, top_p=0.95, seed=7, return_probs=True, kv_cache="fp8", prior_lengths=lens)
    assert torch.equal(t2, toks)
    for b, P in enumerate(lens):
        assert abs(pr[b, P - 1:P + n - 1].sum(-1) - 1).max().item() < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# 6. the default is unchanged
# ---------------------------------------------------------------------------------------------------------------------
def test_kv_cache_bf16_is_bitwise_the_call_without_the_keyword():
    mt, _ = tame_model(L=128)
    g = torch.Generator().manual_seed(13)
    x = torch.randint(0, 336, (3, 33), generator=g).cuda()
    (ta, pa), ka, va = mt.generate_cached(x, 40, top_p=0.9, seed=2, return_probs=True, return_cache=True)
    (tb, pb), kb, vb = mt.generate_cached(x, 40, top_p=0.9, seed=2, return_probs=True, return_cache=True, kv_cache="bf16")
    assert torch.equal(ta, tb) and torch.equal(pa, pb)
    assert all(a.dtype == BF and torch.equal(a, b) for a, b in zip(ka + va, kb + vb))
    a = mt.generate_cached(x, 60, top_p=0.9, seed=2, prefill="batched")
    b = mt.generate_cached(x, 60, top_p=0.9, seed=2, prefill="batched", kv_cache="bf16")
    assert torch.equal(a, b)
