"""The reference's layer-level call surface on the kernels: ``rga([q,k,v], mask)`` (layers.py:64-109),
``EncoderLayer(x, mask)`` (:152-161), ``Encoder(x, mask)`` (:223-233).
G1c / G1d are outputs of the reference's own RelativeGlobalAttention at the kernels' head width (dh = 64), for
L == M and L < M (tests/golden/gen_golden.py mt2).  Tolerances (bf16 operands, fp32 accumulation, against an fp32
reference): output rel-L2 <= 2e-2, attention weights |err| <= 1.5e-2, gradient cosine >= 0.99."""
import os

import numpy as np
import pytest
import torch

from kernel_checks import cos as _cos, rel as _rel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tag", ["c", "d"])
def test_g1_rga_forward_matches_reference(golden_dir, tag):
    from musicgeneration_amd.layers import RelativeGlobalAttention
    g = dict(np.load(os.path.join(golden_dir, f"g1{tag}_rga_dh64.npz")))
    B, h, L, M = (int(v) for v in g["shape"])
    rga = RelativeGlobalAttention(h=h, d=64 * h, max_seq=M)
    rga.load_state_dict({k[2:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("p.")}, strict=True)
    rga = rga.cuda()
    x = torch.from_numpy(g["x"]).cuda().requires_grad_(True)
    mask = torch.from_numpy(g["mask"]).cuda()
    out, w = rga([x, x, x], mask)
    assert out.dtype == x.dtype and out.shape == (B, L, 64 * h) and w.shape == (B, h, L, L)
    assert _rel(out, torch.from_numpy(g["out"])) <= 2e-2
    assert (w.cpu() - torch.from_numpy(g["weights"])).abs().max().item() <= 1.5e-2
    (out * torch.from_numpy(g["wsum"]).cuda()).sum().backward()
    assert _cos(x.grad, torch.from_numpy(g["gx"])) >= 0.99
    assert _cos(rga.E.grad, torch.from_numpy(g["gE"])) >= 0.99
    assert _cos(rga.Wq.weight.grad, torch.from_numpy(g["gWq"])) >= 0.99
    assert _cos(rga.fc.bias.grad, torch.from_numpy(g["gfcb"])) >= 0.999
    # rows of E above the L rows in use receive no gradient (layers.py:111-114)
    assert rga.E.grad[: M - L].abs().max().item() == 0.0 if M > L else True
    # separate q / k / v tensors take the three-projection route and give the same result
    out2, _ = rga([x.detach(), x.detach().clone(), x.detach().clone()], mask)
    assert _rel(out2, out.detach()) <= 1e-2


def test_layer_forward_mask_contract():
    from musicgeneration_amd.layers import RelativeGlobalAttention
    rga = RelativeGlobalAttention(h=2, d=128, max_seq=32).cuda()
    x = torch.randn(1, 32, 128, device="cuda")
    with pytest.raises(NotImplementedError, match="bidirectional"):          # mask=None is an inference path: no backward
        rga([x, x, x], None)
    with torch.no_grad():                                                      # ... the reference's sampling call (layers.py:86-106)
        out, w = rga([x, x, x], None)
    from oracle import ref_cpu as R
    p = {"rga." + k: v.detach().float().cpu() for k, v in rga.state_dict().items()}
    ref, _ = R.rga_forward(p, "rga.", x.float().cpu(), None, 2)
    assert w is None and (out.float().cpu() - ref).abs().max().item() <= 3e-2 * ref.abs().max().item()
    full = torch.zeros(1, 1, 32, 32, dtype=torch.bool, device="cuda")          # nothing masked = not causal
    with pytest.raises(ValueError, match="look-ahead"):
        rga([x, x, x], full)
    with pytest.raises(ValueError):
        rga([x[:, :20], x[:, :20], x[:, :20]], full[..., :20, :20])            # not the look-ahead mask either (any L is fine since round 6)


def test_encoder_and_layer_forward_match_oracle():
    """Encoder.forward(tokens, mask) and EncoderLayer.forward(x, mask) stand-alone (ordinary autograd), against the
    oracle's restatement of layers.py:152-161,223-233 (pinned by G2 in tests/test_oracle_golden.py)."""
    from musicgeneration_amd.layers import Encoder
    from musicgeneration_amd import utils
    from oracle import ref_cpu as R
    V, d, nl, L, B = 90, 128, 2, 64, 2
    pad = V - 1
    p = R.init_params(V, d, nl, L, seed=2)
    for k in p:
        if k.endswith("embedding.weight") or k.endswith("rga.E"):
            p[k] = p[k] * 0.3
    enc = Encoder(num_layers=nl, d_model=d, input_vocab_size=V, rate=0.0, max_len=L)
    enc.load_state_dict({k[len("Decoder."):]: v for k, v in p.items() if k.startswith("Decoder.")}, strict=True)
    enc = enc.cuda().train()
    g = torch.Generator().manual_seed(3)
    tok = torch.randint(0, V - 1, (B, L), generator=g)
    tok[1, -7:] = pad
    _, _, lam = utils.get_masked_with_pad_tensor(L, tok, tok, pad)
    hid, ws = enc(tok.cuda(), lam.cuda())
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    ref, wref = R.decoder_stack(pr, tok, R.look_ahead_mask(tok, pad))
    assert hid.dtype == torch.float32 and len(ws) == nl
    assert _rel(hid, ref.detach()) <= 2e-2
    assert (ws[1].cpu() - wref[1].detach()).abs().max().item() <= 2e-2
    wsum = torch.linspace(-1, 1, hid.numel()).reshape(hid.shape)
    (hid * wsum.cuda()).sum().backward()
    (ref * wsum).sum().backward()
    # (a) EVERY parameter against the oracle with bf16 rounding emulated at the points where the kernels store bf16: this is
    #     the bound that pins the kernels (measured >= 0.9999 on all of them; SURVEY 8c asks 0.999)
    R.EMULATE_BF16 = True
    try:
        pe = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        ref_e, _ = R.decoder_stack(pe, tok, R.look_ahead_mask(tok, pad))
        (ref_e * wsum).sum().backward()
    finally:
        R.EMULATE_BF16 = False
    for name, prm in enc.named_parameters():
        if name.endswith("Wk.bias"):      # exactly-zero true gradient (softmax shift invariance): noise on both sides
            continue
        assert _cos(prm.grad, pe["Decoder." + name].grad) >= 0.999, name
        # (b) against the fp32 oracle: what bf16 ACTIVATIONS cost on this synthetic objective (a linspace-weighted sum of the
        #     hidden states).  The floor is set by the attention-score gradients: dS = P (dP - delta) is a difference of two
        #     O(|dO||V|) terms rounded to bf16 before the dq / dk / dE products, so Wq / Wk / E sit at 0.980-0.987 here
        #     (measured, tools/tol_probe.py) while every other parameter is >= 0.995; halving the logit scale moves them
        #     to 0.982-0.99, i.e. it is rounding of the score gradient, not logit blow-up.
        #     The embedding is the other loose one (0.988): a row is the sum over the one or two positions that hold the token
        #     (B L = 128 positions, 89 tokens), so the rounding of dX there is not averaged out.
        floor = 0.975 if any(t in name for t in ("rga.Wq", "rga.Wk", "rga.E")) else (0.98 if name == "embedding.weight" else 0.99)
        assert _cos(prm.grad, pr["Decoder." + name].grad) >= floor, (name, _cos(prm.grad, pr["Decoder." + name].grad))
    # one layer on its own
    x = (torch.randn(B, L, d, generator=g) * 0.5)
    out, w = enc.enc_layers[0](x.cuda(), lam.cuda())
    o_ref, _ = R.encoder_layer({k: v.detach() for k, v in p.items()}, "Decoder.enc_layers.0.", x, R.look_ahead_mask(tok, pad),
                               d // 64, 0.0, False)
    assert _rel(out, o_ref) <= 2e-2


@pytest.mark.parametrize("d,max_len,L", [(192, 50, 50), (128, 96, 41), (320, 64, 64)])
def test_stand_alone_layers_take_any_length_and_any_64h_width(d, max_len, L):
    """the layer-level call surface (Encoder / EncoderLayer / RelativeGlobalAttention.forward) over the reference's whole range with
    heads of 64: any L <= max_seq (zero-padded to the kernels' 32-key tile inside rga.forward, the relative embedding with zero rows in
    front where the padding reaches past max_seq) and d_model = 64 h for odd h (FFN width d / 2 = 32 * odd, zero-padded per call in
    ops._LinearStd) -- hidden states, attention weights and every gradient against the oracle"""
    from musicgeneration_amd.layers import Encoder
    from musicgeneration_amd import utils
    from oracle import ref_cpu as R
    V, nl, B = 70, 2, 2
    pad = V - 1
    p = R.init_params(V, d, nl, max_len, seed=6)
    for k in p:
        if k.endswith("embedding.weight") or k.endswith("rga.E"):
            p[k] = p[k] * 0.3
    enc = Encoder(num_layers=nl, d_model=d, input_vocab_size=V, rate=0.0, max_len=max_len)
    enc.load_state_dict({k[len("Decoder."):]: v for k, v in p.items() if k.startswith("Decoder.")}, strict=True)
    enc = enc.cuda().train()
    g = torch.Generator().manual_seed(L)
    tok = torch.randint(0, V - 1, (B, L), generator=g)
    tok[1, -5:] = pad
    tok[0, 7] = pad                                                            # an interior pad
    _, _, lam = utils.get_masked_with_pad_tensor(L, tok, tok, pad)
    hid, ws = enc(tok.cuda(), lam.cuda())
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    ref, wref = R.decoder_stack(pr, tok, R.look_ahead_mask(tok, pad))
    assert tuple(hid.shape) == (B, L, d) and tuple(ws[0].shape) == (B, d // 64, L, L)
    assert _rel(hid, ref.detach()) <= 2e-2
    assert (ws[1].cpu() - wref[1].detach()).abs().max().item() <= 2e-2
    wsum = torch.linspace(-1, 1, hid.numel()).reshape(hid.shape)
    (hid * wsum.cuda()).sum().backward()
    R.EMULATE_BF16 = True
    try:
        pe = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        ref_e, _ = R.decoder_stack(pe, tok, R.look_ahead_mask(tok, pad))
        (ref_e * wsum).sum().backward()
    finally:
        R.EMULATE_BF16 = False
    for name, prm in enc.named_parameters():
        if name.endswith("Wk.bias"):
            continue
        assert prm.grad.shape == pe["Decoder." + name].grad.shape, name
        assert _cos(prm.grad, pe["Decoder." + name].grad) >= 0.999, (name, _cos(prm.grad, pe["Decoder." + name].grad))
    # the reference's sampling call (mask=None) at a length that is no multiple of 32
    with torch.no_grad():
        x = torch.randn(B, L, d, generator=g) * 0.5
        out, w = enc.enc_layers[0].rga([x.cuda()] * 3, None)
    pl = {"rga." + k: v.detach().float().cpu() for k, v in enc.enc_layers[0].rga.state_dict().items()}
    ref0, _ = R.rga_forward(pl, "rga.", x, None, d // 64)
    assert w is None and tuple(out.shape) == (B, L, d)
    assert (out.float().cpu() - ref0).abs().max().item() <= 3e-2 * ref0.abs().max().item()
