"""Host-side checks of the 8-bit K/V cache option (generate_cached(kv_cache=...), generate.py --kv-cache) and of the torch
twin of its quantizer that the GPU tests compare the kernels with: no GPU needed."""
import pytest
import torch

from decode_fixtures import host_model


def quant_twin(x):
    """the cache's quantizer (include/mgx.h, ABI 20) in torch: x [..., 64] -> (codes uint8 [..., 64], scales f32 [...]).
    inv = 448 / amax is an IEEE f32 division (a tensor numerator: ``448.0 / t`` would be t.reciprocal() * 448, two roundings)."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    zero = amax == 0
    inv = torch.tensor(448.0, device=amax.device) / torch.where(zero, torch.ones_like(amax), amax)
    codes = (xf * inv[..., None]).to(torch.float8_e4m3fn).view(torch.uint8).clone()
    codes[zero] = 0
    return codes, amax / 448.0


def dequant_twin(codes, scale):
    return codes.view(torch.float8_e4m3fn).float() * scale[..., None]


@pytest.mark.parametrize("kv", ["fp16", "FP8", "", None, "e5m2"])
def test_a_bad_kv_cache_value_is_refused_before_device_work(kv):
    # a CPU model: any device work would raise MgxError instead
    with pytest.raises(ValueError, match="kv_cache"):
        host_model().generate_cached(torch.randint(0, 300, (2, 5)), 4, kv_cache=kv)
    with pytest.raises(ValueError, match="kv_cache"):
        host_model().generate_cached(torch.randint(0, 300, (2, 5)), 4, kv_cache=kv, prior_lengths=[5, 3])


def test_kv_cache_flag_parses_and_needs_a_cached_path(tmp_path):
    from musicgeneration_amd import generate
    base = ["-o", str(tmp_path / "out"), "-d", ""]
    assert generate.get_options(base).kv_cache == "bf16"
    assert generate.get_options(base + ["--kv-cache", "fp8"]).kv_cache == "fp8"
    with pytest.raises(SystemExit):
        generate.get_options(base + ["--kv-cache", "int8"])          # optparse refuses a value outside the choices
    with pytest.raises(SystemExit, match="--grammar or --condition-files"):
        generate.main(base + ["--kv-cache", "fp8"])
    with pytest.raises(SystemExit, match="--grammar or --condition-files"):
        generate.main(base + ["--kv-cache", "fp8", "--reference-mask"])


def test_rel_attn_decode_refuses_mismatched_8bit_caches():
    from musicgeneration_amd import ops
    B, h, L, d = 2, 2, 16, 128
    q, E, pos, ctx = torch.zeros(B, 3 * d, dtype=torch.bfloat16), torch.zeros(L, 64, dtype=torch.bfloat16), torch.zeros(1, dtype=torch.int32), \
        torch.zeros(B, d, dtype=torch.bfloat16)
    kc = torch.zeros(B, h, L, 64, dtype=torch.uint8)
    sc = torch.zeros(B, h, L)
    with pytest.raises(ValueError, match="kscale"):
        ops.rel_attn_decode(q, kc, kc.clone(), E, pos, ctx)                                  # no scales
    with pytest.raises(ValueError, match="kscale"):
        ops.rel_attn_decode(q, kc, kc.clone(), E, pos, ctx, kscale=sc, vscale=sc[:, :, :8])  # a short scale
    with pytest.raises(ValueError, match="kscale"):
        ops.rel_attn_decode(q, kc, kc.clone(), E, pos, ctx, kscale=sc, vscale=sc.double())
    with pytest.raises(ValueError, match="8-bit"):
        ops.rel_attn_decode(q, kc, torch.zeros(B, h, L, 64, dtype=torch.bfloat16), E, pos, ctx, kscale=sc, vscale=sc)
    with pytest.raises(ValueError, match="8-bit"):                                           # scales beside bf16 caches
        ops.rel_attn_decode(q, kc.bfloat16(), kc.bfloat16(), E, pos, ctx, kscale=sc, vscale=sc)
    with pytest.raises(ValueError, match="qkv"):
        ops.kv_store_fp8(torch.zeros(B, 4, 2 * d, dtype=torch.bfloat16), 4, kc, kc.clone(), sc, sc.clone())


def test_torch_twin_error_is_within_one_fp8_step():
    g = torch.Generator().manual_seed(0)
    rows = torch.randn(5, 64, generator=g)
    rows[0] = 0                                                        # all zero: scale 0, codes 0
    rows[1, 7] = 300.0                                                 # one outlier
    rows[2] = rows[2] * 1e-3
    rows[2, 0] = 5.0                                                   # the rest falls into subnormal codes (< 2^-6 of 448)
    rows[3] = -rows[3].abs()                                           # all negative
    rows[4] = rows[4].clamp(-1.9, 1.9)
    rows[4, 3] = -2.0                                                  # a power-of-two amax
    x = rows.to(torch.bfloat16)
    codes, scale = quant_twin(x)
    assert codes.dtype == torch.uint8 and scale.dtype == torch.float32
    assert not codes[0].any() and scale[0] == 0
    deq = dequant_twin(codes, scale)
    amax = x.float().abs().amax(-1, keepdim=True)
    assert ((x.float() - deq).abs() <= amax * 2 ** -4).all()
    # row 2 really holds subnormal codes (exponent field 0, mantissa not 0), and no code is NaN (0x7f / 0xff)
    c2 = codes[2] & 0x7F
    assert ((c2 >> 3) == 0).logical_and(c2 != 0).any()
    assert not ((codes & 0x7F) == 0x7F).any()
    # the largest element maps to +-448, i.e. back to itself up to the rounding of the scale
    assert torch.allclose(deq.abs().amax(-1), amax[:, 0], rtol=2 ** -22, atol=0)
