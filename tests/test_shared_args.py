"""Argument checks of N samples per prompt over a shared prompt cache (generate_cached(samples_per_prompt=N),
generate.py --share-prompt, ABI 26): they run on the host before any device work, so they are tested without a GPU."""
import re
import os

import pytest
import torch

from decode_fixtures import host_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kw,msg", [
    (dict(samples_per_prompt=0), "1 .. 16"),
    (dict(samples_per_prompt=17), "1 .. 16"),
    (dict(samples_per_prompt=4, window=64), "window"),
    (dict(samples_per_prompt=4, kv_cache="fp8"), "bf16"),
    (dict(samples_per_prompt=4, groups=2), "groups"),
    (dict(samples_per_prompt=4, masked_groups=True), "groups"),
    (dict(samples_per_prompt=4, prefill="token"), "prefill"),
    (dict(samples_per_prompt=4, prefill="bogus"), "prefill"),
    (dict(samples_per_prompt=4, return_cache=True), "return_cache"),
    (dict(samples_per_prompt=4, length=57), "max_seq"),                      # Pmax + length > max_seq
    (dict(samples_per_prompt=4, prior_lengths=[1, 5]), "2 entries"),
    (dict(samples_per_prompt=4, prior_lengths=[0, 5, 40]), "1 .. 40"),
    (dict(samples_per_prompt=4, kv_cache="int4"), "kv_cache"),
])
def test_samples_per_prompt_is_refused(kw, msg):
    x = torch.randint(0, 300, (3, 40))                                       # a CPU tensor: nothing reaches a device
    kw = dict(kw)
    with pytest.raises(ValueError, match=msg):
        host_model().generate_cached(x, kw.pop("length", 10), **kw)


def test_shared_prefill_that_pads_past_max_seq_is_refused():
    x = torch.randint(0, 300, (2, 90))                                       # 89 prefill rows pad to 96 > max_seq 92
    with pytest.raises(ValueError, match="max_seq=92"):
        host_model(L=92).generate_cached(x, 2, samples_per_prompt=2)


def test_check_args_keeps_its_positional_form():
    """the new keywords trail: the call as the existing callers make it returns what it did"""
    from musicgeneration_amd import decode
    x = torch.randint(0, 300, (3, 40))
    assert decode.check_args(host_model(), x, 10, False, "auto", [1, 5, 40], "bf16", None, None, None, False) == (40, [1, 5, 40], True, None)
    assert decode.check_args(host_model(), x, 10, False, "auto", None, "bf16") == (40, None, True, None)
    got = decode.check_args(host_model(), x, 10, False, "auto", None, "bf16", samples_per_prompt=3)
    assert got == (40, [40, 40, 40], True, None)
    got = decode.check_args(host_model(), x, 10, True, "batched", [1, 5, 40], "bf16", samples_per_prompt=16)
    assert got == (40, [1, 5, 40], True, None)


def _midi(path, n):
    from musicgeneration_amd import smf
    smf.write_notes(path, [(80, 60 + i % 12, 0.5 * i, 0.5 * i + 0.25) for i in range(n)])
    return path


def test_share_prompt_cli_refusals(tmp_path):
    from musicgeneration_amd import generate
    a, b = _midi(str(tmp_path / "a.mid"), 3), _midi(str(tmp_path / "b.mid"), 30)
    base = ["-o", str(tmp_path / "out"), "-d", "", "--share-prompt"]
    for extra, word in ((["--window", "64"], "--window"), (["--kv-cache", "fp8"], "--kv-cache fp8"), (["-B", "4"], "-B/--beam-size"),
                        (["--reference-mask"], "--reference-mask")):
        with pytest.raises(SystemExit, match="cannot be combined") as e:
            generate.main(base + ["-c", a, "-b", "4"] + extra)
        assert word in str(e.value)
    with pytest.raises(SystemExit, match="add -c FILE"):                     # neither a prompt file nor --grammar
        generate.main(base + ["-b", "4"])
    with pytest.raises(SystemExit, match="at most 16 samples per prompt, got 24"):
        generate.main(base + ["-c", a, "-b", "8", "--best-of", "3"])
    with pytest.raises(SystemExit, match="at most 16 samples per prompt, got 17"):
        generate.main(base + ["--condition-files", f"{a},{b}", "--best-of", "17"])
    with pytest.raises(SystemExit, match="at most 16 samples per prompt, got 32"):
        generate.main(base + ["--grammar", "--repr", "remi", "-b", "32"])
    assert generate.get_options([]).share_prompt is False                    # off by default


def test_header_constants_are_the_ones_ops_uses():
    from musicgeneration_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "mgx.h")).read()
    d = {n: int(v) for n, v in re.findall(r"^#define (MGX_\w+) (\d+)", hdr, re.M)}
    assert ops.SHARED_MAX_N == d["MGX_SHARED_MAX_N"] == 16
    assert ops.SHARED_NQ == d["MGX_SHARED_NQ"] and 1 <= ops.SHARED_NQ <= ops.SHARED_MAX_N
    assert d["MGX_ABI_VERSION"] >= 26 and _lib.EXPECTED_ABI == d["MGX_ABI_VERSION"]


def test_splits_and_workspace_are_host_functions_of_the_shapes():
    from musicgeneration_amd import _lib, ops
    lib = _lib.load()
    for shape in ((0, 4, 100, 10, 128), (2, 0, 100, 10, 128), (2, 4, 0, 10, 128), (2, 4, 100, 0, 128), (2, 4, 100, 10, 0),
                  (-1, 4, 100, 10, 128), (2, 4, -5, 10, 128)):
        assert lib.mgx_rel_attn_decode_shared_splits(*shape) == 0, shape
        assert lib.mgx_rel_attn_decode_shared_workspace(*shape) == 0, shape
    # one split below 1024 keys; doubled while a share holds 512 keys or more and the workgroups stay below 1024; 16 at most
    S = ops.rel_attn_decode_shared_splits
    assert [S(2, 4, lp, 100, 128) for lp in (100, 923, 924, 1947, 1948, 3995, 3996, 8091, 8092, 100000)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 16, 16]
    chunks = (16 + ops.SHARED_NQ - 1) // ops.SHARED_NQ
    assert S(1024, 1, 8092, 100, 64) == 1 and S(512, 1, 8092, 100, 64) == 2 and S(512 // chunks, 16, 8092, 100, 64) == 2
    for shape in ((2, 4, 100, 100, 128), (2, 4, 1000, 500, 128), (4, 8, 4096, 512, 512)):
        s = S(*shape)
        want = 0 if s == 1 else shape[0] * shape[1] * (shape[4] // 64) * s * 68 * 4
        assert lib.mgx_rel_attn_decode_shared_workspace(*shape) == want, shape
    # shape errors come back as status codes with a message, before any launch
    import ctypes
    one = ctypes.c_void_p(16)
    args = lambda *tail: (one,) * 9 + (None, 0) + tail + (None,)                                           # noqa: E731
    assert lib.mgx_rel_attn_decode_shared(*args(2, 17, 100, 10, 128, 200)) == -1 and b"1<=N<=16" in lib.mgx_last_error()
    assert lib.mgx_rel_attn_decode_shared(*args(2, 4, 0, 10, 128, 200)) == -1 and b"Lpre>=1" in lib.mgx_last_error()
    assert lib.mgx_rel_attn_decode_shared(*args(2, 4, 100, 10, 96, 200)) == -1 and b"d%64==0" in lib.mgx_last_error()
    assert lib.mgx_rel_attn_decode_shared(*args(2, 4, 1000, 500, 128, 2000)) == -1 and b"workspace" in lib.mgx_last_error()
    assert lib.mgx_rel_attn_decode_shared(*((None,) + args(2, 4, 100, 10, 128, 200)[1:])) == -2
