"""The host side of FusedAdam's weight decay, lr_scale and EMA: every refusal, the chunk table of mgx_adam_step_groups, the default
no-decay set, the EMA warm-up schedule, the header's entry, and the --ema refusals of generate.py / score.py.  No GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    from musicgeneration_amd.network import MusicTransformer
    torch.manual_seed(0)
    return MusicTransformer(embedding_dim=64, vocab_size=90, num_layer=2, max_seq=32, dropout=0.0)


def test_weight_decay_and_ema_decay_refusals():
    from musicgeneration_amd.optim import check_ema_decay, check_weight_decay
    assert check_weight_decay(0) == 0.0 and check_weight_decay(0.01) == 0.01
    for bad in (-1e-9, -1, float("nan"), float("inf"), "0.1", None, True, [0.1]):
        with pytest.raises(ValueError, match="weight_decay"):
            check_weight_decay(bad)
    assert check_ema_decay(None) is None and check_ema_decay(0.999) == 0.999
    for bad in (0, 0.0, 1, 1.0, -0.1, 1.5, float("nan"), float("inf"), "0.9", False):
        with pytest.raises(ValueError, match="ema_decay"):
            check_ema_decay(bad)


def test_fused_adam_refuses_bad_arguments_before_any_device_work():
    from musicgeneration_amd.optim import FusedAdam
    mt = _model()                                                 # on the CPU: reaching model.store() would raise MgxError instead
    for kw in (dict(weight_decay=-1.0), dict(ema_decay=1.0), dict(lr_scale={"nothing.here": 0.5}), dict(lr_scale={"fc": -1.0}),
               dict(lr_scale=[("fc", 1.0)]), dict(no_decay="all")):
        with pytest.raises(ValueError):
            FusedAdam(mt, **kw)


def test_lr_scale_prefixes_longest_wins_and_a_prefix_without_a_match_lists_the_names():
    from musicgeneration_amd.optim import resolve_lr_scale
    names = [n for n, _ in _model().named_parameters()]
    got = resolve_lr_scale({"Decoder": 0.5, "Decoder.enc_layers.1": 0.0, "Decoder.enc_layers.1.rga.E": 2}, names)
    assert set(got) == set(names)
    assert got["Decoder.embedding.weight"] == 0.5 and got["Decoder.enc_layers.0.rga.E"] == 0.5
    assert got["Decoder.enc_layers.1.FFN_pre.weight"] == 0.0 and got["Decoder.enc_layers.1.rga.E"] == 2.0
    assert got["fc.weight"] == 1.0 and got["fc.bias"] == 1.0
    assert set(resolve_lr_scale(None, names).values()) == {1.0}
    with pytest.raises(ValueError) as e:
        resolve_lr_scale({"Decoder.enc_layers.7": 0.0}, names)
    assert "Decoder.enc_layers.7" in str(e.value) and all(n in str(e.value) for n in names)
    for bad in (-0.5, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="lr_scale"):
            resolve_lr_scale({"fc": bad}, names)


def test_groups_are_the_distinct_pairs_and_more_than_256_are_refused():
    from musicgeneration_amd.optim import MAX_GROUPS, build_groups
    named = list(_model().named_parameters())
    group_of, pairs, exempt = build_groups(named, 0.1, None, {"Decoder.embedding": 0, "Decoder.enc_layers.1": 0.25})
    assert pairs == [(0.0, 0.0), (1.0, 0.0), (1.0, 0.1), (0.25, 0.0), (0.25, 0.1)]
    assert group_of["Decoder.embedding.weight"] == 0 and group_of["Decoder.enc_layers.0.rga.E"] == 1
    assert group_of["Decoder.enc_layers.0.rga.Wq.weight"] == 2 and group_of["Decoder.enc_layers.1.rga.Wq.bias"] == 3
    assert group_of["Decoder.enc_layers.1.FFN_suf.weight"] == 4 and group_of["fc.weight"] == 2 and group_of["fc.bias"] == 1
    assert build_groups(named)[1] == [(1.0, 0.0)]
    # a predicate of the caller's replaces the default
    only_fc = build_groups(named, 0.1, lambda n, p: not n.startswith("fc."))
    assert only_fc[1] == [(1.0, 0.0), (1.0, 0.1)] and [n for n, k in only_fc[0].items() if k == 1] == ["fc.weight", "fc.bias"]
    many = [(f"w{i}.weight", torch.nn.Parameter(torch.zeros(2, 2))) for i in range(MAX_GROUPS + 1)]
    ok = build_groups(many[:MAX_GROUPS], 0.0, None, {f"w{i}.": 1.0 + i for i in range(MAX_GROUPS)})
    assert len(ok[1]) == MAX_GROUPS == 256
    with pytest.raises(ValueError, match="257.*256"):
        build_groups(many, 0.0, None, {f"w{i}.": 1.0 + i for i in range(MAX_GROUPS + 1)})


def test_default_no_decay_leaves_the_projection_matrices_only():
    from musicgeneration_amd.optim import default_no_decay
    decayed = [n for n, p in _model().named_parameters() if not default_no_decay(n, p)]
    want = [f"Decoder.enc_layers.{i}.{m}.weight" for i in range(2)
            for m in ("rga.Wq", "rga.Wk", "rga.Wv", "rga.fc", "FFN_pre", "FFN_suf")] + ["fc.weight"]
    assert decayed == want


def test_chunk_table_on_a_hand_made_layout():
    from musicgeneration_amd.ops import adam_group_chunks
    # short: 10 elements in one chunk; padded: 100 elements with 28 of padding, then 64 more reserved (a padded vocabulary);
    # two neighbours of different groups; the last parameter ends inside its chunk, the buffer two chunks later
    offsets = {"short": (0, 10), "padded": (64, 100), "a": (256, 64), "b": (320, 130)}
    names = ["short", "padded", "a", "b"]
    groups = {"short": 3, "padded": 1, "a": 0, "b": 2}
    assert adam_group_chunks(offsets, names, groups) == [3, 1, 1, 1, 0, 2, 2, 2]
    assert adam_group_chunks(offsets, names, groups, 640) == [3, 1, 1, 1, 0, 2, 2, 2, 2, 2]
    assert len(adam_group_chunks(offsets, names, groups, 450 + 1)) == (451 + 63) // 64
    with pytest.raises(ValueError, match="multiple of 64"):
        adam_group_chunks({"a": (0, 10), "b": (32, 10)}, ["a", "b"], {"a": 0, "b": 0})
    with pytest.raises(ValueError, match="overlaps"):
        adam_group_chunks({"a": (0, 100), "b": (64, 10)}, ["a", "b"], {"a": 0, "b": 0})
    for bad in (256, -1, 1.0, None):
        with pytest.raises(ValueError, match="group of a"):
            adam_group_chunks({"a": (0, 10)}, ["a"], {"a": bad})
    # with the longest-prefix rule in front of it
    from musicgeneration_amd.optim import resolve_lr_scale
    scale = resolve_lr_scale({"p": 0.0, "padded": 1.0}, ["padded", "plain"])
    assert scale == {"padded": 1.0, "plain": 0.0}


def test_ema_warm_up_schedule():
    from musicgeneration_amd.optim import ema_warmup
    assert ema_warmup(0.999, 0) == 0.1 and ema_warmup(0.999, 1) == 2.0 / 11.0
    assert ema_warmup(0.999, 10 ** 6) == 0.999 and ema_warmup(0.5, 8) == 0.5 and ema_warmup(0.5, 7) == 8.0 / 17.0
    assert all(ema_warmup(0.999, u) <= ema_warmup(0.999, u + 1) for u in range(20000))


def test_train_cli_flags_and_refusals(monkeypatch):
    from musicgeneration_amd import train
    opts = (lambda *argv: train.get_options(list(argv)))
    assert train.optim_args(opts()) == {}
    assert train.optim_args(opts("--weight-decay", "0")) == {}
    assert train.optim_args(opts("--weight-decay", "0.01", "--freeze", "Decoder.embedding,Decoder.enc_layers.0", "--lr-scale",
                                 "Decoder.enc_layers.1=0.5,fc=2", "--ema-decay", "0.999")) == {
        "weight_decay": 0.01, "ema_decay": 0.999,
        "lr_scale": {"Decoder.embedding": 0.0, "Decoder.enc_layers.0": 0.0, "Decoder.enc_layers.1": 0.5, "fc": 2.0}}
    for argv, flag in ((["--weight-decay", "-0.1"], "--weight-decay"), (["--weight-decay", "nan"], "--weight-decay"),
                       (["--ema-decay", "1"], "--ema-decay"), (["--ema-decay", "0"], "--ema-decay"),
                       (["--ema-decay", "-0.5"], "--ema-decay"), (["--lr-scale", "fc"], "--lr-scale"),
                       (["--lr-scale", "fc=x"], "--lr-scale"), (["--lr-scale", "fc=-1"], "--lr-scale"),
                       (["--lr-scale", "=1"], "--lr-scale"), (["--lr-scale", "fc=1,,"], "--lr-scale"),
                       (["--freeze", ""], "--freeze"), (["--freeze", "fc,"], "--freeze"),
                       (["--freeze", "fc", "--lr-scale", "fc=0.5"], "--freeze")):
        with pytest.raises(ValueError, match=flag):
            train.optim_args(opts(*argv))

        def built(*a, **k):
            raise AssertionError("a model was built")
        monkeypatch.setattr(train, "MusicTransformer", built)
        with pytest.raises((ValueError, SystemExit), match=flag):     # main refuses before the model (and the device) is touched
            train.main(argv)


def test_header_carries_the_abi_and_the_entry_point():
    from musicgeneration_amd import _lib
    assert _lib.EXPECTED_ABI >= 35
    restype, argtypes = _lib.FUNCTIONS["mgx_adam_step_groups"]
    assert len(argtypes) == 20
    text = open(os.path.join(ROOT, "include", "mgx.h")).read()
    assert re.search(r"int\s+mgx_adam_step_groups\s*\(float\*\s*p,", text) and "35:" in text


@pytest.mark.parametrize("tool", ("generate", "score"))
def test_ema_flag_on_a_checkpoint_without_net_ema_exits_naming_both(tool, tmp_path, monkeypatch):
    import importlib
    mod = importlib.import_module("musicgeneration_amd." + tool)

    def built(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(mod, "MusicTransformer", built)
    ck = str(tmp_path / "old.pth")
    torch.save({"net": {}, "optimizer": {}, "epoch": 0}, ck)
    argv = ["-s", ck, "-d", str(tmp_path), "--ema"] + (["-o", str(tmp_path / "out")] if tool == "generate" else ["-M", "64"])
    with pytest.raises(SystemExit) as e:
        mod.main(argv)
    assert "--ema" in str(e.value) and "net_ema" in str(e.value) and ck in str(e.value)
    with pytest.raises(SystemExit, match="--ema.*-s"):
        mod.main([a for a in argv if a not in ("-s", ck)])
    from musicgeneration_amd.utils import load_net
    torch.save({"net": {"a": 1}, "net_ema": {"a": 2}}, ck)
    assert load_net(ck) == {"a": 1} and load_net(ck, ema=True) == {"a": 2} and load_net(None) is None
