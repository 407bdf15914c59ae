"""bench.py's own surface: --dump-outputs (what the last timed step computed, reproducible run to run) and the split between a
lean plain run and --full."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"loss", "accuracy", "argmax", "logits_sample", "param_sample", "adam_exp_avg_sample", "adam_exp_avg_sq_sample"}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_outputs_samples_large_tensors_and_writes_small_ones_whole(tmp_path):
    """Every value of the stand-in tensors is its own flat index, so a sample shows where it was taken from: the logits
    sample must come from the [B, L, V] view of a column-padded buffer (never from a pad column), the weights and both Adam
    moments must be sampled at the same indices, and a second call must write the same files."""
    import bench
    B, L, V, Vp = 4, 1024, 600, 608                          # B*L*V = 2.46 M > 2 * DUMP_SAMPLE: sampled
    buf = torch.full((B, L, Vp), -1.0)
    buf[:, :, :V] = torch.arange(B * L * V, dtype=torch.float32).reshape(B, L, V)
    logits = buf[:, :, :V]                                   # a strided view, as the model returns it
    n = 3_000_000
    idx = torch.arange(n, dtype=torch.float32)
    opt = types.SimpleNamespace(store=types.SimpleNamespace(param=idx), m=2 * idx, v=3 * idx)
    bucket = torch.randint(0, V, (B * L,), dtype=torch.int32, generator=torch.Generator().manual_seed(0))
    m = {"loss": torch.tensor(5.9), "accuracy": torch.tensor(0.25), "bucket": bucket}
    bench.dump_outputs(str(tmp_path / "a"), m, logits, opt)
    bench.dump_outputs(str(tmp_path / "b"), m, logits, opt)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == NAMES and all(x.dtype == np.float32 for x in a.values())
    assert all(a[k].tobytes() == b[k].tobytes() for k in NAMES)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["loss"].shape == (1,) and a["loss"][0] == np.float32(5.9) and a["accuracy"][0] == 0.25
    assert np.array_equal(a["argmax"], bucket.numpy().astype(np.float32))          # 4096 rows: written whole
    ls = a["logits_sample"]
    assert ls.size == bench.DUMP_SAMPLE and ls.min() >= 0 and ls.max() < B * L * V and np.array_equal(ls, np.floor(ls))
    assert ls.min() < 0.01 * B * L * V and ls.max() > 0.99 * B * L * V                # spread over the whole tensor
    ps = a["param_sample"]
    assert ps.size == bench.DUMP_SAMPLE and ps.min() >= 0 and ps.max() < n
    assert np.array_equal(a["adam_exp_avg_sample"], 2 * ps) and np.array_equal(a["adam_exp_avg_sq_sample"], 3 * ps)


SMALL = ["--batch", "2", "--seq-len", "256", "--layers", "2", "--d-model", "128", "--steps", "3", "--warmup", "1"]


def _bench(*extra, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SMALL, *extra],
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_bit_for_bit(tmp_path):
    """--dump-outputs implies deterministic-reduction mode: two runs with the same arguments write identical float32 files"""
    one = _bench("--dump-outputs", str(tmp_path / "one"))
    two = _bench("--dump-outputs", str(tmp_path / "two"))
    assert one["config"]["deterministic"] and two["config"]["deterministic"] and one["steps"] == 3
    a, b = _load(tmp_path / "one"), _load(tmp_path / "two")
    assert set(a) == set(b) == NAMES
    for k in NAMES:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        assert a[k].tobytes() == b[k].tobytes(), k
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert a["logits_sample"].size == 2 * 256 * 337 and a["argmax"].size == 2 * 256      # small shape: written whole
    assert a["loss"][0] == np.float32(one["config"]["final_loss"])


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_full_adds_the_rest():
    plain = _bench()
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(plain)
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert not plain["config"]["deterministic"]                  # a plain run times the product's default step
    assert not {"roofline", "kernel_ms", "decode", "cpu_baseline", "cfg4", "batch8"} & set(plain)
    full = _bench("--full", "--no-cfg4", "--decode-len", "512", "--decode-batch", "4", "--cpu-seconds", "1", timeout=900)
    assert {"roofline", "kernel_ms", "attention_kernels", "decode", "cpu_baseline", "gpu_over_cpu"} <= set(full)
    assert not full["config"]["deterministic"]
