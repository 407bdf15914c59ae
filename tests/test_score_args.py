"""Scoring, the host side: the window schedule of sequences longer than the model's window, every refusal of
MusicTransformer.score and of generate.py's --best-of (they run before any device work, so no GPU is needed), and the tests' own
reference (tests/score_ref.py) against torch.log_softmax in fp64."""
import numpy as np
import pytest
import torch

import score_ref
from decode_fixtures import host_model

WINDOWS = (2, 3, 5, 32, 33)


@pytest.mark.parametrize("W", WINDOWS)
def test_schedule_scores_every_position_once_with_enough_context(W):
    from musicgeneration_amd.scoring import score_schedule
    for stride in range(1, W):
        for n in range(2, 121):
            sched = score_schedule(n, W, stride)
            seen = np.zeros(n, int)
            for k, (start, width, first) in enumerate(sched):
                assert 0 <= start and start + width <= n and 1 <= width <= W and 1 <= first <= width
                assert width == min(n, W)
                if n > W:
                    assert start == min(k * stride, n - W)
                seen[start + first:start + width] += 1
                if k > 0:                                      # outside window 0: at least W - stride tokens of context
                    assert first >= W - stride, (n, W, stride, k)
                else:
                    assert (start, first) == (0, 1)
            assert seen[0] == 0 and (seen[1:] == 1).all(), (n, W, stride)
            assert sched[-1][0] == max(0, n - W)
            if n <= W:
                assert sched == [(0, n, 1)]


def test_schedule_default_stride_and_refusals():
    from musicgeneration_amd.scoring import score_schedule
    assert score_schedule(100, 32) == score_schedule(100, 32, 16)
    assert score_schedule(10, 2) == score_schedule(10, 2, 1)
    for n, W, stride in ((10, 4, 4), (10, 4, 5), (10, 4, 0), (10, 4, -1), (10, 1, None), (10, 0, None)):
        with pytest.raises(ValueError):
            score_schedule(n, W, stride)


@pytest.mark.parametrize("temperature", (1.0, 0.7))
def test_reference_agrees_with_log_softmax(temperature):
    rng = np.random.default_rng(3)
    rows, V = 40, 37
    logits = torch.from_numpy(rng.normal(size=(rows, V)) * 5).to(torch.bfloat16).to(torch.float64).numpy()
    target = rng.integers(0, V, rows)
    ref = score_ref.token_logprob(logits, target, temperature)
    want = score_ref.log_softmax_torch(logits, temperature, np.ones((rows, V), bool))
    r = np.arange(rows)
    assert np.abs(ref["logp"] - want[r, target]).max() < 1e-12
    assert (ref["hit"] == (logits.argmax(1) == target)).all()
    # with a grammar: a random table, one row of it empty (ignored)
    table = rng.integers(0, 2 ** 32, (V, 2), dtype=np.uint64).astype(np.uint32)
    table[5] = 0
    prev = rng.integers(0, V, rows)
    prev[:3] = 5
    ok = score_ref.allowed_rows(table, prev, logits)
    assert ok[:3].all() and not ok[3:].all()
    ref = score_ref.token_logprob(logits, target, temperature, table, prev)
    want = score_ref.log_softmax_torch(logits, temperature, ok)
    fin = ok[r, target]
    assert np.abs(ref["logp"][fin] - want[r, target][fin]).max() < 1e-12
    assert (ref["logp"][~fin] == -np.inf).all() and (~fin).any()
    masked = np.where(ok, logits, -np.inf)
    assert (ref["hit"] == ((masked.argmax(1) == target) & fin)).all()
    # the fp32 twin is close, and unscored rows are 0 / -1
    tw = score_ref.token_logprob(logits, target, temperature, table, prev, np.float32, True)
    assert np.abs(tw["logp"][fin] - ref["logp"][fin]).max() < 1e-4
    un = score_ref.token_logprob(logits, np.array([-1, V] * (rows // 2)), temperature)
    assert (un["logp"] == 0).all() and (un["hit"] == -1).all() and np.isfinite(un["lse"]).all()


def test_reference_ties_and_non_finite_rows():
    x = np.array([[1.0, 3.0, 3.0, -2.0], [-1.0, -0.0, 0.0, -5.0], [0.0, np.nan, 1.0, 1.0], [0.0, np.inf, 0.0, 0.0],
                  [-np.inf] * 4])
    assert score_ref.token_logprob(x, [1, 1, 2, 0, 0])["hit"].tolist() == [1, 1, 1, 0, 1]
    assert score_ref.token_logprob(x, [2, 2, 3, 1, 1])["hit"].tolist() == [0, 0, 0, 1, 0]
    ref = score_ref.token_logprob(x, [1, 1, 2, 0, 0])
    assert np.isfinite(ref["logp"][:2]).all() and np.isnan(ref["logp"][2:]).all() and np.isnan(ref["lse"][2:]).all()
    lin = score_ref.linear_logprob(np.eye(4)[:2], x[:1].T @ np.ones((1, 4)), None, [1, 2])
    assert lin["hit"].tolist() == [1, 0] and lin["gap"].tolist() == [0.0, 0.0]
    s, c, h, m = score_ref.score_reduce(np.array([[1.0, -2.0, 5.0], [0.5, -np.inf, 0.0]]), np.array([[1, 0, -1], [0, 1, -1]]))
    assert s.tolist() == [-1.0, -np.inf] and c.tolist() == [2, 2] and h.tolist() == [1, 1] and m[0] == 3.0


@pytest.mark.parametrize("kw,msg", [
    (dict(grammar=np.zeros((40, 2), np.uint32), logits="fp32"), "grammar"),
    (dict(logits="fp16"), "logits"),
    (dict(window=1), "window"),
    (dict(window=65), "window"),
    (dict(window=32, stride=32), "stride"),
    (dict(window=32, stride=0), "stride"),
    (dict(stride=64), "stride"),
    (dict(temperature=0.0), "temperature"),
    (dict(lengths=[3, 4]), "3 rows"),
    (dict(lengths=[3, 4, 51]), "0 .. 50"),
    (dict(from_pos=[1, 2]), "3 rows"),
    (dict(from_pos=-1), "from_pos"),
])
def test_score_refusals_need_no_device(kw, msg):
    x = torch.randint(0, 39, (3, 50))                          # a CPU tensor: a refusal that came later would be MgxError
    with pytest.raises(ValueError, match=msg):
        host_model(L=64, V=40, d=64).score(x, **kw)
    from musicgeneration_amd import scoring
    kw = dict(kw)
    with pytest.raises(ValueError, match=msg):
        scoring.check_args(64, 64, 3, 50, **kw)


def test_check_args_resolves_the_logit_path_and_restores_the_mode():
    from musicgeneration_amd import scoring
    assert scoring.check_args(64, 64, 2, 50)[:3] == ("fp32", 64, 32)
    assert scoring.check_args(64, 64, 2, 50, grammar=np.zeros((40, 2), np.uint32))[0] == "bf16"
    assert scoring.check_args(64, 1088, 2, 50)[0] == "bf16"
    with pytest.raises(ValueError, match="1024"):
        scoring.check_args(64, 1088, 2, 50, logits="fp32")
    assert scoring.check_args(64, 64, 2, 50, window=33, from_pos=4, lengths=[50, 0])[1:] == (33, 16, [50, 0], [4, 4])
    mt = host_model(L=64, V=40, d=64)
    mt.train()
    with pytest.raises(ValueError):
        mt.score(torch.zeros(1, 4, dtype=torch.long), window=1)
    assert mt.training                                         # the mode is restored after a refusal too


def test_plan_windows_covers_a_ragged_batch():
    from musicgeneration_amd.scoring import plan_windows
    ns, L, W, stride = [33, 70, 100, 5, 1, 0], 100, 32, 16
    wins, src = plan_windows(ns, L, W, stride)
    assert [w[2] for w in wins] == sorted((w[2] for w in wins), reverse=True)          # batched by width
    for b, n in enumerate(ns):
        for i in range(L):
            k, j = src[b][i]
            if 1 <= i < n:
                rb, start, width, first = wins[k]
                assert rb == b and start + j == i and first <= j < width
            else:
                assert k == -1


def test_best_of_cli_refusals(tmp_path):
    from musicgeneration_amd import generate
    base = ["-o", str(tmp_path / "out"), "-d", ""]
    with pytest.raises(SystemExit, match="--best-of must be at least 1"):
        generate.main(base + ["--best-of", "0"])
    with pytest.raises(SystemExit, match="--best-of cannot be combined with -B"):
        generate.main(base + ["--best-of", "2", "-B", "2"])
    assert generate.get_options([]).best_of == 1
    generate._check_best_of(generate.get_options(["--best-of", "3"]))                  # accepted
    from musicgeneration_amd import score
    with pytest.raises(SystemExit, match="stride"):
        score.main(["-d", str(tmp_path), "-M", "64", "--window", "32", "--stride", "32"])
    with pytest.raises(SystemExit, match="window"):
        score.main(["-d", str(tmp_path), "-M", "64", "--window", "65"])


def test_score_module_entry_point_refuses_before_device_work(tmp_path):
    """python -m musicgeneration_amd.score, as a child process: the window check ends it before any model or device work"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "musicgeneration_amd.score", "-d", str(tmp_path), "-M", "64", "--window", "65"],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "window must lie in 2 .. max_seq (64)" in r.stderr
