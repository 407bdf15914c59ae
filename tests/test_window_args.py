"""The re-anchored decode window (generate_cached(window=, hop=), generate.py --window / --hop) on the host: the schedule
decode.window_schedule plans, which the driver follows, and the refusals, which run before any device work."""
import pytest
import torch

from decode_fixtures import host_model


# lens, length, window, hop, the steps before which a re-anchor happens, the last step's base, the last step's t per row
# (None: not stated, the invariants below pin them)
CASES = [
    ([5], 100, 40, 16, [36, 52, 68, 84], 64, [39]),
    ([3], 10, 4, 2, [2, 4, 6, 8], 8, [3]),
    ([70], 60, 48, 12, [1, 13, 25, 37, 49], None, None),           # a prompt longer than the window
    ([9, 20, 30], 80, 48, 16, [19, 35, 51, 67], 64, [23, 34, 44]),
    ([5], 91, 96, 12, [], 0, None),                                # the window is never filled
]


@pytest.mark.parametrize("lens,length,W,hop,anchors,base_end,t_end", CASES)
def test_window_schedule(lens, length, W, hop, anchors, base_end, t_end):
    from musicgeneration_amd.decode import window_schedule
    bases, ts, got = window_schedule(lens, length, W, hop)
    assert got == anchors
    assert len(bases) == len(ts) == length
    for s in range(length):
        assert len(bases[s]) == len(ts[s]) == len(lens)
        for b, P in enumerate(lens):
            assert 0 <= ts[s][b] <= W - 1, (s, b)
            assert bases[s][b] + ts[s][b] == P - 1 + s, (s, b)      # the column of the step's input token
        prev_base = bases[s - 1] if s else [max(0, P - W) for P in lens]
        prev_t = [v + 1 for v in ts[s - 1]] if s else [min(P, W) - 1 for P in lens]
        moved = [a - b for a, b in zip(bases[s], prev_base)]
        if max(prev_t) == W:                                       # the longest row has filled the window: every row moves by hop
            assert s in got and moved == [hop] * len(lens), s
            assert ts[s] == [v - hop for v in prev_t], s
        else:
            assert s not in got and moved == [0] * len(lens), s
            assert ts[s] == prev_t, s
    if base_end is not None:
        assert bases[-1] == [base_end + max(0, P - W) for P in lens]
    if t_end is not None:
        assert ts[-1] == t_end


def test_window_schedule_default_hop_and_the_prompt_longer_than_the_window():
    from musicgeneration_amd.decode import window_schedule
    assert window_schedule([5], 100, 40) == window_schedule([5], 100, 40, 5)      # max(1, W // 8)
    assert window_schedule([3], 10, 4) == window_schedule([3], 10, 4, 1)
    bases, ts, _ = window_schedule([70], 60, 48, 12)
    assert (bases[0], ts[0]) == ([22], [47])                       # the last 48 prompt tokens
    assert window_schedule([5], 0, 40, 16) == ([], [], [])


def _check(model, x, length, **kw):
    from musicgeneration_amd import decode
    a = dict(return_probs=False, prefill="auto", prior_lengths=None, kv_cache="bf16")
    a.update(kw)
    return decode.check_args(model, x, length, a.pop("return_probs"), a.pop("prefill"), a.pop("prior_lengths"), a.pop("kv_cache"), **a)


@pytest.mark.parametrize("shape,length,kw,L,msg", [
    ((2, 5), 10, dict(window=1), 96, "window"),                    # window outside 2 .. max_seq
    ((2, 5), 10, dict(window=97), 96, "window"),
    ((2, 5), 10, dict(hop=4), 96, "hop"),                          # hop without window
    ((2, 5), 10, dict(window=40, hop=0), 96, "hop"),
    ((2, 5), 10, dict(window=40, hop=40), 96, "hop"),              # hop > W - 1: no cached token would be left
    ((3, 30), 80, dict(window=48, hop=27, prior_lengths=[9, 20, 30]), 96, "hop"),      # hop + spread (21) > W - 1
    ((3, 70), 80, dict(window=48, hop=37, prior_lengths=[9, 20, 70]), 96, "hop"),      # spread 39: start positions 8 and 47
    ((2, 5), 10, dict(window=40, prefill="token"), 96, "prefill"),
    ((2, 5), 10, dict(window=40, prefill="bogus"), 96, "prefill"),
    ((2, 5), 10, dict(window=92, hop=1), 92, "max_seq=92"),        # the re-anchor's 91 rows pad to 96
    ((2, 90), 10, dict(window=92, hop=30), 92, "max_seq=92"),      # the first prefill's 89 rows pad to 96
    ((4, 5), 10, dict(window=40, groups=2), 96, "groups"),
    ((4, 5), 10, dict(window=40, masked_groups=True), 96, "groups"),
    ((2, 5), 10, dict(window=40, kv_cache="int4"), 96, "kv_cache"),
])
def test_window_arguments_are_refused(shape, length, kw, L, msg):
    x = torch.randint(0, 300, shape)
    with pytest.raises(ValueError, match=msg):
        host_model(L).generate_cached(x, length, **kw)


def test_window_lifts_the_length_limit_and_nothing_else():
    m = host_model()
    x = torch.randint(0, 300, (3, 40))
    # accepted: (P, lens, batched prefill, hop); the default hop is max(1, W // 8)
    assert _check(m, x[:, :5], 100, window=40) == (5, None, True, 5)
    assert _check(m, x[:, :5], 100, window=40, return_probs=True, prefill="batched") == (5, None, True, 5)
    assert _check(m, x, 500, window=96, hop=32, prior_lengths=[9, 20, 30]) == (40, [9, 20, 30], True, 32)
    assert _check(m, x, 80, window=48, hop=26, prior_lengths=[9, 20, 30])[3] == 26          # hop + spread == W - 1
    assert _check(m, x, 500, window=2, hop=1) == (40, None, True, 1)
    assert _check(m, x, 5, window=48, prior_lengths=[7, 7, 7]) == (7, None, True, 6)        # equal lengths: the uniform call
    # without window the limit stands, for the uniform and the ragged call
    assert _check(m, x, 56) == (40, None, True, None)
    with pytest.raises(ValueError, match="max_seq"):
        m.generate_cached(x, 57)
    with pytest.raises(ValueError, match="max_seq"):
        m.generate_cached(x, 57, prior_lengths=[1, 5, 40])
    with pytest.raises(ValueError, match="1 .. 40"):               # the other checks hold with a window too
        m.generate_cached(x, 57, prior_lengths=[0, 5, 40], window=48)


def _midi(path, n):
    from musicgeneration_amd import smf
    smf.write_notes(path, [(80, 60 + i % 12, 0.5 * i, 0.5 * i + 0.25) for i in range(n)])
    return path


def test_window_cli_refusals(tmp_path):
    from musicgeneration_amd import generate
    base = ["-o", str(tmp_path / "out"), "-d", ""]
    with pytest.raises(SystemExit, match="--window"):
        generate.main(base + ["--hop", "4"])
    with pytest.raises(SystemExit, match="--reference-mask"):
        generate.main(base + ["--window", "40", "--reference-mask"])
    a, b = _midi(str(tmp_path / "a.mid"), 3), _midi(str(tmp_path / "b.mid"), 30)
    with pytest.raises(SystemExit, match="--reference-mask"):
        generate.main(base + ["--window", "40", "--reference-mask", "--condition-files", f"{a},{b}"])
    with pytest.raises(SystemExit, match="cannot be combined"):   # the other --condition-files refusals stay with --window
        generate.main(base + ["--window", "40", "--grammar", "--condition-files", f"{a},{b}"])
    with pytest.raises(SystemExit, match="exceeds -M 128"):        # and without --window the length refusal stays
        generate.main(base + ["-l", "100", "-M", "128", "--condition-files", f"{a},{b}"])
