"""Argument checks of the ragged-prompt decode (generate_cached(prior_lengths=...), generate.py --condition-files): they
run on the host before any device work, so they are tested without a GPU."""
import pytest
import torch

from decode_fixtures import host_model


@pytest.mark.parametrize("lens,length,kw,msg", [
    ([0, 5, 40], 10, {}, "1 .. 40"),                               # an empty prompt
    ([41, 5, 40], 10, {}, "1 .. 40"),                              # longer than prior is wide
    ([1, 5], 10, {}, "2 entries"),                                 # one length per row
    ([1, 5, 40], 57, {}, "max_seq"),                               # Pmax + length > max_seq
    ([1, 5, 40], 10, dict(prefill="token"), "prefill"),            # no token-by-token prefill of ragged prompts
    ([1, 5, 40], 10, dict(prefill="bogus"), "prefill"),
])
def test_prior_lengths_are_refused(lens, length, kw, msg):
    x = torch.randint(0, 300, (3, 40))
    with pytest.raises(ValueError, match=msg):
        host_model().generate_cached(x, length, prior_lengths=lens, **kw)


def test_ragged_batched_prefill_that_pads_past_max_seq_is_refused():
    x = torch.randint(0, 300, (2, 90))                             # 89 prefill rows pad to 96 > max_seq 92
    with pytest.raises(ValueError, match="max_seq=92"):
        host_model(L=92).generate_cached(x, 2, prior_lengths=[90, 3])


def _midi(path, n):
    from musicgeneration_amd import smf
    smf.write_notes(path, [(80, 60 + i % 12, 0.5 * i, 0.5 * i + 0.25) for i in range(n)])
    return path


def test_condition_files_cli_refusals(tmp_path):
    from musicgeneration_amd import generate
    a, b = _midi(str(tmp_path / "a.mid"), 3), _midi(str(tmp_path / "b.mid"), 30)
    base = ["-o", str(tmp_path / "out"), "-d", "", "--condition-files", f"{a},{b}"]
    for extra in (["-c", a], ["--grammar"], ["--reference-mask"]):
        with pytest.raises(SystemExit, match="cannot be combined"):
            generate.main(base + extra)
    with pytest.raises(SystemExit) as e:
        generate.main(base + ["-l", "100", "-M", "128"])
    msg = str(e.value)
    from musicgeneration_amd.sequence import EventSeq, NoteSeq
    longest = len(EventSeq.from_note_seq(NoteSeq.from_midi_file(b)).to_array())
    assert f"({longest} events)" in msg and "-l 100" in msg and "-M 128" in msg
