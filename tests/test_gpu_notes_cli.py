"""generate.py --well-formed / --max-polyphony / --release on the GPU, as a user runs it: a child process on a saved checkpoint of
the tamed model (nothing is trained).  The written MIDI file must say what the token stream says: as many notes as the row has
note_on events, none of them closed by the fallback length."""
import glob
import os
import re
import subprocess
import sys

import pytest
import torch

from decode_fixtures import prompt_file, tame_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_well_formed_released_samples_are_written_note_for_note(tmp_path):
    from musicgeneration_amd import smf
    from musicgeneration_amd.sequence import DEFAULT_NOTE_LENGTH, EventSeq, NoteSeq
    mt, _ = tame_model(d=128, nl=2, L=256, V=309)
    ckpt = str(tmp_path / "tame.pt")
    torch.save({"net": {k: v.cpu() for k, v in mt.state_dict().items()}}, ckpt)
    prompt = str(tmp_path / "prompt.mid")
    prompt_file(prompt, 5, 60)
    ids = EventSeq.from_note_seq(NoteSeq.from_midi_file(prompt)).to_array()
    out = str(tmp_path / "g") + "/"
    r = subprocess.run([sys.executable, "-m", "musicgeneration_amd.generate", "-s", ckpt, "-o", out, "-b", "2", "-l", "120",
                        "--num-layers", "2", "--d-model", "128", "-M", "256", "-c", prompt, "--well-formed", "--max-polyphony", "4",
                        "--release", "-d", str(tmp_path / "none")], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert f"Prompt: {len(ids)} events" in r.stdout
    files = sorted(glob.glob(out + "gen-*.mid"))
    said = [int(n) for n in re.findall(r"===> \S+ \((\d+) notes\)", r.stdout)]     # the note_on events of every written row
    assert len(files) == 2 == len(said) and min(said) > 5                     # the prompt's five notes and new ones
    tick = 60.0 / 120 / 220                                                   # the writer's resolution at its tempo
    for path, n in zip(files, said):
        notes = smf.read_notes(path, range(128))
        assert len(notes) == n, (path, len(notes), n)
        for v, p, s, e in notes:
            assert abs((e - s) - DEFAULT_NOTE_LENGTH) > tick, (path, p, s, e)  # no note was left to the fallback length


def test_refused_combinations_exit_before_a_model_is_built(tmp_path, monkeypatch):
    from musicgeneration_amd import generate

    def no_model(*a, **k):
        raise AssertionError("a model was built")
    monkeypatch.setattr(generate, "MusicTransformer", no_model)
    base = ["-o", str(tmp_path / "out"), "-d", ""]
    for args, word in ((["--well-formed", "-B", "4"], "-B/--beam-size"), (["--max-polyphony", "4", "-B", "2"], "-B/--beam-size"),
                       (["--well-formed", "--repr", "remi", "--grammar"], "--repr midi_like"),
                       (["--max-polyphony", "4", "--release", "--repr", "remi"], "--repr midi_like")):
        with pytest.raises(SystemExit) as e:
            generate.main(base + args)
        assert word in str(e.value)
    with pytest.raises(SystemExit, match="--grammar"):
        generate._check_notes(generate.get_options(["--well-formed", "--grammar"]))
