"""generate.py --no-repeat-ngram on the GPU, as a user runs it: a child process on a saved checkpoint of the tamed model (nothing is
trained) writes its files; with -B the same flag exits with the refusal before any model is built."""
import glob
import os
import subprocess
import sys

import pytest
import torch

from decode_fixtures import prompt_file, tame_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_no_repeat_ngram_writes_its_files_and_refuses_a_beam(tmp_path):
    mt, _ = tame_model(d=128, nl=2, L=256, V=309)
    ckpt = str(tmp_path / "tame.pt")
    torch.save({"net": {k: v.cpu() for k, v in mt.state_dict().items()}}, ckpt)
    prompt = str(tmp_path / "prompt.mid")
    prompt_file(prompt, 5, 60)
    out = str(tmp_path / "g") + "/"
    common = [sys.executable, "-m", "musicgeneration_amd.generate", "-s", ckpt, "-o", out, "-b", "2", "-l", "60", "--num-layers", "2",
              "--d-model", "128", "-M", "256", "-c", prompt, "-d", str(tmp_path / "none"), "--no-repeat-ngram", "2"]
    r = subprocess.run(common + ["--frequency-penalty", "0.5"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert len(glob.glob(out + "gen-*.mid")) == 2 and r.stdout.count("===> ") == 2
    r = subprocess.run(common + ["-B", "2"], cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode != 0
    assert "--no-repeat-ngram cannot be combined with -B/--beam-size" in r.stderr
