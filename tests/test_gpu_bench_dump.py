"""bench.py end to end at a small size: `--steps` is the number of timed steps, and `--dump-outputs` writes what the last timed
step returned -- the words of every utterance and their offsets -- which must be what the CPU oracle decodes from the same
seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from speechrecognition_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_steps_and_dumped_outputs(tmp_path, oracle_lib):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--utts", "24",
           "--words", "40", "--mix", "4", "--no-cpu-baseline", "--no-dense-mfma", "--no-boundary", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["roofline"]["launches"] == 2 * line["roofline"]["chunks_per_step"] == 2
    assert sorted(os.listdir(out)) == ["word_off.npy", "words.npy"]
    words, woff = np.load(out / "words.npy"), np.load(out / "word_off.npy")
    assert words.dtype == woff.dtype == np.float64 and woff[-1] == len(words) == line["recognised_words_rank0"]
    # bench.py's inputs, from the same seeds
    lex = synth.make_lexicon(40, 3, 1)
    mp = str(tmp_path / "m.mix")
    synth.write_mixset(mp, synth.make_mixset(lex.n_states, 4, 39, seed=23))
    feats, off = synth.make_batch(24, 200, 400, 39, seed=7)
    orc = oracle_lib.Oracle(mp, 39, lex, am_threshold=200.0)
    for u in range(24):
        want = orc.decode(feats[int(off[u]):int(off[u + 1])])
        assert np.array_equal(words[int(woff[u]):int(woff[u + 1])], want.astype(np.float64)), u
    orc.close()
