"""bench.py's command line on a small C4-shaped corpus (--docs 20000, one GPU): a plain run times
exactly --steps steps and reports `ms_per_step` without the --full parts, and --dump-outputs
writes the last timed step's outputs, checked here against the C oracle on the same seeded corpus.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from datagen import corpus
from oracle import ref_c

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOCS = 20_000  # 2.6 MB, ~0.9M tokens: below bench.DUMP_IDS / DUMP_OFFS, so the dump holds every element


def test_plain_run_dumps_the_last_steps_outputs(tmp_path, gpt2_path):
    out_dir = tmp_path / "dump"
    env = dict(os.environ, TMPDIR=str(tmp_path))  # bench.py's corpus cache goes under the test's directory
    env.pop("WORLD_SIZE", None)
    proc = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                           "--docs", str(DOCS), "--dump-outputs", str(out_dir)], cwd=ROOT, env=env, capture_output=True,
                          text=True, timeout=300)
    assert proc.returncode == 0, proc.stderr[-4000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["unit"] == "MB/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert res["ms_per_step"] > 0
    # value = bytes x steps / wall time of the timed steps, ms_per_step = that wall time / steps
    assert res["value"] == pytest.approx(res["config"]["bytes_per_gpu"] / (res["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    # nothing of --full ran
    assert res["parity"] is None and res["user_facing"] is None and res["cpu_baseline"] is None
    assert res["roofline"]["traffic"] is None

    text, off = corpus.corpus_c4_range(0, DOCS, DOCS)
    ids, tok_off = ref_c.RefC.from_file(gpt2_path).encode_packed(text, off, threads=8)
    assert sorted(os.listdir(out_dir)) == ["ids_sample.npy", "n_tokens.npy", "tok_off_sample.npy"]
    n_tokens = np.load(out_dir / "n_tokens.npy")
    got_ids = np.load(out_dir / "ids_sample.npy")
    got_off = np.load(out_dir / "tok_off_sample.npy")
    assert n_tokens.dtype == np.float64 and got_ids.dtype == np.float32 and got_off.dtype == np.float64
    assert n_tokens.tolist() == [float(len(ids))]
    assert res["config"]["tokens_per_gpu"] == len(ids)
    assert np.array_equal(got_ids, ids.astype(np.float32))
    assert np.array_equal(got_off, tok_off.astype(np.float64))
