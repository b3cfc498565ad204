"""k_segment's routing rounds on the GPU, bit-exact against the C oracle: the inputs of
tests/segment_routing_cases.py (their shapes are asserted on the CPU by
tests/test_segment_routing_cpu.py) through Tokenizer.encode_packed, on u16 piece records (the
gpt2 fixture) and u32 ones (the llama3 fixture).  Every input is a batch of its own, so its tiles
start at byte 0."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from complexity_tokenizer import Tokenizer
from datagen import corpus
from oracle import ref_c
from tests import added_cases
from tests import segment_routing_cases as src
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=["gpt2_path", "llama3_path"])
def rig(request):
    path = request.getfixturevalue(request.param)
    with open(path) as f:
        obj = json.load(f)
    rc = ref_c.RefC(obj)
    w = src.find_words(lambda s: rc.encode_packed(*corpus.pack([s.encode()]))[0].tolist())
    return path, obj, Tokenizer.from_file(path), rc, w


def check(tok, rc, docs):
    text, off = corpus.pack([d.encode() for d in docs])
    ids, toff = tok.encode_packed(text, off, timing=True)
    assert_same(ids, toff, *rc.encode_packed(text, off))
    return ids, toff


def filler_docs():
    text, off = corpus.corpus_c2(2000, seed=5)
    return [bytes(text[off[i]:off[i + 1]]).decode() for i in range(len(off) - 1)]


@pytest.mark.parametrize("group", ["slots", "three_tiles", "merged", "every_class", "long_stage", "doc_starts"])
def test_routing_cases(rig, group):
    _, _, tok, rc, w = rig
    picked = [(name, docs) for name, docs, _ in src.cases(w) if name.startswith(group)]
    assert picked
    for name, docs in picked:
        try:
            check(tok, rc, docs)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e)) from None
        if group == "long_stage":
            assert tok.last_stats["long_pieces"] == 40  # every one staged or appended, none spilled


def test_doc_starts_last_tile_of_a_batch(rig):
    """The doc-start input behind other tiles: its tile is the batch's last, ending in a round with
    one live slot (the start of the input is then not a tile's start)."""
    _, _, tok, rc, w = rig
    for empty in (False, True):
        check(tok, rc, [src.filled_tile(w, 400)] + src.doc_start_docs(w, empty))


def test_class0_spill_lean(rig):
    """The crossing of the class-0 capacity inside a round and inside a compaction pass, with the
    lean capacities: the pieces past the first 1040 go to the long list."""
    _, _, tok, rc, w = rig
    for (name, docs), spilled in zip(src.spill_batches(w, filler_docs()), (260, 160)):
        check(tok, rc, src.same_size_hits(w, docs))
        base = tok.last_stats["long_pieces"]  # the filler's own, in the same tiles
        check(tok, rc, docs)
        assert tok.last_stats["long_pieces"] == base + spilled, name


@pytest.mark.parametrize("safe", [False, True])
def test_class0_spill_process_capacities(rig, safe):
    """The same batches in a process of their own with CTOK_SAFE_CAPACITIES unset and set (the
    library reads it once per process)."""
    path = rig[0]
    env = dict(os.environ)
    env.pop("CTOK_SAFE_CAPACITIES", None)
    if safe:
        env["CTOK_SAFE_CAPACITIES"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "segment_routing_cases.py"), path], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    spilled = [int(line.rsplit(" ", 1)[1]) for line in r.stdout.splitlines() if "spilled" in line]
    # safe: every class-0 piece is listed, none spills
    assert spilled == ([0, 0] if safe else [260, 160]), r.stdout


def test_added_tokens_inside_pieces(rig):
    """A table whose added tokens match inside pieces (n_at != 0): every piece <= 32 B is listed,
    no whole-piece probe; over the slot-edge inputs."""
    _, obj, _, _, w = rig
    aobj = added_cases.with_added(obj, "plain")
    tok = Tokenizer.from_str(json.dumps(aobj))
    assert tok.num_piece_added_tokens() > 0
    rc = ref_c.RefC(aobj)
    for name, docs in src.slot_edge_docs(w):
        try:
            check(tok, rc, docs)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e)) from None


def test_two_calls_same_output(rig):
    """Nothing of a call's routing state survives into the next: the spill input and the dense
    round, twice each on one tokenizer, alternating."""
    _, _, tok, rc, w = rig
    spill = src.spill_batches(w, filler_docs())[1][1]
    dense = [src.round_with_merged(w, src.ROUND, "spread") * 2]
    first = {}
    for rep in range(2):
        for name, docs in (("spill", spill), ("dense", dense)):
            ids, toff = check(tok, rc, docs)
            if rep == 0:
                first[name] = (ids.copy(), toff.copy())
            else:
                assert np.array_equal(ids, first[name][0]) and np.array_equal(toff, first[name][1]), name
