"""k_segment's live slots on the GPU (a routing round with at most 128 pieces skips everything of
its slots 2 and 3), bit-exact on ids and token offsets against the C oracle through
Tokenizer.encode_packed: the inputs of tests/segment_live_cases.py, whose shapes are asserted on the
CPU by tests/test_segment_live_cpu.py.  On u16 piece records (the gpt2 fixture), u32 ones (the
llama3 fixture), a table with added tokens inside pieces (every listed piece in class 0) and, for the
non-ASCII tiles, the multilingual fixture.  Every input is a batch of its own of at most three
tiles, so its tiles start at byte 0."""
import json

import pytest

from complexity_tokenizer import Tokenizer
from datagen import corpus
from oracle import ref_c
from tests import added_cases
from tests import segment_live_cases as slc
from tests import segment_routing_cases as src
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["gpt2", "llama3", "gpt2_added"])
def rig(request):
    name = request.param
    path = request.getfixturevalue("llama3_path" if name == "llama3" else "gpt2_path")
    with open(path) as f:
        obj = json.load(f)
    # the words come from the plain table: with added tokens no piece is probed, whatever it is
    base = ref_c.RefC(obj)
    w = src.find_words(lambda s: base.encode_packed(*corpus.pack([s.encode()]))[0].tolist())
    if name == "gpt2_added":
        obj = added_cases.with_added(obj, "plain")
        tok = Tokenizer.from_str(json.dumps(obj))
        assert tok.num_piece_added_tokens() > 0
        return tok, ref_c.RefC(obj), w, True
    return Tokenizer.from_file(path), base, w, False


def check(tok, rc, docs, name=""):
    text, off = corpus.pack([d.encode() for d in docs])
    assert len(text) <= 3 * slc.TILE
    ids, toff = tok.encode_packed(text, off, timing=True)
    try:
        assert_same(ids, toff, *rc.encode_packed(text, off))
    except AssertionError as e:
        raise AssertionError("%s: %s" % (name, e)) from None


@pytest.mark.parametrize("kind", ["hit", "miss", "two_tiles"])
def test_stale_slots(rig, kind):
    """A full round whose slots 2 and 3 hold only merged pieces, then a last round of 1..128
    pieces, all hits or all misses; and the two kinds of round the other way round across tiles."""
    tok, rc, w, _ = rig
    picked = [(n, t) for n, t, _ in slc.stale_cases(w) if n.startswith("stale_" + kind)]
    assert len(picked) == (3 if kind == "two_tiles" else len(slc.STALE_R))
    for name, tiles in picked:
        check(tok, rc, slc.docs_of(tiles), name)


@pytest.mark.parametrize("r", slc.EDGE_R)
@pytest.mark.parametrize("k", slc.EDGE_K)
def test_edge_at_128(rig, k, r):
    """np = 256 k + r: the pieces at 126, 127 and 128 of the last round take every kind in turn
    (the last of them is the tile's last piece, and the end sentinel follows it)."""
    tok, rc, w, _ = rig
    for s in range(len(slc.KINDS)):
        tile, placed = slc.edge_tile(w, k, r, s)
        check(tok, rc, slc.docs_of([tile]), "k %d r %d %r" % (k, r, placed))


def test_mixed_workgroup(rig):
    """Three tiles of one workgroup with last rounds of 100, 200 and 128 pieces: its waves take
    different branches; a document starts on each last round's first piece."""
    tok, rc, w, _ = rig
    tiles = slc.mixed_workgroup(w)
    check(tok, rc, slc.docs_of(tiles), "mixed")
    check(tok, rc, slc.docs_of(tiles[::-1][1:] + tiles[-1:]), "mixed, other order")


def test_class0_spill_in_a_short_round(rig):
    """The class-0 capacity (1040, lean) crossed inside a last round of at most 128 pieces: the
    pieces past it go to the long list."""
    tok, rc, w, generic = rig
    for name, tile, spilled in slc.spill_tiles(w):
        check(tok, rc, slc.docs_of([tile]), name)
        # (with added tokens the hits are listed too: 60 more class-0 pieces in the second tile)
        assert tok.last_stats["long_pieces"] == spilled + (60 if generic and name == "spill_slot1" else 0), name


def test_long_staging_in_a_short_round(rig):
    """More than 32 long pieces in a tile, the staging buffer filling inside a last round of 100
    pieces (30 of them came from slots 2 and 3 of the round before)."""
    tok, rc, w, _ = rig
    tile = slc.long_stage_tile(w)
    check(tok, rc, slc.docs_of([tile]), "long_stage")
    assert tok.last_stats["long_pieces"] == 40


def test_non_ascii_rounds(multi_path):
    """Tiles of 3-byte code points: a last round of more than 128 pieces, then one of fewer, and
    the other way round."""
    with open(multi_path) as f:
        rc = ref_c.RefC(json.load(f))
    tok = Tokenizer.from_file(multi_path)
    for name, tiles in slc.non_ascii_cases():
        check(tok, rc, slc.docs_of_bytes(tiles), name)
        check(tok, rc, slc.docs_of_bytes(tiles[::-1][:1]), name + ", second tile alone")
