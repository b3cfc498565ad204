"""The inputs of tests/segment_live_cases.py have the shapes they claim (CPU only): pieces per tile,
which rounds run slots 2 and 3, what those slots hold, where documents start, where the class-0
capacity is crossed -- computed with the Python oracle's pre-tokenizer and its ids."""
import functools
import json

import pytest

from oracle import ref_py
from tests import segment_live_cases as slc
from tests import segment_routing_cases as src

ROUND, HALF = slc.ROUND, slc.HALF


@pytest.fixture(scope="module", params=["gpt2_path", "llama3_path"])
def oracle(request):
    with open(request.getfixturevalue(request.param)) as f:
        py = ref_py.RefTokenizer(json.load(f))
    enc = functools.lru_cache(maxsize=None)(lambda s: tuple(py.encode(s)))
    return py, enc, src.find_words(enc)


def shape_matches(py, enc, tiles, docs):
    """The batch's tiles hold exactly the pieces of the lists, with their document starts."""
    got = src.shape(docs, py.pieces, enc)
    assert [[p for _, p in t] for t in got] == [[p for p, _ in t] for t in tiles]
    want = slc.claims_of(tiles)
    assert [len(t) for t in got] == want["tile_np"]
    assert [[i for i, (first, _) in enumerate(t) if first] for t in got] == want["doc_start_pieces"]


def test_stale_cases(oracle):
    py, enc, w = oracle
    names = set()
    for name, tiles, claims in slc.stale_cases(w):
        names.add(name)
        shape_matches(py, enc, tiles, slc.docs_of(tiles))
        t0 = [p for p, _ in tiles[0]]
        assert len(t0) == ROUND + claims["upper_merged_then"] and len(t0) - ROUND <= HALF
        assert all(src.is_merged(p, enc) for p in t0[HALF:ROUND])  # slots 2 and 3 of the full round
        got = {src.piece_class(p, enc) for p in t0[HALF:ROUND]}
        assert got == {0, 1, 2, 3, "long"}, name
        if len(tiles) == 2:  # the second tile begins with the round of merged upper slots
            t1 = [p for p, _ in tiles[1]]
            assert all(src.is_merged(p, enc) for p in t1[HALF:ROUND]) and 0 < len(t1) - ROUND <= HALF
    assert {"stale_%s_%d" % (k, r) for k in ("hit", "miss") for r in slc.STALE_R} <= names
    for r in slc.STALE_R:  # the last round is all hits, or all misses
        assert not any(src.is_merged(p, enc) for p, _ in slc.stale_tile(w, r, "hit")[ROUND:])
        assert all(src.piece_class(p, enc) == 0 for p, _ in slc.stale_tile(w, r, "miss")[ROUND:])


@pytest.mark.parametrize("k", slc.EDGE_K)
def test_edge_tiles(oracle, k):
    py, enc, w = oracle
    want = {"hit": "hit", "miss": 0, "w16": 1, "w32": 2, "w64": 3, "long": "long", "doc": "hit"}
    for r in slc.EDGE_R:
        seen = {}
        for s in range(len(slc.KINDS)):
            tile, placed = slc.edge_tile(w, k, r, s)
            assert len(tile) == ROUND * k + r
            shape_matches(py, enc, [tile], slc.docs_of([tile]))
            for j, kind in placed.items():
                assert src.piece_class(tile[j][0], enc) == want[kind]
                seen.setdefault(j - ROUND * k, set()).add(kind)
        # pieces 126, 127 and 128 of the last round, where they exist, took every kind
        assert sorted(seen) == [at for at in (HALF - 2, HALF - 1, HALF) if at < r]
        assert all(kinds == set(slc.KINDS) for kinds in seen.values())
        # so did the tile's last piece, which the end sentinel follows (np = 130: piece 129, a base piece)
        assert r - 1 in seen or r - 1 > HALF


def test_mixed_workgroup(oracle):
    py, enc, w = oracle
    tiles = slc.mixed_workgroup(w)
    shape_matches(py, enc, tiles, slc.docs_of(tiles))
    assert [len(t) - ROUND for t in tiles] == [100, 200, 128]
    assert all(t[ROUND][1] for t in tiles)


def test_spill_and_long_stage(oracle):
    py, enc, w = oracle
    for (name, tile, spilled), slot in zip(slc.spill_tiles(w), (0, 1)):
        shape_matches(py, enc, [tile], slc.docs_of([tile]))
        c0 = [i for i, (p, _) in enumerate(tile) if src.piece_class(p, enc) == 0]
        assert len(c0) == src.CAP0_LEAN + spilled and spilled > 0, name
        x = c0[src.CAP0_LEAN]  # the first piece that spills: in the last round, which has <= 128 pieces
        assert x // ROUND == len(tile) // ROUND == 4 and 0 < len(tile) % ROUND <= HALF, name
        assert (x % ROUND) // slc.SLOT == slot and 0 < x % slc.SLOT, name
    tile = slc.long_stage_tile(w)
    shape_matches(py, enc, [tile], slc.docs_of([tile]))
    longs = [i for i, (p, _) in enumerate(tile) if len(p) > 64]
    assert len(longs) == 40 and len(tile) == ROUND + 100
    assert longs[src.LONG_STAGE] >= ROUND  # the staging buffer fills inside the short last round
    assert all(HALF <= i < ROUND for i in longs[:30])


def test_non_ascii(multi_path):
    with open(multi_path) as f:
        py = ref_py.RefTokenizer(json.load(f))
    enc = lambda s: tuple(py.encode(s))  # noqa: E731
    lasts = []
    for name, tiles in slc.non_ascii_cases():
        docs = slc.docs_of_bytes(tiles)
        got = src.shape(docs, py.pieces, enc)
        assert [[p for _, p in t] for t in got] == [[p for p, _ in t] for t in tiles], name
        assert all(len(c.encode()) == 3 for p, _ in tiles[0] for c in p[1:])
        lasts.append([len(t) % ROUND > HALF for t in tiles])
    assert lasts == [[True, False], [False, True]]
