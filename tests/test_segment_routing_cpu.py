"""The inputs of tests/segment_routing_cases.py have the shapes they claim (CPU only): pieces per
tile, merged pieces per routing round, classes, document starts -- computed with the Python
oracle's pre-tokenizer and its ids ("merged": more than one token, or longer than 8 bytes)."""
import functools
import json

import pytest

from oracle import ref_py
from tests import segment_routing_cases as src


@pytest.fixture(scope="module", params=["gpt2_path", "llama3_path"])
def oracle(request):
    with open(request.getfixturevalue(request.param)) as f:
        py = ref_py.RefTokenizer(json.load(f))
    enc = functools.lru_cache(maxsize=None)(lambda s: tuple(py.encode(s)))
    return py, enc, src.find_words(enc)


def rounds(tile):
    return [tile[i:i + src.ROUND] for i in range(0, len(tile), src.ROUND)]


def test_words(oracle):
    _, enc, w = oracle
    assert len(w.hit) == 2 and len(enc(w.hit)) == 1
    assert len(w.miss) == 3 and len(enc(w.miss)) > 1
    assert [len(x) for x in (w.w16, w.w32, w.w64, w.wlong)] == [12, 24, 48, 80]
    assert src.MERGED_M[-1] == src.ROUND and {src.BUF - 1, src.BUF} <= set(src.MERGED_M)


def test_case_shapes(oracle):
    py, enc, w = oracle
    names = set()
    for name, docs, claims in src.cases(w):
        names.add(name)
        tiles = src.shape(docs, py.pieces, enc)
        assert b"".join(p for d in docs for p in py.pieces(d)) == "".join(docs).encode(), name
        assert [len(t) for t in tiles] == claims["tile_np"], name
        merged = [[src.is_merged(p, enc) for _, p in t] for t in tiles]
        if "merged" in claims:
            assert sum(map(sum, merged)) == claims["merged"], name
        if "round_merged" in claims:
            assert [sum(r) for r in rounds(merged[0])] == claims["round_merged"], name
        if "classes_per_round" in claims:
            for r in rounds(tiles[0]):
                got = {}
                for _, p in r:
                    c = src.piece_class(p, enc)
                    got[c] = got.get(c, 0) + 1
                assert got == claims["classes_per_round"], name
            # a piece's place in its class list differs from its ordinal among the merged pieces
            cls = [src.piece_class(p, enc) for _, p in tiles[0] if src.is_merged(p, enc)]
            assert any(cls[:k].count(c) != k for k, c in enumerate(cls) if k), name
        if "long" in claims:
            assert sum(len(p) > 64 for _, p in tiles[0]) == claims["long"] > src.LONG_STAGE, name
            assert any(len(p) <= 8 and src.is_merged(p, enc) for _, p in tiles[0]), name
        if "doc_start_pieces" in claims:
            assert [i for i, (first, _) in enumerate(tiles[0]) if first] == claims["doc_start_pieces"], name
    # the slot and round edges, from hits and from misses; every merged count at every place
    assert {"slots_%s_%d" % (k, n) for k in ("hit", "miss") for n in src.SLOT_EDGE_N} <= names
    assert {"merged_%d_%s" % (m, p) for m in src.MERGED_M for p in src.PLACES} <= names


def test_three_tiles_last_rounds(oracle):
    py, enc, w = oracle
    docs = dict((n, d) for n, d, _ in src.cases(w))["three_tiles"]
    live = [-(-(len(t) % src.ROUND) // src.SLOT) for t in src.shape(docs, py.pieces, enc)]
    assert live == [1, 2, 4]


def test_doc_starts_last_round_one_slot(oracle):
    py, enc, w = oracle
    for empty in (False, True):
        docs = src.doc_start_docs(w, empty)
        assert ("" in docs) == empty
        (tile,) = src.shape(docs, py.pieces, enc)
        assert 0 < len(tile) % src.ROUND <= src.SLOT


def test_spill_crossing(oracle):
    py, enc, w = oracle
    for (name, docs), (slot, pass_) in zip(src.spill_batches(w, []), [(0, 0), (1, 1)]):
        (tile,) = src.shape(docs, py.pieces, enc)
        c0 = [i for i, (_, p) in enumerate(tile) if src.piece_class(p, enc) == 0]
        assert len(c0) > src.CAP0_LEAN, name
        x = c0[src.CAP0_LEAN]  # the first piece that spills
        r = x // src.ROUND
        assert (x % src.ROUND) // src.SLOT == slot and 0 < x % src.SLOT, name  # inside a slot
        # its ordinal among the round's merged pieces: inside a compaction pass of 64
        k = sum(src.is_merged(p, enc) for _, p in tile[r * src.ROUND:x])
        assert k // 64 == pass_ and 0 < k % 64, name
