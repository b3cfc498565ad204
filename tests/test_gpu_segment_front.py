"""k_segment's mask gathers, routing slots and per-tile doc-start bits on the GPU, bit-exact against
the C oracle through Tokenizer.encode_packed, on u16 piece records (the gpt2 fixture) and u32
ones (the llama3 fixture).  Every input is a batch of its own of at most three tiles (3968 bytes
each), so its tiles start at byte 0; tok_off is what checks the doc-start bits (pdoc)."""
import json
import re

import pytest

from complexity_tokenizer import Tokenizer
from datagen import corpus
from oracle import ref_c
from tests import segment_routing_cases as src
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

TILE = src.TILE
LENGTHS = list(range(1, 10)) + [16, 17, 32, 33, 64, 65]
LETTERS = "qxzjvkwpbg" * 7


@pytest.fixture(scope="module", params=["gpt2_path", "llama3_path"])
def rig(request):
    path = request.getfixturevalue(request.param)
    with open(path) as f:
        obj = json.load(f)
    rc = ref_c.RefC(obj)
    enc = lambda s: rc.encode_packed(*corpus.pack([s.encode()]))[0].tolist()  # noqa: E731
    return Tokenizer.from_file(path), rc, src.find_words(enc), enc


def check_bytes(tok, rc, docs):
    text, off = corpus.pack(docs)
    assert len(text) <= 3 * TILE
    ids, toff = tok.encode_packed(text, off, timing=True)
    assert_same(ids, toff, *rc.encode_packed(text, off))


def check(tok, rc, docs):
    check_bytes(tok, rc, [d.encode() for d in docs])


def eight_byte_token(enc):
    """A piece of 8 bytes (' ' + 7 letters) that is one token: from the English filler corpus."""
    text, _ = corpus.corpus_c2(2000, seed=5)
    seen = set()
    for m in re.finditer(rb" [a-z]{7}(?![a-z])", bytes(text)):
        p = m.group().decode()
        if p not in seen:
            seen.add(p)
            if len(enc(p)) == 1:
                return p
    raise AssertionError("no 8-byte single-token piece in the filler corpus")


def lengths_and_shifts(enc):
    """Pieces of every length in LENGTHS at every start offset mod 4, as ' ' + letters (length 1:
    a digit or a letter behind the other class).  One-byte pieces '7', 'x', '7' move the offset."""
    hit8 = eight_byte_token(enc)
    miss8 = " " + LETTERS[:7]
    assert len(hit8) == 8 and len(enc(miss8)) > 1
    out, pos, placed = [], 0, set()

    def put(piece):
        nonlocal pos
        out.append(piece)
        pos += len(piece)

    put(" start")
    for n in LENGTHS:
        variants = [" " + LETTERS[:n - 1], " " + "etaoinsh"[:n - 1]] if 2 <= n <= 8 else [" " + LETTERS[:n - 1]]
        if n == 8:
            variants = [hit8, miss8]
        for piece in variants:
            for s in range(4):
                pad = "7x7"[:(s - pos) % 4]
                if n == 1:
                    piece = "x" if pad.endswith("7") else "7"
                for c in pad:
                    put(c)
                assert pos % 4 == s
                placed.add((n, s))
                put(piece)
                if n == 1:
                    put(" sep")  # (a word next, so the following pad's digit stands alone)
    assert placed == {(n, s) for n in LENGTHS for s in range(4)}
    return "".join(out)


def test_lengths_and_shifts(rig):
    tok, rc, w, enc = rig
    doc = lengths_and_shifts(enc)
    check(tok, rc, [doc])
    check(tok, rc, [w.hit * 31 + doc])  # the same pieces at other offsets of the 64-byte words
    check(tok, rc, ["ab", doc, "", doc[7:2000]])


@pytest.mark.parametrize("doc_len", [1, 2, 3])
def test_documents_of_one_to_three_bytes(rig, doc_len):
    """Nearly every piece starts a document: three tiles of documents of doc_len bytes."""
    tok, rc, w, _ = rig
    kinds = {1: ["a", " ", "7", ".", "b"], 2: [w.hit, "ab", "a ", " 7", "'s", ".."], 3: [w.miss, w.hit + "c", "a b", "12 ", "'ll", " 's"]}[doc_len]
    n = 3 * TILE // doc_len
    docs = [kinds[(i * 7 + i // 5) % len(kinds)] for i in range(n)]
    assert all(len(d) == doc_len for d in docs)
    check(tok, rc, docs)
    check(tok, rc, [d if i % 11 else "" for i, d in enumerate(docs)])  # empty documents mixed in


def test_tile_sizes(rig):
    """Tiles of exactly 255, 256 and 257 pieces (a round is 256), and of exactly one piece."""
    tok, rc, w, _ = rig
    check(tok, rc, [src.filled_tile(w, 255) + src.filled_tile(w, 256) + src.filled_tile(w, 257)])
    one = " " + ("etaoinshrdlucmfwypvbgkqjxz" * 160)[:TILE - 1]  # a tile that is one piece
    assert len(one) == TILE
    check(tok, rc, [one + src.filled_tile(w, 256)])
    check(tok, rc, [src.filled_tile(w, 257) + one + w.hit])
    check(tok, rc, ["a"])
    check(tok, rc, [w.hit])


@pytest.mark.parametrize("np_", [127, 128, 129, 384, 385])
def test_live_slot_boundary(rig, np_):
    """Tiles whose last round fills half of its four slots, one piece less and one more (127, 128,
    129 pieces; 256 + 128, 256 + 129), from hits and from misses."""
    tok, rc, w, _ = rig
    check(tok, rc, [src.filled_tile(w, np_)])
    check(tok, rc, [w.hit * np_])
    check(tok, rc, [w.miss * np_])
    check(tok, rc, [src.filled_tile(w, np_) + w.miss * np_])


def test_edge_documents(rig):
    """Documents starting at the first and the last piece of a tile and at bytes 0 and 63 of a
    64-byte word, with empty documents between them."""
    tok, rc, w, _ = rig
    base = ((w.hit * 3 + w.miss) * 2000)[:2 * TILE + 500]
    assert (len(w.hit * 3 + w.miss)) % 2 == 1  # pieces drift over the byte offsets mod 64
    cuts = sorted({0, 63, 64, 127, 128, 64 * 31 + 63, 64 * 32, TILE - 64, TILE - 3, TILE - 1, TILE, TILE + 63, TILE + 64,
                   2 * TILE - 2, 2 * TILE - 1, 2 * TILE, 2 * TILE + 63, len(base) - 1, len(base)})
    docs = [base[a:b] for a, b in zip(cuts, cuts[1:])]
    check(tok, rc, docs)
    with_empty = []
    for i, d in enumerate(docs):
        with_empty += [""] * (i % 3) + [d]
    check(tok, rc, [""] + with_empty + ["", ""])
    # a document starting at the last piece of each tile, found from the pieces themselves
    piece = len(w.hit)
    last0 = (TILE - 1) // piece * piece
    body = w.hit * (3 * TILE // piece)
    check(tok, rc, [body[:last0], body[last0:TILE + 64], "", body[TILE + 64:2 * TILE - piece], body[2 * TILE - piece:]])


def test_mask_phase_non_ascii(rig):
    """A 2,000-document slice of the multilingual corpus (C5), three tiles at a time."""
    tok, rc, _, _ = rig
    text, off = corpus.corpus_c5(2000, seed=5)
    docs = corpus.unpack(text, off)
    batch, size = [], 0
    for d in docs:
        d = bytes(d)
        assert len(d) <= 3 * TILE
        if size + len(d) > 3 * TILE:
            check_bytes(tok, rc, batch)
            batch, size = [], 0
        batch.append(d)
        size += len(d)
    check_bytes(tok, rc, batch)


def test_mask_phase_every_ascii_byte(rig):
    """Every byte value 0..127 at every position mod 8 (a dword pair is one pack8): eight runs of
    the 128 values, each one byte further on; then the same with document starts inside."""
    tok, rc, _, _ = rig
    run = bytes(range(128))
    text = b"".join(run + b"a" for _ in range(8))
    seen = {(b, i % 8) for i, b in enumerate(text)}
    assert {(b, p) for b in range(128) for p in range(8)} <= seen
    check_bytes(tok, rc, [text])
    check_bytes(tok, rc, [text[i:i + 37] for i in range(0, len(text), 37)])
    # every value next to every class of neighbour: letter, digit, space, apostrophe
    for nb in (b"a", b"7", b" ", b"'"):
        check_bytes(tok, rc, [b"".join(bytes([b]) + nb for b in range(128)) * 3])
