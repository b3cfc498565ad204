"""Inputs for k_segment's routing rounds: the smallest texts at which the
round's full, partly filled and empty slots (a "live" slot holds a piece), the compaction of its
merged pieces and the list appends can go wrong.

A tile is 3968 bytes, a routing round is 256 pieces, a slot is 64 pieces.  A piece is "merged"
when a later pass produces its ids: it is longer than 8 bytes, or it is not one token.  Every
input is ASCII words after a space, so a piece is " " + letters and byte offsets are character
offsets.  The words are chosen per tokenizer (find_words) and the claims about each input are
checked on the CPU (tests/test_segment_routing_cpu.py) with the oracle's pre-tokenizer and ids.
"""
import itertools
import json
import string
import sys

TILE = 3968
ROUND = 256
SLOT = 64
CAP0_LEAN = 1040  # ctok_internal.h kCap0Lean
LONG_STAGE = 32   # segment.hip kSegLongCap
BUF = 256         # ctok_internal.h kSegListBuf: the compaction buffer holds a whole round

SLOT_EDGE_N = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 511, 512, 513]
MERGED_M = sorted({0, 1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 191, 192, 193, 255, 256,
                   BUF - 1, BUF} | ({BUF + 1} if BUF + 1 <= ROUND else set()))
PLACES = ("start", "end", "spread")


class Words:
    """hit: 2 bytes, one token.  miss: 3 bytes, more than one token.  w16 / w32 / w64 / wlong: words
    of 12, 24, 48 and 80 bytes (the 9..16, 17..32, 33..64 and > 64 byte classes)."""

    def __init__(self, hit, miss):
        self.hit, self.miss = hit, miss
        letters = "qxzjvkwpbg" * 8
        self.w16, self.w32, self.w64, self.wlong = (" " + letters[:k - 1] for k in (12, 24, 48, 80))


def find_words(encode):
    """encode(str) -> ids of one document (the oracle's)."""
    hit = next(" " + c for c in string.ascii_lowercase if len(encode(" " + c)) == 1)
    cons = "qxzjvkwpbg"
    miss = next(" " + a + b for a, b in itertools.product(cons, cons) if len(encode(" " + a + b)) > 1)
    return Words(hit, miss)


def is_merged(piece, encode):
    return len(piece) > 8 or len(encode(piece)) != 1


def piece_class(piece, encode):
    """'hit', or the list the piece is appended to without added tokens: 0 (<= 8 B), 1 (9..16),
    2 (17..32), 3 (33..64), 'long'."""
    n = len(piece)
    if n > 64:
        return "long"
    if n > 32:
        return 3
    if n > 16:
        return 2
    if n > 8:
        return 1
    return "hit" if len(encode(piece)) == 1 else 0


def filled_tile(w, np_):
    """np_ pieces in exactly TILE bytes: words of 2..32 bytes."""
    extra = TILE - 2 * np_
    assert 0 <= extra <= 30 * np_
    letters = "etaoinshrdlucmfwypvbgkqjxz" * 2
    out = []
    for i in range(np_):
        k = min(30, extra)
        extra -= k
        out.append(" " + letters[:1 + k])
    return "".join(out)


def round_with_merged(w, m, place):
    """One round of 256 pieces, m of them merged (3-byte misses among 2-byte hits)."""
    if place == "start":
        at = set(range(m))
    elif place == "end":
        at = set(range(ROUND - m, ROUND))
    else:  # evenly over the round, so over the slot boundaries
        at = {i * ROUND // m for i in range(m)} if m else set()
    assert len(at) == m
    return "".join(w.miss if i in at else w.hit for i in range(ROUND))


def every_class_rounds(w):
    """Two rounds (512 pieces, under one tile) with every class interleaved in piece order."""
    group = [w.hit] * 20 + [w.miss] * 6 + [w.w16] * 3 + [w.w32, w.w64, w.wlong]
    order = [(i * 13) % 32 for i in range(32)]  # a fixed permutation of the 32 (13 is odd)
    g = "".join(group[k] for k in order)
    text = g * 16
    assert len(text) < TILE
    return text


def spill_doc(w, n_hits, n_miss):
    """One tile: n_hits hits, then n_miss > kCap0Lean misses (the crossing of the class-0
    capacity is piece n_hits + 1040)."""
    text = w.hit * n_hits + w.miss * n_miss
    assert len(text) <= TILE and n_miss > CAP0_LEAN
    return text


def long_stage_doc(w, n_long=40):
    """n_long > 32 pieces over 64 B beside short merged ones and hits, in one tile."""
    text = (w.wlong + w.miss + w.hit) * n_long
    assert len(text) <= TILE and n_long > LONG_STAGE
    return text


def doc_start_docs(w, empty):
    """Documents beginning at pieces 63, 64, 65, 255, 256 and the tile's last piece (299: the
    tile's last round has one live slot); every fifth piece is a miss."""
    np_ = 300
    pieces = [w.miss if i % 5 == 2 else w.hit for i in range(np_)]
    cuts = [0, 63, 64, 65, 255, 256, np_ - 1, np_]
    docs = ["".join(pieces[a:b]) for a, b in zip(cuts, cuts[1:])]
    if empty:
        docs.insert(3, "")
    return docs


def cases(w):
    """[(name, docs, claims)]: claims are checked on the CPU by tests/test_segment_routing_cpu.py.
    Every input starts at byte 0 of a batch of its own, so its tiles are the batch's."""
    out = []
    for n in SLOT_EDGE_N:
        out.append(("slots_hit_%d" % n, [w.hit * n], {"tile_np": [n], "merged": 0}))
        out.append(("slots_miss_%d" % n, [w.miss * n], {"tile_np": [n], "merged": n}))
    three = [ROUND + 30, ROUND + 100, ROUND + 200]  # last rounds of 1, 2 and 4 live slots
    out.append(("three_tiles", [filled_tile(w, three[0]) + filled_tile(w, three[1]) + w.hit * three[2]],
                {"tile_np": three}))
    for m in MERGED_M:
        for place in PLACES:
            out.append(("merged_%d_%s" % (m, place), [round_with_merged(w, m, place) * 2],
                        {"tile_np": [2 * ROUND], "round_merged": [m, m]}))
    out.append(("every_class", [every_class_rounds(w)],
                {"tile_np": [2 * ROUND], "classes_per_round": {"hit": 160, 0: 48, 1: 24, 2: 8, 3: 8, "long": 8}}))
    out.append(("long_stage", [long_stage_doc(w)], {"tile_np": [120], "long": 40}))
    for empty in (False, True):
        out.append(("doc_starts_%s" % ("empty" if empty else "plain"), doc_start_docs(w, empty),
                    {"tile_np": [300], "doc_start_pieces": [0, 63, 64, 65, 255, 256, 299]}))
    return out


def slot_edge_docs(w):
    """The slot-edge inputs alone (run again on a table with added tokens inside pieces)."""
    return [(name, docs) for name, docs, _ in cases(w) if name.startswith("slots_") or name == "three_tiles"]


def spill_batches(w, filler):
    """[(name, docs)]: a tile of > 1040 misses first, filled up with a document of hits (no other
    document's pieces share the full class-0 list), then filler documents (str) so that the lean
    long list holds the spilled pieces.  The crossing falls in round 4, slot 0 (pass 0 of the
    round's 256 merged pieces) and, behind 100 hits, in slot 1 (pass 1)."""
    out = []
    for name, doc in (("spill_0", spill_doc(w, 0, 1300)), ("spill_100", spill_doc(w, 100, 1200))):
        assert (TILE - len(doc)) % 2 == 0
        out.append((name, [doc, w.hit * ((TILE - len(doc)) // 2)] + filler))
    return out


def same_size_hits(w, docs):
    """The batch with its first document replaced by hits of the same byte length: the other
    documents lie in the same tiles, and nothing of the first one is merged."""
    assert len(docs[0]) % 2 == 0
    return [w.hit * (len(docs[0]) // 2)] + docs[1:]


def shape(docs, pieces_of, encode_piece):
    """Per tile of the packed batch: the pieces that start in it, as (doc_start, piece) in order.
    pieces_of(str) -> the document's pieces (bytes)."""
    tiles = {}
    pos = 0
    for d in docs:
        first = True
        for p in pieces_of(d):
            tiles.setdefault(pos // TILE, []).append((first, p.decode()))
            first = False
            pos += len(p)
    return [tiles.get(t, []) for t in range((pos + TILE - 1) // TILE)]


def main(argv):
    """Child process of the class-0 spill test: the spill batches with the process's capacities
    (CTOK_SAFE_CAPACITIES is read once per process), bit-exact against the C oracle."""
    import numpy as np

    from complexity_tokenizer import Tokenizer
    from datagen import corpus
    from oracle import ref_c

    path = argv[1]
    with open(path) as f:
        obj = json.load(f)
    rc = ref_c.RefC(obj)
    w = find_words(lambda s: rc.encode_packed(*corpus.pack([s.encode()]))[0].tolist())
    tok = Tokenizer.from_file(path)
    ftext, foff = corpus.corpus_c2(2000, seed=5)
    filler = [bytes(ftext[foff[i]:foff[i + 1]]).decode() for i in range(len(foff) - 1)]
    def run(docs):
        text, off = corpus.pack([d.encode() for d in docs])
        ids, toff = tok.encode_packed(text, off, timing=True)
        rids, roff = rc.encode_packed(text, off)
        return np.array_equal(toff, roff) and np.array_equal(ids, rids), tok.last_stats["long_pieces"]

    for name, docs in spill_batches(w, filler):
        ok, n_long = run(docs)
        ok0, base = run(same_size_hits(w, docs))
        if not (ok and ok0):
            print("%s: differs from the oracle" % name)
            return 1
        print("%s: spilled %d" % (name, n_long - base))
    return 0


if __name__ == "__main__":
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "complexity-tokenizer_amd")]
    sys.exit(main(sys.argv))
