"""Inputs for k_segment's live slots: a routing round with at most 128
pieces skips everything of its slots 2 and 3, so these are the smallest texts at which a skipped
slot could leave something behind, or pick something up -- stale classes, starts, marks and
compaction entries of the round before, the end sentinel next to the edge at 128, waves of one
workgroup on different branches, the class-0 spill and the long-piece staging in a short round.

Built on tests/segment_routing_cases.py (TILE, ROUND, SLOT, the words).  A tile is a list of
(piece, starts_a_document); every tile but a batch's last is exactly TILE bytes, so tile t of the
batch holds the pieces of list t.  The claims are checked on the CPU by
tests/test_segment_live_cpu.py with the oracle's pre-tokenizer and ids.
"""
from tests import segment_routing_cases as src

TILE, ROUND, SLOT = src.TILE, src.ROUND, src.SLOT
HALF = 2 * SLOT  # a round with more pieces than this runs slots 2 and 3

STALE_R = [1, 63, 64, 65, 127, 128]
EDGE_K = [0, 1, 4]
EDGE_R = [127, 128, 129, 130]
# what the pieces next to the edge are in turn; "doc": a hit that starts a document
KINDS = ["hit", "miss", "w16", "w32", "w64", "long", "doc"]
LETTERS = "etaoinshrdlucmfwypvbgkqjxz" * 3


def base_piece(w, i):
    return w.miss if i % 5 == 2 else w.hit


def plain(pieces):
    return [(p, False) for p in pieces]


def exact(w, tile, stretch):
    """The tile at exactly TILE bytes: the hits at the indices in `stretch` become words of up
    to 32 bytes (classes 1 and 2), the first ones the longest."""
    tile = list(tile)
    slack = TILE - sum(len(p) for p, _ in tile)
    assert slack >= 0
    for i in stretch:
        if not slack:
            break
        p, d = tile[i]
        assert p == w.hit
        k = min(30, slack)
        tile[i] = (" " + LETTERS[:1 + k], d)
        slack -= k
    assert slack == 0, "not enough hits to stretch"
    return tile


def docs_of(tiles):
    """The batch's documents: the first piece starts one, and every piece flagged."""
    docs = []
    for t, tile in enumerate(tiles):
        if t + 1 < len(tiles):
            assert sum(len(p) for p, _ in tile) == TILE
        else:
            assert sum(len(p) for p, _ in tile) <= TILE
        for p, d in tile:
            if d or not docs:
                docs.append("")
            docs[-1] += p
    return docs


def claims_of(tiles):
    return {"tile_np": [len(t) for t in tiles],
            "doc_start_pieces": [[i for i, (_, d) in enumerate(t) if d or (ti == 0 and i == 0)] for ti, t in enumerate(tiles)]}


def merged_upper_round(w):
    """A full round: hits in slots 0 and 1, only merged pieces in slots 2 and 3 -- misses, words of
    12, 24 and 48 bytes, and two long ones."""
    group = [w.miss] * 10 + [w.w16] * 3 + [w.w32] * 2 + [w.w64]
    order = [(i * 7) % 16 for i in range(16)]
    upper = [group[k] for k in order] * 8
    upper[5] = upper[100] = w.wlong
    assert len(upper) == HALF
    return plain([w.hit] * HALF + upper)


def stale_tile(w, r, kind):
    """A round whose slots 2 and 3 are full of merged pieces, then a last round of r hits or r
    misses: whatever the first round left for slots 2 and 3 must not be seen again."""
    return merged_upper_round(w) + plain([w.hit if kind == "hit" else w.miss] * r)


def stale_cases(w):
    out = []
    for kind in ("hit", "miss"):
        for r in STALE_R:
            tiles = [stale_tile(w, r, kind)]
            out.append(("stale_%s_%d" % (kind, r), tiles, {"upper_merged_then": r}))
    # the reverse order across two tiles: a tile ending in a short round, then a tile that begins
    # with the round of merged upper slots (and ends in a short round of the other kind)
    for r0, r1 in ((100, 128), (128, 1), (1, 65)):
        t0 = exact(w, stale_tile(w, r0, "miss"), range(HALF))
        out.append(("stale_two_tiles_%d_%d" % (r0, r1), [t0, stale_tile(w, r1, "hit")], {"upper_merged_then": r0}))
    return out


def kind_piece(w, kind):
    return {"hit": w.hit, "miss": w.miss, "w16": w.w16, "w32": w.w32, "w64": w.w64, "long": w.wlong, "doc": w.hit}[kind]


def edge_tile(w, k, r, s):
    """np = 256 k + r pieces; the pieces at 126, 127 and 128 of the last round (those that exist)
    take the kinds KINDS[s], KINDS[s + 1], KINDS[s + 2] (cyclically).  Returns the tile and
    {piece index: kind}."""
    np_ = ROUND * k + r
    tile = plain([base_piece(w, i) for i in range(np_)])
    placed = {}
    for i, at in enumerate((HALF - 2, HALF - 1, HALF)):
        j = ROUND * k + at
        if j < np_:
            kind = KINDS[(s + i) % len(KINDS)]
            tile[j] = (kind_piece(w, kind), kind == "doc")
            placed[j] = kind
    return tile, placed


def mixed_workgroup(w):
    """Three tiles of one workgroup whose last rounds hold 100, 200 and 128 pieces (slots 2 and 3
    skipped, run, skipped); a document starts on the first piece of each last round."""
    tiles = []
    for t, last in enumerate((100, 200, 128)):
        tile = plain([base_piece(w, i + t) for i in range(ROUND + last)])
        tile[ROUND] = (tile[ROUND][0], True)
        if t < 2:
            tile = exact(w, tile, [i for i in range(ROUND) if tile[i][0] == w.hit])
        tiles.append(tile)
    return tiles


def spill_tiles(w):
    """[(name, tile, spilled)]: more than 1040 class-0 pieces in a tile whose last round has at most
    128 pieces, the crossing inside that round (its slot 0; behind 60 hits, its slot 1)."""
    out = []
    for name, hits, misses in (("spill_slot0", 0, 4 * ROUND + 100), ("spill_slot1", 60, 4 * ROUND + HALF - 60)):
        tile = plain([w.hit] * hits + [w.miss] * misses)
        out.append((name, tile, misses - src.CAP0_LEAN))
    return out


def long_stage_tile(w):
    """40 pieces over 64 bytes: 30 in slots 2 and 3 of a full round, 10 in a last round of 100
    pieces, where the staging buffer of 32 fills."""
    upper = [w.wlong if i % 4 == 1 and i // 4 < 30 else w.hit for i in range(HALF)]
    last = [w.wlong if i % 10 == 3 else base_piece(w, i) for i in range(100)]
    tile = plain([w.hit] * HALF + upper + last)
    assert sum(p == w.wlong for p, _ in tile) == 40 > src.LONG_STAGE
    return tile


CJK = "日本語中文字漢한국어"


def cjk_piece(i, n):
    """' ' + n code points of 3 bytes."""
    return " " + "".join(CJK[(i + 3 * j) % len(CJK)] for j in range(n))


def non_ascii_cases():
    """[(name, tiles)]: tiles of 3-byte code points; the first tile's last round has more than 128
    pieces and the second's fewer, and the other way round."""
    full = plain([cjk_piece(i, 1) for i in range(TILE // 4)])  # 992 pieces of 4 bytes: last round 224
    assert len(full) % ROUND > HALF
    short = plain([cjk_piece(i, 2 if i % 5 == 1 and i < 5 * 164 else 1) for i in range(869)])  # 705 of 4 B, 164 of 7 B
    assert sum(len(p.encode()) for p, _ in short) == TILE and 0 < len(short) % ROUND < HALF
    return [("cjk_more_then_fewer", [full, plain([cjk_piece(i, 2) for i in range(ROUND + 100)])]),
            ("cjk_fewer_then_more", [short, plain([cjk_piece(i, 1) for i in range(ROUND + 200)])])]


def docs_of_bytes(tiles):
    """docs_of for tiles whose sizes are byte counts of UTF-8 (one document)."""
    for t, tile in enumerate(tiles):
        n = sum(len(p.encode()) for p, _ in tile)
        assert n == TILE if t + 1 < len(tiles) else n <= TILE
    return ["".join(p for tile in tiles for p, _ in tile)]
