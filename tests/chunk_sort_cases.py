"""Inputs of tests/test_gpu_chunk_sort.py (and their CPU-side check in tests/test_chunk_sort_cpu.py):
texts of space-separated random lowercase words, so that almost no piece is a whole vocab token and
the merge passes' lists hold nearly every piece.

A call under 8192 tiles cuts its merge-pass chunks at 16 tiles (csrc/call_plan.h), so the sort
buffer's capacities (6016 entries in k_bpe_short with the 17..32 B pass folded in, 7168 without,
8192 on wide vocabularies) are met per 16-tile chunk: 63,488 B.  The <= 8 B inputs put a chosen
number of list entries into each chunk by mixing in 9..16 B words; a chunk of 9..16 B pieces holds
at most 7,056, so only the smallest capacity can be passed there, with mostly 9-byte pieces."""
import random

import numpy as np

TILE = 3968        # bytes per pre-tokenizer tile (csrc/ctok_internal.h kTile)
CHUNK_TILES = 16   # tiles per merge-pass chunk of a call under 8192 tiles (csrc/call_plan.h)
SORTCAPS = (6016, 7168, 8192)  # kernels.hip: k_bpe_short folded / narrow, and kSortCap
LETTERS = "abcdefghijklmnopqrstuvwxyz"


def _word(rng, piece_len):
    """A piece of piece_len bytes: a space and piece_len - 1 lowercase letters."""
    return " " + "".join(rng.choices(LETTERS, k=piece_len - 1))


def _text(rng, nbytes, lengths, weights):
    parts, n = [], 0
    while n < nbytes:
        k = rng.choices(lengths, weights)[0]
        parts.append(_word(rng, k))
        n += k
    # (the first word has no leading space: one letter more keeps it at its length)
    return rng.choice(LETTERS) + "".join(parts)[1:]


SHORT = ([2, 3, 4, 5, 6, 7, 8], [1, 2, 7, 20, 30, 20, 20])


def short_mix(seed, tiles, p_long):
    """2..8 B pieces, and 9..16 B pieces with probability p_long (they thin out the <= 8 B list)."""
    rng = random.Random(seed)
    ls, ws = SHORT
    tot = float(sum(ws))
    lengths = ls + list(range(9, 17))
    weights = [w / tot * (1 - p_long) for w in ws] + [p_long / 8] * 8
    return [_text(rng, tiles * TILE, lengths, weights)]


def inputs():
    """name -> list of documents."""
    rng = random.Random(77)
    c1 = list(range(9, 17))
    c2 = list(range(17, 33))
    out = {
        # <= 8 B entries per chunk: above every capacity; below the smallest; between the capacities
        "c0_over": short_mix(1, 64, 0.0),
        "c0_under": short_mix(2, 64, 0.27),
        "c0_mid1": short_mix(3, 64, 0.19),
        "c0_mid2": short_mix(4, 64, 0.12),
        # 9..16 B, every length: a chunk under the capacities, and one over the smallest
        "c1_under": [_text(rng, 64 * TILE, c1, [1] * 8)],
        "c1_over": [_text(rng, 64 * TILE, c1, [32] + [1] * 7)],
        # 17..32 B: a few per tile over 300 tiles, and nothing else over 64 tiles
        "c2_sparse": [_text(rng, 300 * TILE, SHORT[0] + c2, [w * 30 for w in SHORT[1]] + [1] * 16)],
        "c2_dense": [_text(rng, 64 * TILE, c2, [1] * 16)],
        # one length per class: every other bucket empty
        "c0_len8": [_text(rng, 8 * TILE, [8], [1])],
        "c1_len12": [_text(rng, 8 * TILE, [12], [1])],
        "c2_len24": [_text(rng, 8 * TILE, [24], [1])],
        # less than a tile, every class
        "tiny": [_text(rng, 1000, SHORT[0] + c1 + c2, SHORT[1] + [4] * 8 + [2] * 16)],
    }
    return out


def class_of(n):
    return 0 if n <= 8 else 1 if n <= 16 else 2 if n <= 32 else 3


def list_entries(ref, pieces_of, docs):
    """What the merge passes' lists hold of one input, from the oracle: for each piece of <= 32 B
    with more than one token (a whole-token piece is resolved by k_segment's probe) its class, chunk
    and length; and the fraction of the <= 8 B pieces with more than one token.
    ref: oracle.ref_c.RefC; pieces_of: oracle.ref_c.pieces."""
    from datagen import corpus

    text, _ = corpus.pack([d.encode() for d in docs])
    ps, starts, pos = [], [], 0
    for d in docs:
        for p in pieces_of(d.encode()):
            ps.append(p)
            starts.append(pos)
            pos += len(p)
    assert pos == len(text)
    pt, po = corpus.pack(ps)
    _, toff = ref.encode_packed(pt, po)
    ntok = np.diff(np.asarray(toff).astype(np.int64))
    plen = np.array([len(p) for p in ps])
    start = np.array(starts)
    multi = ntok > 1
    short = plen <= 8
    frac = float(multi[short].mean()) if short.any() else 1.0
    keep = multi & (plen <= 32)
    cls = np.array([class_of(n) for n in plen[keep]])
    return cls, start[keep] // (TILE * CHUNK_TILES), plen[keep], frac


def chunk_counts(cls, chunk, c):
    """Entries of class c per chunk."""
    return np.bincount(chunk[cls == c]) if (cls == c).any() else np.zeros(1, dtype=np.int64)
