"""The 17..32 B pass by each of its arms, against the C oracle (CTOK_MID_PACKED, read when the
tokenizer's device tables are made): 0 the 32 + 32 register tier in k_bpe_mid<2>, 1 the packed
tier (tokens and pair values as u16 pairs, csrc/merge_packed_hd.h) in k_bpe_mid<2>, 2 the packed tier
as the third pass of k_bpe_short when the call has no long piece (else as 1).  The packed arms
exist for narrow compact tables whose values all fit 16 bits (the gpt2_50k fixture, the 65,535-id
prefix of llama3); a table without the property (the shuffled-merges table, whose values are
ranks; the 128k-vocabulary llama3 fixture) runs the register tier whatever the switch says.

The batch: pieces of every length 17..32 B in a few hundred short documents -- words over the
fixture's common letters (deep merges), periodic strings (equal pairs repeated, so the leftmost
rule decides), digit runs, consonant strings (they stop merging above 16 tokens) and one document
whose 17..32 B pieces lie across pre-tokenizer tile ends."""
import json
import random

import numpy as np
import pytest

from complexity_tokenizer import Tokenizer
from datagen import corpus
from oracle import ref_c
from tests import id16_cases, packed_cases, toys
from tests.packed_cases import TILE, env as _env
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

DEFAULT_ARM = 2  # csrc/ctok_internal.h kMidPackedDefault
ARMS = [None, "0", "1", "2"]
ARM_IDS = ["default", "register", "packed_mid", "packed_fold"]
PACKED_TABLES = ("gpt2", "trunc65535")


def _docs(seed):
    return packed_cases.docs(seed, 17, 33, 12)


def _class2_lengths(docs):
    """Pieces of 17..32 B per length, by the oracle's pre-tokenizer."""
    cnt = {n: 0 for n in range(17, 33)}
    for d in docs:
        for p in ref_c.pieces(d.encode()):
            if 17 <= len(p) <= 32:
                cnt[len(p)] += 1
    return cnt


@pytest.fixture(scope="module")
def objs(gpt2_path, llama3_path):
    """name -> tokenizer.json object (built once)."""
    cache = {}

    def get(name):
        if name not in cache:
            with open(gpt2_path if name in ("gpt2", "shuffled") else llama3_path) as f:
                obj = json.load(f)
            if name == "shuffled":
                obj = toys.shuffled_merges(obj, seed=16)
            if name == "trunc65535":
                obj = toys.truncated(obj, 65535)
            cache[name] = obj
        return cache[name]

    return get


@pytest.fixture(scope="module")
def cases(objs):
    """(table, batch) -> (tokenizer JSON text, docs, packed text, offsets, oracle ids, oracle
    offsets); each oracle result computed once and shared by the arms."""
    cache = {}

    def docs_of(name, kind):
        base = _docs(32)
        if name == "trunc65535":
            # the table's top ids through 17..32 B pieces: value 0xFFFE beside the 0xFFFF sentinel
            obj = objs(name)
            base = base + [d for d in id16_cases.boundary_docs(obj, reps=2) if 17 <= len(d.encode()) <= 32]
            base.append(id16_cases.tile_end_doc(obj))
        if kind == "long":  # one piece of 101 B: the call has a long piece
            base = base + ["x " + "".join(random.Random(5).choice("etaoinshrdlu") for _ in range(100)) + " y"]
        return base

    def get(name, kind="plain"):
        key = (name, kind)
        if key not in cache:
            docs = docs_of(name, kind)
            text, off = corpus.pack([d.encode() for d in docs])
            obj = objs(name)
            ids, toff = ref_c.RefC(obj).encode_packed(text, off)
            cache[key] = (json.dumps(obj), docs, text, off, ids, toff)
        return cache[key]

    return get


def _expected_arm(name, arm):
    if name not in PACKED_TABLES:
        return 0
    return DEFAULT_ARM if arm is None else int(arm)


_class2_seen = {}


def test_batches_hold_every_length(cases, objs):
    """On the oracle's side first: every length 17..32 B occurs, the long-piece batch has its long
    piece, and the boundary table's top id goes through 17..32 B pieces."""
    _, docs, _, _, _, _ = cases("gpt2")
    cnt = _class2_lengths(docs)
    assert all(c > 0 for c in cnt.values()), cnt
    assert sum(cnt.values()) > 1500
    _, ldocs, _, _, _, _ = cases("gpt2", "long")
    assert max(len(p) for p in ref_c.pieces(ldocs[-1].encode())) > 64
    _, bdocs, _, _, ids, off = cases("trunc65535")
    cnt = _class2_lengths(bdocs)
    assert all(c > 0 for c in cnt.values()), cnt
    top, near = id16_cases.class_counts(bdocs, ids, off, 65535)
    assert top[2] >= 1 and near[2] >= 100, (top, near)


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
@pytest.mark.parametrize("name", ["gpt2", "shuffled", "llama3", "trunc65535"])
def test_mid_arms_vs_oracle(cases, name, arm):
    js, docs, text, off, ref_ids, ref_off = cases(name)
    with _env("CTOK_MID_PACKED", arm):
        tok = Tokenizer.from_str(js)
        ids, toff = tok.encode_packed(text, off, timing=True)
        st = tok.last_stats
    p = tok.table_props
    assert p["short_packed"] == (name in PACKED_TABLES)
    assert p["dev_mid_packed"] == _expected_arm(name, arm)
    assert st["long_pieces"] == 0
    assert_same(ids, toff, ref_ids, ref_off)
    # the 17..32 B class did the work, and the same work in every arm of the table
    c2 = (st["class_bytes"][2], st["class_ids"][2])
    assert c2[0] > 17 * 1500 and c2[1] > 0
    assert _class2_seen.setdefault(name, c2) == c2


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
def test_long_piece_keeps_class_in_mid_kernel(cases, arm):
    """A call with a long piece: k_bpe_short leaves the class to k_bpe_mid<2> (both sides decide
    from the long-piece counter); the class is merged once, in every arm."""
    js, docs, text, off, ref_ids, ref_off = cases("gpt2", "long")
    with _env("CTOK_MID_PACKED", arm):
        tok = Tokenizer.from_str(js)
        ids, toff = tok.encode_packed(text, off, timing=True)
        st = tok.last_stats
    assert tok.table_props["dev_mid_packed"] == _expected_arm("gpt2", arm)
    assert st["long_pieces"] == 1
    assert_same(ids, toff, ref_ids, ref_off)
    c2 = (st["class_bytes"][2], st["class_ids"][2])
    assert c2[0] > 17 * 1500
    assert _class2_seen.setdefault("gpt2-long", c2) == c2


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
def test_no_mid_piece_at_all(objs, arm):
    """No 17..32 B piece in the call: the third pass finds nothing."""
    rng = random.Random(9)
    docs = [" ".join("".join(rng.choice("etaoinshrdlu") for _ in range(rng.randrange(1, 15))) for _ in range(60))
            for _ in range(200)]
    assert sum(_class2_lengths(docs).values()) == 0
    text, off = corpus.pack([d.encode() for d in docs])
    obj = objs("gpt2")
    ref_ids, ref_off = ref_c.RefC(obj).encode_packed(text, off)
    with _env("CTOK_MID_PACKED", arm):
        tok = Tokenizer.from_str(json.dumps(obj))
        ids, toff = tok.encode_packed(text, off, timing=True)
        st = tok.last_stats
    assert_same(ids, toff, ref_ids, ref_off)
    assert st["class_bytes"][2] == 0 and st["class_ids"][2] == 0


@pytest.fixture(scope="module")
def sparse_case(objs):
    """~1.2 MB of " ab" filler (more than 300 tiles) with one 17..32 B word about every 50 tiles."""
    rng = random.Random(11)
    n_tiles, every = 310, 50
    words, parts, pos = [], [], 0
    for k in range(n_tiles // every + 1):
        n = 17 + (5 * k) % 16
        word = " " + "".join(rng.choice("etaoinshrdlu") for _ in range(n - 1))
        target = k * every * TILE + rng.randrange(8, TILE - 40)
        target -= (target - pos) % 3  # (whole " ab" fillers: the word keeps its leading space)
        parts.append((" ab" * (target - pos))[:target - pos])
        parts.append(word)
        words.append(word)
        pos = target + n
    end = n_tiles * TILE
    parts.append((" ab" * (end - pos))[:end - pos])
    doc = "".join(parts)
    obj = objs("gpt2")
    ref = ref_c.RefC(obj)
    text, off = corpus.pack([doc.encode()])
    ref_ids, ref_off = ref.encode_packed(text, off)
    # what the class holds, on the oracle's side: the pieces of 17..32 B and the ids of each
    c2 = [p for p in ref_c.pieces(doc.encode()) if 17 <= len(p) <= 32]
    assert len(c2) == len(words) >= 6 and [p.decode() for p in c2] == words
    wt, wo = corpus.pack(c2)
    word_ids, _ = ref.encode_packed(wt, wo)
    return json.dumps(obj), text, off, ref_ids, ref_off, sum(map(len, c2)), len(word_ids)


@pytest.mark.parametrize("arm", ARMS, ids=ARM_IDS)
def test_sparse_class_chunks(sparse_case, arm):
    """Multi-unit chunks with most tiles empty neither lose nor duplicate a piece."""
    js, text, off, ref_ids, ref_off, want_bytes, want_ids = sparse_case
    assert len(text) >= 300 * TILE
    with _env("CTOK_MID_PACKED", arm):
        tok = Tokenizer.from_str(js)
        ids, toff = tok.encode_packed(text, off, timing=True)
        st = tok.last_stats
    assert_same(ids, toff, ref_ids, ref_off)
    assert st["class_bytes"][2] == want_bytes and st["class_ids"][2] == want_ids


@pytest.mark.parametrize("arm", ["1", "2"], ids=["packed_mid", "packed_fold"])
def test_two_calls_same_output(cases, arm):
    """No state of one piece or call leaks into the next: two calls on one tokenizer agree (and
    with the oracle)."""
    js, docs, text, off, ref_ids, ref_off = cases("gpt2")
    with _env("CTOK_MID_PACKED", arm):
        tok = Tokenizer.from_str(js)
        a_ids, a_off = tok.encode_packed(text, off)
        b_ids, b_off = tok.encode_packed(text, off)
    assert tok.table_props["dev_mid_packed"] == int(arm)
    assert np.array_equal(a_ids, b_ids) and np.array_equal(a_off, b_off)
    assert_same(b_ids, b_off, ref_ids, ref_off)
