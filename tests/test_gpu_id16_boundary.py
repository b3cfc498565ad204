"""Every 16-bit id path at the 0xFFFE / 0xFFFF vocabulary boundary, against the C oracle.

The host narrows ids to 16 bits where the largest model-vocab id is below 0xFFFF (`narrow`: the
key16 merge tables, the NARROW merge passes, u16 piece records; `short_packed`: the packed u16-pair
16-slot tier; `ids16`: the u16 wire of the host-buffer pipeline), with 0xFFFF as the sentinel of
each.  The tables here are prefixes of the llama3_128k fixture with 65,534 .. 65,537 ids
(toys.truncated): the first two are narrow, with id 0xFFFE legal in the second, the last two are
not.  The corpus (tests/id16_cases.py) sends the highest ids of each table through pieces of every
length class; the oracle's output is checked for that before anything is compared with it.  Which
variant ran is read from Tokenizer.table_props and asserted in every arm.
"""
import json
import os

import numpy as np
import pytest

from complexity_tokenizer import PanicException, Tokenizer
from datagen import corpus
from oracle import ref_c, ref_py
from tests import encoding_cases, id16_cases, toys
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

FLIP = 65535  # the largest narrow table: id 0xFFFE exists
SWITCHES = ("CTOK_SHORT_PACKED", "CTOK_FORCE_WIDE_SLOTS", "CTOK_FORCE_WIDE", "CTOK_WIRE32", "CTOK_C3_SPARSE")


class _env:
    """The given switches for the duration of a block, every other switch of SWITCHES unset."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in SWITCHES}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in self.old.items() if v is not None})


def make(obj, **env):
    """A tokenizer made under the switches, its device tables included (they are made by the first
    call, which is where CTOK_FORCE_WIDE_SLOTS and CTOK_SHORT_PACKED are read)."""
    with _env(**env):
        tok = Tokenizer.from_str(json.dumps(obj))
        tok.encode("a b")
    return tok


def run(tok, batch, **env):
    with _env(**env):
        out = tok.encode_packed(*batch, timing=True)
    return out


def props(tok, *keys):
    p = tok.table_props
    return tuple(p[k] for k in keys)


LOADED = ("narrow", "compact", "short_packed", "ids16")
BUILT = ("dev_narrow", "dev_short_packed")
LAST = ("last_rec16", "last_wire16")


@pytest.fixture(scope="module")
def tables(llama3_path):
    with open(llama3_path) as f:
        base = json.load(f)
    return {n: toys.truncated(base, n) for n in id16_cases.N_IDS}


@pytest.fixture(scope="module")
def corpora(tables):
    """n_ids -> (docs, packed batch, oracle ids, oracle offsets): the table's top texts alone (one
    id each, by the whole-piece record), its boundary words, the tile-end document and an
    ordinary-text sample.  The oracle's output must hold the top ids in every length class."""
    c3 = [d.decode() for d in corpus.unpack(*corpus.corpus_c3(2000, seed=3))]
    out = {}
    for n, obj in tables.items():
        tops = id16_cases.top_texts(obj)
        words = id16_cases.boundary_docs(obj)
        docs = tops + words + [id16_cases.tile_end_doc(obj)] + c3
        batch = corpus.pack([d.encode() for d in docs])
        ids, off = ref_c.RefC(obj).encode_packed(*batch)
        assert int(ids.max()) == n - 1
        # each top text is its own single id
        o = off.tolist()
        assert [ids[o[k]:o[k + 1]].tolist() for k in range(len(tops))] == [[n - 1 - k] for k in range(len(tops))]
        w0 = len(tops)
        wids, woff = ids[o[w0]:o[w0 + len(words)]], off[w0:w0 + len(words) + 1] - off[w0]
        top, near = id16_cases.class_counts(words, wids, woff, n)
        for c, name in enumerate(id16_cases.CLASSES):
            assert near[c] >= 100, (n, name, near)
            # (a multi-token piece of the class can hold the top id only if the top token's text
            # leaves room for one more byte: not so for the <= 8 B class of the 65,536-id table,
            # whose top token has 8 bytes)
            room = len(tops[0].encode()) + 1 <= (8, 16, 32, 64, 1 << 30)[c]
            assert top[c] >= 1 or not room, (n, name, top)
        if n == FLIP:
            assert min(top) >= 1, top
        out[n] = (docs, batch, ids, off)
    return out


@pytest.fixture(scope="module")
def flip_tok(tables):
    return make(tables[FLIP])


@pytest.mark.parametrize("n_ids", id16_cases.N_IDS)
def test_tables_around_the_flip(tables, corpora, n_ids):
    narrow = n_ids <= 0xFFFF
    tok = make(tables[n_ids])
    assert props(tok, *LOADED) == (narrow, True, narrow, narrow)
    assert props(tok, *BUILT) == (narrow,) * 2
    _, batch, ref_ids, ref_off = corpora[n_ids]
    ids, off = run(tok, batch)
    st = tok.last_stats
    assert props(tok, *LAST) == (narrow,) * 2
    assert_same(ids, off, ref_ids, ref_off)
    # every merge pass did part of the work
    assert all(st["class_bytes"][c] > 0 and st["class_ids"][c] > 0 for c in range(4)), st
    assert st["long_pieces"] > 0


def test_flip_tables_differ_only_by_the_last_merge(tables, corpora, flip_tok):
    """The 65,536-id table's own corpus (the text of id 0xFFFF among its words) through the
    65,535-id table: that table lacks only the last merge in rank, so its output is the wider
    table's with id 0xFFFF taken apart into that merge's two parts.  (u16 everywhere on one side,
    u32 on the other.)"""
    _, batch, ids36, off36 = corpora[FLIP + 1]
    a, b = tables[FLIP + 1]["model"]["merges"][-1]
    vocab = tables[FLIP + 1]["model"]["vocab"]
    assert vocab[a + b] == FLIP
    parts = np.array([vocab[a], vocab[b]], dtype=np.uint32)
    hit = ids36 == FLIP
    assert hit.sum() >= 20
    want = np.repeat(ids36, np.where(hit, 2, 1))
    pos = np.flatnonzero(want == FLIP)
    want[pos[0::2]], want[pos[1::2]] = parts[0], parts[1]
    want_off = np.concatenate([[0], np.cumsum(np.where(hit, 2, 1))])[off36.astype(np.int64)].astype(np.uint64)
    ids35, off35 = run(flip_tok, batch)
    assert props(flip_tok, *LAST) == (True, True)
    assert_same(ids35, off35, want, want_off)


ARMS = {
    # switches, then dev_narrow, dev_short_packed, compact
    "default": ({}, True, True, True),
    "packed_off": ({"CTOK_SHORT_PACKED": "0"}, True, False, True),
    "wide_slots": ({"CTOK_FORCE_WIDE_SLOTS": "1"}, False, False, True),
    "wide_values": ({"CTOK_FORCE_WIDE": "1"}, True, False, False),
}


@pytest.mark.parametrize("arm", sorted(ARMS))
def test_variant_arms_on_the_flip_table(tables, corpora, arm):
    env, dev_narrow, dev_packed, compact = ARMS[arm]
    tok = make(tables[FLIP], **env)
    assert props(tok, *LOADED) == (True, compact, compact, True)
    assert props(tok, *BUILT) == (dev_narrow, dev_packed)
    _, batch, ref_ids, ref_off = corpora[FLIP]
    ids, off = run(tok, batch)
    # the piece records and the wire follow the vocabulary, not the slot or value switches
    assert props(tok, *LAST) == (True, True)
    assert_same(ids, off, ref_ids, ref_off)


@pytest.mark.parametrize("bound", ["0", "100000000"], ids=["c3_register", "c3_sparse"])
def test_class3_paths_on_the_flip_table(flip_tok, corpora, bound):
    """The 33..64 B class by the register pass and by the sparse path (CTOK_C3_SPARSE, read per
    call): both have a NARROW instance."""
    _, batch, ref_ids, ref_off = corpora[FLIP]
    ids, off = run(flip_tok, batch, CTOK_C3_SPARSE=bound)
    assert_same(ids, off, ref_ids, ref_off)
    assert flip_tok.last_stats["class_ids"][3] > 0


def test_flip_table_vs_python_oracle(tables, corpora, flip_tok):
    docs, _, ref_ids, ref_off = corpora[FLIP]
    py = ref_py.RefTokenizer(tables[FLIP])
    k0 = id16_cases.TOP_K
    pick = docs[:k0] + docs[k0:k0 + 64 * len(id16_cases.SUFFIX_LENS):3]
    want = [py.encode(d) for d in pick]
    assert max(map(max, want)) == FLIP - 1
    assert flip_tok.encode_batch(pick) == want


@pytest.mark.parametrize("how", ["shuffled", "last_two_swapped"])
def test_rank_valued_narrow_tables(tables, corpora, how):
    """Narrow tables whose values are ranks (not compact), so the register tier of the 9..16 B
    pass: every merge shuffled (the top ids' own merges rarely complete: ids up to about 0xFFFB),
    and only the last two merges swapped (id 0xFFFE merges as in the compact table)."""
    obj = toys.shuffled_merges(tables[FLIP], seed=16) if how == "shuffled" else toys.swapped_last_merges(tables[FLIP])
    tok = make(obj)
    assert props(tok, *LOADED) == (True, False, False, True)
    assert props(tok, *BUILT) == (True, False)
    _, batch, _, _ = corpora[FLIP]
    ref_ids, ref_off = ref_c.RefC(obj).encode_packed(*batch)
    assert (ref_ids >= FLIP - 64).sum() >= 100
    if how == "last_two_swapped":
        assert (ref_ids == FLIP - 1).sum() >= 20
    assert_same(*run(tok, batch), ref_ids, ref_off)
    assert props(tok, *LAST) == (True, True)


def test_narrow_table_with_panicking_values(tables, corpora):
    """Invalid merges shift the ranks (src/bpe.rs:60-69): values past the valid list panic when
    used, so the packed tier is not taken.  The top ids' merges are the shifted-out ones: the whole
    corpus panics (in the oracle, so here); the documents that do not, by the oracle one by one,
    are compared id by id, and still reach id 0xFFFE."""
    obj = toys.with_invalid_merges(tables[FLIP], seed=0, n_bad=30)
    tok, rc = make(obj), ref_c.RefC(obj)
    assert props(tok, *LOADED) == (True, True, False, True)
    assert props(tok, *BUILT) == (True, False)
    docs, batch, _, _ = corpora[FLIP]
    with pytest.raises(ref_py.PanicException):
        rc.encode_packed(*batch)
    with pytest.raises(PanicException):
        run(tok, batch)
    quiet = []
    for d in docs[:id16_cases.TOP_K + 64 * len(id16_cases.SUFFIX_LENS) * 6]:
        try:
            rc.encode_batch([d], threads=1)
            quiet.append(d)
        except ref_py.PanicException:
            pass
    assert len(quiet) >= 2000
    batch = corpus.pack([d.encode() for d in quiet])
    ref_ids, ref_off = rc.encode_packed(*batch)
    assert (ref_ids == FLIP - 1).sum() >= 20 and (ref_ids >= FLIP - 64).sum() >= 100
    assert_same(*run(tok, batch), ref_ids, ref_off)
    assert props(tok, *LAST) == (True, True)


@pytest.fixture(scope="module")
def added(tables, corpora):
    """The flip table plus in-piece added tokens with ids 65,535, 65,536 and 70,000: `narrow`
    (piece records u16: they hold vocabulary ids only) without `ids16`."""
    obj = id16_cases.with_added_ids(tables[FLIP])
    docs = corpora[FLIP][0]
    k0 = id16_cases.TOP_K
    n_words = 64 * len(id16_cases.SUFFIX_LENS) * 6
    docs = docs[:k0] + id16_cases.spliced_docs(docs[k0:k0 + n_words]) + docs[k0 + n_words:][:200]
    batch = corpus.pack([d.encode() for d in docs])
    ids, off = ref_c.RefC(obj).encode_packed(*batch)
    for i in id16_cases.ADDED_IDS.values():
        assert (ids == i).sum() >= 100, i
    assert (ids == FLIP - 1).sum() >= 20
    return obj, docs, batch, ids, off


def test_added_ids_past_16_bits_on_a_narrow_table(added):
    obj, docs, batch, ref_ids, ref_off = added
    tok = make(obj)
    assert tok.num_piece_added_tokens() == 3
    assert props(tok, *LOADED) == (True, True, True, False)
    ids, off = run(tok, batch)
    assert props(tok, *LAST) == (True, False)
    assert_same(ids, off, ref_ids, ref_off)
    # the list-of-strings entry points
    o = ref_off.tolist()
    half = len(docs) // 2
    assert tok.encode_batch(docs[half - 300:half + 300]) == [ref_ids[o[k]:o[k + 1]].tolist() for k in range(half - 300, half + 300)]
    fids, foff = tok.encode_batch_flat(docs)
    assert_same(fids, foff, ref_ids, ref_off)
    assert int(fids.max()) == 70000
    py = ref_py.RefTokenizer(obj)
    for k in range(id16_cases.TOP_K, id16_cases.TOP_K + 330, 3):
        assert ids[o[k]:o[k + 1]].tolist() == py.encode(docs[k]), docs[k]


def test_added_ids_below_16_bits_keep_the_u16_wire(tables, corpora):
    """The 65,534-id table with in-piece added tokens 65,534 (0xFFFE: u16 wire) and, in a second
    tokenizer, 65,535 (the sentinel's value: u32 wire)."""
    docs = corpora[FLIP - 1][0]
    k0 = id16_cases.TOP_K
    docs = id16_cases.spliced_docs(docs[k0:k0 + 1500])
    batch = corpus.pack([d.encode() for d in docs])
    for top_added, ids16 in ((0xFFFE, True), (0xFFFF, False)):
        obj = id16_cases.with_added_ids(tables[FLIP - 1], {"ing": top_added, "ll": 0xFFFD, "zz": 300})
        tok = make(obj)
        assert props(tok, *LOADED) == (True, True, True, ids16)
        ref_ids, ref_off = ref_c.RefC(obj).encode_packed(*batch)
        assert (ref_ids == top_added).sum() >= 50
        assert_same(*run(tok, batch), ref_ids, ref_off)
        assert props(tok, *LAST) == (True, ids16)


@pytest.mark.parametrize("rem", [0, 1, 7, "tiny"])
def test_u16_wire_body_and_tail(tables, corpora, flip_tok, rem):
    """k_wire16 packs 8 ids per thread and finishes with a tail: token counts of each remainder,
    and fewer than 8 tokens, with id 0xFFFE last (in the tail) and inside the body; the same
    through the u32 wire (CTOK_WIRE32, read per call)."""
    docs = corpora[FLIP][0]
    top = docs[0]  # the text of id 0xFFFE
    rc = ref_c.RefC(tables[FLIP])
    if rem == "tiny":
        pick = ["e", top]
    else:
        pick = docs[id16_cases.TOP_K:id16_cases.TOP_K + 1000]
        n = len(rc.encode_packed(*corpus.pack([d.encode() for d in pick]))[0])
        pick = pick + ["e"] * ((rem - n - 1) % 8) + [top]
    batch = corpus.pack([d.encode() for d in pick])
    ref_ids, ref_off = rc.encode_packed(*batch)
    if rem == "tiny":
        assert len(ref_ids) < 8
    else:
        assert len(ref_ids) % 8 == rem and (ref_ids[:-8] == FLIP - 1).any()
    assert int(ref_ids[-1]) == FLIP - 1
    for wire32 in (False, True):
        with _env(**({"CTOK_WIRE32": "1"} if wire32 else {})):
            ids, off = flip_tok.encode_batch_flat(pick)
        assert props(flip_tok, *LAST) == (True, not wire32)
        assert_same(ids, off, ref_ids, ref_off)


@pytest.mark.parametrize("n_ids", id16_cases.N_IDS)
def test_decode_round_trip_at_the_boundary(tables, corpora, n_ids):
    """decode_batch of the oracle's ids against the oracle's decode, with ids 65,533 .. 65,536 and
    70,000 among them whether or not the table (or an added token) has them."""
    obj = id16_cases.with_added_ids(tables[n_ids], {"ing": n_ids, "zz": 70000})
    tok, rc = Tokenizer.from_str(json.dumps(obj)), ref_c.RefC(obj)
    docs, _, ref_ids, ref_off = corpora[n_ids]
    o = ref_off.tolist()
    k0 = id16_cases.TOP_K
    batch = [ref_ids[o[k]:o[k + 1]].tolist() for k in list(range(k0)) + list(range(k0, k0 + 900, 3))]
    batch += [[65533, 65534, 65535, 65536, 70000], [n_ids - 1], [n_ids], [70000, 104, 65535, 65534]]
    for skip, clean in ((False, False), (False, True)):
        got = tok.decode_batch_with_options(batch, skip, clean)
        assert got == rc.decode_batch(batch, skip, clean)
    raw = tok.decode_batch_with_options(batch[:k0], False, False)
    assert raw == docs[:k0]  # the top ids' own texts


def test_encode_padded_on_the_flip_table(tables, corpora):
    """One padded encode with a post-processor whose special ids start at 0xFFFF (they cannot occur
    inside a piece: the table stays narrow and ids16), against the Python model of Encoding."""
    obj = encoding_cases.with_post_processor(tables[FLIP], "template")
    tok, ref = make(obj), ref_py.RefTokenizer(obj)
    assert props(tok, *LOADED) == (True, True, True, True)
    docs = corpora[FLIP][0]
    k0 = id16_cases.TOP_K
    ts = docs[:8] + [d for d in docs[k0:k0 + 64 * len(id16_cases.SUFFIX_LENS)] if len(d) < 100][::4]
    r = tok.encode_padded(ts, padding="longest")
    assert props(tok, "last_rec16") == (True,)
    want = [ref.encode_to_encoding(t) for t in ts]
    assert max(max(e.ids) for e in want) >= 0xFFFF and any(FLIP - 1 in e.ids for e in want)
    target = max(len(e.ids) for e in want)
    pid, ptok = ref.pad_id_token()
    for e in want:
        e.pad(target, pid, ptok, False)
    for i, e in enumerate(want):
        L = int(r["row_len"][i])
        assert L == len(e.ids)
        assert r["input_ids"][i, :L].tolist() == e.ids
        assert r["attention_mask"][i, :L].tolist() == e.attention_mask
        assert r["token_type_ids"][i, :L].tolist() == e.type_ids
        assert r["special_tokens_mask"][i, :L].tolist() == e.special_tokens_mask
