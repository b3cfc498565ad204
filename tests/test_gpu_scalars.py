"""The fused encode path (Tokenizer.encode_packed: k_segment's code point classes and NFC flags,
the NFC splice, k_nfc_check, k_norm / nfc_doc) over every Unicode scalar, at 64-byte word and tile
edges, and over NFC scenarios laid out against nfc_doc's 64-byte windows.

Inputs and expectations come from tests/scalar_cases.py; tests/test_scalar_cases_cpu.py ties the
closed-form expectations to the C oracle, so the large tests here need no oracle run.  The three
modes are the three ways the flag and NFC code can run:

* "splice": the default (k_segment flags 64-byte words, the flagged documents are normalised and
  encoded again as a sub-batch and spliced in);
* "rerun":  CTOK_NFC_RERUN=1 (a flag makes the whole batch run again behind k_nfc_check + k_norm);
* "prefix": add_prefix_space, no speculation (k_nfc_check, then k_norm with the prefix space).
"""
import functools
import json

import numpy as np
import pytest

from complexity_tokenizer import Tokenizer
from oracle import ref_c
from tests import scalar_cases as sc

pytestmark = pytest.mark.gpu

MODES = ["splice", "rerun", "prefix"]


def _tok(obj_fn, mode, monkeypatch):
    if mode == "rerun":
        monkeypatch.setenv("CTOK_NFC_RERUN", "1")
    return Tokenizer.from_str(json.dumps(obj_fn(mode == "prefix")))


def _doc_of(off, i):
    return int(np.searchsorted(off, i, side="right")) - 1


def assert_same(got, want, text, off):
    """ids and tok_off equal; on a difference, the first differing document and its bytes."""
    (gi, go), (wi, wo) = got, want
    assert len(go) == len(wo)
    if np.array_equal(go, wo) and np.array_equal(gi, wi):
        return
    bad = np.flatnonzero(go != wo)
    d = int(bad[0]) - 1 if len(bad) else len(wo)
    n = min(len(gi), len(wi))
    diff = np.flatnonzero(gi[:n] != wi[:n])
    if len(diff):
        d = min(d, _doc_of(wo, int(diff[0])))
    raw = bytes(text[int(off[d]):int(off[d + 1])])
    raise AssertionError("doc %d %r differs: gpu %s want %s" % (
        d, raw, gi[int(go[d]):int(go[d + 1])].tolist(), wi[int(wo[d]):int(wo[d + 1])].tolist()))


@functools.lru_cache(None)
def _px(which, aps):
    """(text, off, ids, tok_off) of the documents P + X over "all" / "inert" scalars (shared, read-only)."""
    cps = sc.scalars() if which == "all" else sc.inert_scalars()
    text, off = sc.px_docs(cps)
    ids, tok_off = sc.expected(cps, add_prefix_space=aps)
    return text, off, ids, tok_off


@pytest.mark.parametrize("mode", MODES)
def test_every_scalar(mode, monkeypatch):
    """The four documents P + X for all 1,112,064 scalars X (4,448,256 documents, 22 MB) in one
    call per mode, "prefix" included (the whole set, not the subset), against the closed-form
    rule: the class and the NFC flag the device gives every code point, through cp_range_class,
    cls_bmp and the two-level tables."""
    tok = _tok(sc.probe_obj, mode, monkeypatch)
    text, off, ids, tok_off = _px("all", mode == "prefix")
    got = tok.encode_packed(text, off, timing=True)
    n = tok.last_stats["nfc_docs"]
    print("test_every_scalar[%s]: nfc_docs %d" % (mode, n))
    assert_same(got, (ids, tok_off), text, off)
    if mode == "splice":
        assert n >= 4 * 2060  # flagged by 64-byte word: the neighbours in the word come along
    else:
        assert n == 4 * 2060  # k_nfc_check flags the document of the code point's own byte


@pytest.mark.parametrize("mode", ["splice", "rerun"])
def test_inert_scalars_flag_nothing(mode, monkeypatch):
    """The same documents over the 1,110,004 unflagged scalars: no document is flagged (a false
    flag costs a splice or a whole second run), and the ids are the raw bytes with the rule's merges."""
    tok = _tok(sc.probe_obj, mode, monkeypatch)
    text, off, ids, tok_off = _px("inert", False)
    got = tok.encode_packed(text, off, timing=True)
    assert tok.last_stats["nfc_docs"] == 0
    assert_same(got, (ids, tok_off), text, off)


def _probe2(aps):
    return sc.probe_obj(aps, suffixes=True)


@functools.lru_cache(None)
def _words(lead_bytes, suffix=False):
    """(text, off, oracle ids, oracle tok_off, flagged documents) of the 64-byte documents over the
    subset, flagged and unflagged alternating, behind lead_bytes of "x"."""
    cps = sc.alternating(sc.subset())
    text, off = sc.word_docs(cps, lead_bytes=lead_bytes, suffix=suffix)
    ids, tok_off = ref_c.RefC(_probe2(False)).encode_packed(text, off)
    return text, off, ids, tok_off, 4 * int(sc.flags()[cps].sum())


def test_flag_lands_on_its_own_word(monkeypatch):
    """64-byte documents P + X + "x"..., one per 64-byte word from byte 0 on, flagged and unflagged
    X alternating: a document is flagged by the words it overlaps (nfc.hip k_flag_docs) and every
    document is one word here, so exactly the documents that hold a flagged scalar are normalised."""
    tok = _tok(_probe2, "splice", monkeypatch)
    text, off, ids, tok_off, n_flagged = _words(0)
    assert n_flagged == 4 * 2060 and np.all(off[:-1] % 64 == 0)
    got = tok.encode_packed(text, off, timing=True)
    assert_same(got, (ids, tok_off), text, off)
    assert tok.last_stats["nfc_docs"] == n_flagged


@pytest.mark.parametrize("mode", ["splice", "rerun"])
@pytest.mark.parametrize("tail", ["x", "suffix"])
@pytest.mark.parametrize("s", [0, 1, 2, 3])
def test_word_straddle(s, tail, mode, monkeypatch):
    """The same documents behind one document of 63 - s bytes: every P sits at word offset 63 - s
    and every X's lead byte at 64 - s, so s = 1, 2, 3 send every multi-byte X through k_segment's
    lead_cont route with the lead 1, 2, 3 bytes back, and s = 0 puts P and X into different words.
    lead_cont classes only X's bytes in the second word, which the (P, lead) merges cannot show:
    tail "suffix" puts SUFFIXES[pi] behind X, whose merge with X's last byte does (a mutant with
    back = 2 for 3 passed the "x" documents and fails these)."""
    tok = _tok(_probe2, mode, monkeypatch)
    text, off, ids, tok_off, n_flagged = _words(63 - s, tail == "suffix")
    got = tok.encode_packed(text, off, timing=True)
    assert_same(got, (ids, tok_off), text, off)
    assert tok.last_stats["nfc_docs"] >= n_flagged


@functools.lru_cache(None)
def _tiles():
    docs, _ = sc.tile_edge_docs()
    text, off = sc.pack(docs)
    return (text, off) + tuple(ref_c.RefC(_probe2(False)).encode_packed(text, off))


@pytest.mark.parametrize("mode", ["splice", "rerun"])
def test_tile_edges(mode, monkeypatch):
    """One scalar per (class, UTF-8 length, flagged or not), behind each prefix, with its lead byte
    1, 2 and 3 bytes before a tile's end (3,968 bytes), inside a document and as a document's last
    character, without and with the suffix behind it: the code point runs from the tile's last word
    into the look-ahead word, which the next tile reads as its context word with the bytes before
    it (s_all[-1])."""
    tok = _tok(_probe2, mode, monkeypatch)
    text, off, ids, tok_off = _tiles()
    got = tok.encode_packed(text, off, timing=True)
    assert_same(got, (ids, tok_off), text, off)
    assert tok.last_stats["nfc_docs"] > 0


@functools.lru_cache(None)
def _windows(aps):
    docs = sc.nfc_window_docs()
    return sc.nfc_expected(docs, add_prefix_space=aps) + (sum(map(sc.has_flagged, docs)),)


@pytest.mark.parametrize("mode", MODES)
def test_nfc_windows(mode, monkeypatch):
    """Every NFC scenario of scalar_cases.nfc_scenarios (every decomposable scalar and its NFD,
    every two-part pair with the composition exclusions and the 4-byte pairs, Hangul L V T, every
    ordered pair of combining classes, expansion runs that grow a document 3x, mark runs of 64 and
    256) under every layout of nfc_window_docs (against nfc_doc's 64-byte windows), one call per
    mode on the no-merge byte tokenizer: the ids are the bytes of `unicodedata`'s NFC."""
    tok = _tok(sc.bytes_obj, mode, monkeypatch)
    text, off, ids, tok_off, n_flagged = _windows(mode == "prefix")
    got = tok.encode_packed(text, off, timing=True)
    assert_same(got, (ids, tok_off), text, off)
    if mode == "splice":
        assert tok.last_stats["nfc_docs"] >= n_flagged
    else:
        assert tok.last_stats["nfc_docs"] == n_flagged
