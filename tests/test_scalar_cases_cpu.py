"""tests/scalar_cases.py against the C oracle (CPU only): the expectations that
tests/test_gpu_scalars.py uses without the oracle are tied to it here.

* The closed-form rule (scalar_cases.expected) equals the C oracle's ids for the documents P + X
  of every Unicode scalar X and the four prefixes; with add_prefix_space on the subset.
* The counts the GPU tests rely on: 2,060 flagged scalars, 3,440 run edges, 23,239 scalars in the
  subset, and the merged first tokens per prefix.
* Every NFC-window document: the oracle's ids on the no-merge byte tokenizer are the bytes of
  `unicodedata`'s NFC (behind the prefix space in the add_prefix_space twin).
"""
import unicodedata

import numpy as np
import pytest

from oracle import ref_c
from tests import scalar_cases as sc


def _same(got, want):
    (gi, go), (wi, wo) = got, want
    assert np.array_equal(go, wo), "tok_off differs first at doc %d" % (int(np.flatnonzero(go != wo)[0]) - 1)
    assert np.array_equal(gi, wi), "ids differ first at %d" % int(np.flatnonzero(gi != wi)[0])


def test_counts():
    assert unicodedata.unidata_version == "13.0.0"
    assert len(sc.scalars()) == 1_112_064
    assert len(sc.flagged_scalars()) == 2060 and len(sc.inert_scalars()) == 1_110_004
    assert len(sc.run_edges()) == 3440
    assert len(sc.subset()) == 23_239
    f = sc.flags()
    changing = sum(1 for cp in sc.flagged_scalars().tolist() if unicodedata.normalize("NFC", chr(cp)) != chr(cp))
    marks = sum(1 for cp in sc.flagged_scalars().tolist() if unicodedata.combining(chr(cp)))
    assert (changing, marks) == (1120, 872)
    assert not f[0xD800:0xE000].any()


def test_rule_equals_oracle_for_every_scalar():
    cps = sc.scalars()
    text, off = sc.px_docs(cps)
    assert len(off) - 1 == 4_448_256 and int(off[-1]) == 21_978_624
    want = sc.expected(cps)
    assert len(want[0]) == 20_865_803
    assert sc.merged_counts(want[0]) == [145_619, 1_914, 964_381, 19]
    _same(ref_c.RefC(sc.probe_obj()).encode_packed(text, off), want)
    # ids decode back to the bytes of NFC(doc): spot-checked through the scalar rule on the flagged ones
    for pi in range(4):
        for cp in sc.flagged_scalars().tolist()[::7]:
            doc = sc.PREFIXES[pi].decode() + chr(cp)
            ids = sc.rule_ids(doc, pi)
            raw = []
            for i in ids:
                raw += [i] if i < 256 else [sc.PREFIXES[(i - 256) // sc.N_LEADS][0], sc.LEAD0 + (i - 256) % sc.N_LEADS]
            assert bytes(raw) == unicodedata.normalize("NFC", doc).encode()


def test_rule_equals_oracle_with_prefix_space_on_the_subset():
    cps = sc.subset()
    text, off = sc.px_docs(cps)
    assert len(off) - 1 == 92_956
    _same(ref_c.RefC(sc.probe_obj(True)).encode_packed(text, off), sc.expected(cps, add_prefix_space=True))


def test_rule_vectorised_equals_rule_per_document():
    cps = sc.subset()
    for aps in (False, True):
        ids, off = sc.expected(cps, add_prefix_space=aps)
        flat = [i for pi in range(4) for cp in cps.tolist()
                for i in sc.rule_ids(sc.PREFIXES[pi].decode() + chr(cp), pi, aps)]
        assert ids.tolist() == flat


@pytest.mark.parametrize("aps", [False, True])
def test_nfc_window_documents_round_trip(aps):
    docs = sc.nfc_window_docs()
    text, off, want, woff = sc.nfc_expected(docs, add_prefix_space=aps)
    _same(ref_c.RefC(sc.bytes_obj(aps)).encode_packed(text, off), (want, woff))


def test_nfc_scenarios_hold_what_they_should():
    scen = [s for _, s in sc.nfc_scenarios()]
    have = set(scen)
    assert "\U00011099\U000110ba" in have and "\U00011935\U00011930" in have  # 4-byte pairs
    assert "\u0915\u093c" in have and "\u0958" in have  # a composition exclusion: the pair stays, U+0958 expands
    assert "\U0001d160" * 40 in have                                            # 4 -> 12 bytes
    assert sum(1 for s in scen if len(s) == 2 and 0x1100 <= ord(s[0]) < 0x1113 and 0x1161 <= ord(s[1]) < 0x1176) >= 399
    assert max(len(s) for s in scen) == 257  # no mark run longer than 256
    docs = sc.nfc_window_docs()
    grow = max(len(unicodedata.normalize("NFC", d).encode()) / len(d.encode()) for d in docs)
    assert 2.5 < grow <= 3.0


def test_layouts_are_where_they_should_be():
    # one-word documents: 64 bytes each, flagged and unflagged alternating
    cps = sc.alternating(sc.subset())
    f = sc.flags()[cps]
    assert f[0:4120:2].all() and not f[1:4120:2].any()
    text, off = sc.word_docs(cps[:100], prefixes=[0])
    assert np.array_equal(np.diff(off.astype(np.int64)), np.full(100, 64))
    # straddles: P at word offset 63 - s, X's lead byte at 64 - s
    for s in range(4):
        text, off = sc.word_docs(cps[:50], lead_bytes=63 - s)
        assert int(off[1]) == 63 - s and all(int(o) % 64 == 63 - s for o in off[1:-1])
        assert bytes(text[int(off[1]):int(off[1]) + 1]) == b"a"
    # tile edges: every placed lead byte lies 1..3 bytes before a tile edge
    docs, placed = sc.tile_edge_docs()
    blob = b"".join(docs)
    assert len(blob) % (3 * sc.TILE) == 0
    for lead, cp in placed:
        x = chr(cp).encode()
        assert blob[lead:lead + len(x)] == x and sc.TILE - lead % sc.TILE in (1, 2, 3)
        assert blob[lead - 1:lead] in sc.PREFIXES
    reps = sc.tile_representatives()
    assert len(placed) == len(reps) * 4 * 3 * 4 * 2
    assert {len(chr(c).encode()) for c in reps.tolist()} == {2, 3, 4}


def test_suffix_merges_show_the_class_of_the_last_byte():
    """In the suffix documents P + X + S + "x"... the oracle merges X's last byte with S exactly
    when X is non-ASCII and of the prefix's class (unflagged X: NFC leaves the document alone), as
    it merges P with X's lead byte: the suffix probe shows what the prefix probe cannot."""
    cps = sc.inert_scalars()
    cps = cps[np.isin(cps, sc.subset())]
    text, off = sc.word_docs(cps, suffix=True)
    ids, tok_off = ref_c.RefC(sc.probe_obj(suffixes=True)).encode_packed(text, off)
    doc = np.searchsorted(tok_off, np.arange(len(ids)), side="right") - 1
    pre = np.zeros(len(tok_off) - 1, dtype=bool)
    suf = np.zeros(len(tok_off) - 1, dtype=bool)
    pre[doc[(ids >= 256) & (ids < sc.SUFFIX_ID0)]] = True
    suf[doc[ids >= sc.SUFFIX_ID0]] = True
    want = np.concatenate([(cps >= 0x80) & (sc.classes()[cps] == pi) for pi in range(4)])
    assert np.array_equal(pre, want) and np.array_equal(suf, want) and want.sum() > 5000
    obj = sc.probe_obj(suffixes=True)
    assert len(obj["model"]["vocab"]) == 460 + 256 and len(obj["model"]["merges"]) == 204 + 256
    assert len(sc.probe_obj()["model"]["vocab"]) == 460 and len(sc.probe_obj()["model"]["merges"]) == 204
