"""The inputs of tests/text_tail_cases.py are what they claim (CPU only), by the Python oracle: the
text the pipeline runs on has B bytes, it ends in the claimed last piece of the claimed class, and
the poisoned tails are live -- encoding text + tail as one text changes the tokens of the last piece --
so a kernel that looked past the end of the text would give other ids than the oracle's.  And what
the entry points refuse before they touch a device is refused on a host without one."""
import ctypes
import json

import numpy as np
import pytest

from complexity_tokenizer import Tokenizer
from complexity_tokenizer import _native as _n
from tests import text_tail_cases as ttc


@pytest.fixture(scope="module")
def base(gpt2_path):
    with open(gpt2_path) as f:
        return json.load(f)


@pytest.fixture(scope="module", params=ttc.VARIANTS)
def world(request, base):
    """(variant, oracle, cases, {(case name, tail): live})"""
    orc = ttc.Oracle(ttc.variant_json(base, request.param))
    cs = ttc.cases(request.param)
    live = {(c["name"], t): orc.live(c["text"], t) for c in cs for t in ttc.TEXT_TAILS}
    return request.param, orc, cs, live


def test_tile_size_is_read_from_the_code():
    assert ttc.TILE % 64 == 0 and ttc.TILE > 1024
    with open(ttc.CSRC + "/ctok_internal.h") as f:
        assert "constexpr int kTile = kTileWords * 64;  // %d bytes" % ttc.TILE in f.read()


def test_texts_end_in_the_claimed_piece_at_the_claimed_length(world):
    variant, orc, cs, _ = world
    assert len({c["name"] for c in cs}) == len(cs)
    for c in cs:
        assert orc.n_bytes(c["text"]) == c["B"], c["name"]
        last = orc.py.pieces(c["text"])[-1]
        assert last == c["piece"].encode(), c["name"]
        assert ttc.class_of(len(last)) == c["cls"], c["name"]
    # the cached oracle is the oracle
    for c in cs[::17]:
        assert orc.encode(c["text"]) == orc.py.encode(c["text"]), c["name"]


def test_every_edge_and_every_class_is_there(world):
    variant, orc, cs, _ = world
    Bs = {c["B"] for c in cs}
    assert {b % 4 for b in Bs if b < 128} == {0, 1, 2, 3}
    assert {63, 64, 65, ttc.TILE - 1, ttc.TILE, ttc.TILE + 1, 2 * ttc.TILE} <= Bs
    by_name = {}
    for c in cs:
        by_name.setdefault(c["name"].split("@")[0], set()).add(c["B"])
    for name, _, piece, cls in ttc.SHORT:
        assert by_name[name] >= set(ttc.B_WORD + ttc.B_TILE) and {b % 4 for b in by_name[name]} == {0, 1, 2, 3}, name
    assert [len(p.encode()) for _, _, p, _ in ttc.SHORT[:4]] == [4, 14, 24, 48]
    assert [ttc.class_of(len(p.encode())) for _, _, p, _ in ttc.SHORT[:4]] == [0, 1, 2, 3]
    for name, _, piece, cls in ttc.LONG:
        assert {b % 4 for b in by_name[name]} == {0, 1, 2, 3} and len(piece) == int(name[1:]), name
    assert [len(p) for _, _, p, _ in ttc.LONG] == [65, 256, 257, 1025, 4097]
    assert max(Bs) <= 3 * ttc.TILE
    # letters of 2, 3 and 4 bytes end exactly at B
    ends = {n: p.encode() for n, _, p, _ in ttc.SHORT}
    assert ends["e2"][-2:] == b"\xc3\xa9" and ends["e3"][-3:] == "\u754c".encode() and ends["e4"][-4:] == "\U00020000".encode()


def test_every_text_tail_is_live_for_a_case_and_every_case_under_a_tail(world):
    variant, orc, cs, live = world
    assert set(ttc.TEXT_TAILS) == {"zeros", "a", "7", "bang", "spaces", "s_spaces", "acute"}
    for t in ttc.TEXT_TAILS:
        assert any(live[c["name"], t] for c in cs), (variant, t)
    for c in cs:
        assert any(live[c["name"], t] for t in ttc.TEXT_TAILS), (variant, c["name"])
    # by construction: a letter run grows under letters, a digit run under digits, ...
    for B in (64, ttc.TILE):
        assert live["c8@%d" % B, "a"] and live["digits@%d" % B, "7"] and live["punct@%d" % B, "bang"]
        assert live["spaces@%d" % B, "spaces"] and live["space@%d" % B, "a"] and live["it_apostrophe@%d" % B, "s_spaces"]
        assert live["e2@%d" % B, "a"] and live["e3@%d" % B, "a"] and live["e4@%d" % B, "a"]
        assert live["punct@%d" % B, "zeros"]  # U+0000 is neither space, letter nor number: zeros are no neutral tail
        # U+0301 composes with the e in front under NFC; without a normaliser it is a piece of its own
        assert live["cafe@%d" % B, "acute"] == (variant != "raw")


def test_capacity_cases_hit_every_remainder(world):
    """Token counts 0, 1 and 7 mod 8 (k_wire16 and widen16 work in eights) in every length class."""
    variant, orc, cs, _ = world
    picked = ttc.capacity_cases(variant, lambda text: len(orc.encode(text)))
    for c, r in picked:
        assert orc.n_bytes(c["text"]) == c["B"] and orc.py.pieces(c["text"])[-1] == c["piece"].encode(), c["name"]
        assert len(orc.encode(c["text"])) % 8 == r and ttc.class_of(len(c["piece"])) == c["cls"], c["name"]
    assert {(c["cls"], r) for c, r in picked} == {(k, r) for k in (0, 1, 2, 3, "long") for r in (0, 1, 7)}, variant


def test_history_and_window_cases_exist(world):
    variant, orc, cs, live = world
    names = {c["name"] for c in cs}
    assert set(ttc.HISTORY) <= names and set(ttc.WINDOWS) <= names
    by = {c["name"]: c for c in cs}
    for n in ttc.HISTORY:
        docs = [by[n]["text"]]
        for split in (False, True):
            more = ttc.poison_docs(docs, split)[-1].encode()
            B = len(docs[-1].encode())
            assert len(more) >= B + 16
            tail = more[B:B + 16]
            assert (tail[0] & 0xC0) == 0x80 if split else tail.isalpha()
    assert orc.n_bytes(ttc.MARK_DOC) == len(ttc.MARK_DOC.encode()) - (0 if variant == "raw" else 1) + (variant == "prefix_space")


RULES = [  # include/ctok.h, "buffers of the device entry points": what tests/test_gpu_text_tail.py quotes
    "d_utf8 must be 16-byte aligned when n_bytes > 0",
    "d_ids of the decode 4-byte aligned when n_ids > 0",
    "checked at the entry, before any device is used",
    "a refused call launches nothing and writes nothing",
    "must be readable device memory",
    "What those bytes hold changes no result",
    "nothing past n_bytes + 16 is read",
    "a result does not depend on what an earlier call left in them",
    "ids_cap may be exactly the number of ids: nothing past ids[n_tokens) and tok_off[n_docs] is written",
    "tok_off is complete, tok_off[n_docs] holds the number of ids needed",
    "ids[0 .. ids_cap) hold the first ids_cap ids, and nothing past them is written",
]


def test_the_header_states_the_rules():
    import re
    with open(ttc.ROOT + "/include/ctok.h") as f:
        text = re.sub(r"\s+", " ", f.read().replace("\n *", " "))
    for rule in RULES:
        assert rule in text, rule
    for name in ("ctok_encode_batch_device", "ctok_encode_padded_device", "ctok_encode_windows_device", "ctok_decode_batch_device"):
        decl = text.index("int %s(" % name)
        assert "buffers of the device entry points" in text[decl - 700:decl], name


def test_misaligned_device_pointers_are_refused_before_any_device_is_used(base):
    """include/ctok.h: "CTOK_E_ARG otherwise, checked at the entry, before any device is used": the
    same on a host without a device, where a call that passes the check fails with CTOK_E_DEVICE."""
    tok = Tokenizer.from_str(json.dumps(base))
    off = np.array([0, 5], dtype=np.uint64)
    n, w = ctypes.c_uint64(), ctypes.c_uint64()
    opts = _n.PadOpts(0, 0, 8)
    for ptr in (4096 + 1, 4096 + 4, 4096 + 8):
        rc = _n.lib.ctok_encode_batch_device(tok._h, ptr, off.ctypes.data, 1, 5, 4096, 64, off.ctypes.data, ctypes.byref(n), None, None)
        assert rc == _n.CTOK_E_ARG and "16-byte aligned" in _n.last_error(), ptr
        rc = _n.lib.ctok_encode_padded_device(tok._h, ptr, off.ctypes.data, 1, 5, ctypes.byref(opts), 4096, None, None, None, 64,
                                              off.ctypes.data, ctypes.byref(w), None, None)
        assert rc == _n.CTOK_E_ARG and "16-byte aligned" in _n.last_error(), ptr
        rc = _n.lib.ctok_encode_windows_device(tok._h, ptr, off.ctypes.data, 1, 5, ctypes.byref(opts), 2, 4096, None, None, None,
                                               64, 4096, 4096, None, 8, off.ctypes.data, ctypes.byref(n), ctypes.byref(w), None, None)
        assert rc == _n.CTOK_E_ARG and "16-byte aligned" in _n.last_error(), ptr
    rc = _n.lib.ctok_decode_batch_device(tok._h, 4096 + 2, off.ctypes.data, 1, 5, 0, 4096, 64, off.ctypes.data, ctypes.byref(n), None, None)
    assert rc == _n.CTOK_E_ARG and "4-byte aligned" in _n.last_error()
    # an empty text has no pointer to check
    if _n.lib.ctok_device_count() == 0:
        rc = _n.lib.ctok_encode_batch_device(tok._h, 4096 + 1, off.ctypes.data, 0, 0, None, 0, off.ctypes.data, ctypes.byref(n), None, None)
        assert rc == _n.CTOK_E_DEVICE
