"""tests/decoder_ref.py (the restatement of src/decoders.rs the Decoder's tests compare with) against
the reference's own unit tests, recorded in tests/golden/decoder_reference_tests.json, and against the
worked examples of the rules.  No GPU."""
import json
import os

import pytest

from tests import decoder_cases as dc
from tests import decoder_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "decoder_reference_tests.json"), encoding="utf-8") as _f:
    GOLDEN = json.load(_f)


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_reference_unit_tests(case):
    got = ref.decode(tuple(case["decoder"]), case["tokens"])
    if "equals" in case:
        assert got == case["equals"]
    else:
        assert case["contains"] in got
    if case["name"] == "test_byte_level_decode":
        assert got == " Hello world"


def test_six_reference_tests_are_recorded():
    assert len(GOLDEN) == 6 and len({c["decoder"][0] for c in GOLDEN}) == 6


EXAMPLES = [
    (("byte_level",), ["â", "Ĥ"], "\ufffd"),  # E2 82
    (("byte_level",), ["ð", "Ł", "A", "Ģ"], "\ufffdA\ufffd"),  # F0 9F 41 80
    (("byte_level",), ["a b", "\x7f", "\x00"], "a b\x7f\x00"),  # ASCII outside the byte map stays
    (("byte_level",), ["\u0080", " ", "\u00ad", "\u00a0", "▁", "😀", "Ń", "ń"], " \ufffd"),  # dropped, but ' ' stays and U+0143 -> AD
    (("metaspace", "▁", True), [" ▁a"], " a"),  # an original leading space counts too
    (("metaspace", "▁", False), ["▁a"], " a"),
    (("wordpiece", "##", True), ["", "a", "##", "b", ".", "'", "c"], "a b.'c"),
    (("wordpiece", "##", True), ["x", "", "y"], "x  y"),
    (("wordpiece", "##", True), ["##a", "b"], "a b"),
    (("wordpiece", "", True), ["a", "b", "."], "ab."),
    (("wordpiece", "##", True), ["a", " ", "."], "a  ."),
    (("wordpiece", "##", True), ["a", "'", "b"], "a'b"),
    (("bpe", "</w>"), ["a</w>", "b", "</w>", "\u3000"], "a b"),
    (("bpe", ""), ["a", "b"], "a b"),
    (("ctc", "<pad>", "|"), ["H", "H", "E", "<pad>", "L", "L", "O", "|", "W"], "HELO W"),
    (("ctc", "<pad>", "|"), ["a", "<pad>", "a", "a", "|", "a"], "aa a"),
    (("strip", "_", 2, 2), ["___"], ""),
    (("strip", "_", 5, 0), ["_a", "_"], "a_"),
    (("replace", "", "-"), ["abc"], "-a-b-c-"),
    (("replace", "aa", "b"), ["aaa"], "ba"),
    (("sequence", [("fuse",), ("ctc", "<pad>", "")]), [], " "),
    (("sequence", [("fuse",), ("bpe", "x")]), ["a", " \tx"], "a"),
    (("sequence", []), ["a", "b"], "ab"),
    (("sequence", [("sequence", []), ("wordpiece", "##", False)]), ["a", "b"], "ab"),
]


@pytest.mark.parametrize("dec,tokens,want", EXAMPLES)
def test_worked_examples(dec, tokens, want):
    assert ref.decode(dec, tokens) == want


def test_byte_map():
    m = ref.unicode_to_bytes()
    assert len(m) == 256 and sorted(m.values()) == list(range(256))
    assert m["Ġ"] == 0x20 and m["Ċ"] == 0x0A and m["!"] == 0x21 and m["ÿ"] == 0xFF
    assert max(map(ord, m)) == 0x143 and m["Ń"] == 0xAD


def test_flat_steps_and_cases():
    assert ref.flat_steps(("sequence", [])) == [(5, 0, b"", b"", 0, 0, 0)]
    assert [s[0] for s in ref.flat_steps(("sequence", [("sequence", [("fuse",), ("bpe", "x")]), ("byte_level",)]))] == [5, 3, 0]
    assert {d[0] for d in dc.EVERY} == set(ref.KINDS) | {"sequence"}
    for d in dc.EVERY:  # every decoder runs over every quirk
        for q in dc.QUIRKS:
            assert isinstance(ref.decode(d, q), str)
    assert dc.random_token_lists("vocab", 1, 5, 9) == dc.random_token_lists("vocab", 1, 5, 9)
    assert len(ref.WHITE_SPACE) == 25
