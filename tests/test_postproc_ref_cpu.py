"""tests/postproc_ref.py (the restatement of src/postprocessors.rs the PostProcessor's tests compare
with) against the reference's own unit tests, recorded in tests/golden/postproc_reference_tests.json,
and against the table of quirks of tests/postproc_cases.py, whose expected outputs are written out by
hand.  No GPU."""
import json
import os

import pytest

from tests import postproc_cases as pc
from tests import postproc_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))

with open(os.path.join(HERE, "golden", "postproc_reference_tests.json"), encoding="utf-8") as _f:
    GOLDEN = json.load(_f)


def _processor(p):
    if p[0] == "bert":
        return ("bert", tuple(p[1]), tuple(p[2]))
    return ("roberta", tuple(p[1]), tuple(p[2]), p[3])


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_reference_unit_tests(case):
    if case["call"] == "process":
        assert ref.process(_processor(case["processor"]), case["ids"], case["pair"]) == case["equals"]
    elif case["call"] == "truncate":
        ids = list(case["ids"])
        pair = None if case["pair"] is None else list(case["pair"])
        ref.truncate(ids, pair, case["max_length"], case["strategy"])
        if "ids_equal" in case:
            assert ids == case["ids_equal"]
        if "pair_equals" in case:
            assert pair == case["pair_equals"]
        if "total_len" in case:
            assert len(ids) + len(pair) == case["total_len"]
            assert (ids, pair) == ([1, 2], [4, 5, 6])  # the pair down to the ids' length, then the ids first
    else:
        assert ref.pad(case["ids"], case["target_length"], case["pad_token_id"], case["pad_left"]) == case["equals"]


def test_six_reference_tests_are_recorded():
    assert len(GOLDEN) == 6 and len({c["name"] for c in GOLDEN}) == 6


@pytest.mark.parametrize("i", range(len(pc.QUIRKS)))
def test_quirks(i):
    p, ids, pair, want = pc.QUIRKS[i]
    assert ref.process(p, ids, pair) == want
    tagged = ref.process_tagged(p, ids, pair)
    assert [c[0] for c in tagged] == want
    for id_, src in tagged:  # a copied cell holds an id of the sequence it names
        assert src == ref.SPECIAL or id_ in (ids if src == ref.A else pair)


ADDED = [
    (pc.BERT, 2, 3),
    (pc.ROBERTA, 2, 4),
    (pc.DEFAULT, 2, 2),  # the entries that occur, not the occurrences: </s> twice counts once
    (("template", "<s> $A", None, [("<s>", 1)]), 1, 0),  # pair=None gives 0
    (("template", "<s> $A", "$B", [("<s>", 1), ("<s>", 2), ("<s>", 3)]), 3, 0),  # duplicated entries count each
    (("template", "<s> $A", "<s>", [("s", 1), ("", 2), ("$A", 3), ("> $", 4)]), 4, 2),  # a substring, whatever it is
    (("template", "$A", "$A", pc.SPECIALS), 0, 0),
    (("sequence", []), 0, 0),
    (("sequence", [pc.BERT, pc.ROBERTA, ("sequence", [pc.DEFAULT])]), 6, 9),  # the sum
]


@pytest.mark.parametrize("p,single,pair", ADDED)
def test_added_tokens(p, single, pair):
    assert ref.added_tokens_single(p) == single
    assert ref.added_tokens_pair(p) == pair


def test_truncate_by_hand():
    def t(ids, pair, n, s):
        ids, pair = list(ids), (None if pair is None else list(pair))
        ref.truncate(ids, pair, n, s)
        return ids, pair

    assert t([1, 2, 3, 4, 5], None, 3, "only_first") == ([1, 2, 3], None)
    assert t([1, 2], [3, 4, 5], 1, "only_first") == ([], [3, 4, 5])  # no more than the first sequence has
    assert t([1, 2, 3], None, 1, "only_second") == ([1, 2, 3], None)  # removes nothing from a row without a pair
    assert t([1, 2, 3], [], 1, "only_second") == ([1, 2, 3], [])
    assert t([1, 2, 3], [4, 5, 6], 4, "longest_first") == ([1, 2], [4, 5])  # equal lengths: the first sequence first
    assert t([1, 2, 3], [4, 5, 6], 3, "longest_first") == ([1], [4, 5])
    assert t([1, 2, 3, 4, 5], [6], 3, "longest_first") == ([1, 2], [6])
    assert t([1], [2, 3, 4, 5], 0, "longest_first") == ([], [])
    assert t([1, 2, 3], None, 1, "longest_first") == ([1], None)
    assert t([1, 2, 3], [4], 9, "longest_first") == ([1, 2, 3], [4])


def test_pad_and_masks_by_hand():
    assert ref.pad([1, 2, 3], 5, 9, True) == [9, 9, 1, 2, 3]
    assert ref.pad([1, 2, 3], 2, 9, False) == [1, 2, 3]  # a longer row stays as it is
    got = ref.process_padded(pc.BERT, [[1, 2], [3]], [[4], None], pad_to="longest", pad_id=7)
    assert got["input_ids"] == [[101, 1, 2, 102, 4, 102], [101, 3, 102, 7, 7, 7]]
    assert got["attention_mask"] == [[1, 1, 1, 1, 1, 1], [1, 1, 1, 0, 0, 0]]
    assert got["token_type_ids"] == [[0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0]]
    assert got["special_tokens_mask"] == [[1, 0, 0, 1, 0, 1], [1, 0, 1, 1, 1, 1]]
    assert got["row_len"] == [6, 3] and got["width"] == 6
    got = ref.process_padded(pc.BERT, [[1, 2], [3]], None, truncate_to=1, strategy="only_first", pad_to=2, pad_left=True)
    assert got["input_ids"] == [[101, 1, 102], [101, 3, 102]] and got["width"] == 3  # truncate_to bounds the inputs
    got = ref.process_padded(pc.BERT, [[1], []], None, pad_to=4, pad_left=True, pad_id=7)
    assert got["input_ids"] == [[7, 101, 1, 102], [7, 7, 101, 102]]
    assert got["attention_mask"] == [[0, 1, 1, 1], [0, 0, 1, 1]]
