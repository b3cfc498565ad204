"""tests/pipeline_ref.py, the restatement the PipelineTokenizer suites compare against, checked on its
own: hand-worked cases, the existing restatement (oracle/ref_py.RefTokenizer) on the gpt2_50k fixture
for the default pipeline, and what the reference's own unit tests assert
(tests/golden/pipeline_reference_tests.json).  No GPU."""
import json
import os

import pytest

from datagen.build_tokenizers import fixture_path
from oracle import ref_py
from tests import pipeline_cases as pc
from tests import pipeline_ref as pr

HERE = os.path.dirname(os.path.abspath(__file__))


def ref_of(sp):
    return pr.PipelineRef(**sp)


def test_hand_worked_word_bpe():
    r = ref_of(pc.spec(pc.ABC, [("a", "a"), ("aa", "aa")]))
    assert r.encode("aaa") == [6, 0] and r.encode("aaaaa") == [7, 0] and r.encode("") == []
    # a char without a one-char vocab string is dropped: its neighbours meet and merge
    r = ref_of(pc.spec(pc.ABC, [("a", "b")]))
    assert r.encode("a?b") == [3] and r.encode("???") == [] and r.encode("a b") == [3]
    # a later duplicate pair overwrites the rank; the new id is the filtered list's entry at that rank
    r = ref_of(pc.spec(pc.ABC, [("a", "b"), ("b", "c"), ("a", "b")]))
    assert r.merge_ranks == {(0, 1): 2, (1, 2): 1} and r.merge_new_ids == [3, 4, 3] and r.encode("abc") == [0, 4]


def test_hand_worked_rank_shift_and_panic():
    r = ref_of(pc.spec(*pc.SHIFT))
    assert r.merge_ranks == {(0, 1): 1, (1, 2): 2} and r.merge_new_ids == [3, 4]
    assert r.encode("ab") == [4] and r.encode("abab") == [4, 4] and r.encode("cb") == [2, 1]
    for text in ("bc", "aabc"):  # seen adjacent is enough: (a, b) would be the better pair of "aabc"
        with pytest.raises(pr.PanicException, match="the len is 2 but the index is 2"):
            r.encode(text)
    r = ref_of(pc.spec(*pc.LATE))
    assert r.encode("aa") == [4] and r.encode("cb") == [5]
    for text in ("aab", "baab"):  # the bad pair stands adjacent only after (a, a) merged
        with pytest.raises(pr.PanicException, match="the len is 3 but the index is 3"):
            r.encode(text)


def test_hand_worked_added_tokens():
    r = ref_of(pc.spec(pc.ABC, [("a", "b")], added_tokens=pc.AT))
    assert r.encode("<s>ab") == [100, 3] and r.encode("ab<s>ab") == [3, 100, 3] and r.encode("ab[X]") == [3, 102]
    assert r.encode("<s>[X]") == [100, 102] and r.encode("a<s>>b") == [0, 101, 1]
    assert r.tokenize("a<s>>b") == ["ab"]
    r = ref_of(pc.spec(pc.ABC, [("a", "b")], added_tokens=pc.FLAGS))
    assert r.encode("a <w> b") == [0, 100, 1]
    assert r.encode("a<w> <w>") == [0]  # the first occurrence fails its check and hides the second
    assert r.encode("a <l>b") == [0, 101, 1] and r.encode("a<l>b") == [3] and r.encode("<l>b") == [101, 1]
    assert r.encode("a<r> b") == [0, 102, 1] and r.encode("a<r>b") == [3] and r.encode("a<r>") == [0, 102]
    # with a pre-tokenizer the white space is gone before the checks see it
    r = ref_of(pc.spec(pc.ABC, [("a", "b")], pre_tokenizer=("whitespace",), added_tokens=pc.FLAGS))
    assert r.encode("a <l>b") == [0, 101, 1] and r.encode("a<r> b") == [0, 102, 1] and r.encode("x<w>y <w>") == [100]


def test_hand_worked_components_and_decode():
    vocab = {"h": 0, "i": 1, "hi": 2, "▁": 3, "▁hi": 4, "<s>": 5}
    sp = pc.spec(vocab, [("h", "i"), ("▁", "hi")], ("lowercase",), ("metaspace", "▁", True), ("metaspace", "▁", True), None,
                 [pc.added("<s>", 5, special=True)])
    r = ref_of(sp)
    # Metaspace turns ' ' into the replacement and then splits on the white space that is left: one word
    assert r.words("HI hi") == ["▁hi▁hi"] and r.words("HI\thi") == ["▁hi", "hi"]
    assert r.encode("HI hi") == [4, 4] and r.tokenize("Hi") == ["▁hi"]
    assert r.decode_with_options([5, 4, 4, 99], False, False) == "<s> hi hi"
    assert r.decode_with_options([5, 4, 4, 99], True, False) == "hi hi"
    r = ref_of(pc.spec(vocab, [], decoder=None))
    assert r.decode_with_options([0, 1, 77, 3], False, False) == "hi▁" and r.decode([0, 1]) == "hi"
    r = ref_of(pc.spec({"a": 0, " ": 1, ".": 2}, [], decoder=("fuse",)))
    assert r.decode([0, 1, 2, 1, 1, 0]) == "a. a" and r.decode_with_options([0, 1, 2, 1, 1, 0], False, False) == "a .  a"


def test_parser_defaults_and_none():
    assert pr.parse_normalizer(None) == ("nfc",) and pr.parse_normalizer({"x": 1}) == ("nfc",) and pr.parse_normalizer([1]) == ("nfc",)
    assert pr.parse_normalizer({"type": "Nope"}) is None and pr.parse_normalizer({"type": 7}) is None
    assert pr.parse_normalizer({"type": "Sequence", "normalizers": [{"type": "Nope"}]}) is None
    assert pr.parse_normalizer({"type": "Sequence", "normalizers": [{"type": "Nope"}, {"type": "NFD"}, 3]}) == \
        ("sequence", [("nfd",), ("nfc",)])
    assert pr.parse_normalizer({"type": "Sequence"}) is None
    assert pr.parse_normalizer({"type": "Replace", "pattern": {"String": "a"}, "content": "b"}) == ("replace", "a", "b")
    assert pr.parse_normalizer({"type": "Replace", "pattern": {"Regex": "a"}}) == ("replace", "", "")
    assert pr.parse_normalizer({"type": "Precompiled", "precompiled_charsmap": "xyz"}) == ("precompiled", [("xyz", "xyz")])
    assert pr.parse_normalizer({"type": "BertNormalizer", "lowercase": False}) == ("bert", True, True, None, False)
    assert pr.parse_pre_tokenizer(None) == ("byte_level", False) and pr.parse_pre_tokenizer({"type": "Nope"}) is None
    assert pr.parse_pre_tokenizer({"type": "Metaspace", "replacement": ""}) == ("metaspace", "▁", True)
    assert pr.parse_pre_tokenizer({"type": "Metaspace", "replacement": "_x", "add_prefix_space": False}) == ("metaspace", "_", False)
    assert pr.parse_pre_tokenizer({"type": "Split", "pattern": {"Regex": "-"}, "behavior": "Isolated", "invert": True}) == \
        ("split", "-", "Isolated", True)
    assert pr.parse_pre_tokenizer({"type": "Split", "pattern": {"String": "-"}, "behavior": "What"}) == ("split", "", "Removed", False)
    assert pr.parse_decoder(None) == ("byte_level",) and pr.parse_decoder({"type": "Replace"}) is None
    assert pr.parse_decoder({"type": "Strip", "content": "xy", "start": 2, "stop": -1}) == ("strip", "x", 2, 0)
    assert pr.parse_decoder({"type": "Sequence", "decoders": []}) is None
    assert pr.parse_post_processor(None, {}) is None and pr.parse_post_processor({"type": "Nope"}, {}) is None
    tp = {"type": "TemplateProcessing", "single": [{"SpecialToken": {"id": "<s>"}}, {"Sequence": {"id": "A"}}, {"SpecialToken": {}}, 5]}
    assert pr.parse_post_processor(tp, {"<s>": 1}) == ("template", "<s> $A", None, [("<s>", 1)])
    assert pr.parse_post_processor({"type": "BertProcessing"}, {"[SEP]": 9}) == ("bert", ("[CLS]", 101), ("[SEP]", 9))
    assert pr.parse_merges(["a b", ["c", "d"], "abc", "a b c", ["x"], 7, " a", ["e f", "g"]]) == [("a", "b"), ("c", "d"), ("", "a")]


def test_default_pipeline_agrees_with_the_existing_restatement(tmp_path):
    """NFC -> ByteLevel on the gpt2_50k fixture: RefTokenizer.encode and decode"""
    with open(fixture_path("gpt2_50k", str(tmp_path))) as f:
        obj = json.load(f)
    old, new = ref_py.RefTokenizer(obj), pr.PipelineRef.from_json(obj)
    assert new.normalizer == ("nfc",) and new.pre_tokenizer == ("byte_level", False) and new.decoder == ("byte_level",)
    texts = ["Hello world!", "  two  spaces\n\nand lines ", "don't they'll 123 4567", "café café 中文 🙂", "<|endoftext|>x<|endoftext|>", ""]
    for t in texts:
        ids = old.encode(t)
        assert new.encode(t) == ids, t
        for skip in (False, True):
            for clean in (False, True):
                assert new.decode_with_options(ids, skip, clean) == old.decode_with_options(ids, skip, clean)


def test_what_the_reference_asserts():
    with open(os.path.join(HERE, "golden", "pipeline_reference_tests.json")) as f:
        gold = json.load(f)
    assert [g["source"][:3] for g in gold["recorded"]] == ["src", "src"]
    for g in gold["recorded"] + gold["derived"]:
        if g["kind"] == "bpe_encode":
            r = pr.PipelineRef(g["vocab"], [tuple(m) for m in g["merges"]])
            assert r.bpe(g["text"]) == g["ids"] and r.encode(g["text"]) == g["ids"], g["source"]
        elif g["kind"] == "vocab_size":
            assert pr.PipelineRef.from_json(g["json"]).vocab_size == g["vocab_size"], g["source"]
        else:
            assert pr.PipelineRef.from_json(g["json"]).encode(g["text"]) == g["ids"], g["source"]


def test_case_table_is_sound():
    """every case encodes, every panic case panics at the text, with the length and the rank it names"""
    for name, (sp, texts) in list(pc.CASES.items()) + list(pc.pipelines().items()):
        r = ref_of(sp)
        for t in texts:
            r.encode(t)
            r.tokenize(t)
    for name, (sp, texts, bad, n, rank) in pc.PANICS.items():
        r = ref_of(sp)
        for i, t in enumerate(texts):
            if i != bad:
                r.encode(t)
        with pytest.raises(pr.PanicException, match="the len is %d but the index is %d" % (n, rank)):
            r.encode(texts[bad])
    vocab, merges = pc.random_vocab(21, invalid=3)
    r = ref_of(pc.spec(vocab, merges))
    assert len(r.merge_new_ids) == len(merges) - 3 and 280 <= len(vocab) <= 320
    # the shift is live: some pair's new id is not the id of its own concatenation
    assert any(r.merge_new_ids[rank] != vocab[a + b] for rank, (a, b) in enumerate(merges)
               if a + b in vocab and rank < len(r.merge_new_ids))
