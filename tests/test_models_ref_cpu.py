"""The restatements of the reference's three stand-alone models (tests/models_ref.py) against
hand-worked cases from src/models.rs:300-741, and what of complexity_tokenizer.models needs no
device: the exports, the argument errors and the host string helpers of decode.  No GPU."""
import random

import pytest

import complexity_tokenizer
from complexity_tokenizer import ByteLevelBpeModel, CharBpeModel, WordLevelModel, models
from tests import models_ref
from tests.models_ref import RefByteLevelBpeModel, RefCharBpeModel, RefWordLevelModel

B2U = models_ref.bytes_to_unicode()
G = B2U[0x20]  # the byte-map char of the space


def _both(vocab, merges, **kw):
    """the char model with an empty suffix and the byte-level model without the prefix space: on
    ASCII words both run the same merge loop over the same strings"""
    return (RefCharBpeModel(vocab, merges, "", **kw), RefByteLevelBpeModel(vocab, merges, add_prefix_space=False, **kw))


def test_one_merge_per_step_is_not_all_occurrences():
    vocab = {"<unk>": 0, "a": 1, "b": 2, "ab": 3, "aba": 4}
    for m in _both(vocab, [("ab", "a"), ("a", "b")]):
        assert m.encode("abab") == [4, 2]  # aba b; merging every (a, b) at once would give ab ab = [3, 3]


def test_repeated_char():
    vocab = {"<unk>": 0, "a": 1, "aa": 2}
    for m in _both(vocab, [("a", "a")]):
        assert m.encode("aaa") == [2, 1] and m.encode("aaaa") == [2, 2]


def test_last_duplicate_wins():
    vocab = {"<unk>": 0, "a": 1, "b": 2, "c": 3, "ab": 4, "bc": 5}
    for m in _both(vocab, [("a", "b"), ("b", "c"), ("a", "b")]):
        assert m.encode("abc") == [1, 5]
    for m in _both(vocab, [("a", "b"), ("b", "c")]):
        assert m.encode("abc") == [4, 3]


def test_merge_parts_outside_the_vocab():
    vocab = {"<unk>": 0, "abc": 5}
    for m in _both(vocab, [("a", "b"), ("ab", "c")]):
        assert m.encode("abc") == [5] and m.encode("ab") == [0] and m.encode("ba") == [0, 0]


def test_unk_token_absent_is_id_0():
    vocab = {"a": 3, "zero": 0}
    assert RefWordLevelModel(vocab, "[UNK]").encode("a q") == [3, 0]
    assert RefCharBpeModel(vocab, [], "", "[UNK]").encode("aq") == [3, 0]
    assert RefByteLevelBpeModel(vocab, [], "[UNK]", False).encode("aq") == [3, 0]
    assert RefWordLevelModel(vocab, "a").encode("q") == [3]


def test_prefix_space_and_byte_level_words():
    m = RefByteLevelBpeModel({}, [])
    assert m.words("") == [" "] and m.words("a") == [" a"] and m.words(" a") == [" a"]
    assert m.words("a  b") == [" a", " ", " b"]
    n = RefByteLevelBpeModel({}, [], add_prefix_space=False)
    assert n.words("") == [] and n.words("a  b") == ["a", " ", " b"] and n.words("a ") == ["a", " "]
    assert n.words("a\tb\nc\u00a0d e") == ["a\tb\nc\u00a0d", " e"]
    vocab = {"<unk>": 0, G: 1, G + "a": 2, "a": 3, "b": 4}
    m = RefByteLevelBpeModel(vocab, [(G, "a")])
    assert m.encode("") == [1] and m.encode("a") == [2] and m.encode("a  b") == [2, 1, 1, 4]
    assert m.encode("\u00e9") == [1, 0, 0]  # one token per byte


def test_suffix():
    vocab = {"<unk>": 0, "a": 1, "a</w>": 2, "aa</w>": 3, "b": 4}
    m = RefCharBpeModel(vocab, [("a", "a</w>")])
    assert m.encode("a") == [2] and m.encode("aa") == [3] and m.encode("aaa b") == [1, 3, 0]
    assert m.tokenize_word("b") == ["b</w>"]
    e = RefCharBpeModel(vocab, [("a", "a")], "")
    assert e.tokenize_word("aab") == ["aa", "b"] and e.encode("aab") == [0, 4]


def test_decode_cases():
    assert models_ref.from_utf8_lossy(b"a\xe2\x82") == "a\ufffd"           # a truncated 3-byte sequence
    assert models_ref.from_utf8_lossy(b"\x80a") == "\ufffda"               # a lone continuation byte
    assert models_ref.from_utf8_lossy(b"\xe0\x80") == "\ufffd\ufffd"       # E0 needs A0..BF
    assert models_ref.from_utf8_lossy(b"\xf5") == "\ufffd"
    assert models_ref.from_utf8_lossy(b"\xf0\x9f\x98\x80\xf0\x9f\x98") == "\U0001F600\ufffd"
    assert models_ref.from_utf8_lossy(b"\xed\xa0\x80") == "\ufffd\ufffd\ufffd"  # a surrogate
    rng = random.Random(5)
    for _ in range(3000):
        raw = bytes(rng.choice(b"a\x80\xbf\xc2\xe0\xe2\xed\xf0\xf4\xf5\x9f\xa0\x90") for _ in range(rng.randint(0, 8)))
        want = raw.decode("utf-8", errors="replace")  # (CPython replaces maximal subparts as well)
        assert models_ref.from_utf8_lossy(raw) == want and models.from_utf8_lossy(raw) == want, raw
    assert models_ref.trim_end("a \u3000") == "a" and models_ref.trim_end("a\x1f") == "a\x1f"
    assert "a\x1f".rstrip() == "a"  # (Python's own set is another)
    vocab = {"<unk>": 0, "a</w>": 1, "b": 2, "\u3000</w>": 3, "\x1f</w>": 4}
    m = RefCharBpeModel(vocab, [])
    assert m.decode([2, 1, 2, 1]) == "ba ba" and m.decode([1, 3]) == "a" and m.decode([1, 4]) == "a \x1f"
    assert m.decode([9, 2]) == "b"
    e = RefCharBpeModel({"a": 1, "b": 2}, [], "")
    assert e.decode([1, 2]) == "a b"  # with an empty suffix every token ends with it
    assert RefWordLevelModel({"x": 1, "y": 2}).decode([2, 7, 1]) == "y x"
    bl = RefByteLevelBpeModel({G + "a": 1, B2U[0xE2] + B2U[0x82]: 2, "\u4e2d": 3, B2U[0x80]: 4}, [])
    assert bl.decode([1, 2]) == " a\ufffd" and bl.decode([3, 1]) == " a" and bl.decode([4]) == "\ufffd"
    # shared ids: the smallest string by UTF-8 bytes
    for m in (RefWordLevelModel({"b": 1, "a": 1, "\u00e9": 1, "Z": 1}), RefCharBpeModel({"b": 1, "a": 1, "Z": 1}, [])):
        assert m.id_to_token(1) == "Z" and m.vocab_size >= 3
    assert RefWordLevelModel({"\U00010000": 1, "\uffff": 1}).id_to_token(1) == "\uffff"  # bytes, not UTF-16


def test_fast_loop_is_the_literal_loop():
    rng = random.Random(11)
    for _ in range(300):
        pool = list("abc")
        merges = []
        for _ in range(rng.randint(0, 12)):
            a, b = rng.choice(pool), rng.choice(pool)
            merges.append((a, b))
            pool.append(a + b)
        rng.shuffle(merges)
        ranks = models_ref.merge_ranks(merges)
        word = [rng.choice("abc") for _ in range(rng.randint(1, 30))]
        assert models_ref.merge_loop(word, ranks) == models_ref.merge_loop_literal(word, ranks)


def test_exports():
    for name in ("WordLevelModel", "CharBpeModel", "ByteLevelBpeModel"):
        assert name in complexity_tokenizer.__all__ and hasattr(complexity_tokenizer, name)
    assert complexity_tokenizer.__version__ == "0.3.3"
    assert models._bytes_to_unicode() == B2U
    assert set(models._WHITE_SPACE) == set(models_ref.WHITE_SPACE)


def test_argument_errors():
    with pytest.raises(TypeError, match="PyDict"):
        WordLevelModel([("a", 1)])
    with pytest.raises(TypeError, match="PyString"):
        WordLevelModel({1: 1})
    with pytest.raises(TypeError, match="integer"):
        CharBpeModel({"a": "1"}, [])
    with pytest.raises(OverflowError):
        CharBpeModel({"a": -1}, [])
    with pytest.raises(OverflowError):
        ByteLevelBpeModel({"a": 1 << 32}, [])
    with pytest.raises(TypeError, match="Vec"):
        CharBpeModel({"a": 1}, "ab")
    with pytest.raises(TypeError, match="PyTuple"):
        CharBpeModel({"a": 1}, [["a", "b"]])
    with pytest.raises(ValueError, match="length 2"):
        ByteLevelBpeModel({"a": 1}, [("a", "b", "c")])
    with pytest.raises(TypeError, match="PyString"):
        ByteLevelBpeModel({"a": 1}, [("a", 1)])
    with pytest.raises(TypeError, match="Sequence"):
        CharBpeModel({"a": 1}, 5)
    with pytest.raises(TypeError, match="PyString"):
        CharBpeModel({"a": 1}, [], end_of_word_suffix=None)
    with pytest.raises(TypeError, match="PyString"):
        WordLevelModel({"a": 1}, unk_token=3)
    with pytest.raises(TypeError, match="PyBool"):
        ByteLevelBpeModel({"a": 1}, [], add_prefix_space="yes")
