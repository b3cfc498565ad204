"""tests/pretok_ref.py (the restatement the PreTokenizer is judged by) against expectations written by
hand from the reference's src/pretokenizers.rs, each with the lines it follows.  No GPU."""
import pytest

from tests import pretok_ref as ref

S = "sequence"

EXPECT = [
    # the reference's own unit tests, :605-718
    (("whitespace",), "hello world", ["hello", "world"]),
    (("punctuation",), "hello, world!", ["hello", ",", " world", "!"]),  # :203-224 keeps the space in " world"
    (("digits", True), "hello123world", ["hello", "1", "2", "3", "world"]),
    (("bert",), "Hello, world!", ["Hello", ",", "world", "!"]),
    (("bert",), "Hello世界", ["Hello", "世", "界"]),
    (("char_delimiter_split", "_"), "hello_world_test", ["hello", "world", "test"]),
    (("unicode_scripts",), "Helloこんにちは", ["Hello", "こんにちは"]),
    (("split", r"\s", "Isolated", False), "hello world test", ["hello", " ", "world", " ", "test"]),
    (("split", "!", "MergedWithPrevious", False), "hello! world!", ["hello!", " world!"]),
    (("split", r"\$", "MergedWithNext", False), "price $100 and $50", ["price ", "$100 and ", "$50"]),
    (("split", r"\d", "Contiguous", False), "abc123def456", ["abc", "123", "def", "456"]),
    # whitespace inside or as words: digits :243-275, gpt2 :436-441
    (("digits", False), "a 12 b3", ["a ", "12", " b", "3"]),
    (("digits", False), "12ab", ["12", "ab"]),
    (("digits", True), "a٣1", ["a٣", "1"]),  # is_ascii_digit, :249
    (("gpt2",), "a  b", ["a", "  ", "b"]),  # no look-ahead: the run of spaces is one piece, :13
    (("gpt2",), "we'll go", ["we", "'ll", " go"]),
    (("gpt2",), "x 's", ["x", " '", "s"]),  # the space takes the quote before a contraction can
    # the fixed range list, :227-240: U+2003 and U+3000 are "punctuation"; bert tests whitespace first, :450
    (("punctuation",), "a b　c", ["a", " ", "b", "　", "c"]),
    (("bert",), "a b　c", ["a", "b", "c"]),
    (("punctuation",), "a¿bÀ", ["a", "¿", "bÀ"]),
    (("bert",), "x\U00030000y\U0002ebf0", ["x", "\U00030000", "y\U0002ebf0"]),  # :482-496 ends at 2EBEF
    # byte_level, :158-185
    (("byte_level", False), "a b", ["a", "Ġb"]),
    (("byte_level", True), "a b", ["Ġa", "Ġb"]),
    (("byte_level", True), " a", ["Ġa"]),
    (("byte_level", True), "", []),
    (("byte_level", True), "'s", ["Ġ'", "s"]),
    (("byte_level", False), "'s", ["'s"]),
    (("byte_level", False), "é\n", ["Ã©", "Ċ"]),
    (("byte_level", True), "\n", ["ĠĊ"]),  # the prefix and the newline are one \s+
    # metaspace, :188-200
    (("metaspace", "▁", True), "hello world", ["▁hello▁world"]),
    (("metaspace", "▁", True), "", ["▁"]),
    (("metaspace", "▁", False), "", []),
    (("metaspace", "▁", True), "a\nb c", ["▁a", "b▁c"]),
    (("metaspace", "▁", True), "\n", ["▁"]),
    (("metaspace", "　", True), "a　b\tc", ["　a　b", "c"]),  # the replacement is whitespace and stays
    ((S, [("whitespace",), ("metaspace", "▁", True)]), "a b", ["▁a", "▁b"]),  # before every word it is given
    # unicode_scripts, :508-594
    (("unicode_scripts",), "1a", ["1a"]),  # a word of Common so far accepts anything
    (("unicode_scripts",), "a1α", ["a1", "α"]),  # Common joins, the last non-Common script decides
    (("unicode_scripts",), "a 1α", ["a", "1α"]),  # whitespace forgets the script
    (("unicode_scripts",), "aअआb", ["a", "अआ", "b"]),  # Unknown is a script like any other
    (("unicode_scripts",), "a[b", ["a[b"]),  # 0x41..=0x7A is Latin, '[' included, :570
    (("unicode_scripts",), "a。b", ["a。b"]),
    (("unicode_scripts",), "aжјa", ["a", "жј", "a"]),
    # split, :298-433
    (("split", "x", "Removed", False), "abc", ["abc"]),  # no match: the word as it is, :306-308
    (("split", "x", "Removed", False), "", [""]),
    (("split", "b", "Removed", False), "abc", ["b"]),
    (("split", "b", "Removed", True), "abcb", ["a", "c"]),
    (("split", "b", "Isolated", True), "abc", ["a", "b", "c"]),  # invert matters for Removed only
    (("split", "b", "nonsense", False), "abcb", ["b", "b"]),  # components.rs:159
    (("split", "(?=b)", "Isolated", False), "abc", ["abc"]),  # the crate rejects look-ahead: vec![text], :299-302
    (("split", "aa", "Isolated", False), "aaaaa", ["aa", "aa", "a"]),
    # the five behaviours on adjacent matches
    (("split", "!", "Removed", False), "a!!b", ["!", "!"]),
    (("split", "!", "Removed", True), "a!!b", ["a", "b"]),
    (("split", "!", "Isolated", False), "a!!b", ["a", "!", "!", "b"]),
    (("split", "!", "MergedWithPrevious", False), "a!!b", ["a!!", "b"]),
    (("split", "!", "MergedWithPrevious", False), "!!b", ["!!", "b"]),
    (("split", "!", "MergedWithNext", False), "a!!b", ["a", "!", "!b"]),
    (("split", "!", "MergedWithNext", False), "a!!", ["a", "!", "!"]),
    (("split", "!", "Contiguous", False), "a!!b!", ["a", "!!", "b", "!"]),
    (("split", r"\d+", "MergedWithPrevious", False), "a12b3", ["a12", "b3"]),
    # the empty word through a Sequence, :114-124
    ((S, [("split", "a", "Removed", False), ("split", "b", "Isolated", False)]), "", [""]),
    ((S, [("split", "a", "Removed", False), ("whitespace",)]), "", []),
    ((S, [("split", "a", "Removed", False), ("metaspace", "▁", True)]), "", ["▁"]),
    ((S, [("split", "a", "Removed", False), ("metaspace", "▁", False)]), "", []),
    ((S, [("whitespace",), ("split", "a", "Removed", False)]), "", []),
    ((S, [("whitespace",), ("punctuation",), ("digits", True)]), "ab, c12", ["ab", ",", "c", "1", "2"]),
]


@pytest.mark.parametrize("i", range(len(EXPECT)))
def test_expectation(i):
    pt, text, want = EXPECT[i]
    assert ref.pre_tokenize(pt, text) == want


def test_whitespace_is_the_25_code_points():
    ws = [c for c in range(0x110000) if not 0xD800 <= c < 0xE000 and ref.pre_tokenize(("whitespace",), "a" + chr(c) + "b") == ["a", "b"]]
    assert len(ws) == 25 and set(ws) == set(ref.WHITE_SPACE)
    assert 0x1C not in ws and 0x200B not in ws  # (str.split would split on U+001C)
    assert ref.pre_tokenize(("whitespace_split",), " a b ") == ["a", "b"]


def test_bytes_to_unicode_is_a_bijection_on_printables():
    enc = [ref.byte_level(bytes([b]).decode("latin-1"), False) for b in (0x21, 0x7E)]
    assert enc == [["!"], ["~"]]
    assert ref.pre_tokenize(("byte_level", False), "\x00") == ["Ā"] and ref.pre_tokenize(("byte_level", False), "\x7f") == ["ġ"]
