"""tests/normalizer_ref.py (the restatement of the reference's src/normalizers.rs the Normalizer tests
compare with) checked against cases worked by hand from the reference's rules, its own unit tests
(src/normalizers.rs:219-284) among them.  No GPU."""
from tests import normalizer_ref as ref


def test_the_reference_unit_tests():
    assert ref.normalize(("nfc",), "e\u0301") == "\u00e9"
    assert ref.normalize(("lowercase",), "HELLO World") == "hello world"
    assert ref.normalize(("strip_accents",), "caf\u00e9") == "cafe"
    assert ref.normalize(("strip_accents",), "na\u00efve") == "naive"
    bert_sequence = ("sequence", [("nfc",), ("lowercase",), ("strip_accents",), ("strip",)])
    assert ref.normalize(bert_sequence, "  CAF\u00c9  ") == "cafe"
    bert = ("bert", True, True, True, True)
    assert ref.normalize(bert, "HELLO") == "hello" and ref.normalize(bert, "Caf\u00e9") == "cafe"
    assert ref.normalize(("precompiled", [("\ufb01", "fi"), ("\ufb02", "fl")]), "\ufb01le") == "file"


def test_bert_by_hand():
    # a space on each side of every CJK code point, then lowercase
    assert ref.normalize(("bert", True, True, None, True), "Hello\u4e16\u754c") == "hello \u4e16  \u754c "
    # lowercase comes last: with the accents kept U+0130 ends as i + U+0307, which nothing strips any
    # more; with them stripped, NFD gives I + U+0307, the mark goes and "I" is lower-cased
    assert ref.normalize(("bert", True, True, False, True), "\u0130") == "i\u0307"
    assert ref.normalize(("bert", True, True, None, True), "\u0130") == "i"
    # strip_accents None follows lowercase; False keeps the accent; NFC always runs
    assert ref.normalize(("bert", True, True, None, False), "Cafe\u0301") == "Caf\u00e9"
    assert ref.normalize(("bert", True, True, False, True), "Cafe\u0301") == "caf\u00e9"
    assert ref.normalize(("bert", True, True, True, False), "Caf\u00e9") == "Cafe"
    # clean_text: controls go (U+0085 is one, so it is not turned into a space), \t \n \r and the
    # other White_Space code points become U+0020, U+001C is a control, U+200B stays
    assert ref.clean_text("a\x00b\tc\nd\re\x7ff\x85g\u00a0h\u2028i\x1cj\u200bk") == "ab c d efg h ij\u200bk"
    assert ref.normalize(("bert", False, False, None, False), "a\x00\u4e16") == "a\x00\u4e16"
    assert ref.handle_chinese_chars("\u3400\u4dbf\u4dc0\U0002ceaf\U0002ceb0\ufaff\ufb00") == \
        " \u3400  \u4dbf \u4dc0 \U0002ceaf \U0002ceb0 \ufaff \ufb00"


def test_replace_by_hand():
    assert ref.normalize(("replace", "aa", "b"), "aaaaa") == "bba"
    assert ref.normalize(("replace", "", "-"), "abc") == "-a-b-c-"
    assert ref.normalize(("replace", "", "-"), "") == "-"
    assert ref.normalize(("precompiled", [("a", "b"), ("b", "c")]), "ab") == "cc"  # list order, each over the whole


def test_strip_is_not_str_strip():
    assert ref.normalize(("strip",), "\x1c a \x1c") == "\x1c a \x1c"
    assert "\x1c a \x1c".strip() == "a"
    assert ref.normalize(("strip",), " \u3000\u0085\u00a0x\u2028\u205f") == "x"
    assert ref.normalize(("strip",), "\u200bx\u200b") == "\u200bx\u200b"
    assert ref.normalize(("strip",), " \t\u2003") == ""
    assert len(ref.WHITE_SPACE) == 25


def test_strip_accents_is_five_ranges_not_category_m():
    assert ref.normalize(("strip_accents",), "\u05d0\u0591") == "\u05d0\u0591"  # U+0591 is Mn and stays
    assert ref.normalize(("strip_accents",), "a\u0300\u036f\u0370\u1ab0\u1dc0\u20d0\u20ff\u2100\ufe20\ufe2f\ufe30") == "a\u0370\u2100\ufe30"
    assert ref.normalize(("strip_accents",), "\u1e69") == "s"  # NFD first: s + U+0323 + U+0307


def test_affixes_and_sequences():
    assert ref.normalize(("prepend", "\u2581"), "") == "\u2581" and ref.normalize(("append", "!"), "") == "!"
    seq = ("sequence", [("prepend", "<"), ("sequence", [("append", ">"), ("replace", "<", "[")])])
    assert ref.normalize(seq, "x") == "[x>"
    assert [s[0] for s in ref.flat_steps(seq)] == [8, 9, 7]
