"""GPU parity of `PreTokenizer.split(..., regex=True)` (the DFA kernels of csrc/pretok.hip) and of
sequences and pipelines that hold it, against tests/pretok_ref.py and tests/pipeline_encoding_ref.py.
Exact equality of word lists; tests/test_regex_dfa_cpu.py runs the same rules on the CPU first.
Every bound the shapes depend on is read from `PreTokenizer.limits()`."""
import json

import numpy as np
import pytest

import complexity_tokenizer as ct
from complexity_tokenizer import PipelineTokenizer, PreTokenizer, UnsupportedConfigError
from oracle.ref_py import bytes_to_unicode
from tests import pipeline_cases as plc
from tests import pretok_cases as pc
from tests import pretok_ref as ref
from tests import regex_split_cases as rc
from tests.pipeline_encoding_ref import PanicException, PipelineEncodingRef, enc_dict

pytestmark = pytest.mark.gpu


def check(pt, texts):
    p = rc.to_pretokenizer(pt)
    got = p.pre_tokenize_batch(texts)
    assert len(got) == len(texts)
    bad = [i for i, t in enumerate(texts) if got[i] != ref.pre_tokenize(pt, t)]
    assert not bad, (pt, len(bad), texts[bad[0]][:80], got[bad[0]][:8], ref.pre_tokenize(pt, texts[bad[0]])[:8])
    return p


def every_behaviour(pattern):
    return [("split", pattern, b, inv) for b in pc.BEHAVIORS for inv in ((False, True) if b == "Removed" else (False,))]


SIZES = (0, 1, 63, 64, 65, 127, 128, 129)


def test_sizes_around_a_bitmap_word():
    texts = [("ab1 22b" * 20)[:n] for n in SIZES] + [("7" * 200)[:n] for n in SIZES] + [("abab a" * 30)[:n] for n in SIZES]
    for pattern in (r"\p{N}{1,3}", "ab|a", "a|ab", r"\s+\S", "(?:ab)+c?"):
        for pt in every_behaviour(pattern):
            check(pt, texts)


def _boundaries():
    lim = PreTokenizer.limits()
    return (64, 128, lim["scan_tile_bytes"], lim["scan_tile_bytes"] * (pc.THREADS // pc.SPAN))


def test_matches_across_and_up_to_every_boundary():
    """a three-byte match that ends exactly on a bitmap word, a prefix-max tile and a workgroup's
    tiles, that straddles each with every split of its bytes, and that starts on it; texts one byte
    either side of each size"""
    texts = []
    for b in _boundaries():
        for start in range(b - 4, b + 2):
            texts.append("x" * start + "123" + "y")
            texts.append("x" * start + "1234")  # (the second match is one digit)
        texts += ["x" * (n - 3) + "123" for n in (b - 1, b, b + 1)] + ["1" * n for n in (b - 1, b, b + 1)]
    for pt in (("split", r"\p{N}{1,3}", "Isolated", False), ("split", r"\p{N}{1,3}", "Removed", False),
               ("split", "[0-9][0-9][0-9]", "MergedWithPrevious", False), ("split", r"\d+?\d", "Contiguous", False)):
        check(pt, texts)


def test_matches_across_a_round_of_the_carry():
    """k_pt_dfa_carry keeps its running maximum between rounds of THREADS tiles: a chain from before a
    round's end into the next one, and a head right after it"""
    b = PreTokenizer.limits()["scan_round_bytes"]
    texts = ["x" * (b - 5) + "1234567 12", "x" * (b - 2) + "12" + "y" * 8 + "3", "x" * (b + 1)]
    check(("split", r"\p{N}{1,3}", "Isolated", False), texts)
    check(("sequence", [("whitespace",), ("split", r"\p{N}{1,3}", "Removed", False)]), texts)


@pytest.mark.parametrize("offset", range(4))
def test_one_chain_longer_than_a_tile(offset):
    """1,000 digits are one chain of 334 matches that one thread walks; the word starts `offset` + 1
    bytes into the text, so the triples do not align to lanes"""
    text = "x" * offset + " " + "7" * 1000
    assert len("7" * 1000) > PreTokenizer.limits()["scan_tile_bytes"] - 64
    for b in ("Isolated", "Removed", "MergedWithNext"):
        check(("sequence", [("whitespace",), ("split", r"\p{N}{1,3}", b, False)]), [text, text + " 12345", "", text])


def test_wide_scalars_under_the_dot_and_negated_classes():
    texts = ["aé世😀\nb", "é", "世", "😀", "😀😀\n😀", "aéb世b😀b", "\n\n", "é\n世", "٣é１😀", "ab" + "世" * 70 + "b", "😀" * 33 + "ab"]
    for pattern in (".", "..", ".+", r"[^\n]+?b", "[^a]b", r"\P{L}\p{L}", r"\P{N}{2}", r"[^é世]😀?", r"\S\s?"):
        for pt in every_behaviour(pattern)[:3]:
            check(pt, texts)


def test_priorities():
    """leftmost-first, not leftmost-longest: the pairs differ where the crate makes them differ"""
    first = rc.to_pretokenizer(("split", "a|ab", "Isolated", False))
    longer = rc.to_pretokenizer(("split", "ab|a", "Isolated", False))
    assert first.pre_tokenize("xaby") == ["x", "a", "by"] and longer.pre_tokenize("xaby") == ["x", "ab", "y"]
    greedy = rc.to_pretokenizer(("split", "a+", "Isolated", False))  # (a class atom: its own path, with the flag too)
    lazy = rc.to_pretokenizer(("split", "a+?", "Isolated", False))
    assert greedy.pre_tokenize("baaab") == ["b", "aaa", "b"] and lazy.pre_tokenize("baaab") == ["b", "a", "a", "a", "b"]
    texts = ["xaby abab aab", "baaab aa", "ababab", "abcbc abc ac"]
    for pattern in ("a|ab", "ab|a", "a+?", "a+?b?", "(ab|a)(bc|c)?", "(a|ab)(c|bcd)?"):
        check(("split", pattern, "Isolated", False), texts)


def test_no_match_and_the_empty_text():
    for pattern in (r"\p{N}{1,3}", "q|zz"):
        p = check(("split", pattern, "Removed", False), ["no match here", "", "é"])
        assert p.pre_tokenize("no match here") == ["no match here"] and p.pre_tokenize("") == [""]
        check(("split", pattern, "Removed", True), ["no match here", "", "é"])
        check(("sequence", [("split", pattern, "Isolated", False), ("whitespace",)]), ["no match here", "", "a1b"])
    assert rc.to_pretokenizer(("split", r"\p{N}{1,3}", "Isolated", False)).pre_tokenize_batch([]) == []


def test_each_side_of_the_lds_threshold():
    small, large = r"\d{1,3}(?:,\d{3})+", "[abcdefgh]{1,3000}x"
    lim = PreTokenizer.limits()
    a, b = PreTokenizer.split_plan(small), PreTokenizer.split_plan(large)
    assert a["gate"] == b["gate"] == "dfa"
    assert a["table_in_lds"] and a["table_bytes"] <= lim["lds_table_bytes"] < b["table_bytes"] and not b["table_in_lds"]
    texts = ["1,234,567 12,34 1,000", "abcdefghx x ax hgfedcbaabx" + "ab" * 40 + "x", "", "x" * 70 + "hax"]
    for pattern in (small, large):
        for pt in every_behaviour(pattern):
            check(pt, texts)


@pytest.mark.parametrize("pool", sorted(pc.POOLS))
def test_seeded_random_strings(pool):
    texts = pc.random_texts(pool, 20265, 400, 150)
    pts = [("split", r"\p{N}{1,3}", "Isolated", False), ("split", rc.GPT2_LIKE, "Isolated", False), ("split", r"\s+\S", "Removed", False),
           ("split", r"\d+\.\d+|\d+", "Removed", True), ("split", "a+?b?", "MergedWithPrevious", False),
           ("split", r"[^\n]+?b", "MergedWithNext", False), ("split", "(ab|a)(bc|c)?", "Contiguous", False),
           ("sequence", [("whitespace",), ("split", "x{0,2}y|[a-c][X-Z]", "Contiguous", False)]),
           ("sequence", [("punctuation",), ("split", r".+?\s", "Isolated", False), ("byte_level", False)])]
    for pt in pts:
        check(pt, texts)


def test_packed_form_is_the_batch_form():
    texts = pc.QUIRKS + pc.random_texts("digits", 4, 200)
    raw = [t.encode() for t in texts]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    for pt in (("split", r"\p{N}{1,3}", "Isolated", False), ("sequence", [("whitespace",), ("split", r"\d+\.\d+|\d+", "Removed", False)])):
        p = rc.to_pretokenizer(pt)
        words, word_off, text_word = p.pre_tokenize_packed(np.frombuffer(b"".join(raw), dtype=np.uint8), off)
        body, wo, tw = words.tobytes(), word_off.tolist(), text_word.tolist()
        assert tw[0] == 0 and tw[-1] == len(wo) - 1 and wo[-1] == len(body) and wo == sorted(wo)
        got = [[body[wo[j]:wo[j + 1]].decode() for j in range(tw[i], tw[i + 1])] for i in range(len(texts))]
        assert got == p.pre_tokenize_batch(texts) == [ref.pre_tokenize(pt, t) for t in texts]


def test_the_work_bound(monkeypatch):
    default = PreTokenizer.limits()["max_regex_run"]
    monkeypatch.setenv("CTOK_PRETOK_MAX_REGEX_RUN", str(1 << 40))  # nothing raises the cap
    assert PreTokenizer.limits()["max_regex_run"] == default
    monkeypatch.setenv("CTOK_PRETOK_MAX_REGEX_RUN", "96")
    cap = PreTokenizer.limits()["max_regex_run"]
    assert cap == 96
    pt = ("sequence", [("whitespace",), ("split", ".+", "Isolated", False)])
    p = rc.to_pretokenizer(pt)
    assert PreTokenizer.split_plan(".+")["cyclic"]
    fits = ["ab", "cd " + "é" * cap, "é" * cap + " " + "世" * cap]
    assert p.pre_tokenize_batch(fits) == [ref.pre_tokenize(pt, t) for t in fits]
    with pytest.raises(UnsupportedConfigError) as e:
        p.pre_tokenize_batch(["ab", "é" * cap, "cd " + "é" * (cap + 1), "x" * (2 * cap)])
    assert "text 2" in str(e.value) and str(cap) in str(e.value)
    assert p.pre_tokenize_batch(fits) == [ref.pre_tokenize(pt, t) for t in fits]  # (the handle goes on)
    # a pattern whose matches are bounded has no cap
    bounded = ("split", r"\p{N}{1,3}", "Isolated", False)
    assert not PreTokenizer.split_plan(bounded[1])["cyclic"]
    check(bounded, ["7" * (4 * cap), "x" * (4 * cap)])


def test_without_the_keyword_nothing_changes():
    for pattern in ("a|b", r"\p{N}{1,3}", "[0-9][0-9][0-9]", ".", r"\d{2}"):
        with pytest.raises(UnsupportedConfigError):
            PreTokenizer.split(pattern, "Isolated")
        with pytest.raises(UnsupportedConfigError):
            PreTokenizer.split(pattern, "Isolated", regex=False)
        assert "regex=True" in repr(PreTokenizer.split(pattern, "Isolated", regex=True))
    with pytest.raises(TypeError):
        PreTokenizer.split("a|b", "Isolated", False, 0, True)  # keyword-only
    with pytest.raises(UnsupportedConfigError) as e:
        PreTokenizer.split(r"\bfoo", "Isolated", regex=True)
    assert r"\bfoo" in str(e.value) and "word boundary" in str(e.value)
    # a literal and a class atom keep their paths with the flag
    for pattern, text, want in (("ab", "xaby", ["x", "ab", "y"]), (r"\d+", "a12b", ["a", "12", "b"])):
        assert PreTokenizer.split(pattern, "Isolated", regex=True).pre_tokenize(text) == want


# ---- a DeepSeek-shaped tokenizer.json --------------------------------------------------------------------

LOOK_AHEAD = r"[!-/:-~！-／：-～‘-‟　-。]+|\s?\p{L}+|\s+(?!\S)|\s+"  # (the crate rejects look-ahead: the reference drops the step)


def deepseek_shaped():
    enc = bytes_to_unicode()
    vocab = {enc[b]: b for b in range(256)}
    merges = []
    for a, b in (("1", "2"), ("12", "3"), ("4", "5"), ("a", "b"), (enc[0x20], "a"), ("c", "d"), (enc[0xE4], enc[0xB8]),
                 (enc[0xE4] + enc[0xB8], enc[0x80])):
        merges.append((a, b))
        vocab[a + b] = len(vocab)
    pre = ("sequence", [("split", r"\p{N}{1,3}", "Isolated", False), ("split", "[一-龥]+", "Isolated", False),
                        ("split", LOOK_AHEAD, "Isolated", False), ("byte_level", False)])
    sp = plc.spec(vocab, merges, None, pre, None, None, [plc.added("<s>", 1000, special=True)])
    obj = plc.tokenizer_json(sp, {"pre_tokenizer": plc.pre_tokenizer_json(pre)})
    texts = ["ab 1234567 cd", "一丁一12345ab", "price 1234 ab一一 12", "", " ", "<s>123 45 ab", "123123123 1 12 abab4545", "a1b22c333d4444",
             "x" * 70 + "1234" + "一" * 30 + " ab 123"]
    return obj, texts


def test_a_deepseek_shaped_file():
    obj, texts = deepseek_shaped()
    with pytest.raises(UnsupportedConfigError):
        PipelineTokenizer.from_str(json.dumps(obj))  # still refused without the keyword
    tok = PipelineTokenizer.from_str(json.dumps(obj), regex_split=True)
    assert "regex=True" in repr(tok.pre_tokenizer) and "regex=True" in repr(tok)
    oracle = PipelineEncodingRef.from_json(obj)
    for t in texts:
        assert tok.encode(t) == oracle.encode(t), t
        assert tok.tokenize(t) == oracle.tokenize(t), t
    assert tok.tokenize("1234567") == ["123", "45", "6", "7"]  # the triples are cut before the merges run
    assert tok.encode_batch(texts) == [oracle.encode(t) for t in texts]
    want = []
    for t in texts:
        try:
            want.append(oracle.encode_to_encoding(t).as_dict())
        except PanicException:
            want.append(None)
    clean = [t for t, w in zip(texts, want) if w is not None]
    assert len(clean) >= 5
    got = tok.encode_batch_to_encoding(clean)
    for g, t, w in zip(got, clean, [w for w in want if w is not None]):
        assert enc_dict(g) == w, (t, enc_dict(g), w)
    # the other constructors take the keyword too
    from complexity_tokenizer.pipeline import parse_tokenizer_json
    spec = parse_tokenizer_json(obj)
    with pytest.raises(UnsupportedConfigError):
        PipelineTokenizer.from_spec(spec)
    assert PipelineTokenizer.from_spec(spec, regex_split=True).encode_batch(texts) == [oracle.encode(t) for t in texts]
