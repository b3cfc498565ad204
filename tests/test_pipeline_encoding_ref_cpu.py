"""The Encoding path of PipelineTokenizer on the CPU: the restatement tests/pipeline_encoding_ref.py on
cases worked out by hand, and csrc/pipeline_enc_hd.h, which the kernels share, by
tools/pipeline_enc_check.cpp built with g++ over a case file of a few thousand words with the
restatement's answers.  No GPU."""
import os
import random
import subprocess

import pytest

from tests import pipeline_cases as pc
from tests.pipeline_encoding_ref import PanicException, PipelineEncodingRef, find_work

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HELLO = {"h": 0, "e": 1, "l": 2, "o": 3, "he": 4, "hel": 5, "lo": 6, "[CLS]": 7, "[SEP]": 8}
HELLO_MERGES = [("h", "e"), ("he", "l"), ("l", "o")]
BERT = ("bert", ("[CLS]", 7), ("[SEP]", 8))
SPECIAL = [pc.added("[CLS]", 7, special=True), pc.added("[SEP]", 8, special=True)]


def hello_ref():
    return PipelineEncodingRef(**pc.spec(HELLO, HELLO_MERGES, ("lowercase",), ("whitespace",), None, BERT, SPECIAL))


def test_lowercase_finds_the_later_word_and_falls_back():
    e = hello_ref().encode_to_encoding("Hello hello hello")
    assert e.ids == [7, 5, 6, 5, 6, 5, 6, 8]
    # "hello" is first found at 6, then at 12; the third word misses: (17, 17)
    assert e.offsets == [(6, 9), (9, 11), (12, 15), (15, 17), (17, 17), (17, 17)]
    assert e.word_ids == [0, 0, 1, 1, 2, 2]
    # the post-processor's two ids are counted at the end; [CLS] at 0 is marked by its id
    assert e.special_tokens_mask == [1, 0, 0, 0, 0, 0, 1, 1]
    assert e.type_ids == [0] * 8 and e.attention_mask == [1] * 8
    assert e.tokens == ["hel", "lo"] * 3 and e.sequence_ids == [0] * 6
    assert find_work(["hello"] * 3, "Hello hello hello") == 11 + 6 + 0


def byte_level_ref():
    from oracle.ref_py import bytes_to_unicode
    vocab = {c: i for i, c in enumerate(bytes_to_unicode().values())}
    return PipelineEncodingRef(**pc.spec(vocab, [], None, ("byte_level", False)))


def test_fallback_inside_a_char_panics_only_before_a_word():
    ref = byte_level_ref()
    with pytest.raises(PanicException, match="^byte index 4 is not a char boundary"):
        ref.encode_to_encoding("é€")  # words "Ã©" (4 bytes, missed: ends at 4, inside "€") and "âĤ¬"
    e = ref.encode_to_encoding("é b")  # "Ã©" ends at 4 = the text's end, "Ġb" finds "b"... after the end: a miss at (4, 4)
    assert e.offsets[:2] == [(0, 2), (2, 4)] and e.offsets[-1][1] == 4


def test_pairs_restart_and_the_single_form():
    ref = hello_ref()
    e = ref.encode_to_encoding("hello", "lo hello")
    assert e.ids == [7, 5, 6, 6, 5, 6, 8]  # process(merged, None): one [SEP], at the end
    assert e.type_ids == [0, 0, 1, 1, 1, 0, 0] and e.special_tokens_mask == [1, 0, 0, 0, 0, 1, 1]
    assert e.offsets == [(0, 3), (3, 5), (0, 2), (3, 6), (6, 8)] and e.word_ids == [0, 0, 0, 1, 1]
    assert e.sequence_ids == [0, 0, 1, 1, 1]


def test_template_without_the_sequence_panics():
    sp = pc.spec(HELLO, HELLO_MERGES, None, ("whitespace",), None, ("template", "[CLS]", None, [("[CLS]", 7)]), SPECIAL)
    ref = PipelineEncodingRef(**sp)
    assert ref.encode_to_encoding("h").ids == [7] and ref.encode_to_encoding("").ids == [7]
    with pytest.raises(PanicException, match="attempt to subtract with overflow"):
        ref.encode_to_encoding("h e")


def test_call_inherits_truncation_and_padding():
    ref = hello_ref()
    out = ref.call(["hello hello", "lo"], padding="longest", truncation=True, max_length=3)
    assert [e.ids for e in out] == [[7, 5, 6], [7, 6, 8]] and out[0].overflowing[0].tokens == ["lo"]
    assert ref.call(["hello hello", "lo"], padding="longest")[1].ids == [7, 6, 8, 0, 0, 0]
    with pytest.raises(PanicException):  # four tokens, six ids: tokens[5..4]
        ref.call(["hello hello"], truncation=True, max_length=5)
    assert ref.pad_id_token() == (0, "h") and ref.model_max_length == 512
    assert [e.tokens for e in ref.call(["hello"], add_special_tokens=False)] == [["hel", "lo"]]


def hexs(b):
    return b.hex() if b else "-"


def case_file(path):
    """sequences over a small alphabet, through the restatement: normalisers that change the bytes make the
    searches miss, short texts make the fallbacks clip, multi-byte chars make them panic"""
    rng = random.Random(5)
    refs = [PipelineEncodingRef(**pc.spec(pc.CHARS, pc.CHAR_MERGES, n, p)) for n, p in (
        (("lowercase",), ("whitespace",)), (None, ("byte_level", False)), (None, ("metaspace", "▁", True)), (("nfkc",), ("bert",)),
        (("prepend", "ab "), ("whitespace",)), (("strip_accents",), ("whitespace_split",)))]
    alphabet = ["a", "b", "A", "B", " ", " ", "é", "É", "中", "😀", "ﬁ", "Ġ", "▁", "-", "aé", "ab ab"]
    n_words = n_panics = 0
    with open(path, "w") as f:
        for _ in range(1500):
            ref = rng.choice(refs)
            text = "".join(rng.choice(alphabet) for _ in range(rng.randrange(0, 24)))
            words = ref.words(text)
            panic, spans = -1, None
            try:
                spans = ref.words_with_offsets(words, text)
            except PanicException as e:
                panic = int(str(e).split()[2])
                n_panics += 1
                for k in range(len(words) - 1, -1, -1):  # the words before the one that panics
                    try:
                        spans = ref.words_with_offsets(words[:k], text)
                        break
                    except PanicException:
                        pass
            work = find_work(words, text) if panic < 0 else -1
            f.write("S %s %d %d %d\n" % (hexs(text.encode()), len(spans), panic, work))
            for w, a, b in spans:
                f.write("W %s %d %d\n" % (hexs(w.encode()), a, b))
            n_words += len(spans)
            if panic < 0:
                e = ref.encode_single_to_encoding(text, 0)
                for wi, (w, a, b) in enumerate(spans):
                    ks = [k for k in range(len(e.ids)) if e.word_ids[k] == wi]
                    lens = [len(ref.id_to_token_map.get(e.ids[k], "").encode()) for k in ks]
                    f.write("T %d %d %d %s\n" % (a, b, len(ks), " ".join(map(str, lens + [x for k in ks for x in e.offsets[k]]))))
    return n_words, n_panics


def test_pipeline_enc_check(tmp_path):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "pipeline_enc_check.cpp")
    exe = str(tmp_path / "pipeline_enc_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    cases = str(tmp_path / "cases.txt")
    n_words, n_panics = case_file(cases)
    assert n_words >= 3000 and n_panics >= 10
    out = subprocess.run([exe, cases], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok (1500 sequences"), out.stdout[-2000:] + out.stderr[-2000:]
