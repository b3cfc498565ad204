"""Batches for the PreTokenizer's tests (tests/test_pretok_cpu.py on the CPU build of csrc/pretok_hd.h,
tests/test_gpu_pretokenizer.py on the device), each with the pre-tokenizer it is for, in the tuples of
tests/pretok_ref.py.  The boundary shapes are derived from the implementation's constants: a bitmap
word (and a wavefront) is SPAN bytes, a wavefront walks WAVE_TILE bytes in the script carry and a
workgroup TILE."""
import os
import random
import re

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "complexity-tokenizer_amd", "csrc")


def _constant(header, name):
    with open(os.path.join(_CSRC, header)) as f:
        return int(re.search(r"constexpr uint32_t %s = (\d+);" % name, f.read()).group(1))


# the kernels' own constants (csrc/pretok_hd.h, csrc/pretok_internal.h)
SPAN = _constant("pretok_hd.h", "kSpan")
THREADS = _constant("pretok_internal.h", "kThreads")
WAVE_TILE = _constant("pretok_internal.h", "kWaveWords") * SPAN
TILE = WAVE_TILE * (THREADS // SPAN)
CARRY_ROUND = THREADS * WAVE_TILE  # bytes k_pt_script_carry takes in one round of its loop
BOUNDS = (SPAN, WAVE_TILE, TILE)
BEHAVIORS = ("Removed", "Isolated", "MergedWithPrevious", "MergedWithNext", "Contiguous")

# every constructor and flag value
SINGLE = [("whitespace",), ("whitespace_split",), ("byte_level", False), ("byte_level", True), ("metaspace", "▁", True),
          ("metaspace", "▁", False), ("metaspace", "_", True), ("metaspace", "　", True), ("metaspace", "\U0001F600", False),
          ("punctuation",), ("digits", False), ("digits", True), ("gpt2",), ("bert",), ("char_delimiter_split", "_"),
          ("char_delimiter_split", "、"), ("unicode_scripts",)]
SPLITS = [("split", p, b, inv) for p in (r"\s", r"\d", r"\d+", "ab", "aa", r"\p{L}+", "!", r"[^\s\p{L}\p{N}]", r"[a-c一-鿿_]+", r"\.")
          for b in BEHAVIORS for inv in ((False, True) if b == "Removed" else (False,))]
SEQUENCES = [("sequence", [("whitespace",), ("punctuation",), ("digits", True)]),
             ("sequence", [("bert",), ("split", r"\d", "Contiguous", False)]),
             ("sequence", [("metaspace", "▁", True), ("unicode_scripts",)])]
EVERY = SINGLE + SPLITS + SEQUENCES

QUIRKS = ["hello, world!", "Hello, world!", "Hello世界", "hello_world_test", "Helloこんにちは",
          "hello world test", "hello! world!", "price $100 and $50", "abc123def456", "hello123world", "", " ", "  ", "\n",
          "a b c　d e f", "we'll they're I'm it's 'tis don't 'll'll", "'s", " 's", "''s", "x 'll", "a  b   c ",
          "\t\n x", "aaaaa", "aaaa", "aa", "a", "!!a!!b!!", "12 345٣٤", "abab aab", "éÉ αβγ ж א ا",
          "abc123αβ 1a2б!?", "▁a ▁", "a▁b", "\U0001F600\U00020000x", "1α", "αβa1b", "...a", "a.b..c",
          "¡hola! ¿qué?", "x、y。z", "가ᄀ กขk"]

CASES = {}


def case(f):
    CASES[f.__name__] = f
    return f


def _around(b):
    return (b - 1, b, b + 1)


@case
def straddling_whitespace_and_punctuation():
    """a multi-byte whitespace or punctuation code point across every boundary"""
    texts = []
    for b in BOUNDS:
        for k in _around(b):
            for ch in (" ", "\u3000", "\u2003", "\u2014", "\u3002", "\U0001F600"):
                for back in range(len(ch.encode())):
                    texts.append("a" * (k - back) + ch + "b c")
    return ("sequence", [("bert",)]), texts


@case
def straddling_punctuation_isolated():
    return ("punctuation",), straddling_whitespace_and_punctuation()[1]


@case
def straddling_scripts():
    return ("unicode_scripts",), straddling_whitespace_and_punctuation()[1]


@case
def word_starts_at_a_boundary():
    texts = ["x" * (k - 1) + " " + "word" for b in BOUNDS for k in _around(b)]
    texts += ["x" * (k - 3) + "　" + "word" for b in BOUNDS for k in _around(b)]
    return ("whitespace",), texts


@case
def gpt2_across_a_boundary():
    """'ll and ` ?\\p{L}+` with each of their bytes on either side"""
    texts = []
    for b in BOUNDS:
        for k in range(b - 5, b + 2):
            texts += ["a" * k + "'ll go", "a" * k + " été x", "1" * k + "'re", "." * k + " 'd", " " * k + "'ve 12"]
    return ("gpt2",), texts


@case
def byte_level_across_a_boundary():
    return ("byte_level", True), gpt2_across_a_boundary()[1] + ["'s", "é", " x", "\n", "'ll'll"]


@case
def literal_across_a_boundary():
    texts = ["x" * k + "abcé" + "y" * 3 for b in BOUNDS for k in range(b - 6, b + 2)]
    return ("split", "abcé", "Isolated", False), texts


def _runs_of_a():
    ks = sorted({k for b in BOUNDS for k in range(b - 3, b + 4)} | set(range(0, 8)))
    return ["a" * k for k in ks] + ["b" + "a" * k + "b" for k in ks]


@case
def self_overlapping_literal_removed():
    return ("split", "aa", "Removed", False), _runs_of_a()


@case
def self_overlapping_literal_removed_inverted():
    return ("split", "aa", "Removed", True), _runs_of_a()


@case
def self_overlapping_literal_merged_with_previous():
    return ("split", "aa", "MergedWithPrevious", False), _runs_of_a()


@case
def self_overlapping_literal_contiguous():
    return ("split", "aa", "Contiguous", False), _runs_of_a()


@case
def common_run_longer_than_a_tile():
    """a Latin and a Greek letter with more than a workgroup tile of Common code points between
    them, and the same run after whitespace"""
    texts = []
    for n in (SPAN + 1, WAVE_TILE + 1, TILE + 1, 2 * TILE + 7):
        texts += ["a" + "1" * n + "α", "a " + "1" * n + "α", "a" + "1" * n + "aα", "α" + "." * n + "　" + "-" * n + "a",
                  "1" * n + "a" + "2" * n + "bα"]
    return ("unicode_scripts",), texts


@case
def common_run_across_a_carry_round():
    """k_pt_script_carry keeps its running value between rounds of THREADS wavefront tiles: a silent
    run of Common code points from before a round's end into the next round, one that covers a
    whole round and more, and the same after whitespace (which forgets the script)"""
    r = CARRY_ROUND
    return ("unicode_scripts",), ["a" + "1" * (r - 700) + "b" + "2" * 1400 + "α" + "3" * (2 * r + 5) + "β" + "4" * 10 + "a",
                                  "a" + "1" * (r + 9) + " " + "2" * (r + 3) + "α" + "." * r + "a"]


@case
def a_text_that_loses_every_word_is_not_an_empty_text():
    """Metaspace makes "▁x" of "x", the split drops all of it and ByteLevel leaves the text no byte:
    it owns no word, while the empty text beside it owns what the program makes of the empty word"""
    return ("sequence", [("metaspace", "▁", True), ("split", "▁x", "Removed", True), ("byte_level", False)]), ["x", "", "x y", "x", ""]


@case
def a_text_that_loses_every_word_beside_the_empty_word():
    return ("sequence", [("split", "x", "Removed", True), ("split", "q", "Isolated", False)]), ["x", "", "xx", "axb", ""]


@case
def many_metaspaces_over_the_empty_word():
    """every Metaspace with a prefix adds a replacement: the words of the empty text are not bounded
    by a constant"""
    return ("sequence", [("metaspace", "▁", True)] * 100), ["", "a b", ""]


@case
def one_long_word():
    return ("sequence", [("whitespace",), ("split", "zz", "Removed", False), ("unicode_scripts",)]), ["a" * 70000, "b" * 70000 + " c"]


@case
def one_long_word_rewritten():
    return ("sequence", [("metaspace", "▁", True), ("byte_level", False)]), ["a" * 70000]


@case
def whitespace_only_and_empty_texts():
    return ("whitespace",), ["", "a b", "", " 　\n", "c", ""]


@case
def empty_texts_under_bert():
    return ("bert",), ["", "", "x", ""]


@case
def empty_word_through_splits():
    return ("sequence", [("split", "a", "Removed", False), ("split", r"\d+", "Isolated", False)]), ["", "b", "", "a1b", ""]


@case
def empty_word_dies_in_whitespace():
    return ("sequence", [("split", "a", "Removed", False), ("whitespace",)]), ["", "b a", ""]


@case
def empty_word_becomes_the_replacement():
    return ("sequence", [("split", "a", "Removed", False), ("metaspace", "▁", True)]), ["", "b a", "", "", "a"]


@case
def empty_word_becomes_the_replacement_and_goes_on():
    return ("sequence", [("split", "q", "Removed", False), ("metaspace", "_", True), ("punctuation",), ("split", "_", "Isolated", False)]), ["", "b a", ""]


@case
def empty_text_under_metaspace():
    return ("metaspace", "▁", True), ["", "a", "", " ", "\n"]


@case
def rejected_pattern_is_the_identity():
    return ("sequence", [("split", r"(?=a)", "Isolated", False), ("split", r"\1", "Removed", False)]), ["", "a b", "xay"]


@case
def unknown_behavior_is_removed():
    return ("split", r"\d", "isolated", False), ["a1b22c", "abc", ""]


@case
def adjacent_matches_every_behavior():
    texts = ["!!", "a!!b", "!!b", "a!!", "!a!", "a!b!!c!!!", "!", ""]
    return ("sequence", [("whitespace",)]), texts  # (the behaviours themselves run over these in the tests)


ADJACENT = adjacent_matches_every_behavior()[1]

POOLS = {
    "ascii": "abcXYZ'stmdrevl  \t\n",
    "punct_ws": "!,.-_$\u00a1\u00bf\u2014\u2026\u3001\u3002\u2e3a\u2000\u2003\u200a\u2028\u2029\u202f\u205f\u3000\u0085\u000b\u00a0\u1680\u200b a",
    "digits": "0123456789٣१１²Ⅷ a.",
    "cjk": "世界㐀豈こカㇰ가ᄀ ab　",
    "mixed_scripts": "aZéαΩжԱאاกअḀἀ 1.-",
    "four_byte": "\U00020000\U0002a700\U0002b820\U00030000\U0001F600\U0001D7CE\U00010330 a1",
}


def random_texts(pool, seed, n=1500, hi=200):
    rng = random.Random(seed)
    chars = POOLS[pool]
    return ["".join(rng.choice(chars) for _ in range(rng.randrange(0, hi + 1))) for _ in range(n)]
