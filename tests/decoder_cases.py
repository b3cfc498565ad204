"""Decoders and token lists for the tests of complexity_tokenizer.Decoder (tests/decoder_ref.py has
the decoders' form): every variant at its defaults and at odd arguments, the token lists behind the
quirks of src/decoders.rs, and seeded random token lists from four pools."""
import random

DEFAULTS = [
    ("byte_level",), ("metaspace", "▁", True), ("wordpiece", "##", True), ("bpe", "</w>"), ("ctc", "<pad>", None), ("fuse",),
    ("strip", " ", 0, 0), ("replace", "a", "b"),
]
ODD = [
    ("metaspace", "▁", False), ("metaspace", " ", True), ("metaspace", "_", True), ("metaspace", "𝄞", True),
    ("wordpiece", "##", False), ("wordpiece", "", True), ("wordpiece", "é", True), ("wordpiece", "#", False),
    ("bpe", ""), ("bpe", "é"), ("bpe", " "),
    ("ctc", "<pad>", "|"), ("ctc", "", None), ("ctc", "<pad>", ""), ("ctc", "|", "|"), ("ctc", "", ""), ("ctc", "a", "b"),
    ("strip", "_", 1, 1), ("strip", "_", 2, 2), ("strip", "_", 5, 0), ("strip", "é", 1, 3), ("strip", "▁", 10 ** 6, 10 ** 6),
    ("strip", " ", 0, 2 ** 64 - 1), ("strip", "a", 3, 0),
    ("replace", "", "-"), ("replace", "aa", "b"), ("replace", "a", ""), ("replace", "", ""), ("replace", "é", "▁▁"),
    ("replace", "aba", "x"), ("replace", " ", "  "), ("replace", "##", "é"),
]
SEQUENCES = [
    ("sequence", []),
    ("sequence", [("fuse",), ("ctc", "<pad>", "")]),
    ("sequence", [("fuse",), ("bpe", "x")]),
    ("sequence", [("sequence", []), ("wordpiece", "##", True)]),
    ("sequence", [("wordpiece", "##", False), ("sequence", [("replace", " ", "_"), ("strip", "_", 1, 1)])]),
    ("sequence", [("replace", "▁", " "), ("byte_level",), ("strip", " ", 1, 0)]),
    ("sequence", [("ctc", "<pad>", "|"), ("replace", "", "."), ("metaspace", ".", True)]),
    ("sequence", [("byte_level",), ("byte_level",)]),
]
EVERY = DEFAULTS + ODD + SEQUENCES

# the token lists behind the worked examples, the empty shapes, and tokens of one class of bytes
QUIRKS = [
    [], [""], ["", ""],
    ["", "a", "##", "b", ".", "'", "c"], ["x", "", "y"], ["##a", "b"], ["a", " ", "."], ["a", "'", "b"],
    ["a</w>", "b", "</w>", "\u3000"],
    ["H", "H", "E", "<pad>", "L", "L", "O", "|", "W"], ["a", "<pad>", "a", "a", "|", "a"],
    ["___"], ["_a", "_"], ["abc"], ["aaa"], ["a", "aa", "a"], ["ab", "ab", "a"],
    ["▁Hello", "▁world"], [" ▁", "▁"], ["▁"], [" "], ["Hello", "##world"], ["ĠHello", "Ġworld"], ["Hello", " ", "World"],
    ["_Hello_"], ["x", "x", "xx", " ", "x"],
    [" ", ".", ",", "!", "?", ":", ";", "'"], [" .", " ,", "' ", " '", "  ", "''", ". ."], [" ' ", "' '", " ' ' "], ["'", " ", "'", " ", "."],
    ["a", " ", " ", ".", " ", "'", " ", "b"],
    [" ", "\t", "\u3000", "\u0085"], ["a", "\u0085"], ["a", "\u00a0", "\u2003", "\u1680"], ["\u3000", "a", "\u3000"], ["a \n"],
    # ByteLevel: a UTF-8 sequence split across tokens, and documents that end inside one
    ["Ã", "©"], ["â", "Ĥ", "¬"], ["â", "Ĥ"], ["ð", "Ł", "A", "Ģ"], ["ðŁ", "ĺĢ"], ["ðŁĺ"], ["Ã"], ["A", "Ģ"], ["é", "▁", "\x7f", "\x00", "\u00ad", "\u00a0"],
    ["ł", "Ń", "Ġ", "ń", "Ą"], ["Ãł", "¡", "ÿ"],
    ["##", "##", "a"], ["##"], ["a", "##"], ["é", "éa", "aé"], ["</w>", "</w>"], ["a</w>", "</w>b", "c</w>"], ["<pad>", "<pad>"], ["|", "|"],
    ["", "", "a", "", "a"],
]

_VOCAB = ["the", "##ing", "##s", "un", "able</w>", "er</w>", "low", "est", "</w>", "##", "<pad>", "|", "[UNK]", "a", "b", "ab", "aa",
          "é", "éa", "x", "▁", "▁the", "_", "__", ""]
_SET = [" ", ".", ",", "!", "?", ":", ";", "'", " .", "' ", " '", "  ", "a"]
_BYTEMAP = ["Ġ", "Ã", "©", "â", "Ĥ", "¬", "ð", "Ł", "ĺ", "Ģ", "A", "z", "Ċ", "ł", "Ń", "ń", "¡", "ÿ", "\u00ad", "\x00", " ", "▁", "é"]
_MIXED = ["hello", "мир", "世界", "שלום", "😀", "é", " ", "\u3000", "\u0085", "\u00a0", "\n", "a", "_", "▁", "é", "ab", "aba",
          "</w>", "##"]
POOLS = {"vocab": _VOCAB, "set_bytes": _SET, "byte_map": _BYTEMAP, "mixed": _MIXED}


def random_token_lists(pool, seed, n, max_tokens):
    rng = random.Random("%s/%d" % (pool, seed))
    items = POOLS[pool]
    out = []
    for _ in range(n):
        k = rng.randrange(0, max_tokens + 1) if rng.random() < 0.5 else rng.randrange(0, 8)
        out.append([rng.choice(items) for _ in range(k)])
    return out


# Things that must be decided across the boundary between two workgroups' tiles.  (glued to the padding
# token?, tokens, the bytes of the thing at their start).  "y" is in no rule's string and is ASCII, so
# every op before the one under test copies the padding byte for byte: WordPiece (no prefix, first
# token), BPE (no suffix) and ByteLevel's first pass leave the thing at the same byte in the next op's
# input as in the batch.
STRADDLERS = [
    (True, ["é", "x"], 2), (True, ["世界"], 3), (True, ["😀"], 4),                     # a multi-byte char
    (True, ["##", "b"], 2), (True, ["##b", "##"], 2),                               # a ## prefix (Replace, Strip see it as bytes)
    (True, ["</w>", "c</w>"], 4), (True, ["a</w>"], 5),                             # a </w> suffix
    (True, ["aaa", "a"], 3), (True, ["éa"], 3), (True, ["▁▁x"], 6), (True, ["yy"], 2),  # a Replace match, the Metaspace replacement
    (True, ["Ã", "©"], 4), (True, ["â", "Ĥ"], 4), (True, ["ðŁ", "ĺ"], 6),           # ByteLevel: a char, and invalid units of 2 and 3 bytes
    (True, [" .", " '", "' "], 2), (True, ["\u3000"], 3), (True, ["a\u2003\u2003"], 7),  # clean-up patterns, trim_end
]
# what ByteLevel's first pass makes of a straddler's start: the bytes of the thing in the second pass's input
BYTE_LEVEL_SPANS = {"Ã": 2, "â": 2, "ðŁ": 3}


def straddling(at):
    """Documents, each for a batch of its own, whose thing has bytes on both sides of byte `at` of the
    batch (a multiple of the tile): [(document, first byte of the thing, its length)]."""
    out = []
    for glued, toks, span in STRADDLERS:
        for back in range(1, span):
            pad = "y" * (at - back)
            doc = [pad + toks[0]] + toks[1:] if glued else [pad] + toks
            start = len(pad.encode("utf-8"))
            assert start < at < start + span and "".join(doc).encode("utf-8")[start:start + span] == "".join(toks).encode("utf-8")[:span]
            out.append((doc, start, span))
    return out


def straddling_tokens(at):
    """Documents, each for a batch of its own, whose interesting tokens start at token `at` of the batch:
    with back = 0 the token at `at` opens a tile and the neighbour it is compared with closes the one
    before; 1 and 2 put the pair and the prefixed token on either side."""
    out = []
    for back in (0, 1, 2):
        for fill in ("a", "<pad>", ""):
            doc = [fill] * (at - back) + ["a", "a", "##b", "a", "<pad>", "a", "</w>", "|", "|", "x</w>", "a"]
            assert len(doc) > at
            out.append(doc)
    return out


def set_run_across(at, n, seed):
    """One token with a run of exactly n set bytes that has bytes on both sides of byte `at`: under
    WordPiece the one token is the clean-up's input as it stands."""
    rng = random.Random(seed)
    run = "".join(rng.choice(" .,!?:;'") for _ in range(n))
    start = at - n // 2
    doc = ["y" * start + run + "y"]
    assert start < at < start + n and start // 256 != (start + n - 1) // 256
    return doc
