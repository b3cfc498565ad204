"""Inputs for the end of the text (include/ctok.h, "Text buffers of the device entry points"): the
encode kernels read the aligned dword, and k_segment the words, that hold the text's last byte, so
up to 16 bytes past n_bytes are read and must be masked.  Each case is one text that ends in a
chosen last piece, placed so that the length B of the text the pipeline runs on sits on an edge:
every B mod 4, around a 64-byte bitmap word, around the end of a pre-tokenizer tile.  The tails are
what a caller's memory may hold after the text.  A tail is "live" for a case when encoding
text + tail as one text changes the tokens of the case's last piece: a kernel that let one byte of
such a tail through its mask would give other ids.

The claims (each last piece's length and class, which tails are live where) are checked on the CPU
by tests/test_text_tail_cpu.py with the Python oracle; tests/test_gpu_text_tail.py runs the cases.
"""
import functools
import json
import os
import re

from oracle import ref_py

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "complexity-tokenizer_amd", "csrc")


def tile_bytes():
    """kTile of csrc/ctok_internal.h: the bytes of a pre-tokenizer tile."""
    with open(os.path.join(CSRC, "ctok_internal.h")) as f:
        src = f.read()
    words = re.search(r"constexpr int kTileWords = (\d+);", src)
    assert words and re.search(r"constexpr int kTile = kTileWords \* 64;", src), "ctok_internal.h: kTile is defined otherwise"
    return int(words.group(1)) * 64


TILE = tile_bytes()
PAD = 16  # bytes past n_bytes that must be readable (include/ctok.h)

# plain / prefix_space / nfc as tests/test_gpu_encoding.py test_offsets_and_word_ids makes them (the
# fixture's "normalizer": null is NFC too, src/huggingface/parsing.rs:89); raw: no normaliser at
# all, the pipeline runs on the caller's text without watching for NFC
VARIANTS = ["plain", "prefix_space", "nfc", "raw"]


def variant_json(base, variant):
    obj = json.loads(json.dumps(base))
    if variant == "prefix_space":
        obj["pre_tokenizer"]["add_prefix_space"] = True
    elif variant == "nfc":
        obj["normalizer"] = {"type": "NFC"}
    elif variant == "raw":
        obj["normalizer"] = {"type": "Sequence", "normalizers": []}
    else:
        assert variant == "plain"
    return obj


TAILS = {
    "zeros": b"\x00" * 16,
    "a": b"a" * 16,
    "7": b"7" * 16,
    "bang": b"!" * 16,
    "spaces": b" " * 16,
    "s_spaces": b"s" + b" " * 15,
    "acute": b"\xcc\x81" * 8,   # U+0301: composes with a letter in front under NFC
    "cont": b"\x80" * 16,      # continuation bytes
    "lead3": b"\xe4" * 16,     # lead bytes of 3-byte code points
    "ff": b"\xff" * 16,
}
assert all(len(t) == PAD for t in TAILS.values())


def tail_str(tail):
    """The tail as text, or None where it is not UTF-8 (liveness is defined for text only)."""
    try:
        return TAILS[tail].decode("utf-8")
    except UnicodeDecodeError:
        return None


TEXT_TAILS = [k for k in TAILS if tail_str(k) is not None]

LETTERS = "etaoinshrdlucmfwypvbgkqjxz"


def letters(n, seed):
    return "".join(LETTERS[(7 * i * i + 3 * i + seed) % 26] for i in range(n))


# (name, what the text ends in, its last piece, the piece's class); classes as csrc/ctok_internal.h:
# 0: <= 8 B, 1: 9..16 B, 2: 17..32 B, 3: 33..64 B, "long": more
SHORT = [
    ("c8", " the", " the", 0),
    ("c16", " international", " international", 1),
    ("c32", " " + letters(23, 1), " " + letters(23, 1), 2),
    ("c64", " " + letters(47, 2), " " + letters(47, 2), 3),
    ("digits", " 1234567", " 1234567", 0),
    ("punct", " !?!", " !?!", 0),
    ("spaces", "   ", "   ", 0),
    ("space", " ", " ", 0),
    ("it_apostrophe", " it'", "'", 0),          # a contraction one byte short
    ("e2", " caf\u00e9", " caf\u00e9", 0),       # letters of 2, 3 and 4 bytes ending exactly at B
    ("e3", " \u4e16\u754c", " \u4e16\u754c", 0),
    ("e4", " \U00020000", " \U00020000", 0),
    ("cafe", " cafe", " cafe", 0),              # a following U+0301 composes under NFC
]
# 65 and 256 B: the dense wave tier; 257 and 1025 B: the segmented tiers; 4097 B: k_bpe_long's
# global-memory tier
LONG = [("L%d" % n, " " + letters(n - 1, n), " " + letters(n - 1, n), "long") for n in (65, 256, 257, 1025, 4097)]


def class_of(n_bytes):
    return 0 if n_bytes <= 8 else 1 if n_bytes <= 16 else 2 if n_bytes <= 32 else 3 if n_bytes <= 64 else "long"


B_MOD4 = [100, 101, 102, 103]
B_WORD = [63, 64, 65]
B_TILE = [TILE - 1, TILE, TILE + 1, 2 * TILE]

FILL = ("the quick brown fox jumps over a lazy dog while seventeen international committees deliberate about "
        "it's 1234 reasons, we're sure; extraordinarily long words notwithstanding ")


def filler(n):
    """n >= 1 bytes of ASCII words that begin and end with a letter."""
    assert n >= 1
    s = (FILL * (n // len(FILL) + 1))[:n]
    return s if s[-1].isalpha() else s[:-1] + "z"


def cases(variant):
    """[{name, text, piece, cls, B}]: B is the length of the text the pipeline runs on (the prefix
    space counted), one document."""
    lead = 1 if variant == "prefix_space" else 0
    out = []

    def add(name, end, piece, cls, B):
        n = B - lead - len(end.encode())
        if n < 1:
            return
        out.append({"name": "%s@%d" % (name, B), "text": filler(n) + end, "piece": piece, "cls": cls, "B": B})

    for name, end, piece, cls in SHORT:
        for B in B_MOD4 + B_WORD + B_TILE:
            add(name, end, piece, cls, B)
    for name, end, piece, cls in LONG:
        L = len(end)
        for B in [L + 2 + j for j in range(4)] + [b for b in B_TILE if b >= L + 2 and b not in range(L + 2, L + 6)]:
            add(name, end, piece, cls, B)
    assert max(c["B"] for c in out) <= 3 * TILE
    return out


class Oracle:
    """ref_py.RefTokenizer.encode with each word's ids computed once (the fillers repeat)."""

    def __init__(self, obj):
        self.py = ref_py.RefTokenizer(obj)
        self.word_ids = functools.lru_cache(maxsize=None)(lambda w: tuple(self.py._encode_word(w)))

    def words(self, text):
        return self.py._pre_tokenize(self.py._normalize(text, self.py.normalizer), self.py.pre_tokenizer)

    def encode(self, text):
        return [i for w in self.words(text) for i in self.word_ids(w)]

    def n_bytes(self, text):
        """Bytes of the text the pipeline runs on."""
        t = self.py._normalize(text, self.py.normalizer)
        pt = self.py.pre_tokenizer
        return len(t.encode()) + (1 if pt[0] == "ByteLevel" and pt[1] and t and not t.startswith(" ") else 0)

    def live(self, text, tail):
        """Encoding text + tail as one text changes the tokens that cover the text's last piece."""
        w1, w2 = self.words(text), self.words(text + tail_str(tail))
        return [self.word_ids(w) for w in w2[:len(w1)]] != [self.word_ids(w) for w in w1]


def capacity_cases(variant, ntok_of):
    """[(case, r)]: for a last piece of each class, the shortest texts of 70 bytes and more whose token
    counts are r = 0, 1 and 7 mod 8 (ntok_of(text) -> the oracle's token count)."""
    lead = 1 if variant == "prefix_space" else 0
    out = []
    for name, end, piece, cls in SHORT[:4] + LONG[:1]:
        for r in (0, 1, 7):
            for B in range(len(end) + 70, len(end) + 400):
                text = filler(B - lead - len(end.encode())) + end
                if ntok_of(text) % 8 == r:
                    out.append(({"name": "%s@%d" % (name, B), "text": text, "piece": piece, "cls": cls, "B": B}, r))
                    break
    return out


# the cases whose text the host entries encode after a longer "poisoning" call (call history)
HISTORY = ["c8@64", "c16@65", "c32@103", "c64@%d" % TILE, "space@%d" % TILE, "spaces@100", "it_apostrophe@102",
           "digits@63", "punct@101", "e2@%d" % (TILE + 1), "e3@63", "e4@100", "cafe@101", "L65@%d" % (TILE - 1), "L257@%d" % TILE]
WINDOWS = ["c8@63", "c32@64", "space@65", "e3@%d" % (TILE - 1), "cafe@%d" % TILE, "L257@%d" % (TILE + 1), "L4097@%d" % (2 * TILE)]
MARK_DOC = "cafe\u0301 "  # in front of a case's text: NFC composes it, so the document is normalised


def poison_docs(docs, split):
    """docs with the last one made longer: letters follow where it ended (split False), or it ends
    one character earlier and "\u00e9"s follow so that a continuation byte falls where it ended."""
    last = docs[-1]
    if split:
        k = len(last[-1].encode())
        more = last[:-1] + "x" * (k - 1) + "\u00e9" * 12
        assert more.encode()[len(last.encode())] == 0xA9
    else:
        more = last + "abcdefghijklmnopqrstuvwxyz and more"
    return docs[:-1] + [more]
