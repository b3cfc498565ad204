"""The reference's Normalizer (src/normalizers.rs:43-202) restated in plain Python, for the tests of
complexity_tokenizer.Normalizer and of csrc/normalize_hd.h.

A normaliser is a tuple: ("nfc",), ("nfd",), ("nfkc",), ("nfkd",), ("lowercase",), ("strip",),
("strip_accents",), ("replace", pattern, replacement), ("prepend", s), ("append", s),
("bert", clean_text, handle_chinese_chars, strip_accents, lowercase), ("precompiled", [(from, to), ...])
and ("sequence", [normaliser, ...]).  unicodedata.normalize, str.lower and str.replace stand for the
crate's nfc()/nfd()/nfkc()/nfkd(), str::to_lowercase and str::replace; the rest is written out here.
"""
import struct
import unicodedata

# char::is_whitespace: the 25 White_Space code points.  str.strip() would also drop U+001C..U+001F.
WHITE_SPACE = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B))
                        + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
ACCENT_RANGES = ((0x0300, 0x036F), (0x1AB0, 0x1AFF), (0x1DC0, 0x1DFF), (0x20D0, 0x20FF), (0xFE20, 0xFE2F))
CHINESE_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
                  (0x2B820, 0x2CEAF), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))


def _in(ranges, c):
    return any(a <= c <= b for a, b in ranges)


def strip(text):
    a, b = 0, len(text)
    while a < b and ord(text[a]) in WHITE_SPACE:
        a += 1
    while b > a and ord(text[b - 1]) in WHITE_SPACE:
        b -= 1
    return text[a:b]


def strip_accents(text):
    return "".join(ch for ch in unicodedata.normalize("NFD", text) if not _in(ACCENT_RANGES, ord(ch)))


def clean_text(text):
    out = []
    for ch in text:
        c = ord(ch)
        if ch not in "\t\n\r" and (c <= 0x1F or 0x7F <= c <= 0x9F):
            continue
        out.append(" " if c in WHITE_SPACE else ch)
    return "".join(out)


def handle_chinese_chars(text):
    return "".join(" " + ch + " " if _in(CHINESE_RANGES, ord(ch)) else ch for ch in text)


def bert(text, clean, chinese, strip_acc, lowercase):
    if clean:
        text = clean_text(text)
    if chinese:
        text = handle_chinese_chars(text)
    text = unicodedata.normalize("NFC", text)
    if lowercase if strip_acc is None else strip_acc:
        text = strip_accents(text)
    if lowercase:
        text = text.lower()
    return text


def normalize(norm, text):
    kind = norm[0]
    if kind in ("nfc", "nfd", "nfkc", "nfkd"):
        return unicodedata.normalize(kind.upper(), text)
    if kind == "lowercase":
        return text.lower()
    if kind == "strip":
        return strip(text)
    if kind == "strip_accents":
        return strip_accents(text)
    if kind == "replace":
        return text.replace(norm[1], norm[2])
    if kind == "prepend":
        return norm[1] + text
    if kind == "append":
        return text + norm[1]
    if kind == "bert":
        return bert(text, *norm[1:])
    if kind == "precompiled":
        for a, b in norm[1]:
            text = text.replace(a, b)
        return text
    if kind == "sequence":
        for n in norm[1]:
            text = normalize(n, text)
        return text
    raise ValueError(kind)


# ---- the same normalisers as the steps of include/ctok_normalizer.h ----------------------------------

KINDS = {"nfc": 0, "nfd": 1, "nfkc": 2, "nfkd": 3, "lowercase": 4, "strip": 5, "strip_accents": 6, "replace": 7,
         "prepend": 8, "append": 9, "bert": 10, "precompiled": 11}


def flat_steps(norm):
    """[(kind, flags, a, b)] with a, b as bytes; sequences flattened"""
    kind = norm[0]
    if kind == "sequence":
        return [s for n in norm[1] for s in flat_steps(n)]
    a = b = b""
    flags = 0
    if kind == "replace":
        a, b = norm[1].encode(), norm[2].encode()
    elif kind in ("prepend", "append"):
        a = norm[1].encode()
    elif kind == "bert":
        _, clean, chinese, strip_acc, lowercase = norm
        flags = (1 if clean else 0) | (2 if chinese else 0) | (4 if lowercase else 0) | \
            (0 if strip_acc is None else 16 if strip_acc else 8)
    elif kind == "precompiled":
        for f, t in norm[1]:
            f, t = f.encode(), t.encode()
            a += struct.pack("<II", len(f), len(t)) + f + t
    return [(KINDS[kind], flags, a, b)]


def to_normalizer(norm):
    """the complexity_tokenizer.Normalizer of a tuple"""
    from complexity_tokenizer import Normalizer
    kind = norm[0]
    if kind == "sequence":
        return Normalizer.sequence([to_normalizer(n) for n in norm[1]])
    if kind == "bert":
        return Normalizer.bert(*norm[1:])
    return getattr(Normalizer, kind)(*norm[1:])
