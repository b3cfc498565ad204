"""The reference's PreTokenizer (src/pretokenizers.rs:69-594) restated in plain Python, for the tests
of complexity_tokenizer.PreTokenizer and of csrc/pretok_hd.h.

A pre-tokenizer is a tuple: ("whitespace",), ("whitespace_split",), ("byte_level", add_prefix_space),
("metaspace", replacement, add_prefix_space), ("punctuation",), ("digits", individual_digits),
("gpt2",), ("bert",), ("char_delimiter_split", delimiter), ("unicode_scripts",),
("split", pattern, behavior, invert) and ("sequence", [pre-tokenizer, ...]).  The `regex` module
stands for the Rust regex crate (as oracle/ref_py.py has it for GPT2_PATTERN); a pattern the crate
rejects (oracle/rust_regex.py) leaves the word as it is.
"""
import struct

import regex

from oracle import rust_regex
from oracle.ref_py import GPT2_PATTERN, bytes_to_unicode

# char::is_whitespace: the 25 White_Space code points
WHITE_SPACE = frozenset([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B))
                        + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000])
# is_unicode_punctuation, :227-240 (char::is_ascii_punctuation is its first four ranges)
PUNCT_RANGES = ((0x21, 0x2F), (0x3A, 0x40), (0x5B, 0x60), (0x7B, 0x7E), (0xA1, 0xBF), (0x2000, 0x206F), (0x2E00, 0x2E7F),
                (0x3000, 0x303F))
# is_chinese_char, :482-496
CHINESE_RANGES = ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF), (0x2A700, 0x2B73F), (0x2B740, 0x2B81F),
                  (0x2B820, 0x2CEAF), (0x2CEB0, 0x2EBEF), (0x30000, 0x3134F), (0xF900, 0xFAFF), (0x2F800, 0x2FA1F))
# get_unicode_script, :566-594: the match arms in order (the first that holds wins)
COMMON, UNKNOWN = "Common", "Unknown"
SCRIPT_ARMS = (
    ("Latin", ((0x41, 0x7A), (0xC0, 0x24F), (0x1E00, 0x1EFF))),
    ("Greek", ((0x370, 0x3FF), (0x1F00, 0x1FFF))),
    ("Cyrillic", ((0x400, 0x4FF), (0x500, 0x52F))),
    ("Arabic", ((0x600, 0x6FF), (0x750, 0x77F), (0x8A0, 0x8FF))),
    ("Hebrew", ((0x590, 0x5FF),)),
    ("Han", ((0x4E00, 0x9FFF), (0x3400, 0x4DBF), (0x20000, 0x2A6DF))),
    ("Hiragana", ((0x3040, 0x309F),)),
    ("Katakana", ((0x30A0, 0x30FF), (0x31F0, 0x31FF))),
    ("Hangul", ((0xAC00, 0xD7AF), (0x1100, 0x11FF), (0x3130, 0x318F))),
    ("Thai", ((0xE00, 0xE7F),)),
    (COMMON, ((0x0, 0x40), (0x5B, 0x60), (0x7B, 0xBF), (0x2000, 0x206F), (0x3000, 0x303F))),
)
BEHAVIORS = ("Removed", "Isolated", "MergedWithPrevious", "MergedWithNext", "Contiguous")
KINDS = {"whitespace": 0, "whitespace_split": 1, "byte_level": 2, "metaspace": 3, "punctuation": 4, "digits": 5, "gpt2": 6,
         "bert": 7, "char_delimiter_split": 8, "unicode_scripts": 9, "split": 10}
_BYTE_ENCODER = bytes_to_unicode()


def _in(ranges, c):
    return any(a <= c <= b for a, b in ranges)


def is_ws(ch):
    return ord(ch) in WHITE_SPACE


def is_punct(ch):
    return _in(PUNCT_RANGES, ord(ch))


def script_of(ch):
    for name, ranges in SCRIPT_ARMS:
        if _in(ranges, ord(ch)):
            return name
    return UNKNOWN


def _split_on(text, drop):
    """str::split(pred).filter(non-empty)"""
    out, cur = [], []
    for ch in text:
        if drop(ch):
            if cur:
                out.append("".join(cur))
            cur = []
        else:
            cur.append(ch)
    if cur:
        out.append("".join(cur))
    return out


def _isolating(text, drop, isolate):
    """the loops of punctuation_split (:203-224) and bert_pretokenize (:445-479)"""
    words, cur = [], []
    for ch in text:
        if drop(ch):
            if cur:
                words.append("".join(cur))
                cur = []
        elif isolate(ch):
            if cur:
                words.append("".join(cur))
                cur = []
            words.append(ch)
        else:
            cur.append(ch)
    if cur:
        words.append("".join(cur))
    return words


def byte_level(text, add_prefix_space):  # :158-185
    if add_prefix_space and text and not text.startswith(" "):
        text = " " + text
    words = []
    for m in GPT2_PATTERN.finditer(text):
        enc = "".join(_BYTE_ENCODER[b] for b in m.group(0).encode("utf-8"))
        if enc:
            words.append(enc)
    return words


def metaspace(text, replacement, add_prefix_space):  # :188-200
    if add_prefix_space:
        text = replacement + text
    return _split_on(text.replace(" ", replacement), lambda ch: is_ws(ch) and ch != replacement)


def digits(text, individual):  # :243-275
    words, cur, in_digits = [], [], False
    for ch in text:
        d = "0" <= ch <= "9"
        if d != in_digits:
            if cur:
                words.append("".join(cur))
                cur = []
            in_digits = d
        if d and individual:
            if cur:
                words.append("".join(cur))
                cur = []
            words.append(ch)
        else:
            cur.append(ch)
    if cur:
        words.append("".join(cur))
    return words


def unicode_scripts(text):  # :508-546
    words, cur, script = [], [], None
    for ch in text:
        if is_ws(ch):
            if cur:
                words.append("".join(cur))
                cur = []
                script = None
            continue
        s = script_of(ch)
        if script is None or script == s or s == COMMON:
            cur.append(ch)
            if script is None and s != COMMON:
                script = s
        else:
            if cur:
                words.append("".join(cur))
            cur = [ch]
            script = s
    if cur:
        words.append("".join(cur))
    return words


def split(text, pattern, behavior, invert):  # regex_split_with_behavior, :298-433
    if not rust_regex.compiles(pattern):
        return [text]
    ms = [(m.start(), m.end()) for m in regex.finditer(pattern, text)]
    if not ms:
        return [text]
    out, last = [], 0
    if behavior == "Isolated":
        for a, b in ms:
            if a > last:
                out.append(text[last:a])
            out.append(text[a:b])
            last = b
        if last < len(text):
            out.append(text[last:])
    elif behavior == "MergedWithPrevious":
        for a, b in ms:
            if a > last:
                out.append(text[last:a] + text[a:b])
            elif out:
                out.append(out.pop() + text[a:b])
            else:
                out.append(text[a:b])
            last = b
        if last < len(text):
            out.append(text[last:])
    elif behavior == "MergedWithNext":
        pending = None
        for a, b in ms:
            if a > last:
                out.append((pending or "") + text[last:a])
            elif pending is not None:
                out.append(pending)
            pending = text[a:b]
            last = b
        if last < len(text):
            out.append((pending or "") + text[last:])
        elif pending is not None:
            out.append(pending)
    elif behavior == "Contiguous":
        cur = ""
        for a, b in ms:
            if a > last:
                if cur:
                    out.append(cur)
                    cur = ""
                out.append(text[last:a])
            cur += text[a:b]
            last = b
        if cur:
            out.append(cur)
        if last < len(text):
            out.append(text[last:])
    else:  # Removed, and every string that names no behaviour (components.rs:154-160)
        for a, b in ms:
            if invert:
                if a > last:
                    out.append(text[last:a])
            else:
                out.append(text[a:b])
            last = b
        if invert and last < len(text):
            out.append(text[last:])
    return [w for w in out if w]


def pre_tokenize(pt, text):
    kind = pt[0]
    if kind in ("whitespace", "whitespace_split"):
        return _split_on(text, is_ws)
    if kind == "byte_level":
        return byte_level(text, pt[1])
    if kind == "metaspace":
        return metaspace(text, pt[1], pt[2])
    if kind == "punctuation":
        return _isolating(text, lambda ch: False, is_punct)
    if kind == "digits":
        return digits(text, pt[1])
    if kind == "gpt2":
        return [m.group(0) for m in GPT2_PATTERN.finditer(text)]
    if kind == "bert":
        return _isolating(text, is_ws, lambda ch: _in(CHINESE_RANGES, ord(ch)) or is_punct(ch))
    if kind == "char_delimiter_split":
        return _split_on(text, lambda ch: ch == pt[1])
    if kind == "unicode_scripts":
        return unicode_scripts(text)
    if kind == "split":
        return split(text, pt[1], pt[2], pt[3])
    if kind == "sequence":  # :114-124
        words = [text]
        for sub in pt[1]:
            words = [w for word in words for w in pre_tokenize(sub, word)]
        return words
    raise ValueError(kind)


def flat_steps(pt):
    """(kind, flags, a: bytes, cp) of include/ctok_pretokenizer.h, sequences flattened"""
    kind = pt[0]
    if kind == "sequence":
        return [s for sub in pt[1] for s in flat_steps(sub)]
    if kind in ("byte_level", "digits"):
        return [(KINDS[kind], 1 if pt[1] else 0, b"", 0)]
    if kind == "metaspace":
        return [(KINDS[kind], 1 if pt[2] else 0, b"", ord(pt[1]))]
    if kind == "char_delimiter_split":
        return [(KINDS[kind], 0, b"", ord(pt[1]))]
    if kind == "split":
        b = BEHAVIORS.index(pt[2]) if pt[2] in BEHAVIORS else 0
        return [(KINDS[kind], b | (8 if pt[3] else 0), pt[1].encode("utf-8"), 0)]
    return [(KINDS[kind], 0, b"", 0)]


def pack_steps(pt):
    """the program as tools/pretok_check.cpp reads it (0x100: a pattern the Rust crate rejects)"""
    prog = flat_steps(pt)
    return struct.pack("<Q", len(prog)) + b"".join(
        struct.pack("<IIIQ", k | (0x100 if k == KINDS["split"] and not rust_regex.compiles(a.decode("utf-8")) else 0), f, cp, len(a)) + a
        for k, f, a, cp in prog)


def to_pretokenizer(pt, device=0):
    from complexity_tokenizer import PreTokenizer as P
    kind = pt[0]
    if kind == "sequence":
        return P.sequence([to_pretokenizer(sub, device) for sub in pt[1]], device=device)
    if kind == "split":
        return P.split(pt[1], pt[2], pt[3], device=device)
    return getattr(P, kind)(*pt[1:], device=device)
