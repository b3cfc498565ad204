"""Patterns and helpers shared by the tests of `split(..., regex=True)`: tests/test_regex_dfa_cpu.py
(the compiler and the rules on the CPU) and tests/test_gpu_regex_split.py (the kernels).

A pre-tokenizer is a tuple as in tests/pretok_ref.py; here every `split` of it is made with the
regex flag (CTOK_PRETOK_REGEX), which the restatement does not know and does not need: it runs
every pattern through the `regex` module anyway.
"""
import struct

from oracle import rust_regex
from tests import pretok_ref as ref

REGEX_FLAG = 16  # include/ctok_pretokenizer.h CTOK_PRETOK_REGEX

GPT2_LIKE = r"'s|'t|'re| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+"

# patterns the engine takes (none is a literal or a class atom), the issue's ten first
ACCEPTED = [
    r"\p{N}{1,3}", r"[0-9][0-9][0-9]", r"a|ab", r"ab|a", r"(ab|a)(bc|c)?", r"a+?b?", r"[^\n]+?b", r"\d+\.\d+|\d+", r"x{0,2}y",
    GPT2_LIKE,
    r".", r".+", r"..", r"(?:\d)+", r"(?:ab)+c?", r"\s+\S", r"(a|b)c{2,}", r"a{2}", r"a{2,}?", r"a{1,3}?b", r"\s\s", r"a\s", r"\s+?",
    r"[a-z][0-9]", r"[^a]b", r"\P{L}\p{L}", r"\D\d", r"\S{2,3}", r"(?:a|b|ab)+", r"a(|b)c", r"(a?)+b", r"(?:a??b)+", r"\p{L}+'\p{L}+",
    r"[一-鿿]{2}", r"é+|世界?", r" ?[^\s\p{L}\p{N}]+[\r\n]*", r"\s*[\r\n]+|\s+", r"[^\r\n\p{L}\p{N}]?\p{L}+", r"(?:\.|,)\d",
    r"\d{1,3}(?:,\d{3})+",
]

# a pattern and the construct its refusal names
REFUSED = [
    ("", "empty string"), ("a*", "empty string"), ("a?", "empty string"), (r"\s*", "empty string"), ("(a|)", "empty string"),
    ("(a*)+", "empty string"), ("a{0,3}", "empty string"), ("(?:a|b*)", "empty string"), ("()", "empty string"),
    ("^a", "anchor"), ("a$", "anchor"), (r"\Aa", "anchor"), (r"a\z", "anchor"), (r"\bfoo", "word boundary"), (r"a\B", "word boundary"),
    (r"\<a", "word boundary"), (r"\w", r"\w"), (r"\W+", r"\W"), ("(?i)a", "flag"), ("(?P<n>a)", "flag"), ("[[:alpha:]]", "POSIX"),
    ("[a[b]]", "nested"), ("[a&&b]", "set operation"), ("[a~~b]", "set operation"), (r"\pL", r"\p"), (r"\p{Lu}", r"\p"),
    (r"\P{Greek}x", r"\P"), ("[a-]", "'-'"), (r"a\x41", "escape"),
]


def with_regex(steps):
    """flat steps (kind, flags, a, cp) with the regex flag on every `split`"""
    return [(k, f | REGEX_FLAG if k == ref.KINDS["split"] else f, a, cp) for k, f, a, cp in steps]


def pack_steps(pt):
    """the program as tools/pretok_check.cpp reads it, every `split` with the regex flag"""
    prog = with_regex(ref.flat_steps(pt))
    return struct.pack("<Q", len(prog)) + b"".join(
        struct.pack("<IIIQ", k | (0x100 if k == ref.KINDS["split"] and not rust_regex.compiles(a.decode("utf-8")) else 0), f, cp, len(a)) + a
        for k, f, a, cp in prog)


def to_pretokenizer(pt, device=0):
    """the PreTokenizer of a tuple, every `split` with regex=True"""
    from complexity_tokenizer import PreTokenizer as P
    kind = pt[0]
    if kind == "sequence":
        return P.sequence([to_pretokenizer(sub, device) for sub in pt[1]], device=device)
    if kind == "split":
        return P.split(pt[1], pt[2], pt[3], device=device, regex=True)
    return getattr(P, kind)(*pt[1:], device=device)
