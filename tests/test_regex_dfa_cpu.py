"""The general `split` engine on the CPU: csrc/regex_dfa.cpp (pattern -> DFA) and the rules that run it
(csrc/pretok_hd.h dfa_len, dfa_walk), through two stand-alone tools built with g++ and the address
and undefined-behaviour sanitizers.  tools/regex_dfa_check.cpp gives every start's match and the
resolved chain of a batch, checked against the `regex` module (which stands for the Rust crate, as
in tests/pretok_ref.py); tools/pretok_check.cpp takes whole programs whose `split` steps carry the
regex flag through the rules the kernels run, checked against tests/pretok_ref.py.  No GPU."""
import os
import random
import struct
import subprocess

import pytest
import regex

from oracle import rust_regex
from tests import pretok_cases as pc
from tests import pretok_ref as ref
from tests import regex_split_cases as rc
from tests.test_pretok_cpu import PATTERNS as GATE_ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "complexity-tokenizer_amd")
IN_MATCH, MATCH_START = 1, 2  # pretok_hd.h kInMatch, kMatchStart

HAND = ["", "a", "ab", "abc", "abab", "aab", "abcbc", "aaab", "xxxy", "xxy", "y", "1234567", "12,345,678", "3.14 2.", "1.5.25",
        "it's we're don't 's't", "  a  \n\n b", "éé世界世", "世界世界世", "\n\nb", "ab\nb", "a  b", "x1y22z333", "abcc accc bc",
        "٣٤٥٦ 1２3", "aaaa", "a 　b", "\U0001F600b\U0001F600", "l'été d'or"]


def _build(tmp_path_factory, name):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(PKG, "tools", name + ".cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def dfa_tool(tmp_path_factory):
    return _build(tmp_path_factory, "regex_dfa_check")


@pytest.fixture(scope="module")
def prog_tool(tmp_path_factory):
    return _build(tmp_path_factory, "pretok_check")


@pytest.fixture(scope="module")
def texts():
    out = list(HAND)
    for i, pool in enumerate(sorted(pc.POOLS)):
        out += pc.random_texts(pool, 977 + i, 60, 40)
    rng = random.Random(3)
    out += ["".join(rng.choice("ab c1 2.\n'sxyé世٣,") for _ in range(rng.randrange(0, 40))) for _ in range(300)]
    return out


def run_dfa(tool, pattern, raw, cap=None):
    """(len[], mark[], over) of the packed batch"""
    off = [0]
    for r in raw:
        off.append(off[-1] + len(r))
    p = pattern.encode("utf-8")
    inp = struct.pack("<Q", len(p)) + p + struct.pack("<Q", len(raw)) + struct.pack("<%dQ" % (len(raw) + 1), *off) + b"".join(raw)
    r = subprocess.run([tool] + (["--cap", str(cap)] if cap is not None else []), input=inp, capture_output=True)
    assert r.returncode == 0, (pattern, r.returncode, r.stderr[-2000:])
    n = off[-1]
    assert len(r.stdout) == 5 * n + 4
    return off, struct.unpack_from("<%dI" % n, r.stdout), r.stdout[4 * n:5 * n], struct.unpack_from("<I", r.stdout, 5 * n)[0]


def plan(tool, pattern):
    r = subprocess.run([tool, "--plan", pattern], capture_output=True, check=True)
    head, reason = r.stdout.decode("utf-8").split("\n")[:2]
    gate, symbols, states, nfa, cyclic, longest = map(int, head.split())
    return {"gate": gate, "n_symbols": symbols, "n_states": states, "n_nfa": nfa, "cyclic": bool(cyclic), "longest_match": longest,
            "reason": reason}


def test_enough_patterns():
    assert len(rc.ACCEPTED) >= 30 and len(set(rc.ACCEPTED)) == len(rc.ACCEPTED)


@pytest.mark.parametrize("pattern", rc.ACCEPTED)
def test_match_ends_and_chain(dfa_tool, texts, pattern):
    """Every start's match is `regex`'s match(t, i) (leftmost-first: the same priorities), and the
    marks of the walked chains are finditer's matches."""
    assert rust_regex.compiles(pattern)
    rx = regex.compile(pattern)
    assert plan(dfa_tool, pattern)["gate"] == 4
    off, length, mark, over = run_dfa(dfa_tool, pattern, [t.encode("utf-8") for t in texts])
    assert over == 0xFFFFFFFF
    for k, t in enumerate(texts):
        at = [0]  # the byte offset of every code point, and of the end
        for ch in t:
            at.append(at[-1] + len(ch.encode("utf-8")))
        want_len = [0] * at[-1]
        for i in range(len(t)):
            m = rx.match(t, i)
            if m:
                want_len[at[i]] = at[m.end()] - at[i]
        want_mark = [0] * at[-1]
        for m in rx.finditer(t):
            for b in range(at[m.start()], at[m.end()]):
                want_mark[b] = IN_MATCH
            want_mark[at[m.start()]] |= MATCH_START
        assert list(length[off[k]:off[k + 1]]) == want_len, (pattern, t)
        assert list(mark[off[k]:off[k + 1]]) == want_mark, (pattern, t)


def test_the_work_bound_counts_code_points(dfa_tool):
    """a run of exactly the cap passes, one code point more raises the flag at its start; a pattern
    with bounded matches has no cap"""
    for word, over in (("é" * 5, 0xFFFFFFFF), ("é" * 6, 0), ("ab\n" + "é" * 5, 0xFFFFFFFF)):
        assert run_dfa(dfa_tool, ".+", [word.encode("utf-8")], cap=5)[3] == over
    assert run_dfa(dfa_tool, ".+", [b"ab", "é".encode("utf-8") * 6, b"abcdefg"], cap=5)[3] == 2
    assert run_dfa(dfa_tool, r"\p{N}{1,3}", [b"1234567890"], cap=2)[3] == 0xFFFFFFFF


# every "unsupported" row of tests/test_pretok_cpu.py PATTERNS under the regex flag: 4 = a DFA, 3 = still refused
UNSUPPORTED_NOW = {
    "": 3, "a|b": 4, "(a)": 4, ".": 4, "^a": 3, "a$": 3, r"\w": 3, r"\w+": 3, r"\bfoo": 3, "a*": 3, "a?": 3, r"\s*": 3, r"\s+?": 4,
    r"\d{2}": 4, "(?i)a": 3, r"\s\s": 4, r"a\s": 4, "[a-z][0-9]": 4, "[[:alpha:]]": 3, "[a&&b]": 3, r"\pL": 3, r"\p{Lu}": 3, r"\<a": 3,
    "[a-]": 3, "[" + "".join(chr(0x61 + i) + "," for i in range(17))[:-1] + "]": 4,
}


def test_gate_table(dfa_tool):
    """Gates 0..2 are what they were; every pattern no earlier gate takes is a DFA or still refused
    with a reason; the library (no device needed) says the same as the tool, and its old call is
    unchanged."""
    from complexity_tokenizer import PreTokenizer, _native
    names = {"rejected": 0, "literal": 1, "class": 2, "unsupported": 3}
    assert {p for p, g in GATE_ROWS if g == "unsupported"} == set(UNSUPPORTED_NOW)
    for pattern, gate in GATE_ROWS:
        lib = PreTokenizer.split_plan(pattern)
        raw = pattern.encode("utf-8")
        assert _native.lib.ctok_pretok_split_class(raw, len(raw)) == names[gate]
        if gate == "rejected":
            assert lib["gate"] == "rejected" and lib["reason"]
            continue
        want = UNSUPPORTED_NOW.get(pattern, names[gate])
        got = plan(dfa_tool, pattern)
        assert got["gate"] == want, (pattern, got)
        assert lib["gate"] == ("rejected", "literal", "class", "unsupported", "dfa")[want], (pattern, lib)
        assert bool(got["reason"]) == (want == 3) and lib["reason"] == got["reason"]
        for k in ("n_symbols", "n_states", "n_nfa", "cyclic", "longest_match"):
            assert lib[k] == got[k], (pattern, k)
        if want == 4:
            assert 2 <= got["n_symbols"] <= 64 and 1 <= got["n_states"] <= 4096 and got["cyclic"] == (got["longest_match"] == 0)


@pytest.mark.parametrize("pattern,construct", rc.REFUSED)
def test_refused_loudly(dfa_tool, pattern, construct):
    if not rust_regex.compiles(pattern):
        pytest.fail("the row is for a pattern the crate compiles: %r" % pattern)
    got = plan(dfa_tool, pattern)
    assert got["gate"] == 3 and construct in got["reason"], got
    from complexity_tokenizer import PreTokenizer, UnsupportedConfigError
    with pytest.raises(UnsupportedConfigError) as e:
        PreTokenizer.split(pattern, "Isolated", regex=True, device=1 << 20)  # (the pattern is judged before the device)
    assert construct in str(e.value) and (not pattern or pattern in str(e.value))


def test_longest_match_and_cycles(dfa_tool):
    for pattern, longest in ((r"\p{N}{1,3}", 3), ("[0-9][0-9][0-9]", 3), ("ab|a", 2), ("a|ab", 1), ("(ab|a)(bc|c)?", 4), ("x{0,2}y", 3),
                             (r"\d{1,3}(?:,\d{3}){2}", 11)):
        got = plan(dfa_tool, pattern)
        assert not got["cyclic"] and got["longest_match"] == longest, (pattern, got)
    for pattern in (".+", r"\d+\.\d+|\d+", "(?:ab)+c?", rc.GPT2_LIKE, "a+?b", "(a|b)c{2,}"):
        assert plan(dfa_tool, pattern)["cyclic"], pattern


def test_caps_at_their_edges(dfa_tool):
    """4096 DFA states, 2^14 NFA states and 64 symbols pass; one more of each is refused"""
    got = plan(dfa_tool, "a{4095}")  # the start and one state per `a`
    assert got["gate"] == 4 and got["n_states"] == 4096 and got["longest_match"] == 4095
    got = plan(dfa_tool, "a{4096}")
    assert got["gate"] == 3 and "4096 DFA states" in got["reason"]
    branch = "(?:a|a|a|a|a|a|a|a)"  # 8 characters and 7 splits a copy, and the match state
    got = plan(dfa_tool, branch + "{1092}")
    assert got["gate"] == 4 and got["n_nfa"] == 15 * 1092 + 1 <= 1 << 14
    got = plan(dfa_tool, branch + "{1093}")
    assert 15 * 1093 + 1 > 1 << 14 and got["gate"] == 3 and "16384 NFA states" in got["reason"]
    han = [chr(0x4E00 + i) for i in range(63)]  # every character its own symbol, the rest, the ill-formed byte
    got = plan(dfa_tool, "|".join(han[:62]))
    assert got["gate"] == 4 and got["n_symbols"] == 64
    got = plan(dfa_tool, "|".join(han))
    assert got["gate"] == 3 and "64 symbols" in got["reason"]


# ---- whole programs through the rules the kernels run --------------------------------------------------------

def run_prog(tool, pt, raw):
    off = [0]
    for r in raw:
        off.append(off[-1] + len(r))
    n = len(raw)
    inp = rc.pack_steps(pt) + struct.pack("<Q", n) + struct.pack("<%dQ" % (n + 1), *off) + b"".join(raw)
    r = subprocess.run([tool], input=inp, capture_output=True)
    assert r.returncode == 0, (pt, r.returncode, r.stderr[-2000:])
    n_words, n_bytes = struct.unpack_from("<2Q", r.stdout)
    text_word = struct.unpack_from("<%dQ" % (n + 1), r.stdout, 16)
    word_off = struct.unpack_from("<%dQ" % (n_words + 1), r.stdout, 16 + 8 * (n + 1))
    body = r.stdout[16 + 8 * (n + 1) + 8 * (n_words + 1):]
    assert len(body) == n_bytes == word_off[n_words] and text_word[n] == n_words and text_word[0] == 0
    return [[body[word_off[j]:word_off[j + 1]] for j in range(text_word[i], text_word[i + 1])] for i in range(n)]


PROG_PATTERNS = [r"\p{N}{1,3}", "a|ab", "ab|a", r"\s+\S", r"a+?b?", r"\d+\.\d+|\d+", rc.GPT2_LIKE, r".+?[a-c]"]
PROGRAMS = [("sequence", [first, ("split", p, b, inv)])
            for p in PROG_PATTERNS for first in (("whitespace",), ("punctuation",))
            for b in pc.BEHAVIORS for inv in (False, True)]


def test_without_the_flag_nothing_changes(prog_tool):
    """the tool's input format is the old one: the same program without the flag is still refused"""
    pt = ("split", "a|ab", "Isolated", False)
    inp = ref.pack_steps(pt) + struct.pack("<QQ", 1, 0) + struct.pack("<Q", 0)
    assert subprocess.run([prog_tool], input=inp, capture_output=True).returncode == 7
    assert run_prog(prog_tool, pt, [b"xaby"]) == [[b"x", b"a", b"by"]]
    assert run_prog(prog_tool, ("split", "ab|a", "Isolated", False), [b"xaby"]) == [[b"x", b"ab", b"y"]]


@pytest.mark.parametrize("k", range(0, len(PROGRAMS), 10))
def test_programs_all_behaviours(prog_tool, texts, k):
    """five behaviours x invert after a step that cuts words: a match cannot cross a word boundary"""
    for pt in PROGRAMS[k:k + 10]:
        got = run_prog(prog_tool, pt, [t.encode("utf-8") for t in texts])
        bad = [i for i, t in enumerate(texts) if [w.decode("utf-8") for w in got[i]] != ref.pre_tokenize(pt, t)]
        assert not bad, (pt, len(bad), texts[bad[0]], got[bad[0]][:8], ref.pre_tokenize(pt, texts[bad[0]])[:8])


def test_not_utf8_stays_inside_its_bounds(prog_tool, dfa_tool):
    """the byte soup of tests/test_pretok_cpu.py in buffers of exact size under the sanitizers: an
    ill-formed byte is a symbol of its own, and a text that is UTF-8 after all gives what the
    restatement gives"""
    rng = random.Random(5)
    raw = [bytes(rng.choice([0x61, 0x20, 0x27, 0x73, 0x31, 0xC3, 0xA9, 0xE2, 0x80, 0x83, 0xE3, 0xF0, 0x9F, 0xED, 0xA0, 0xC0, 0xF4, 0x90])
                 for _ in range(rng.randrange(0, 12))) for _ in range(3000)]
    for pattern in (".+", r"\S+?s", "[^a]{2}", r"\P{L}\p{N}?", rc.GPT2_LIKE):
        run_dfa(dfa_tool, pattern, raw)
        for b in ("Isolated", "Removed"):
            pt = ("sequence", [("whitespace",), ("split", pattern, b, False)])
            got = run_prog(prog_tool, pt, raw)
            for i, t in enumerate(raw):
                try:
                    s = t.decode("utf-8")
                except UnicodeDecodeError:
                    continue
                assert [w.decode("utf-8") for w in got[i]] == ref.pre_tokenize(pt, s), (pt, t)
