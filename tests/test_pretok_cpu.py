"""csrc/pretok_hd.h (the PreTokenizer's rules behind pretok.hip) checked on the CPU against the
restatement tests/pretok_ref.py: tools/pretok_check.cpp, built with g++ and the address and
undefined-behaviour sanitizers, runs a program over a packed batch the way the kernels' threads do
(bitmaps per 64-byte word, count per bitmap word, write into buffers of exactly the counted size).
Also the generated `\\d` table and the gates of the `split` patterns.  No GPU."""
import os
import struct
import subprocess
import sys

import pytest
import regex

from oracle import rust_regex
from tests import pretok_cases as pc
from tests import pretok_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "complexity-tokenizer_amd")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pt") / "pretok_check")
    src = os.path.join(PKG, "tools", "pretok_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                    "-o", exe], check=True)
    return exe


def run_raw(tool, pt, raw):
    off = [0]
    for r in raw:
        off.append(off[-1] + len(r))
    n = len(raw)
    inp = ref.pack_steps(pt) + struct.pack("<Q", n) + struct.pack("<%dQ" % (n + 1), *off) + b"".join(raw)
    r = subprocess.run([tool], input=inp, capture_output=True)
    assert r.returncode == 0, (pt, r.returncode, r.stderr[-2000:])
    n_words, n_bytes = struct.unpack_from("<2Q", r.stdout)
    text_word = struct.unpack_from("<%dQ" % (n + 1), r.stdout, 16)
    word_off = struct.unpack_from("<%dQ" % (n_words + 1), r.stdout, 16 + 8 * (n + 1))
    body = r.stdout[16 + 8 * (n + 1) + 8 * (n_words + 1):]
    assert len(body) == n_bytes == word_off[n_words] and text_word[n] == n_words and text_word[0] == 0
    return [[body[word_off[j]:word_off[j + 1]] for j in range(text_word[i], text_word[i + 1])] for i in range(n)]


def check(tool, pt, texts):
    got = run_raw(tool, pt, [t.encode("utf-8") for t in texts])
    bad = [i for i, t in enumerate(texts) if [w.decode("utf-8") for w in got[i]] != ref.pre_tokenize(pt, t)]
    assert not bad, (pt, len(bad), texts[bad[0]][:80], got[bad[0]][:8], ref.pre_tokenize(pt, texts[bad[0]])[:8])


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_case(tool, name):
    pt, texts = pc.CASES[name]()
    check(tool, pt, texts)


@pytest.mark.parametrize("i", range(len(pc.EVERY)))
def test_quirks_under_every_pre_tokenizer(tool, i):
    check(tool, pc.EVERY[i], pc.QUIRKS + pc.ADJACENT)


@pytest.mark.parametrize("pool", sorted(pc.POOLS))
def test_seeded_random_strings(tool, pool):
    texts = pc.random_texts(pool, 20263, 300, 150)
    for pt in pc.EVERY:
        check(tool, pt, texts)


def test_not_utf8_passes_through_inside_its_bounds(tool):
    """The device entry takes bytes as they are: the rules must stay inside the buffer (the tool's
    buffers are exactly as long as the batch, under the address sanitizer); a text that is UTF-8
    after all gives what the restatement gives."""
    import random
    rng = random.Random(5)
    raw = [bytes(rng.choice([0x61, 0x20, 0x27, 0x73, 0x31, 0xC3, 0xA9, 0xE2, 0x80, 0x83, 0xE3, 0xF0, 0x9F, 0xED, 0xA0, 0xC0, 0xF4, 0x90])
                 for _ in range(rng.randrange(0, 12))) for _ in range(3000)]
    for pt in pc.SINGLE + pc.SEQUENCES + [("split", " ", "Isolated", False), ("split", r"\S+", "Removed", False)]:
        got = run_raw(tool, pt, raw)
        for i, t in enumerate(raw):
            try:
                s = t.decode("utf-8")
            except UnicodeDecodeError:
                continue
            assert [w.decode("utf-8") for w in got[i]] == ref.pre_tokenize(pt, s), (pt, t)


def test_digit_table_matches_regex_on_every_code_point():
    with open(os.path.join(PKG, "csrc", "gen", "pretok_data.h")) as f:
        src = f.read()
    lo, hi = ([int(v, 16) for v in regex.findall(r"0x[0-9A-F]+", src.split(name + "[")[-1].split("};")[0].split("{")[1])]
              for name in ("pt_nd_lo", "pt_nd_hi"))
    assert len(lo) == len(hi) == int(regex.search(r"#define PT_N_ND (\d+)", src).group(1))
    table = set()
    for a, b in zip(lo, hi):
        assert a <= b
        table.update(range(a, b + 1))
    digit = regex.compile(r"\d")
    for c in range(0x110000):
        if 0xD800 <= c < 0xE000:
            assert c not in table
        else:
            assert (digit.fullmatch(chr(c)) is not None) == (c in table), hex(c)


def test_digit_table_is_reproducible(tmp_path):
    out = str(tmp_path / "pretok_data.h")
    subprocess.run([sys.executable, os.path.join(PKG, "tools", "gen_pretok_tables.py"), out], check=True)
    with open(out) as f, open(os.path.join(PKG, "csrc", "gen", "pretok_data.h")) as g:
        assert f.read() == g.read()


# pattern, the gate that takes it
PATTERNS = [
    (r"(?=a)", "rejected"), (r"a(?!b)", "rejected"), (r"(?<=a)b", "rejected"), (r"\1", "rejected"), (r"(a", "rejected"),
    (r"[a", "rejected"), (r"\p{Foo}", "rejected"), (r"a\q", "rejected"), ("\\", "rejected"),
    ("a", "literal"), ("ab", "literal"), ("aa", "literal"), ("!", "literal"), (r"\$", "literal"), (r"\.", "literal"),
    (r"\n", "literal"), (r"a\tb", "literal"), ("▁", "literal"), ("世界", "literal"), (" ", "literal"),
    ("-", "literal"), (r"\\", "literal"), (r"\[\]", "literal"), ("a-b", "literal"),
    (r"\s", "class"), (r"\S", "class"), (r"\d", "class"), (r"\D+", "class"), (r"\d+", "class"), (r"\p{L}", "class"),
    (r"\P{L}+", "class"), (r"\p{N}+", "class"), (r"\P{N}", "class"), (r"[abc]", "class"), (r"[^abc]+", "class"),
    (r"[a-z0-9_]+", "class"), (r"[^\s\p{L}\p{N}]+", "class"), (r"[\.\-]", "class"), ("[一-鿿]", "class"),
    ("", "unsupported"), ("a|b", "unsupported"), ("(a)", "unsupported"), (".", "unsupported"), ("^a", "unsupported"),
    ("a$", "unsupported"), (r"\w", "unsupported"), (r"\w+", "unsupported"), (r"\bfoo", "unsupported"), ("a*", "unsupported"),
    ("a?", "unsupported"), (r"\s*", "unsupported"), (r"\s+?", "unsupported"), (r"\d{2}", "unsupported"), ("(?i)a", "unsupported"),
    (r"\s\s", "unsupported"), (r"a\s", "unsupported"), ("[a-z][0-9]", "unsupported"), ("[[:alpha:]]", "unsupported"),
    ("[a&&b]", "unsupported"), (r"\pL", "unsupported"), (r"\p{Lu}", "unsupported"), (r"\<a", "unsupported"), ("[a-]", "unsupported"),
    ("[" + "".join(chr(0x61 + i) + "," for i in range(17))[:-1] + "]", "unsupported"),
]


def test_enough_patterns():
    assert len(PATTERNS) >= 30 and len({p for p, _ in PATTERNS}) == len(PATTERNS)


@pytest.mark.parametrize("pattern,gate", PATTERNS)
def test_split_pattern_gates(tool, pattern, gate):
    """Gate 1 is oracle/rust_regex.py's decision (the library's rust_regex_rejects restated); the
    tool prints gates 2 and 3 of what the crate compiles.  A pattern that runs also compiles for
    the `regex` module the restatement uses."""
    assert rust_regex.compiles(pattern) == (gate != "rejected")
    if gate == "rejected":
        return
    r = subprocess.run([tool, "--classify", pattern], capture_output=True, check=True)
    assert {"1": "literal", "2": "class", "3": "unsupported"}[r.stdout.decode().strip()] == gate
    if gate != "unsupported":
        regex.compile(pattern)


def test_library_gate_agrees():
    """ctok_pretok_split_class: all three gates as the library applies them (no device needed)."""
    from complexity_tokenizer import _native
    names = ["rejected", "literal", "class", "unsupported"]
    for pattern, gate in PATTERNS:
        raw = pattern.encode("utf-8")
        assert names[_native.lib.ctok_pretok_split_class(raw, len(raw))] == gate, pattern


def test_no_such_device_and_the_order_of_refusals():
    """There is no CPU fallback: a device that does not exist is DeviceError, on a machine with a
    GPU or without one.  The arguments and the pattern are judged first, so an unsupported pattern
    is UnsupportedConfigError and a bad argument TypeError / ValueError wherever the code runs."""
    from complexity_tokenizer import DeviceError, PreTokenizer, UnsupportedConfigError
    none = 1 << 20
    for make in (PreTokenizer.whitespace, PreTokenizer.whitespace_split, PreTokenizer.byte_level, PreTokenizer.metaspace,
                 PreTokenizer.punctuation, PreTokenizer.digits, PreTokenizer.gpt2, PreTokenizer.bert, PreTokenizer.unicode_scripts,
                 lambda device: PreTokenizer.char_delimiter_split("_", device=device),
                 lambda device: PreTokenizer.split(r"\d+", "Isolated", device=device),
                 lambda device: PreTokenizer.split("(?=a)", device=device),
                 lambda device: PreTokenizer.sequence([], device=device)):
        with pytest.raises(DeviceError):
            make(device=none)
    with pytest.raises(UnsupportedConfigError) as e:
        PreTokenizer.split("a|b", device=none)
    assert "a|b" in str(e.value)
    with pytest.raises(ValueError):
        PreTokenizer.metaspace("ab", device=none)
    with pytest.raises(TypeError):
        PreTokenizer.digits(1, device=none)
