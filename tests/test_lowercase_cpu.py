"""csrc/lowercase_hd.h (Rust's str::to_lowercase behind lowercase.hip) checked on the CPU against
Python's str.lower(): tools/lowercase_check.cpp, built with g++, lower-cases batches of texts the way
the kernel's threads do.  Also the generated tables: tools/gen_lowercase_tables.py reproduces
csrc/gen/lowercase_data.h, and the counts DESIGN.md records hold.  No GPU."""
import os
import random
import struct
import subprocess
import sys
import unicodedata

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "complexity-tokenizer_amd")

SCALARS = [c for c in range(0x110000) if not 0xD800 <= c < 0xE000]


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lc") / "lowercase_check")
    src = os.path.join(PKG, "tools", "lowercase_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    return exe


def lower_batch(tool, texts):
    raw = [t.encode("utf-8") for t in texts]
    off = [0]
    for r in raw:
        off.append(off[-1] + len(r))
    n = len(raw)
    inp = struct.pack("<Q", n) + struct.pack("<%dQ" % (n + 1), *off) + b"".join(raw)
    r = subprocess.run([tool], input=inp, capture_output=True)
    assert r.returncode == 0, r.returncode
    out_off = struct.unpack_from("<%dQ" % (n + 1), r.stdout)
    body = r.stdout[8 * (n + 1):]
    assert len(body) == out_off[n]
    return [body[out_off[i]:out_off[i + 1]].decode("utf-8") for i in range(n)]


def check(tool, texts):
    got = lower_batch(tool, texts)
    for t, g in zip(texts, got):
        assert g == t.lower(), (t, g, t.lower())


def test_every_code_point_alone(tool):
    check(tool, [chr(c) for c in SCALARS])


def test_sigma_contexts(tool):
    ign = "\u0301"  # a case-ignorable, uncased mark
    texts = ["\u03a3", "\u0391\u03a3", "\u03a3\u0391", "\u0391.\u03a3", "\u0391\u03a3a", "\u0391\u03a3 ", "\u0391 \u03a3",
             "a\u03a3.", "a.\u03a3.", "a\u03a3.b", "\u03a3\u03a3", "\u0391\u03a3\u03a3", "\u0391\u03a3\u03a3\u0391", "1\u03a3",
             "a\u03a31", "a" + ign + "\u03a3",
             "a" + ign * 3 + "\u03a3" + ign * 3, "a" + ign + "\u03a3" + ign + "b", ign + "\u03a3", "a" + ign * 5000 + "\u03a3",
             "a" + "." * 5000 + "\u03a3" + "." * 5000, "a" + "." * 5000 + "\u03a3" + "." * 5000 + "b",
             "\u0345\u03a3", "a\u0345\u03a3", "\u0391\u03a3\u0345", "\u02b0\u03a3", "A\u03a3\U0001D400",
             "\U0001D400\u03a3", "a\u03a3\u00ad", "a\u00ad\u03a3\u00adb", "\u0130\u03a3", "\u03a3\u0130\u03a3"]
    check(tool, texts)
    # the context never leaves the text: a sigma last in one text with a letter first in the next
    assert lower_batch(tool, ["\u0391\u03a3", "\u0391"]) == ["\u03b1\u03c2", "\u03b1"]
    assert lower_batch(tool, ["\u0391", "\u03a3"]) == ["\u03b1", "\u03c3"]
    assert lower_batch(tool, ["\u0391", "", "\u03a3", "", "\u0391\u03a3", "a"]) == ["\u03b1", "", "\u03c3", "", "\u03b1\u03c2", "a"]


def test_lengths_that_change(tool):
    grow = [c for c in SCALARS if len(chr(c).lower().encode()) > len(chr(c).encode())]
    shrink = [c for c in SCALARS if len(chr(c).lower().encode()) < len(chr(c).encode())]
    assert len(grow) == 3 and len(shrink) == 22 and 0x23A in grow and 0x212A in shrink
    assert [c for c in SCALARS if len(chr(c).lower()) > 1] == [0x130]
    texts = []
    for c in grow + shrink:
        texts += [chr(c), "x" + chr(c), chr(c) + "x", chr(c) * 70, ("ab" + chr(c)) * 40]
    check(tool, texts)


def test_seeded_random_strings(tool):
    rng = random.Random(20260)
    changing = [c for c in SCALARS if chr(c).lower() != chr(c)]
    pools = [list(range(0x20, 0x7F)), changing, [0x3A3, 0x391, 0x61, 0x2E, 0x301, 0x20, 0x345, 0x130, 0xAD],
             SCALARS]
    texts = []
    for i in range(3000):
        pool = pools[i % len(pools)]
        texts.append("".join(chr(rng.choice(pool)) for _ in range(rng.randrange(0, 40))))
    check(tool, texts)


def test_tables_are_reproducible_and_counted(tmp_path):
    out = str(tmp_path / "lowercase_data.h")
    subprocess.run([sys.executable, os.path.join(PKG, "tools", "gen_lowercase_tables.py"), out], check=True)
    with open(out) as f, open(os.path.join(PKG, "csrc", "gen", "lowercase_data.h")) as g:
        assert f.read() == g.read()
    sys.path.insert(0, os.path.join(PKG, "tools"))
    try:
        import gen_lowercase_tables as gen
    finally:
        sys.path.pop(0)
    mapping, cased, ign, n_cased, n_ign = gen.tables()
    assert unicodedata.unidata_version == "13.0.0"
    assert len(mapping) + 1 == 1393 and n_cased == 4141 and n_ign == 2413  # (+ 1: U+03A3, handled in code)
    # U+03A3 is the only code point whose lower case depends on its context
    for c in SCALARS:
        ch = chr(c)
        if ("a" + ch).lower() != "a" + ch.lower() or (ch + "a").lower() != ch.lower() + "a":
            assert c == 0x3A3, hex(c)


def test_unicode_version_boundary():
    """The `regex` module's Unicode data is newer than Python's 13.0: its Changes_When_Lowercased
    differs from str.lower() on 95 code points, all unassigned in 13.0."""
    regex = pytest.importorskip("regex")
    cwl = regex.compile(r"\p{Changes_When_Lowercased}")
    diff = [c for c in SCALARS if bool(cwl.fullmatch(chr(c))) != (chr(c).lower() != chr(c))]
    assert len(diff) == 95
    assert all(unicodedata.category(chr(c)) == "Cn" for c in diff)
