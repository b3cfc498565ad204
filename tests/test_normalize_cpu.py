"""csrc/normalize_hd.h (the Normalizer's steps behind normalize.hip) checked on the CPU against the
restatement tests/normalizer_ref.py: tools/normalize_check.cpp, built with g++ and the address and
undefined-behaviour sanitizers, runs a program of steps over a batch the way the kernels' threads do
(count per span, sums, write per span into a buffer of exactly the counted size).  Also the generated
tables: tools/gen_normalize_tables.py reproduces csrc/gen/normalize_data.h and asserts the expansion
facts DESIGN.md 4.6g records.  No GPU."""
import os
import struct
import subprocess
import sys
import unicodedata

import pytest

from tests import normalizer_cases as nc
from tests import normalizer_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "complexity-tokenizer_amd")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nz") / "normalize_check")
    src = os.path.join(PKG, "tools", "normalize_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                    "-o", exe], check=True)
    return exe


def run_tool(tool, norm, texts, steps=False):
    raw = [t.encode("utf-8") for t in texts]
    off = [0]
    for r in raw:
        off.append(off[-1] + len(r))
    n = len(raw)
    prog = ref.flat_steps(norm)
    inp = [struct.pack("<Q", len(prog))]
    for kind, flags, a, b in prog:
        inp.append(struct.pack("<IIQQ", kind, flags, len(a), len(b)) + a + b)
    inp.append(struct.pack("<Q", n) + struct.pack("<%dQ" % (n + 1), *off) + b"".join(raw))
    r = subprocess.run([tool] + (["--steps"] if steps else []), input=b"".join(inp), capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out_off = struct.unpack_from("<%dQ" % (n + 1), r.stdout)
    body = r.stdout[8 * (n + 1):]
    assert len(body) == out_off[n]
    got = [body[out_off[i]:out_off[i + 1]].decode("utf-8") for i in range(n)]
    return (got, int(r.stderr.split()[-1])) if steps else got


def check(tool, norm, texts):
    got = run_tool(tool, norm, texts)
    bad = [i for i, t in enumerate(texts) if got[i] != ref.normalize(norm, t)]
    assert not bad, (norm, len(bad), texts[bad[0]], got[bad[0]], ref.normalize(norm, texts[bad[0]]))


@pytest.mark.parametrize("name", sorted(nc.CASES))
def test_case(tool, name):
    norm, texts = nc.CASES[name]()
    check(tool, norm, texts)


def test_long_run_takes_linear_steps(tool):
    """Canonical ordering is a pass per class present, not an insertion sort: a run of 60,000 marks
    in three classes takes a small multiple of 60,000 inner steps, and twice the run twice as many."""
    got, n1 = run_tool(tool, ("nfd",), ["a" + nc.MARKS * 20000], steps=True)
    assert got == [unicodedata.normalize("NFD", "a" + nc.MARKS * 20000)]
    _, n2 = run_tool(tool, ("nfd",), ["a" + nc.MARKS * 40000], steps=True)
    assert n1 <= 16 * 60000 and n2 <= 2 * n1 + 64, (n1, n2)
    _, n3 = run_tool(tool, ("nfkc",), ["a" + nc.MARKS * 20000], steps=True)
    assert n3 <= 24 * 60000, n3


@pytest.mark.parametrize("pool", sorted(nc.POOLS))
def test_seeded_random_strings(tool, pool):
    texts = nc.random_texts(pool, 20261)
    for norm in [(k,) for k in nc.FORMS] + [("strip_accents",), ("strip",), nc.BERT_DEFAULT, ("bert", True, False, False, False),
                                            ("replace", "a", "aa"), ("replace", "\u0301", ""), nc.ALL_KINDS]:
        check(tool, norm, texts)


def test_not_utf8_passes_through_inside_its_bounds(tool):
    """The device entry takes bytes as they are: the steps must stay inside the buffer (the tool's
    buffers are exactly as long as the batch, under the address sanitizer) and copy raw bytes."""
    import random
    rng = random.Random(5)
    raw = [bytes(rng.choice([0x61, 0xC3, 0xA9, 0xE2, 0x80, 0xCC, 0x81, 0xF0, 0x9F, 0xED, 0xA0, 0xC0, 0xF4, 0x90, 0xEA, 0xB0])
                 for _ in range(rng.randrange(0, 12))) for _ in range(4000)]
    off = [0]
    for r in raw:
        off.append(off[-1] + len(r))
    for norm in (("nfkc",), ("strip_accents",), nc.BERT_DEFAULT, ("strip",), ("replace", "", "-"), ("replace", "a\u0301", "b")):
        prog = ref.flat_steps(norm)
        inp = [struct.pack("<Q", len(prog))]
        for kind, flags, a, b in prog:
            inp.append(struct.pack("<IIQQ", kind, flags, len(a), len(b)) + a + b)
        inp.append(struct.pack("<Q", len(raw)) + struct.pack("<%dQ" % len(off), *off) + b"".join(raw))
        r = subprocess.run([tool], input=b"".join(inp), capture_output=True)
        assert r.returncode == 0, (norm, r.returncode, r.stderr[-2000:])
        out_off = struct.unpack_from("<%dQ" % len(off), r.stdout)
        body = r.stdout[8 * len(off):]
        for i, t in enumerate(raw):  # a text that is UTF-8 after all gives what the restatement gives
            try:
                s = t.decode("utf-8")
            except UnicodeDecodeError:
                continue
            assert body[out_off[i]:out_off[i + 1]].decode("utf-8") == ref.normalize(norm, s), (norm, t)


def test_tables_are_reproducible_and_counted(tmp_path):
    out = str(tmp_path / "normalize_data.h")
    subprocess.run([sys.executable, os.path.join(PKG, "tools", "gen_normalize_tables.py"), out], check=True)
    with open(out) as f, open(os.path.join(PKG, "csrc", "gen", "normalize_data.h")) as g:
        assert f.read() == g.read()
    sys.path.insert(0, os.path.join(PKG, "tools"))
    try:
        import gen_normalize_tables as gen
    finally:
        sys.path.pop(0)
    decomp_d, decomp_k, pairs, props = gen.tables()
    assert unicodedata.unidata_version == "13.0.0"
    assert (len(decomp_d), len(decomp_k), len(pairs)) == (2061, 5736, 941)
    f = gen.facts(decomp_d, decomp_k)  # (asserts them itself)
    assert f["nfd"] == (4, 0x1F82, 3.0) and f["nfkd"] == (18, 0xFDFA, 11.0)
    assert max(unicodedata.combining(chr(c)) for c in nc.SCALARS) < 256
    assert len({unicodedata.combining(chr(c)) for c in nc.SCALARS} - {0}) == 55


def test_unicode_version_boundary():
    """The `regex` module's Unicode data is newer than Python's 13.0.  Normalisation stability
    (UAX #15 section 3) keeps every string of code points assigned in 13.0 identical under newer
    data, so the crate's tables can differ only on code points unassigned here: every code point
    that has a decomposition or a combining class for `regex` but none for unicodedata is Cn here
    (DESIGN.md section 2)."""
    regex = pytest.importorskip("regex")
    ccc, nfkd = regex.compile(r"\P{ccc=0}"), regex.compile(r"\p{NFKD_QC=N}")
    d_ccc = [c for c in nc.SCALARS if bool(ccc.fullmatch(chr(c))) != (unicodedata.combining(chr(c)) != 0)]
    d_nfkd = [c for c in nc.SCALARS if bool(nfkd.fullmatch(chr(c))) != (unicodedata.normalize("NFKD", chr(c)) != chr(c))]
    assert d_ccc and d_nfkd  # (the data is newer indeed)
    assert all(unicodedata.category(chr(c)) == "Cn" for c in d_ccc + d_nfkd)
