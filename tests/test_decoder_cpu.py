"""csrc/decoder_hd.h (the Decoder's rules behind decoder.hip) checked on the CPU against the
restatement tests/decoder_ref.py: tools/decoder_check.cpp, built with g++ and the address and
undefined-behaviour sanitizers, runs a program over a packed batch the way the kernels' threads do
(a thread per byte or token in workgroups of 256, count per workgroup, scan, write into buffers of
exactly the counted size).  No GPU."""
import os
import random
import struct
import subprocess

import pytest

from tests import decoder_cases as dc
from tests import decoder_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "complexity-tokenizer_amd")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dc") / "decoder_check")
    src = os.path.join(PKG, "tools", "decoder_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                    "-o", exe], check=True)
    return exe


def run_raw(tool, dec, docs):
    """docs: lists of tokens as bytes; the texts as bytes"""
    flat = [t for d in docs for t in d]
    tok_off, doc_tok = [0], [0]
    for t in flat:
        tok_off.append(tok_off[-1] + len(t))
    for d in docs:
        doc_tok.append(doc_tok[-1] + len(d))
    n = len(docs)
    inp = (ref.pack_steps(dec) + struct.pack("<Q", n) + struct.pack("<%dQ" % (n + 1), *doc_tok)
           + struct.pack("<%dQ" % len(tok_off), *tok_off) + b"".join(flat))
    r = subprocess.run([tool], input=inp, capture_output=True)
    assert r.returncode == 0, (dec, r.returncode, r.stderr[-2000:])
    n_bytes, = struct.unpack_from("<Q", r.stdout)
    off = struct.unpack_from("<%dQ" % (n + 1), r.stdout, 8)
    body = r.stdout[8 + 8 * (n + 1):]
    assert len(body) == n_bytes == off[n] and off[0] == 0 and all(off[i] <= off[i + 1] for i in range(n))
    return [body[off[i]:off[i + 1]] for i in range(n)]


def check(tool, dec, docs):
    got = run_raw(tool, dec, [[t.encode("utf-8") for t in d] for d in docs])
    bad = [i for i, d in enumerate(docs) if got[i] != ref.decode(dec, d).encode("utf-8")]
    assert not bad, (dec, len(bad), docs[bad[0]][:40], got[bad[0]][:120], ref.decode(dec, docs[bad[0]])[:120])


@pytest.mark.parametrize("i", range(len(dc.EVERY)))
def test_quirks_under_every_decoder(tool, i):
    check(tool, dc.EVERY[i], dc.QUIRKS)
    check(tool, dc.EVERY[i], [[]] + dc.QUIRKS[::-1] + [[], []])


@pytest.mark.parametrize("pool", sorted(dc.POOLS))
def test_seeded_random_token_lists(tool, pool):
    docs = dc.random_token_lists(pool, 20264, 300, 150)
    for dec in dc.EVERY:
        check(tool, dec, docs)


BOUNDARY_DECODERS = dc.DEFAULTS + [("replace", "aa", "b"), ("replace", "", "é"), ("replace", "yy", "é"), ("replace", "##", ""),
                                   ("wordpiece", "##", False), ("ctc", "a", "##b"), ("ctc", "<pad>", "|"), ("strip", "y", 10 ** 9, 1),
                                   ("metaspace", "é", True), ("bpe", "a</w>"), ("sequence", [("wordpiece", "##", True), ("bpe", "</w>")])]


@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513])
def test_totals_around_a_tile(tool, n):
    """A workgroup's tile is 256 units: batches of n bytes and of n tokens, in one document and in many."""
    for docs in ([["a"] * n], [["a" * n]], [["a"]] * n, [[""] * n + ["a"]], [[]] * n, [["ab"] * (n // 2), ["a"] * (n % 2)]):
        for dec in BOUNDARY_DECODERS:
            check(tool, dec, docs)


@pytest.mark.parametrize("at", [256, 512])
def test_things_that_straddle_a_tile(tool, at):
    """Every document is a batch of its own, so that its thing -- a multi-byte char, a prefix, a suffix,
    a Replace match, an invalid unit, a clean-up pattern, trailing white space -- has bytes on both
    sides of byte `at` of the op's input, and a token and its neighbour lie in two tiles
    (tests/decoder_cases.py straddling() asserts the positions)."""
    for dec in BOUNDARY_DECODERS if at == 256 else BOUNDARY_DECODERS[::3]:  # (a process per batch: the second tile, fewer decoders)
        for doc, _, _ in dc.straddling(at):
            check(tool, dec, [doc])
        for doc in dc.straddling_tokens(at):
            check(tool, dec, [doc])


def test_runs_of_set_bytes(tool):
    rng = random.Random(7)
    docs = []
    for n in (1, 2, 63, 64, 65, 200, 700):
        docs.append(["".join(rng.choice(" .,!?:;'") for _ in range(n))])
        docs.append(["a" * 250] + [rng.choice(" .,!?:;'") for _ in range(n)] + ["b"])
        docs.append([" '" * n, "' " * n, " ." * n])
    check(tool, ("wordpiece", "##", True), docs)
    check(tool, ("wordpiece", "", True), docs)
    for n in (63, 64, 65, 200):  # a run of exactly n set bytes across a tile boundary of the clean-up's input
        for at in (256, 768):
            check(tool, ("wordpiece", "##", True), [dc.set_run_across(at, n, n + at)])


def test_not_utf8_passes_through_inside_its_bounds(tool):
    """The device entry takes bytes as they are: the rules must stay inside the buffers (the tool's
    are exactly as long as the batch, under the address sanitizer); a document that is UTF-8 after
    all gives what the restatement gives."""
    rng = random.Random(5)
    alphabet = [0x61, 0x20, 0x27, 0x2E, 0x23, 0x5F, 0xC3, 0xA9, 0xE2, 0x96, 0x81, 0x80, 0xE3, 0xF0, 0x9F, 0xED, 0xA0, 0xC0, 0xF4, 0x90,
                0xC4, 0xA0, 0xC5, 0x83]
    docs = []
    for _ in range(3000):
        k = rng.randrange(0, 4)
        docs.append([bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 7))) for _ in range(k)])
    for dec in dc.EVERY:
        got = run_raw(tool, dec, docs)
        for i, d in enumerate(docs):
            try:
                toks = [t.decode("utf-8") for t in d]
            except UnicodeDecodeError:
                continue
            assert got[i] == ref.decode(dec, toks).encode("utf-8"), (dec, d)
