"""csrc/postproc_compile.cpp and csrc/postproc_hd.h (the PostProcessor's template compiler and the
rules behind postproc.hip) checked on the CPU against the restatement tests/postproc_ref.py:
tools/postproc_check.cpp, built with g++ and the address and undefined-behaviour sanitizers, compiles a
program and runs it over a packed batch the way the kernels' threads do (a thread per row, the scan, a
thread per cell in workgroups of 256 over staged tables, buffers of exactly the counted size).  No GPU."""
import os
import struct
import subprocess

import pytest

from tests import postproc_cases as pc
from tests import postproc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "complexity-tokenizer_amd")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pp") / "postproc_check")
    src = os.path.join(PKG, "tools", "postproc_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src,
                    "-o", exe], check=True)
    return exe


def run_raw(tool, p, batch, pairs=None, truncate_to=None, strategy="longest_first", padded=False, pad_to=None, pad_id=0,
            pad_left=False, all_pairs=False):
    n = len(batch)
    off = [0]
    for ids in batch:
        off.append(off[-1] + len(ids))
    flat = [i for ids in batch for i in ids]
    mode = 0 if pairs is None else 2 if all_pairs else 1
    inp = [ref.pack_steps(p),
           struct.pack("<IIQIIQII", 0 if truncate_to is None else 1, ref.STRATEGIES[strategy], truncate_to or 0, 1 if padded else 0,
                       1 if pad_left else 0, pad_to if isinstance(pad_to, int) else 0, pad_id, mode),
           struct.pack("<Q", n), struct.pack("<%dQ" % (n + 1), *off)]
    pflat = []
    if mode:
        poff = [0]
        for pr in pairs:
            poff.append(poff[-1] + len(pr or []))
            pflat += pr or []
        inp.append(struct.pack("<%dQ" % (n + 1), *poff))
        if mode == 1:
            inp.append(bytes(0 if pr is None else 1 for pr in pairs))
    inp += [struct.pack("<%dI" % len(flat), *flat), struct.pack("<%dI" % len(pflat), *pflat)]
    return subprocess.run([tool], input=b"".join(inp), capture_output=True)


def run(tool, p, batch, pairs=None, **kw):
    r = run_raw(tool, p, batch, pairs, **kw)
    assert r.returncode == 0, (p, r.returncode, r.stderr[-2000:])
    n = len(batch)
    _, _, total, width = struct.unpack_from("<4Q", r.stdout)
    at = 32
    if not kw.get("padded"):
        off = struct.unpack_from("<%dQ" % (n + 1), r.stdout, at)
        ids = struct.unpack_from("<%dI" % total, r.stdout, at + 8 * (n + 1))
        assert len(r.stdout) == at + 8 * (n + 1) + 4 * total and off[0] == 0 and off[n] == total
        return [list(ids[off[i]:off[i + 1]]) for i in range(n)]
    assert total == n * width and len(r.stdout) == at + 4 * n + 16 * total
    out = {"row_len": list(struct.unpack_from("<%dI" % n, r.stdout, at)), "width": width}
    at += 4 * n
    for name in ("input_ids", "attention_mask", "token_type_ids", "special_tokens_mask"):
        cells = struct.unpack_from("<%dI" % total, r.stdout, at)
        out[name] = [list(cells[i * width:(i + 1) * width]) for i in range(n)]
        at += 4 * total
    return out


def check(tool, p, batch, pairs=None, **kw):
    """ragged against process, padded against process_padded"""
    want = [ref.process(p, ids, None if pairs is None else pairs[i]) for i, ids in enumerate(batch)]
    assert run(tool, p, batch, pairs, **kw) == want, p
    for pad_left in (False, True):
        got = run(tool, p, batch, pairs, padded=True, pad_left=pad_left, pad_id=0xFFFFFFFF, **kw)
        assert got == ref.process_padded(p, batch, pairs, pad_left=pad_left, pad_id=0xFFFFFFFF), (p, pad_left)


@pytest.mark.parametrize("i", range(len(pc.QUIRKS)))
def test_quirk_table(tool, i):
    p, ids, pair, want = pc.QUIRKS[i]
    assert run(tool, p, [ids], None if pair is None else [pair]) == [want]
    assert run(tool, p, [[], ids, ids, []], [None, pair, None, []]) == [ref.process(p, [], None), want, ref.process(p, ids, None),
                                                                      ref.process(p, [], [])]


@pytest.mark.parametrize("i", range(len(pc.EVERY)))
def test_quirk_rows_under_every_processor(tool, i):
    batch, pairs = [r[0] for r in pc.QUIRK_ROWS], [r[1] for r in pc.QUIRK_ROWS]
    check(tool, pc.EVERY[i], batch, pairs)
    check(tool, pc.EVERY[i], batch[::-1], pairs[::-1])
    check(tool, pc.EVERY[i], batch, None)


@pytest.mark.parametrize("seed", range(4))
def test_seeded_random_batches(tool, seed):
    batch, pairs = pc.random_rows(seed, 120)
    assert any(p is None for p in pairs) and any(p == [] for p in pairs) and any(p for p in pairs)
    assert any(0 in r for r in batch) and any(0xFFFFFFFF in r for r in batch)
    for p in pc.EVERY[seed::4]:
        check(tool, p, batch, pairs)
    full = [[] if pr is None else pr for pr in pairs]
    want = [ref.process(pc.BERT, ids, full[i]) for i, ids in enumerate(batch)]
    assert run(tool, pc.BERT, batch, full, all_pairs=True) == want  # no has_pair array: every row has a pair


def test_batches_of_no_rows(tool):
    for p in (pc.BERT, ("sequence", [])):
        assert run(tool, p, []) == [] == run(tool, p, [], [])
        got = run(tool, p, [], padded=True, pad_to=5)
        assert got["input_ids"] == [] and got["width"] == 5


@pytest.mark.parametrize("n", [1, 2, 64, 65, 4096])
def test_flat_lists(tool, n):
    p = pc.flat_list(n)
    r = run_raw(tool, p, [[1]], [[2]])
    assert r.returncode == 0 and struct.unpack_from("<2Q", r.stdout) == (n, n)
    batch = [[], [7], [1, 2, 3], [0xFFFFFFFF]]
    pairs = [None, [], [4, 5], None]
    check(tool, p, batch, pairs)


def test_a_flat_list_of_4097_items_is_refused(tool):
    for p in (pc.flat_list(4097), ("template", "$A " * 4097, None, []), ("sequence", [("template", "$A $A", None, [])] * 13),
              ("sequence", [("template", "$A $A", None, [])] * 1024)):
        r = run_raw(tool, p, [[1]])
        assert r.returncode == 3 and b"4096" in r.stderr, (r.returncode, r.stderr[-300:])
    assert b"4097 items" in run_raw(tool, pc.flat_list(4097), [[1]]).stderr
    assert b"8192 items" in run_raw(tool, ("sequence", [("template", "$A $A", None, [])] * 13), [[1]]).stderr
    # ten steps of "$A $A" are 1024 copies, twelve are 4096
    assert run(tool, ("sequence", [("template", "$A $A", None, [])] * 10), [[5]]) == [[5] * 1024]
    assert run(tool, ("sequence", [("template", "$A $A", None, [])] * 12), [[5, 6]]) == [[5, 6] * 4096]
    # only the list of rows with a pair is too long
    r = run_raw(tool, ("template", "$A", "$B " * 4097, []), [[1]])
    assert r.returncode == 3


@pytest.mark.parametrize("strategy", ["only_first", "only_second", "longest_first"])
def test_truncation_against_the_pop_loop(tool, strategy):
    """every (na, nb, truncate_to) with na, nb <= 12, and rows without a pair"""
    batch, pairs = [], []
    for na in range(13):
        for nb in [None] + list(range(13)):
            batch.append(list(range(1, na + 1)))
            pairs.append(None if nb is None else list(range(100, 100 + nb)))
    p = ("template", "$A <s> $B", "$B <s> $A", [("<s>", 0)])
    for to in range(26):
        want = []
        for ids, pr in zip(batch, pairs):
            ids, pr = list(ids), (None if pr is None else list(pr))
            ref.truncate(ids, pr, to, strategy)
            want.append(ref.process(p, ids, pr))
        assert run(tool, p, batch, pairs, truncate_to=to, strategy=strategy) == want, to


@pytest.mark.parametrize("pad_left", [False, True])
def test_padding(tool, pad_left):
    batch, pairs = pc.random_rows(11, 40)
    longest = max(len(ref.process(pc.BERT, ids, pairs[i])) for i, ids in enumerate(batch))
    for pad_to in ("longest", None, longest - 3, longest, longest + 5, 0):
        for to in (None, 6):
            got = run(tool, pc.BERT, batch, pairs, padded=True, pad_to=pad_to, pad_left=pad_left, pad_id=3, truncate_to=to)
            want = ref.process_padded(pc.BERT, batch, pairs, truncate_to=to, pad_to=pad_to, pad_left=pad_left, pad_id=3)
            assert got == want, (pad_to, to)
            if to is None:
                assert got["width"] == max(longest, pad_to if isinstance(pad_to, int) else 0)


def test_offsets_out_of_order_are_reported(tool):
    r = run_raw(tool, pc.BERT, [[1, 2], [3]])
    assert r.returncode == 0
    # (run_raw packs what it is given; a hand-made input with off = [0, 2, 1] would read ids[2:1])
    inp = ref.pack_steps(pc.BERT) + struct.pack("<IIQIIQII", 0, 0, 0, 0, 0, 0, 0, 0) + struct.pack("<Q3Q", 2, 0, 2, 1) + struct.pack("<I", 1)
    assert subprocess.run([tool], input=inp, capture_output=True).returncode == 4
