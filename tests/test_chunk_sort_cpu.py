"""The merge passes' chunk order (csrc/chunk_sort_hd.h) on the host: the bucket of every length
1..64 for every pass against hand-written tables, and a scalar model of the kernel's counting sort
(permutation of the sorted prefix, bucket-monotone in the chosen direction, list order after it) at
E = 0, 1, 63, 64, 65, SORTCAP - 1, SORTCAP, SORTCAP + 1, 4 x SORTCAP, with one bucket only and
with alternating extreme buckets: tools/chunk_sort_check.cpp built with g++ and run.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_sort_rule_and_model(tmp_path):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "chunk_sort_check.cpp")
    exe = str(tmp_path / "chunk_sort_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_gpu_inputs_reach_every_edge(gpt2_path, llama3_path):
    """The inputs of tests/test_gpu_chunk_sort.py, by the oracle: at least 90 % of each input's
    <= 8 B pieces have more than one token (so they are list entries), and the lists' sizes per
    chunk lie where the test wants them against the sort buffer's three capacities."""
    import json

    from oracle import ref_c
    from tests import chunk_sort_cases as cs

    lo, mid, hi = cs.SORTCAPS
    ins = cs.inputs()
    for path in (gpt2_path, llama3_path):
        with open(path) as f:
            ref = ref_c.RefC(json.load(f))
        got = {}
        for name, docs in ins.items():
            cls, chunk, plen, frac = cs.list_entries(ref, ref_c.pieces, docs)
            assert frac >= 0.9, (name, frac)
            got[name] = (cls, chunk, plen)

        def counts(name, c, whole=True):
            n = cs.chunk_counts(*got[name][:2], c)
            return n[:-1] if whole and len(n) > 1 else n  # (the text can end a few bytes into one more chunk)

        def lengths(name, c):
            cls, _, plen = got[name]
            return set(plen[cls == c].tolist())

        assert counts("c0_over", 0).min() > hi
        assert 0.9 * lo < counts("c0_under", 0).min() and counts("c0_under", 0).max() < lo
        assert lo < counts("c0_mid1", 0).min() and counts("c0_mid1", 0).max() < mid
        assert mid < counts("c0_mid2", 0).min() and counts("c0_mid2", 0).max() < hi
        assert lengths("c0_over", 0) >= set(range(3, 9))  # (a 2-byte piece is nearly always a token)
        assert counts("c1_under", 1).max() < lo and lengths("c1_under", 1) == set(range(9, 17))
        assert lo < counts("c1_over", 1).min() and lengths("c1_over", 1) == set(range(9, 17))
        n2 = counts("c2_sparse", 2, whole=False)
        assert len(n2) >= 300 // cs.CHUNK_TILES and 0 < n2.max() <= 6 * cs.CHUNK_TILES and lengths("c2_sparse", 2) == set(range(17, 33))
        assert counts("c2_dense", 2).min() > 2000 and lengths("c2_dense", 2) == set(range(17, 33))
        assert lengths("c0_len8", 0) == {8} and lengths("c1_len12", 1) == {12} and lengths("c2_len24", 2) == {24}
        assert sum(len(d.encode()) for d in ins["tiny"]) < cs.TILE
        assert all(len(lengths("tiny", c)) > 1 for c in range(3))
