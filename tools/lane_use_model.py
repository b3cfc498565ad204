#!/usr/bin/env python3
"""Lane use of the merge passes' divergent loops under a chunk order (CPU model, no GPU).

class_pass (csrc/kernels.hip) gives a piece to a thread; a wavefront runs each loop as often as
its slowest lane.  This model takes the first DOCS documents of a BASELINE config, the pieces and
token counts of oracle/ref_py.py, cuts the text into tiles and chunks as the kernel does, walks
each chunk's class list in the order under test in blocks of 64 entries, and reports per loop

    lane use = sum of the lanes' iterations / (64 x sum of the blocks' longest lane)

Loops (iterations include the look that finds nothing, where the loop ends on one):
    lds8        <= 8 B pass, merge_lds8_run: one iteration per merge, and the last look
    tier16      9..16 B pass, the 16-slot tier: n - max(m, 8) steps (a look more when m > 8)
    lds8@16     9..16 B pass, merge_lds8_run after the tier (pieces that came down to 8 tokens)
    tier32      17..32 B pass, the 32-slot tier: n - max(m, 16) steps (a look more when m > 16)
Orders (csrc/chunk_sort_hd.h): list (unsorted), coarse (four buckets of width 2 / 2 / 4), exact
(one bucket per length; <= 5, 6, 7, 8 in the <= 8 B pass), and the variants the issue compares:
two (<= 6, 7..8) for the <= 8 B pass and width2 for the 17..32 B pass.  The first SORTCAP entries
of a chunk are sorted, the rest follow in list order; `today` is all-or-nothing as before.

usage: python tools/lane_use_model.py [CONFIG] [DOCS] [--sortcap N] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

from datagen import corpus  # noqa: E402
from datagen.build_tokenizers import fixture_path  # noqa: E402
from oracle import ref_py  # noqa: E402

TILE = 3968
FIXTURE = {"C3": "llama3_128k", "C5": "multi_32k", "C5NFC": "multi_32k"}


def pieces_of(tok, cfg, n_docs):
    """(start byte, length, token count) of every piece, docs packed back to back."""
    text, off = corpus.CONFIGS[cfg](n_docs=n_docs)
    docs = corpus.unpack(text, off)
    cache = {}
    start, length, ntok = [], [], []
    pos = 0
    for d in docs:
        p = pos
        for piece in ref_py.GPT2_PATTERN.finditer(d.decode("utf-8", "replace")):
            b = piece.group(0).encode("utf-8")
            m = cache.get(b)
            if m is None:
                m = cache[b] = len(tok.bpe("".join(tok.byte_encoder[c] for c in b)))
            start.append(p)
            length.append(len(b))
            ntok.append(m)
            p += len(b)
        pos += len(d)
    return np.array(start), np.array(length), np.array(ntok)


def bucket(rule, N, n):
    lo = 1 if N == 8 else N // 2 + 1
    if rule == "coarse":
        return np.minimum(3, (n - lo) // (4 if N == 32 else 2))
    if rule == "exact":
        return np.maximum(n, 5) - 5 if N == 8 else n - lo
    if rule == "two":
        return (n > 6).astype(np.int64)
    if rule == "width2":
        return (n - lo) // 2
    raise ValueError(rule)


def lane_use(chunk, n, trips, rule, N, sortcap, all_or_nothing=False):
    """chunk: chunk number per entry (list order); trips: dict loop -> iterations per entry."""
    tot = {k: 0 for k in trips}
    mx = {k: 0 for k in trips}
    bounds = np.flatnonzero(np.diff(chunk)) + 1
    for a, z in zip(np.concatenate([[0], bounds]), np.concatenate([bounds, [len(chunk)]])):
        order = np.arange(a, z)
        es = 0 if rule == "list" else (z - a if z - a <= sortcap else 0) if all_or_nothing else min(z - a, sortcap)
        if es:
            order[:es] = a + np.argsort(bucket(rule, N, n[a:a + es]), kind="stable")
        pad = (-len(order)) % 64
        for k, t in trips.items():
            v = np.concatenate([t[order], np.zeros(pad, dtype=t.dtype)]).reshape(-1, 64)
            tot[k] += int(v.sum())
            mx[k] += int(v.max(axis=1).sum())
    return {k: tot[k] / (64.0 * mx[k]) if mx[k] else float("nan") for k in trips}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C4")
    ap.add_argument("docs", nargs="?", type=int, default=20000)
    ap.add_argument("--sortcap", type=int, default=6016)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = a.config.upper()
    fx = FIXTURE.get(cfg, "gpt2_50k")
    with open(fixture_path(fx, os.environ.get("TMPDIR", "/tmp"))) as f:
        tok = ref_py.RefTokenizer(json.load(f))
    start, n, m = pieces_of(tok, cfg, a.docs)
    tile = start // TILE
    lines = ["lane use of the merge loops, %s (%s), first %d docs, %d pieces, %d B; SORTCAP %d" %
             (cfg, fx, a.docs, len(n), int(start[-1] + n[-1]) if len(n) else 0, a.sortcap)]

    def report(name, sel, kt, N, trips, rules):
        chunk = tile[sel] // kt
        lines.append("%s: %d entries, %d chunks of %d tiles, mean merges %.2f" %
                     (name, int(sel.sum()), len(np.unique(chunk)), kt, float((n[sel] - m[sel]).mean()) if sel.any() else 0.0))
        for label, rule, aon in rules:
            u = lane_use(chunk, n[sel], {k: v[sel] for k, v in trips.items()}, rule, N, a.sortcap, aon)
            lines.append("    %-22s %s" % (label, "  ".join("%s %.3f" % (k, v) for k, v in u.items())))

    c0 = (n <= 8) & (m > 1)  # (a whole-token piece of <= 8 B never reaches the list)
    report("<= 8 B pass", c0, 64, 8, {"lds8": n - m + 1},
           [("today (list order)", "list", False), ("exact", "exact", False), ("two (<= 6, 7..8)", "two", False),
            ("coarse (width 2)", "coarse", False)])
    c1 = (n >= 9) & (n <= 16)
    down = m <= 8
    report("9..16 B pass", c1, 64, 16,
           {"tier16": n - np.maximum(m, 8) + (m > 8), "lds8@16": np.where(down, 8 - m + 1, 0)},
           [("unsorted", "list", False), ("today (coarse)", "coarse", True), ("exact", "exact", False)])
    c2 = (n >= 17) & (n <= 32)
    report("17..32 B pass", c2, 256, 32, {"tier32": n - np.maximum(m, 16) + (m > 16)},
           [("unsorted", "list", False), ("today (coarse)", "coarse", True), ("width2", "width2", False),
            ("exact", "exact", False)])
    hist = np.bincount(n[c0], minlength=9)[1:9]
    lines.append("<= 8 B entries by length 1..8: %s" % " ".join("%.1f%%" % (100.0 * h / max(1, c0.sum())) for h in hist))
    out = "\n".join(lines) + "\n"
    sys.stdout.write(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)


if __name__ == "__main__":
    main()
