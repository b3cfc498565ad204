#!/usr/bin/env python3
"""Per-stage HIP-event times of PipelineTokenizer's Encoding path (encode_encodings_flat).

Default: --rows rows of about --ids ids each, cut at blanks from a seeded datagen corpus (ASCII rows
only, so that no row panics on a char boundary), through Sequence[NFKC, Lowercase] -> Whitespace ->
BertProcessing over the gpt2_50k fixture's vocab and merges.  After --warmup calls (the first grows the
handle's buffers) the median over --reps calls of every stage -- those of ctok_pipeline_stage_ms, then
find, spans and rows -- is printed with the host call's wall time, one JSON line.

--find-worst-case: the basis of the bound on a sequence's find work.  One sequence,
alone in the batch, of "A " * n under Lowercase -> Whitespace: every word "a" misses and scans to the
text's end, 64 positions a window.  n doubles the work from 2^20 up to the handle's limit; each size is
one call after a warm-up.  --partial-worst-case: the same for the compares of partial matches, which
the work does not count: "A" + "a" * h + " " + "a" * h + "A", whose first word matches all but its last
byte at every position.  Needs a HIP device.
Usage: tools/pipeline_encoding_timing.py [--rows N] [--ids N] [--reps R] [--warmup W] | --find-worst-case | --partial-worst-case
"""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "complexity-tokenizer_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def lower_ws():
    from complexity_tokenizer import Normalizer, PipelineTokenizer, PreTokenizer
    return PipelineTokenizer.from_components({"a": 0}, [], Normalizer.lowercase(), PreTokenizer.whitespace())


def timed(tok, text):
    from complexity_tokenizer import UnsupportedConfigError
    tok.encode_encodings_flat(["A a"])  # the warm-up: tables and code resident
    t0 = time.perf_counter()
    try:
        tok.encode_encodings_flat([text])
    except UnsupportedConfigError as e:
        return None, str(e)
    wall = (time.perf_counter() - t0) * 1e3
    return dict(tok.last_stats["encoding_stages"])["find"], wall


def find_worst_case():
    from complexity_tokenizer import PipelineTokenizer
    tok = lower_ws()
    limit = PipelineTokenizer.encoding_limits(tok._h)["max_find_work"]
    k = 20
    while True:
        # n words that miss over 2n bytes: work = sum of (2n - j) for j < n = (3n^2 + n) / 2
        n = int(math.sqrt(2 * (1 << k) / 3))
        ms, wall = timed(tok, "A " * n)
        if ms is None:
            print(json.dumps({"find_work_target": 1 << k, "words": n, "limit": limit, "refused": wall}), flush=True)
            break
        print(json.dumps({"find_work_target": 1 << k, "words": n, "find_work": tok.last_stats["encoding"]["max_find_work"], "limit": limit,
                          "ms_find": round(ms, 3), "ms_wall_host_call": round(wall, 3)}), flush=True)
        if ms > 6000 or (1 << k) >= limit:
            break
        k += 1


def partial_worst_case():
    from complexity_tokenizer import PipelineTokenizer
    tok = lower_ws()
    limit = PipelineTokenizer.encoding_limits(tok._h)["max_find_work"]
    h = 1 << 10
    while True:
        ms, wall = timed(tok, "A" + "a" * h + " " + "a" * h + "A")
        if ms is None:
            print(json.dumps({"half_bytes": h, "limit": limit, "refused": wall}), flush=True)
            break
        print(json.dumps({"half_bytes": h, "lane_compares_about": h * h // 128, "find_work": tok.last_stats["encoding"]["max_find_work"],
                          "limit": limit, "ms_find": round(ms, 3), "ms_wall_host_call": round(wall, 3)}), flush=True)
        if ms > 6000 or h >= 1 << 15:  # (a word of more symbols is refused before the search)
            break
        h *= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--ids", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--find-worst-case", action="store_true")
    ap.add_argument("--partial-worst-case", action="store_true")
    args = ap.parse_args()
    if args.find_worst_case:
        return find_worst_case()
    if args.partial_worst_case:
        return partial_worst_case()
    from complexity_tokenizer import Normalizer, PipelineTokenizer, PostProcessor, PreTokenizer, parse_tokenizer_json
    from datagen import corpus
    from datagen.build_tokenizers import fixture_path
    with open(fixture_path("gpt2_50k", tempfile.gettempdir())) as f:
        spec = parse_tokenizer_json(json.load(f))
    top = max(spec["vocab"].values())
    added = [dict(id=top + 1, content="[CLS]", special=True), dict(id=top + 2, content="[SEP]", special=True)]
    tok = PipelineTokenizer.from_components(spec["vocab"], spec["merges"], Normalizer.sequence([Normalizer.nfkc(), Normalizer.lowercase()]),
                                            PreTokenizer.whitespace(), None, PostProcessor.bert("[CLS]", top + 1, "[SEP]", top + 2), added)
    # rows of about --ids ids: the corpus cut at blanks every so many bytes, the bytes per id from a sample
    text, off = corpus.corpus_c1()
    whole = " ".join(d.decode() for d in corpus.unpack(text, off) if d.isascii())
    sample = whole[:1 << 20]
    per_id = len(sample) / max(len(tok.encode(sample)), 1)
    width = max(int(args.ids * per_id), 8)
    rows, at = [], 0
    while len(rows) < args.rows:
        if at + width >= len(whole):
            at = 0
        end = whole.find(" ", at + width)
        end = len(whole) if end < 0 else end
        rows.append(whole[at:end])
        at = end + 1
    for _ in range(max(args.warmup, 1)):
        tok.encode_encodings_flat(rows)
    runs, walls = [], []
    for _ in range(max(args.reps, 1)):
        t0 = time.perf_counter()
        tok.encode_encodings_flat(rows)
        walls.append((time.perf_counter() - t0) * 1e3)
        runs.append(dict(tok.last_stats["stages"] + tok.last_stats["encoding_stages"]))
    st = tok.last_stats
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    print(json.dumps({"rows": len(rows), "bytes_in": st["bytes_in"], "words": st["words"], "ids": st["ids"],
                      "ids_per_row": round(st["ids"] / len(rows), 1), "cells": st["encoding"]["cells"],
                      "max_find_work": st["encoding"]["max_find_work"], "reps": len(runs),
                      "ms_stages_median": [[k, round(v, 3)] for k, v in med.items()], "ms_device": round(sum(med.values()), 3),
                      "ms_wall_host_call_median": round(statistics.median(walls), 3)}), flush=True)


if __name__ == "__main__":
    main()
