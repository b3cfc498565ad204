#!/usr/bin/env python3
"""Per-stage HIP-event times of complexity_tokenizer.PipelineTokenizer on a seeded corpus from datagen.

The batch goes through encode_packed --warmup times (the first call grows the handle's device
buffers), then --reps times; the median of every stage of ctok_pipeline_stage_ms is printed with the
rate over the input bytes, one JSON line.  The pipelines use the gpt2_50k fixture's vocab and merges:
  default                 the file as it is: NFC -> ByteLevel
  nfkc_lower_whitespace   Sequence[NFKC, Lowercase] -> Whitespace over the same tables
With --worst-case it times instead one call, after a warm-up, over the single word "a" * N under the
merges (a, a), (aa, aa), ... for N = 2048 .. 32768: the basis of the cap on a segment's symbols
(DESIGN.md 4.6k).  With --added-worst-case it times the segments stage under the added-token set that
costs the most compares a byte: 127 tokens of 64 bytes, "<" * 62 and one more char each, that share
the first byte and never stand in a text of "<" only (the filter pass over batches of 16 MiB, 64 MiB and
the handle's bound), and the same set with a token "<" that needs white space behind it, which stands
everywhere, fails its check and so sends one thread through the whole word with every other token
compared at every byte (one word of a quarter, a half and the whole of the handle's bound): the basis of
the two work bounds there.  Needs a HIP device.
Usage: tools/pipeline_timing.py [--corpus c1|c2|c3] [--docs N] [--pipeline NAME] [--reps R] [--warmup W] | --worst-case |
       --added-worst-case
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "complexity-tokenizer_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def worst_case():
    import numpy as np
    from complexity_tokenizer import PipelineTokenizer
    levels = 15
    vocab = {"a" * (1 << k): k for k in range(levels + 1)}
    merges = [("a" * (1 << k), "a" * (1 << k)) for k in range(levels)]
    tok = PipelineTokenizer.from_components(vocab, merges)
    for n in (2048, 4096, 8192, 16384, 32768):
        text = np.frombuffer(b"a" * n, dtype=np.uint8)
        off = np.array([0, n], dtype=np.uint64)
        tok.encode_packed(text[:64], np.array([0, 64], dtype=np.uint64))  # the warm-up: tables and code resident
        t0 = time.perf_counter()
        ids, _ = tok.encode_packed(text, off)
        wall = (time.perf_counter() - t0) * 1e3
        st = tok.last_stats
        print(json.dumps({"worst_case_symbols": n, "ids": ids.tolist(), "ms_merges": round(dict(st["stages"])["merges"], 3),
                          "ms_wall_host_call": round(wall, 3)}), flush=True)


def added_worst_case():
    import numpy as np
    from complexity_tokenizer import PipelineTokenizer
    long_ones = [dict(id=100 + i, content="<" * 62 + chr(0x100 + i), special=False) for i in range(127)]

    def timed(tok, text, off):
        tok.encode_packed(text[:64], np.array([0, 64], dtype=np.uint64))  # the warm-up
        t0 = time.perf_counter()
        tok.encode_packed(text, off)
        return dict(tok.last_stats["stages"])["segments"], (time.perf_counter() - t0) * 1e3

    # (the text's char has no vocab string: no symbols, so only the segments stage works)
    tok = PipelineTokenizer.from_components({"a": 0}, [], added_tokens=long_ones)
    lim = PipelineTokenizer.limits(tok._h)
    group = sum(len(t["content"].encode()) for t in long_ones)
    per = 1 << 16  # texts of 64 KiB: unflagged words, the filter pass alone
    for n in (16 << 20, 64 << 20, lim["max_batch_bytes"] // per * per):
        text = np.frombuffer(b"<" * n, dtype=np.uint8)
        ms, wall = timed(tok, text, np.arange(0, n + 1, per, dtype=np.uint64))
        print(json.dumps({"filter_pass_bytes": n, "group_bytes": group, "bound_bytes": lim["max_batch_bytes"], "compares_bound": n * group,
                          "ms_segments": round(ms, 3), "ms_wall_host_call": round(wall, 3)}), flush=True)
    tok = PipelineTokenizer.from_components({"a": 0}, [], added_tokens=long_ones + [dict(id=99, content="<", special=False, rstrip=True)])
    cap = PipelineTokenizer.limits(tok._h)["max_flagged_word_bytes"]
    for n in (cap // 4, cap // 2, cap):
        text = np.frombuffer(b"<" * n, dtype=np.uint8)
        ms, wall = timed(tok, text, np.array([0, n], dtype=np.uint64))
        print(json.dumps({"flagged_word_bytes": n, "group_bytes": group + 1, "bound_bytes": cap, "compares_bound": n * (group + 1),
                          "ms_segments": round(ms, 3), "ms_wall_host_call": round(wall, 3), "segments": tok.last_stats["segments"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=("c1", "c2", "c3"), default="c1")
    ap.add_argument("--docs", type=int, default=None)
    ap.add_argument("--pipeline", choices=("default", "nfkc_lower_whitespace"), default="default")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--worst-case", action="store_true")
    ap.add_argument("--added-worst-case", action="store_true")
    args = ap.parse_args()
    if args.worst_case:
        return worst_case()
    if args.added_worst_case:
        return added_worst_case()
    from complexity_tokenizer import Normalizer, PipelineTokenizer, PreTokenizer, parse_tokenizer_json
    from datagen import corpus
    from datagen.build_tokenizers import fixture_path
    make = getattr(corpus, "corpus_" + args.corpus)
    text, off = make(n_docs=args.docs) if args.docs else make()
    path = fixture_path("gpt2_50k", tempfile.gettempdir())
    if args.pipeline == "default":
        tok = PipelineTokenizer.from_file(path)
    else:
        with open(path) as f:
            spec = parse_tokenizer_json(json.load(f))
        tok = PipelineTokenizer.from_components(spec["vocab"], spec["merges"], Normalizer.sequence([Normalizer.nfkc(), Normalizer.lowercase()]),
                                                PreTokenizer.whitespace(), None, None, spec["added_tokens"])
    for _ in range(max(args.warmup, 1)):
        tok.encode_packed(text, off)
    runs, walls = [], []
    for _ in range(max(args.reps, 1)):
        t0 = time.perf_counter()
        tok.encode_packed(text, off)
        walls.append((time.perf_counter() - t0) * 1e3)
        runs.append(dict(tok.last_stats["stages"]))
    st = tok.last_stats
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    dev = sum(med.values())
    print(json.dumps({"pipeline": args.pipeline, "corpus": args.corpus, "docs": st["texts"], "bytes_in": st["bytes_in"], "words": st["words"],
                      "segments": st["segments"], "symbols": st["symbols"], "ids": st["ids"], "reps": len(runs),
                      "ms_stages_median": [[k, round(v, 3)] for k, v in med.items()], "ms_device": round(dev, 3),
                      "mb_per_s": round(st["bytes_in"] / 1e6 / (dev / 1e3), 1) if dev else None,
                      "ms_wall_host_call_median": round(statistics.median(walls), 3)}), flush=True)


if __name__ == "__main__":
    main()
