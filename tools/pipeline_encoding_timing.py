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
byte at every position.

--windows: the padded batches and stride windows on one batch: --texts seeded texts of
tests/pipeline_cases.random_texts (--max-words words at most each) over its seeded vocabulary, Whitespace,
no post-processor; --max-length, --stride, --padding.  (a) encode_windows_device over torch tensors, every
array and then all but the offsets: the medians and the spread of the plan and write stages, the bytes the
write kernel wrote and its rate, next to a device-to-device hipMemcpyAsync of as many bytes timed in the
same run.  (b) the whole encode_windows call against the route through Encodings: `__call__` with the same
options and the lists stacked into numpy arrays.  Needs a HIP device.
Usage: tools/pipeline_encoding_timing.py [--rows N] [--ids N] [--reps R] [--warmup W] | --find-worst-case | --partial-worst-case
       | --windows [--texts N] [--max-words N] [--max-length M] [--stride S] [--padding P]
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


def spread(xs):
    xs = sorted(xs)
    return {"median": round(statistics.median(xs), 4), "min": round(xs[0], 4), "max": round(xs[-1], 4)}


def stack_encodings(batch, width, pad_id):
    """the route that exists without the arrays: the Encodings' lists, main and overflowing, stacked"""
    import numpy as np
    wins = [w for e in batch.encodings() for w in [e] + e.overflowing]
    out = {k: np.zeros((len(wins), width), dtype=np.uint32) for k in ("input_ids", "attention_mask", "token_type_ids", "special_tokens_mask")}
    out["input_ids"][:] = pad_id
    out["special_tokens_mask"][:] = 1
    offs = np.zeros((len(wins), width, 2), dtype=np.uint64)
    for i, w in enumerate(wins):
        n = len(w.ids)
        out["input_ids"][i, :n], out["attention_mask"][i, :n] = w.ids, w.attention_mask
        out["token_type_ids"][i, :n], out["special_tokens_mask"][i, :n] = w.type_ids, w.special_tokens_mask
        if w.offsets:
            offs[i, :len(w.offsets)] = w.offsets
    out["offset_mapping"] = offs
    return out


def windows(args):
    import ctypes

    import numpy as np
    import torch

    from complexity_tokenizer import PipelineTokenizer, PreTokenizer
    from tests import pipeline_cases as pc
    vocab, merges = pc.random_vocab(11)
    tok = PipelineTokenizer.from_components(vocab, merges, None, PreTokenizer.whitespace(), None, None,
                                            [dict(id=len(vocab), content="<pad>", special=True)])
    texts = pc.random_texts(51, args.texts, vocab, max_words=args.max_words)
    m, stride, padding = args.max_length, args.stride, None if args.padding == "none" else args.padding
    reps, warmup = max(args.reps, 3), max(args.warmup, 1)
    first = tok.encode_windows(texts, max_length=m, stride=stride, padding=padding)
    n, w = first["input_ids"].shape
    dev = torch.device("cuda", 0)
    raw = [t.encode() for t in texts]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    d_text = torch.from_numpy(np.frombuffer(b"".join(raw) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    cells = [torch.empty(n * w, dtype=torch.int32, device=dev) for _ in range(6)]
    offsets = torch.empty(2 * n * w, dtype=torch.int64, device=dev)
    recs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)]
    win_row = torch.empty(n, dtype=torch.int32, device=dev)
    row_win = torch.empty(len(texts) + 1, dtype=torch.int64, device=dev)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    result = {"texts": len(texts), "max_length": m, "stride": stride, "padding": padding, "windows": n, "width": w, "reps": reps}
    for name, with_offsets in (("all_arrays", True), ("without_offsets", False)):
        plan, write = [], []
        for i in range(warmup + reps):
            tok.encode_windows_device(d_text.data_ptr(), d_off.data_ptr(), len(texts), int(off[-1]), d_ids=cells[0].data_ptr(), cap=n * w,
                                      d_win_len=recs[0].data_ptr(), d_win_row=win_row.data_ptr(), win_cap=n, d_row_win=row_win.data_ptr(),
                                      max_length=m, stride=stride, padding=padding, d_attention=cells[1].data_ptr(),
                                      d_type_ids=cells[2].data_ptr(), d_special=cells[3].data_ptr(),
                                      d_offsets=offsets.data_ptr() if with_offsets else 0, d_word_ids=cells[4].data_ptr(),
                                      d_sequence_ids=cells[5].data_ptr(), d_win_start=recs[1].data_ptr(), d_win_off_len=recs[2].data_ptr(),
                                      d_win_seq_len=recs[3].data_ptr())
            if i >= warmup:
                st = dict(tok.last_stats["window_stages"])
                plan.append(st["plan"])
                write.append(st["write"])
        nbytes = tok.last_stats["windows"]["bytes_written"]
        # the yardstick: a device-to-device copy of as many bytes
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        copies = []
        for i in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), nbytes, 3, None)  # hipMemcpyDeviceToDevice
            b.record()
            torch.cuda.synchronize()
            assert rc == 0
            if i >= warmup:
                copies.append(a.elapsed_time(b))
        del src, dst
        wr_ms, cp_ms = statistics.median(write), statistics.median(copies)
        result[name] = {"bytes_written": nbytes, "ms_plan": spread(plan), "ms_write": spread(write),
                        "write_GBps": round(nbytes / wr_ms / 1e6, 1), "ms_memcpy_d2d": spread(copies),
                        "memcpy_GBps_of_bytes_copied": round(nbytes / cp_ms / 1e6, 1)}
    new, old = [], []
    kw = dict(max_length=m, stride=stride, padding=padding)
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        got = tok.encode_windows(texts, return_offsets=True, **kw)
        t1 = time.perf_counter()
        want = stack_encodings(tok(texts, truncation=True, **kw), w, tok._pad_id_token()[0])
        t2 = time.perf_counter()
        if i >= warmup:
            new.append((t1 - t0) * 1e3)
            old.append((t2 - t1) * 1e3)
    assert all(np.array_equal(got[k], want[k]) for k in want), "the two routes differ"
    result["ms_encode_windows_call"] = spread(new)
    result["ms_call_and_stack"] = spread(old)
    result["speedup"] = round(statistics.median(old) / statistics.median(new), 1)
    print(json.dumps(result), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--ids", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--find-worst-case", action="store_true")
    ap.add_argument("--partial-worst-case", action="store_true")
    ap.add_argument("--windows", action="store_true")
    ap.add_argument("--texts", type=int, default=20000)
    ap.add_argument("--max-words", type=int, default=12)
    ap.add_argument("--max-length", type=int, default=128)
    ap.add_argument("--stride", type=int, default=32)
    ap.add_argument("--padding", default="max_length", choices=["none", "longest", "max_length"])
    args = ap.parse_args()
    if args.windows:
        return windows(args)
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
