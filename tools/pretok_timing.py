#!/usr/bin/env python3
"""Per-stage HIP-event times of complexity_tokenizer.PreTokenizer on a seeded corpus from datagen.

For each of a few pre-tokenizers the batch goes through pre_tokenize_packed twice (the first call
grows the handle's device buffers); the second call's ctok_pretokenizer_stage_ms values are printed
with the rate over the input bytes, one JSON line per pre-tokenizer.  With --segment the same bytes
also go through the gpt2_50k tokenizer's encode once, for k_segment's time beside them (scale only:
k_segment splits, classifies and routes pieces, it does not write words).  With --regex the batch
goes through split('(?:\\d)+', regex=True), which runs as a DFA, and split('\\d+'), the class atom beside
it, alternating, and the median split-stage times and their ratio are printed.  With --regex-worst the
worst case of the DFA path is timed instead of the corpus: one word of R code points under '.+' (about
R * R / 2 steps) for R = 2^LO .. 2^HI, the sweep that fixes knobs.h kMaxRegexRun (R above the built-in
cap is refused and printed as such).  Needs a HIP device.
Usage: tools/pretok_timing.py [--docs N] [--corpus c3|c5nfc] [--segment] [--regex] [--regex-worst LO HI]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "complexity-tokenizer_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def stage_ms(pt, name):
    return sum(ms for n, ms in pt.last_stats["stages"] if n == name)


def regex_rows(text, off, corpus_name, docs, reps=7):
    """the DFA path against the class path of the same split, alternating, after a warm-up of both"""
    from complexity_tokenizer import PreTokenizer as P
    arms = {"split('(?:\\d)+', 'Removed', regex=True)": P.split(r"(?:\d)+", "Removed", regex=True), "split('\\d+', 'Removed')": P.split(r"\d+", "Removed")}
    times = {k: [] for k in arms}
    out = {}
    for k, pt in arms.items():
        out[k] = pt.pre_tokenize_packed(text, off)
    a, b = out.values()
    assert all((x == y).all() for x, y in zip(a, b)), "the two arms differ"
    for _ in range(reps):
        for k, pt in arms.items():
            pt.pre_tokenize_packed(text, off)
            times[k].append(stage_ms(pt, "split"))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    nb = int(off[-1])
    for k, v in times.items():
        print(json.dumps({"pre_tokenizer": k, "corpus": corpus_name, "docs": docs, "bytes_in": nb, "reps": reps,
                          "ms_split_median": round(med[k], 3), "ms_split_min": round(min(v), 3), "ms_split_max": round(max(v), 3),
                          "mb_per_s": round(nb / 1e6 / (med[k] / 1e3), 1)}), flush=True)
    dfa, cls = med.values()
    print(json.dumps({"regex_over_class_ratio": round(dfa / cls, 3)}), flush=True)


def regex_worst(lo, hi):
    import numpy as np
    from complexity_tokenizer import PreTokenizer as P, UnsupportedConfigError
    pt = P.split(".+", "Isolated", regex=True)
    pt.pre_tokenize_packed(np.frombuffer(b"warm up", dtype=np.uint8), np.array([0, 7], dtype=np.uint64))
    for e in range(lo, hi + 1):
        r = 1 << e
        text = np.full(r, ord("a"), dtype=np.uint8)
        off = np.array([0, r], dtype=np.uint64)
        try:
            pt.pre_tokenize_packed(text, off)
        except UnsupportedConfigError:
            print(json.dumps({"worst_case_run": r, "refused": True, "cap": P.limits()["max_regex_run"]}), flush=True)
            continue
        print(json.dumps({"worst_case_run": r, "pattern": ".+", "steps": r * (r + 1) // 2, "ms_split": round(stage_ms(pt, "split"), 3)}),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--corpus", choices=("c3", "c5nfc"), default="c5nfc")
    ap.add_argument("--segment", action="store_true")
    ap.add_argument("--regex", action="store_true")
    ap.add_argument("--regex-worst", type=int, nargs=2, metavar=("LO", "HI"))
    args = ap.parse_args()
    from complexity_tokenizer import PreTokenizer
    from datagen import corpus
    if args.regex_worst:
        return regex_worst(*args.regex_worst)
    text, off = (corpus.corpus_c3 if args.corpus == "c3" else corpus.corpus_c5nfc)(n_docs=args.docs)
    if args.regex:
        return regex_rows(text, off, args.corpus, args.docs)
    P = PreTokenizer
    progs = {
        "whitespace": P.whitespace(), "bert": P.bert(), "byte_level": P.byte_level(), "sequence([bert, digits(True)])":
        P.sequence([P.bert(), P.digits(True)]), "punctuation": P.punctuation(), "gpt2": P.gpt2(), "metaspace": P.metaspace(),
        "unicode_scripts": P.unicode_scripts(), "split(' ', 'MergedWithNext')": P.split(" ", "MergedWithNext"),
        "split('\\\\d+', 'Removed')": P.split(r"\d+", "Removed"),
    }
    for name, pt in progs.items():
        pt.pre_tokenize_packed(text, off)
        t0 = time.perf_counter()
        pt.pre_tokenize_packed(text, off)
        wall = (time.perf_counter() - t0) * 1e3
        st = pt.last_stats
        dev = sum(ms for _, ms in st["stages"])
        print(json.dumps({"pre_tokenizer": name, "corpus": args.corpus, "docs": args.docs, "bytes_in": st["bytes_in"],
                          "bytes_out": st["bytes_out"], "words": st["words"], "steps_rewriting": st["steps_rewriting"],
                          "ms_stages": [[n, round(ms, 3)] for n, ms in st["stages"]], "ms_device": round(dev, 3),
                          "mb_per_s": round(st["bytes_in"] / 1e6 / (dev / 1e3), 1) if dev else None,
                          "ms_wall_host_call": round(wall, 3)}), flush=True)
    if args.segment:
        import numpy as np
        import torch
        from complexity_tokenizer import Tokenizer
        from datagen.build_tokenizers import fixture_path
        import tempfile
        tok = Tokenizer.from_file(fixture_path("gpt2_50k", tempfile.gettempdir()))
        nb, n_docs = int(off[-1]), len(off) - 1
        d_text = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        d_text[:nb] = torch.from_numpy(np.asarray(text[:nb])).cuda()
        d_off = torch.from_numpy(np.asarray(off).astype(np.int64)).cuda()
        cap = nb + n_docs + 16
        d_ids = torch.empty(cap, dtype=torch.int32, device="cuda")
        d_toff = torch.empty(n_docs + 1, dtype=torch.int64, device="cuda")
        a = (d_text.data_ptr(), d_off.data_ptr(), n_docs, nb, d_ids.data_ptr(), cap, d_toff.data_ptr())
        for _ in range(3):
            tok.encode_packed_device(*a)
        tok.encode_packed_device(*a, timing=True)
        ms = tok.last_stats["ms_segment"]
        print(json.dumps({"k_segment": "gpt2_50k encode, timed call", "bytes_in": nb, "ms_segment": round(ms, 3),
                          "mb_per_s": round(nb / 1e6 / (ms / 1e3), 1) if ms else None}), flush=True)


if __name__ == "__main__":
    main()
