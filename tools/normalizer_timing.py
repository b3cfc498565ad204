#!/usr/bin/env python3
"""Per-step HIP-event times of complexity_tokenizer.Normalizer on a seeded corpus from datagen.

For each of a few normalisers the batch goes through normalize_packed twice (the first call grows
the handle's device buffers); the second call's ctok_normalizer_stage_ms values are printed, one
JSON line per normaliser.  Needs a HIP device.
Usage: tools/normalizer_timing.py [--docs N] [--corpus c3|c5nfc]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20000)
    ap.add_argument("--corpus", choices=("c3", "c5nfc"), default="c5nfc")
    args = ap.parse_args()
    from complexity_tokenizer import Normalizer
    from datagen import corpus
    text, off = (corpus.corpus_c3 if args.corpus == "c3" else corpus.corpus_c5nfc)(n_docs=args.docs)
    N = Normalizer
    progs = {
        "nfc": N.nfc(), "nfd": N.nfd(), "nfkc": N.nfkc(), "nfkd": N.nfkd(), "lowercase": N.lowercase(), "strip": N.strip(),
        "strip_accents": N.strip_accents(), "replace(' ', '_')": N.replace(" ", "_"), "bert": N.bert(),
        "sequence(nfkc, lowercase)": N.sequence([N.nfkc(), N.lowercase()]),
    }
    for name, nz in progs.items():
        nz.normalize_packed(text, off)
        t0 = time.perf_counter()
        out, _ = nz.normalize_packed(text, off)
        wall = (time.perf_counter() - t0) * 1e3
        st = nz.last_stats
        print(json.dumps({"normalizer": name, "corpus": args.corpus, "docs": args.docs, "bytes_in": st["bytes_in"],
                          "bytes_out": st["bytes_out"], "steps_changed": st["steps_changed"],
                          "ms_steps": [[n, round(ms, 3)] for n, ms in st["stages"]],
                          "ms_device": round(sum(ms for _, ms in st["stages"]), 3), "ms_wall_host_call": round(wall, 3)}))


if __name__ == "__main__":
    main()
