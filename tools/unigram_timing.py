#!/usr/bin/env python3
"""Unigram trainer and model timing (complexity_tokenizer.UnigramTrainer / UnigramModel,
csrc/unigram.hip): where a training's time goes, phase by phase, and what the model's encode costs.
Prints one JSON line.

usage: python tools/unigram_timing.py [n_docs] [vocab_size] [runs] [--oracle]

Corpus: the C2 sample of tools/trainer_timing.py (n_docs = 5,000, seed 31), every document a text,
the reference's defaults apart from vocab_size (8,000).  One warm-up training, then `runs` timed ones
on a new trainer each; the medians of their stats() are reported: HIP-event ms of the Metaspace
kernels (ms_text), the substring counts (ms_count), the char index and the lattice (ms_lattice), the
Viterbi searches and backtracks of all iterations (ms_viterbi, and per iteration), and the host wall
time of the whole call (ms_host: it holds the NFC pre-tokenization, the merging of the chunks'
counts, the seed sort, the string table and the M-steps).  Then the trained model encodes the same
documents as one batch (median wall ms of `runs` calls after a warm-up) and one document of 20,000
chars.  --oracle adds the wall time of the Python restatement (tests/unigram_ref.py) on one CPU core."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "complexity-tokenizer_amd")]

from complexity_tokenizer import UnigramTrainer  # noqa: E402
from datagen import corpus  # noqa: E402


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n_docs = int(args[0]) if len(args) > 0 else 5_000
    vocab_size = int(args[1]) if len(args) > 1 else 8_000
    runs = int(args[2]) if len(args) > 2 else 3
    text, off = corpus.corpus_c2(n_docs, seed=31)
    texts = [d.decode() for d in corpus.unpack(text, off)]
    stats, model = [], None
    for k in range(1 + runs):
        tr = UnigramTrainer(vocab_size=vocab_size)
        t = time.perf_counter()
        model = tr.train_from_iterator(texts)
        wall = 1e3 * (time.perf_counter() - t)
        st = tr.stats()
        st["wall_ms"] = wall
        if k >= 1:
            stats.append(st)
    med = {k: _median([s[k] for s in stats]) for k in stats[0] if k != "vocab_sizes"}
    out = {"what": "Unigram training of %d C2 docs (%d bytes), vocab_size %d, the other arguments default: medians of %d "
                   "trainings after 1 warm-up" % (len(texts), sum(len(t.encode()) for t in texts), vocab_size, runs)}
    out["train"] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in med.items()}
    out["train"]["vocab_sizes"] = stats[0]["vocab_sizes"]
    out["train"]["ms_viterbi_per_iteration"] = round(med["ms_viterbi"] / max(1, med["iterations"]), 3)
    out["train"]["final_vocab"] = model.vocab_size
    enc = []
    for k in range(1 + runs):
        t = time.perf_counter()
        ids, _ = model.encode_batch_flat(texts)
        enc.append(1e3 * (time.perf_counter() - t))
    long_text = "".join(texts)[:20_000]
    one = []
    for k in range(1 + runs):
        t = time.perf_counter()
        model.encode_batch_flat([long_text])
        one.append(1e3 * (time.perf_counter() - t))
    out["encode"] = {"batch_wall_ms": round(_median(enc[1:]), 3), "batch_ids": int(len(ids)),
                     "one_text_of_%d_chars_wall_ms" % len(long_text): round(_median(one[1:]), 3)}
    if "--oracle" in sys.argv:
        from tests.unigram_ref import RefUnigramTrainer
        t = time.perf_counter()
        ref = RefUnigramTrainer(vocab_size=vocab_size)
        ref.train_from_iterator(texts)
        out["oracle"] = {"wall_ms": round(1e3 * (time.perf_counter() - t), 1), "iterations": ref.iterations,
                         "note": "tests/unigram_ref.py on one CPU core"}
    else:
        out["oracle"] = "not measured"
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
