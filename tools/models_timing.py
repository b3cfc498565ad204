#!/usr/bin/env python3
"""Stage times of the stand-alone models' encode (complexity_tokenizer.WordLevelModel, CharBpeModel,
ByteLevelBpeModel; csrc/strmerge.hip): HIP-event ms of the start bits, the word list, the initial
symbols with the merges, and the emit (ctok_models_stage_ms).  Prints one JSON line per
measurement and asserts nothing.

usage: python tools/models_timing.py corpus [n_docs] [runs]
           the first n_docs (default 2,000) C1 docs through the three models: the BPE models on
           BpeTrainer(vocab_size=300, min_frequency=1)'s vocab and merges, the word-level model on
           the 2,000 most frequent words; 1 warm-up call, then the median of `runs` (default 5)
       python tools/models_timing.py worst N [N ...]
           one word of N symbols that takes N - 1 rounds, each a single merge: "a" * N under the
           merges (a, a), (aa, aa), (aaaa, aaaa), ... -- the basis of the cap on a word's symbols
           (csrc/strmerge_internal.h kMaxWordSymbols).  N above the cap is refused by the library;
           a candidate is skipped when four times the time of the one before is above 6 s."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "complexity-tokenizer_amd")]

from complexity_tokenizer import BpeTrainer, ByteLevelBpeModel, CharBpeModel, WordLevelModel  # noqa: E402
from complexity_tokenizer.models import models_limits  # noqa: E402

STAGES = ("starts", "word_list", "merge", "emit")


def _run(model, texts, runs):
    rows = []
    for k in range(1 + runs):
        t = time.perf_counter()
        ids, _ = model.encode_batch_flat(texts)
        wall = 1e3 * (time.perf_counter() - t)
        if k:
            rows.append(model.stage_ms() + [wall])
    med = [sorted(r[i] for r in rows)[len(rows) // 2] for i in range(len(STAGES) + 1)]
    out = {s: round(v, 4) for s, v in zip(STAGES, med)}
    out.update(device_ms=round(sum(med[:-1]), 4), wall_ms=round(med[-1], 3), ids=int(len(ids)))
    return out


def corpus_times(n_docs, runs):
    from datagen import corpus
    text, off = corpus.corpus_c1()
    docs = [d.decode() for d in corpus.unpack(text, off)][:n_docs]
    vocab, merges = BpeTrainer(vocab_size=300, min_frequency=1).train(docs[:600])
    counts = {}
    for d in docs:
        for w in d.split():
            counts[w] = counts.get(w, 0) + 1
    words = sorted(counts, key=lambda w: (-counts[w], w))[:2000]
    base = {"docs": len(docs), "bytes": sum(len(d.encode()) for d in docs), "limits": models_limits()}
    for name, model in (("char_bpe", CharBpeModel(vocab, merges, "")), ("byte_level_bpe", ByteLevelBpeModel(vocab, merges)),
                        ("word_level", WordLevelModel({w: i for i, w in enumerate(words)}, words[0]))):
        print(json.dumps(dict(base, model=name, merges=len(merges), **_run(model, docs, runs))), flush=True)


def worst_times(sizes):
    prev = None
    for n in sizes:
        if prev is not None and 4 * prev > 6_000:
            print(json.dumps({"worst_word_symbols": n, "skipped": "four times the time before is above 6 s"}), flush=True)
            continue
        merges, t = [], "a"
        while 2 * len(t) <= n:
            merges.append((t, t))
            t += t
        model = ByteLevelBpeModel({"<unk>": 0, "a": 1}, merges, add_prefix_space=False)
        try:
            r = _run(model, ["a" * n], 1)
        except NotImplementedError as e:  # UnsupportedConfigError: above the cap
            print(json.dumps({"worst_word_symbols": n, "refused": str(e)}), flush=True)
            continue
        prev = r["merge"]
        print(json.dumps(dict(worst_word_symbols=n, merges=len(merges), **r)), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "worst":
        worst_times([int(a) for a in sys.argv[2:]])
    else:
        a = sys.argv[2:] if len(sys.argv) > 1 and sys.argv[1] == "corpus" else sys.argv[1:]
        corpus_times(int(a[0]) if a else 2000, int(a[1]) if len(a) > 1 else 5)
