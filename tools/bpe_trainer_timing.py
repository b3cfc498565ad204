#!/usr/bin/env python3
"""Classic BPE trainer timing (complexity_tokenizer.BpeTrainer, csrc/bpe_train.hip): what the pair
table that stays on the device buys over counting all pairs again before every merge (the
reference's literal algorithm, CTOK_BPE_TRAIN_RECOUNT=1, on the same kernels), and beside them the
INL Trainer's per-merge cost on the same words.  Prints one JSON line.

usage: python tools/bpe_trainer_timing.py [n_docs] [merges] [runs]

Corpus: the C2 sample of tools/trainer_timing.py (n_docs = 20,000, seed 31) at vocab_size = initial
vocab + merges (2,000).  Each arm runs in a fresh child process: 2 warm-up trainings, then `runs`
timed ones on a new trainer each; the medians of their stats() are reported, with
ms_per_merge_device = (ms_best + ms_merges + ms_pairs) / merges from HIP events and
ms_per_merge_wall = ms_host / merges from the host clock (ms_host: the training after the counting,
the initial vocabulary and the upload of the words included)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "complexity-tokenizer_amd")]

from complexity_tokenizer import BpeTrainer, Trainer  # noqa: E402
from datagen import corpus  # noqa: E402


def _texts(n_docs):
    text, off = corpus.corpus_c2(n_docs, seed=31)
    return [d.decode() for d in corpus.unpack(text, off)]


def _child_bpe(n_docs, merges, runs):
    texts = _texts(n_docs)
    initial = len(BpeTrainer(vocab_size=0).train(texts)[0])
    out = []
    for k in range(2 + runs):
        tr = BpeTrainer(vocab_size=initial + merges, min_frequency=2)
        t = time.perf_counter()
        _, m = tr.train(texts)
        wall = 1e3 * (time.perf_counter() - t)
        st = tr.stats()
        st["wall_ms"] = wall
        st["n_merges"] = len(m)
        if k >= 2:
            out.append(st)
    print(json.dumps({"docs": len(texts), "bytes": sum(len(t.encode()) for t in texts), "initial_vocab": initial,
                      "runs": out}), flush=True)


def _child_inl(n_docs, merges, runs):
    texts = _texts(n_docs)
    words = BpeTrainer().word_counts(texts)
    raw = {w.encode(): c for w, c in words.items() if c >= 2}
    n_bytes = len({b for w in raw for b in w})
    out = []
    for k in range(2 + runs):
        tr = Trainer(vocab_size=4 + n_bytes + merges, min_frequency=2)
        t = time.perf_counter()
        tr.train_from_word_freqs(raw)
        wall = 1e3 * (time.perf_counter() - t)
        tm = tr.timing()
        tm["wall_ms"] = wall
        tm["n_merges"] = tr.num_merges
        if k >= 2:
            out.append(tm)
    print(json.dumps({"unique_words": len(raw), "runs": out}), flush=True)


def _median(runs, key):
    v = sorted(r[key] for r in runs)
    return v[len(v) // 2]


def main():
    n_docs = int(sys.argv[1]) if len(sys.argv) > 1 else 20_000
    merges = int(sys.argv[2]) if len(sys.argv) > 2 else 2_000
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    res = {}
    for arm, child, env_add in (("resident", "--child-bpe", {}), ("recount", "--child-bpe", {"CTOK_BPE_TRAIN_RECOUNT": "1"}),
                                ("inl_trainer", "--child-inl", {})):
        env = dict(os.environ)
        env.pop("CTOK_BPE_TRAIN_RECOUNT", None)
        env.pop("CTOK_BPE_TRAIN_SLOTS", None)
        env.update(env_add)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), child, str(n_docs), str(merges), str(runs)],
                           env=env, check=True, capture_output=True, text=True)
        res[arm] = json.loads(r.stdout.strip().splitlines()[-1])
    out = {"what": "classic BPE training of %d C2 docs (%d bytes), %d merges asked: medians of %d trainings after 2 "
                   "warm-up trainings, each arm in a fresh process" % (res["resident"]["docs"], res["resident"]["bytes"], merges, runs)}
    for arm in ("resident", "recount"):
        rr = res[arm]["runs"]
        n = max(1, _median(rr, "n_merges"))
        med = {k: _median(rr, k) for k in rr[0]}
        out[arm] = {
            "merges": med["n_merges"], "unique_words": med["unique_words"], "initial_symbols": med["initial_symbols"],
            "table_capacity": med["table_capacity"], "rebuilds": med["rebuilds"],
            "ms_count": round(med["ms_count"], 3), "ms_pairs": round(med["ms_pairs"], 3), "ms_best": round(med["ms_best"], 3),
            "ms_merges": round(med["ms_merges"], 3), "ms_host": round(med["ms_host"], 2), "wall_ms": round(med["wall_ms"], 2),
            "ms_per_merge_device": round((med["ms_best"] + med["ms_merges"] + med["ms_pairs"]) / n, 5),
            "ms_per_merge_wall": round(med["ms_host"] / n, 5),
        }
    ri = res["inl_trainer"]["runs"]
    n = max(1, _median(ri, "n_merges"))
    out["inl_trainer"] = {"merges": _median(ri, "n_merges"), "unique_words": res["inl_trainer"]["unique_words"],
                          "ms_pairs": round(_median(ri, "ms_pairs"), 3), "ms_merges": round(_median(ri, "ms_merges"), 2),
                          "ms_heap": round(_median(ri, "ms_heap"), 2), "wall_ms": round(_median(ri, "wall_ms"), 2),
                          "ms_per_merge": round((_median(ri, "ms_merges") + _median(ri, "ms_heap")) / n, 5),
                          "note": "Trainer.train_from_word_freqs on the same words of count >= 2 (host clock around "
                                  "each merge's kernel, drain and map update; its code is unchanged)"}
    out["recount_over_resident_device"] = round(out["recount"]["ms_per_merge_device"] / max(out["resident"]["ms_per_merge_device"], 1e-9), 2)
    out["recount_over_resident_wall"] = round(out["recount"]["ms_per_merge_wall"] / max(out["resident"]["ms_per_merge_wall"], 1e-9), 2)
    out["runs"] = {arm: res[arm]["runs"] for arm in res}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("--child-bpe", "--child-inl"):
        (_child_bpe if sys.argv[1] == "--child-bpe" else _child_inl)(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
