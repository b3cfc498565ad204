#!/usr/bin/env python3
"""WordPiece trainer timing (complexity_tokenizer.WordPieceTrainer, csrc/wordpiece.hip): what keeping
every position's longest match and the pair table on the device buys over walking every word and
counting all pairs again in every round (the reference's literal recount, CTOK_WP_TRAIN_RECOUNT=1,
on the same kernels).  Beside them, as context: this commit's BpeTrainer on the same texts (not a build of the
parent commit; its kernels are the parent's) and the wall time of the Python oracle (tests/wordpiece_ref.py).  Prints one JSON line.

usage: python tools/wordpiece_timing.py [n_docs] [merges] [runs] [--no-oracle]

Corpus: the C2 sample of tools/trainer_timing.py (n_docs = 20,000, seed 31) at vocab_size = initial
vocab + merges (2,000), min_frequency 2.  Each arm runs in a fresh child process: 2 warm-up
trainings, then `runs` timed ones on a new trainer each; the medians of their stats() are reported,
with the device ms per round split into add / walk / best (HIP events; pairs: the counts from the
words, initial and rebuilds) and ms_per_round_wall = ms_host / rounds from the host clock."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "complexity-tokenizer_amd")]

from complexity_tokenizer import BpeTrainer, WordPieceTrainer  # noqa: E402
from datagen import corpus  # noqa: E402


def _texts(n_docs):
    text, off = corpus.corpus_c2(n_docs, seed=31)
    return [d.decode() for d in corpus.unpack(text, off)]


def _child_wp(n_docs, merges, runs):
    texts = _texts(n_docs)
    initial = WordPieceTrainer(vocab_size=0)
    initial.train_from_iterator(texts)
    initial = initial.vocab_size
    out = []
    for k in range(2 + runs):
        tr = WordPieceTrainer(vocab_size=initial + merges, min_frequency=2)
        t = time.perf_counter()
        tr.train_from_iterator(texts)
        wall = 1e3 * (time.perf_counter() - t)
        st = tr.stats()
        st["wall_ms"] = wall
        if k >= 2:
            out.append(st)
    print(json.dumps({"docs": len(texts), "bytes": sum(len(t.encode()) for t in texts), "initial_vocab": initial,
                      "runs": out}), flush=True)


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
    print(json.dumps({"runs": out}), flush=True)


def _child_oracle(n_docs, merges, runs):
    from tests.wordpiece_ref import RefWordPieceTrainer
    texts = _texts(n_docs)
    ref = RefWordPieceTrainer(vocab_size=0)
    words = ref.word_counts(texts)
    ref.train_words(words)
    ref = RefWordPieceTrainer(vocab_size=len(ref.vocab) + merges, min_frequency=2)
    t = time.perf_counter()
    ref.train_words(words)
    print(json.dumps({"wall_ms": 1e3 * (time.perf_counter() - t), "merges": len(ref.merges),
                      "note": "tests/wordpiece_ref.py from the word counts on (its incremental mode, on one CPU core)"}),
          flush=True)


def _median(runs, key):
    v = sorted(r[key] for r in runs)
    return v[len(v) // 2]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    n_docs = int(args[0]) if len(args) > 0 else 20_000
    merges = int(args[1]) if len(args) > 1 else 2_000
    runs = int(args[2]) if len(args) > 2 else 3
    arms = [("resident", "--child-wp", {}), ("recount", "--child-wp", {"CTOK_WP_TRAIN_RECOUNT": "1"}),
            ("bpe_trainer", "--child-bpe", {})]
    if "--no-oracle" not in sys.argv:
        arms.append(("oracle", "--child-oracle", {}))
    res = {}
    for arm, child, env_add in arms:
        env = dict(os.environ)
        for k in ("CTOK_WP_TRAIN_RECOUNT", "CTOK_BPE_TRAIN_RECOUNT", "CTOK_BPE_TRAIN_SLOTS"):
            env.pop(k, None)
        env.update(env_add)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), child, str(n_docs), str(merges), str(runs)],
                           env=env, check=True, capture_output=True, text=True)
        res[arm] = json.loads(r.stdout.strip().splitlines()[-1])
    out = {"what": "WordPiece training of %d C2 docs (%d bytes), %d rounds asked: medians of %d trainings after 2 "
                   "warm-up trainings, each arm in a fresh process; bpe_trainer is this commit's BpeTrainer" % (res["resident"]["docs"], res["resident"]["bytes"], merges, runs)}
    for arm in ("resident", "recount"):
        rr = res[arm]["runs"]
        med = {k: _median(rr, k) for k in rr[0]}
        n = max(1, med["merges"])
        out[arm] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in med.items()}
        out[arm].update({
            "ms_per_round_add": round(med["ms_add"] / n, 5), "ms_per_round_walk": round(med["ms_walk"] / n, 5),
            "ms_per_round_best": round(med["ms_best"] / n, 5), "ms_per_round_pairs": round(med["ms_pairs"] / n, 5),
            "ms_per_round_device": round((med["ms_add"] + med["ms_walk"] + med["ms_best"] + med["ms_pairs"]) / n, 5),
            "ms_per_round_wall": round(med["ms_host"] / n, 5),
        })
    rb = res["bpe_trainer"]["runs"]
    n = max(1, _median(rb, "n_merges"))
    out["bpe_trainer"] = {"merges": _median(rb, "n_merges"), "unique_words": _median(rb, "unique_words"),
                          "ms_count": round(_median(rb, "ms_count"), 3), "ms_host": round(_median(rb, "ms_host"), 2),
                          "wall_ms": round(_median(rb, "wall_ms"), 2),
                          "ms_per_merge_device": round((_median(rb, "ms_best") + _median(rb, "ms_merges") + _median(rb, "ms_pairs")) / n, 5),
                          "ms_per_merge_wall": round(_median(rb, "ms_host") / n, 5),
                          "note": "this commit's BpeTrainer.train on the same texts, not a build of the parent commit (no NFC, no "
                                  "Lowercase; its kernels are the parent's)"}
    out["oracle"] = res.get("oracle", "not measured")
    out["recount_over_resident_device"] = round(out["recount"]["ms_per_round_device"] / max(out["resident"]["ms_per_round_device"], 1e-9), 2)
    out["recount_over_resident_wall"] = round(out["recount"]["ms_per_round_wall"] / max(out["resident"]["ms_per_round_wall"], 1e-9), 2)
    out["runs"] = {arm: res[arm].get("runs") for arm in res if arm != "oracle"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] in ("--child-wp", "--child-bpe", "--child-oracle"):
        {"--child-wp": _child_wp, "--child-bpe": _child_bpe, "--child-oracle": _child_oracle}[sys.argv[1]](
            int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    else:
        main()
