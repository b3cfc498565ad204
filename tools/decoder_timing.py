#!/usr/bin/env python3
"""Per-stage HIP-event times of complexity_tokenizer.Decoder on packed tokens made from a seeded
corpus from datagen.

The tokens are the words a PreTokenizer makes of the corpus (pre_tokenize_packed's output is
decode_packed's input): `byte_level` words for the ByteLevel decoder, `metaspace` words for
Metaspace, `bert` words for the others.  For each decoder the batch goes through decode_packed twice
(the first call grows the handle's device buffers); the second call's ctok_decoder_stage_ms values
are printed with the rate over the input bytes, one JSON line per decoder.  With --ids the `bert`
words also go in as ids of their own vocabulary, for the gather's time.  Needs a HIP device.
Usage: tools/decoder_timing.py [--docs N] [--corpus c3|c5nfc] [--ids]
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
    ap.add_argument("--ids", action="store_true")
    args = ap.parse_args()
    import numpy as np
    from complexity_tokenizer import Decoder, PreTokenizer
    from datagen import corpus
    text, off = (corpus.corpus_c3 if args.corpus == "c3" else corpus.corpus_c5nfc)(n_docs=args.docs)
    P, D = PreTokenizer, Decoder
    words = {"bert": P.bert().pre_tokenize_packed(text, off), "byte_level": P.byte_level().pre_tokenize_packed(text, off),
             "metaspace": P.metaspace().pre_tokenize_packed(text, off)}
    progs = [
        ("fuse", D.fuse(), "bert"), ("byte_level", D.byte_level(), "byte_level"), ("metaspace", D.metaspace(), "metaspace"),
        ("wordpiece('##', False)", D.wordpiece("##", False), "bert"), ("wordpiece", D.wordpiece(), "bert"), ("bpe('')", D.bpe(""), "bert"),
        ("ctc", D.ctc(), "bert"), ("strip('T', 1, 1)", D.strip("T", 1, 1), "bert"), ("replace('e', 'EE')", D.replace("e", "EE"), "bert"),
        ("replace('', '-')", D.replace("", "-"), "bert"),
        ("sequence([wordpiece, replace(' ', '_'), strip('_', 1, 1)])",
         D.sequence([D.wordpiece(), D.replace(" ", "_"), D.strip("_", 1, 1)]), "bert"),
    ]

    def report(name, dec, tokens, call):
        call()
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        st = dec.last_stats
        dev = sum(ms for _, ms in st["stages"])
        print(json.dumps({"decoder": name, "tokens_of": tokens, "corpus": args.corpus, "docs": args.docs, "tokens": st["tokens"],
                          "bytes_in": st["bytes_in"], "bytes_out": st["bytes_out"], "passes": st["passes"],
                          "ms_stages": [[n, round(ms, 3)] for n, ms in st["stages"]], "ms_device": round(dev, 3),
                          "mb_per_s": round(st["bytes_in"] / 1e6 / (dev / 1e3), 1) if dev else None,
                          "ms_wall_host_call": round(wall, 3)}), flush=True)

    for name, dec, tokens in progs:
        w = words[tokens]
        report(name, dec, tokens, lambda: dec.decode_packed(*w))
    if args.ids:
        body, wo, tw = words["bert"]
        raw, o = body.tobytes(), wo.tolist()
        vocab, ids = {}, np.empty(len(o) - 1, dtype=np.uint32)
        for j in range(len(o) - 1):
            ids[j] = vocab.setdefault(raw[o[j]:o[j + 1]], len(vocab))
        dec = D.wordpiece("##", False)
        dec.set_vocab([k.decode("utf-8") for k in vocab])
        report("wordpiece('##', False), ids", dec, "bert", lambda: dec.decode_ids_packed(ids, tw))


if __name__ == "__main__":
    main()
