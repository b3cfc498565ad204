#!/usr/bin/env python3
"""Per-stage HIP-event times of complexity_tokenizer.PostProcessor on a seeded batch.

The batch is --rows rows of --len ids, every row with a pair of --len ids, under
PostProcessor.bert.  It goes through process_padded (padded to the longest row: four [rows, width]
matrices and row_len) and through process_packed (ragged: ids and offsets), each twice (the first
call grows the handle's device buffers); the second call's ctok_postprocessor_stage_ms values are
printed next to the bytes each pass moves and the time those bytes take at --tb-per-s, one JSON line
per form.  With --mixed the rows' lengths vary from 0 to --len and a third of the rows has no pair.
Needs a HIP device.
Usage: tools/postproc_timing.py [--rows N] [--len L] [--mixed] [--tb-per-s R]
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
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--len", type=int, default=128)
    ap.add_argument("--mixed", action="store_true")
    ap.add_argument("--tb-per-s", type=float, default=6.29, help="the memory rate the bounds are taken at")
    args = ap.parse_args()
    import numpy as np
    from complexity_tokenizer import PostProcessor
    rng = np.random.default_rng(20264)
    n = args.rows
    if args.mixed:
        la = rng.integers(0, args.len + 1, n)
        lb = rng.integers(0, args.len + 1, n)
        has = (rng.integers(0, 3, n) > 0).astype(np.uint8)
    else:
        la = np.full(n, args.len)
        lb = np.full(n, args.len)
        has = np.ones(n, dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum(la)]).astype(np.uint64)
    poff = np.concatenate([[0], np.cumsum(lb)]).astype(np.uint64)
    ids = rng.integers(1000, 30000, int(off[-1]), dtype=np.uint32)
    pids = rng.integers(1000, 30000, int(poff[-1]), dtype=np.uint32)
    pp = PostProcessor.bert("[CLS]", 101, "[SEP]", 102)

    def report(form, call):
        call()
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        st = pp.last_stats
        rows, out = st["rows"], st["ids_out"]
        cells = rows * st["width"] if form == "padded" else out
        # count: off, pair_off (8 B each) and has_pair (1 B) in, the two lengths (8 B) and the row's length (8 B) out;
        # scan: the lengths in and out; write: one id in per copied cell, per cell 4 B out (ragged) or 4 x 4 B (padded),
        # and per row its offsets and lengths in (32 B)
        moved = {"count": rows * (8 + 8 + 1 + 8 + 8), "scan": rows * 16,
                 "write": out * 4 + cells * (16 if form == "padded" else 4) + rows * 32}
        print(json.dumps({"form": form, "rows": rows, "ids_in": st["ids_in"], "pair_ids_in": st["pair_ids_in"], "ids_out": out,
                          "width": st["width"], "ms_stages": [[k, round(ms, 4)] for k, ms in st["stages"]],
                          "bytes_moved": moved, "ms_bound": {k: round(v / (args.tb_per_s * 1e12) * 1e3, 4) for k, v in moved.items()},
                          "gb_per_s": {k: round(moved[k] / 1e9 / (ms / 1e3), 1) if ms else None for k, ms in st["stages"]},
                          "ms_wall_host_call": round(wall, 3)}), flush=True)

    report("padded", lambda: pp.process_padded((ids, off), (pids, poff, has), pad_to="longest"))
    report("ragged", lambda: pp.process_packed(ids, off, pids, poff, has))


if __name__ == "__main__":
    main()
