#!/usr/bin/env python3
"""Device-path probe of the stride windows beside the padded encode on one batch (profiling helper
for rocprofv3 --kernel-trace --stats, not product code): long documents (JOIN consecutive C1
documents each) through ctok_encode_padded_device (truncated to MAX_LENGTH: k_pad_len, k_pad_rows)
and ctok_encode_windows_device (k_win_len, the scan, k_win_rows) on HBM-resident buffers.
usage: windows_probe.py [n_docs] [join] [max_length] [stride] [reps]
Prints one JSON line: the batch, the outputs' sizes, each call's best wall time (the calls end in
a device synchronise) and the algorithmic bytes of k_win_rows (4 B per id read + 16 B per cell)."""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "complexity-tokenizer_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from complexity_tokenizer import Tokenizer  # noqa: E402
from complexity_tokenizer import _native as _n  # noqa: E402
from datagen import corpus  # noqa: E402
from datagen.build_tokenizers import fixture_path  # noqa: E402

args = [int(a) for a in sys.argv[1:6]]
n_docs, join, m, stride, reps = args + [2_000_000, 1000, 512, 128, 10][len(args):]
tok = Tokenizer.from_file(fixture_path("gpt2_50k", "/tmp"))
text, off = corpus.corpus_c1(n_docs=n_docs)
off = np.ascontiguousarray(np.append(off[:-1:join], off[-1]))
rows, nb = len(off) - 1, int(off[-1])
dev = torch.device("cuda", 0)
d_text = torch.zeros(nb + 64, dtype=torch.uint8, device=dev)
d_text[:nb] = torch.from_numpy(text[:nb]).to(dev)
d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
flags = _n.CTOK_P_ADD_SPECIAL | _n.CTOK_P_NO_POSTPROCESS  # (no padding: row_len and win_len are the ids read)


def i32(n):
    return torch.empty(max(n, 1), dtype=torch.int32, device=dev)


def i64(n):
    return torch.empty(max(n, 1), dtype=torch.int64, device=dev)


# the padded encode, truncated: [rows, m]
pad_out = [i32(rows * m) for _ in range(4)]
d_row_len = i64(rows)
opts = _n.PadOpts(flags | _n.CTOK_P_TRUNCATE, 0, m)
ex = _n.Exec(0, None, 0)
width = ctypes.c_uint64()


def padded():
    rc = _n.lib.ctok_encode_padded_device(tok._h, d_text.data_ptr(), d_off.data_ptr(), rows, nb, ctypes.byref(opts),
                                          *[a.data_ptr() for a in pad_out], rows * m, d_row_len.data_ptr(),
                                          ctypes.byref(width), ctypes.byref(ex), None)
    assert rc == _n.CTOK_OK, _n.last_error()


# the windows: a first call with no room reports the sizes
d_row_win = i64(rows + 1)
kw = dict(max_length=m, stride=stride, no_postprocess=True, d_row_win=d_row_win.data_ptr())
try:
    tok.encode_windows_device(d_text.data_ptr(), d_off.data_ptr(), rows, nb, d_ids=0, cap=0, d_win_len=0, d_win_row=0,
                              win_cap=0, **kw)
    n_win, w = 0, 0
except ValueError as e:
    n_win, w = e.args[1:]
win_out = [i32(n_win * w) for _ in range(4)]
d_len, d_start, d_row = i64(n_win), i64(n_win), i32(n_win)


def windows():
    return tok.encode_windows_device(d_text.data_ptr(), d_off.data_ptr(), rows, nb, d_ids=win_out[0].data_ptr(),
                                     d_attention=win_out[1].data_ptr(), d_type_ids=win_out[2].data_ptr(),
                                     d_special=win_out[3].data_ptr(), cap=n_win * w, d_win_len=d_len.data_ptr(),
                                     d_win_row=d_row.data_ptr(), d_win_start=d_start.data_ptr(), win_cap=n_win, **kw)


def best(f):
    f()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t)
    return min(ts) * 1e3


ms_pad, ms_win = best(padded), best(windows)
assert windows() == (n_win, w)
torch.cuda.synchronize(dev)
# the main windows are the truncated rows
first = d_row_win[:rows]
assert torch.equal(win_out[0].view(n_win, w)[first].cpu(), pad_out[0][: rows * int(width.value)].view(rows, -1).cpu())
n_ids = int(tok.last_stats["tokens"])
win_ids = int(d_len.sum().item())  # ids the windows read (overlaps read twice)
print(json.dumps({"rows": rows, "bytes": nb, "ids": n_ids, "max_length": m, "stride": stride,
                  "padded_cells": rows * int(width.value), "n_windows": n_win, "width": w, "window_cells": n_win * w,
                  "k_win_rows_algorithmic_bytes": 4 * win_ids + 16 * n_win * w,
                  "k_pad_rows_algorithmic_bytes": 4 * int(d_row_len.sum().item()) + 16 * rows * int(width.value),
                  "ms_call_padded": round(ms_pad, 4), "ms_call_windows": round(ms_win, 4)}))
