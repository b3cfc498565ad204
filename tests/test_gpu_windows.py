"""Overflowing stride windows on the GPU (Tokenizer.encode_windows over ctok_encode_windows,
pad.hip k_win_len / k_win_rows) against the Python oracle: per text ref.encode_to_encoding or
encode_from_ids, RefEncoding.truncate_with_stride when longer than max_length (a restatement of
src/encoding.rs:175-223), RefEncoding.pad on the main window, then [enc] + enc.overflowing
flattened.  All four arrays up to row_len, row_len, the sample mapping, the window starts and the
rows' first windows must be identical, and every cell past row_len a padding cell."""
import ctypes
import json
import random

import numpy as np
import pytest

from complexity_tokenizer import PanicException, Tokenizer
from complexity_tokenizer import _native as _n
from oracle import ref_py
from tests import added_cases, encoding_cases, toys

pytestmark = pytest.mark.gpu

ARRAYS = ("input_ids", "attention_mask", "token_type_ids", "special_tokens_mask")


@pytest.fixture(scope="module")
def base(gpt2_path):
    with open(gpt2_path) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def bytes_pair():
    """The byte chars with no merges: "a" * n encodes to exactly n ids."""
    return pair_of(toys.tok_json({c: i for i, c in enumerate(toys.byte_chars())}, []))


def pair_of(obj):
    return Tokenizer.from_str(json.dumps(obj)), ref_py.RefTokenizer(obj)


def oracle_windows(ref, texts, m, s, pairs=None, add_special_tokens=True, padding=None, pad_left=False, pad_id=None):
    """-> (windows as RefEncodings, their rows, their starts, each row's first window + total, pad id)"""
    enc_of = ref.encode_to_encoding if add_special_tokens else ref.encode_from_ids
    encs = [enc_of(t, None if pairs is None else pairs[r]) for r, t in enumerate(texts)]
    for e in encs:
        if len(e.ids) > m:
            e.truncate_with_stride(m, s)
    pid, ptok = ref.pad_id_token()
    if pad_id is not None:
        pid = pad_id
    if padding is not None:
        target = m if padding == "max_length" else max((len(e.ids) for e in encs), default=0)
        for e in encs:
            e.pad(target, pid, ptok, pad_left)
    flat, rows, starts, first = [], [], [], []
    for r, e in enumerate(encs):
        first.append(len(flat))
        flat.append(e)
        rows.append(r)
        starts.append(0)
        pos = m  # the reference's loop: start = pos - stride, pos = the window's end
        for o in e.overflowing:
            flat.append(o)
            rows.append(r)
            starts.append(pos - s)
            pos = pos - s + len(o.ids)
    return flat, rows, starts, first + [len(flat)], pid


def check(got, want, what=""):
    flat, rows, starts, first, pid = want
    assert got["row_window"].tolist() == first, what
    assert got["overflow_to_sample_mapping"].tolist() == rows, what
    assert got["window_start"].tolist() == starts, what
    assert got["row_len"].tolist() == [len(e.ids) for e in flat], what
    width = max((len(e.ids) for e in flat), default=0)
    for k in ARRAYS:
        assert got[k].dtype == np.uint32 and got[k].shape == (len(flat), width), (what, k)
    for w, e in enumerate(flat):
        L = len(e.ids)
        assert got["input_ids"][w, :L].tolist() == e.ids, (what, w)
        assert got["attention_mask"][w, :L].tolist() == e.attention_mask, (what, w)
        assert got["token_type_ids"][w, :L].tolist() == e.type_ids, (what, w)
        assert got["special_tokens_mask"][w, :L].tolist() == e.special_tokens_mask, (what, w)
    past = np.arange(width)[None, :] >= got["row_len"][:, None]
    assert (got["input_ids"][past] == pid).all() and (got["attention_mask"][past] == 0).all(), what
    assert (got["token_type_ids"][past] == 0).all() and (got["special_tokens_mask"][past] == 1).all(), what


GRID = [(m, s) for m in (1, 2, 3, 5, 8) for s in sorted({0, 1, m - 1}) if s < m]


@pytest.mark.parametrize("m,s", GRID)
def test_arithmetic_grid(bytes_pair, m, s):
    tok, ref = bytes_pair
    texts = ["a" * n for n in (0, 1, m - 1, m, m + 1, 2 * m - s, 2 * m - s + 1, 3 * m + 1, 200)]
    want = oracle_windows(ref, texts, m, s)
    assert [len(ref.encode(t)) for t in texts] == [len(t) for t in texts]
    check(tok.encode_windows(texts, max_length=m, stride=s), want, "m %d s %d" % (m, s))


def test_many_rows(bytes_pair):
    """A wave's windows span many rows and the row search crosses every boundary."""
    tok, ref = bytes_pair
    lens = [i % 71 for i in range(300)]
    random.Random(11).shuffle(lens)
    texts = ["a" * n for n in lens]
    got = tok.encode_windows(texts, max_length=7, stride=3, padding="longest")
    check(got, oracle_windows(ref, texts, 7, 3, padding="longest"))
    assert got["input_ids"].shape[0] > 4 * 300


def test_more_windows_than_wavefronts(bytes_pair):
    """k_win_rows launches at most 6144 wavefronts; past that each takes several consecutive windows
    and steps from row to row, over rows of one window and empty rows too."""
    tok, ref = bytes_pair
    rng = random.Random(5)
    texts = ["a" * rng.choice((0, 1, 2, 3, 4, 9, 17, 40)) for _ in range(3000)]
    got = tok.encode_windows(texts, max_length=3, stride=2, padding="longest", pad_left=True)
    assert got["input_ids"].shape[0] > 4 * 6144
    check(got, oracle_windows(ref, texts, 3, 2, padding="longest", pad_left=True))


@pytest.mark.parametrize("kind", ["none", "template", "bert"])
def test_post_processors(base, kind):
    tok, ref = pair_of(encoding_cases.with_post_processor(base, kind))
    ts = encoding_cases.texts()
    if kind == "none":
        check(tok.encode_windows(ts, max_length=7, stride=3), oracle_windows(ref, ts, 7, 3), kind)
        check(tok.encode_windows(ts, max_length=6, stride=0), oracle_windows(ref, ts, 6, 0), kind)
    else:
        # the post-processor does not extend `tokens`: the last window slices past their end
        with pytest.raises(ref_py.PanicException):
            oracle_windows(ref, ts, 7, 3)
        with pytest.raises(PanicException, match="encoding.rs:189"):
            tok.encode_windows(ts, max_length=7, stride=3)
    # no row longer than max_length: one window per row, the arrays of encode_padded bit for bit
    for opts in (dict(padding="longest"), dict(padding="max_length"), dict(padding="longest", pad_left=True), dict()):
        got = tok.encode_windows(ts, max_length=512, stride=128, **opts)
        check(got, oracle_windows(ref, ts, 512, 128, **opts), "%s %s" % (kind, opts))
        pad = tok.encode_padded(ts, truncation=True, max_length=512, **opts)
        assert got["input_ids"].shape[0] == len(ts)
        for k in ARRAYS + ("row_len",):
            assert np.array_equal(got[k], pad[k]), (kind, opts, k)


def test_pairs(base):
    """Type ids across window boundaries that fall inside the second sequence."""
    tok, ref = pair_of(encoding_cases.with_post_processor(base, "none"))
    ts = encoding_cases.texts()
    prs = ts[::-1]
    want = oracle_windows(ref, ts, 9, 4, pairs=prs)
    mixed = [e for e, st in zip(want[0], want[2]) if st and 0 < sum(e.type_ids) < len(e.ids)]
    later = [e for e, st in zip(want[0], want[2]) if st and e.type_ids and min(e.type_ids) == 1]
    assert mixed and later  # overflow windows that straddle the two sequences, and that lie in the second
    check(tok.encode_windows(ts, prs, max_length=9, stride=4), want)
    check(tok.encode_windows(ts, prs, max_length=9, stride=4, padding="max_length", pad_left=True),
          oracle_windows(ref, ts, 9, 4, pairs=prs, padding="max_length", pad_left=True))


def test_no_special_tokens_splits_added_tokens(base):
    """add_special_tokens=False is Tokenizer.encode's flavour: words are split on added tokens that
    match inside a piece.  Encoding::from_ids leaves ids without a vocab string out of `tokens`
    (src/bindings/tokenizer.rs:88-97), so a row holding an added token with an id of its own
    panics in the reference when it overflows; one whose id is the vocab's does not."""
    obj = json.loads(json.dumps(base))
    own = max(obj["model"]["vocab"].values()) + 1
    for content, i in (("ing", own), ("the", obj["model"]["vocab"]["the"])):
        obj["added_tokens"].append({"id": i, "content": content, "single_word": False, "lstrip": False, "rstrip": False,
                                    "normalized": False, "special": False})
    tok, ref = pair_of(obj)
    assert tok.num_piece_added_tokens() == 2
    ts = added_cases.short_docs(40, seed=3) + ["xthe thethe athenb clothed bathes", "sing", "singing in the rain all day long", ""]
    m, s = 6, 2
    ok, bad = [], []
    for t in ts:
        try:
            oracle_windows(ref, [t], m, s, add_special_tokens=False)
            ok.append(t)
        except ref_py.PanicException:
            bad.append(t)
    want = oracle_windows(ref, ok, m, s, add_special_tokens=False)
    vocab_id = obj["model"]["vocab"]["the"]
    plain = ref_py.RefTokenizer(base)
    assert any(e.overflowing and e.ids != plain.encode(t)[:m] for e, t in zip(want[0], ok))  # the split matters there
    assert any(own in e.ids and not e.overflowing for e in want[0])       # a short row with the id of its own
    assert any(vocab_id in o.ids for e in want[0] for o in e.overflowing)  # the split inside an overflowing row
    check(tok.encode_windows(ok, max_length=m, stride=s, add_special_tokens=False), want)
    assert len(bad) >= 3 and all(own in ref.encode(t) for t in bad)
    for texts in ([bad[0]], [bad[-1]], ts):
        with pytest.raises(PanicException, match="encoding.rs:189"):
            tok.encode_windows(texts, max_length=m, stride=s, add_special_tokens=False)


@pytest.mark.parametrize("opts", [dict(padding="longest"), dict(padding="max_length"),
                                  dict(padding="longest", pad_left=True), dict(padding="max_length", pad_left=True),
                                  dict(padding="max_length", pad_id=7), dict(padding="longest", pad_left=True, pad_id=0)])
def test_padding(base, opts):
    """Only the main window of a row is padded; overflowing windows keep their slice length."""
    tok, ref = pair_of(encoding_cases.with_post_processor(base, "none"))
    ts = ["hello world", "", "a", "the " * 40, "numbers 12345 and punctuation!!!", "x y"]
    for texts, m, s in ((ts, 12, 5), (ts[:3] + ts[5:], 12, 5)):  # (the second batch: no row reaches max_length)
        want = oracle_windows(ref, texts, m, s, **opts)
        assert want[4] == opts.get("pad_id", ref.special_tokens["[PAD]"])
        check(tok.encode_windows(texts, max_length=m, stride=s, **opts), want, str(opts))


def test_nfc_active_document(base):
    """A batch with documents NFC changes on an NFC tokenizer: the splice path of the encode."""
    obj = encoding_cases.with_post_processor(base, "none")
    obj["normalizer"] = {"type": "NFC"}
    tok, ref = pair_of(obj)
    ts = ["plain text before", "cafe\u0301 au lait " * 6, "", "nai\u0308ve words", "nothing flagged here",
          "xe\u0301y and A\u030a\u0301b once more"]
    ts += ["filler doc %d with some more words in it" % i for i in range(40)]
    assert any(ref._normalize(t, ref.normalizer) != t for t in ts)
    check(tok.encode_windows(ts, max_length=5, stride=2, padding="longest"),
          oracle_windows(ref, ts, 5, 2, padding="longest"))
    assert tok.last_stats["nfc_docs"] > 0


# ---------------------------------------------------------------------------------- the C ABI

SENTINEL = 0xABCDEF01


def abi_call(tok, texts, m, s, cap, win_cap, masks=True, flags=_n.CTOK_P_ADD_SPECIAL):
    from complexity_tokenizer import pack_texts
    text, off = pack_texts(texts)
    arrs = [np.full(max(cap, 1), SENTINEL, dtype=np.uint32) for _ in range(4)]
    win_len = np.full(max(win_cap, 1), SENTINEL, dtype=np.uint64)
    win_start = np.full(max(win_cap, 1), SENTINEL, dtype=np.uint64)
    win_row = np.full(max(win_cap, 1), SENTINEL, dtype=np.uint32)
    row_win = np.full(len(texts) + 1, SENTINEL, dtype=np.uint64)
    nout, wout = ctypes.c_uint64(), ctypes.c_uint64()
    opts = _n.PadOpts(flags, 0, m)
    rc = _n.lib.ctok_encode_windows(tok._h, text.ctypes.data, off.ctypes.data, len(texts), ctypes.byref(opts), s,
                                    arrs[0].ctypes.data, *[a.ctypes.data if masks else None for a in arrs[1:]], cap,
                                    win_len.ctypes.data, win_row.ctypes.data, win_start.ctypes.data if masks else None,
                                    win_cap, row_win.ctypes.data, ctypes.byref(nout), ctypes.byref(wout), None, None)
    return rc, int(nout.value), int(wout.value), arrs, win_len, win_row, win_start, row_win


def as_result(n, w, arrs, win_len, win_row, win_start, row_win):
    out = {k: a[: n * w].reshape((n, w)) for k, a in zip(ARRAYS, arrs)}
    out.update(row_len=win_len[:n].astype(np.int64), overflow_to_sample_mapping=win_row[:n].astype(np.int64),
               window_start=win_start[:n].astype(np.int64), row_window=row_win.astype(np.int64))
    return out


@pytest.mark.parametrize("short", ["cap", "win_cap"])
def test_abi_capacity(bytes_pair, short):
    tok, ref = bytes_pair
    texts = ["a" * n for n in (0, 3, 9, 20, 4)]
    want = oracle_windows(ref, texts, 4, 1)
    n, w = len(want[0]), 4
    cap, win_cap = (n * w - 1, n) if short == "cap" else (n * w, n - 1)
    rc, nout, wout, arrs, win_len, win_row, win_start, row_win = abi_call(tok, texts, 4, 1, cap, win_cap)
    assert rc == _n.CTOK_E_CAPACITY
    assert (nout, wout) == (n, w) and row_win.tolist() == want[3]
    for a in arrs + [win_len, win_row, win_start]:
        assert (a == SENTINEL).all()  # nothing else written
    rc, nout, wout, *bufs = abi_call(tok, texts, 4, 1, n * w, n)
    assert rc == _n.CTOK_OK and (nout, wout) == (n, w)
    check(as_result(nout, wout, *bufs), want)


def test_abi_null_masks_and_device_buffers(base):
    """Null masks and a null win_start are accepted; the device variant on torch tensors writes
    what the host variant returns."""
    import torch
    from complexity_tokenizer import pack_texts
    tok, ref = pair_of(encoding_cases.with_post_processor(base, "none"))
    ts = encoding_cases.texts()
    want = oracle_windows(ref, ts, 7, 3)
    n, w = len(want[0]), 7
    rc, nout, wout, arrs, win_len, win_row, win_start, row_win = abi_call(tok, ts, 7, 3, n * w, n, masks=False)
    assert rc == _n.CTOK_OK and (nout, wout) == (n, w)
    assert arrs[0][: n * w].reshape(n, w).tolist() == tok.encode_windows(ts, max_length=7, stride=3)["input_ids"].tolist()
    assert all((a == SENTINEL).all() for a in arrs[1:]) and (win_start == SENTINEL).all()
    assert win_row[:n].tolist() == want[1] and row_win.tolist() == want[3]

    host = tok.encode_windows(ts, max_length=7, stride=3, padding="longest")
    dev = torch.device("cuda", 0)
    text, off = pack_texts(ts)
    n_bytes = int(off[-1])
    d_text = torch.from_numpy(np.concatenate([text[:n_bytes], np.zeros(16, np.uint8)])).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_arrs = [torch.empty(n * w, dtype=torch.int32, device=dev) for _ in range(4)]
    d_len, d_start = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
    d_row = torch.empty(n, dtype=torch.int32, device=dev)
    d_row_win = torch.empty(len(ts) + 1, dtype=torch.int64, device=dev)
    kw = dict(max_length=7, stride=3, padding="longest", d_ids=d_arrs[0].data_ptr(), d_attention=d_arrs[1].data_ptr(),
              d_type_ids=d_arrs[2].data_ptr(), d_special=d_arrs[3].data_ptr(), d_win_len=d_len.data_ptr(),
              d_win_row=d_row.data_ptr(), d_win_start=d_start.data_ptr(), d_row_win=d_row_win.data_ptr())
    with pytest.raises(ValueError) as too_small:
        tok.encode_windows_device(d_text.data_ptr(), d_off.data_ptr(), len(ts), n_bytes, cap=n * w, win_cap=n - 1, **kw)
    assert too_small.value.args[1:] == (n, w)
    assert tok.encode_windows_device(d_text.data_ptr(), d_off.data_ptr(), len(ts), n_bytes, cap=n * w, win_cap=n, **kw) == (n, w)
    torch.cuda.synchronize(dev)
    for k, a in zip(ARRAYS, d_arrs):
        assert np.array_equal(a.cpu().numpy().view(np.uint32).reshape(n, w), host[k]), k
    assert d_len.cpu().tolist() == host["row_len"].tolist() and d_row.cpu().tolist() == want[1]
    assert d_start.cpu().tolist() == want[2] and d_row_win.cpu().tolist() == want[3]
