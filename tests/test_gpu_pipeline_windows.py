"""PipelineTokenizer's padded batches and stride windows as GPU arrays: every array, record and error of
encode_padded, encode_windows and encode_windows_device is exactly that of tests/pipeline_windows_ref.py --
the window boundaries, a record per window, the padding, pairs, the panics after a post-processor and
without special tokens, the agreement with `__call__`'s Encodings, the optional outputs, and the device
entry over torch tensors with poisoned surroundings."""
import itertools

import numpy as np
import pytest

import complexity_tokenizer as ct
from complexity_tokenizer import PipelineTokenizer
from tests import decoder_ref, normalizer_ref, postproc_ref, pretok_ref
from tests import pipeline_cases as pc
from tests import pipeline_windows_ref as wr
from tests.pipeline_encoding_ref import PanicException, PipelineEncodingRef

pytestmark = pytest.mark.gpu

G = 8
S32 = 0x5A5A5A5A
S64 = 0x5A5A5A5A5A5A5A5A
ALL = dict(return_offsets=True, return_word_ids=True, return_sequence_ids=True)
PADDED_KEYS = ("input_ids", "attention_mask", "token_type_ids", "special_tokens_mask", "row_len", "offset_mapping", "word_ids",
               "offsets_len", "sequence_ids", "sequence_len")


def build(sp):
    return PipelineTokenizer.from_components(
        sp["vocab"], sp["merges"],
        None if sp["normalizer"] is None else normalizer_ref.to_normalizer(sp["normalizer"]),
        None if sp["pre_tokenizer"] is None else pretok_ref.to_pretokenizer(sp["pre_tokenizer"]),
        None if sp["decoder"] is None else decoder_ref.to_decoder(sp["decoder"]),
        None if sp["post_processor"] is None else postproc_ref.to_postprocessor(sp["post_processor"]),
        sp["added_tokens"])


def world(**kw):
    sp = wr.world_spec(**kw)
    return build(sp), PipelineEncodingRef(**sp)


def call(tok, texts, pairs, mode, **kw):
    if mode == "windows":
        return tok.encode_windows(texts, pairs, **ALL, **kw)
    kw.pop("stride", None)
    return tok.encode_padded(texts, pairs, truncation=mode == "cut", **ALL, **kw)


def compare(tok, ref, texts, pairs=None, mode="windows", **kw):
    """the arrays, or the panic, of the reference; returns what the reference gave"""
    want = wr.windows_ref(ref, texts, pairs, mode=mode, **kw)
    if isinstance(want, PanicException):
        with pytest.raises(ct.PanicException):
            call(tok, texts, pairs, mode, **kw)
        return want
    got = call(tok, texts, pairs, mode, **kw)
    assert set(got) == set(want if mode == "windows" else PADDED_KEYS)
    for k, g in got.items():
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (k, g.shape, want[k].shape, kw)
        assert np.array_equal(g, want[k]), (k, kw, np.argwhere(g != want[k])[:4].tolist())
    return want


# ---- 1. window boundaries ----------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 256, 257])
def test_window_boundaries(m):
    tok, ref = world()
    seen = 0
    for mm, stride, texts in wr.boundary_cases():
        if mm != m:
            continue
        want = compare(tok, ref, texts, max_length=m, stride=stride)
        assert isinstance(want, dict)
        compare(tok, ref, texts, mode="cut", max_length=m)
        seen += 1
    assert seen == (1 if m == 1 else 2 if m == 2 else 3)


# ---- 2. a record per window --------------------------------------------------------------------------------

def test_a_record_per_window():
    tok, ref = world()
    texts = wr.many_windows_texts()
    want = compare(tok, ref, texts, max_length=2, stride=1)
    assert int(np.diff(want["row_window"]).max()) == 4999 and len(texts) > 3000
    assert tok.last_stats["windows"]["windows"] == want["row_window"][-1] and [n for n, _ in tok.last_stats["window_stages"]] == ["plan", "write"]
    compare(tok, ref, texts, max_length=3, stride=0, padding="longest", pad_left=True)


# ---- 3. padding --------------------------------------------------------------------------------------------

TEXTS = ["a b c q r x a b", "", "a", "a b c q", "ab ab x q r", "x r"]


@pytest.mark.parametrize("mode", [None, "cut", "windows"])
def test_padding(mode):
    tok, ref = world()
    for padding, left in itertools.product((None, "longest", "max_length"), (False, True)):
        want = compare(tok, ref, TEXTS, mode=mode, max_length=4, stride=1, padding=padding, pad_left=left)
        over = want["window_start"] > 0
        if mode == "windows":
            # overflowing windows are never padded
            assert over.sum() >= 3 and (want["attention_mask"][over].sum(axis=1) == want["row_len"][over]).all()
        else:
            assert not over.any()
        compare(tok, ref, TEXTS, mode=mode, max_length=4, stride=1, padding=padding, pad_left=left, pad_id=77)


def test_pad_id_by_the_reference_rule():
    for added, pid in ((wr.SPECIAL + [pc.added("[PAD]", 12, special=True)], 12), (wr.SPECIAL, 11), (wr.SPECIAL[:4], 0),
                       (wr.SPECIAL[:4] + [pc.added("<pad>", 13)], 0)):  # (an added token that is not special does not count)
        tok, ref = world(added=added)
        want = compare(tok, ref, ["a b", "a"], mode=None, padding="longest")
        assert want["input_ids"][1, 1] == pid
    tok, ref = world()
    tok.padding_side, tok.model_max_length = "left", 3
    ref.model_max_length = 3
    got = tok.encode_padded(["a b c q", "a"], truncation=True, padding="max_length")  # max_length None, pad_left not given
    assert got["input_ids"].tolist() == [[0, 1, 2], [11, 11, 0]]
    assert np.array_equal(tok.encode_windows(["a b c q", "a"], padding="max_length")["input_ids"],
                          wr.windows_ref(ref, ["a b c q", "a"], mode="windows", padding="max_length", pad_left=True)["input_ids"])


# ---- 4. pairs ----------------------------------------------------------------------------------------------

def test_pairs_border_inside_first_and_last_cell():
    tok, ref = world()
    # m = 4, stride = 1: windows [0, 4), [3, 7), [6, 10), ...; the pair begins at position n_a
    texts = [wr.row(n_a) for n_a in (3, 5, 6, 7, 0, 4)]
    pairs = [wr.row(5, 2)] * 4 + [wr.row(9), ""]
    want = compare(tok, ref, texts, pairs, max_length=4, stride=1, padding="max_length")
    rw = want["row_window"]
    assert want["token_type_ids"][rw[0] + 1].tolist() == [1, 1, 1, 1] and want["token_type_ids"][rw[1] + 1].tolist() == [0, 0, 1, 1]
    assert want["token_type_ids"][rw[2] + 1].tolist() == [0, 0, 0, 1] and want["sequence_ids"][rw[3] + 1].tolist() == [0, 0, 0, 0]
    for left in (False, True):
        compare(tok, ref, texts, pairs, mode="cut", max_length=6, padding="longest", pad_left=left)
        compare(tok, ref, texts, pairs, mode=None, padding="longest", pad_left=left)


# ---- 5. a post-processor -----------------------------------------------------------------------------------

LONG = ("template", "[CLS] [CLS] $A [SEP] [SEP]", None, [("[CLS]", 7), ("[SEP]", 8)])


@pytest.mark.parametrize("pp", [wr.BERT, wr.ROBERTA, wr.NOTHING], ids=["bert", "roberta", "nothing"])
def test_post_processor(pp):
    tok, ref = world(post_processor=pp)
    texts = ["a b c", "", "x"]  # n = 3, 0, 1
    adds = pp is not wr.NOTHING
    for m in range(1, 8):
        for kw in (dict(), dict(padding="max_length", pad_left=True)):
            want = compare(tok, ref, texts, mode="cut", max_length=m, **kw)
            # cut: P > m > n, which for n + 2 ids is m = n + 1 alone (n = 3: m = 4; n = 0: m = 1; n = 1: m = 2)
            assert isinstance(want, PanicException) == (adds and m in (1, 2, 4)), m
            want = compare(tok, ref, texts, max_length=m, stride=m // 2, **kw)
            # windows: every overflowing row once the post-processor added an id
            assert isinstance(want, PanicException) == (adds and m < 5), m
    assert isinstance(compare(tok, ref, texts, texts[::-1], max_length=8, stride=3, padding="longest"), dict)
    assert isinstance(compare(tok, ref, texts, mode=None, max_length=1, padding="max_length"), dict)  # no truncation, no panic


def test_panic_of_the_lowest_row_and_its_message():
    tok, ref = world(post_processor=LONG)
    a, b = "a b c", "a b c q r"  # n = 3 and 5, P = 7 and 9: cut at 6 panics on both
    for texts in (["", a, b], ["", b, a, a]):
        assert isinstance(compare(tok, ref, texts, mode="cut", max_length=6), PanicException)
        with pytest.raises(ct.PanicException) as old:
            tok(texts, truncation=True, max_length=6)
        with pytest.raises(ct.PanicException) as new:
            tok.encode_padded(texts, truncation=True, max_length=6)
        n = 3 if texts[1] == a else 5
        assert str(new.value) == str(old.value) == "range end index %d out of range for slice of length %d (tokens)" % (n, n)
        assert isinstance(compare(tok, ref, texts, max_length=4, stride=1), PanicException)
        with pytest.raises(ct.PanicException) as old:
            tok(texts, truncation=True, max_length=4, stride=1)
        with pytest.raises(ct.PanicException) as new:
            tok.encode_windows(texts, max_length=4, stride=1)
        assert str(new.value) == str(old.value) and str(new.value).endswith("for slice of length %d (tokens)" % n)
    # stride 0 windows: the old route is encode_with_truncation
    with pytest.raises(ct.PanicException) as old:
        tok.encode_with_truncation(b, None, 4, 0)
    with pytest.raises(ct.PanicException) as new:
        tok.encode_windows(["", b], max_length=4)
    assert str(new.value) == str(old.value) == "range end index 8 out of range for slice of length 5 (tokens)"
    compare(tok, ref, ["x", "a"], max_length=8)  # the handle is fine after the panics
    # an error of the encode comes first: the subtraction panic of a template that drops the ids
    tok, ref = world(post_processor=("template", "[CLS]", None, [("[CLS]", 7)]))
    with pytest.raises(ct.PanicException, match="attempt to subtract with overflow"):
        tok.encode_windows(["a", "a b"], max_length=1)


# ---- 6. without special tokens -----------------------------------------------------------------------------

def test_without_special_tokens():
    tok, ref = world(added=wr.SPECIAL + [pc.added("<n>", 50)], post_processor=wr.BERT)
    assert tok.encode("a <n> b") == [0, 50, 1]
    kw = dict(add_special_tokens=False)
    clean = ["a b c q r", "", "x", "ab ab a"]
    for pairs in (None, ["x r", "a b c", "", "q"]):
        want = compare(tok, ref, clean, pairs, max_length=2, stride=1, padding="longest", **kw)  # vocab-only rows: no panic
        assert isinstance(want, dict) and want["offsets_len"].sum() == 0 and (want["word_ids"] == wr.NONE).all()
        compare(tok, ref, clean, pairs, mode="cut", max_length=3, padding="max_length", pad_left=True, **kw)
        compare(tok, ref, clean, pairs, mode=None, padding="longest", **kw)
    # t tokens for P ids: cut panics at P > m > t alone
    row = "<n> a <n> b <n>"  # P = 5, t = 2
    assert tok.encode(row) == [50, 0, 50, 1, 50]
    for m in range(1, 7):
        want = compare(tok, ref, ["a", row, "a <n>"], mode="cut", max_length=m, **kw)
        assert isinstance(want, PanicException) == (m in (3, 4)), m  # ("a <n>": P = 2, t = 1, no m between them)
    for m in range(1, 7):
        want = compare(tok, ref, ["a", "a b c", row], max_length=m, stride=0, **kw)
        assert isinstance(want, PanicException) == (m < 5), m
    with pytest.raises(ct.PanicException) as old:
        tok(["a", row, "<n> <n> <n> <n>"], truncation=True, max_length=3, stride=1, **kw)
    with pytest.raises(ct.PanicException) as new:
        tok.encode_windows(["a", row, "<n> <n> <n> <n>"], max_length=3, stride=1, **kw)
    assert str(new.value) == str(old.value)
    with pytest.raises(ct.PanicException) as old:
        tok(["a", row], ["a", "<n>"], truncation=True, max_length=4, **kw)
    with pytest.raises(ct.PanicException) as new:
        tok.encode_padded(["a", row], ["a", "<n>"], truncation=True, max_length=4, **kw)
    assert str(new.value) == str(old.value) == "range end index 2 out of range for slice of length 2 (tokens)"


# ---- 7. agreement with the old route -----------------------------------------------------------------------

def flat(encs):
    return [w for e in encs for w in [e] + e.overflowing]


@pytest.mark.parametrize("use_pairs", [False, True], ids=["single", "pairs"])
def test_agreement_with_call(use_pairs):
    vocab, merges = pc.random_vocab(11)
    sp = pc.spec(vocab, merges, None, ("whitespace",), None, None, [pc.added("<pad>", 900, special=True)])
    tok = build(sp)
    texts = pc.random_texts(41, 120, vocab)
    pairs = pc.random_texts(42, 120, vocab, max_words=5) if use_pairs else None
    for m, s, padding in ((6, 2, None), (5, 0, "longest"), (7, 6, "max_length"), (16, 3, "longest")):
        encs = tok(texts, pairs, truncation=True, max_length=m, stride=s, padding=padding).encodings()
        wins = flat(encs) if s else encs  # (stride 0 is Encoding::truncate: its one remainder encoding is not returned)
        got = tok.encode_windows(texts, pairs, max_length=m, stride=s, padding=padding, **ALL) if s else \
            tok.encode_padded(texts, pairs, truncation=True, max_length=m, padding=padding, **ALL)
        assert len(wins) == len(got["input_ids"]) and (s == 0 or len(wins) > len(texts))
        assert got["row_len"].tolist() == [len(w.ids) for w in wins]
        assert got["offsets_len"].tolist() == [len(w.offsets) for w in wins] and got["sequence_len"].tolist() == [len(w.sequence_ids) for w in wins]
        for i, w in enumerate(wins):
            n, no, ns = len(w.ids), len(w.offsets), len(w.sequence_ids)
            assert got["input_ids"][i, :n].tolist() == w.ids and got["attention_mask"][i, :n].tolist() == w.attention_mask
            assert got["token_type_ids"][i, :n].tolist() == w.type_ids and got["special_tokens_mask"][i, :n].tolist() == w.special_tokens_mask
            assert [tuple(x) for x in got["offset_mapping"][i, :no].tolist()] == w.offsets and got["word_ids"][i, :no].tolist() == w.word_ids
            assert got["sequence_ids"][i, :ns].tolist() == [wr.NONE if x is None else x for x in w.sequence_ids]
            assert not got["attention_mask"][i, n:].any() and (got["word_ids"][i, no:] == wr.NONE).all()


# ---- 8. optional outputs -----------------------------------------------------------------------------------

def test_optional_outputs():
    tok, ref = world()
    kw = dict(max_length=4, stride=1, padding="max_length", pad_left=True)
    full = tok.encode_windows(TEXTS, TEXTS[::-1], **ALL, **kw)
    for off, word, seq in itertools.product((False, True), repeat=3):
        got = tok.encode_windows(TEXTS, TEXTS[::-1], return_offsets=off, return_word_ids=word, return_sequence_ids=seq, **kw)
        assert ("offset_mapping" in got) == off and ("word_ids" in got) == word and ("sequence_ids" in got) == seq
        assert ("offsets_len" in got) == (off or word) and ("sequence_len" in got) == seq
        for k, g in got.items():
            assert np.array_equal(g, full[k]), (k, off, word, seq)
        written = tok.last_stats["windows"]["bytes_written"]
        assert written == full["input_ids"].size * (16 + 16 * off + 4 * word + 4 * seq)


# ---- 9. the device entry -----------------------------------------------------------------------------------

def dev():
    import torch
    return torch.device("cuda", 0)


def filled(n, value, dtype):
    import torch
    return torch.full((n,), value, dtype=dtype, device=dev())


CELLS32 = ("ids", "attention", "type_ids", "special", "word_ids", "sequence_ids")
RECS64 = ("win_len", "win_start", "win_off_len", "win_seq_len")


def device_call(tok, seqs, rows, cap, win_cap, tail, stream=None, skip=(), **kw):
    """encode_windows_device over sequences at an odd offset inside poisoned memory, outputs between guards"""
    import torch
    raw = [t.encode() for t in seqs]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    buf = np.frombuffer(tail * 3 + b"".join(raw) + tail * 3, dtype=np.uint8).copy()
    d_text = torch.from_numpy(buf).to(dev())
    d_off = torch.from_numpy(off.view(np.int64)).to(dev())
    o = {k: filled(cap + 2 * G, S32, torch.int32) for k in CELLS32}
    o["offsets"] = filled(2 * cap + 2 * G, S64, torch.int64)
    o.update({k: filled(win_cap + 2 * G, S64, torch.int64) for k in RECS64})
    o["win_row"] = filled(win_cap + 2 * G, S32, torch.int32)
    o["row_win"] = filled(rows + 1 + 2 * G, S64, torch.int64)
    p = {k: (0 if k in skip else v[G:].data_ptr()) for k, v in o.items()}
    torch.cuda.synchronize()
    try:
        n = tok.encode_windows_device(d_text.data_ptr() + 3 * len(tail), d_off.data_ptr(), rows, int(off[-1]), d_ids=p["ids"], cap=cap,
                                      d_win_len=p["win_len"], d_win_row=p["win_row"], win_cap=win_cap, d_row_win=p["row_win"],
                                      d_attention=p["attention"], d_type_ids=p["type_ids"], d_special=p["special"], d_offsets=p["offsets"],
                                      d_word_ids=p["word_ids"], d_sequence_ids=p["sequence_ids"], d_win_start=p["win_start"],
                                      d_win_off_len=p["win_off_len"], d_win_seq_len=p["win_seq_len"],
                                      stream=stream.cuda_stream if stream is not None else 0, **kw)
    except BufferError as e:
        n = e
    torch.cuda.synchronize()
    return n, {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint64) for k, v in o.items()}


NAMES = {"ids": "input_ids", "attention": "attention_mask", "type_ids": "token_type_ids", "special": "special_tokens_mask",
         "word_ids": "word_ids", "sequence_ids": "sequence_ids", "win_len": "row_len", "win_start": "window_start",
         "win_off_len": "offsets_len", "win_seq_len": "sequence_len", "win_row": "overflow_to_sample_mapping"}


def untouched(v):
    return (v == (S32 if v.dtype == np.uint32 else S64)).all()


def test_device_entry():
    import torch
    tok, ref = world(normalizer=("lowercase",))
    texts = ["ABC ab q r x a b", "Ab ab q", "", "a b x", "AB" + " " * 61 + "ab"]  # (the first: "abc" completes only in the tail)
    pairs = ["x", "", "ab AB a a a", "r", "abc"]
    tail = b"c ab\xC3"
    side = torch.cuda.Stream(device=dev())
    for use_pairs, stream in ((False, None), (True, side)):
        seqs = [x for ab in zip(texts, pairs) for x in ab] if use_pairs else texts
        kw = dict(max_length=3, stride=1, padding="max_length", pad_left=use_pairs, pairs=use_pairs)
        want = wr.windows_ref(ref, texts, pairs if use_pairs else None, mode="windows", max_length=3, stride=1, padding="max_length",
                              pad_left=use_pairs)
        n, w = want["input_ids"].shape
        R = len(texts)
        assert n > R and w == 3
        got, o = device_call(tok, seqs, R, n * w, n, tail, stream, **kw)  # both capacities exact, guards on both sides
        assert got == (n, w)
        for key, name in NAMES.items():
            cnt = n * w if key in CELLS32 else n
            assert o[key][G:G + cnt].tolist() == want[name].reshape(-1).tolist(), key
            assert untouched(o[key][:G]) and untouched(o[key][G + cnt:]), key
        assert o["offsets"][G:G + 2 * n * w].tolist() == want["offset_mapping"].reshape(-1).tolist()
        assert untouched(o["offsets"][:G]) and untouched(o["offsets"][G + 2 * n * w:])
        assert o["row_win"][G:G + R + 1].tolist() == want["row_window"].tolist() and untouched(o["row_win"][G + R + 1:]) and untouched(o["row_win"][:G])
        # outputs that are not wanted: the others are the same
        skip = ("attention", "type_ids", "special", "offsets", "word_ids", "sequence_ids", "win_start", "win_off_len", "win_seq_len")
        got, o = device_call(tok, seqs, R, n * w, n, tail, stream, skip=skip, **kw)
        assert got == (n, w) and o["ids"][G:G + n * w].tolist() == want["input_ids"].reshape(-1).tolist()
        assert o["win_len"][G:G + n].tolist() == want["row_len"].tolist() and all(untouched(o[k]) for k in skip)
        # one short, for each capacity: the needed counts come back, row_win is filled and nothing else is written
        for cap, win_cap in ((n * w - 1, n), (n * w, n - 1)):
            e, o = device_call(tok, seqs, R, cap, win_cap, tail, stream, **kw)
            assert isinstance(e, BufferError) and e.needed == (n, w)
            assert o["row_win"][G:G + R + 1].tolist() == want["row_window"].tolist() and untouched(o["row_win"][G + R + 1:])
            assert all(untouched(v) for k, v in o.items() if k != "row_win")
    # mode cut through the device entry; no rows
    want = wr.windows_ref(ref, texts, mode="cut", max_length=3, padding="longest")
    got, o = device_call(tok, texts, len(texts), 15, 5, tail, windows=False, max_length=3, padding="longest")
    assert got == (5, 3) and o["ids"][G:G + 15].tolist() == want["input_ids"].reshape(-1).tolist() and untouched(o["ids"][G + 15:])
    got, o = device_call(tok, [], 0, 0, 0, tail, max_length=3)
    assert got == (0, 0) and o["row_win"][G] == 0 and untouched(o["row_win"][G + 1:]) and untouched(o["ids"])
    # a panic through the device entry; a misaligned pointer is refused before anything runs
    tokb, _ = world(post_processor=wr.BERT)
    with pytest.raises(ct.PanicException, match=r"^range end index 4 out of range for slice of length 2 \(tokens\)"):
        device_call(tokb, ["a", "a b"], 2, 64, 8, tail, max_length=3, stride=1)
    for bad in (dict(d_ids=2), dict(d_win_row=6), dict(d_win_len=4), dict(d_row_win=12), dict(d_offsets=4), dict(d_sequence_ids=1)):
        args = dict(d_ids=4, cap=1, d_win_len=8, d_win_row=4, win_cap=1, d_row_win=8, max_length=3)
        args.update(bad)
        with pytest.raises(ValueError, match="aligned"):
            tok.encode_windows_device(8, 8, 1, 0, **args)


# ---- 10. arguments -----------------------------------------------------------------------------------------

def test_arguments():
    tok, _ = world()
    for kw in (dict(max_length=4, stride=4), dict(max_length=4, stride=9), dict(max_length=0), dict(max_length=3, stride=-1)):
        with pytest.raises(ValueError, match="stride must be smaller than max_length"):
            tok.encode_windows(["a"], **kw)
        with pytest.raises(ValueError, match="stride must be smaller than max_length"):
            tok.encode_windows_device(0, 0, 0, 0, d_ids=0, cap=0, d_win_len=0, d_win_row=0, win_cap=0, d_row_win=0, **kw)
    for f in (tok.encode_windows, tok.encode_padded):
        with pytest.raises(ValueError, match="padding must be"):
            f(["a"], padding="left")
    with pytest.raises(ValueError, match="padding must be"):
        tok.encode_windows_device(0, 0, 0, 0, d_ids=0, cap=0, d_win_len=0, d_win_row=0, win_cap=0, d_row_win=0, max_length=4, padding="x")
    with pytest.raises(ValueError, match="one entry per text"):
        tok.encode_padded(["a"], ["a", "b"])
    with pytest.raises(TypeError):
        tok.encode_windows("a", max_length=4)
