"""PipelineTokenizer's Encodings on the GPU: exact equality of every field, every panic and every refusal
with tests/pipeline_encoding_ref.py -- the search windows of k_pe_word_find, the needle trim, the order
of the searches and the fallbacks, the token spans, the processed rows, the order of the errors, the work
bound, the Python surface, and the device entry over torch tensors with poisoned tails."""
import numpy as np
import pytest

import complexity_tokenizer as ct
from complexity_tokenizer import PipelineTokenizer, UnsupportedConfigError
from oracle.ref_py import bytes_to_unicode
from tests import decoder_ref, normalizer_ref, postproc_ref, pretok_ref
from tests import pipeline_cases as pc
from tests.pipeline_encoding_ref import PanicException, PipelineEncodingRef, enc_dict, find_work

pytestmark = pytest.mark.gpu

G = 8
S32 = 0x5A5A5A5A
S64 = 0x5A5A5A5A5A5A5A5A

ABQ = {"a": 0, "b": 1, "c": 2, "q": 3, "r": 4, "x": 5, "ab": 6, "[CLS]": 7, "[SEP]": 8, "<s>": 9, "</s>": 10}
SPECIAL = [pc.added("[CLS]", 7, special=True), pc.added("[SEP]", 8, special=True), pc.added("<s>", 9, special=True),
           pc.added("</s>", 10, special=True), pc.added("<pad>", 11, special=True)]
BERT = ("bert", ("[CLS]", 7), ("[SEP]", 8))
ROBERTA = ("roberta", ("<s>", 9), ("</s>", 10), False)


def build(sp):
    return PipelineTokenizer.from_components(
        sp["vocab"], sp["merges"],
        None if sp["normalizer"] is None else normalizer_ref.to_normalizer(sp["normalizer"]),
        None if sp["pre_tokenizer"] is None else pretok_ref.to_pretokenizer(sp["pre_tokenizer"]),
        None if sp["decoder"] is None else decoder_ref.to_decoder(sp["decoder"]),
        None if sp["post_processor"] is None else postproc_ref.to_postprocessor(sp["post_processor"]),
        sp["added_tokens"])


def world(vocab=ABQ, merges=(("a", "b"),), normalizer=None, pre_tokenizer=("whitespace",), post_processor=None, added=SPECIAL):
    sp = pc.spec(vocab, list(merges), normalizer, pre_tokenizer, None, post_processor, added)
    return build(sp), PipelineEncodingRef(**sp)


def want_rows(ref, texts, pairs=None):
    """the oracle's rows, or the panic of the lowest row"""
    out = []
    for i, t in enumerate(texts):
        try:
            out.append(ref.encode_to_encoding(t, pairs[i] if pairs is not None else None).as_dict())
        except PanicException as e:
            return e
    return out


def compare(tok, ref, texts, pairs=None):
    want = want_rows(ref, texts, pairs)
    if isinstance(want, PanicException):
        with pytest.raises(ct.PanicException) as got:
            tok.encode_encodings_flat(texts, pairs)
        assert str(got.value) == str(want)
        return want
    got = tok.encode_batch_pairs_to_encoding(list(zip(texts, pairs))) if pairs is not None else tok.encode_batch_to_encoding(texts)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert enc_dict(g) == w, (i, texts[i], enc_dict(g), w)
    return want


# ---- the search ------------------------------------------------------------------------------------------

def test_search_windows():
    """lowercase makes a word differ from where it came from, so a search runs past it: hits at the window
    edges, needles around a window's size, and needles that end at, or would end past, the text's end"""
    tok, ref = world(normalizer=("lowercase",))
    texts = []
    for at in (0, 63, 64, 65, 127):
        for m in (1, 63, 64, 65, 200):
            needle = "q" * (m - 1) + "r"
            texts.append(" " * at + needle)                      # a hit at `at` that ends exactly at the text's end
            texts.append("Q" * at + needle + " x")               # the same after bytes that are no white space
            texts.append(needle.upper() + " " * at + needle)     # the word is searched for twice
    # the completion lies in the next text of the batch: "abc" must not be found at the "ab" that ends the text
    for k in (0, 59, 60, 61, 124):
        texts += ["ABC" + " " * k + " ab", "c ab"]
    texts += ["AB ab ab", "  ab  ab", "AB" + " a" * 40 + " ab", "ABx" + "a" * 70 + " abx"]  # two in a window; a partial match first
    want = compare(tok, ref, texts)
    assert want[0]["offsets"] == [(0, 1)] and want[15]["offsets"][0] == (63, 64) and want[-4]["offsets"][:2] == [(3, 5), (6, 8)]
    k = texts.index("ABC ab")
    assert want[k]["offsets"] == [(0, 2), (2, 3), (4, 6)]  # "abc" falls back to (0, 3): tokens ab, c; "ab" is found at 4


def test_trimming():
    vocab = dict(ABQ, **{"Ġ": 20, "▁": 21})
    tok, ref = world(vocab=vocab, pre_tokenizer=("whitespace_split",))
    want = compare(tok, ref, ["Ġ ĠĠa ▁ Ġ▁a a", "ĠĠa", "▁ a▁ ▁▁", "xĠ Ġ ĠĠ ▁Ġ▁ ab"])
    assert want[1]["offsets"] == [(4, 5), (5, 5), (5, 5)]  # the needle "a" at 4: the two Ġ start there and are clipped
    assert want[0]["offsets"][0] == (0, 2)  # a word of only trimmed chars searches itself


def test_order_and_fallback():
    tok, ref = world(normalizer=("lowercase",), post_processor=BERT)
    texts = ["a a a", "Ab ab ab", "", "AB", "a", "", "ab AB ab Ab"]
    want = compare(tok, ref, texts)
    assert want[0]["offsets"] == [(0, 1), (2, 3), (4, 5)] and want[0]["special_tokens_mask"] == [1, 0, 0, 1, 1]  # (the two added ids count at the end)
    assert want[1]["offsets"] == [(3, 5), (6, 8), (8, 8)] and want[1]["word_ids"] == [0, 1, 2]
    assert want[2]["ids"] == [7, 8] and want[2]["offsets"] == []
    # a fallback clipped to the text: the word has more bytes than the text
    tok2, ref2 = world(normalizer=("prepend", "xxxx"))
    assert compare(tok2, ref2, ["AB", "", "b"])[0]["offsets"][-1][1] == 2
    # search_start == len with words still to come: every later word is (len, len)
    tok3, ref3 = world(normalizer=("sequence", [("lowercase",), ("prepend", "b b ")]))
    assert compare(tok3, ref3, ["AB", "ab"])[1]["offsets"] == [(1, 2), (2, 2), (2, 2)]


def test_fallback_inside_a_char():
    tok, ref = world(vocab={"f": 0, "i": 1, "é": 2, "a": 3}, merges=(), normalizer=("nfkd",))
    assert compare(tok, ref, ["ﬁ", "a", "aﬁ"])[0]["offsets"] == [(0, 1), (1, 2)]  # the last word ends inside the ligature: no panic
    e = compare(tok, ref, ["a", "ﬁ a", "ﬁ é"])
    assert str(e) == "byte index 2 is not a char boundary"
    # ByteLevel: the two cases of the contract
    vocab = {c: i for i, c in enumerate(bytes_to_unicode().values())}
    tok, ref = world(vocab=vocab, merges=(), pre_tokenizer=("byte_level", False), added=())
    assert str(compare(tok, ref, ["é b", "é€"])) == "byte index 4 is not a char boundary"
    want = compare(tok, ref, ["é b", "hello world"])
    assert want[1]["offsets"][5] == (6, 8) and want[1]["offsets"][-1] == (11, 11)  # "Ġ" takes two bytes of "world"'s span


def test_empty_words_and_texts():
    tok, ref = world(pre_tokenizer=None)
    want = compare(tok, ref, ["ab", "", "a b", ""])
    assert want[1]["ids"] == [] and want[2]["offsets"] == [(0, 2)]  # (the blank has no id: a and b merge)
    compare(tok, ref, ["", ""], ["", "ab"])


def test_many_words_and_texts():
    tok, ref = world(normalizer=("lowercase",), post_processor=ROBERTA)
    for n in (65, 2049, 5000):
        compare(tok, ref, [" ".join(("ab", "B", "q", "xr")[i % 4] for i in range(n))])
    texts = pc.random_texts(7, 300)
    tok, ref = world(vocab=dict(pc.random_vocab(11)[0]), merges=pc.random_vocab(11)[1], normalizer=("nfkc",), added=())
    assert isinstance(compare(tok, ref, texts), PanicException)  # NFKC changes byte lengths: the lowest such text's panic is the call's
    clean = [t for t in texts if not isinstance(want_rows(ref, [t]), PanicException)]
    assert len(clean) >= 250
    compare(tok, ref, clean)
    assert tok.last_stats["encoding"]["rows"] == len(clean) and [n for n, _ in tok.last_stats["encoding_stages"]] == ["find", "spans", "rows"]


# ---- the spans -------------------------------------------------------------------------------------------

def test_token_longer_than_its_word():
    vocab = {c: i for i, c in enumerate(bytes_to_unicode().values())}
    merges, cur = [], "Ġ"
    for ch in "hello":
        merges.append((cur, ch))
        cur += ch
        vocab.setdefault(cur, 400 + len(cur))
    tok, ref = world(vocab=vocab, merges=merges, pre_tokenizer=("byte_level", False), added=())
    want = compare(tok, ref, ["hello hello", " hello"])
    assert want[0]["ids"][-1] == vocab["Ġhello"] and want[0]["offsets"][-1] == (6, 11)  # 7 bytes of string, the span of "hello"


def test_ids_without_strings_shared_ids_and_empty_words():
    # filtered = [ab, bc]: (a, b) has rank 1 and so bc's id: the id's string "bc" gives the length, not "ab"
    tok, ref = world(vocab=pc.SHIFT[0], merges=pc.SHIFT[1], added=())
    compare(tok, ref, ["ab a b", "abab cb ba"])
    # two strings share id 0: the last one's length ("AAA": 3 bytes) counts, as id_to_token answers
    tok, ref = world(vocab={"a": 0, "AAA": 0, "b": 1, "ab": 2}, merges=(("a", "b"),), added=())
    assert tok.id_to_token(0) == "AAA"
    assert compare(tok, ref, ["aaaaa b", "ab a"])[0]["offsets"][:3] == [(0, 3), (3, 5), (5, 5)]
    # a merge whose new id has no vocab string: filtered [xy, ab] gives (a, b) rank 0 and xy's id 77... as a string of no bytes
    tok, ref = world(vocab={"a": 0, "b": 1, "x": 2, "y": 3, "xy": 4, "ab": 5, "zz": 9}, merges=(("a", "b"), ("x", "y")), added=())
    compare(tok, ref, ["ab xy", "a"])
    # a word that yields no id still takes a word index
    tok, ref = world()
    assert compare(tok, ref, ["a zzz b", "zzz", "zz a"])[0]["word_ids"] == [0, 2]


def test_spans_in_every_merge_tier():
    sp = pc.spec(*pc.chain(11), pre_tokenizer=("whitespace",))
    tok, ref = build(sp), PipelineEncodingRef(**sp)
    compare(tok, ref, ["a" * 33 + " b " + "a" * 2049 + " ab", "a" * 32 + "b" * 33])
    assert tok.last_stats["tier2_segments"] >= 2 and tok.last_stats["tier3_segments"] == 1


# ---- the rows --------------------------------------------------------------------------------------------

TEXTS = ["ab a", "", "q", "a b ab x"]
PAIRS = ["x", "ab", "", "r r"]


@pytest.mark.parametrize("pp", [None, BERT, ROBERTA, ("template", "[CLS] $A [SEP] $A", None, [("[CLS]", 7), ("[SEP]", 8)]),
                                ("template", "$A [SEP] $A <s>", "$A $B", [("[SEP]", 8), ("<s>", 9)])])
def test_rows(pp):
    tok, ref = world(post_processor=pp)
    want = compare(tok, ref, TEXTS)
    wantp = compare(tok, ref, TEXTS, PAIRS)
    assert wantp[0]["type_ids"][:3] == [0, 0, 1] or pp is not None
    if pp is None:
        assert wantp[3]["type_ids"] == [0, 0, 0, 0, 1, 1] and wantp[3]["offsets"][4:] == [(0, 1), (2, 3)] and wantp[3]["word_ids"][4:] == [0, 1]
    if pp == BERT:
        assert want[0]["special_tokens_mask"] == [1, 0, 1, 1] and wantp[0]["type_ids"] == [0, 0, 1, 0, 0]


def test_template_without_the_sequence():
    tok, ref = world(post_processor=("template", "[CLS]", None, [("[CLS]", 7)]))
    assert [w["ids"] for w in compare(tok, ref, ["a", "", "ab"])] == [[7]] * 3  # one id each: no row is shorter
    assert str(compare(tok, ref, ["a", "a b", "b"])) == "attempt to subtract with overflow"
    tok, ref = world(post_processor=("template", "$B", None, []))  # no cells at all
    assert [w["ids"] for w in compare(tok, ref, ["", ""])] == [[], []]
    assert str(compare(tok, ref, ["", "a"])) == "attempt to subtract with overflow"
    assert tok.encode_to_encoding("").ids == []


def test_special_id_from_the_merges():
    """"ab" has the id of a special added token: the merge's id is marked 1"""
    tok, ref = world(added=[pc.added("<ab>", 6, special=True), pc.added("<n>", 0, special=False)], post_processor=BERT)
    want = compare(tok, ref, ["ab a b", "x"], ["ab", "a"])
    assert want[0]["ids"] == [7, 6, 0, 1, 6, 8] and want[0]["special_tokens_mask"] == [0, 1, 0, 0, 1, 1]


# ---- errors ----------------------------------------------------------------------------------------------

def test_error_order():
    # (b, c) has a rank past the filtered list: a merge panic; "ﬁ b" a char-boundary panic
    tok, ref = world(vocab=dict(pc.SHIFT[0], f=10, i=11), merges=pc.SHIFT[1], normalizer=("nfkd",), added=())
    texts = ["a", "bc", "ab", "a", "a"]
    pairs = ["a", "a", "a", "ﬁ b", "a"]
    assert str(compare(tok, ref, texts, pairs)).startswith("index out of bounds")
    texts[1], pairs[1], texts[3], pairs[3] = "ﬁ b", "a", "a", "bc"
    assert str(compare(tok, ref, texts, pairs)) == "byte index 2 is not a char boundary"
    # in one sequence the char boundary comes first; in one row the text before the pair
    assert str(compare(tok, ref, ["a", "bc ﬁ b"])) == "byte index 4 is not a char boundary"
    assert str(compare(tok, ref, ["bc"], ["ﬁ b"])).startswith("index out of bounds")
    assert str(compare(tok, ref, ["ﬁ b"], ["bc"])) == "byte index 2 is not a char boundary"
    compare(tok, ref, ["ab", "a b"], ["c", "ﬁ"])  # the handle is fine after the panics


def test_work_bound(monkeypatch):
    monkeypatch.setenv("CTOK_PIPELINE_MAX_FIND_WORK", "4096")
    tok, ref = world(normalizer=("lowercase",))
    lim = PipelineTokenizer.encoding_limits(tok._h)
    assert lim["max_find_work"] == 4096 and lim["max_find_compares"] == 256
    # lowercase: every "a" of "A A A ..." misses and scans to the text's end; the x's are found
    at, over = "x " + "A " * 29 + "x" * 92, "x " * 3 + "A " * 30 + "x" * 86
    assert find_work(ref.words(at), at) == 4096 and find_work(ref.words(over), over) == 4097
    compare(tok, ref, ["a", at, "b"])
    assert tok.last_stats["encoding"]["max_find_work"] == 4096
    with pytest.raises(UnsupportedConfigError, match=r"sequence 1 \(row 1\).* has work 4097,"):
        tok.encode_batch_to_encoding(["a", over, over + " Q Q"])
    with pytest.raises(UnsupportedConfigError, match=r"sequence 3 \(row 1, the pair\)"):
        tok.encode_batch_pairs_to_encoding([("a", "b"), ("a", over)])
    # partial matches cost compares that the work does not count: a lane that compares more than the limit's bytes stops the call
    heavy = "A" + "a" * 1000 + " " + "a" * 1000 + "A"
    assert find_work(ref.words(heavy), heavy) < 4096
    with pytest.raises(UnsupportedConfigError, match=r"sequence 1 \(row 1\).* partial matches"):
        tok.encode_batch_to_encoding(["a", heavy])
    compare(tok, ref, ["ab AB", at, heavy[:200] + " a"])  # the next call on the same handle
    monkeypatch.setenv("CTOK_PIPELINE_MAX_FIND_WORK", str(1 << 62))  # nothing raises the limit
    assert PipelineTokenizer.encoding_limits()["max_find_work"] < 1 << 40


# ---- the surface -----------------------------------------------------------------------------------------

def dicts(encs):
    return [enc_dict(e) for e in encs]


def ref_dicts(encs):
    return [e.as_dict() for e in encs]


def test_surface():
    tok, ref = world(normalizer=("lowercase",), post_processor=BERT)
    texts, pairs = ["Ab ab q", "", "a b x r q ab ab", "[CLS] ab"], ["x", "ab ab", "", "r"]
    assert enc_dict(tok.encode_to_encoding(texts[0])) == ref.encode_to_encoding(texts[0]).as_dict() == enc_dict(tok.encode_plus(texts[0]))
    assert enc_dict(tok.encode_pair_to_encoding(texts[0], pairs[0])) == ref.encode_to_encoding(texts[0], pairs[0]).as_dict()
    assert dicts(tok.batch_encode_plus(texts)) == ref_dicts(ref.call(texts))
    assert tok.model_max_length == 512 and tok.padding_side == "right" and tok.truncation_side == "right"
    assert tok._pad_id_token() == ref.pad_id_token() == (11, "<pad>")
    for kw in (dict(), dict(add_special_tokens=False), dict(padding="longest"), dict(padding="max_length", max_length=12),
               dict(padding="left"), dict(truncation=True, max_length=7),
               dict(truncation=True, max_length=7, stride=2, padding="max_length", add_special_tokens=False)):
        assert dicts(tok(texts, **kw).encodings()) == ref_dicts(ref.call(texts, **kw)), kw
        assert dicts(tok(texts, pairs, **kw).encodings()) == ref_dicts(ref.call(texts, pairs, **kw)), kw
    # tokens has no entry for the post-processor's ids: slicing it past its end panics
    with pytest.raises(ct.PanicException):
        tok(texts, truncation=True, max_length=8)
    with pytest.raises(PanicException):
        ref.call(texts, truncation=True, max_length=8)
    with pytest.raises(ct.PanicException):
        tok(texts, pairs, truncation=True, max_length=7, stride=2)
    with pytest.raises(PanicException):
        ref.call(texts, pairs, truncation=True, max_length=7, stride=2)
    # windows with a stride need a token per id: no post-processor
    tok0, ref0 = world(normalizer=("lowercase",))
    for kw in (dict(truncation=True, max_length=4, stride=2), dict(truncation=True, max_length=3, stride=1, padding="longest"),
               dict(truncation=True, max_length=4)):
        assert dicts(tok0(texts, **kw).encodings()) == ref_dicts(ref0.call(texts, **kw)), kw
        assert dicts(tok0(texts, pairs, **kw).encodings()) == ref_dicts(ref0.call(texts, pairs, **kw)), kw
    enc = tok0.encode_with_truncation(texts[2], pairs[1], max_length=6, stride=1)
    w = ref0.encode_to_encoding(texts[2], pairs[1])
    w.truncate_with_stride(6, 1)
    assert enc_dict(enc) == w.as_dict() and len(enc.overflowing) == 1
    # padded batches without truncation; Iterator::zip; a str is a batch of one; offsets on request
    assert dicts(tok.encode_batch_with_padding(texts)) == ref_dicts(ref.call(texts, padding="longest"))
    got =tok.encode_batch_pairs_with_padding(list(zip(texts, pairs)), 20, True)
    want = ref.call(texts, pairs)
    for e in want:
        e.pad(20, 11, "<pad>", True)
    assert dicts(got) == ref_dicts(want)
    assert dicts(tok(texts, pairs[:2]).encodings()) == ref_dicts(ref.call(texts[:2], pairs[:2]))
    one = tok(texts[0], pairs[0], padding="max_length", max_length=9, return_offsets_mapping=True, return_special_tokens_mask=True)
    w = ref.call([texts[0]], [pairs[0]], padding="max_length", max_length=9)[0].as_dict()
    assert len(one) == 1 and one.to_dict() == {"input_ids": [w["ids"]], "attention_mask": [w["attention_mask"]], "token_type_ids": [w["type_ids"]],
                                               "special_tokens_mask": [w["special_tokens_mask"]], "offset_mapping": [w["offsets"]]}
    tok.padding_side, tok.model_max_length, tok.truncation_side = "left", 10, "left"
    ref.model_max_length = 10
    want = ref.call(texts, padding="max_length")
    assert [e.ids for e in tok(texts, padding="max_length").encodings()] == [[11] * (10 - len(e.ids)) + e.ids for e in ref.call(texts)]
    assert len(want[0].ids) == 10 and tok.truncation_side == "left"
    with pytest.raises(TypeError):
        tok(3)


@pytest.mark.parametrize("name", ["bert_bert", "nfkc_lower_whitespace"])
def test_tokenizer_json_pipelines(name):
    obj, texts = pc.json_pipelines()[name]
    import json
    tok = PipelineTokenizer.from_str(json.dumps(obj))
    ref = PipelineEncodingRef.from_json(obj)
    texts = texts[:48]
    compare(tok, ref, texts)  # (as it is: a normaliser that changes byte lengths makes some of these texts panic)
    clean = [t for t in texts if not isinstance(want_rows(ref, [t]), PanicException)]
    assert len(clean) >= 24
    compare(tok, ref, clean)
    compare(tok, ref, clean, clean[::-1])
    kw = dict(padding="longest", truncation=True, max_length=9)
    # (a row with fewer than 9 tokens and more than 9 ids panics slicing `tokens`: test_surface has that case)
    ok = [t for t in clean if not (len(ref.encode_single_to_encoding(t, 0).ids) < 9 < len(ref.encode_to_encoding(t).ids))]
    assert dicts(tok(ok, **kw).encodings()) == ref_dicts(ref.call(ok, **kw))


# ---- the device entry ------------------------------------------------------------------------------------

def dev():
    import torch
    return torch.device("cuda", 0)


def filled(n, value, dtype):
    import torch
    return torch.full((n,), value, dtype=dtype, device=dev())


def device_call(tok, seqs, rows, pairs, cells_cap, ids_cap, tail):
    """encode_encodings_device over sequences at an odd offset inside poisoned memory, outputs with guards"""
    import torch
    raw = [t.encode() for t in seqs]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    buf = np.frombuffer(tail * 3 + b"".join(raw) + tail * 3, dtype=np.uint8).copy()
    d_text = torch.from_numpy(buf).to(dev())
    d_off = torch.from_numpy(off.view(np.int64)).to(dev())
    o = {"ids": filled(cells_cap + 2 * G, S32, torch.int32), "type_ids": filled(cells_cap + 2 * G, S32, torch.int32),
         "special": filled(cells_cap + 2 * G, S32, torch.int32), "row_off": filled(rows + 1 + 2 * G, S64, torch.int64),
         "offsets": filled(2 * ids_cap + 2 * G, S64, torch.int64), "word_ids": filled(ids_cap + 2 * G, S32, torch.int32),
         "seq_ids": filled(ids_cap + 2 * G, S32, torch.int32), "seq_off": filled(rows + 1 + 2 * G, S64, torch.int64),
         "n_a": filled(rows + 2 * G, S64, torch.int64)}
    p = {k: v[G:].data_ptr() for k, v in o.items()}
    try:
        n = tok.encode_encodings_device(d_text.data_ptr() + 3 * len(tail), d_off.data_ptr(), rows, int(off[-1]), d_ids=p["ids"],
                                        d_type_ids=p["type_ids"], d_special=p["special"], cells_cap=cells_cap, d_row_off=p["row_off"],
                                        d_offsets=p["offsets"], d_word_ids=p["word_ids"], ids_cap=ids_cap, d_seq_off=p["seq_off"],
                                        d_n_a=p["n_a"], d_seq_ids=p["seq_ids"], pairs=pairs)
    except BufferError as e:
        n = e
    torch.cuda.synchronize()
    return n, {k: v.cpu().numpy().view(np.uint32 if v.dtype == torch.int32 else np.uint64) for k, v in o.items()}


def test_device_entry():
    tok, ref = world(normalizer=("lowercase",), post_processor=BERT)
    texts = ["ABC ab", "Ab ab q", "", "a b x", "AB" + " " * 61 + "ab"]  # (the first: "abc" completes only in the tail)
    pairs = ["x", "", "ab AB", "r", "abc"]
    tail = b"c ab\xC3"
    for use_pairs in (False, True):
        seqs = [x for ab in zip(texts, pairs) for x in ab] if use_pairs else texts
        want = want_rows(ref, texts, pairs if use_pairs else None)
        flat = {k: [x for w in want for x in w[k]] for k in ("ids", "type_ids", "special_tokens_mask", "word_ids")}
        offs = [x for w in want for ab in w["offsets"] for x in ab]
        cells, n = len(flat["ids"]), len(flat["word_ids"])
        row_off = np.concatenate(([0], np.cumsum([len(w["ids"]) for w in want]))).tolist()
        seq_off = np.concatenate(([0], np.cumsum([len(w["word_ids"]) for w in want]))).tolist()
        R = len(texts)
        got, o = device_call(tok, seqs, R, use_pairs, cells, n, tail)  # both capacities exact
        assert got == (cells, n)
        for key, name, cnt in (("ids", "ids", cells), ("type_ids", "type_ids", cells), ("special", "special_tokens_mask", cells),
                               ("word_ids", "word_ids", n)):
            assert o[key][G:G + cnt].tolist() == flat[name] and (o[key][:G] == S32).all() and (o[key][G + cnt:] == S32).all(), key
        assert o["offsets"][G:G + 2 * n].tolist() == offs and (o["offsets"][:G] == S64).all() and (o["offsets"][G + 2 * n:] == S64).all()
        assert o["row_off"][G:G + R + 1].tolist() == row_off and (o["row_off"][G + R + 1:] == S64).all()
        assert o["seq_off"][G:G + R + 1].tolist() == seq_off and (o["seq_off"][G + R + 1:] == S64).all()
        assert o["n_a"][G:G + R].tolist() == [w["sequence_ids"].count(0) for w in want] and (o["n_a"][G + R:] == S64).all()
        assert [tok.id_to_token(i) or "" for i in o["seq_ids"][G:G + n].tolist()] == [t for w in want for t in w["tokens"]]
        # one short, for each capacity: the needed counts come back and nothing is written
        for cc, ic in ((cells - 1, n), (cells, n - 1)):
            e, o = device_call(tok, seqs, R, use_pairs, cc, ic, tail)
            assert isinstance(e, BufferError) and e.needed == (cells, n)
            assert all((v == (S32 if v.dtype == np.uint32 else S64)).all() for v in o.values())
    got, o = device_call(tok, [], 0, False, 0, 0, tail)
    assert got == (0, 0) and o["row_off"][G] == 0 and o["seq_off"][G] == 0 and (o["row_off"][G + 1:] == S64).all() and (o["ids"] == S32).all()
    # a char-boundary panic through the device entry; an unaligned output is refused before anything runs
    tok, ref = world(vocab={"f": 0, "i": 1, "a": 2}, merges=(), normalizer=("nfkd",))
    with pytest.raises(ct.PanicException, match="^byte index 2 is not a char boundary"):
        device_call(tok, ["a", "ﬁ a"], 2, False, 8, 8, tail)
    with pytest.raises(ValueError, match="aligned"):
        tok.encode_encodings_device(8, 8, 1, 0, d_ids=2, d_type_ids=4, d_special=4, cells_cap=1, d_row_off=8, d_offsets=8, d_word_ids=4,
                                    ids_cap=1, d_seq_off=8, d_n_a=8)
