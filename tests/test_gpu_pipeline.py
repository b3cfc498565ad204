"""PipelineTokenizer on the GPU: exact equality with tests/pipeline_ref.py everywhere -- the merge tiers
and their thresholds, the initial symbols, the rank / new-id quirks and the panic, the added-token loop
inside a word, whole pipelines end to end, tokenize, decode, and the device entry over torch tensors
with poisoned tails (as tests/test_gpu_text_tail.py does for the other entries)."""
import json

import numpy as np
import pytest

from complexity_tokenizer import PanicException, PipelineTokenizer, Tokenizer, UnsupportedConfigError, device_count
from datagen import corpus
from datagen.build_tokenizers import fixture_path
from tests import decoder_ref, normalizer_ref, postproc_ref, pretok_ref
from tests import pipeline_cases as pc
from tests import pipeline_ref as pr

pytestmark = pytest.mark.gpu

G = 8
S32 = 0x5A5A5A5A
S64 = 0x5A5A5A5A5A5A5A5A
TIER_SIZES = (1, 2, 31, 32, 33, 2047, 2048, 2049)


def build(sp):
    """the PipelineTokenizer of a spec, through from_components and the component constructors"""
    return PipelineTokenizer.from_components(
        sp["vocab"], sp["merges"],
        None if sp["normalizer"] is None else normalizer_ref.to_normalizer(sp["normalizer"]),
        None if sp["pre_tokenizer"] is None else pretok_ref.to_pretokenizer(sp["pre_tokenizer"]),
        None if sp["decoder"] is None else decoder_ref.to_decoder(sp["decoder"]),
        None if sp["post_processor"] is None else postproc_ref.to_postprocessor(sp["post_processor"]),
        sp["added_tokens"])


def check(sp, texts, tok=None):
    tok = tok or build(sp)
    ref = pr.PipelineRef(**sp)
    want = [ref.encode(t) for t in texts]
    got = tok.encode_batch(texts)
    bad = [i for i in range(len(texts)) if got[i] != want[i]]
    assert not bad, (len(bad), texts[bad[0]], got[bad[0]], want[bad[0]])
    return tok, ref, want


# ---- tiers -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain_world():
    """the worst case of the loop, "a" * n under (a, a), (aa, aa), ...: the oracle's answers, computed once"""
    sp = pc.spec(*pc.chain(11), pre_tokenizer=("whitespace",))
    ref = pr.PipelineRef(**sp)
    return sp, {n: ref.encode("a" * n) for n in TIER_SIZES}


def test_tiers_worst_case_merges(chain_world):
    sp, want = chain_world
    tok = build(sp)
    texts = ["a" * n for n in TIER_SIZES]
    assert tok.encode_batch(texts) == [want[n] for n in TIER_SIZES]
    assert tok.last_stats["tier2_segments"] == 3 and tok.last_stats["tier3_segments"] == 1 and tok.last_stats["max_segment_symbols"] == 2049
    # every size as words of one text, and b's that never merge between them
    one = " ".join("a" * n + " " + "b" * (n % 40) for n in reversed(TIER_SIZES))
    assert tok.encode(one) == [i for n in reversed(TIER_SIZES) for i in want[n] + [0] * (n % 40)]
    assert sum(want[2049]) == 12 + 1 and len(want[2047]) == 11  # (2048 + 1; 2047 is eleven ones)


def test_tiers_merges_that_never_apply():
    sp = pc.spec({"a": 3, "b": 5, "ab": 9}, [("a", "b")], pre_tokenizer=("whitespace",))
    tok = build(sp)
    texts = ["a" * n for n in TIER_SIZES] + ["b" * n for n in TIER_SIZES]
    assert tok.encode_batch(texts) == [[3] * n for n in TIER_SIZES] + [[5] * n for n in TIER_SIZES]
    # one merge at the very end of a long segment, in each wave tier
    assert tok.encode_batch(["a" * 2047 + "b", "a" * 2100 + "b" + "b" * 40]) == [[3] * 2046 + [9], [3] * 2099 + [9] + [5] * 40]


def test_word_above_the_cap_is_refused(monkeypatch):
    monkeypatch.setenv("CTOK_PIPELINE_MAX_WORD_SYMBOLS", "4096")
    tok = build(pc.spec({"a": 0, "b": 1}, [], pre_tokenizer=("whitespace",)))
    assert PipelineTokenizer.limits(tok._h)["max_word_symbols"] == 4096
    assert tok.encode_batch(["b", "a" * 4096]) == [[1], [0] * 4096]
    with pytest.raises(UnsupportedConfigError, match="a word of 4097 symbols"):
        tok.encode_batch(["b", "a" * 4097 + " b"])
    assert tok.encode("ab") == [0, 1]  # the handle is fine after a refusal
    # dropped chars are no symbols: 4097 chars, 4096 of them kept
    assert tok.encode("a" * 2000 + "?" + "a" * 2096) == [0] * 4096
    monkeypatch.setenv("CTOK_PIPELINE_MAX_WORD_SYMBOLS", str(1 << 40))  # nothing raises the cap
    assert PipelineTokenizer.limits()["max_word_symbols"] < 1 << 20


def test_flagged_word_above_the_work_bound_is_refused():
    """one thread walks a word that holds an added token, and a byte can cost it a compare of every token that
    shares its first byte: the bound on such a word follows from the largest such group"""
    heavy = [pc.added("<" * 254 + chr(0x100 + i), 500 + i) for i in range(127)] + [pc.added("[X]", 100)]
    sp = pc.spec(pc.ABC, [("a", "b")], pre_tokenizer=("whitespace",), added_tokens=heavy)
    tok = build(sp)
    ref = pr.PipelineRef(**sp)
    lim = PipelineTokenizer.limits(tok._h)
    cap = lim["max_flagged_word_bytes"]
    assert cap == (1 << 23) // (127 * 256) and lim["max_batch_bytes"] == (1 << 40) // (127 * 256)  # (the largest group: '<')
    texts = ["ab [X]", "c" * (cap - 3) + "[X]", "b" * (cap + 1) + " a[X]"]  # at the bound; above it without a token
    assert tok.encode_batch(texts) == [ref.encode(t) for t in texts]
    with pytest.raises(UnsupportedConfigError, match="a word of %d bytes holds an added token" % (cap + 1)):
        tok.encode_batch(["ab", "c" * (cap - 2) + "[X]"])
    assert tok.tokenize("c" * (cap - 2) + "[X]") == ref.tokenize("c" * (cap - 2) + "[X]")  # no added-token loop, no bound
    assert tok.encode("ab[X]") == [3, 100]
    # the filter pass can spend a compare of the whole group at every byte of a batch: refused before it runs
    many = ["x" * (1 << 20)] * (lim["max_batch_bytes"] // (1 << 20) + 1)
    with pytest.raises(UnsupportedConfigError, match="batches of more than %d bytes are not supported" % lim["max_batch_bytes"]):
        tok.encode_batch_flat(many)
    assert tok.tokenize_batch(["ab"] + many[:1])[0] == ["ab"] and tok.encode("ab[X]") == [3, 100]
    light = build(pc.CASES["added"][0])  # three short tokens that start with '<': 11 bytes
    big = PipelineTokenizer.limits(light._h)["max_flagged_word_bytes"]
    assert big == (1 << 23) // 11 and PipelineTokenizer.limits()["max_flagged_word_bytes"] == 1 << 20
    word = "x" * (big - 4) + "<s>c"  # (x has no vocab string: no symbols, so the symbol cap is not in the way)
    assert light.encode_batch(["ab", word]) == [[3], [100, 2]]
    with pytest.raises(UnsupportedConfigError, match="a word of %d bytes holds an added token" % (big + 1)):
        light.encode("x" + word)


def test_many_words_and_texts_cross_the_multi_block_scan():
    sp = pc.CASES["added"][0]
    rng = np.random.default_rng(5)
    pool = ["ab", "a", "abc", "<s>ab", "c<s>>", "", "ab ab", "b [X]a", "   "]
    texts = [pool[i] for i in rng.integers(0, len(pool), size=5000)]
    tok, _, want = check(sp, texts)
    assert tok.last_stats["texts"] == 5000 and tok.last_stats["words"] > 4096 and tok.last_stats["segments"] > tok.last_stats["words"]
    ids, off = tok.encode_batch_flat(texts)
    assert off.tolist() == np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist() and ids.tolist() == [i for w in want for i in w]


# ---- the case table: initial symbols, quirks, added tokens ----------------------------------------------

@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_case_table(name):
    sp, texts = pc.CASES[name]
    tok, ref, want = check(sp, texts)
    for t in texts:  # alone: a batch of one
        assert tok.encode(t) == ref.encode(t), t
    assert tok.encode_batch([]) == [] and tok.encode_batch([""]) == [ref.encode("")]
    assert tok.encode_batch(texts[::-1] + texts) == want[::-1] + want
    assert [tok.tokenize(t) for t in texts] == [ref.tokenize(t) for t in texts]


def test_initial_symbols_by_hand():
    tok = build(pc.CASES["chars"][0])
    assert tok.encode("aé中😀b") == [0, 8, 1]          # 1-, 2-, 3- and 4-byte chars: (é, 中) first, then (é中, 😀)
    assert tok.encode("aé") == [7] and tok.encode("中😀") == [6] and tok.encode("😀é中a") == [4, 5, 0]
    assert tok.encode("xyz") == [] and tok.encode("?!") == []  # only unknown chars
    assert tok.encode("é?中") == [5]                    # the unknown char is dropped: its neighbours merge
    assert tok.encode_batch(["", "   ", "é"]) == [[], [], [2]]
    ids, off = tok.encode_batch_flat([])
    assert ids.size == 0 and off.tolist() == [0]
    tok = build(pc.CASES["no_pretok"][0])              # no pre-tokenizer: the whole text is the word
    assert tok.encode("a b") == [0, 10, 1] and tok.encode("") == [] and tok.encode_batch(["", ""]) == [[], []]


def test_quirks_by_hand():
    assert build(pc.CASES["aaa"][0]).encode("aaa") == [6, 0]
    assert build(pc.CASES["duplicate"][0]).encode("abc") == [0, 4]
    assert build(pc.CASES["shift"][0]).encode_batch(["ab", "abab", "cb"]) == [[4], [4, 4], [2, 1]]
    assert build(pc.CASES["shared_id"][0]).encode("ab Ab") == [3, 3]


@pytest.mark.parametrize("name", sorted(pc.PANICS))
def test_out_of_range_rank_panics(name):
    sp, texts, bad, n, rank = pc.PANICS[name]
    tok = build(sp)
    ref = pr.PipelineRef(**sp)
    with pytest.raises(PanicException) as e:
        tok.encode_batch(texts)
    assert str(e.value) == "index out of bounds: the len is %d but the index is %d" % (n, rank)
    with pytest.raises(pr.PanicException) as r:
        ref.encode(texts[bad])
    assert str(r.value) == str(e.value)
    clean = [t for i, t in enumerate(texts) if i != bad]
    assert tok.encode_batch(clean) == [ref.encode(t) for t in clean]  # the handle is fine, and so are the texts around it
    with pytest.raises(PanicException):
        tok.tokenize(texts[bad])


def test_panic_in_the_wave_tiers():
    """the bad pair far inside a long segment, at the first scan and after a merge, in LDS and in global memory"""
    first = build(pc.spec(*pc.SHIFT, pre_tokenizer=("whitespace",)))  # (b, c) is marked: met by the first scan
    late = build(pc.spec(*pc.LATE, pre_tokenizer=("whitespace",)))    # (cb, b) is marked: a a b -> cb b makes it
    for n in (100, 3000):
        with pytest.raises(PanicException, match="the len is 2 but the index is 2"):
            first.encode_batch(["ab", "cb " + "a" * n + "bc" + "a" * n, "bc"])
        with pytest.raises(PanicException, match="the len is 3 but the index is 3"):
            late.encode_batch(["aa", "cb " + "b" * n + "aab" + "b" * n, "aab"])
        assert first.encode("a" * n + "cb" + "a" * n) == [0] * n + [2, 1] + [0] * n
        assert late.encode("b" * n + "aa" + "c" * n) == [1] * n + [4] + [2] * n


def test_added_tokens_by_hand():
    tok = build(pc.CASES["added"][0])
    assert tok.encode_batch(["<s>ab", "ab<s>ab", "ab[X]", "<s>[X]", "a<s>>b"]) == [[100, 3], [3, 100, 3], [3, 102], [100, 102], [0, 101, 1]]
    tok = build(pc.CASES["flags"][0])  # no pre-tokenizer: the white-space checks see real spaces
    assert tok.encode_batch(["a <w> b", "a<w> <w>", "a <l>b", "a<l>b", "a<r> b", "a<r>b"]) == [[0, 100, 1], [0], [0, 101, 1], [3], [0, 102, 1], [3]]
    assert build(pc.spec(pc.ABC, [("a", "b")])).encode("a<s>b") == [3]  # a tokenizer with no added tokens


# ---- pipelines end to end --------------------------------------------------------------------------------

PIPELINES = pc.pipelines()


@pytest.mark.parametrize("name", sorted(PIPELINES))
def test_pipeline_end_to_end(name):
    sp, texts = PIPELINES[name]
    tok, ref, want = check(sp, texts)
    assert [s for s, _ in tok.last_stats["stages"]] == ["normalize", "pre_tokenize", "segments", "symbols", "merges", "emit"]
    assert tok.tokenize_batch(texts[:40]) == [ref.tokenize(t) for t in texts[:40]]
    # ids of special tokens' vocab strings, an added token's id that has no vocab string, an id far outside
    extra = [[sp["vocab"].get("[CLS]", 900), 5, 901, 999999, sp["vocab"].get("<mask>", 902), 7], []]
    for skip in (False, True):
        for clean in (False, True):
            got = tok.decode_batch_with_options(want[:40] + extra, skip, clean)
            assert got == [ref.decode_with_options(w, skip, clean) for w in want[:40] + extra], (skip, clean)
    assert tok.decode(want[-1]) == ref.decode(want[-1]) and tok.decode_batch(want[:3]) == [ref.decode(w) for w in want[:3]]
    if sp["post_processor"] is not None:  # the chaining point
        ids, off = tok.encode_batch_flat(texts[:8])
        out, out_off = tok.post_processor.process_packed(ids, off)
        assert [out[int(out_off[i]):int(out_off[i + 1])].tolist() for i in range(8)] == [ref.process(w) for w in want[:8]]


JSON_PIPELINES = pc.json_pipelines()


@pytest.mark.parametrize("name", sorted(JSON_PIPELINES))
def test_pipeline_loaded_from_tokenizer_json(name):
    """the path from_file / from_str take: parse_tokenizer_json, then every component built from its spec"""
    obj, texts = JSON_PIPELINES[name]
    tok = PipelineTokenizer.from_str(json.dumps(obj))
    ref = pr.PipelineRef.from_json(obj)
    for comp in ("normalizer", "pre_tokenizer", "decoder", "post_processor"):
        assert (getattr(tok, comp) is None) == (getattr(ref, comp) is None), comp
    want = [ref.encode(t) for t in texts]
    assert tok.encode_batch(texts) == want
    assert tok.tokenize_batch(texts[:20]) == [ref.tokenize(t) for t in texts[:20]]
    ids = want[:20] + [[v for k, v in obj["model"]["vocab"].items() if k.startswith(("<", "[", "|"))] + [3, 3, 7]]
    for skip in (False, True):
        for clean in (False, True):
            assert tok.decode_batch_with_options(ids, skip, clean) == [ref.decode_with_options(w, skip, clean) for w in ids], (skip, clean)
    if ref.post_processor is not None:
        assert [tok.post_processor.process(w) for w in want[:6]] == [ref.process(w) for w in want[:6]]
        assert tok.post_processor.process(want[1], want[2]) == ref.process(want[1], want[2])


def test_default_pipeline_on_the_gpt2_fixture(tmp_path):
    """NFC -> ByteLevel from the file: equal to the oracle and to Tokenizer's fused path, an independent device path"""
    path = fixture_path("gpt2_50k", str(tmp_path))
    text, off = corpus.corpus_c1()
    docs = [d.decode() for d in corpus.unpack(text, off)][:120] + ["<|endoftext|>a<|endoftext|>", "", "café 中文 🙂 don't"]
    tok = PipelineTokenizer.from_file(path)
    assert repr(tok.normalizer) == "Normalizer.nfc()" and repr(tok.pre_tokenizer) == "PreTokenizer.byte_level(False)"
    assert repr(tok.decoder) == "Decoder.byte_level()"
    with open(path) as f:
        ref = pr.PipelineRef.from_json(json.load(f))
    assert (tok.post_processor is None) == (ref.post_processor is None)
    want = [ref.encode(d) for d in docs]
    got = tok.encode_batch(docs)
    assert got == want
    fused = Tokenizer.from_file(path)
    fused.device = 0
    assert fused.encode_batch(docs) == got
    assert tok.vocab_size == fused.vocab_size == ref.vocab_size and tok.special_tokens == fused.special_tokens
    assert tok.token_to_id("Ġthe") == fused.token_to_id("Ġthe") and tok.id_to_token(262) == fused.id_to_token(262)
    assert tok.decode_batch(got[:20]) == fused.decode_batch(got[:20]) == [ref.decode(w) for w in want[:20]]
    assert tok.tokenize(docs[0]) == ref.tokenize(docs[0])


def test_from_str_and_unsupported_split():
    sp = pc.spec(pc.ABC, [("a", "b")], added_tokens=[pc.added("<s>", 50, special=True)])
    obj = pc.tokenizer_json(sp, {"normalizer": {"type": "Lowercase"}, "pre_tokenizer": {"type": "Whitespace"}, "decoder": {"type": "Unknown"},
                                 "post_processor": {"type": "TemplateProcessing", "single": [{"SpecialToken": {"id": "<s>"}}, {"Sequence": {"id": "A"}}]}})
    tok = PipelineTokenizer.from_str(json.dumps(obj))
    ref = pr.PipelineRef.from_json(obj)
    assert tok.decoder is None and ref.decoder is None and tok.post_processor is not None
    assert tok.encode("AB <s>c") == ref.encode("AB <s>c") == [3, 50, 2]
    assert tok.decode_with_options([3, 50, 2], False, False) == ref.decode_with_options([3, 50, 2], False, False) == "abc"
    assert tok.post_processor.process(tok.encode("ab")) == ref.process([3]) == [50, 3]
    obj["pre_tokenizer"] = {"type": "Split", "pattern": {"Regex": "a|b"}, "behavior": "Isolated"}
    with pytest.raises(UnsupportedConfigError):
        PipelineTokenizer.from_str(json.dumps(obj))


def test_components_on_two_devices_are_refused():
    if device_count() < 2:
        pytest.skip("one device visible")
    from complexity_tokenizer import Normalizer, PreTokenizer
    with pytest.raises(ValueError, match="one"):
        PipelineTokenizer.from_components(pc.ABC, [], Normalizer.nfc(device=0), PreTokenizer.whitespace(device=1))


# ---- the device entry ------------------------------------------------------------------------------------

def dev():
    import torch
    return torch.device("cuda", 0)


def filled(n, value, dtype):
    import torch
    return torch.full((n,), value, dtype=dtype, device=dev())


def device_call(tok, texts, ids_cap, tail=b"\xF0\x9F<s>ab \xE4\xB8"):
    """encode_packed_device over a text that sits at an odd offset inside poisoned memory, outputs with
    guards -> (n or the exception, ids with guards, tok_off with guards)"""
    import torch
    raw = [t.encode() for t in texts]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    nb = int(off[-1])
    buf = np.frombuffer(tail * 3 + b"".join(raw) + tail * 3, dtype=np.uint8).copy()
    d_text = torch.from_numpy(buf).to(dev())
    d_off = torch.from_numpy(off.view(np.int64)).to(dev())
    d_ids = filled(ids_cap + 2 * G, S32, torch.int32)
    d_toff = filled(len(raw) + 1 + 2 * G, S64, torch.int64)
    try:
        n = tok.encode_packed_device(d_text.data_ptr() + 3 * len(tail), d_off.data_ptr(), len(raw), nb, d_ids[G:].data_ptr(), ids_cap,
                                     d_toff[G:].data_ptr())
    except BufferError as e:
        n = e
    torch.cuda.synchronize()
    return n, d_ids.cpu().numpy().view(np.uint32), d_toff.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("name", ["added", "flags", "nfkc_lower_whitespace", "none_metaspace"])
def test_device_entry_writes_nothing_past_its_outputs(name):
    sp, texts = (pc.CASES.get(name) or PIPELINES[name])
    texts = texts[:40]
    tok = build(sp)
    ref = pr.PipelineRef(**sp)
    want = [ref.encode(t) for t in texts]
    flat = [i for w in want for i in w]
    toff = np.concatenate(([0], np.cumsum([len(w) for w in want]))).tolist()
    n, ids, off = device_call(tok, texts, len(flat))  # ids_cap exactly the number of ids
    assert n == len(flat)
    assert ids[G:G + n].tolist() == flat and (ids[:G] == S32).all() and (ids[G + n:] == S32).all()
    assert off[G:G + len(texts) + 1].tolist() == toff and (off[:G] == S64).all() and (off[G + len(texts) + 1:] == S64).all()
    # a capacity that is too small: the needed size is reported and nothing is written
    e, ids, off = device_call(tok, texts, max(len(flat) - 1, 0))
    assert isinstance(e, BufferError) and e.needed == len(flat)
    assert (ids == S32).all() and (off == S64).all()
    # the same handle with a larger and then a smaller batch: the grow-only buffers are reused
    big = texts * 5
    n2, ids2, off2 = device_call(tok, big, 5 * len(flat) + 3)
    assert n2 == 5 * len(flat) and ids2[G:G + n2].tolist() == flat * 5 and (ids2[G + n2:] == S32).all()
    n3, ids3, off3 = device_call(tok, texts[:3], len(flat))
    k = toff[3]
    assert n3 == k and ids3[G:G + k].tolist() == flat[:k] and (ids3[G + k:] == S32).all()
    assert off3[G:G + 4].tolist() == toff[:4] and (off3[G + 4:] == S64).all()
    n0, ids0, off0 = device_call(tok, [], 0)
    assert n0 == 0 and off0[G] == 0 and (off0[G + 1:] == S64).all() and (ids0 == S32).all()


def test_device_entry_drops_ill_formed_bytes():
    """a byte that is not well-formed UTF-8 is a unit in no vocab string: it gives no id, and what stands
    around it meets"""
    import torch
    tok = build(pc.spec(pc.CHARS, pc.CHAR_MERGES))
    raw = [b"a\xFFb", b"\xC3", b"\xA9a\xC3\xA9", b"\xE4\xB8a\x80b"]  # (text 1 ends with a lead byte, text 2 starts with its continuation)
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    d_text = torch.from_numpy(np.frombuffer(b"".join(raw) + b"\xA9" * 16, dtype=np.uint8).copy()).to(dev())
    d_off = torch.from_numpy(off.view(np.int64)).to(dev())
    d_ids = filled(32, S32, torch.int32)
    d_toff = filled(len(raw) + 1, S64, torch.int64)
    n = tok.encode_packed_device(d_text.data_ptr(), d_off.data_ptr(), len(raw), int(off[-1]), d_ids.data_ptr(), 32, d_toff.data_ptr())
    ids, toff = d_ids.cpu().numpy().view(np.uint32), d_toff.cpu().numpy().view(np.uint64)
    assert toff.tolist() == [0, 1, 1, 2, 3] and n == 3 and ids[:3].tolist() == [9, 7, 9]
    with pytest.raises(ValueError, match="not UTF-8"):
        tok.encode_packed(np.frombuffer(b"a\xFFb", dtype=np.uint8), np.array([0, 3], dtype=np.uint64))
