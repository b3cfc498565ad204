"""GPU parity of complexity_tokenizer.Decoder (csrc/decoder.hip) against the restatement of the
reference's src/decoders.rs (tests/decoder_ref.py).  Exact equality of the texts everywhere; the
batches are those of tests/decoder_cases.py, which tests/test_decoder_cpu.py runs through the CPU
build of the same rules first.  A workgroup's tile is 256 units (csrc/decoder_internal.h kThreads),
and the scan of the workgroups' counts takes another path from 4,096 workgroups on."""
import random

import numpy as np
import pytest

from complexity_tokenizer import CharBpeModel, Decoder, PreTokenizer, UnsupportedConfigError, WordPieceModel
from tests import decoder_cases as dc
from tests import decoder_ref as ref

pytestmark = pytest.mark.gpu

TILE = 256


def check(dec, docs, made=None):
    d = made or ref.to_decoder(dec)
    got = d.decode_batch(docs)
    assert len(got) == len(docs)
    bad = [i for i, t in enumerate(docs) if got[i] != ref.decode(dec, t)]
    assert not bad, (dec, len(bad), docs[bad[0]][:40], got[bad[0]][:120], ref.decode(dec, docs[bad[0]])[:120])
    return d


@pytest.mark.parametrize("i", range(len(dc.EVERY)))
def test_quirks_under_every_decoder(i):
    dec = dc.EVERY[i]
    d = check(dec, dc.QUIRKS)
    for t in dc.QUIRKS:  # decode is the batch of one
        assert d.decode(t) == d.decode_batch([t])[0] == ref.decode(dec, t), (dec, t)


@pytest.mark.parametrize("pool", sorted(dc.POOLS))
def test_seeded_random_token_lists(pool):
    docs = dc.random_token_lists(pool, 20264, 1500, 200)
    for dec in dc.EVERY:
        check(dec, docs)


BOUNDARY_DECODERS = dc.DEFAULTS + [("wordpiece", "##", False), ("replace", "aa", "b"), ("replace", "", "é"), ("replace", "éa", ""),
                                   ("ctc", "a", "##b"), ("strip", "a", 10 ** 9, 1), ("metaspace", "é", True),
                                   ("sequence", [("wordpiece", "##", True), ("bpe", "</w>"), ("byte_level",)])]


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 4095, 4096, 4097])
def test_totals_around_a_tile(n):
    """Batches of n bytes and of n tokens, in one document and in many."""
    docs_sets = [[["a"] * n], [["a" * n]], [["ab"] * (n // 2) + ["a"] * (n % 2)], [["a"]] * n, [["aa", "a"]] * (n // 3) + [["a" * (n % 3)]],
                 [[""] * n], [[]] * n]
    for dec in BOUNDARY_DECODERS:
        for docs in docs_sets:
            check(dec, docs)


STRADDLE_DECODERS = BOUNDARY_DECODERS + [("ctc", "<pad>", "|"), ("replace", "aa", "bcd"), ("replace", "yy", "é"), ("replace", "##", ""),
                                         ("replace", "</w>", "-"), ("strip", "y", 10 ** 9, 0), ("bpe", "a</w>"), ("replace", "▁▁", " ")]


@pytest.mark.parametrize("at", [TILE, 2 * TILE, 4096])
def test_things_that_straddle_a_tile(at):
    """A multi-byte char, a ## prefix, a </w> suffix, a Replace match, the Metaspace replacement, an
    invalid UTF-8 unit, a clean-up pattern and trailing white space, each with bytes on both sides of
    byte `at` of its batch: every document is a batch of its own, so its first byte is byte 0 of the
    first op's input (tests/decoder_cases.py straddling() asserts the positions; the padding is copied
    byte for byte by a first op, so the alignment holds for ByteLevel's lossy pass, the clean-up and
    trim_end too).  The same for tokens: a token and the neighbour it is compared with in two tiles."""
    docs = dc.straddling(at)
    for tok, span in dc.BYTE_LEVEL_SPANS.items():  # the lossy pass sees the mapped unit across `at` as well
        assert any(d[0].endswith(tok) and start < at < start + span for d, start, _ in docs)
    token_docs = dc.straddling_tokens(at)
    for dec in STRADDLE_DECODERS:
        made = ref.to_decoder(dec)
        for doc, _, _ in docs:
            check(dec, [doc], made)
        for doc in token_docs:
            check(dec, [doc], made)


@pytest.mark.parametrize("n", [63, 64, 65, 200])
def test_runs_of_set_bytes(n):
    rng = random.Random(n)
    run = "".join(rng.choice(" .,!?:;'") for _ in range(n))
    docs = [[run], ["x", run, "y"], list(run), [" '" * (n // 2) + " " * (n % 2)], ["' " * (n // 2), "." * (n % 2)], [" ." * (n // 2)]]
    for dec in (("wordpiece", "##", True), ("wordpiece", "", True), ("wordpiece", "'", True)):
        made = check(dec, docs)
        for at in (TILE, 3 * TILE, 4096):  # a run of exactly n set bytes across a tile boundary of the clean-up's input
            for seed in range(3):
                check(dec, [dc.set_run_across(at, n, 100 * n + seed)], made)


def test_many_empty_tokens_and_empty_documents():
    docs = [[], [""] * 10000 + ["a"], [], [], ["a"], [], ["", ""], [], []]
    for dec in dc.EVERY:
        check(dec, docs)
    for dec in dc.DEFAULTS:
        check(dec, [[], []])
        check(dec, [[]])


def test_a_scan_of_more_than_4096_workgroups():
    n = 4096 * TILE + 3
    docs = [["ab" * (n // 2)], ["a"], []]
    for dec in (("fuse",), ("replace", "ba", "é"), ("strip", "a", 1, 1)):
        check(dec, docs)
    check(("wordpiece", "##", False), [["a"] * n, ["##a"], []])


def _pack(docs):
    flat = [t.encode() for d in docs for t in d]
    tok_off = np.zeros(len(flat) + 1, dtype=np.uint64)
    np.cumsum([len(t) for t in flat], out=tok_off[1:])
    doc_tok = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=doc_tok[1:])
    return np.frombuffer(b"".join(flat), dtype=np.uint8), tok_off, doc_tok


def _texts(text, off):
    raw, o = text.tobytes(), off.tolist()
    return [raw[o[i]:o[i + 1]].decode() for i in range(len(o) - 1)]


def test_packed_form_is_the_batch_form():
    docs = dc.QUIRKS + dc.random_token_lists("mixed", 3, 200, 60)
    for dec in (("wordpiece", "##", True), ("byte_level",), ("replace", "", "-"), dc.SEQUENCES[4]):
        d = ref.to_decoder(dec)
        text, off = d.decode_packed(*_pack(docs))
        assert off.dtype == np.uint64 and off[0] == 0 and int(off[-1]) == text.size and off.tolist() == sorted(off.tolist())
        assert _texts(text, off) == d.decode_batch(docs) == [ref.decode(dec, t) for t in docs]


def test_an_output_larger_than_the_first_guess_is_fetched():
    """decode_packed guesses the output's size; a larger one is fetched from the handle, not computed again."""
    docs = [["a" * 500, "a"], [], ["ba"] * 300]
    for dec in (("replace", "a", "é" * 9), ("replace", "", "--"), ("sequence", [("replace", "a", "\u00e9"), ("byte_level",)])):
        d = check(dec, docs)
        assert d.last_stats["bytes_out"] > d.last_stats["bytes_in"] + d.last_stats["tokens"] + 65
        assert d.decode_batch([["b"]]) == [ref.decode(dec, ["b"])]  # (and the handle goes on)


def test_the_empty_batch():
    for dec in (("fuse",), ("byte_level",), ("wordpiece", "##", True), ("replace", "", "-"), ("sequence", [])):
        d = ref.to_decoder(dec)
        assert d.decode_batch([]) == []
        text, off = d.decode_packed(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64))
        assert text.size == 0 and off.tolist() == [0]
        d.set_vocab(["a"])
        assert d.decode_ids_batch([]) == []


def test_ids_form():
    holes = {0: "[UNK]", 1: "un", 3: "##able", 4: "", 7: "é</w>", 8: "##", 12: " ", 13: "."}
    as_list = ["a", "##b", "", "c</w>", "é", "."]
    batch = [[1, 3, 13], [], [2, 1, 5, 3], [99, 4, 1, 4, 3], [7, 7, 8, 0], [2 ** 32 - 1, 6, 9, 10, 11], [12, 13, 1], [1, 1, 2, 1]]
    for dec in dc.DEFAULTS + [("wordpiece", "##", False), ("ctc", "un", " "), dc.SEQUENCES[4]]:
        d = ref.to_decoder(dec)
        with pytest.raises(ValueError):
            d.decode_ids_batch([[1]])
        with pytest.raises(ValueError):
            d.decode_ids_packed(np.zeros(1, dtype=np.uint32), np.array([0, 1], dtype=np.uint64))
        for vocab, table in ((holes, holes), (as_list, dict(enumerate(as_list)))):
            d.set_vocab(vocab)
            want = [ref.decode(dec, [table[i] for i in ids if i in table]) for ids in batch]
            assert d.decode_ids_batch(batch) == want, dec
            flat = np.array([i for ids in batch for i in ids], dtype=np.uint32)
            off = np.cumsum([0] + [len(ids) for ids in batch]).astype(np.uint64)
            assert _texts(*d.decode_ids_packed(flat, off)) == want
        assert d.last_stats["stages"][0][0] == "gather" and d.last_stats["tokens"] == sum(i < 6 for ids in batch for i in ids)
    d = Decoder.fuse()
    d.set_vocab({})
    assert d.decode_ids_batch([[0, 1], []]) == ["", ""]
    with pytest.raises(RuntimeError):  # CTOK_E_CAPACITY
        d.set_vocab({2 ** 27: "a"})
    d.set_vocab({2 ** 20: "a"})
    assert d.decode_ids_batch([[2 ** 20, 2 ** 20 + 1, 2 ** 27, 0]]) == ["a"]
    rng = random.Random(2)
    big = [[rng.randrange(0, 16) for _ in range(rng.randrange(0, 300))] for _ in range(400)]
    d = Decoder.wordpiece()
    d.set_vocab(holes)
    assert d.decode_ids_batch(big) == [ref.decode(("wordpiece", "##", True), [holes[i] for i in ids if i in holes]) for ids in big]


def test_device_pointers_round_trip():
    import torch
    dec = ("sequence", [("wordpiece", "##", True), ("replace", "a", "éé"), ("strip", " ", 1, 1)])
    d = ref.to_decoder(dec)
    docs = dc.QUIRKS + dc.random_token_lists("vocab", 7, 300, 80)
    raw, tok_off, doc_tok = _pack(docs)
    want_text, want_off = d.decode_packed(raw, tok_off, doc_tok)
    nb = int(want_text.size)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_raw = torch.from_numpy(raw.copy()).to(dev)
        d_tok_off = torch.from_numpy(tok_off.view(np.int64)).to(dev)
        d_doc_tok = torch.from_numpy(doc_tok.view(np.int64)).to(dev)
        d_text = torch.full((nb + 32,), 0xAB, dtype=torch.uint8, device=dev)
        d_off = torch.full((len(docs) + 1,), -7, dtype=torch.int64, device=dev)
        stream.synchronize()
        args = (d_raw.data_ptr(), d_tok_off.data_ptr(), d_doc_tok.data_ptr(), len(docs), len(tok_off) - 1, int(tok_off[-1]),
                d_text.data_ptr())
        for cap in (0, nb - 1):  # too small: the needed size comes back and nothing is written
            with pytest.raises(BufferError) as e:
                d.decode_packed_device(*args, cap, d_off.data_ptr(), stream.cuda_stream)
            assert e.value.needed_bytes == nb
            assert bool((d_text == 0xAB).all()) and bool((d_off == -7).all())
        got = d.decode_packed_device(*args, nb, d_off.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    assert got == nb
    text = d_text.cpu().numpy()
    assert text[:nb].tobytes() == want_text.tobytes() and bool((text[nb:] == 0xAB).all())
    assert d_off.cpu().numpy().view(np.uint64).tolist() == want_off.tolist()
    assert _texts(want_text, want_off) == [ref.decode(dec, t) for t in docs]


def test_device_path_takes_ill_formed_bytes():
    """The device entry takes bytes as they are; a document whose tokens are UTF-8 gives what the
    restatement gives whatever its neighbours hold.  Offsets out of order are refused."""
    import torch
    rng = random.Random(11)
    alphabet = [0x61, 0x20, 0x27, 0x2E, 0x23, 0x5F, 0xC3, 0xA9, 0xE2, 0x96, 0x81, 0x80, 0xE3, 0xF0, 0x9F, 0xED, 0xA0, 0xC0, 0xF4, 0xC4, 0xC5, 0x83]
    docs = [[bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 7))) for _ in range(rng.randrange(0, 4))] for _ in range(2000)]
    flat = [t for d in docs for t in d]
    tok_off = np.cumsum([0] + [len(t) for t in flat]).astype(np.uint64)
    doc_tok = np.cumsum([0] + [len(d) for d in docs]).astype(np.uint64)
    nb = int(tok_off[-1])
    dev = torch.device("cuda", 0)
    d_raw = torch.from_numpy(np.frombuffer(b"".join(flat), dtype=np.uint8).copy()).to(dev)
    d_tok_off = torch.from_numpy(tok_off.view(np.int64)).to(dev)
    d_doc_tok = torch.from_numpy(doc_tok.view(np.int64)).to(dev)
    for dec in dc.DEFAULTS + [("replace", "", "-"), ("strip", "é", 2, 2), ("metaspace", "é", True), dc.SEQUENCES[5]]:
        d = ref.to_decoder(dec)
        cap = 8 * nb + 8 * len(docs)
        d_text = torch.zeros(cap, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(len(docs) + 1, dtype=torch.int64, device=dev)
        n = d.decode_packed_device(d_raw.data_ptr(), d_tok_off.data_ptr(), d_doc_tok.data_ptr(), len(docs), len(flat), nb,
                                   d_text.data_ptr(), cap, d_off.data_ptr())
        body, off = d_text.cpu().numpy()[:n].tobytes(), d_off.cpu().numpy().tolist()
        assert off[0] == 0 and off[-1] == n and off == sorted(off)
        for i, doc in enumerate(docs):
            try:
                toks = [t.decode("utf-8") for t in doc]
            except UnicodeDecodeError:
                continue
            assert body[off[i]:off[i + 1]] == ref.decode(dec, toks).encode("utf-8"), (dec, doc)
    d = Decoder.fuse()
    bad = torch.from_numpy(np.array([0, 5, 3, nb], dtype=np.int64)).to(dev)
    three = torch.from_numpy(np.array([0, 3], dtype=np.int64)).to(dev)
    d_text = torch.zeros(nb + 8, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(2, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):  # CTOK_E_ARG: tok_off decreases
        d.decode_packed_device(d_raw.data_ptr(), bad.data_ptr(), three.data_ptr(), 1, 3, nb, d_text.data_ptr(), nb + 8, d_off.data_ptr())
    with pytest.raises(ValueError):  # tok_off does not end at n_bytes
        d.decode_packed_device(d_raw.data_ptr(), d_tok_off.data_ptr(), d_doc_tok.data_ptr(), len(docs), len(flat), nb + 1,
                               d_text.data_ptr(), nb + 8, d_off.data_ptr())


def test_behind_the_pre_tokenizer():
    """pre_tokenize_packed's (words, word_off, text_word) is decode_packed's input: the whitespace
    words of a text through strip() are the words joined."""
    texts = ["hello  world", "", " a\tb\u3000c ", "é 世界 😀", "   "] + [" ".join(t) for t in dc.random_token_lists("mixed", 5, 200, 30)]
    raw = [t.encode() for t in texts]
    off = np.cumsum([0] + [len(r) for r in raw]).astype(np.uint64)
    words, word_off, text_word = PreTokenizer.whitespace().pre_tokenize_packed(np.frombuffer(b"".join(raw), dtype=np.uint8), off)
    text, text_off = Decoder.strip().decode_packed(words, word_off, text_word)
    assert _texts(text, text_off) == ["".join(t.split()) for t in texts]
    text, text_off = Decoder.wordpiece("no word starts so", cleanup=False).decode_packed(words, word_off, text_word)
    assert _texts(text, text_off) == [" ".join(t.split()) for t in texts]


def test_models_decode_batch():
    vocab = {"[UNK]": 0, "un": 1, "##aff": 2, "##able": 3, "##": 4, "#": 5, ".": 6, "é": 7, "##é": 8, "x": 9, "X": 9}
    rng = random.Random(4)
    batch = [[1, 2, 3], [], [4, 1], [5, 1, 5, 1], [77, 1, 2 ** 32 - 1, 6], [9, 8, 7]] + \
        [[rng.randrange(0, 12) for _ in range(rng.randrange(0, 40))] for _ in range(300)]
    for prefix in ("##", "#", "é"):
        m = WordPieceModel(vocab, prefix)
        assert m.decode_batch(batch) == [m.decode(x) for x in batch]
        assert m.decode_batch(batch[:3]) == [m.decode(x) for x in batch[:3]]  # (the decoder is bound once)
        assert m.decode_batch([]) == []
    vocab = {"<unk>": 0, "a</w>": 1, "b": 2, "\u3000</w>": 3, "\x1f</w>": 4, "B": 2, "</w>": 5, "bb": 6, "é": 7, " ": 8}
    for suffix in ("</w>", "", "b"):
        m = CharBpeModel(vocab, [], suffix)
        assert m.decode_batch(batch) == [m.decode(x) for x in batch]
        assert m.decode_batch([[1, 3], [1, 4]]) == [m.decode([1, 3]), m.decode([1, 4])]
    for bad, err in (([[-1]], OverflowError), ([[2 ** 32]], OverflowError), ([["a"]], TypeError), ([[1.5]], TypeError), (["ab"], TypeError)):
        for m in (WordPieceModel({"a": 1}), CharBpeModel({"a": 1}, [])):
            with pytest.raises(err):
                m.decode_batch(bad)
            with pytest.raises(err):
                m.decode(bad[0])


def test_argument_errors():
    for bad in ("", "ab", "▁▁"):
        with pytest.raises(ValueError):
            Decoder.metaspace(bad)
        with pytest.raises(ValueError):
            Decoder.strip(bad)
    for bad in (1, b"_", None):
        with pytest.raises(TypeError):
            Decoder.metaspace(bad)
        with pytest.raises(TypeError):
            Decoder.strip(bad)
        with pytest.raises(TypeError):
            Decoder.wordpiece(bad)
        with pytest.raises(TypeError):
            Decoder.bpe(bad)
        with pytest.raises(TypeError):
            Decoder.ctc(bad)
        with pytest.raises(TypeError):
            Decoder.replace(bad, "a")
        with pytest.raises(TypeError):
            Decoder.replace("a", bad)
    with pytest.raises(TypeError):
        Decoder.ctc("<pad>", 1)
    with pytest.raises(TypeError):
        Decoder.metaspace("_", "yes")
    with pytest.raises(TypeError):
        Decoder.wordpiece("##", 1)
    for bad in (1.0, "1", None, True):
        with pytest.raises(TypeError):
            Decoder.strip("_", bad)
        with pytest.raises(TypeError):
            Decoder.strip("_", 0, bad)
    with pytest.raises(OverflowError):
        Decoder.strip("_", -1)
    with pytest.raises(OverflowError):
        Decoder.strip("_", 0, 2 ** 64)
    with pytest.raises(TypeError):
        Decoder.sequence("ab")
    with pytest.raises(TypeError):
        Decoder.sequence([Decoder.fuse(), "fuse"])
    with pytest.raises(UnsupportedConfigError):
        Decoder.sequence([Decoder.fuse()] * 1025)
    assert Decoder.sequence([Decoder.fuse()] * 1024).decode(["a", "b"]) == "ab"
    d = Decoder.fuse()
    with pytest.raises(TypeError):
        d.decode(b"x")
    with pytest.raises(TypeError):
        d.decode("a bare str")
    with pytest.raises(TypeError):
        d.decode_batch("a bare str")
    with pytest.raises(TypeError):
        d.decode_batch(["a bare str"])
    with pytest.raises(TypeError):
        d.decode(["a", b"b"])
    with pytest.raises(TypeError):
        d.decode_batch([["a", 1]])
    with pytest.raises(TypeError):
        d.set_vocab({1: b"a"})
    with pytest.raises(TypeError):
        d.set_vocab({"a": "a"})
    with pytest.raises(ValueError):  # CTOK_E_ARG: not UTF-8
        d.decode_packed(np.array([0xC3, 0x28], dtype=np.uint8), np.array([0, 2], dtype=np.uint64), np.array([0, 1], dtype=np.uint64))
    with pytest.raises(ValueError):  # a token that ends inside a char
        d.decode_packed(np.array([0xC3, 0xA9], dtype=np.uint8), np.array([0, 1, 2], dtype=np.uint64), np.array([0, 2], dtype=np.uint64))
    with pytest.raises(ValueError):
        d.decode_packed(np.zeros(2, dtype=np.uint8), np.array([0, 2, 1], dtype=np.uint64), np.array([0, 2], dtype=np.uint64))
    import ctypes
    from complexity_tokenizer import _native
    nb, fresh = ctypes.c_uint64(), Decoder.fuse()
    assert _native.lib.ctok_decoder_fetch(fresh._h, None, 0, np.zeros(1, dtype=np.uint64).ctypes.data, ctypes.byref(nb)) == _native.CTOK_E_ARG
    assert repr(Decoder.wordpiece()) == "Decoder.wordpiece('##', True)"
    assert repr(Decoder.sequence([Decoder.ctc(word_delimiter_token="|"), Decoder.strip("_", 1), Decoder.replace("a", "")])) == \
        "Decoder.sequence([Decoder.ctc('<pad>', '|'), Decoder.strip('_', 1, 0), Decoder.replace('a', '')])"
    assert repr(Decoder.byte_level()) == "Decoder.byte_level()" and repr(Decoder.metaspace()) == "Decoder.metaspace('▁', True)"
    assert repr(Decoder.bpe()) == "Decoder.bpe('</w>')" and repr(Decoder.fuse()) == "Decoder.fuse()"


def test_stats_and_stage_names():
    d = Decoder.sequence([Decoder.wordpiece(), Decoder.replace("l", "LL")])
    assert d.decode_batch([["he", "##llo", "."], ["x"]]) == ["heLLLLo.", "x"]
    st = d.last_stats
    assert st["steps"] == 2 and st["passes"] == 3 and st["docs"] == 2 and st["tokens"] == 4  # (wordpiece: the rule, the clean-up)
    assert st["bytes_in"] == 9 and st["bytes_out"] == 9 and st["bytes_peak"] == 9
    assert [n for n, _ in st["stages"]] == ["gather", "wordpiece", "replace"]
    assert st["stages"][0][1] == 0.0 and all(ms > 0.0 for _, ms in st["stages"][1:])
    d = Decoder.byte_level()
    assert d.decode_batch([["â", "Ĥ"]]) == ["�"]
    st = d.last_stats
    assert st["passes"] == 2 and st["bytes_in"] == 4 and st["bytes_out"] == 3 and st["bytes_peak"] == 4
