"""CPU tests of complexity_tokenizer.UnigramTrainer and UnigramModel: csrc/unigram_hd.h (what the
kernels of csrc/unigram.hip share) driven by tools/unigram_check.cpp, built with g++ under
AddressSanitizer and UBSan, against the Python restatement; the reference's signatures
(src/bindings/trainers.rs:164-196, src/bindings/models.rs:60-64), argument errors in the style of
WordPieceTrainer's, the C ABI's exports, the host-only methods and the loud failure without a device.
No GPU."""
import ctypes
import inspect
import os
import random
import struct
import subprocess

import pytest

import complexity_tokenizer
from complexity_tokenizer import DeviceError, UnigramModel, UnigramTrainer
from complexity_tokenizer import _native as _n
from tests import unigram_cases as uc
from tests.unigram_ref import WHITE_SPACE, RefUnigramModel, RefUnigramTrainer, metaspace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "complexity-tokenizer_amd")


@pytest.fixture(scope="module")
def tool(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("uni") / "unigram_check")
    src = os.path.join(PKG, "tools", "unigram_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    src, "-o", exe], check=True)
    return exe


def u64(*v):
    return struct.pack("<%dQ" % len(v), *v)


def pack_texts(texts):
    raw = [t.encode("utf-8") if isinstance(t, str) else t for t in texts]
    off = [0]
    for r in raw:
        off.append(off[-1] + len(r))
    return u64(len(raw)) + u64(*off) + b"".join(raw)


def run(tool, job):
    r = subprocess.run([tool], input=job, capture_output=True)
    assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
    return r.stdout


def tool_encode(tool, vocab, unk, texts):
    """what UnigramModel does with the kernels' shared code: ids per text"""
    m = RefUnigramModel(vocab, unk)
    pats = [(t.encode("utf-8"), i) for t, (i, _) in m.vocab.items() if t]
    wl = max([len(t) for t in m.vocab] + [0])
    job = u64(1, len(pats)) + b"".join(u64(len(p)) + p + u64(i) for p, i in pats)
    job += u64(len(vocab)) + b"".join(struct.pack("<d", s) for _, s in m.list)
    job += u64(m.unk_id) + struct.pack("<d", m.min_score) + u64(wl, max(wl, 1)) + pack_texts(texts)
    out = run(tool, job)
    ids, at = [], 0
    for _ in texts:
        (n,) = struct.unpack_from("<Q", out, at)
        ids.append(list(struct.unpack_from("<%dQ" % n, out, at + 8)))
        at += 8 + 8 * n
    assert at == len(out)
    return ids


@pytest.mark.parametrize("kind", ["ties", "special", "repeat", "random"])
def test_lookup_and_viterbi_step_follow_the_oracle(tool, kind):
    rng = random.Random("tool" + kind)
    for _ in range(25):
        vocab = uc.random_model(rng, kind)
        unk = rng.choice(["<unk>", "a"])
        texts = [uc.random_text(rng) for _ in range(8)] + ["", "a"]
        assert tool_encode(tool, vocab, unk, texts) == uc.ref_encode(vocab, texts, unk), vocab


def test_window_in_chars_across_code_point_widths(tool):
    vocab = uc.hand_vocab()
    longest = "\U0001F600" * 5  # 5 chars, 20 bytes: the window is counted in chars
    texts = [longest, longest + "a", "a" + longest, longest * 2, "abé中c", "abé中", "é中\U0001F600▁" * 3, "ñ" + longest + "ñ",
             "abcabca" * 9, "中" * 63 + "abc", "é" * 64 + "é中", "a" * 257]
    want = uc.ref_encode(vocab, texts)
    assert want[0] == [17] and want[1] == [17, 1] and 0 in want[7]
    assert tool_encode(tool, vocab, "<unk>", texts) == want
    # a vocab without a match for anything: the fallback alone, id 0 without <unk>
    assert tool_encode(tool, [("zz", -1.0)], "<unk>", ["ab"]) == [[0, 0]] == uc.ref_encode([("zz", -1.0)], ["ab"])
    assert tool_encode(tool, [], "<unk>", ["ab", ""]) == [[0, 0], []] == uc.ref_encode([], ["ab", ""])


def tool_metaspace(tool, texts):
    out = run(tool, u64(2) + pack_texts(texts))
    (n,) = struct.unpack_from("<Q", out, 0)
    off = struct.unpack_from("<%dQ" % (n + 1), out, 8)
    body = out[8 * (n + 2):]
    assert len(body) == off[n]
    return [body[off[i]:off[i + 1]].decode("utf-8") for i in range(n)]


def meta_want(texts):  # (the check gets NFC text, as the kernel does)
    return [s for t in texts for s in metaspace(t)]


def test_metaspace_spans(tool):
    ws = [chr(c) for c in WHITE_SPACE]
    texts = ["hello world", "a\tb", "", "a▁ b", "", "", "\t", " ", "  a  ", "\n\n", "x"]
    for w in ws:
        texts += [w, w + w, w + "a", "a" + w, "a" + w + w + "b", "é" + w + "中" + w + "\U0001F600"]
    for k in range(56, 70):  # chars, spaces and cuts on both sides of the 64-byte span
        texts += ["a" * k + " b", "a" * k + "\tb", "a" * k + "　b", "a" * k + "中 \U0001F600", " " * k, "\t" * k + "z", ""]
    assert tool_metaspace(tool, texts) == meta_want(texts)
    assert tool_metaspace(tool, []) == [] and tool_metaspace(tool, [""]) == ["▁"] and tool_metaspace(tool, ["", ""]) == ["▁", "▁"]
    rng = random.Random(5)
    for _ in range(20):
        texts = uc.texts_over(rng.random(), rng.randint(1, 40), ["a", "é", "中", "\U0001F600", " ", " ", "\t", "　", "▁"], 0, 50)
        assert tool_metaspace(tool, texts) == meta_want(texts)
    # bytes that are not UTF-8: nothing is read outside the text (the sanitizers watch)
    for junk in (b"\xe2", b"\xe2\x80", b"a\xf0\x9f", b"\x80\x80 \xe2\x80", b"\xc2", b"\xff\xfe\t\x80"):
        run(tool, u64(2) + pack_texts([junk, b"ok", junk * 30]))


def test_substrings_of_every_sentence(tool):
    for sentences in (["▁hello▁world", "▁", "é中\U0001F600a", ""], meta_want(uc.unicode_corpus()[:80]), meta_want(uc.aab()[:60])):
        raw = "".join(sentences).encode("utf-8")
        for L in (1, 2, 16, 1000):
            out = run(tool, u64(3, L) + pack_texts(sentences))
            (n,) = struct.unpack_from("<Q", out, 0)
            pairs = struct.unpack_from("<%dQ" % (2 * n), out, 8)
            got = {}
            for i in range(n):
                s = raw[pairs[2 * i]:pairs[2 * i + 1]].decode("utf-8")
                got[s] = got.get(s, 0) + 1
            assert got == RefUnigramTrainer(max_piece_length=L).count_substrings(sentences)


def test_signatures_are_the_references():
    assert "UnigramTrainer" in complexity_tokenizer.__all__ and "UnigramModel" in complexity_tokenizer.__all__
    p = inspect.signature(UnigramTrainer.__init__).parameters
    assert list(p)[1:] == ["vocab_size", "special_tokens", "initial_vocab_size", "shrinking_factor", "n_iterations",
                           "max_piece_length", "device"]
    assert [p[k].default for k in list(p)[1:]] == [8000, None, 1000000, 0.75, 16, 16, 0]
    p = inspect.signature(UnigramModel.__init__).parameters
    assert list(p)[1:] == ["vocab", "unk_token", "device"] and [p[k].default for k in list(p)[2:]] == ["<unk>", 0]
    p = inspect.signature(RefUnigramTrainer.__init__).parameters
    assert [p[k].default for k in list(p)[1:]] == [8000, None, 1000000, 0.75, 16, 16]
    for name in ("train", "train_from_iterator", "train_sentences", "get_vocab", "sentences", "substring_counts",
                 "expected_counts", "stats"):
        assert callable(getattr(UnigramTrainer, name))
    for name in ("encode", "decode", "token_to_id", "id_to_token", "encode_batch", "encode_batch_flat", "get_vocab"):
        assert callable(getattr(UnigramModel, name))
    # the getter is the vocab's size, not the target (src/bindings/trainers.rs:211-214)
    assert UnigramTrainer(vocab_size=500).vocab_size == 0


def test_argument_errors():
    for kw in (dict(vocab_size="10"), dict(vocab_size=True), dict(n_iterations=2.0), dict(max_piece_length=None),
               dict(shrinking_factor="0.5"), dict(shrinking_factor=None), dict(special_tokens="<unk>"),
               dict(special_tokens=["<unk>", 3])):
        with pytest.raises(TypeError):
            UnigramTrainer(**kw)
    for kw in (dict(vocab_size=-1), dict(vocab_size=1 << 64), dict(initial_vocab_size=-1), dict(n_iterations=1 << 64),
               dict(max_piece_length=-2)):
        with pytest.raises(OverflowError):
            UnigramTrainer(**kw)
    for sf in (1, 0.5, -1, float("nan"), float("inf")):  # any float or int
        UnigramTrainer(shrinking_factor=sf)
    with pytest.raises(TypeError):
        UnigramTrainer().train_from_iterator("one text")
    with pytest.raises(TypeError):
        UnigramTrainer().train("one_file.txt")
    with pytest.raises(TypeError):
        UnigramTrainer().train_sentences("▁a")
    with pytest.raises(TypeError):
        UnigramTrainer().train_sentences([b"a"])
    with pytest.raises(IOError):
        UnigramTrainer().train([os.path.join(ROOT, "no", "such", "file.txt")])
    for vocab in ("ab", [("a",)], [["a", 1.0]], [(3, 1.0)], [("a", "1")], [("a", None)], [("a", 1.0, 2)]):
        with pytest.raises(TypeError):
            UnigramModel(vocab)
    with pytest.raises(TypeError):
        UnigramModel([("a", 1.0)], unk_token=None)
    with pytest.raises(TypeError):
        UnigramModel([("a", 1.0)]).encode(b"a")
    UnigramModel([("a", float("nan")), ("b", float("inf")), ("c", -float("inf")), ("d", 3)])  # any float


def test_train_reads_lines_before_it_needs_a_device(tmp_path):
    p = tmp_path / "bad.txt"
    p.write_bytes(b"ok\n\xff\xfe\n")
    with pytest.raises(IOError):
        UnigramTrainer().train([str(p)])


def test_exports_and_header():
    lib = ctypes.CDLL(_n.LIB_PATH)
    with open(os.path.join(ROOT, "include", "ctok_unigram.h")) as f:
        header = f.read()
    names = [n for n in _n.SIGS if n.startswith("ctok_uni_")]
    assert len(names) == 14
    for name in names:
        assert hasattr(lib, name) and name + "(" in header, name
    # the conventions are stated where the C ABI is declared
    for words in ("among\n * equal counts, ascending UTF-8 bytes", "CTOK_E_PANIC", "libm's log", "-inf quirk",
                  "the smallest start"):
        assert words in header, words


def test_null_arguments_are_refused():
    h = ctypes.c_void_p()
    assert _n.lib.ctok_uni_trainer_create(None, ctypes.byref(h)) == _n.CTOK_E_ARG
    cfg = _n.UniTrainerConfig(vocab_size=10, n_special=1, special=b"a", special_off=None)
    assert _n.lib.ctok_uni_trainer_create(ctypes.byref(cfg), ctypes.byref(h)) == _n.CTOK_E_ARG
    off = (ctypes.c_uint64 * 2)(0, 1)
    cfg = _n.UniTrainerConfig(vocab_size=10, n_special=1, special=b"\xff", special_off=off)
    assert _n.lib.ctok_uni_trainer_create(ctypes.byref(cfg), ctypes.byref(h)) == _n.CTOK_E_ARG
    t = UnigramTrainer()
    assert _n.lib.ctok_uni_trainer_train(t._h, None, None, 1) == _n.CTOK_E_ARG
    assert _n.lib.ctok_uni_trainer_train(None, None, None, 0) == _n.CTOK_E_ARG
    assert _n.lib.ctok_uni_trainer_train_sentences(t._h, None, None, 1) == _n.CTOK_E_ARG
    assert _n.lib.ctok_uni_trainer_train_sentences(t._h, b"\xc3", off, 1) == _n.CTOK_E_ARG  # not UTF-8
    assert _n.lib.ctok_uni_trainer_stats(t._h, None) == _n.CTOK_E_ARG
    assert _n.lib.ctok_uni_trainer_result(t._h, None, None) == _n.CTOK_E_ARG
    assert _n.lib.ctok_uni_trainer_sentences(t._h, None) == _n.CTOK_E_ARG
    assert _n.lib.ctok_uni_trainer_substring_counts(t._h, None, None) == _n.CTOK_E_ARG
    assert _n.lib.ctok_uni_trainer_expected_counts(t._h, None, None) == _n.CTOK_E_ARG
    assert _n.lib.ctok_uni_trainer_vocab_size(None) == 0 and _n.lib.ctok_uni_model_vocab_size(None) == 0
    _n.lib.ctok_uni_trainer_destroy(None)
    _n.lib.ctok_uni_model_destroy(None)
    assert _n.lib.ctok_uni_model_create(None, None, None, 1, b"<unk>", 0, ctypes.byref(h)) == _n.CTOK_E_ARG
    assert _n.lib.ctok_uni_model_create(None, None, None, 0, None, 0, ctypes.byref(h)) == _n.CTOK_E_ARG
    assert _n.lib.ctok_uni_model_create(None, None, None, 0, b"<unk>", 0, None) == _n.CTOK_E_ARG
    sc = (ctypes.c_double * 1)(1.0)
    assert _n.lib.ctok_uni_model_create(b"\xff", off, sc, 1, b"<unk>", 0, ctypes.byref(h)) == _n.CTOK_E_ARG
    m = UnigramModel([("a", 1.0)])
    assert _n.lib.ctok_uni_model_encode_batch(m._h, None, None, 1, None, None) == _n.CTOK_E_ARG


def test_before_training_everything_is_empty():
    t = UnigramTrainer(vocab_size=100)
    assert t.get_vocab() == [] and t.sentences() == [] and t.substring_counts() == {} and t.expected_counts() == {}
    st = t.stats()
    assert st["iterations"] == 0 and st["vocab_sizes"] == [] and st["table_capacity"] == 0 and st["sentences"] == 0


def test_model_host_methods_follow_the_oracle():
    vocab = [("a", -1.0), ("b", float("nan")), ("a", -3.0), ("<unk>", -2.0), ("", -1.0), ("中文", 0.5)]
    m, r = UnigramModel(vocab), RefUnigramModel(vocab)
    assert m.vocab_size == r.vocab_size() == 5
    got = m.get_vocab()
    uc.same_vocab(got, vocab)
    for ids in ([0, 1], [2, 5, 5], [9, 0, 99], [], [4, 3]):
        assert m.decode(ids) == r.decode(ids), ids
    for i in range(8):
        assert m.id_to_token(i) == r.id_to_token(i)
    for t in ("a", "b", "", "x", "中文"):
        assert m.token_to_id(t) == r.token_to_id(t)
    assert UnigramModel([]).vocab_size == 0
    with pytest.raises(OverflowError):
        m.decode([-1])


def test_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(DeviceError):
        UnigramTrainer(vocab_size=50).train_from_iterator(["hello world"])
    with pytest.raises(DeviceError):
        UnigramTrainer(vocab_size=50).train_sentences(["▁ab"])
    with pytest.raises(DeviceError):
        UnigramModel([("a", 1.0)]).encode("a")
