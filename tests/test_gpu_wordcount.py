"""GPU word counting of the trainer (csrc/wordcount.hip): Trainer.word_counts() after count_batch
against the oracle's count (oracle/trainer_ref.py RefTrainer._count_into, keys mapped back through
bytes_to_unicode), on the smallest inputs at which each mechanism can go wrong: NUL bytes, document
edges, the dword / clipped-length boundaries of the byte compare, one hot word (on-chip
aggregation and its flush), many unique words, a table too small (overflow), chunking, the host
fallback, and the size of what is read back."""
import ctypes
import random

import numpy as np
import pytest

from complexity_tokenizer import Trainer
from complexity_tokenizer import _native as _n
from datagen import corpus
from oracle import ref_py, trainer_ref

pytestmark = pytest.mark.gpu

_U2B = {c: b for b, c in ref_py.bytes_to_unicode().items()}


def _oracle(texts, **kw):
    ref = trainer_ref.RefTrainer(**kw)
    wf = {}
    ref._count_into(wf, texts)
    return {bytes(_U2B[c] for c in w): n for w, n in wf.items()}


def _gpu(texts, **kw):
    t = Trainer(**kw)
    t.count_batch(texts)
    return t.word_counts(), t.count_stats()


def _check(texts, host_chunks=0, **kw):
    want = _oracle(texts, **kw)
    got, st = _gpu(texts, **kw)
    print("count_stats", st)
    if got != want:
        diff = [(w, got.get(w), want.get(w)) for w in sorted(set(got) | set(want)) if got.get(w) != want.get(w)]
        raise AssertionError("%d words differ (word, gpu, oracle), first %r" % (len(diff), diff[:5]))
    assert st["host_chunks"] == host_chunks and st["chunks"] >= 1
    assert st["words"] == sum(want.values())
    if not host_chunks:
        assert st["unique_words"] >= len(want) and st["ms_device"] > 0
    return got, st


def _c1_texts(n=400):
    text, off = corpus.corpus_c1()
    return [d.decode() for d in corpus.unpack(text, off)][:n]


def _rand_texts(seed, n, alpha, lo=1, hi=40):
    rng = random.Random(seed)
    return ["".join(rng.choice(alpha) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


@pytest.fixture(scope="module")
def many_unique():
    """50,000 distinct words of 3..12 bytes (a space, then letters), each 1..4 times, shuffled
    into documents; with the oracle's count."""
    rng = random.Random(11)
    words = set()
    while len(words) < 50_000:
        words.add(" " + "".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(2, 11))))
    occ = [w for w in sorted(words) for _ in range(rng.randint(1, 4))]
    rng.shuffle(occ)
    texts = ["".join(occ[i:i + 500]) for i in range(0, len(occ), 500)]
    return texts, _oracle(texts)


def test_basic_c1():
    got, st = _check(_c1_texts(400))
    assert len(got) > 500 and st["pieces"] >= st["words"] > 0


def test_unicode_and_nfc():
    """Multi-byte chars and decomposed sequences (e + U+0301, n + U+0303) that NFC composes on the
    GPU: the words are counted in the normalised text, whose length differs from the input's."""
    alpha = ["\u00e9", "e\u0301", "\u4e2d", "\u6587", "\U0001f600", "a", " ", "n\u0303", "\u00df"]
    texts = _rand_texts(4, 400, alpha, 1, 12)
    got, _ = _check(texts)
    raw = b"".join(t.encode() for t in texts)
    assert b"\xcc\x81" in raw and b"\xcc\x83" in raw  # the input holds the combining marks
    assert not any(b"\xcc\x81" in w or b"\xcc\x83" in w for w in got)  # the counted words do not
    assert any(w not in raw for w in got)  # some key is not a substring of the raw input


def test_nul_bytes_documents_and_last_byte():
    """Zero-padded keys, pieces joined across documents, empty documents, and equal-length words
    that differ only in the last byte."""
    texts = ["a\x00 a\x00\x00 a", "ab", "ab", "", "x" * 40 + " " + "x" * 39 + "y"]
    got, _ = _check(texts)
    assert got == {b"a": 1, b"\x00": 1, b" a": 2, b"\x00\x00": 1, b"ab": 2, b"x" * 40: 1, b" " + b"x" * 39 + b"y": 1}


def test_length_boundaries():
    """Words of 1 .. 5000 bytes around the compare's dword steps, the hash's byte limit and long
    words; for every length a pair sharing all but the last byte and a pair where one is a prefix
    of the other (length n and n + 1 of the same letter run); 1..3 occurrences scattered over
    documents.  Plus two words past the descriptor's clipped length (65535) that differ only in
    length, and two of equal length there that differ in the last byte."""
    rng = random.Random(5)
    occ = []
    for n in (1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 5000):
        for w in ("q" * n, "q" * (n + 1), "q" * (n - 1) + "r", "q" * (n - 1) + "s"):
            occ += [w] * rng.randint(1, 3)
    occ += ["k" * 65535, "k" * 65536, "k" * 70000, "k" * 69999 + "j", "k" * 70000]
    rng.shuffle(occ)
    # letter runs are single pieces; " " + run is the piece after the first of a document
    texts = [" ".join(occ[i:i + 3]) for i in range(0, len(occ), 3)]
    got, _ = _check(texts)
    assert got.get(b"k" * 70000, 0) + got.get(b" " + b"k" * 70000, 0) == 2


def test_one_hot_word():
    """One word 200,000 times: contention on one slot, on-chip aggregation and its flush; and the
    readback is the table's entries, not the text (800 KB of text, one word out)."""
    texts = [" the" * 200_000]
    got, st = _check(texts)
    assert got == {b" the": 200_000}
    assert st["bytes_d2h"] < len(texts[0])
    assert st["unique_words"] == 1
    got, st = _check([" the" * 200] * 1000)
    assert got == {b" the": 200_000}
    assert st["bytes_d2h"] < 800_000


def test_many_unique_words(many_unique):
    texts, want = many_unique
    got, st = _gpu(texts)
    print("count_stats", st)
    assert got == want
    assert st["host_chunks"] == 0 and st["unique_words"] == len(want)


def test_rerun_with_larger_table():
    """5,000 distinct words, each once: the first table (pieces / 2 rounded up to 4,096 slots) is
    smaller than the unique words, so the chunk is counted again on the device with the larger
    table; nothing goes to the host walk."""
    rng = random.Random(13)
    words = set()
    while len(words) < 5_000:
        words.add(" " + "".join(rng.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(4, 9))))
    words = sorted(words)
    texts = ["".join(words[i:i + 250]) for i in range(0, len(words), 250)]
    got, st = _check(texts)
    assert len(got) == 5_000 and set(got.values()) == {1}
    assert st["rerun_chunks"] == 1 and st["host_chunks"] == 0 and st["unique_words"] == 5_000


def test_overflow_counts_stay_exact(many_unique, monkeypatch):
    """A table far too small for the chunk's words: the probe sequences run out, the chunk is
    counted on the host path, the counts are exact and the call returns normally."""
    texts, want = many_unique
    monkeypatch.setenv("CTOK_TRAIN_COUNT_SLOTS", "4096")
    got, st = _gpu(texts)
    print("count_stats", st)
    assert got == want
    assert st["chunks"] == 1 and st["host_chunks"] == 1
    # with chunks small enough for the same table, the device path counts them all
    monkeypatch.setenv("CTOK_TRAIN_CHUNK_BYTES", "6000")
    got, st = _gpu(texts)
    assert got == want
    assert st["chunks"] > 1 and st["host_chunks"] == 0


def test_min_word_length():
    lines = ["hello world hello world", "hello hello hello", "wörld wörld"]
    _check(lines, min_word_length=3)
    got, st = _check(lines + ["a bc def gh i, jkl"], min_word_length=3)
    assert got[b" def"] == 1 and got[b" bc"] == 1 and b"a" not in got and b" i" not in got and b"," not in got
    assert st["pieces"] == st["words"] + 3  # "a", " i" and "," are dropped on the device


def test_chunking(monkeypatch):
    texts = _c1_texts(400) + ["x" * 5000 + " tail"]
    one, st1 = _gpu(texts)
    monkeypatch.setenv("CTOK_TRAIN_CHUNK_BYTES", "700")
    many, st = _gpu(texts)
    assert one == many == _oracle(texts)
    assert st1["chunks"] == 1 and st1["host_chunks"] == 0
    assert st["chunks"] > 10 and st["host_chunks"] == 0
    monkeypatch.delenv("CTOK_TRAIN_CHUNK_BYTES")
    t = Trainer()
    for i in range(0, len(texts), 128):
        t.count_batch(texts[i:i + 128])
        assert t.count_stats()["host_chunks"] == 0
    assert t.word_counts() == one


def test_host_fallback(monkeypatch):
    texts = _c1_texts(400)
    dev, _ = _gpu(texts)
    monkeypatch.setenv("CTOK_TRAIN_COUNT", "host")
    host, st = _check(texts, host_chunks=1)
    assert host == dev
    assert st["ms_device"] == 0 and st["unique_words"] == 0


def _raw_word_counts(t):
    nw, nb = ctypes.c_uint64(), ctypes.c_uint64()
    assert _n.lib.ctok_trainer_word_counts(t._h, 1, None, 0, None, None, 0, ctypes.byref(nw), ctypes.byref(nb)) == 0
    blob = np.zeros(nb.value + 1, dtype=np.uint8)
    off = np.zeros(nw.value + 1, dtype=np.uint64)
    freqs = np.zeros(nw.value + 1, dtype=np.uint32)
    assert _n.lib.ctok_trainer_word_counts(t._h, 1, blob.ctypes.data, nb.value, off.ctypes.data, freqs.ctypes.data,
                                           nw.value, ctypes.byref(nw), ctypes.byref(nb)) == 0
    return blob.tobytes(), off.tobytes(), freqs.tobytes()


def test_deterministic_and_sorted():
    texts = _c1_texts(300)
    outs = []
    for _ in range(2):
        t = Trainer(vocab_size=300)
        t.count_batch(texts)
        assert t.count_stats()["host_chunks"] == 0
        outs.append(_raw_word_counts(t))
    assert outs[0] == outs[1]
    words = list(t.word_counts())
    assert words == sorted(words) and len(words) > 100
    # the counts feed training as before
    t.finish_training()
    assert t.word_counts() == {}
