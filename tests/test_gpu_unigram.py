"""GPU parity of complexity_tokenizer.UnigramTrainer and UnigramModel (csrc/unigram.hip) against the
restatement of the reference's src/trainers.rs and src/models.rs (tests/unigram_ref.py): the model's
Viterbi encode, Metaspace after NFC, the substring counts, whole trainings with every score compared
bit for bit, the reference's quirks, and its panic.  Exact equality everywhere.  Every corpus goes
through the restatement first and the properties a test relies on are asserted there."""
import random

import pytest

from complexity_tokenizer import PanicException, UnigramModel, UnigramTrainer
from datagen import corpus
from tests import unigram_cases as uc
from tests.unigram_ref import INF, WHITE_SPACE, RefUnigramModel, RefUnigramTrainer, metaspace
from tests.unigram_ref import PanicException as RefPanic

pytestmark = pytest.mark.gpu

_cache = {}
SPAN = 64  # csrc/unigram_hd.h kSpan


def _c1():
    if "c1" not in _cache:
        text, off = corpus.corpus_c1()
        _cache["c1"] = [d.decode() for d in corpus.unpack(text, off)][:340]
    return _cache["c1"]


def _model_same(vocab, texts, unk="<unk>", ref_fn="encode"):
    m, r = UnigramModel(vocab, unk), RefUnigramModel(vocab, unk)
    want = [getattr(r, ref_fn)(t) for t in texts]
    got = m.encode_batch(texts)
    bad = [i for i in range(len(texts)) if got[i] != want[i]]
    assert not bad, (len(bad), texts[bad[0]][:80], got[bad[0]][:20], want[bad[0]][:20])
    assert m.vocab_size == r.vocab_size()
    return m, want


# ---- 1. the model -----------------------------------------------------------------------------------

def test_model_hand_vocab_edges():
    vocab = uc.hand_vocab()
    longest = "\U0001F600" * 5
    texts = ["", "a", "\U0001F600", "ñ", "abca", "zabc", "abcz", "abcaz", longest, longest + "a", "a" + longest, "abé中c",
             "abé中", "é中\U0001F600▁é中", "▁a▁a▁", " a b", "", "中\U0001F600a中\U0001F600", "xyz"]
    m, want = _model_same(vocab, texts)
    assert want[0] == [] and want[8] == [17] and want[9] == [17, 1] and want[3] == [0] and want[18] == [0, 0, 0]
    assert m.encode("abca") == want[4] == [14] and m.encode("") == []
    assert UnigramModel(vocab).encode_batch([]) == []
    # <unk> absent: an unknown char is id 0; <unk> not first: its own id
    _, want = _model_same([("a", -1.0), ("b", -2.0)], ["xa", "x", "ab"])
    assert want == [[0, 0], [0], [0, 1]]
    _, want = _model_same([("a", -1.0), ("<unk>", -2.0)], ["xa", "x"])
    assert want == [[1, 0], [1]]
    _, want = _model_same([("a", -1.0), ("b", -2.0)], ["xb"], unk="b")
    assert want == [[1, 1]]
    _model_same([], ["ab", ""])
    _model_same([("", -1.0)], ["ab", ""])


def test_model_tie_repeat_and_quirks():
    # equal sums: ab (-2) against a + b (-1 + -1): the smallest start
    _, want = _model_same([("a", -1.0), ("b", -1.0), ("ab", -2.0), ("<unk>", -5.0)], ["ab", "abab", "aab", "ba"])
    assert want == [[2], [2, 2], [0, 2], [1, 0]]
    _, want = _model_same([("ab", -2.0), ("a", -1.0), ("b", -1.0), ("abab", -4.0)], ["abab", "ababab"])
    assert want == [[3], [0, 3]]
    # a repeated string: the last id and score; vocab_size counts distinct strings
    vocab = [("a", -1.0), ("b", -1.0), ("a", -9.0), ("ab", -3.0), ("b", -0.5)]
    m, want = _model_same(vocab, ["ab", "aabb", "ba"])
    assert m.vocab_size == 3 and want[0] == [3] and m.token_to_id("a") == 2 and m.id_to_token(0) == "a"
    # -inf and NaN on the only path: nothing reaches the end, id 0
    _, want = _model_same([("a", -INF), ("b", -1.0), ("c", -1.0)], ["bab", "ab", "bcb", "a", ""])
    assert want == [[0], [0], [1, 2, 1], [0], []]
    _, want = _model_same([("x", -1.0), ("a", uc.NAN), ("b", -1.0), ("ab", -3.0)], ["bab", "bb", "a", "aab", "ba"])
    assert want == [[2, 3], [2, 2], [0], [0], [0]]
    _model_same([("a", INF), ("b", -INF), ("ab", uc.NAN), ("c", 0.0), ("<unk>", -0.0)], ["abc", "cab", "aaa", "ca", "cb", "x"])


@pytest.mark.parametrize("kind", ["ties", "special", "repeat", "random"])
def test_model_random_models(kind):
    rng = random.Random("gpu" + kind)
    for _ in range(12):
        vocab = uc.random_model(rng, kind)
        _model_same(vocab, [uc.random_text(rng) for _ in range(12)] + ["", "a"], unk=rng.choice(["<unk>", "a"]))


def test_model_random_scores_400_texts():
    rng = random.Random(400)
    toks = sorted({"".join(rng.choice(uc.ALPHA) for _ in range(rng.choice([1, 1, 2, 2, 3, 4, 5]))) for _ in range(150)})
    vocab = [("<unk>", -20.0)] + [(t, -rng.random() * 15.0) for t in toks]
    texts = [uc.random_text(rng, 0, 90) for _ in range(400)]
    assert min(map(len, texts)) == 0 and max(map(len, texts)) == 90
    m, want = _model_same(vocab, texts)
    assert len({i for w in want for i in w}) > len(vocab) // 2  # most of the vocab is in use
    # encode_batch_flat: offsets around empty texts
    batch = ["", "ab", "", "", "é中", ""]
    ids, off = m.encode_batch_flat(batch)
    r = RefUnigramModel(vocab)
    assert off.tolist()[0] == 0 and [ids[off[i]:off[i + 1]].tolist() for i in range(6)] == [r.encode(t) for t in batch]
    assert off[1] == 0 and off[3] == off[4] and off[5] == off[6] == len(ids)
    ids, off = m.encode_batch_flat(["", ""])
    assert len(ids) == 0 and off.tolist() == [0, 0, 0]


def test_model_lane_and_block_edges_and_a_long_text():
    rng = random.Random(64)
    vocab = uc.hand_vocab()
    texts = []
    for n in (63, 64, 65, 255, 256, 257):
        texts.append("".join(rng.choice("abc") for _ in range(n)))                      # n chars, n bytes
        texts.append("".join(rng.choice(uc.ALPHA) for _ in range(n)))                   # n chars
        t = ""
        while len(t.encode()) < n - 4:
            t += rng.choice(uc.ALPHA)
        texts.append(t + "a" * (n - len(t.encode())))                                   # n bytes
    assert sorted({len(t.encode()) for t in texts[2::3]}) == [63, 64, 65, 255, 256, 257]
    _model_same(vocab, texts)
    # a window wider than a wavefront: tokens of up to 70 chars
    wide = vocab + [("a" * 70, -3.0), ("ab" * 33, -2.0), ("c" * 65, -1.0)]
    _, want = _model_same(wide, ["a" * 70, "a" * 139 + "b", "ab" * 40, "c" * 200 + "ab" * 33 + "a" * 71, "c" * 64])
    assert want[0] == [len(vocab)] and len(vocab) + 2 in want[3]
    # 20,000 chars through the ring of best values (the restatement's lattice formulation, which
    # tests/test_unigram_ref_cpu.py holds against the double loop; the loop itself is quadratic)
    long_text = "".join(rng.choice(uc.ALPHA + ["a", "b", "c", "x"]) for _ in range(20000))
    _model_same(vocab, [long_text, "ab"], ref_fn="encode_lattice")


# ---- 2. pretokenize ---------------------------------------------------------------------------------

def _sentences_same(texts):
    tr = UnigramTrainer(vocab_size=1 << 40)  # no EM iteration: pretokenize and the seed vocab only
    tr.train_from_iterator(texts)
    want = [s for t in texts for s in metaspace(t)]
    got = tr.sentences()
    assert got == want, next((g, w) for g, w in zip(got + [None], want + [None]) if g != w)
    return tr


def test_sentences_white_space_nfc_and_spans():
    ws = [chr(c) for c in WHITE_SPACE]
    assert len(ws) == 25
    texts = ["hello world", "a\tb", "", "a▁ b", "", "", "e\u0301", "e\u0301 e\u0301\te\u0301", "s\u0323\u0307", "\u00e9"]
    for w in ws:
        texts += [w, w + w, w + "a", "a" + w, "a" + w + w + "b", w + "a" + w]
    for k in range(SPAN - 6, SPAN + 4):
        texts += ["a" * k + " b", "a" * k + "\tb", "a" * k + "　b", "a" * k + "中 \U0001F600 é", " " * k, "\t" * k + "z", ""]
    tr = _sentences_same(texts)
    st = tr.stats()
    assert st["sentences"] == len(tr.sentences()) and st["iterations"] == 0
    _sentences_same(["", "", ""])
    _sentences_same(["\t", "\n\n"])
    _sentences_same(uc.unicode_corpus())


# ---- 3. substring counts ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["aab", "unicode"])
@pytest.mark.parametrize("length", [1, 2, 16, 1000])
def test_substring_counts(name, length):
    texts = uc.aab() if name == "aab" else uc.unicode_corpus()
    ref = RefUnigramTrainer(vocab_size=1 << 40, max_piece_length=length)
    ref.train_from_iterator(texts)
    assert max(map(len, ref.sentences)) < 1000 and max(map(len, ref.sentences)) > 16
    tr = UnigramTrainer(vocab_size=1 << 40, max_piece_length=length)
    tr.train_from_iterator(texts)
    assert tr.substring_counts() == ref.substring_counts
    uc.same_vocab(tr.get_vocab(), ref.get_vocab())


def test_substring_counts_reruns_and_chunks(monkeypatch):
    texts = uc.distinct_corpus()
    assert len(texts) == 60 and all(len(t.encode()) == 90 for t in texts)
    ref = RefUnigramTrainer(vocab_size=1 << 40)
    ref.train_from_iterator(texts)
    # nearly every substring is distinct: more than the table's first size (half the candidates)
    cands = sum(len(s) * 16 - 120 for s in ref.sentences)
    assert len(ref.substring_counts) > 0.9 * cands
    tr = UnigramTrainer(vocab_size=1 << 40)
    tr.train_from_iterator(texts)
    st = tr.stats()
    assert st["chunks"] == 1 and st["rerun_chunks"] == 1 and tr.substring_counts() == ref.substring_counts
    # 6 texts a chunk: 10 chunks, every one counted again at 8192 slots, the cap
    monkeypatch.setenv("CTOK_TRAIN_CHUNK_BYTES", "540")
    monkeypatch.setenv("CTOK_TRAIN_COUNT_SLOTS", "8192")
    tr.train_from_iterator(texts)
    st = tr.stats()
    assert st["chunks"] == 10 and st["rerun_chunks"] == 10 and st["table_capacity"] == 8192
    assert tr.substring_counts() == ref.substring_counts and tr.sentences() == ref.sentences
    uc.same_vocab(tr.get_vocab(), ref.get_vocab())
    tr.train_sentences(ref.sentences)  # sentences given directly go through the same chunks
    assert tr.stats()["chunks"] > 1 and tr.substring_counts() == ref.substring_counts
    # no capacity within the cap: an error, and the vocab stays
    before = tr.get_vocab()
    monkeypatch.setenv("CTOK_TRAIN_COUNT_SLOTS", "1024")
    with pytest.raises(RuntimeError, match="overflows"):
        tr.train_from_iterator(texts)
    uc.same_vocab(tr.get_vocab(), before)


# ---- 4. trainings -----------------------------------------------------------------------------------

HELD_OUT = ["hello world", "aab ab", "", "é中 a", "the quick brown fox", "▁", "aaaa bbbb", "zzz"]


def _training_same(texts, sentences=None, **cfg):
    ref = RefUnigramTrainer(**cfg)
    rm = ref.train_sentences(sentences) if sentences is not None else ref.train_from_iterator(texts)
    tr = UnigramTrainer(**cfg)
    m = tr.train_sentences(sentences) if sentences is not None else tr.train_from_iterator(texts)
    _trained_same(tr, m, ref, rm)
    return tr, m, ref


def _trained_same(tr, m, ref, rm):
    assert tr.sentences() == ref.sentences
    st = tr.stats()
    assert st["iterations"] == ref.iterations and st["vocab_sizes"] == ref.sizes
    assert tr.expected_counts() == {t: int(c) for t, c in ref.expected_counts.items()}
    uc.same_vocab(tr.get_vocab(), ref.get_vocab())
    uc.same_vocab(m.get_vocab(), ref.get_vocab())
    assert tr.vocab_size == len(ref.vocab) and m.vocab_size == rm.vocab_size()
    assert m.encode_batch(HELD_OUT) == [rm.encode(t) for t in HELD_OUT]


def test_training_c1_defaults():
    docs = _c1()
    tr, m, ref = _training_same(docs[:300], vocab_size=500)
    assert ref.iterations == 16 and ref.sizes[0] == 67601
    assert sum(1 for _, s in tr.get_vocab() if s == -INF) > 0
    one = RefUnigramTrainer(vocab_size=500, n_iterations=1)
    one.train_from_iterator(docs[:300])
    assert sum(1 for _, s in one.vocab if s == -INF) == 66781  # mostly -inf after the first M-step
    held = docs[300:340]
    rm = RefUnigramModel(ref.get_vocab())
    assert m.encode_batch(held) == [rm.encode(t) for t in held]


@pytest.mark.parametrize("vocab_size", [5, 10, 40])
@pytest.mark.parametrize("length", [1, 2, 4, 16])
def test_training_aab(vocab_size, length):
    _training_same(uc.aab(), vocab_size=vocab_size, max_piece_length=length)


def test_training_unicode():
    _, _, ref = _training_same(uc.unicode_corpus(), vocab_size=30)
    assert ref.iterations > 3
    _training_same(uc.unicode_corpus(), vocab_size=12, max_piece_length=3, shrinking_factor=0.6)


def test_training_quirk_configurations():
    for name, texts, cfg in uc.quirk_configs():
        try:
            _training_same(texts, **cfg)
        except AssertionError as e:
            raise AssertionError(name + ": " + str(e)) from e


def test_training_twice_and_sentences_given():
    tr = UnigramTrainer(vocab_size=12)
    ref = RefUnigramTrainer(vocab_size=12)
    for texts in (uc.aab()[:50], uc.unicode_corpus()[:50], uc.aab()[:50]):
        _trained_same(tr, tr.train_from_iterator(texts), ref, ref.train_from_iterator(texts))
    # sentences given directly: no normaliser, no split (a space and a tab are chars like any other)
    sentences = ["a b\tc", "▁ab", "", "éé", "a b\tc"]
    _, _, ref = _training_same(None, sentences=sentences, vocab_size=6)
    assert ref.sentences == sentences and "\t" in "".join(ref.substring_counts)


def test_train_files_crlf_and_no_final_newline(tmp_path):
    p, q = tmp_path / "a.txt", tmp_path / "b.txt"
    p.write_bytes("aab ab\r\nab\tba\r\n\r\nbaab aab".encode())
    q.write_bytes("é中 ab\nab\n".encode())
    ref = RefUnigramTrainer(vocab_size=8)
    rm = ref.train([str(p), str(q)])
    assert ref.sentences == ["▁aab▁ab", "▁ab", "ba", "▁", "▁baab▁aab", "▁é中▁ab", "▁ab"]
    tr = UnigramTrainer(vocab_size=8)
    _trained_same(tr, tr.train([str(p), str(q)]), ref, rm)


# ---- 5. the panic -----------------------------------------------------------------------------------

def test_the_panic_example():
    cfg, texts = uc.PANIC["cfg"], uc.PANIC["texts"]
    with pytest.raises(RefPanic):
        RefUnigramTrainer(**cfg).train_from_iterator(texts)
    tr = UnigramTrainer(**cfg)
    with pytest.raises(PanicException, match="trainers.rs"):
        tr.train_from_iterator(texts)
    assert tr.get_vocab() == [] and tr.vocab_size == 0
    # after a training: the previous vocab stays, and the trainer still trains
    ref = RefUnigramTrainer(**cfg)
    ok = ["ab ab", "ba"]
    rm = ref.train_from_iterator(ok)
    _trained_same(tr, tr.train_from_iterator(ok), ref, rm)
    before = tr.get_vocab()
    with pytest.raises(PanicException):
        tr.train_from_iterator(texts)
    uc.same_vocab(tr.get_vocab(), before)
    _trained_same(tr, tr.train_from_iterator(ok), ref, ref.train_from_iterator(ok))
