"""Self-checks of tests/unigram_ref.py, the Python restatement of the reference's UnigramTrainer
(src/trainers.rs:287-546) and UnigramModel (src/models.rs:150-299) that the GPU tests compare with:
the reference's own known answers, Metaspace, the lattice-then-Viterbi formulation of the kernels
against the literal double loop, the quirk configurations, the panic and where it cannot happen.
No GPU."""
import random

import pytest

from tests import unigram_cases as uc
from tests.unigram_ref import (INF, WHITE_SPACE, PanicException, RefUnigramModel, RefUnigramTrainer, as_usize, lines_of, ln,
                               metaspace, rust_min)


def test_reference_known_answer():
    # test_unigram_trainer, src/trainers.rs:572-589
    t = RefUnigramTrainer(vocab_size=50, initial_vocab_size=100, n_iterations=2)
    m = t.train_from_iterator(["hello world", "hello there", "world peace"])
    assert m.vocab_size() > 0
    assert t.sentences == ["▁hello▁world", "▁hello▁there", "▁world▁peace"]
    assert t.iterations == 2 and t.sizes == [75, 56] and len(t.vocab) == 56
    assert all(s in m.vocab for s in ("<unk>", "<s>", "</s>"))
    # the seed order: count descending, then bytes ascending
    t0 = RefUnigramTrainer(vocab_size=50, initial_vocab_size=100, n_iterations=0)
    t0.train_from_iterator(["hello world", "hello there", "world peace"])
    # e, l and ▁ occur 6 times each, o 4 times
    assert [v for v, _ in t0.vocab[:4]] == ["e", "l", "▁", "o"] and len(t0.vocab) == 100


def test_metaspace():
    assert metaspace("hello world") == ["▁hello▁world"]
    assert metaspace("a\tb") == ["▁a", "b"]
    assert metaspace("") == ["▁"]
    assert metaspace("a▁ b") == ["▁a▁▁b"]
    assert metaspace("\tb") == ["▁", "b"] and metaspace("a\n\n") == ["▁a"]
    assert metaspace("é") == ["▁é"]
    assert len(WHITE_SPACE) == 25 and all(chr(c).isspace() for c in WHITE_SPACE)
    for c in WHITE_SPACE:
        want = ["▁x▁y"] if c == 0x20 else ["▁x", "y"]
        assert metaspace("x" + chr(c) + "y") == want, hex(c)
    assert metaspace("x\u001cy​z") == ["▁x\u001cy​z"]  # Python's isspace / a zero width space: not White_Space
    assert lines_of(b"a b\r\nc\r\n\r\nlast") == ["a b", "c", "", "last"] and lines_of(b"") == []


def test_small_functions():
    assert rust_min(0.0, uc.NAN) == 0.0 and rust_min(-1.0, -INF) == -INF
    assert as_usize(uc.NAN) == 0 and as_usize(-3.0) == 0 and as_usize(7.9) == 7 and as_usize(1e30) == (1 << 64) - 1
    assert ln(0.0) == -INF and ln(1.0) == 0.0
    m = RefUnigramModel([("a", -1.0), ("b", uc.NAN), ("a", -3.0), ("<unk>", -2.0)])
    assert m.vocab_size() == 3 and m.token_to_id("a") == 2 and m.id_to_token(0) == "a" and m.unk_id == 3
    assert m.min_score == -13.0 and m.decode([0, 9, 1, 2]) == "aba"
    assert RefUnigramModel([("a", 1.0)]).unk_id == 0 and RefUnigramModel([("a", 1.0)]).min_score == -10.0


def test_model_tie_and_quirks():
    m = RefUnigramModel([("a", -1.0), ("b", -1.0), ("ab", -2.0), ("<unk>", -5.0)])
    assert m.encode("abab") == [2, 2]  # equal sums: the smallest start
    assert m.encode("xa") == [3, 0] and m.encode("") == []
    # nothing finite reaches a position: id 0 and the ids behind it
    m = RefUnigramModel([("a", -INF), ("b", -1.0), ("c", -1.0)])
    assert m.min_score == -INF and m.encode("bab") == [0] and m.encode("ab") == [0]
    m = RefUnigramModel([("x", -1.0), ("a", uc.NAN), ("b", -1.0)])
    assert m.min_score == -11.0 and m.encode("bab") == [0] and m.encode("bb") == [2, 2] and m.encode("a") == [0]


@pytest.mark.parametrize("kind", ["ties", "special", "repeat", "random"])
def test_lattice_viterbi_equals_the_double_loop(kind):
    rng = random.Random("lattice" + kind)
    used = set()
    for _ in range(60):
        vocab = uc.random_model(rng, kind)
        m = RefUnigramModel(vocab, rng.choice(["<unk>", "<unk>", "a"]))
        for _ in range(6):
            t = uc.random_text(rng)
            want = m.encode(t)
            assert m.encode_lattice(t) == want, (vocab, t)
            used.update(want)
    assert len(used) > 5
    if kind == "repeat":  # the last index of a repeated string is the one in use
        m = RefUnigramModel([("a", -1.0), ("b", -1.0), ("a", -9.0)])
        assert m.encode("ab") == [2, 1] == m.encode_lattice("ab")


def test_quirk_configurations_train():
    for name, texts, cfg in uc.quirk_configs():
        t = RefUnigramTrainer(**cfg)
        m = t.train_from_iterator(texts)
        specials = cfg.get("special_tokens", ["<unk>", "<s>", "</s>"])
        assert all(any(v == s for v, _ in t.vocab) for s in specials), name
        assert [v for v, _ in t.vocab] == [m.id_to_token(i) for i in range(len(t.vocab))], name
        assert len({v for v, _ in t.vocab}) == len(t.vocab), name
        if name == "no_iterations":
            assert t.iterations == 0
        if name == "shrink_1.5":
            assert t.iterations == 3 and t.sizes[0] == t.sizes[2]  # the target is above the size: nothing is dropped
        if name in ("shrink_nan", "shrink_negative"):
            assert t.sizes == [10]
        if name == "vocab_size_0":
            assert t.iterations == 16 and all(a > b for a, b in zip(t.sizes, t.sizes[1:]))
        if name == "piece_1":
            assert all(len(v) == 1 or v in specials for v, _ in t.vocab)
        if name == "initial_0":
            assert t.iterations == 0 and [s for _, s in t.vocab] == [-100.0] * 3
        if name == "empty_texts":
            assert t.sentences == ["▁"] * 3
    # most entries are -inf after the first M-step of a default-sized seed vocab
    t = RefUnigramTrainer(vocab_size=100, n_iterations=1)
    t.train_from_iterator(uc.aab())
    assert sum(1 for _, s in t.vocab if s == -INF) > len(t.vocab) // 2


def test_training_twice_starts_over():
    t = RefUnigramTrainer(vocab_size=12)
    t.train_from_iterator(uc.aab()[:50])
    first = t.get_vocab()
    t.train_from_iterator(uc.unicode_corpus()[:50])
    t.train_from_iterator(uc.aab()[:50])
    uc.same_vocab(t.get_vocab(), first)


def test_the_panic_example_panics():
    t = RefUnigramTrainer(vocab_size=7)
    t.train_from_iterator(["ab ab"])
    before = t.get_vocab()
    t2 = RefUnigramTrainer(**uc.PANIC["cfg"])
    with pytest.raises(PanicException):
        t2.train_from_iterator(uc.PANIC["texts"])
    assert t2.vocab == []
    # why: 'z' falls out of the 15 seed entries while <unk> stays with count 0, so after the first
    # M-step the fallback scores -inf and nothing reaches the end of the sentence "▁z"
    seed = RefUnigramTrainer(**dict(uc.PANIC["cfg"], n_iterations=0))
    seed.train_from_iterator(uc.PANIC["texts"])
    kept = [v for v, _ in seed.vocab]
    assert "z" not in kept[:15] and "<unk>" in kept[:15]
    t.vocab_size_target = 5
    t.max_piece_length, t.shrinking_factor, t.initial_vocab_size = 4, 0.9, 15
    with pytest.raises(PanicException):
        t.train_from_iterator(uc.PANIC["texts"])
    assert t.get_vocab() == before


def test_default_initial_vocab_size_never_panics():
    rng = random.Random(77)
    panics = 0
    for i in range(300):
        texts = ["".join(rng.choice("abcxz  ") for _ in range(rng.randint(0, 9))) for _ in range(rng.randint(1, 4))]
        cfg = dict(vocab_size=rng.randint(0, 12), max_piece_length=rng.randint(1, 6),
                   shrinking_factor=rng.choice([0.5, 0.75, 0.9]), n_iterations=rng.randint(1, 6))
        RefUnigramTrainer(**cfg).train_from_iterator(texts)  # the default initial_vocab_size
        try:
            RefUnigramTrainer(initial_vocab_size=rng.randint(3, 20), **cfg).train_from_iterator(texts)
        except PanicException:
            panics += 1
    assert panics > 0  # (a small initial_vocab_size does panic now and then)
