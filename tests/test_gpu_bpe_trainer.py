"""GPU parity of the classic BPE trainer (complexity_tokenizer.BpeTrainer, csrc/bpe_train.hip) against
the restatement of the reference's src/bpe_trainer.rs (tests/bpe_trainer_ref.py): the White_Space
split and the word counts, whole trainings merge by merge, the reference's quirks and stops, the two
tie conventions, the exactness of the pair table that stays on the device, its rebuilds, a long word
and the u32 overflow guard.  Every corpus goes through the restatement first and the properties a
test relies on (number of merges, a tie, a stop) are asserted on its output."""
import random

import pytest

from complexity_tokenizer import BpeTrainer
from datagen import corpus
from tests.bpe_trainer_ref import WHITE_SPACE, RefBpeTrainer

pytestmark = pytest.mark.gpu

_cache = {}


def _texts(seed, n, alpha, lo=1, hi=40):
    rng = random.Random(seed)
    return ["".join(rng.choice(alpha) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def _corpus(name):
    if name == "c1":
        text, off = corpus.corpus_c1()
        return [d.decode() for d in corpus.unpack(text, off)][:600], dict(vocab_size=400, min_frequency=2)
    if name == "aab":
        return _texts(3, 500, "aab "), dict(vocab_size=120, min_frequency=1)
    if name == "unicode":  # decomposed and composed e-acute stay distinct: no NFC here
        alpha = ["e\u0301", "\u00e9", "\u4e2d", "\u6587", "\U0001F600", "a", " ", "\u00f1", "\u00df"]
        return _texts(4, 400, alpha, 1, 12), dict(vocab_size=200, min_frequency=1)
    raise KeyError(name)


def _ref(name, **kw):
    """The restatement's training of a named corpus (run once per module and configuration)."""
    texts, base = _corpus(name)
    cfg = dict(base, **kw)
    key = (name, tuple(sorted(cfg.items(), key=str)))
    if key not in _cache:
        ref = RefBpeTrainer(**cfg)
        ref.train(texts)
        _cache[key] = ref
    return texts, cfg, _cache[key]


def _same(got, ref):
    vocab, merges = got
    if merges != ref.merges:
        n = min(len(merges), len(ref.merges))
        k = next((i for i in range(n) if merges[i] != ref.merges[i]), n)
        raise AssertionError("first differing merge %d: gpu %r, oracle %r (of %d / %d)"
                             % (k, merges[k:k + 1], ref.merges[k:k + 1], len(merges), len(ref.merges)))
    assert vocab == ref.vocab


# ---- 1. split and count ---------------------------------------------------------------------------

_SPACES = sorted(WHITE_SPACE)
_BIG = "z" * 70000  # longer than the count table's clipped length (0xFFFF)
_COUNT_BATCHES = {
    "all 25 spaces": ["a" + s + "b" for s in _SPACES] + ["x" + "".join(_SPACES) + "y", "".join(_SPACES) + "end"],
    "not spaces": ["a\x1cb", "c\x1d\x1e\x1fd a\x1cb", "e\u200bf"],
    "empty texts": ["", "", "a", "", " ", ""],
    "one word per text": ["ab", "cd", "ab", "\u00e9", "e\u0301"],
    "a word over bytes 31/32": ["a" * 29 + " " + "bcdef g"],
    "a code point over bytes 31/32": ["a" * 29 + " b\u00e9c \u4e2d"],
    "a space over bytes 31/32": ["a" * 30 + "\u3000" + "b", "a" * 31 + "\u00a0" + "b"],
    "a 70,000-byte word": [_BIG, "q " + _BIG + " q", _BIG[:-1], "z" * 65535 + " " + "z" * 65536],
    "natural text": None,
}


def _count_batch(name):
    return _corpus("c1")[0][:200] if name == "natural text" else _COUNT_BATCHES[name]


@pytest.mark.parametrize("name", list(_COUNT_BATCHES))
def test_word_counts(name):
    texts = _count_batch(name)
    want = RefBpeTrainer().build_word_frequencies(texts)
    if name == "one word per text":
        assert want == {"ab": 2, "cd": 1, "\u00e9": 1, "e\u0301": 1}  # words end at text boundaries: never "abcd"
    if name == "not spaces":
        assert want == {"a\x1cb": 2, "c\x1d\x1e\x1fd": 1, "e\u200bf": 1}
    assert BpeTrainer().word_counts(texts) == want


def test_word_counts_in_chunks(monkeypatch):
    texts = [t for name in _COUNT_BATCHES for t in _count_batch(name)]
    want = RefBpeTrainer().build_word_frequencies(texts)
    tr = BpeTrainer()
    assert tr.word_counts(texts) == want and tr.stats()["chunks"] == 1
    monkeypatch.setenv("CTOK_TRAIN_CHUNK_BYTES", "40000")
    assert tr.word_counts(texts) == want
    st = tr.stats()
    assert st["chunks"] >= 3 and st["host_chunks"] == 0


def test_word_counts_table_overflow_falls_back_to_the_host_walk(monkeypatch):
    texts = [t for name in _COUNT_BATCHES for t in _count_batch(name)]
    want = RefBpeTrainer().build_word_frequencies(texts)
    assert len(want) > 64
    monkeypatch.setenv("CTOK_TRAIN_COUNT_SLOTS", "64")
    tr = BpeTrainer()
    assert tr.word_counts(texts) == want
    assert tr.stats()["host_chunks"] == 1


# ---- 2. whole trainings ---------------------------------------------------------------------------

def test_training_c1():
    texts, cfg, ref = _ref("c1")
    assert len(ref.merges) > 50 and ref.tie_merges
    tr = BpeTrainer(**cfg)
    _same(tr.train(texts), ref)
    st = tr.stats()
    assert st["merges"] == len(ref.merges) and st["unique_words"] == len(ref.word_freqs)
    assert st["words"] == sum(ref.word_freqs.values())
    assert tr.vocab_size == 400 and tr.min_frequency == 2


def test_training_overlapping_runs():
    texts, cfg, ref = _ref("aab")
    assert ("a", "a") in ref.merges and len(ref.merges) > 50
    _same(BpeTrainer(**cfg).train(texts), ref)


def test_training_multi_byte_alphabet():
    texts, cfg, ref = _ref("unicode")
    assert "e" in ref.vocab and "\u0301" in ref.vocab and "\u00e9" in ref.vocab and len(ref.merges) > 50
    _same(BpeTrainer(**cfg).train(texts), ref)


@pytest.mark.parametrize("kw", [dict(end_of_word_suffix="</w>"), dict(continuing_subword_prefix="##"),
                                dict(end_of_word_suffix="</w>", continuing_subword_prefix="##"),
                                dict(end_of_word_suffix="\u00e9", continuing_subword_prefix="a")],
                         ids=["suffix", "prefix", "both", "both, colliding with the alphabet"])
def test_training_suffix_and_prefix(kw):
    for name in ("c1", "aab"):
        texts, cfg, ref = _ref(name, **kw)
        assert len(ref.merges) > 50
        if "end_of_word_suffix" in kw:
            # (with a prefix too the suffix's chars after its first are prefixed: look for its last char)
            assert any(kw["end_of_word_suffix"][-1] in t for t in ref.vocab)
        if "continuing_subword_prefix" in kw:
            assert any(a.startswith(kw["continuing_subword_prefix"]) for a, _ in ref.merges)
        _same(BpeTrainer(**cfg).train(texts), ref)


def test_default_arguments_are_the_references():
    texts = _corpus("c1")[0][:50]
    ref = RefBpeTrainer()
    ref.train(texts)
    assert [ref.vocab[t] for t in ("<unk>", "<pad>", "<s>", "</s>")] == [0, 1, 2, 3]
    tr = BpeTrainer()
    _same(tr.train(texts), ref)
    assert tr.vocab_size == 30000 and tr.min_frequency == 2


# ---- 3. quirks and stops --------------------------------------------------------------------------

def test_duplicate_special_and_merged_string_already_in_the_vocab():
    texts = ["ab ab ab abc abc ab", "abd ab cab"] * 5
    cfg = dict(vocab_size=12, min_frequency=1, special_tokens=["ab", "<pad>", "ab"])
    ref = RefBpeTrainer(**cfg)
    ref.train(texts)
    assert ref.initial_vocab_size == 6  # ab, <pad>, a, b, c, d: the repeated special did not grow it
    assert ref.merges[0] == ("a", "b") and len(ref.merges) > 2
    assert len(ref.vocab) == ref.initial_vocab_size + len(ref.merges) - 1  # no growth on the first merge
    _same(BpeTrainer(**cfg).train(texts), ref)


def test_vocab_size_at_or_below_the_initial_vocab():
    texts = _corpus("aab")[0]
    for vs in (0, 3, 6):
        ref = RefBpeTrainer(vocab_size=vs, min_frequency=1)
        ref.train(texts)
        assert ref.merges == [] and len(ref.vocab) == 6
        _same(BpeTrainer(vocab_size=vs, min_frequency=1).train(texts), ref)


def test_min_frequency_at_and_above_the_best_count():
    texts = _corpus("aab")[0]
    top = _ref("aab")[2].best_counts[0]
    for mf, n in ((top + 1, 0), (top, 1)):
        ref = RefBpeTrainer(vocab_size=7, min_frequency=mf)
        ref.train(texts)
        assert len(ref.merges) == n
        _same(BpeTrainer(vocab_size=7, min_frequency=mf).train(texts), ref)


def test_min_frequency_zero_and_training_until_no_pair_is_left():
    texts = _corpus("c1")[0][:20]
    for mf in (0, 1):
        ref = RefBpeTrainer(vocab_size=10 ** 9, min_frequency=mf)
        ref.train(texts)
        assert ref.stopped_on == "no_pairs" and len(ref.merges) > 20
        assert all(len(s) == 1 for s in ref.splits.values())
        _same(BpeTrainer(vocab_size=10 ** 9, min_frequency=mf).train(texts), ref)


@pytest.mark.parametrize("texts", [[], [""], ["", ""], [" \n\t", "\u3000\u00a0", "\u2028"]])
def test_no_words(texts):
    want = {"<unk>": 0, "<pad>": 1, "<s>": 2, "</s>": 3}
    assert RefBpeTrainer(vocab_size=50, min_frequency=1).train(texts) == (want, [])
    tr = BpeTrainer(vocab_size=50, min_frequency=1)
    assert tr.train(texts) == (want, [])
    assert tr.pair_counts() == {} and tr.stats()["unique_words"] == 0


def test_word_of_frequency_zero():
    words = {"ab": 0, "cd": 3, "abcd": 0}
    ref = RefBpeTrainer(vocab_size=50, min_frequency=0, special_tokens=[])
    ref.train_words(words)
    assert ref.merges == [("c", "d")] and ref.splits["abcd"] == ["a", "b", "cd"]
    tr = BpeTrainer(vocab_size=50, min_frequency=0, special_tokens=[])
    _same(tr.train_words(words), ref)
    assert tr.pair_counts() == {}


# ---- 4. ties --------------------------------------------------------------------------------------

@pytest.mark.parametrize("words,tie_at", [({"cd": 2, "ab": 2}, 0),
                                          ({"ab": 5, "gh": 2, "cd": 2, "ef": 2}, 1),
                                          ({"ba": 4, "ab": 4, "aab": 1, "bba": 1}, 0)])
def test_ties_follow_the_convention(words, tie_at):
    cfg = dict(vocab_size=40, min_frequency=1, special_tokens=[])
    ref = RefBpeTrainer(**cfg)
    ref.train_words(words)
    assert tie_at in ref.tie_merges
    tr = BpeTrainer(**cfg)
    _same(tr.train_words(words), ref)
    sym = tr.symbols()
    assert sym == sorted(ref.sym_id, key=ref.sym_id.get)  # the ids the convention compares


# ---- 5. exactness of the resident table -------------------------------------------------------------

_RUNS = {"abababab": 3, "aaaaaaa": 2, "xaaay": 1}


@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("case", ["aab", "runs"])
def test_pair_table_is_exact_after_k_merges(case, k):
    if case == "aab":
        texts = _corpus("aab")[0]
        words = RefBpeTrainer().build_word_frequencies(texts)
    else:
        words = _RUNS
    base = RefBpeTrainer(vocab_size=0, min_frequency=1)
    base.train_words(words)
    cfg = dict(vocab_size=base.initial_vocab_size + k, min_frequency=1)
    ref = RefBpeTrainer(**cfg)
    ref.train_words(words)
    assert len(ref.merges) == k
    want = ref.count_pairs()  # a fresh count of the restatement's splits at that point
    assert want and ref.merges[-1] not in want  # (the merged pair's own count ended at 0)
    tr = BpeTrainer(**cfg)
    _same(tr.train_words(words), ref)
    assert tr.pair_counts() == want
    if case == "runs":  # (11 pairs in all: nothing outgrows the smallest table)
        assert tr.stats()["rebuilds"] == 0  # the table was updated in place, not counted again


def test_resident_table_equals_recount_before_every_merge(monkeypatch):
    texts, cfg, ref = _ref("c1")
    tr = BpeTrainer(**cfg)
    got = tr.train(texts)
    assert tr.stats()["rebuilds"] < len(ref.merges) // 10
    monkeypatch.setenv("CTOK_BPE_TRAIN_RECOUNT", "1")
    again = BpeTrainer(**cfg)
    assert again.train(texts) == got
    assert again.stats()["rebuilds"] >= len(ref.merges) - 1
    _same(got, ref)


# ---- 6. rebuilds ----------------------------------------------------------------------------------

def test_capped_table_rebuilds_and_gives_the_same_result(monkeypatch):
    """The cap just above the most live pairs any merge chooses from (they grow from the initial
    count on, so a cap just above the initial count would be below the live pairs later): every
    count fits, and the slots of dead pairs run out, so the table is counted again."""
    texts, cfg, ref = _ref("c1")
    slots = max(ref.live_pairs) + 8
    assert ref.live_pairs[0] > 500 and len(ref.seen_pairs) > slots
    monkeypatch.setenv("CTOK_BPE_TRAIN_SLOTS", str(slots))
    tr = BpeTrainer(**cfg)
    _same(tr.train(texts), ref)
    st = tr.stats()
    assert st["rebuilds"] >= 1 and st["table_capacity"] == slots


def test_table_grows_with_the_live_pairs():
    """Two letters: the table starts with 64 slots (4 possible pairs), and the pairs of more than
    100 merged symbols outgrow it."""
    texts, cfg, ref = _ref("aab")
    assert ref.live_pairs[0] <= 4 and max(ref.live_pairs) > 64
    tr = BpeTrainer(**cfg)
    _same(tr.train(texts), ref)
    st = tr.stats()
    # (the capacity never shrinks and holds every live pair; far fewer rebuilds than merges)
    assert st["table_capacity"] >= max(ref.live_pairs) and 1 <= st["rebuilds"] < len(ref.merges) // 2
    assert tr.pair_counts() == ref.count_pairs()


def test_table_cap_below_the_live_pairs_is_an_error_not_a_loop(monkeypatch):
    """CTOK_E_ARG (ValueError): the cap is an argument the training cannot be run with."""
    texts, cfg, ref = _ref("c1")
    monkeypatch.setenv("CTOK_BPE_TRAIN_SLOTS", str(ref.live_pairs[0] // 2))
    with pytest.raises(ValueError, match="CTOK_BPE_TRAIN_SLOTS"):
        BpeTrainer(**cfg).train(texts)
    monkeypatch.setenv("CTOK_BPE_TRAIN_SLOTS", str(max(ref.live_pairs[:10]) + 1))  # enough at first, not later
    assert max(ref.live_pairs) > max(ref.live_pairs[:10]) + 1
    with pytest.raises(ValueError, match="CTOK_BPE_TRAIN_SLOTS"):
        BpeTrainer(**cfg).train(texts)
    monkeypatch.delenv("CTOK_BPE_TRAIN_SLOTS")
    _same(BpeTrainer(**cfg).train(texts), ref)  # nothing is left behind by the failed calls


# ---- 7. long word ---------------------------------------------------------------------------------

def test_long_word_of_repeats():
    rng = random.Random(7)
    words = {"ab" * 4096: 1}
    while len(words) < 51:
        words.setdefault("".join(rng.choice("abc") for _ in range(rng.randint(2, 8))), rng.randint(1, 50))
    cfg = dict(vocab_size=4 + 3 + 14, min_frequency=1)
    ref = RefBpeTrainer(**cfg)
    ref.train_words(words)
    assert len(ref.merges) == 14 and len(ref.splits["ab" * 4096]) < 8192 // 8
    tr = BpeTrainer(**cfg)
    _same(tr.train_words(words), ref)
    assert tr.pair_counts() == ref.count_pairs()


# ---- 8. overflow guard ----------------------------------------------------------------------------

def test_first_best_count_of_2_to_the_32_is_refused():
    with pytest.raises(ValueError, match="u32"):
        RefBpeTrainer(vocab_size=50).train_words({"ab": 0xFFFFFFFF, "abc": 2})
    with pytest.raises(ValueError, match="u32"):
        BpeTrainer(vocab_size=50).train_words({"ab": 0xFFFFFFFF, "abc": 2})
    # one below: 2^32 - 1 fits
    words = {"ab": 0xFFFFFFFD, "abc": 2}
    ref = RefBpeTrainer(vocab_size=50, min_frequency=1)
    ref.train_words(words)
    assert ref.best_counts[0] == 0xFFFFFFFF
    _same(BpeTrainer(vocab_size=50, min_frequency=1).train_words(words), ref)
