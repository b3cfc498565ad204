"""GPU parity of complexity_tokenizer.WordPieceTrainer and WordPieceModel (csrc/lowercase.hip,
csrc/wordpiece.hip) against the restatement of the reference's src/trainers.rs and src/models.rs
(tests/wordpiece_ref.py): Lowercase, the word counts through NFC and Lowercase, whole trainings merge
by merge with the words' final tokens and the resident pair table, the reference's quirks and stops,
the conventions, rebuilds, long words, and the model's encode.  Exact equality everywhere.  Every
corpus goes through the restatement first and the properties a test relies on are asserted there."""
import random

import numpy as np
import pytest

from complexity_tokenizer import WordPieceModel, WordPieceTrainer
from complexity_tokenizer.wordpiece import lowercase
from datagen import corpus
from tests.bpe_trainer_ref import WHITE_SPACE, split_whitespace
from tests.wordpiece_ref import RefWordPieceModel, RefWordPieceTrainer

pytestmark = pytest.mark.gpu

_cache = {}
SCALARS = [c for c in range(0x110000) if not 0xD800 <= c < 0xE000]
SPAN = 64  # csrc/wordpiece_internal.h kLowerSpan


def _texts(seed, n, alpha, lo=1, hi=40):
    rng = random.Random(seed)
    return ["".join(rng.choice(alpha) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def _corpus(name):
    if name == "c1":
        text, off = corpus.corpus_c1()
        return [d.decode() for d in corpus.unpack(text, off)][:600], dict(vocab_size=400, min_frequency=2)
    if name == "aab":
        return _texts(3, 500, "aab "), dict(vocab_size=120, min_frequency=1)
    if name == "unicode":  # NFC composes e + U+0301, Lowercase folds the capitals
        alpha = ["e\u0301", "\u00e9", "\u00c9", "\u4e2d", "\u6587", "\U0001F600", "a", "A", " ", "\u00f1", "\u03a3", "\u0130"]
        return _texts(4, 400, alpha, 1, 12), dict(vocab_size=200, min_frequency=1)
    raise KeyError(name)


def _ref(name, **kw):
    """The restatement's training of a named corpus (run once per module and configuration)."""
    texts, base = _corpus(name)
    cfg = dict(base, **kw)
    key = (name, tuple(sorted(cfg.items(), key=str)))
    if key not in _cache:
        ref = RefWordPieceTrainer(**cfg)
        ref.model = ref.train_from_iterator(texts)
        _cache[key] = ref
    return texts, cfg, _cache[key]


def _same(tr, model, ref):
    """merges in order, vocab, every word's final tokens, the pair table, the model handed back"""
    merges = tr.merges()
    if merges != ref.merges:
        n = min(len(merges), len(ref.merges))
        k = next((i for i in range(n) if merges[i] != ref.merges[i]), n)
        raise AssertionError("first differing merge %d: gpu %r, oracle %r (of %d / %d)"
                             % (k, merges[k:k + 1], ref.merges[k:k + 1], len(merges), len(ref.merges)))
    assert tr.get_vocab() == ref.vocab and tr.vocab_size == len(ref.vocab)
    assert tr.tokens() == ref.tokens
    assert model.get_vocab() == ref.vocab
    if tr.stats()["table_capacity"]:
        assert tr.pair_counts() == ref.final_pairs


def _train_words(words, **cfg):
    ref = RefWordPieceTrainer(**cfg)
    ref.model = ref.train_words(words)
    tr = WordPieceTrainer(**cfg)
    model = tr.train_words(words)
    _same(tr, model, ref)
    return tr, model, ref


# ---- 1. Lowercase -----------------------------------------------------------------------------------

def _lower_same(texts):
    got = lowercase(texts)
    want = [t.lower() for t in texts]
    bad = [i for i in range(len(texts)) if got[i] != want[i]]
    assert not bad, (len(bad), texts[bad[0]], got[bad[0]], want[bad[0]])


def test_lowercase_length_changes_across_spans():
    changing = [c for c in SCALARS if len(chr(c).lower().encode()) != len(chr(c).encode())]
    assert len(changing) == 25
    texts = []
    for c in changing:
        ch = chr(c)
        n = len(ch.encode())
        # the code point ends before, on, across and after the span boundary; last in its text
        texts += ["a" * (SPAN - n + k) + ch for k in range(-1, n + 1)]
        texts += ["a" * (SPAN - 1) + ch + "B" * 70 + ch, ch, ch * 100]
    _lower_same(texts)
    _lower_same(["".join(chr(c) for c in changing) * 9])  # all of them in one text, offsets drifting both ways


def test_lowercase_sigma_contexts():
    ign = "\u0301"
    texts = ["\u03a3", "\u0391\u03a3", "\u0391.\u03a3", "\u0391\u03a3a", "\u03a3\u0391"]
    for k in range(SPAN - 6, SPAN + 3):  # the sigma and its context on both sides of the span boundary
        texts += ["b" * k + "a\u03a3", "b" * k + "a" + ign * 3 + "\u03a3" + ign * 2, "b" * k + "a\u03a3" + ign * 3 + "c",
                  " " * k + "\u03a3" + ign, "b" * k + "\u03a3\u03a3\u03a3"]
    texts += ["a" + ign * 5000 + "\u03a3", "a" + ign * 5000 + "\u03a3" + ign * 5000 + "x", "." * 5000 + "\u03a3"]
    _lower_same(texts)
    # the context does not cross a text boundary, wherever the boundary falls in a span
    for k in (0, 1, SPAN - 3, SPAN - 2, SPAN * 3 - 2):
        batch = ["c" * k + "\u0391\u03a3", "\u0391", "", "\u03a3", "a" + ign, "\u03a3b"]
        assert lowercase(batch) == ["c" * k + "\u03b1\u03c2", "\u03b1", "", "\u03c3", "a" + ign, "\u03c3b"]


def test_lowercase_empty_unchanged_and_every_mapping():
    assert lowercase([]) == [] and lowercase([""]) == [""] and lowercase(["", "", ""]) == ["", "", ""]
    _lower_same(["", "A", "", "", "b" * 200, ""])
    _lower_same(["plain ascii, already lower case. " * 20, "\u00e9\u4e2d\U0001F600 no capitals"])
    changing = [c for c in SCALARS if chr(c).lower() != chr(c)]
    assert len(changing) == 1393
    _lower_same([chr(c) for c in changing])
    _lower_same(["".join(chr(c) for c in changing[i::7]) for i in range(7)])
    rng = random.Random(5)
    pool = changing + list(range(0x20, 0x7F)) * 4 + [0x3A3, 0x301, 0x2E] * 50
    _lower_same(["".join(chr(rng.choice(pool)) for _ in range(rng.randrange(0, 90))) for _ in range(400)])


def test_unchanged_text_is_not_copied():
    tr = WordPieceTrainer()
    assert tr.word_counts(["all lower case ascii", "and \u00e9 too"]) == {"all": 1, "lower": 1, "case": 1, "ascii": 1, "and": 1,
                                                                        "\u00e9": 1, "too": 1}
    assert tr.stats()["lowered_chunks"] == 0 and tr.stats()["chunks"] == 1
    assert tr.word_counts(["One capital"]) == {"one": 1, "capital": 1}
    assert tr.stats()["lowered_chunks"] == 1


# ---- 2. word counts ---------------------------------------------------------------------------------

def _count_batches():
    from tests.test_gpu_bpe_trainer import _COUNT_BATCHES, _count_batch
    return {name: _count_batch(name) for name in _COUNT_BATCHES}


def test_word_counts_nfc_then_lower():
    tr = WordPieceTrainer()
    assert tr.word_counts(["Hello hello HELLO"]) == {"hello": 3}
    assert tr.word_counts(["E\u0301", "\u0130", "e\u0301 \u00c9"]) == {"\u00e9": 3, "i\u0307": 1}
    assert tr.word_counts(["\u0391\u03a3", "\u0391", "\u03a3 \u0391\u03a3\u0391"]) == {"\u03b1\u03c2": 1, "\u03b1": 1, "\u03c3": 1,
                                                                              "\u03b1\u03c3\u03b1": 1}
    assert tr.word_counts([]) == {} and tr.word_counts(["", " "]) == {}


@pytest.mark.parametrize("name", ["all 25 spaces", "not spaces", "empty texts", "one word per text",
                                  "a word over bytes 31/32", "a code point over bytes 31/32", "a space over bytes 31/32",
                                  "a 70,000-byte word", "natural text"])
def test_word_counts_of_the_bpe_trainers_batches(name):
    texts = _count_batches()[name]
    want = RefWordPieceTrainer().word_counts(texts)
    if name == "one word per text":
        assert want == {"ab": 2, "cd": 1, "\u00e9": 2}  # NFC: the two spellings of e-acute are one word
    assert WordPieceTrainer().word_counts(texts) == want


def test_word_counts_in_chunks_and_on_the_host_walk(monkeypatch):
    texts = [t.upper() if i % 3 == 0 else t for i, ts in enumerate(_count_batches().values()) for t in ts]
    want = RefWordPieceTrainer().word_counts(texts)
    tr = WordPieceTrainer()
    assert tr.word_counts(texts) == want and tr.stats()["chunks"] == 1
    monkeypatch.setenv("CTOK_TRAIN_CHUNK_BYTES", "40000")
    assert tr.word_counts(texts) == want
    st = tr.stats()
    assert st["chunks"] >= 3 and st["host_chunks"] == 0 and 1 <= st["lowered_chunks"] <= st["chunks"]
    monkeypatch.delenv("CTOK_TRAIN_CHUNK_BYTES")
    assert len(want) > 64
    monkeypatch.setenv("CTOK_TRAIN_COUNT_SLOTS", "64")  # the table overflows: the host walks the lower-cased text
    assert tr.word_counts(texts) == want and tr.stats()["host_chunks"] == 1


# ---- 3. whole trainings -----------------------------------------------------------------------------

def test_training_c1():
    texts, cfg, ref = _ref("c1")
    assert len(ref.merges) > 200 and ref.tie_merges and ref.stopped_on == "vocab_size"
    assert any(w != w.lower() for t in texts for w in t.split())  # Lowercase has work to do
    tr = WordPieceTrainer(**cfg)
    model = tr.train_from_iterator(texts)
    _same(tr, model, ref)
    st = tr.stats()
    assert st["merges"] == len(ref.merges) and st["unique_words"] == len(ref.word_freqs)
    assert st["words"] == sum(ref.word_freqs.values()) and tr.vocab_size == 400
    # far fewer words are walked than the reference tokenises (every word in every round)
    print("walked", st["walked_words"], "of", len(ref.word_freqs) * len(ref.merges))
    assert 0 < st["walked_words"] < len(ref.word_freqs) * len(ref.merges) // 4
    # encode of every training word = the trainer's final tokens, where all of them are keys
    words = [w for w in ref.tokens if all(t in ref.vocab for t in ref.tokens[w]) and len(w) <= 100]
    assert len(words) > len(ref.tokens) // 2
    assert model.encode_batch(words) == [[ref.vocab[t] for t in ref.tokens[w]] for w in words]
    assert model.encode_batch(words) == [ref.model.encode(w) for w in words]


def test_training_overlapping_runs():
    texts, cfg, ref = _ref("aab")
    assert ("a", "##a") in ref.merges and len(ref.merges) > 50
    tr = WordPieceTrainer(**cfg)
    _same(tr, tr.train_from_iterator(texts), ref)


def test_training_multi_byte_alphabet():
    texts, cfg, ref = _ref("unicode")
    assert "\u00e9" in ref.vocab and "\u0301" not in ref.vocab and "A" not in ref.vocab and "\u03c2" in ref.vocab
    assert "i" in ref.vocab and "\u0307" in ref.vocab and len(ref.merges) > 50
    tr = WordPieceTrainer(**cfg)
    _same(tr, tr.train_from_iterator(texts), ref)


@pytest.mark.parametrize("prefix", ["##", "#", "", "\u00e9"])
def test_training_prefixes(prefix):
    texts, cfg, ref = _ref("aab", continuing_subword_prefix=prefix, vocab_size=60)
    assert len(ref.merges) > 30
    tr = WordPieceTrainer(**cfg)
    model = tr.train_from_iterator(texts)
    _same(tr, model, ref)
    assert model.encode_batch(texts[:50]) == [ref.model.encode(t) for t in texts[:50]]


@pytest.mark.parametrize("specials", [["[UNK]", "ab", "##a"], ["x", "[UNK]", "x"], ["a", "##", "##b", "aab"], []],
                         ids=["inside words", "repeated", "a char, the prefix, prefix + char", "none"])
def test_training_specials(specials):
    texts, cfg, ref = _ref("aab", special_tokens=tuple(specials), vocab_size=50)
    assert ref.merges
    if specials[:1] == ["x"]:
        assert ref.vocab["x"] == 2 and 0 not in ref.vocab.values()  # overwritten, and next_id moved on
    cfg = dict(cfg, special_tokens=list(specials))
    tr = WordPieceTrainer(**cfg)
    _same(tr, tr.train_from_iterator(texts), ref)


def _prefix_words(seed):
    rng = random.Random(seed)
    words = {}
    for _ in range(30):
        w = "".join(rng.choice("ab#") for _ in range(rng.randint(1, 7)))
        words[w] = rng.randint(1, 9)
    return words


@pytest.mark.parametrize("special", [False, True], ids=["prefix no special", "prefix a special"])
@pytest.mark.parametrize("prefix,seed", [("#", 1), ("#", 2), ("#", 5), ("##", 2), ("##", 5), ("##", 7)])
def test_training_words_that_contain_the_prefix(prefix, seed, special):
    """Words made of the prefix's own chars: a round's merged string can be prefix + one char, the very
    string later chars already hold as their fallback token.  From then on it is a key: those
    positions take its vocab id as key, and its pairs are counted under one symbol."""
    specials = ["[UNK]"] + ([prefix] if special else [])
    tr, _, ref = _train_words(_prefix_words(seed), vocab_size=40, min_frequency=1, special_tokens=specials,
                              continuing_subword_prefix=prefix)
    made = [a + b[len(prefix):] for a, b in ref.merges]
    assert any(m.startswith(prefix) and len(m) == len(prefix) + 1 for m in made)
    assert any(w.startswith(prefix) for w in ref.word_freqs) and len(ref.merges) > 30


def test_prefix_plus_char_becomes_a_key():
    words = {"#ab": 5, "xab": 4, "#ac": 3, "yac": 3, "xad": 6}
    tr, _, ref = _train_words(words, vocab_size=30, min_frequency=1, special_tokens=[], continuing_subword_prefix="#")
    # ("#", "#a") makes "#a" a key; "yac" holds it behind its first char and "#ac" at its start:
    # ("#a", "#c") has 3 + 3 = 6 under one symbol, before ("#a", "#b") with 5
    assert ref.merges[:5] == [("x", "#a"), ("#", "#a"), ("xa", "#d"), ("#a", "#c"), ("#a", "#b")]
    assert ref.best_counts[3] == 6 and tr.merges()[3] == ("#a", "#c")
    # one merge later the table holds the pair once, under the key's symbol
    tr, _, ref = _train_words(words, vocab_size=len(ref.vocab) - len(ref.merges) + 2, min_frequency=1, special_tokens=[],
                              continuing_subword_prefix="#")
    assert ref.final_pairs[("#a", "#c")] == 6 and tr.pair_counts()[("#a", "#c")] == 6


def test_min_frequency_drops_words():
    texts, cfg, ref = _ref("aab", min_frequency=4, vocab_size=40)
    counts = RefWordPieceTrainer().word_counts(texts)
    assert 0 < len(ref.word_freqs) < len(counts) and min(ref.word_freqs.values()) >= 4
    tr = WordPieceTrainer(**cfg)
    _same(tr, tr.train_from_iterator(texts), ref)


def test_stops():
    # vocab_size below the initial vocab: the chars are in, nothing is merged
    tr, model, ref = _train_words({"ab": 2, "b\u00e9": 3}, vocab_size=2, min_frequency=1)
    assert ref.merges == [] and model.vocab_size == 8 and tr.stats()["table_capacity"] == 0
    # no pairs left
    tr, model, ref = _train_words({"ab": 3, "ac": 2, "zz": 1}, vocab_size=100, min_frequency=2, special_tokens=["[UNK]"])
    assert ref.stopped_on == "no_pairs" and tr.merges() == [("a", "##b"), ("a", "##c")]
    assert model.get_vocab() == {"[UNK]": 0, "a": 1, "b": 2, "c": 3, "ab": 4, "ac": 5}
    # no words at all, and only words of one char
    _train_words({}, vocab_size=10, min_frequency=1)
    tr, model, ref = _train_words({"a": 5, "b": 1}, vocab_size=10, min_frequency=1, special_tokens=[])
    assert ref.stopped_on == "no_pairs" and model.get_vocab() == {"a": 0, "b": 1}


def test_forced_ties():
    tr, _, ref = _train_words({"ab": 2, "ad": 2}, vocab_size=5, min_frequency=1, special_tokens=["##d"])
    assert ref.tie_merges == [0] and tr.merges() == [("a", "##d")]  # key(##d) = 0 < key(##b) = 2^31 + 'b'
    tr, _, ref = _train_words({"ba": 2, "ab": 2, "cc": 2}, vocab_size=20, min_frequency=1, special_tokens=[])
    assert ref.tie_merges[:2] == [0, 1] and tr.merges()[0] == ("a", "##b")
    words = {w: 3 for w in _texts(11, 40, "abcd", 2, 5)}
    _, _, ref = _train_words(words, vocab_size=30, min_frequency=1)
    assert len(ref.tie_merges) >= 3


def test_second_training_on_one_trainer():
    """The vocab is never cleared and ids start at 0 again: the second training's ids collide with the
    first one's, and the colliding strings' keys spill (include/ctok_wordpiece.h)."""
    cfg = dict(vocab_size=22, min_frequency=1, special_tokens=["[UNK]"])
    ref, tr = RefWordPieceTrainer(**cfg), WordPieceTrainer(**cfg)
    first = {"abab": 3, "abc": 2, "cab": 2}
    ref.train_words(first)
    assert ref.stopped_on == "no_pairs"
    _same(tr, tr.train_words(first), ref)
    n_first = len(ref.vocab)
    second = {"dcab": 2, "dab": 4, "ed": 3, "abde": 2}
    model = ref.train_words(second)
    assert len(ref.vocab) > n_first and len(set(ref.vocab.values())) < len(ref.vocab)  # ids collide
    assert ref.merges and any(k >= (1 << 31) + 0x110000 for k in ref._key.values())    # a key spilled
    got = tr.train_words(second)
    _same(tr, got, ref)
    ids = sorted(set(ref.vocab.values()))
    assert [got.id_to_token(i) for i in ids] == [model.id_to_token(i) for i in ids]
    assert got.decode(ids) == model.decode(ids)


def test_long_words():
    rng = random.Random(7)
    words = {"ab" * 4096: 1, "z" * 70000: 2}
    while len(words) < 52:
        words.setdefault("".join(rng.choice("abc") for _ in range(rng.randint(2, 8))), rng.randint(1, 50))
    tr, model, ref = _train_words(words, vocab_size=5 + 4 + 8, min_frequency=1)
    assert len(ref.merges) == 8 and ("##z", "##z") in ref.merges and len(ref.tokens["ab" * 4096]) < 8192
    assert model.encode("z" * 70000 + " ab") == ref.model.encode("z" * 70000 + " ab")  # over max_input_chars: unk


def test_train_files(tmp_path):
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    a.write_bytes("Hello World\r\nhello there\r\n\r\nWORLD peace".encode())
    b.write_bytes("e\u0301te\u0301 \u00c9T\u00c9\nhello\rworld\r\n".encode())
    cfg = dict(vocab_size=60, min_frequency=1)
    ref = RefWordPieceTrainer(**cfg)
    ref.train([str(a), str(b)])
    assert ref.word_freqs["hello"] == 3 and ref.word_freqs["\u00e9t\u00e9"] == 2 and "world" in ref.word_freqs
    tr = WordPieceTrainer(**cfg)
    _same(tr, tr.train([str(a), str(b)]), ref)
    with pytest.raises(IOError):
        tr.train([str(a), str(tmp_path / "missing.txt")])


# ---- 4. the resident state --------------------------------------------------------------------------

def test_default_equals_recount_every_round(monkeypatch):
    texts, cfg, ref = _ref("c1")
    tr = WordPieceTrainer(**cfg)
    model = tr.train_from_iterator(texts)
    assert tr.stats()["rebuilds"] < len(ref.merges) // 10
    monkeypatch.setenv("CTOK_WP_TRAIN_RECOUNT", "1")
    again = WordPieceTrainer(**cfg)
    model2 = again.train_from_iterator(texts)
    assert again.merges() == tr.merges() and model2.get_vocab() == model.get_vocab() and again.tokens() == tr.tokens()
    st = again.stats()
    assert st["rebuilds"] >= len(ref.merges) - 1 and st["walked_words"] == len(ref.word_freqs) * len(ref.merges)
    _same(again, model2, ref)


@pytest.mark.parametrize("k", [1, 2, 5])
def test_pair_table_is_exact_after_k_merges(k):
    texts = _corpus("aab")[0]
    words = RefWordPieceTrainer().word_counts(texts)
    base = RefWordPieceTrainer(vocab_size=0, min_frequency=1)
    base.train_words(words)
    cfg = dict(vocab_size=len(base.vocab) + k, min_frequency=1)
    tr, _, ref = _train_words(words, **cfg)
    assert len(ref.merges) == k and ref.final_pairs and tr.pair_counts() == ref.final_pairs
    assert tr.stats()["rebuilds"] == 0  # updated in place, not counted again


def test_capped_table_rebuilds_and_gives_the_same_result(monkeypatch):
    texts, cfg, ref = _ref("c1")
    slots = max(ref.live_pairs) + 8
    assert ref.live_pairs[0] > 300 and len(ref.seen_pairs) > slots
    monkeypatch.setenv("CTOK_BPE_TRAIN_SLOTS", str(slots))
    tr = WordPieceTrainer(**cfg)
    _same(tr, tr.train_from_iterator(texts), ref)
    st = tr.stats()
    assert st["rebuilds"] >= 1 and st["table_capacity"] == slots


def test_table_cap_below_the_live_pairs_is_an_error_not_a_loop(monkeypatch):
    texts, cfg, ref = _ref("c1")
    monkeypatch.setenv("CTOK_BPE_TRAIN_SLOTS", str(ref.live_pairs[0] // 2))
    tr = WordPieceTrainer(**cfg)
    with pytest.raises(ValueError, match="CTOK_BPE_TRAIN_SLOTS"):
        tr.train_from_iterator(texts)
    # the failed call leaves the trainer as it was: no vocab, no merges, no tokens
    assert tr.vocab_size == 0 and tr.get_vocab() == {} and tr.merges() == [] and tr.tokens() == {} and tr.pair_counts() == {}
    monkeypatch.delenv("CTOK_BPE_TRAIN_SLOTS")
    _same(tr, tr.train_from_iterator(texts), ref)  # the same trainer, as if the failed call had not been
    # a failure in a second training keeps the first one's vocab
    tr = WordPieceTrainer(vocab_size=60, min_frequency=1)
    first = tr.train_words({"ab": 3, "abc": 2}).get_vocab()
    with pytest.raises(ValueError, match="u32"):
        tr.train_words({"qr": 0xFFFFFFFF, "qrs": 2})
    assert tr.get_vocab() == first and "q" not in first and tr.merges() == []


def test_best_count_of_2_to_the_32_is_refused():
    with pytest.raises(ValueError, match="u32"):
        RefWordPieceTrainer(vocab_size=50).train_words({"ab": 0xFFFFFFFF, "abc": 2})
    with pytest.raises(ValueError, match="u32"):
        WordPieceTrainer(vocab_size=50).train_words({"ab": 0xFFFFFFFF, "abc": 2})
    _, _, ref = _train_words({"ab": 0xFFFFFFFD, "abc": 2}, vocab_size=50, min_frequency=1)
    assert ref.best_counts[0] == 0xFFFFFFFF


# ---- 5. the model -----------------------------------------------------------------------------------

def _models(vocab, *args):
    return WordPieceModel(vocab, *args), RefWordPieceModel(vocab, *args)


def _encode_same(m, r, texts):
    want = [r.encode(t) for t in texts]
    assert m.encode_batch(texts) == want
    ids, off = m.encode_batch_flat(texts)
    assert ids.dtype == np.uint32 and off.tolist() == np.cumsum([0] + [len(w) for w in want]).tolist()
    return want


def test_model_known_answers():
    m, r = _models({"[UNK]": 0, "hello": 1, "world": 2, "##ing": 3, "play": 4, "##ed": 5})
    assert m.encode("hello world") == [1, 2] and m.decode([1, 2]) == "hello world"
    m, r = _models({"[UNK]": 0, "play": 1, "##ing": 2, "##ed": 3})
    assert m.encode("playing") == [1, 2] and m.decode([1, 2]) == "playing"
    # unk moves on one char and does not give up the word; without unk in the vocab nothing is pushed
    assert m.encode("xplaying") == [0] * 5 + [2] and m.encode("playxing") == [1, 0, 2]
    _encode_same(m, r, ["xplaying", "playxing played", "ing", "##ing", "pla", "playeding x"])
    m, r = _models({"play": 1, "##ing": 2})
    assert m.encode("playxing zz") == [1, 2]
    _encode_same(m, r, ["playxing zz", "zz", "", "playing"])
    m, r = _models({"[UNK]": 0, "play": 1, "##ing": 2}, "##", "play")  # another unk token
    assert m.encode("xplay") == [1, 1, 1, 1, 1] == r.encode("xplay")


def test_model_max_input_chars_per_word():
    vocab = {"[UNK]": 0, "a": 1, "##a": 2, "\u00e9": 3, "##\u00e9": 4, "\U0001F600": 5, "##\U0001F600": 6}
    m, r = _models(vocab)
    texts = ["a" * 100, "a" * 101, "\u00e9" * 100, "\u00e9" * 101, "\U0001F600" * 100, "\U0001F600" * 101,
             "a" * 99 + "\u00e9", "a" * 100 + "\u00e9", "a" * 101 + " " + "a" * 100 + "\u3000" + "\u00e9" * 101]
    want = _encode_same(m, r, texts)
    assert len(want[0]) == 100 and want[1] == [0] and len(want[4]) == 100 and want[5] == [0]
    m, r = _models({"a": 1, "##a": 2}, "##", "[UNK]", 3)  # no unk: a long word gives nothing
    assert _encode_same(m, r, ["aaa aaaa aa"]) == [[1, 2, 2, 1, 2]]
    m, r = _models(vocab, "##", "[UNK]", 0)
    assert _encode_same(m, r, ["a aa"]) == [[0, 0]]


def test_model_boundaries_and_long_patterns():
    vocab = {"[UNK]": 0}
    for i, t in enumerate(["a", "##a", "ab", "##ab", "##b", "\u00e9", "##\u00e9", "##\u4e2d", "a\u00e9\u4e2d", "##b\u00e9",
                           "abababababab", "##abababababababab", "x" * 40, "##" + "y" * 70]):
        vocab[t] = i + 1
    m, r = _models(vocab)
    texts = []
    for k in list(range(58, 68)) + list(range(250, 260)):  # words and code points across bytes 64 and 256
        texts += ["a" * (k % 7) + " " + "ab" * 3 + " " * (k - 8 - k % 7) + "ab\u00e9\u4e2dab\u00e9 a\u00e9\u4e2d",
                  " " * k + "abababababababab", "b" * (k - 60 if k < 70 else k - 200) + "\u00e9" * 40]
    texts += ["abababababa", "ababababababa", "x" * 39, "x" * 41, "a" + "y" * 69, "a" + "y" * 70 + "b", "ab" * 50]
    _encode_same(m, r, texts)


def test_model_spaces_and_empty_texts():
    m, r = _models({"[UNK]": 0, "a": 1, "b": 2, "##b": 3, "end": 4})
    spaces = sorted(WHITE_SPACE)
    texts = ["", " ", "".join(spaces), "", "a" + "".join(spaces) + "b"] + ["a" + s + "ab" for s in spaces] + \
            ["".join(spaces) + "end", "a\x1cb", "a\u200bb", ""]
    want = _encode_same(m, r, texts)
    assert want[0] == want[1] == want[2] == [] and want[4] == [1, 2] and want[5] == [1, 1, 3]
    assert m.encode_batch([]) == [] and m.encode_batch(["", ""]) == [[], []]
    assert [m.encode(t) for t in texts] == want  # encode is a batch of one


def test_model_on_a_trained_vocab_and_decode_round_trips():
    texts, cfg, ref = _ref("c1")
    m = WordPieceModel(ref.vocab)
    docs = [t.lower() for t in texts[:150]] + texts[150:200]
    want = _encode_same(m, ref.model, docs)
    assert any(ref.vocab["[UNK]"] in w for w in want)  # capitals are not in the vocab: the model has no normaliser
    for t, ids in zip(docs[:150], want[:150]):
        assert m.decode(ids) == ref.model.decode(ids)
        if ref.vocab["[UNK]"] not in ids:
            assert m.decode(ids) == " ".join(split_whitespace(t))
