"""GPU parity of complexity_tokenizer.WordLevelModel, CharBpeModel and ByteLevelBpeModel
(csrc/strmerge.hip) against the restatement of the reference's src/models.rs:300-741
(tests/models_ref.py): the hand-worked cases, the three merge tiers at their boundaries, the cap on
a word's symbols, text boundaries, the splits, foreign chars, random merge lists and the trainer's
output.  Exact equality everywhere.  Every case goes through the restatement first and the
property a case relies on is asserted there."""
import os
import random

import numpy as np
import pytest

from complexity_tokenizer import BpeTrainer, ByteLevelBpeModel, CharBpeModel, UnsupportedConfigError, WordLevelModel
from complexity_tokenizer.models import models_limits
from datagen import corpus
from tests.bpe_trainer_ref import WHITE_SPACE
from tests.models_ref import RefByteLevelBpeModel, RefCharBpeModel, RefWordLevelModel, bytes_to_unicode

pytestmark = pytest.mark.gpu

B2U = bytes_to_unicode()
G = B2U[0x20]
LIMITS = models_limits()
T1, T2 = LIMITS["tier1"], LIMITS["tier2"]
TIER_LENGTHS = [T1 - 1, T1, T1 + 1, T2 - 1, T2, T2 + 1, 3 * T2 + 1]


def _pair(kind, vocab, *args, **kw):
    """(the model on the GPU, its restatement)"""
    gpu, ref = {"wl": (WordLevelModel, RefWordLevelModel), "char": (CharBpeModel, RefCharBpeModel),
                "byte": (ByteLevelBpeModel, RefByteLevelBpeModel)}[kind]
    return gpu(vocab, *args, **kw), ref(vocab, *args, **kw)


def _same(m, ref, texts):
    """ids and offsets of the batch, whole, against the restatement; -> the restatement's ids"""
    want = ref.encode_batch(texts)
    ids, off = m.encode_batch_flat(texts)
    want_off = np.cumsum([0] + [len(w) for w in want]).astype(np.uint64)
    assert off.dtype == np.uint64 and off.tolist() == want_off.tolist()
    assert ids.tolist() == [i for w in want for i in w]
    return want


def _merges(rng, alpha, n, shuffle=False, dup=0):
    """n merges whose parts are drawn from the alphabet and earlier results; in creation order the
    list is proper (a result ranks behind its parts), shuffled it is not; dup pairs given again"""
    pool, merges = list(alpha), []
    for _ in range(n):
        a, b = rng.choice(pool), rng.choice(pool)
        merges.append((a, b))
        pool.append(a + b)
    if shuffle:
        rng.shuffle(merges)
    for _ in range(dup):
        merges.insert(rng.randrange(len(merges) + 1), rng.choice(merges))
    return merges


def _vocab(alpha, merges, drop=5):
    """ids for the alphabet, the parts and the results, every drop-th string left out"""
    strings = sorted(set(alpha) | {x for m in merges for x in m} | {a + b for a, b in merges})
    v = {"<unk>": 0}
    v.update({s: i + 1 for i, s in enumerate(strings) if i % drop})
    return v


# ---- 1. the hand-worked cases ----------------------------------------------------------------------

HAND = [
    ({"<unk>": 0, "a": 1, "b": 2, "ab": 3, "aba": 4}, [("ab", "a"), ("a", "b")], ["abab"], [[4, 2]]),
    ({"<unk>": 0, "a": 1, "aa": 2}, [("a", "a")], ["aaa", "aaaa"], [[2, 1], [2, 2]]),
    ({"<unk>": 0, "a": 1, "b": 2, "c": 3, "ab": 4, "bc": 5}, [("a", "b"), ("b", "c"), ("a", "b")], ["abc"], [[1, 5]]),
    ({"<unk>": 0, "abc": 5}, [("a", "b"), ("ab", "c")], ["abc", "ab", "ba"], [[5], [0], [0, 0]]),
    ({"a": 3, "zero": 0}, [], ["aq"], [[3, 0]]),
]


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_worked(case):
    vocab, merges, texts, want = HAND[case]
    unk = "[UNK]" if case == 4 else "<unk>"  # (case 4: an unk token that is not in the vocab is id 0)
    for kind, args in (("char", (merges, "", unk)), ("byte", (merges, unk, False))):
        m, ref = _pair(kind, vocab, *args)
        assert ref.encode_batch(texts) == want
        _same(m, ref, texts)
        assert [m.encode(t) for t in texts] == want


def test_prefix_space_suffix_and_lookups():
    vocab = {"<unk>": 0, G: 1, G + "a": 2, "a": 3, "b": 4}
    m, ref = _pair("byte", vocab, [(G, "a")])
    texts = ["", "a", "a  b", " a", "\u00e9"]
    assert ref.encode_batch(texts) == [[1], [2], [2, 1, 1, 4], [2], [1, 0, 0]]
    _same(m, ref, texts)
    assert m.vocab_size == 5 and m.token_to_id(G + "a") == 2 and m.id_to_token(2) == G + "a" and m.id_to_token(9) is None
    assert m.get_vocab() == vocab
    vocab = {"<unk>": 0, "a": 1, "a</w>": 2, "aa</w>": 3, "b": 4}
    m, ref = _pair("char", vocab, [("a", "a</w>")])
    texts = ["a", "aa", "aaa b"]
    assert ref.encode_batch(texts) == [[2], [3], [1, 3, 0]]  # a one-char word is char + suffix
    _same(m, ref, texts)
    m, ref = _pair("char", vocab, [("a", "a")], "")
    assert ref.encode("aab") == [0, 4]
    _same(m, ref, ["aab", "a", "aa b"])


def test_decode():
    vocab = {"<unk>": 0, "a</w>": 1, "b": 2, "\u3000</w>": 3, "\x1f</w>": 4, "B": 2}
    m, ref = _pair("char", vocab, [])
    for ids in ([2, 1, 2, 1], [1, 3], [1, 4], [9, 2], []):
        assert m.decode(ids) == ref.decode(ids)
    assert m.decode([1, 3]) == "a" and m.decode([1, 4]) == "a \x1f" and m.id_to_token(2) == "B"
    m, ref = _pair("char", {"a": 1, "b": 2}, [], "")
    assert m.decode([1, 2]) == ref.decode([1, 2]) == "a b"
    m, ref = _pair("wl", {"x": 1, "y": 2, "w": 2})
    assert m.decode([2, 7, 1]) == ref.decode([2, 7, 1]) == "w x"
    vocab = {G + "a": 1, B2U[0xE2] + B2U[0x82]: 2, "\u4e2d": 3, B2U[0x80]: 4, B2U[0xE0] + B2U[0x80]: 5, B2U[0xF5]: 6}
    m, ref = _pair("byte", vocab, [])
    for ids in ([1, 2], [3, 1], [4], [5], [6], [2, 4, 1]):
        assert m.decode(ids) == ref.decode(ids)
    assert m.decode([1, 2]) == " a\ufffd" and m.decode([5]) == "\ufffd\ufffd" and m.decode([6]) == "\ufffd"


# ---- 2. the tiers ------------------------------------------------------------------------------------

def _tier_words(alpha, pad, bytes_per_symbol):
    """one word per tier length, of exactly that many symbols"""
    rng = random.Random(7)
    words = []
    for n in TIER_LENGTHS:
        w = "".join(rng.choice(alpha) for _ in range(n // bytes_per_symbol))
        words.append(w + pad * (n - bytes_per_symbol * len(w)))
    return words


@pytest.mark.parametrize("shuffle", [False, True], ids=["proper", "shuffled"])
@pytest.mark.parametrize("alpha", ["ab", "\u4e2d\u6587"], ids=["ascii", "3byte"])
def test_tiers_char(alpha, shuffle):
    merges = _merges(random.Random(21), alpha, 40, shuffle, dup=3 if shuffle else 0)
    m, ref = _pair("char", _vocab(alpha, merges), merges, "")
    words = _tier_words(alpha, alpha[0], 1)
    assert [len(w) for w in words] == TIER_LENGTHS
    want = _same(m, ref, words)
    assert all(len(w) < n for w, n in zip(want, TIER_LENGTHS))  # merges happened in every tier
    _same(m, ref, [" ".join(words)])  # all tiers in one text
    s, r = _pair("char", _vocab(alpha, merges), [(a, b + "</w>") if i % 3 == 0 else (a, b) for i, (a, b) in enumerate(merges)])
    _same(s, r, words)


@pytest.mark.parametrize("shuffle", [False, True], ids=["proper", "shuffled"])
@pytest.mark.parametrize("multi", [False, True], ids=["ascii", "3byte"])
def test_tiers_byte(multi, shuffle):
    alpha = [B2U[b] for b in "\u4e2d".encode()] + ["a"] if multi else ["a", "b"]
    merges = _merges(random.Random(22), alpha, 40, shuffle, dup=3 if shuffle else 0)
    first = [(alpha[0], alpha[1]), (alpha[0] + alpha[1], alpha[2])] if multi else []  # (pairs the words do hold)
    merges = merges + first if shuffle else first + merges
    vocab = _vocab(alpha, merges)
    m, ref = _pair("byte", vocab, merges, add_prefix_space=False)
    words = _tier_words("\u4e2d", "a", 3) if multi else _tier_words("ab", "a", 1)
    assert [len(w.encode()) for w in words] == TIER_LENGTHS  # symbols are bytes
    want = _same(m, ref, words)
    assert all(len(w) < n for w, n in zip(want, TIER_LENGTHS))
    # the virtual leading space counts as a symbol: one byte fewer is the same tier length
    merges = merges + [(G, "a"), (G + "a", "a")]
    p, pref = _pair("byte", _vocab(alpha + [G], merges), merges, add_prefix_space=True)
    texts = [w[1:] + ("aa" if len(w[0].encode()) == 3 else "") for w in words]
    assert [len(pref.words(t)[0].encode()) for t in texts] == TIER_LENGTHS
    _same(p, pref, texts)


def test_word_above_a_lowered_cap():
    alpha = "ab"
    merges = _merges(random.Random(23), alpha, 20)
    vocab = _vocab(alpha, merges)
    texts = ["ab" * 20, "a" * 101, "ba ab"]
    old = os.environ.get("CTOK_MODELS_MAX_WORD_SYMBOLS")
    os.environ["CTOK_MODELS_MAX_WORD_SYMBOLS"] = "100"
    try:
        assert models_limits()["max_word_symbols"] == 100
        for kind, args in (("char", (merges, "")), ("byte", (merges, "<unk>", False))):
            m, ref = _pair(kind, vocab, *args)
            with pytest.raises(UnsupportedConfigError, match="101 symbols"):
                m.encode_batch(texts)
            _same(m, ref, [texts[0], texts[2]])              # the same call without the word
            _same(m, ref, [texts[0], "a" * 100, texts[2]])  # (and with a word at the lowered cap)
        os.environ["CTOK_MODELS_MAX_WORD_SYMBOLS"] = str(1 << 40)  # nothing raises the cap
        assert models_limits()["max_word_symbols"] == LIMITS["max_word_symbols"]
    finally:
        if old is None:
            del os.environ["CTOK_MODELS_MAX_WORD_SYMBOLS"]
        else:
            os.environ["CTOK_MODELS_MAX_WORD_SYMBOLS"] = old


# ---- 3. text boundaries ------------------------------------------------------------------------------

def test_text_boundaries():
    alpha = "ab"
    merges = [("a", "b"), ("b", "a"), ("ab", "ab"), ("ba", "a"), ("b", "b")]
    vocab = _vocab(alpha, merges, drop=100)
    batches = [
        ["ab", "ab", "ba", "b", "b", "a"],         # no whitespace at either end: a word must not cross
        ["", "", "ab", "", "b", "", "", "", "ab ab", ""],
        ["", "", ""],
        [""],
        [],
        ["b" * 31, "a" * 33, "", "ab" * 40],       # boundaries that are no bitmap-word boundaries
    ]
    models = [_pair("char", vocab, merges, ""), _pair("char", vocab, merges), _pair("byte", vocab, merges),
              _pair("byte", vocab, merges, add_prefix_space=False), _pair("wl", vocab)]
    for m, ref in models:
        assert ref.encode_batch(["ab", "ab"]) == [ref.encode("ab")] * 2
        for texts in batches:
            _same(m, ref, texts)
    m, ref = models[0]
    assert ref.encode("abab") != ref.encode("ab") * 2  # (so the first batch tells a crossing word)
    m, ref = models[2]
    assert ref.encode_batch(["", ""]) == [[vocab.get(G, 0)]] * 2  # an empty text is the word " "


# ---- 4. the splits -----------------------------------------------------------------------------------

def test_white_space_splits():
    merges = [("a", "b"), ("b", "a"), ("ab", "a")]
    vocab = _vocab("ab", merges, drop=100)
    vocab.update({"ab\x1cab": 50, "ab": 51})
    ws = sorted(WHITE_SPACE)
    texts = ["ab%sab" % c for c in ws] + ["%sab%s%sba%s" % (c, c, c, c) for c in ws] + ["".join(ws), "ab" + "".join(ws) + "ab"]
    stay = ["ab%sab" % c for c in "\x1c\x1d\x1e\x1f\u200b"]
    for m, ref in (_pair("char", vocab, merges, ""), _pair("char", vocab, merges), _pair("wl", vocab)):
        assert all(len(ref.encode(t)) == 2 * len(ref.encode("ab")) for t in texts[:25])
        assert "ab\x1cab".split() == ["ab", "ab"] and ref.encode("ab\x1cab") != ref.encode("ab ab")
        _same(m, ref, texts + stay)


def test_byte_level_splits():
    alpha = ["a", "b", G, B2U[0x09], B2U[0x0A], B2U[0xC2], B2U[0xA0]]
    merges = [(G, "a"), (G, G), ("a", B2U[0x09]), (B2U[0x09], "b"), (B2U[0xC2], B2U[0xA0]), ("a", B2U[0x0A]), (G + "a", "b")]
    vocab = _vocab(alpha, merges, drop=100)
    texts = ["a  b", "   ", " a", "a ", "  a  ", "a\tb", "a\nb a", "a\u00a0b", "\u00a0", "\tb", "a   b    ab", " ", "ab"]
    for prefix in (True, False):
        m, ref = _pair("byte", vocab, merges, add_prefix_space=prefix)
        assert ref.words("a\tb\nc\u00a0d") == [(" " if prefix else "") + "a\tb\nc\u00a0d"]
        assert ref.words("a  b")[-2:] == [" ", " b"]
        _same(m, ref, texts)
    assert _pair("byte", vocab, merges)[1].encode(" a") == _pair("byte", vocab, merges)[1].encode("a")


# ---- 5. the word-level model -------------------------------------------------------------------------

def test_word_level():
    vocab = {"<unk>": 7, "hello": 1, "he": 0xFFFF, "\U0001F600\U0001F600": 0x10000, "\u4e2d": 0xFFFFFFFF, "": 9, "a b": 10}
    m, ref = _pair("wl", vocab)
    texts = ["hello he", "hell", "helloo", "h", "x" * 100, "\U0001F600\U0001F600 \U0001F600", "\u4e2d\u4e2d \u4e2d", "a b",
             "hello\u3000he\thello", ""]
    want = _same(m, ref, texts)
    assert want[:5] == [[1, 0xFFFF], [7], [7], [7], [7]] and want[5] == [0x10000, 7] and want[6] == [7, 0xFFFFFFFF]
    e, eref = _pair("wl", {})
    assert eref.encode("a b") == [0, 0]
    _same(e, eref, ["a b", "", "hello"])
    assert e.vocab_size == 0 and m.vocab_size == 7 and m.decode([1, 0xFFFF]) == "hello he"
    u, uref = _pair("wl", vocab, "[UNK]")
    assert uref.encode("q") == [0]
    _same(u, uref, texts)


# ---- 6. foreign chars --------------------------------------------------------------------------------

def test_foreign_chars():
    merges = [("x", "y"), ("a", "a")]
    vocab = {"<unk>": 0, "a": 1, "aa": 2, "xy": 3, "y": 4}
    texts = ["qq", "qqq aqqa", "\u4e2d\u4e2d", "x", "xy", "yx", "xyxy", "qxyq", "\U0001F600\U0001F600a"]
    m, ref = _pair("char", vocab, merges, "")
    want = _same(m, ref, texts)
    assert want[0] == [0, 0] and want[2] == [0, 0] and want[3] == [0] and want[4] == [3] and want[5] == [4, 0]
    m, ref = _pair("char", vocab, merges)  # every last char is foreign under the suffix
    _same(m, ref, texts)
    m, ref = _pair("byte", vocab, merges, add_prefix_space=False)
    want = _same(m, ref, texts)
    assert want[0] == [0, 0] and want[2] == [0] * 6 and want[4] == [3]


# ---- 7. random parity --------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(5))
def test_random_parity(seed):
    rng = random.Random(100 + seed)
    alpha = "abcd\u00e9\u4e2d"
    texts = ["".join(rng.choice(alpha + " ") for _ in range(rng.randint(0, 40))) for _ in range(2000)]
    merges = _merges(rng, alpha, 60, shuffle=True, dup=6)
    vocab = _vocab(alpha, merges, drop=4)
    for suffix in ("", "</w>"):
        ms = [(a, b + suffix) if suffix and i % 2 else (a, b) for i, (a, b) in enumerate(merges)]
        _same(*_pair("char", vocab, ms, suffix), texts)
    balpha = sorted({B2U[b] for b in alpha.encode()}) + [G]
    bmerges = _merges(rng, balpha, 80, shuffle=True, dup=6)
    for prefix in (True, False):
        _same(*_pair("byte", _vocab(balpha, bmerges, drop=4), bmerges, add_prefix_space=prefix), texts)
    words = sorted({w for t in texts for w in t.split(" ") if w})
    wvocab = {w: i for i, w in enumerate(rng.sample(words, len(words) // 2))}
    _same(*_pair("wl", wvocab, words[0]), texts)


# ---- 8. with the trainer -----------------------------------------------------------------------------

def test_with_the_trainer():
    text, off = corpus.corpus_c1()
    docs = [d.decode() for d in corpus.unpack(text, off)][:600]
    vocab, merges = BpeTrainer(vocab_size=300, min_frequency=1).train(docs)
    assert len(merges) > 50
    _same(*_pair("char", vocab, merges, ""), docs)
    _same(*_pair("byte", vocab, merges), docs)


def test_calls_agree_and_models_do_not_disturb_each_other():
    merges = _merges(random.Random(31), "ab", 10)
    vocab = _vocab("ab", merges, drop=100)
    a, aref = _pair("char", vocab, merges, "")
    b, bref = _pair("byte", vocab, merges[:3])
    texts = ["abba ab", "", "b" * 50, "ab"]
    for _ in range(2):
        ia, oa = a.encode_batch_flat(texts)
        ib, ob = b.encode_batch_flat(texts)
        assert a.encode_batch(texts) == aref.encode_batch(texts) == [a.encode(t) for t in texts]
        assert b.encode_batch(texts) == bref.encode_batch(texts) == [b.encode(t) for t in texts]
        assert [ia[int(oa[i]):int(oa[i + 1])].tolist() for i in range(len(texts))] == aref.encode_batch(texts)
        assert [ib[int(ob[i]):int(ob[i + 1])].tolist() for i in range(len(texts))] == bref.encode_batch(texts)
    with pytest.raises(TypeError):
        a.encode(5)
