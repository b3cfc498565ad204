"""Corpora, models and configurations that the Unigram tests share (tests/test_unigram_ref_cpu.py,
tests/test_unigram_cpu.py, tests/test_gpu_unigram.py).  Everything is seeded."""
import random
import struct

from tests.unigram_ref import RefUnigramModel

INF = float("inf")
NAN = float("nan")
ALPHA = ["a", "b", "c", "▁", "é", "中", "\U0001F600"]

# the trainer's panic (ISSUE, re-derived by tests/test_unigram_ref_cpu.py): initial_vocab_size drops
# a char while "<unk>" is kept with count 0
PANIC = dict(texts=["z", "cxcxx  b"], cfg=dict(vocab_size=5, max_piece_length=4, shrinking_factor=0.9, initial_vocab_size=15))


def texts_over(seed, n, alpha, lo=1, hi=40):
    rng = random.Random(seed)
    return ["".join(rng.choice(alpha) for _ in range(rng.randint(lo, hi))) for _ in range(n)]


def aab():
    return texts_over(3, 500, "aab ")


def unicode_corpus():  # 1-4-byte chars; NFC composes e + U+0301; a tab and U+3000 cut sentences
    alpha = ["e\u0301", "\u00e9", "中", "文", "\U0001F600", "a", "b", " ", " ", "ñ", "▁", "\t", "\u3000"]
    return texts_over(4, 300, alpha, 0, 40)


def distinct_corpus():  # nearly every substring occurs once: the count table's first size overflows
    rng = random.Random(9)
    chars = [chr(c) for c in range(0x4E00, 0x4E00 + 3000)]
    return ["".join(rng.choice(chars) for _ in range(30)) for _ in range(60)]


# the quirk configurations: (name, texts, trainer arguments)
def quirk_configs():
    a = aab()[:120]
    return [
        ("special_is_substring", a, dict(vocab_size=10, special_tokens=["<unk>", "aa", "b"])),
        ("repeated_special", a, dict(vocab_size=10, special_tokens=["<unk>", "<s>", "<s>", "ab"])),
        ("empty_special", a, dict(vocab_size=10, special_tokens=["", "<unk>"])),
        ("no_unk", a, dict(vocab_size=10, special_tokens=["<s>"])),
        ("no_specials", a, dict(vocab_size=10, special_tokens=[])),
        ("piece_1", a, dict(vocab_size=2, max_piece_length=1)),
        ("piece_3_shorter_than_unk", a, dict(vocab_size=10, max_piece_length=3)),
        ("shrink_0.5", a, dict(vocab_size=10, shrinking_factor=0.5)),
        ("shrink_1.5", a, dict(vocab_size=10, shrinking_factor=1.5, n_iterations=3)),
        ("shrink_nan", a, dict(vocab_size=10, shrinking_factor=NAN)),
        ("shrink_negative", a, dict(vocab_size=10, shrinking_factor=-1)),
        ("no_iterations", a, dict(vocab_size=10, n_iterations=0)),
        ("vocab_size_0", a, dict(vocab_size=0)),
        ("small_initial", a, dict(vocab_size=6, initial_vocab_size=40)),
        ("initial_0", a, dict(vocab_size=6, initial_vocab_size=0)),
        ("no_texts", [], dict(vocab_size=1)),
        ("empty_texts", ["", "", ""], dict(vocab_size=1)),
    ]


def bits(x: float) -> bytes:
    return struct.pack("<d", x)


def same_vocab(got, want):
    """[(token, score)] equal with every score compared bit for bit (NaN and -0.0 included)"""
    assert [t for t, _ in got] == [t for t, _ in want]
    bad = [i for i in range(len(want)) if bits(got[i][1]) != bits(want[i][1])]
    assert not bad, (len(bad), got[bad[0]], want[bad[0]], got[bad[0]][1].hex(), want[bad[0]][1].hex())


def hand_vocab():
    """tokens of 1 to 5 chars over ALPHA with exactly representable scores"""
    toks = ["<unk>", "a", "b", "c", "▁", "é", "中", "\U0001F600", "ab", "bc", "▁a", "é中",
            "中\U0001F600a", "abc", "abca", "é中\U0001F600▁", "abé中c", "\U0001F600\U0001F600\U0001F600\U0001F600\U0001F600"]
    return [(t, -1.0 - 0.5 * len(t) - 0.25 * (i % 3)) for i, t in enumerate(toks)]


def random_model(rng, kind):
    """a small model over ALPHA; kind: 'ties' (scores -1.0 / -2.0), 'special' (NaN, +-inf among them),
    'repeat' (repeated strings), 'random' (any finite f64 in a range)"""
    n = rng.randint(1, 14)
    toks = []
    for _ in range(n):
        toks.append("".join(rng.choice(ALPHA) for _ in range(rng.choice([1, 1, 1, 2, 2, 3, 4, 5]))))
    if kind == "repeat":
        toks += [rng.choice(toks) for _ in range(rng.randint(1, 4))]
        rng.shuffle(toks)
    if rng.random() < 0.5:
        toks.insert(rng.randrange(len(toks) + 1), "<unk>")
    if rng.random() < 0.1:
        toks.append("")
    scores = []
    for _ in toks:
        if kind == "ties":
            scores.append(rng.choice([-1.0, -2.0]))
        elif kind == "special" and rng.random() < 0.3:
            scores.append(rng.choice([NAN, -INF, INF, 0.0, -0.0]))
        else:
            scores.append(-rng.random() * 12.0)
    return list(zip(toks, scores))


def random_text(rng, lo=0, hi=24, extra="xyzñ"):
    alpha = ALPHA * 3 + list(extra)
    return "".join(rng.choice(alpha) for _ in range(rng.randint(lo, hi)))


def ref_encode(vocab, texts, unk="<unk>"):
    m = RefUnigramModel(vocab, unk)
    return [m.encode(t) for t in texts]
