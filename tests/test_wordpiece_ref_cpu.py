"""The WordPiece oracle (tests/wordpiece_ref.py) checked by itself: the reference's own known answers
(src/models.rs:825-857, src/trainers.rs:552-569), one training worked out by hand, the conventions,
and the argument the GPU trainer rests on -- a word's tokens change only where the round's new string
matches -- against the literal loop that tokenises every word in every round.  Also
tools/wp_table_check.cpp (csrc/wp_table_hd.h on the CPU).  No GPU."""
import os
import random
import subprocess

import pytest

from tests.wordpiece_ref import RefWordPieceModel, RefWordPieceTrainer, pretokenize, read_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wp_table_check(tmp_path):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "wp_table_check.cpp")
    exe = str(tmp_path / "wp_table_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_model_known_answers():
    m = RefWordPieceModel({"[UNK]": 0, "hello": 1, "world": 2, "##ing": 3, "play": 4, "##ed": 5})
    assert m.encode("hello world") == [1, 2] and m.decode([1, 2]) == "hello world"
    m = RefWordPieceModel({"[UNK]": 0, "play": 1, "##ing": 2, "##ed": 3})
    assert m.encode("playing") == [1, 2] and m.decode([1, 2]) == "playing"
    # a start with no match gives unk and moves on one char; it does not give up the word
    assert m.encode("xplaying") == [0] * 5 + [2]  # ("##play" is no key; "##ing" is found at its start)
    assert m.encode("playxing") == [1, 0, 2]
    assert RefWordPieceModel({"play": 1, "##ing": 2}).encode("playxing zz") == [1, 2]
    long = RefWordPieceModel({"[UNK]": 0, "a": 1, "##a": 2}, max_input_chars_per_word=3)
    assert long.encode("aaa aaaa") == [1, 2, 2, 0]
    # among strings that share an id the smallest by UTF-8 bytes is the id's token
    assert RefWordPieceModel({"b": 1, "a": 1, "\u00e9": 1}).id_to_token(1) == "a"


def test_trainer_known_answer():
    t = RefWordPieceTrainer(vocab_size=100, min_frequency=1)
    m = t.train_from_iterator(["hello world", "hello there", "world peace"])
    assert m.vocab_size() > 0 and t.vocab_size == m.vocab_size()
    assert t.stopped_on == "no_pairs"  # 5 words: every one ends as a single token
    assert all(len(v) == 1 for v in t.tokens.values())
    assert m.encode("hello world peace") == [m.token_to_id(w) for w in ("hello", "world", "peace")]


def test_training_by_hand():
    t = RefWordPieceTrainer(vocab_size=10, min_frequency=2, special_tokens=["[UNK]"], literal=True)
    m = t.train_words({"ab": 3, "ac": 2, "zz": 1})
    # "zz" is dropped; [UNK] 0, then a b c in code point order; (a, ##b) has 3, (a, ##c) 2
    assert t.merges == [("a", "##b"), ("a", "##c")] and t.best_counts == [3, 2]
    assert m.vocab == {"[UNK]": 0, "a": 1, "b": 2, "c": 3, "ab": 4, "ac": 5}
    assert t.stopped_on == "no_pairs" and t.tokens == {"ab": ["ab"], "ac": ["ac"]}
    # a tie: the smallest (key(a), key(b)); "##d" as a special gives (a, ##d) the keys (1, 0),
    # before (a, ##b) with (1, 2^31 + 'b')
    t = RefWordPieceTrainer(vocab_size=5, min_frequency=1, special_tokens=["##d"])
    t.train_words({"ab": 2, "ad": 2})
    assert t.merges == [("a", "##d")] and t.tie_merges == [0] and t.stopped_on == "vocab_size"
    assert t.key("##d") == 0 and t.key("##b") == (1 << 31) + ord("b")
    # vocab_size below the initial vocab: nothing is merged, the chars are in all the same
    t = RefWordPieceTrainer(vocab_size=2, min_frequency=1)
    assert t.train_words({"ab": 2}).vocab_size() == 7 and t.merges == []


def test_quirks():
    # a repeated special overwrites its id and next_id still moves on
    t = RefWordPieceTrainer(vocab_size=3, min_frequency=1, special_tokens=["x", "x"])
    assert t.train_words({"a": 1}).vocab == {"x": 1, "a": 2}
    # the vocab is never cleared and ids start at 0 again: a second training collides
    t = RefWordPieceTrainer(vocab_size=8, min_frequency=1, special_tokens=["[UNK]"])
    t.train_words({"ab": 2})
    assert t.vocab == {"[UNK]": 0, "a": 1, "b": 2, "ab": 3}
    m = t.train_words({"cab": 2})
    assert m.vocab["c"] == 1 and m.vocab["a"] == 1 and t.vocab_size == 7
    assert t.merges == [("##a", "##b"), ("c", "##ab")] and m.vocab["##ab"] == 2 and m.vocab["cab"] == 3
    assert t.key("a") == 1 and t.key("c") == (1 << 31) + 0x110000  # "a" < "c" keeps the id as its key
    assert m.id_to_token(1) == "a"
    # pretokenize: NFC, then lower, then the 25 White_Space code points
    assert pretokenize("E\u0301 HELLO\u3000\u0130\x1cX") == ["\u00e9", "hello", "i\u0307\x1cx"]


def test_read_lines(tmp_path):
    p = tmp_path / "f.txt"
    p.write_bytes(b"a b\r\nc\r\r\n\nd")
    assert read_lines(str(p)) == ["a b", "c\r", "", "d"]
    p.write_bytes(b"a\n\xff\n")
    with pytest.raises(IOError):
        read_lines(str(p))
    with pytest.raises(IOError):
        read_lines(str(tmp_path / "missing.txt"))


SPECIALS = [["[UNK]"], [], ["a"], ["ab"], ["b", "ab", "b"], ["[UNK]", "ba", "aab"]]


def seeded_case(seed):
    rng = random.Random(seed)
    alphabet = ["ab", "abc", "a\u00e9", "ab#"][seed % 4]
    prefix = ["##", "#", ""][seed % 3]
    specials = list(SPECIALS[seed % len(SPECIALS)])
    if seed % 5 == 0:
        specials.append(prefix + "a")  # prefix + char as a key
    if seed % 7 == 0 and prefix:
        specials.append(prefix)        # the prefix itself
    if seed % 11 == 0:
        specials.append(prefix + "ab")
    words = {}
    for _ in range(rng.randrange(1, 14)):
        w = "".join(rng.choice(alphabet) for _ in range(rng.randrange(1, 7)))
        words[w] = rng.randrange(1, 5)
    return prefix, specials, words, rng.randrange(3, 30)


@pytest.mark.parametrize("seed", range(60))
def test_incremental_matches_the_literal_loop(seed):
    prefix, specials, words, target = seeded_case(seed)
    a = RefWordPieceTrainer(target, 1, specials, prefix, literal=True)
    b = RefWordPieceTrainer(target, 1, specials, prefix, literal=False)
    for wf in (words, {w[::-1] + "b": f + 1 for w, f in words.items()}):  # (a second training on the same trainers)
        grow = target + (0 if wf is words else 6)
        a.target = b.target = grow
        ma, mb = a.train_words(wf), b.train_words(wf)
        assert a.merges == b.merges and a.vocab == b.vocab and a.tokens == b.tokens
        assert a.best_counts == b.best_counts and a.stopped_on == b.stopped_on
        assert a.merged_was_key == 0  # merged is never a key already
        for w in wf:  # the model's encode gives the trainer's tokens where all of them are keys
            if all(t in a.vocab for t in a.tokens[w]):
                assert ma.encode(w) == [a.vocab[t] for t in a.tokens[w]] == mb.encode(w)
