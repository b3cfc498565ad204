"""CPU tests of the classic BPE trainer's oracle (tests/bpe_trainer_ref.py, the restatement of the
reference's src/bpe_trainer.rs): the reference's own trainer tests (:474-511), a training worked out
by hand, and the quirks the GPU tests rely on.  No GPU."""
from tests.bpe_trainer_ref import RefBpeTrainer


def test_kat_bpe_trainer_basic():
    """src/bpe_trainer.rs:474-495."""
    tr = RefBpeTrainer(vocab_size=100, min_frequency=1, show_progress=False)
    vocab, merges = tr.train(["hello world", "hello there", "world hello", "hello hello hello"])
    assert len(vocab) >= 4
    assert merges
    assert all(a + b in vocab for a, b in merges)
    assert [vocab[t] for t in ("<unk>", "<pad>", "<s>", "</s>")] == [0, 1, 2, 3]


def test_kat_bpe_trainer_with_suffix():
    """src/bpe_trainer.rs:497-511."""
    tr = RefBpeTrainer(vocab_size=50, min_frequency=1, end_of_word_suffix="</w>", show_progress=False)
    vocab, _ = tr.train(["hello world"])
    assert any("</w>" in k for k in vocab)


def test_hand_computed_training():
    """Words ab x3, abc x2, bc x1.  Chars: b 6, a 5, c 3.  Pairs: (a, b) 3 + 2 = 5, (b, c) 2 + 1 = 3,
    so (a, b) merges first.  Then the words are [ab], [ab, c], [b, c]: (ab, c) 2 and (b, c) 1, so
    (ab, c) merges and the vocab is full."""
    tr = RefBpeTrainer(vocab_size=5, min_frequency=1, special_tokens=[])
    vocab, merges = tr.train_words({"ab": 3, "abc": 2, "bc": 1})
    assert vocab == {"b": 0, "a": 1, "c": 2, "ab": 3, "abc": 4}
    assert merges == [("a", "b"), ("ab", "c")]
    assert tr.best_counts == [5, 2] and tr.tie_merges == [] and tr.stopped_on == "vocab_size"
    assert tr.splits == {"ab": ["ab"], "abc": ["abc"], "bc": ["b", "c"]}
    assert tr.count_pairs() == {("b", "c"): 1}
    # one merge fewer: the counts the second merge chose from
    tr = RefBpeTrainer(vocab_size=4, min_frequency=1, special_tokens=[])
    tr.train_words({"ab": 3, "abc": 2, "bc": 1})
    assert tr.count_pairs() == {("ab", "c"): 2, ("b", "c"): 1}


def test_tie_conventions():
    """Equal char frequencies: ascending code point.  Equal pair counts: the smallest pair of
    symbol ids, i.e. here the pair whose first char comes first."""
    tr = RefBpeTrainer(vocab_size=6, min_frequency=1, special_tokens=[])
    vocab, merges = tr.train_words({"cd": 2, "ab": 2})
    assert [vocab[c] for c in "abcd"] == [0, 1, 2, 3]
    assert merges == [("a", "b"), ("c", "d")]
    assert tr.tie_merges == [0]  # the second merge had no rival left


def test_merge_is_left_to_right_and_overlaps_skip():
    assert RefBpeTrainer.merge_pair(list("aaa"), "a", "a", "aa") == ["aa", "a"]
    assert RefBpeTrainer.merge_pair(list("aaaa"), "a", "a", "aa") == ["aa", "aa"]
    assert RefBpeTrainer.merge_pair(list("abab"), "a", "b", "ab") == ["ab", "ab"]
    assert RefBpeTrainer.merge_pair(list("ba"), "a", "b", "ab") == ["b", "a"]


def test_duplicate_special_and_merged_string_already_in_vocab():
    """A repeated special overwrites its id (the vocab does not grow for it, next_id still moves on);
    a merged string that is in the vocab already gets a new id, the vocab does not grow, the merge is
    listed and training goes on."""
    tr = RefBpeTrainer(vocab_size=7, min_frequency=1, special_tokens=["ab", "<pad>", "ab"])
    vocab, merges = tr.train(["ab ab ab abc abc"])
    assert tr.initial_vocab_size == 5  # ab, <pad>, a, b, c
    assert merges[0] == ("a", "b")
    assert vocab["ab"] == 5            # vocab.len() at that merge, not the special's 2
    assert merges[1] == ("ab", "c") and vocab["abc"] == 5  # the vocab did not grow on the first merge
    assert len(vocab) == 6 and tr.stopped_on == "no_pairs"


def test_continuing_subword_prefix_symbols_are_not_in_the_initial_vocab():
    tr = RefBpeTrainer(vocab_size=6, min_frequency=1, special_tokens=[], continuing_subword_prefix="##")
    vocab, merges = tr.train_words({"aba": 2})
    assert tr.initial_vocab_size == 2 and "##a" not in vocab and "##b" not in vocab
    assert merges == [("a", "##b"), ("a##b", "##a")]
    assert vocab == {"a": 0, "b": 1, "a##b": 2, "a##b##a": 3}


def test_stops():
    tr = RefBpeTrainer(vocab_size=100, min_frequency=6, special_tokens=[])
    assert tr.train_words({"ab": 3, "abc": 2})[1] == [] and tr.stopped_on == "min_frequency"
    tr = RefBpeTrainer(vocab_size=100, min_frequency=5, special_tokens=[])
    assert tr.train_words({"ab": 3, "abc": 2})[1] == [("a", "b")]
    tr = RefBpeTrainer(vocab_size=100, min_frequency=0, special_tokens=[])
    assert tr.train_words({"ab": 3, "abc": 2})[1] == [("a", "b"), ("ab", "c")] and tr.stopped_on == "no_pairs"
    tr = RefBpeTrainer(vocab_size=3, min_frequency=1)
    assert tr.train(["ab ab"]) == ({"<unk>": 0, "<pad>": 1, "<s>": 2, "</s>": 3, "a": 4, "b": 5}, [])
    assert RefBpeTrainer().train([]) == ({"<unk>": 0, "<pad>": 1, "<s>": 2, "</s>": 3}, [])
    assert RefBpeTrainer().train(["", " \u3000\n"])[1] == []
    # a word of frequency 0 adds no pair (count_pairs skips it)
    tr = RefBpeTrainer(vocab_size=100, min_frequency=0, special_tokens=[])
    assert tr.train_words({"ab": 0})[1] == []
