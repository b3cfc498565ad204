"""The reference's classic BPE trainer restated on Python strings, as the test oracle of
complexity_tokenizer.BpeTrainer.

Reference: BpeTrainer, src/bpe_trainer.rs:100-399 (Complexity-ML/complexity-tokenizer v0.3.3), line
by line: every pair of every word is counted again before every merge, symbols are strings and
compared as strings.  The two orders the reference leaves to hash iteration follow the conventions
of include/ctok_bpe_trainer.h:
  - characters of equal total frequency enter the vocabulary in ascending code point order;
  - among the pairs with the largest count the smallest (symbol id of first, symbol id of second)
    wins, with symbol ids handed out as the header says: the characters in vocabulary order, the
    prefixed strings in ascending code point order, the merged strings in merge order.
White_Space is the explicit set of 25 code points that Rust's str::split_whitespace splits on
(tests/test_unicode_tables.py pins the same set); it is not Python's str.split().
"""
import re

DEFAULT_SPECIALS = ["<unk>", "<pad>", "<s>", "</s>"]

WHITE_SPACE = frozenset(chr(c) for c in (
    [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B))
    + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000]))
assert len(WHITE_SPACE) == 25
_WS_RUN = re.compile("[" + "".join(re.escape(c) for c in sorted(WHITE_SPACE)) + "]+")


def split_whitespace(text):
    """str::split_whitespace: the maximal runs of non-White_Space chars."""
    return [w for w in _WS_RUN.split(text) if w]


class RefBpeTrainer:
    def __init__(self, vocab_size=30000, min_frequency=2, special_tokens=None, show_progress=True,
                 end_of_word_suffix=None, continuing_subword_prefix=None):
        self.vocab_size = vocab_size
        self.min_frequency = min_frequency
        self.special_tokens = list(DEFAULT_SPECIALS if special_tokens is None else special_tokens)
        self.end_of_word_suffix = end_of_word_suffix
        self.continuing_subword_prefix = continuing_subword_prefix
        # what the tests look at besides the result
        self.word_freqs = {}
        self.splits = {}
        self.sym_id = {}
        self.best_counts = []   # the count of every merge
        self.tie_merges = []    # indices of the merges chosen among several pairs of the largest count
        self.stopped_on = None  # "vocab_size" | "no_pairs" | "min_frequency"
        self.live_pairs = []    # the number of distinct pairs every merge chose from
        self.seen_pairs = set() # every pair that had a count at some merge

    # build_word_frequencies :240-273
    def build_word_frequencies(self, texts):
        wf = {}
        for text in texts:
            for word in split_whitespace(text):
                if self.end_of_word_suffix is not None:
                    word = word + self.end_of_word_suffix
                wf[word] = wf.get(word, 0) + 1
        return wf

    # build_initial_vocab :276-320
    def build_initial_vocab(self, word_freqs):
        vocab = {}
        next_id = 0
        for token in self.special_tokens:
            vocab[token] = next_id
            next_id += 1
        char_freqs = {}
        for word, freq in word_freqs.items():
            for c in word:
                char_freqs[c] = char_freqs.get(c, 0) + freq
        char_vec = sorted(char_freqs.items(), key=lambda cf: (-cf[1], ord(cf[0])))  # convention: ties by code point
        for c, _ in char_vec:
            if c not in vocab:
                vocab[c] = next_id
                next_id += 1
            self.sym_id.setdefault(c, len(self.sym_id))
        return vocab

    # split_word :323-338
    def split_word(self, word):
        chars = list(word)
        if self.continuing_subword_prefix is not None and len(chars) > 1:
            return [chars[0]] + [self.continuing_subword_prefix + c for c in chars[1:]]
        return chars

    # count_pairs :341-375
    def count_pairs(self):
        pair_freqs = {}
        for word, splits in self.splits.items():
            freq = self.word_freqs.get(word, 0)
            if len(splits) < 2 or freq == 0:
                continue
            for pair in zip(splits, splits[1:]):
                pair_freqs[pair] = pair_freqs.get(pair, 0) + freq
        return pair_freqs

    # merge_pair :378-399
    @staticmethod
    def merge_pair(splits, first, second, merged):
        result = []
        i = 0
        while i < len(splits):
            if i < len(splits) - 1 and splits[i] == first and splits[i + 1] == second:
                result.append(merged)
                i += 2
            else:
                result.append(splits[i])
                i += 1
        return result

    def train(self, texts):
        return self.train_words(self.build_word_frequencies(texts), suffixed=True)

    def train_words(self, word_freqs, suffixed=False):
        """train :100-228 from step 2 on.  suffixed=False: the words are given without the
        end_of_word_suffix (as BpeTrainer.train_words takes them)."""
        if not suffixed and self.end_of_word_suffix is not None:
            wf = {}
            for w, f in word_freqs.items():
                wf[w + self.end_of_word_suffix] = wf.get(w + self.end_of_word_suffix, 0) + f
            word_freqs = wf
        self.word_freqs = dict(word_freqs)
        self.sym_id = {}
        self.best_counts, self.tie_merges, self.stopped_on = [], [], "vocab_size"
        self.live_pairs, self.seen_pairs = [], set()
        vocab = self.build_initial_vocab(self.word_freqs)
        self.splits = {word: self.split_word(word) for word in self.word_freqs}
        if self.continuing_subword_prefix is not None:  # the prefixed symbols' ids: ascending code point
            follows = sorted({c for word in self.word_freqs for c in list(word)[1:]}, key=ord)
            for c in follows:
                self.sym_id.setdefault(self.continuing_subword_prefix + c, len(self.sym_id))
        self.initial_vocab_size = len(vocab)
        merges = []
        while len(vocab) < self.vocab_size:
            pair_freqs = self.count_pairs()
            if not pair_freqs:
                self.stopped_on = "no_pairs"
                break
            self.live_pairs.append(len(pair_freqs))
            self.seen_pairs.update(pair_freqs)
            top = max(pair_freqs.values())
            tied = [p for p, f in pair_freqs.items() if f == top]
            best = min(tied, key=lambda p: (self.sym_id[p[0]], self.sym_id[p[1]]))  # convention: ties by symbol ids
            if not merges and top >= 1 << 32:
                raise ValueError("a pair count of %d does not fit the reference's u32 counts" % top)
            if top < self.min_frequency:
                self.stopped_on = "min_frequency"
                break
            if len(tied) > 1:
                self.tie_merges.append(len(merges))
            self.best_counts.append(top)
            merged = best[0] + best[1]
            vocab[merged] = len(vocab)
            merges.append(best)
            self.sym_id.setdefault(merged, len(self.sym_id))
            for word, splits in self.splits.items():
                if best[0] in splits:  # (merge_pair changes no other word)
                    self.splits[word] = self.merge_pair(splits, best[0], best[1], merged)
        self.vocab, self.merges = vocab, merges
        return vocab, merges
