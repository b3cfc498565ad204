"""The reference's WordPiece trainer and model restated on Python strings, as the test oracle of
complexity_tokenizer.WordPieceTrainer and complexity_tokenizer.WordPieceModel.

Reference (Complexity-ML/complexity-tokenizer v0.3.3), line by line:
  WordPieceTrainer   src/trainers.rs:64-279 (pretokenize :79-89, train :92-109, train_from_texts
                     :112-127, train_from_word_freqs :130-225, tokenize_for_training :228-273)
  WordPieceModel     src/models.rs:17-142
The normaliser is Sequence[NFC, Lowercase] (unicodedata NFC, str.lower()), the pre-tokenizer
str::split_whitespace: the 25 White_Space code points of tests/bpe_trainer_ref.py.

The orders the reference leaves to hash iteration follow include/ctok_wordpiece.h:
  - chars enter the vocab in ascending code point order;
  - among the pairs of the largest count the smallest (key(a), key(b)) wins.  key(t) is the vocab
    id of t when t is a key, else t is prefix + char and key(t) = 2^31 + code point.  A trainer
    that trains a second time hands ids out from 0 again, so two keys can share an id: keys are
    given at the start of a training to the vocab strings in (id, UTF-8 bytes) order and then to
    every merged string, and a string whose id an earlier string holds takes the next free value
    from 2^31 + 0x110000 up instead;
  - in the model, among vocab strings that share an id, id_to_token and decode use the smallest
    string by UTF-8 bytes.
"""
import unicodedata

from tests.bpe_trainer_ref import split_whitespace

DEFAULT_SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
KEY_CHAR = 1 << 31
KEY_SPILL = KEY_CHAR + 0x110000


def normalize(text):
    """Sequence[NFC, Lowercase]"""
    return unicodedata.normalize("NFC", text).lower()


def pretokenize(text):
    return split_whitespace(normalize(text))


def read_lines(path):
    """BufRead::lines: split at \\n, one trailing \\r dropped, no empty last line; IOError on a
    missing file or invalid UTF-8."""
    with open(path, "rb") as f:
        raw = f.read()
    lines = raw.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    out = []
    for ln in lines:
        if ln.endswith(b"\r"):
            ln = ln[:-1]
        try:
            out.append(ln.decode("utf-8"))
        except UnicodeDecodeError as e:
            raise IOError("stream did not contain valid UTF-8") from e
    return out


class RefWordPieceModel:
    def __init__(self, vocab, prefix="##", unk_token="[UNK]", max_input_chars_per_word=100):
        self.vocab = dict(vocab)
        self.vocab_r = {}
        for k in sorted(self.vocab, key=lambda s: s.encode("utf-8"), reverse=True):
            self.vocab_r[self.vocab[k]] = k  # convention: the smallest string keeps the id
        self.longest_key = max(map(len, self.vocab), default=0)
        self.prefix = prefix
        self.unk_token = unk_token
        self.max_input_chars_per_word = max_input_chars_per_word

    def tokenize_word(self, word):
        chars = word  # (a str indexes by char)
        unk = self.vocab.get(self.unk_token)
        if len(chars) > self.max_input_chars_per_word:
            return [] if unk is None else [unk]
        tokens = []
        start = 0
        while start < len(chars):
            end = min(len(chars), start + self.longest_key)  # (no longer candidate can be a key)
            found = False
            while start < end:
                substr = chars[start:end]
                token = self.prefix + substr if start > 0 else substr
                if token in self.vocab:
                    tokens.append(self.vocab[token])
                    found = True
                    break
                end -= 1
            if not found:
                if unk is not None:
                    tokens.append(unk)
                start += 1
            else:
                start = end
        return tokens

    def encode(self, text):
        out = []
        for word in split_whitespace(text):
            out.extend(self.tokenize_word(word))
        return out

    def decode(self, ids):
        result = ""
        for i in ids:
            token = self.vocab_r.get(i)
            if token is None:
                continue
            if token.startswith(self.prefix):
                result += token[len(self.prefix):]
            else:
                if result:
                    result += " "
                result += token
        return result

    def vocab_size(self):
        return len(self.vocab)

    def token_to_id(self, token):
        return self.vocab.get(token)

    def id_to_token(self, i):
        return self.vocab_r.get(i)


class RefWordPieceTrainer:
    def __init__(self, vocab_size=30000, min_frequency=2, special_tokens=None, continuing_subword_prefix="##",
                 max_input_chars_per_word=100, literal=False):
        self.target = vocab_size
        self.min_frequency = min_frequency
        self.special_tokens = list(DEFAULT_SPECIALS if special_tokens is None else special_tokens)
        self.prefix = continuing_subword_prefix
        self.max_input_chars_per_word = max_input_chars_per_word
        # literal: tokenise every word again in every round, as the reference does.  Otherwise a
        # word is tokenised again only when the round's new string, without the prefix, occurs in
        # it: no other word can match the new string anywhere, so the results are the same
        # (tests/test_wordpiece_ref_cpu.py compares the two).
        self.literal = literal
        self.vocab = {}  # never cleared (the reference's quirk: a second training starts from it)
        self._longest_key = None  # (chars of the longest key while a training keeps it up to date)
        # what the tests look at besides the result
        self.word_freqs = {}
        self.merges = []
        self.tokens = {}
        self.best_counts = []
        self.tie_merges = []
        self.stopped_on = None
        self.merged_was_key = 0
        self.pair_freqs = {}    # of the last round counted
        self.live_pairs = []    # the number of distinct pairs every round chose from
        self.seen_pairs = set() # every pair that had a count in some round

    @property
    def vocab_size(self):
        return len(self.vocab)

    def word_counts(self, texts):
        wf = {}
        for text in texts:
            for word in pretokenize(text):
                wf[word] = wf.get(word, 0) + 1
        return wf

    def train(self, files):
        texts = []
        for path in files:
            texts.extend(read_lines(path))
        return self.train_from_iterator(texts)

    def train_from_iterator(self, texts):
        return self.train_words(self.word_counts(texts))

    # tokenize_for_training :228-273
    def tokenize_for_training(self, word):
        chars = word  # (a str indexes by char)
        longest_key = max(map(len, self.vocab), default=0) if self._longest_key is None else self._longest_key
        tokens = []
        start = 0
        while start < len(chars):
            end = min(len(chars), start + longest_key)  # (no longer candidate can be a key)
            found = False
            while start < end:
                substr = chars[start:end]
                token = self.prefix + substr if start > 0 else substr
                if token in self.vocab:
                    tokens.append(token)
                    found = True
                    break
                end -= 1
            if not found:
                tokens.append(self.prefix + chars[start] if start > 0 else chars[start])
                start += 1
            else:
                start = end
        return tokens

    def _give_key(self, t):
        k = self.vocab[t]
        if k >= KEY_CHAR:
            raise ValueError("a vocab id of 2^31 or more")
        if k in self._taken:
            k = self._spill
            self._spill += 1
        self._taken.add(k)
        self._key[t] = k

    def key(self, t):
        if t in self._key:
            return self._key[t]
        return KEY_CHAR + ord(t[len(self.prefix):])  # prefix + char, not a key

    # train_from_word_freqs :130-225
    def train_words(self, word_freqs):
        word_freqs = {w: f for w, f in word_freqs.items() if f >= self.min_frequency and w}
        self.word_freqs = word_freqs
        self.merges, self.best_counts, self.tie_merges = [], [], []
        self.stopped_on = "vocab_size"
        self.pair_freqs, self.live_pairs, self.seen_pairs = {}, [], set()
        next_id = 0
        for token in self.special_tokens:
            self.vocab[token] = next_id
            next_id += 1
        chars = sorted({c for word in word_freqs for c in word}, key=ord)  # convention: ascending code point
        for c in chars:
            if c not in self.vocab:
                self.vocab[c] = next_id
                next_id += 1
        self._key, self._taken, self._spill = {}, set(), KEY_SPILL
        for t in sorted(self.vocab, key=lambda s: (self.vocab[s], s.encode("utf-8"))):
            self._give_key(t)
        self.tokens = {}
        self._longest_key = max(map(len, self.vocab), default=0)
        stale = set(word_freqs)
        pair_freqs = {}
        while len(self.vocab) < self.target:
            if self.literal:
                pair_freqs = {}
            for word in (word_freqs if self.literal else stale):
                freq = word_freqs[word]
                old = self.tokens.get(word, [])
                if not self.literal:  # (the word's old pairs leave the counts, its new ones enter)
                    for pair in zip(old, old[1:]):
                        pair_freqs[pair] -= freq
                        if not pair_freqs[pair]:
                            del pair_freqs[pair]
                tokens = self.tokens[word] = self.tokenize_for_training(word)
                for pair in zip(tokens, tokens[1:]):
                    pair_freqs[pair] = pair_freqs.get(pair, 0) + freq
            stale = set()
            self.pair_freqs = pair_freqs
            if not pair_freqs:
                self.stopped_on = "no_pairs"
                break
            self.live_pairs.append(len(pair_freqs))
            self.seen_pairs.update(pair_freqs)
            top = max(pair_freqs.values())
            if top >= 1 << 32:
                raise ValueError("a pair count of %d does not fit the reference's u32 counts" % top)
            tied = [p for p, f in pair_freqs.items() if f == top]
            a, b = min(tied, key=lambda p: (self.key(p[0]), self.key(p[1])))
            if len(tied) > 1:
                self.tie_merges.append(len(self.merges))
            self.best_counts.append(top)
            rest = b[len(self.prefix):] if b.startswith(self.prefix) else b
            merged = a + rest
            if merged in self.vocab:
                self.merged_was_key += 1
                raise ValueError("merged %r is already a key: the reference would loop forever" % merged)
            self.vocab[merged] = next_id
            next_id += 1
            self._give_key(merged)
            self._longest_key = max(self._longest_key, len(merged))
            self.merges.append((a, b))
            plain = merged[len(self.prefix):] if merged.startswith(self.prefix) and len(merged) > len(self.prefix) else merged
            stale = {w for w in word_freqs if plain in w or merged in w}
        self.final_pairs = self.count_pairs()
        self._longest_key = None
        return RefWordPieceModel(self.vocab, self.prefix, "[UNK]", self.max_input_chars_per_word)

    def count_pairs(self):
        """A fresh count of the pairs of every word tokenised against the vocab as it is now."""
        self.tokens = {word: self.tokenize_for_training(word) for word in self.word_freqs}
        pair_freqs = {}
        for word, freq in self.word_freqs.items():
            tokens = self.tokens[word]
            for pair in zip(tokens, tokens[1:]):
                pair_freqs[pair] = pair_freqs.get(pair, 0) + freq
        return pair_freqs
