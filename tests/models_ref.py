"""Plain-Python restatement of the reference's WordLevelModel, ByteLevelBpeModel and CharBpeModel
(Complexity-ML/complexity-tokenizer v0.3.3, src/models.rs:300-741), the yardstick of
tests/test_gpu_models.py.  The reference is a Rust crate and cannot be built where these tests run,
so its behaviour is restated here line by line, with its line numbers, and checked against
hand-worked cases in tests/test_models_ref_cpu.py.

The orders the reference leaves to hash iteration are fixed as include/ctok_models.h states: among
vocab strings that share an id, id_to_token and decode use the smallest string by UTF-8 bytes.
"""
from tests.bpe_trainer_ref import WHITE_SPACE, split_whitespace


def _vocab_r(vocab):
    out = {}
    for k in sorted(vocab, key=lambda s: s.encode("utf-8"), reverse=True):
        out[vocab[k]] = k
    return out


def merge_loop_literal(tokens, ranks):
    """:487-514 and :662-689 as they stand: every step scans all adjacent pairs, takes the smallest
    rank (a later pair replaces the best only when its rank is smaller, so the leftmost of equals
    stays) and merges that one occurrence."""
    tokens = list(tokens)
    while True:
        best = None
        for i in range(len(tokens) - 1):
            rank = ranks.get((tokens[i], tokens[i + 1]))
            if rank is not None and (best is None or rank < best[1]):
                best = (i, rank)
        if best is None:
            return tokens
        i = best[0]
        tokens[i:i + 2] = [tokens[i] + tokens[i + 1]]


_NO_RANK = float("inf")


def merge_loop(tokens, ranks):
    """merge_loop_literal with the pairs' ranks kept in a list: a merge changes only the two pairs
    next to it, so the other entries still hold what the literal scan would look up.  The same
    steps in the same order (tests/test_models_ref_cpu.py compares the two); the long words of the
    tier tests need it."""
    tokens = list(tokens)
    r = [ranks.get((tokens[i], tokens[i + 1]), _NO_RANK) for i in range(len(tokens) - 1)]
    while r:
        best = min(r)
        if best == _NO_RANK:
            break
        i = r.index(best)  # the leftmost
        tokens[i:i + 2] = [tokens[i] + tokens[i + 1]]
        del r[i]
        if i < len(r):
            r[i] = ranks.get((tokens[i], tokens[i + 1]), _NO_RANK)
        if i > 0:
            r[i - 1] = ranks.get((tokens[i - 1], tokens[i]), _NO_RANK)
    return tokens


def merge_ranks(merges):
    """:436-440, :627-631: HashMap::insert, a later duplicate of a pair overwrites the rank."""
    ranks = {}
    for rank, (a, b) in enumerate(merges):
        ranks[(a, b)] = rank
    return ranks


def bytes_to_unicode():
    """:369-390"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    cs = list(bs)
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


def from_utf8_lossy(raw):
    """String::from_utf8_lossy: one U+FFFD per maximal invalid subpart (the Unicode "maximal
    subpart" practice, core::str::lossy), as a walk over a table of the valid second bytes."""
    second = {}
    for b in range(0xC2, 0xE0):
        second[b] = (2, 0x80, 0xBF)
    for b in range(0xE0, 0xF0):
        second[b] = (3, 0xA0 if b == 0xE0 else 0x80, 0x9F if b == 0xED else 0xBF)
    for b in range(0xF0, 0xF5):
        second[b] = (4, 0x90 if b == 0xF0 else 0x80, 0x8F if b == 0xF4 else 0xBF)
    out, i = [], 0
    while i < len(raw):
        b = raw[i]
        if b < 0x80:
            out.append(chr(b))
            i += 1
            continue
        if b not in second:
            out.append("\ufffd")
            i += 1
            continue
        width, lo, hi = second[b]
        j = i + 1
        while j < i + width and j < len(raw) and (lo if j == i + 1 else 0x80) <= raw[j] <= (hi if j == i + 1 else 0xBF):
            j += 1
        out.append(raw[i:j].decode("utf-8") if j == i + width else "\ufffd")
        i = j
    return "".join(out)


def trim_end(s):
    """str::trim_end: char::is_whitespace is the White_Space property."""
    n = len(s)
    while n and s[n - 1] in WHITE_SPACE:
        n -= 1
    return s[:n]


class _Ref:
    def __init__(self, vocab, unk_token):
        self.vocab = dict(vocab)
        self.vocab_r = _vocab_r(self.vocab)
        self.unk_token = unk_token

    @property
    def unk_id(self):
        return self.vocab.get(self.unk_token, 0)  # :332, :521, :696

    @property
    def vocab_size(self):
        return len(self.vocab)

    def token_to_id(self, token):
        return self.vocab.get(token)

    def id_to_token(self, id):
        return self.vocab_r.get(id)

    def encode_batch(self, texts):
        return [self.encode(t) for t in texts]


class RefWordLevelModel(_Ref):
    """:316-362"""

    def __init__(self, vocab, unk_token="<unk>"):
        super().__init__(vocab, unk_token)

    def encode(self, text):  # :331-337
        unk = self.unk_id
        return [self.vocab.get(w, unk) for w in split_whitespace(text)]

    def decode(self, ids):  # :340-346
        return " ".join(self.vocab_r[i] for i in ids if i in self.vocab_r)


class RefByteLevelBpeModel(_Ref):
    """:421-589"""

    def __init__(self, vocab, merges, unk_token="<unk>", add_prefix_space=True):
        super().__init__(vocab, unk_token)
        self.ranks = merge_ranks(merges)
        self.add_prefix_space = add_prefix_space
        self.byte_encoder = bytes_to_unicode()
        self.byte_decoder = {c: b for b, c in self.byte_encoder.items()}

    def words(self, text):
        """:523-554: a word starts at the text's start and at every U+0020"""
        if self.add_prefix_space and not text.startswith(" "):
            text = " " + text
        out, cur = [], ""
        for c in text:
            if c == " " and cur:
                out.append(cur)
                cur = ""
            cur += c
        if cur:
            out.append(cur)
        return out

    def tokenize_word(self, word):  # :471-517
        return merge_loop([self.byte_encoder[b] for b in word.encode("utf-8")], self.ranks)

    def encode(self, text):  # :520-557
        unk = self.unk_id
        return [self.vocab.get(t, unk) for w in self.words(text) for t in self.tokenize_word(w)]

    def decode(self, ids):  # :560-568, :462-468
        tokens = "".join(self.vocab_r[i] for i in ids if i in self.vocab_r)
        return from_utf8_lossy(bytes(self.byte_decoder[c] for c in tokens if c in self.byte_decoder))


class RefCharBpeModel(_Ref):
    """:612-741"""

    def __init__(self, vocab, merges, end_of_word_suffix="</w>", unk_token="<unk>"):
        super().__init__(vocab, unk_token)
        self.ranks = merge_ranks(merges)
        self.suffix = end_of_word_suffix

    def tokenize_word(self, word):  # :644-692
        if not word:
            return []
        chars = list(word)
        return merge_loop(chars[:-1] + [chars[-1] + self.suffix], self.ranks)

    def encode(self, text):  # :695-705
        unk = self.unk_id
        return [self.vocab.get(t, unk) for w in split_whitespace(text) for t in self.tokenize_word(w)]

    def decode(self, ids):  # :708-725
        out = ""
        for i in ids:
            t = self.vocab_r.get(i)
            if t is None:
                continue
            if t.endswith(self.suffix):
                out += t[:len(t) - len(self.suffix)] + " "
            else:
                out += t
        return trim_end(out)
