"""A Python restatement of the reference's Unigram trainer and model (Complexity-ML/complexity-tokenizer
v0.3.3): UnigramTrainer, src/trainers.rs:287-546 (binding src/bindings/trainers.rs:156-215), and
UnigramModel, src/models.rs:150-299 (binding src/bindings/models.rs:52-87), line by line.  The GPU
implementation is compared with this file; nothing here is shared with it.

Python floats are f64 and `a + b` rounds once, as Rust's does; `ln` is libm's log (math.log), and
the restatement maps a count of 0 to -inf itself (math.log(0.0) raises).

One order the reference leaves to randomly seeded hash iteration is fixed here as in the library
(include/ctok_unigram.h): the seed sort is a stable sort by count over HashMap iteration order, so
the order among equal counts is random there; here **among equal counts, ascending UTF-8 bytes**.
Everything after the seed sort is deterministic.

The trainer's backtrack indexes with `prev as usize` unguarded (src/trainers.rs:533-536): a position
that nothing finite reaches has prev = -1, and the next `best_token[pos]` is out of bounds: a panic
(PanicException here).
"""
import math
import unicodedata

INF = float("inf")
META = "▁"

# the 25 White_Space code points (char::is_whitespace)
WHITE_SPACE = [0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) + \
              [0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
_SPLIT = frozenset(chr(c) for c in WHITE_SPACE if c != 0x20)


class PanicException(Exception):
    pass


def metaspace(text: str) -> list:
    """UnigramTrainer::pretokenize (src/trainers.rs:344-354): NFC, then Metaspace with '▁' and
    add_prefix_space (src/pretokenizers.rs:188-200)."""
    t = META + unicodedata.normalize("NFC", text)
    t = t.replace(" ", META)
    out, cur = [], []
    for c in t:  # split(|c| c.is_whitespace() && c != replacement), empty parts dropped
        if c in _SPLIT:
            if cur:
                out.append("".join(cur))
            cur = []
        else:
            cur.append(c)
    if cur:
        out.append("".join(cur))
    return out


def lines_of(raw: bytes) -> list:
    """BufRead::lines: split at \\n, a final \\r of a line dropped, no last empty line."""
    lines = raw.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return [(ln[:-1] if ln.endswith(b"\r") else ln).decode("utf-8") for ln in lines]


def rust_min(a: float, b: float) -> float:
    """f64::min: a NaN operand is ignored"""
    if b != b:
        return a
    if a != a:
        return b
    return b if b < a else a


def as_usize(x: float) -> int:
    """`x as usize`: saturating, NaN gives 0"""
    if x != x or x <= 0.0:
        return 0
    if x >= 18446744073709551616.0:
        return (1 << 64) - 1
    return int(x)


def ln(x: float) -> float:
    if x == 0.0:
        return -INF
    return math.log(x)


class RefUnigramModel:
    def __init__(self, vocab, unk_token="<unk>"):
        self.list = [(t, float(s)) for t, s in vocab]
        self.vocab, self.vocab_r = {}, {}
        min_score = 0.0
        for i, (t, s) in enumerate(self.list):
            self.vocab[t] = (i, s)
            self.vocab_r[i] = t
            min_score = rust_min(min_score, s)
        self.unk_id = self.vocab[unk_token][0] if unk_token in self.vocab else 0
        self.min_score = min_score - 10.0

    def encode(self, text: str) -> list:
        """tokenize (src/models.rs:225-269), the literal double loop"""
        if not text:
            return []
        n = len(text)
        best = [(-INF, -1, 0)] * (n + 1)
        best[0] = (0.0, -1, 0)
        for end in range(1, n + 1):
            for start in range(end):
                hit = self.vocab.get(text[start:end])
                if hit is not None:
                    tid, score = hit
                elif end - start == 1:
                    tid, score = self.unk_id, self.min_score
                else:
                    continue
                new = best[start][0] + score
                if new > best[end][0]:
                    best[end] = (new, start, tid)
        out, pos = [], n
        while pos > 0:
            _, prev, tid = best[pos]
            out.append(tid)
            pos = prev
        out.reverse()
        return out

    def lattice(self, text: str) -> list:
        """row[start][j] = id of text[start : start + j + 1] or None, j < window: the vocab's longest
        string in chars.  Independent of every score."""
        w = max([len(t) for t in self.vocab] + [0])
        return [[(self.vocab[text[s:s + j + 1]][0] if s + j + 1 <= len(text) and text[s:s + j + 1] in self.vocab else None)
                 for j in range(w)] for s in range(len(text))]

    def encode_lattice(self, text: str) -> list:
        """The formulation of the kernels: the lattice first, then per end the maximum of
        best[start] + score over the candidate starts, the smallest start among equal sums, and
        nothing where no sum is above -inf."""
        n = len(text)
        if not n:
            return []
        rows = self.lattice(text)
        w = len(rows[0])
        score_of = [s for _, s in self.list]
        best, back = [0.0] + [-INF] * n, [(-1, 0)] * (n + 1)
        for end in range(1, n + 1):
            top, arg = -INF, None
            for j in range(min(max(w, 1), end)):  # length j + 1, from the longest down: the starts ascend
                start = end - j - 1
                tid = rows[start][j] if j < w else None
                if tid is not None:
                    sc = score_of[tid]
                elif j == 0:
                    tid, sc = self.unk_id, self.min_score
                else:
                    continue
                cand = best[start] + sc
                if cand > -INF and (cand > top or (cand == top and (arg is None or start < arg[0]))):
                    top, arg = cand, (start, tid)
            if arg is not None:
                best[end], back[end] = top, arg
        out, pos = [], n
        while pos > 0:
            prev, tid = back[pos]
            out.append(tid)
            pos = prev
        out.reverse()
        return out

    def decode(self, ids) -> str:
        return "".join(self.vocab_r[i] for i in ids if i in self.vocab_r)

    def vocab_size(self) -> int:
        return len(self.vocab)

    def token_to_id(self, token):
        hit = self.vocab.get(token)
        return None if hit is None else hit[0]

    def id_to_token(self, i):
        return self.vocab_r.get(i)


class RefUnigramTrainer:
    def __init__(self, vocab_size=8000, special_tokens=None, initial_vocab_size=1000000, shrinking_factor=0.75,
                 n_iterations=16, max_piece_length=16):
        self.vocab_size_target = vocab_size
        self.special_tokens = ["<unk>", "<s>", "</s>"] if special_tokens is None else list(special_tokens)
        self.initial_vocab_size = initial_vocab_size
        self.shrinking_factor = float(shrinking_factor)
        self.n_iterations = n_iterations
        self.max_piece_length = max_piece_length
        self.vocab = []
        # what the parity tests read
        self.sentences = []
        self.substring_counts = {}
        self.expected_counts = {}
        self.iterations = 0
        self.sizes = []

    def train(self, files):
        texts = []
        for path in files:
            with open(path, "rb") as f:
                texts += lines_of(f.read())
        return self.train_from_iterator(texts)

    def train_from_iterator(self, texts):
        sentences = []
        for t in texts:
            sentences += metaspace(t)
        return self.train_sentences(sentences)

    def count_substrings(self, sentences) -> dict:
        freqs = {}
        for s in sentences:
            n = min(len(s), self.max_piece_length)
            for start in range(len(s)):
                for end in range(start + 1, min(start + n, len(s)) + 1):
                    sub = s[start:end]
                    freqs[sub] = freqs.get(sub, 0) + 1
        return freqs

    def train_sentences(self, sentences):
        """train_from_sentences (src/trainers.rs:390-482).  A panic leaves self.vocab as it was (the
        library's rule; the reference's object is poisoned by then)."""
        before = self.vocab
        try:
            return self._train(list(sentences))
        except PanicException:
            self.vocab = before
            raise

    def _train(self, sentences):
        self.sentences = sentences
        freqs = self.count_substrings(sentences)
        self.substring_counts = dict(freqs)
        for t in self.special_tokens:
            freqs[t] = 1
        # the convention: among equal counts, ascending UTF-8 bytes
        items = sorted(freqs.items(), key=lambda kv: (-kv[1], kv[0].encode("utf-8")))
        del items[self.initial_vocab_size:]
        total = 0.0
        for _, f in items:
            total += float(f)
        self.vocab = [(t, ln(float(f) / total)) for t, f in items]
        self.iterations, self.sizes, self.expected_counts = 0, [], {}
        for _ in range(self.n_iterations):
            if len(self.vocab) <= self.vocab_size_target:
                break
            vocab_map = dict(self.vocab)
            expected = {}
            for s in sentences:
                for tok in self.viterbi_segment(s, vocab_map):
                    expected[tok] = expected.get(tok, 0.0) + 1.0
            target = max(as_usize(float(len(self.vocab)) * self.shrinking_factor), self.vocab_size_target)
            scored = [(t, expected.get(t, 0.0)) for t, _ in self.vocab]
            scored.sort(key=lambda tc: -tc[1])  # stable
            del scored[target:]
            total_count = 0.0
            for _, c in scored:
                total_count += c
            self.expected_counts = {t: expected.get(t, 0.0) for t, _ in self.vocab}
            self.vocab = [(t, ln(c / total_count) if total_count > 0.0 else -100.0) for t, c in scored]
            self.iterations += 1
            self.sizes.append(len(self.vocab))
        for t in self.special_tokens:
            if not any(v == t for v, _ in self.vocab):
                self.vocab.append((t, -100.0))
        return RefUnigramModel(list(self.vocab), "<unk>")

    def viterbi_segment(self, sentence: str, vocab_map: dict) -> list:
        """src/trainers.rs:485-540"""
        if not sentence:
            return []
        n = len(sentence)
        best = [(-INF, -1)] * (n + 1)
        best[0] = (0.0, -1)
        token = [""] * (n + 1)
        for end in range(1, n + 1):
            for start in range(max(end - self.max_piece_length, 0), end):
                sub = sentence[start:end]
                if sub in vocab_map:
                    score = vocab_map[sub]
                elif end - start == 1:
                    score = vocab_map.get("<unk>", -100.0)
                else:
                    continue
                new = best[start][0] + score
                if new > best[end][0]:
                    best[end] = (new, start)
                    token[end] = sub
        out, pos = [], n
        while pos > 0:
            if pos > n:
                raise PanicException("index out of bounds: the len is %d but the index is %d" % (n + 1, pos))
            out.append(token[pos])
            pos = best[pos][1] if best[pos][1] >= 0 else (1 << 64) - 1  # `as usize`
        out.reverse()
        return out

    def get_vocab(self) -> list:
        return list(self.vocab)
