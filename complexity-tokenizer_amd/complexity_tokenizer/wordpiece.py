"""`complexity_tokenizer.WordPieceTrainer` and `complexity_tokenizer.WordPieceModel` (reference
src/bindings/trainers.rs:94-153 over src/trainers.rs:64-279, src/bindings/models.rs:8-49 over
src/models.rs:17-142) on the GPU, through include/ctok_wordpiece.h.

The trainer's normaliser (NFC, Lowercase), its whitespace split, the word counts, the greedy longest
match of every word, the pair counts and the search for the most frequent pair run on the GPU
(csrc/lowercase.hip, csrc/wordpiece.hip, csrc/bpe_train.hip, csrc/wordcount.hip), and so does the
model's encode; the native host runtime keeps the strings, and decode is host string work.  There is
no CPU fallback: without a HIP device the calls raise DeviceError.  The orders the reference leaves
to hash iteration are fixed as the header states.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as _n
from .bpe_trainer import _array, _raise, _strings

DEFAULT_SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]


def _uint(name, v, limit):
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
        raise TypeError("argument '%s': '%s' object cannot be interpreted as an integer" % (name, type(v).__name__))
    if v < 0:
        raise OverflowError("argument '%s': can't convert negative int to unsigned" % name)
    if v > limit:
        raise OverflowError("argument '%s': out of range" % name)
    return int(v)


def _string(name, v):
    if not isinstance(v, str):
        raise TypeError("argument '%s': '%s' object cannot be converted to 'PyString'" % (name, type(v).__name__))
    if "\0" in v:
        raise ValueError("argument '%s': embedded NUL" % name)
    return v.encode("utf-8")


def _pack(strings):
    """list[bytes] -> (uint8 blob with a spare byte, uint64 offsets)"""
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in strings], out=off[1:])
    return np.frombuffer(b"".join(strings) + b"\0" * 16, dtype=np.uint8), off


def lowercase(texts, device=0) -> list:
    """str::to_lowercase of every text on the GPU (ctok_lowercase); for tests."""
    from . import pack_texts
    buf, off = pack_texts(texts)
    n = len(off) - 1
    cap = int(off[n]) * 3 // 2 + 16
    out = np.zeros(cap, dtype=np.uint8)
    out_off = np.zeros(n + 1, dtype=np.uint64)
    rc = _n.lib.ctok_lowercase(buf.ctypes.data, off.ctypes.data, n, device, out.ctypes.data, cap, out_off.ctypes.data)
    if rc:
        _raise(rc)
    raw, o = out.tobytes(), out_off.tolist()
    return [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(n)]


class WordPieceModel:
    """WordPieceModel(vocab, continuing_subword_prefix="##", unk_token="[UNK]",
    max_input_chars_per_word=100) -- src/bindings/models.rs:16-29."""

    def __init__(self, vocab, continuing_subword_prefix="##", unk_token="[UNK]", max_input_chars_per_word=100, device=0):
        if not isinstance(vocab, dict):
            raise TypeError("argument 'vocab': '%s' object cannot be converted to 'PyDict'" % type(vocab).__name__)
        keys, ids = [], []
        for k, v in vocab.items():
            if not isinstance(k, str):
                raise TypeError("argument 'vocab': '%s' object cannot be converted to 'PyString'" % type(k).__name__)
            keys.append(k.encode("utf-8"))
            ids.append(_uint("vocab", v, 0xFFFFFFFF))
        prefix = _string("continuing_subword_prefix", continuing_subword_prefix)
        unk = _string("unk_token", unk_token)
        max_chars = _uint("max_input_chars_per_word", max_input_chars_per_word, 0xFFFFFFFFFFFFFFFF)
        self._vocab = dict(zip(vocab.keys(), ids))
        self._vocab_r = {}
        for k in sorted(self._vocab, key=lambda s: s.encode("utf-8"), reverse=True):
            self._vocab_r[self._vocab[k]] = k  # among strings that share an id, the smallest keeps it
        self._prefix = continuing_subword_prefix
        self.device = device
        blob, off = _pack(keys)
        idv = np.asarray(ids, dtype=np.uint32)
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_wp_model_create(blob.ctypes.data, off.ctypes.data, idv.ctypes.data, len(keys), prefix, unk,
                                         max_chars, device, ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_n, "lib", None) if _n is not None else None  # (None at interpreter teardown)
        if h and lib is not None:
            lib.ctok_wp_model_destroy(h)
            self._h = None

    def encode_batch_flat(self, texts):
        """(ids: uint32 array, offsets: uint64 array[len(texts) + 1]) of a batch; extension."""
        from . import pack_texts
        buf, off = pack_texts(texts)
        n = len(off) - 1
        ids, toff = ctypes.POINTER(ctypes.c_uint32)(), ctypes.POINTER(ctypes.c_uint64)()
        rc = _n.lib.ctok_wp_model_encode_batch(self._h, buf.ctypes.data, off.ctypes.data, n, ctypes.byref(ids),
                                               ctypes.byref(toff))
        if rc:
            _raise(rc)
        o = np.ctypeslib.as_array(toff, shape=(n + 1,)).copy()
        total = int(o[n])
        return (np.ctypeslib.as_array(ids, shape=(total,)).copy() if total else np.zeros(0, dtype=np.uint32)), o

    def encode_batch(self, texts) -> list:
        """encode of every text, in one pass over the batch on the GPU; extension."""
        ids, off = self.encode_batch_flat(texts)
        ids, off = ids.tolist(), off.tolist()
        return [ids[off[i]:off[i + 1]] for i in range(len(off) - 1)]

    def encode(self, text) -> list:
        """src/models.rs:98-106: no normaliser; every split_whitespace word by greedy longest match."""
        if not isinstance(text, str):
            raise TypeError("argument 'text': '%s' object cannot be converted to 'PyString'" % type(text).__name__)
        return self.encode_batch([text])[0]

    def decode(self, ids) -> str:
        """src/models.rs:109-126"""
        result = []
        empty = True
        for i in ids:
            token = self._vocab_r.get(_uint("ids", i, 0xFFFFFFFF))
            if token is None:
                continue
            if token.startswith(self._prefix):
                token = token[len(self._prefix):]
            else:
                if not empty:
                    result.append(" ")
            result.append(token)
            empty = empty and not token
        return "".join(result)

    def decode_batch(self, batch) -> list:
        """decode of every id list, in one pass over the batch on the GPU: Decoder.wordpiece(prefix,
        cleanup=False) over the model's id -> token map, bound at the first call; extension."""
        dec = getattr(self, "_decoder", None)
        if dec is None:
            from .decoders import Decoder
            dec = Decoder.wordpiece(self._prefix, cleanup=False, device=self.device)
            dec.set_vocab(self._vocab_r)
            self._decoder = dec
        return dec.decode_ids_batch(batch)

    @property
    def vocab_size(self) -> int:
        return len(self._vocab)

    def token_to_id(self, token):
        return self._vocab.get(token)

    def id_to_token(self, id):
        return self._vocab_r.get(id)

    def get_vocab(self) -> dict:
        """A copy of the vocab; extension."""
        return dict(self._vocab)


class WordPieceTrainer:
    """WordPieceTrainer(vocab_size=30000, min_frequency=2, special_tokens=None,
    continuing_subword_prefix="##", max_input_chars_per_word=100) -- src/bindings/trainers.rs:102-134."""

    def __init__(self, vocab_size=30000, min_frequency=2, special_tokens=None, continuing_subword_prefix="##",
                 max_input_chars_per_word=100, device=0):
        vocab_size = _uint("vocab_size", vocab_size, 0xFFFFFFFFFFFFFFFF)
        min_frequency = _uint("min_frequency", min_frequency, 0xFFFFFFFF)
        max_chars = _uint("max_input_chars_per_word", max_input_chars_per_word, 0xFFFFFFFFFFFFFFFF)
        if special_tokens is None:
            special_tokens = DEFAULT_SPECIALS
        if isinstance(special_tokens, (str, bytes)):
            raise TypeError("argument 'special_tokens': Can't extract `str` to `Vec`")
        sp = [s.encode("utf-8") if isinstance(s, str) else None for s in special_tokens]
        if any(s is None for s in sp):
            raise TypeError("argument 'special_tokens': 'list' items must be str")
        prefix = _string("continuing_subword_prefix", continuing_subword_prefix)
        off = np.zeros(len(sp) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in sp], out=off[1:])
        cfg = _n.WpTrainerConfig(
            vocab_size=vocab_size, min_frequency=min_frequency, special=b"".join(sp),
            special_off=off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n_special=len(sp),
            continuing_subword_prefix=prefix, max_input_chars_per_word=max_chars, device=device)
        self._prefix = continuing_subword_prefix
        self._max_chars = max_chars
        self.device = device
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_wp_trainer_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_n, "lib", None) if _n is not None else None  # (None at interpreter teardown)
        if h and lib is not None:
            lib.ctok_wp_trainer_destroy(h)
            self._h = None

    @property
    def vocab_size(self) -> int:
        """The entries of the trainer's vocab, not the target (src/bindings/trainers.rs:149-152)."""
        return int(_n.lib.ctok_wp_trainer_vocab_size(self._h))

    def _result(self):
        vocab, merges = _n.BpeStrings(), _n.BpeStrings()
        ids = ctypes.POINTER(ctypes.c_uint32)()
        rc = _n.lib.ctok_wp_trainer_result(self._h, ctypes.byref(vocab), ctypes.byref(ids), ctypes.byref(merges))
        if rc:
            _raise(rc)
        m = _strings(merges)
        return dict(zip(_strings(vocab), _array(ids, int(vocab.n)))), list(zip(m[0::2], m[1::2]))

    def _model(self) -> WordPieceModel:
        # WordPieceModel::new(vocab.clone(), prefix, "[UNK]", max_input_chars_per_word) :219-224
        return WordPieceModel(self._result()[0], self._prefix, "[UNK]", self._max_chars, device=self.device)

    def train(self, files) -> WordPieceModel:
        """src/trainers.rs:92-109: every BufRead::lines line of every file is a text of its own."""
        if isinstance(files, (str, bytes)):
            raise TypeError("argument 'files': Can't extract `str` to `Vec`")
        texts = []
        for path in files:
            if not isinstance(path, str):
                raise TypeError("argument 'files': '%s' object cannot be converted to 'PyString'" % type(path).__name__)
            with open(path, "rb") as f:  # (a missing file is an IOError here as there)
                raw = f.read()
            lines = raw.split(b"\n")
            if lines[-1] == b"":
                lines.pop()
            for ln in lines:
                if ln.endswith(b"\r"):
                    ln = ln[:-1]
                try:
                    texts.append(ln.decode("utf-8"))
                except UnicodeDecodeError:
                    raise IOError("stream did not contain valid UTF-8") from None
        return self.train_from_iterator(texts)

    def train_from_iterator(self, texts) -> WordPieceModel:
        """src/bindings/trainers.rs:143-147 -> src/trainers.rs:112-127"""
        from . import pack_texts
        buf, off = pack_texts(texts)
        rc = _n.lib.ctok_wp_trainer_train(self._h, buf.ctypes.data, off.ctypes.data, len(off) - 1)
        if rc:
            _raise(rc)
        return self._model()

    def train_words(self, words) -> WordPieceModel:
        """train_from_word_freqs (src/trainers.rs:130-225) on a {word: frequency} dict given
        directly (no normaliser runs); extension."""
        ws = []
        for w in words:
            if not isinstance(w, str):
                raise TypeError("'%s' object cannot be converted to 'PyString'" % type(w).__name__)
            ws.append(w.encode("utf-8"))
        fs = [int(words[w]) for w in words]
        if any(f < 0 or f > 0xFFFFFFFF for f in fs):
            raise OverflowError("a word frequency is out of range for u32")
        freqs = np.asarray(fs, dtype=np.uint32)
        blob, off = _pack(ws)
        rc = _n.lib.ctok_wp_trainer_train_words(self._h, blob.ctypes.data, off.ctypes.data, freqs.ctypes.data, len(ws))
        if rc:
            _raise(rc)
        return self._model()

    def word_counts(self, texts) -> dict:
        """The normaliser, split and count of train_from_iterator alone: {word: count}; extension."""
        from . import pack_texts
        buf, off = pack_texts(texts)
        rc = _n.lib.ctok_wp_trainer_count(self._h, buf.ctypes.data, off.ctypes.data, len(off) - 1)
        if rc:
            _raise(rc)
        words = _n.BpeStrings()
        freqs = ctypes.POINTER(ctypes.c_uint32)()
        rc = _n.lib.ctok_wp_trainer_word_counts(self._h, ctypes.byref(words), ctypes.byref(freqs))
        if rc:
            _raise(rc)
        return dict(zip(_strings(words), _array(freqs, int(words.n))))

    def get_vocab(self) -> dict:
        """Debug: the trainer's vocab (it is kept across trainings, as in the reference)."""
        return self._result()[0]

    def merges(self) -> list:
        """The last training's (a, b) token strings in merge order; extension."""
        return self._result()[1]

    def tokens(self) -> dict:
        """Debug: the last training's words with their final tokens, read back from the device."""
        words, toks = _n.BpeStrings(), _n.BpeStrings()
        off = ctypes.POINTER(ctypes.c_uint64)()
        rc = _n.lib.ctok_wp_trainer_tokens(self._h, ctypes.byref(words), ctypes.byref(toks), ctypes.byref(off))
        if rc:
            _raise(rc)
        w, t = _strings(words), _strings(toks)
        o = _array(off, len(w) + 1) if w else [0]
        return {w[i]: t[o[i]:o[i + 1]] for i in range(len(w))}

    def stats(self) -> dict:
        """What the last counting and training did (ctok_wp_trainer_info); extension."""
        st = _n.WpTrainerStats()
        rc = _n.lib.ctok_wp_trainer_stats(self._h, ctypes.byref(st))
        if rc:
            _raise(rc)
        return {name: getattr(st, name) for name, _ in st._fields_}

    def pair_counts(self) -> dict:
        """Debug: the device's live pair table after the last training as {(a, b): count}."""
        a, b = _n.BpeStrings(), _n.BpeStrings()
        c = ctypes.POINTER(ctypes.c_int64)()
        rc = _n.lib.ctok_wp_trainer_pair_counts(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        if rc:
            _raise(rc)
        return dict(zip(zip(_strings(a), _strings(b)), _array(c, int(a.n))))
