"""`complexity_tokenizer.BpeTrainer`: the classic frequency-BPE trainer (reference
src/bindings/trainers.rs:218-279 over src/bpe_trainer.rs) on the GPU, through include/ctok_bpe_trainer.h.

The whitespace word split, the word counts, the pair counts, the search for the most frequent pair
and every merge's pass over the words run on the GPU (csrc/bpe_train.hip, csrc/wordcount.hip); the
native host runtime keeps the strings.  There is no CPU fallback: without a HIP device the calls
raise DeviceError.  The two orders the reference leaves to hash iteration are fixed as the header
states: equal character frequencies in ascending code point order, equal pair counts by the
smallest pair of symbol ids.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as _n


def _raise(code):
    from . import _raise as r
    r(code)


def _strings(view) -> list:
    """A ctok_bpe_strings view as a list of str (copied: the view dies with the next call)."""
    n = int(view.n)
    if not n:
        return []
    off = np.ctypeslib.as_array(view.off, shape=(n + 1,)).tolist()
    raw = ctypes.string_at(view.bytes, off[n]) if off[n] else b""
    return [raw[off[i]:off[i + 1]].decode("utf-8") for i in range(n)]


def _array(ptr, n) -> list:
    return np.ctypeslib.as_array(ptr, shape=(n,)).tolist() if n else []


class BpeTrainer:
    """BpeTrainer(vocab_size=30000, min_frequency=2, special_tokens=None, show_progress=True,
    end_of_word_suffix=None, continuing_subword_prefix=None) -- src/bindings/trainers.rs:226-262."""

    def __init__(self, vocab_size=30000, min_frequency=2, special_tokens=None, show_progress=True,
                 end_of_word_suffix=None, continuing_subword_prefix=None, device=0):
        for name, v in (("vocab_size", vocab_size), ("min_frequency", min_frequency)):
            if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
                raise TypeError("argument '%s': '%s' object cannot be interpreted as an integer" % (name, type(v).__name__))
            if v < 0:
                raise OverflowError("argument '%s': can't convert negative int to unsigned" % name)
        if vocab_size > 0xFFFFFFFFFFFFFFFF:
            raise OverflowError("argument 'vocab_size': Python int too large to convert to C long")
        if min_frequency > 0xFFFFFFFF:
            raise OverflowError("argument 'min_frequency': out of range for u32")
        if special_tokens is None:
            special_tokens = ["<unk>", "<pad>", "<s>", "</s>"]
        if isinstance(special_tokens, (str, bytes)):
            raise TypeError("argument 'special_tokens': Can't extract `str` to `Vec`")
        sp = [s.encode("utf-8") if isinstance(s, str) else None for s in special_tokens]
        if any(s is None for s in sp):
            raise TypeError("argument 'special_tokens': 'list' items must be str")
        for name, v in (("end_of_word_suffix", end_of_word_suffix),
                        ("continuing_subword_prefix", continuing_subword_prefix)):
            if v is not None and not isinstance(v, str):
                raise TypeError("argument '%s': '%s' object cannot be converted to 'PyString'" % (name, type(v).__name__))
            if v is not None and "\0" in v:
                raise ValueError("argument '%s': embedded NUL" % name)
        off = np.zeros(len(sp) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in sp], out=off[1:])
        cfg = _n.BpeTrainerConfig(
            vocab_size=vocab_size, min_frequency=min_frequency, special=b"".join(sp),
            special_off=off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), n_special=len(sp),
            end_of_word_suffix=None if end_of_word_suffix is None else end_of_word_suffix.encode("utf-8"),
            continuing_subword_prefix=(None if continuing_subword_prefix is None
                                       else continuing_subword_prefix.encode("utf-8")),
            show_progress=1 if show_progress else 0, device=device)
        self._vocab_size = int(vocab_size)
        self._min_frequency = int(min_frequency)
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_bpe_trainer_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_n, "lib", None) if _n is not None else None  # (None at interpreter teardown)
        if h and lib is not None:
            lib.ctok_bpe_trainer_destroy(h)
            self._h = None

    @property
    def vocab_size(self) -> int:
        """The configured target (src/bindings/trainers.rs:270-273)."""
        return self._vocab_size

    @property
    def min_frequency(self) -> int:
        """src/bindings/trainers.rs:275-278."""
        return self._min_frequency

    def _result(self):
        vocab, merges = _n.BpeStrings(), _n.BpeStrings()
        ids = ctypes.POINTER(ctypes.c_uint32)()
        rc = _n.lib.ctok_bpe_trainer_result(self._h, ctypes.byref(vocab), ctypes.byref(ids), ctypes.byref(merges))
        if rc:
            _raise(rc)
        m = _strings(merges)
        return dict(zip(_strings(vocab), _array(ids, int(vocab.n)))), list(zip(m[0::2], m[1::2]))

    def train(self, texts):
        """train(texts) -> (vocab: dict[str, int], merges: list[tuple[str, str]])
        (src/bindings/trainers.rs:264-268 -> src/bpe_trainer.rs:100-228)."""
        from . import pack_texts
        buf, off = pack_texts(texts)
        rc = _n.lib.ctok_bpe_trainer_train(self._h, buf.ctypes.data, off.ctypes.data, len(off) - 1)
        if rc:
            _raise(rc)
        return self._result()

    def train_words(self, words):
        """The training of train() on a {word: frequency} dict given directly (the
        end_of_word_suffix is appended to the words here too); extension."""
        ws = []
        for w in words:
            if not isinstance(w, str):
                raise TypeError("'%s' object cannot be converted to 'PyString'" % type(w).__name__)
            ws.append(w.encode("utf-8"))
        fs = [int(words[w]) for w in words]
        if any(f < 0 or f > 0xFFFFFFFF for f in fs):
            raise OverflowError("a word frequency is out of range for u32")
        freqs = np.asarray(fs, dtype=np.uint32)
        off = np.zeros(len(ws) + 1, dtype=np.uint64)
        np.cumsum([len(w) for w in ws], out=off[1:])
        blob = np.frombuffer(b"".join(ws) + b"\0", dtype=np.uint8)
        rc = _n.lib.ctok_bpe_trainer_train_words(self._h, blob.ctypes.data, off.ctypes.data, freqs.ctypes.data, len(ws))
        if rc:
            _raise(rc)
        return self._result()

    def word_counts(self, texts) -> dict:
        """The split and count of train() alone: {word: count} of the texts, each split on
        White_Space by itself, before the end_of_word_suffix; extension."""
        from . import pack_texts
        buf, off = pack_texts(texts)
        rc = _n.lib.ctok_bpe_trainer_count(self._h, buf.ctypes.data, off.ctypes.data, len(off) - 1)
        if rc:
            _raise(rc)
        words = _n.BpeStrings()
        freqs = ctypes.POINTER(ctypes.c_uint32)()
        rc = _n.lib.ctok_bpe_trainer_word_counts(self._h, ctypes.byref(words), ctypes.byref(freqs))
        if rc:
            _raise(rc)
        return dict(zip(_strings(words), _array(freqs, int(words.n))))

    def stats(self) -> dict:
        """What the last training did (ctok_bpe_trainer_info, include/ctok_bpe_trainer.h); extension."""
        st = _n.BpeTrainerStats()
        rc = _n.lib.ctok_bpe_trainer_stats(self._h, ctypes.byref(st))
        if rc:
            _raise(rc)
        return {name: getattr(st, name) for name, _ in st._fields_}

    def symbols(self) -> list:
        """The symbol strings by symbol id (the ids the tie rule compares); extension."""
        v = _n.BpeStrings()
        rc = _n.lib.ctok_bpe_trainer_symbols(self._h, ctypes.byref(v))
        if rc:
            _raise(rc)
        return _strings(v)

    def pair_counts(self) -> dict:
        """Debug: the device's live pair table after the last training as {(first, second): count},
        pairs whose count fell to 0 dropped."""
        sym = self.symbols()
        a, b = ctypes.POINTER(ctypes.c_uint32)(), ctypes.POINTER(ctypes.c_uint32)()
        c = ctypes.POINTER(ctypes.c_int64)()
        n = ctypes.c_uint64()
        rc = _n.lib.ctok_bpe_trainer_pair_counts(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(n))
        if rc:
            _raise(rc)
        n = int(n.value)
        out = {}
        for x, y, v in zip(_array(a, n), _array(b, n), _array(c, n)):
            if v:
                out[(sym[x], sym[y])] = v
        return out
