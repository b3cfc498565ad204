"""`complexity_tokenizer.UnigramTrainer` and `complexity_tokenizer.UnigramModel` (reference
src/bindings/trainers.rs:156-215 over src/trainers.rs:287-546, src/bindings/models.rs:52-87 over
src/models.rs:150-299) on the GPU, through include/ctok_unigram.h.

The trainer's normaliser (NFC), its Metaspace pre-tokenizer, the substring counts, the lookup of
every vocab string at every char and the Viterbi search of every EM iteration run on the GPU
(csrc/unigram.hip), and so does the model's encode; the native host runtime keeps the strings, sorts
and takes the logarithms, and decode is host string work.  There is no CPU fallback: without a HIP
device the calls raise DeviceError.  The order the reference leaves to hash iteration (among equal
seed counts: ascending UTF-8 bytes), the panic rule and the -inf quirk are stated in the header.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as _n
from .bpe_trainer import _array, _raise, _strings
from .wordpiece import _pack, _string, _uint

DEFAULT_SPECIALS = ["<unk>", "<s>", "</s>"]
_USIZE = 0xFFFFFFFFFFFFFFFF


def _float(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise TypeError("argument '%s': must be real number, not %s" % (name, type(v).__name__))
    return float(v)


class UnigramModel:
    """UnigramModel(vocab, unk_token="<unk>") -- src/bindings/models.rs:60-64.  vocab is a list of
    (token, score); the id of a token is its index."""

    def __init__(self, vocab, unk_token="<unk>", device=0):
        if isinstance(vocab, (str, bytes)):
            raise TypeError("argument 'vocab': Can't extract `str` to `Vec`")
        toks, keys, scores = [], [], []
        for item in vocab:
            if not isinstance(item, tuple) or len(item) != 2:
                raise TypeError("argument 'vocab': items must be (str, float) tuples")
            t, s = item
            if not isinstance(t, str):
                raise TypeError("argument 'vocab': '%s' object cannot be converted to 'PyString'" % type(t).__name__)
            toks.append(t)
            keys.append(t.encode("utf-8"))
            scores.append(_float("vocab", s))
        unk = _string("unk_token", unk_token)
        self._list = list(zip(toks, scores))
        self._vocab = {t: i for i, t in enumerate(toks)}  # a repeated string keeps its last index
        self._vocab_r = dict(enumerate(toks))
        self.device = device
        blob, off = _pack(keys)
        sc = np.asarray(scores, dtype=np.float64)
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_uni_model_create(blob.ctypes.data, off.ctypes.data, sc.ctypes.data, len(keys), unk, device,
                                          ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_n, "lib", None) if _n is not None else None  # (None at interpreter teardown)
        if h and lib is not None:
            lib.ctok_uni_model_destroy(h)
            self._h = None

    def encode_batch_flat(self, texts):
        """(ids: uint32 array, offsets: uint64 array[len(texts) + 1]) of a batch; extension."""
        from . import pack_texts
        buf, off = pack_texts(texts)
        n = len(off) - 1
        ids, toff = ctypes.POINTER(ctypes.c_uint32)(), ctypes.POINTER(ctypes.c_uint64)()
        rc = _n.lib.ctok_uni_model_encode_batch(self._h, buf.ctypes.data, off.ctypes.data, n, ctypes.byref(ids),
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
        """src/models.rs:272-274: a Viterbi search over the chars of the whole text."""
        if not isinstance(text, str):
            raise TypeError("argument 'text': '%s' object cannot be converted to 'PyString'" % type(text).__name__)
        return self.encode_batch([text])[0]

    def decode(self, ids) -> str:
        """src/models.rs:277-283: the known ids' strings behind each other"""
        out = []
        for i in ids:
            token = self._vocab_r.get(_uint("ids", i, 0xFFFFFFFF))
            if token is not None:
                out.append(token)
        return "".join(out)

    @property
    def vocab_size(self) -> int:
        return len(self._vocab)

    def token_to_id(self, token):
        return self._vocab.get(token)

    def id_to_token(self, id):
        return self._vocab_r.get(id)

    def get_vocab(self) -> list:
        """A copy of the (token, score) list; extension."""
        return list(self._list)


class UnigramTrainer:
    """UnigramTrainer(vocab_size=8000, special_tokens=None, initial_vocab_size=1000000,
    shrinking_factor=0.75, n_iterations=16, max_piece_length=16) -- src/bindings/trainers.rs:164-196."""

    def __init__(self, vocab_size=8000, special_tokens=None, initial_vocab_size=1000000, shrinking_factor=0.75,
                 n_iterations=16, max_piece_length=16, device=0):
        vocab_size = _uint("vocab_size", vocab_size, _USIZE)
        initial_vocab_size = _uint("initial_vocab_size", initial_vocab_size, _USIZE)
        n_iterations = _uint("n_iterations", n_iterations, _USIZE)
        max_piece_length = _uint("max_piece_length", max_piece_length, _USIZE)
        shrinking_factor = _float("shrinking_factor", shrinking_factor)
        if special_tokens is None:
            special_tokens = DEFAULT_SPECIALS
        if isinstance(special_tokens, (str, bytes)):
            raise TypeError("argument 'special_tokens': Can't extract `str` to `Vec`")
        sp = [s.encode("utf-8") if isinstance(s, str) else None for s in special_tokens]
        if any(s is None for s in sp):
            raise TypeError("argument 'special_tokens': 'list' items must be str")
        off = np.zeros(len(sp) + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in sp], out=off[1:])
        cfg = _n.UniTrainerConfig(
            vocab_size=vocab_size, special=b"".join(sp), special_off=off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
            n_special=len(sp), initial_vocab_size=initial_vocab_size, shrinking_factor=shrinking_factor,
            n_iterations=n_iterations, max_piece_length=max_piece_length, device=device)
        self.device = device
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_uni_trainer_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_n, "lib", None) if _n is not None else None  # (None at interpreter teardown)
        if h and lib is not None:
            lib.ctok_uni_trainer_destroy(h)
            self._h = None

    @property
    def vocab_size(self) -> int:
        """The entries of the trainer's vocab, not the target (src/bindings/trainers.rs:211-214)."""
        return int(_n.lib.ctok_uni_trainer_vocab_size(self._h))

    def get_vocab(self) -> list:
        """The trainer's vocab as [(token, score)] in its order; extension."""
        vocab = _n.BpeStrings()
        score = ctypes.POINTER(ctypes.c_double)()
        rc = _n.lib.ctok_uni_trainer_result(self._h, ctypes.byref(vocab), ctypes.byref(score))
        if rc:
            _raise(rc)
        return list(zip(_strings(vocab), _array(score, int(vocab.n))))

    def _model(self) -> UnigramModel:
        # UnigramModel::new(self.vocab.clone(), "<unk>") :481
        return UnigramModel(self.get_vocab(), "<unk>", device=self.device)

    def train(self, files) -> UnigramModel:
        """src/trainers.rs:357-371: every BufRead::lines line of every file is a text of its own."""
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

    def train_from_iterator(self, texts) -> UnigramModel:
        """src/bindings/trainers.rs:205-209 -> src/trainers.rs:374-387"""
        from . import pack_texts
        buf, off = pack_texts(texts)
        rc = _n.lib.ctok_uni_trainer_train(self._h, buf.ctypes.data, off.ctypes.data, len(off) - 1)
        if rc:
            _raise(rc)
        return self._model()

    def train_sentences(self, sentences) -> UnigramModel:
        """train_from_sentences (src/trainers.rs:390-482) on sentences given directly (no normaliser,
        no split); extension."""
        if isinstance(sentences, (str, bytes)):
            raise TypeError("argument 'sentences': Can't extract `str` to `Vec`")
        ss = []
        for s in sentences:
            if not isinstance(s, str):
                raise TypeError("'%s' object cannot be converted to 'PyString'" % type(s).__name__)
            ss.append(s.encode("utf-8"))
        blob, off = _pack(ss)
        rc = _n.lib.ctok_uni_trainer_train_sentences(self._h, blob.ctypes.data, off.ctypes.data, len(ss))
        if rc:
            _raise(rc)
        return self._model()

    def sentences(self) -> list:
        """Debug: the last training's sentences, the device's pretokenize output."""
        v = _n.BpeStrings()
        rc = _n.lib.ctok_uni_trainer_sentences(self._h, ctypes.byref(v))
        if rc:
            _raise(rc)
        return _strings(v)

    def _counts(self, fn) -> dict:
        v = _n.BpeStrings()
        c = ctypes.POINTER(ctypes.c_uint64)()
        rc = fn(self._h, ctypes.byref(v), ctypes.byref(c))
        if rc:
            _raise(rc)
        return dict(zip(_strings(v), _array(c, int(v.n))))

    def substring_counts(self) -> dict:
        """Debug: the last training's substring counts, before the specials and the truncation."""
        return self._counts(_n.lib.ctok_uni_trainer_substring_counts)

    def expected_counts(self) -> dict:
        """Debug: the last E-step's {vocab string: times the segmentations used it}."""
        return self._counts(_n.lib.ctok_uni_trainer_expected_counts)

    def stats(self) -> dict:
        """What the last training did (ctok_uni_trainer_info); extension."""
        st = _n.UniTrainerStats()
        rc = _n.lib.ctok_uni_trainer_stats(self._h, ctypes.byref(st))
        if rc:
            _raise(rc)
        out = {name: getattr(st, name) for name, _ in st._fields_ if name != "vocab_sizes"}
        out["vocab_sizes"] = [int(st.vocab_sizes[i]) for i in range(int(st.iterations))]
        return out
