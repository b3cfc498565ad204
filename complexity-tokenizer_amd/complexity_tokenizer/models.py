"""`complexity_tokenizer.WordLevelModel`, `CharBpeModel` and `ByteLevelBpeModel` (reference
src/bindings/models.rs:89-214 over src/models.rs:300-741) on the GPU, through include/ctok_models.h.

With WordPieceModel and UnigramModel these complete the reference's stand-alone models: the
(vocab, merges) pair `BpeTrainer.train()` returns goes straight into CharBpeModel or
ByteLevelBpeModel.  Encode runs on the GPU (csrc/strmerge.hip): the word split, the initial tokens
and the merge loop "lowest rank, leftmost, one merge per step" keyed on token strings, so a merge's
parts and result need not be vocab entries and a token outside the vocab becomes unk only at the
very end.  decode is host string work.  There is no CPU fallback: without a HIP device the
constructors raise DeviceError.  The one deliberate difference from the reference is the cap on a
word's symbols (include/ctok_models.h): a longer word raises UnsupportedConfigError.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as _n
from .bpe_trainer import _raise
from .wordpiece import _pack, _string, _uint

# Rust's char::is_whitespace: the 25 White_Space code points (csrc/ws_split_hd.h), not str.rstrip()'s set
_WHITE_SPACE = "".join(chr(c) for c in ([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B))
                                        + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000]))


def _bytes_to_unicode() -> dict:
    """src/models.rs:369-390: the GPT-2 byte map."""
    bs = list(range(0x21, 0x7F)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs = list(bs)
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {b: chr(c) for b, c in zip(bs, cs)}


_BYTE_DECODER = {c: b for b, c in _bytes_to_unicode().items()}


def from_utf8_lossy(raw: bytes) -> str:
    """String::from_utf8_lossy as a byte walk: one U+FFFD per maximal invalid subpart."""
    out = []
    i, n = 0, len(raw)

    def cont(k):
        return k < n and 0x80 <= raw[k] <= 0xBF

    while i < n:
        b = raw[i]
        if b < 0x80:
            out.append(chr(b))
            i += 1
            continue
        bad = 0  # bytes of the invalid subpart
        if 0xC2 <= b <= 0xDF:
            need = 2
            if not cont(i + 1):
                bad = 1
        elif 0xE0 <= b <= 0xEF:
            need = 3
            lo, hi = (0xA0, 0xBF) if b == 0xE0 else (0x80, 0x9F) if b == 0xED else (0x80, 0xBF)
            if not (i + 1 < n and lo <= raw[i + 1] <= hi):
                bad = 1
            elif not cont(i + 2):
                bad = 2
        elif 0xF0 <= b <= 0xF4:
            need = 4
            lo, hi = (0x90, 0xBF) if b == 0xF0 else (0x80, 0x8F) if b == 0xF4 else (0x80, 0xBF)
            if not (i + 1 < n and lo <= raw[i + 1] <= hi):
                bad = 1
            elif not cont(i + 2):
                bad = 2
            elif not cont(i + 3):
                bad = 3
        else:  # 80..C1, F5..FF
            need, bad = 1, 1
        if bad:
            out.append("\ufffd")
            i += bad
        else:
            out.append(raw[i:i + need].decode("utf-8"))
            i += need
    return "".join(out)


def _vocab_arg(vocab):
    if not isinstance(vocab, dict):
        raise TypeError("argument 'vocab': '%s' object cannot be converted to 'PyDict'" % type(vocab).__name__)
    keys, ids = [], []
    for k, v in vocab.items():
        if not isinstance(k, str):
            raise TypeError("argument 'vocab': '%s' object cannot be converted to 'PyString'" % type(k).__name__)
        keys.append(k.encode("utf-8"))
        ids.append(_uint("vocab", v, 0xFFFFFFFF))
    return keys, ids


def _merges_arg(merges):
    """PyO3 `Vec<(String, String)>`: a non-str sequence of 2-tuples of str."""
    if isinstance(merges, (str, bytes)):
        raise TypeError("argument 'merges': Can't extract `str` to `Vec`")
    try:
        items = list(merges)
    except TypeError:
        raise TypeError("argument 'merges': '%s' object cannot be converted to 'Sequence'" % type(merges).__name__) from None
    flat = []
    for m in items:
        if not isinstance(m, tuple):
            raise TypeError("argument 'merges': '%s' object cannot be converted to 'PyTuple'" % type(m).__name__)
        if len(m) != 2:
            raise ValueError("argument 'merges': expected tuple of length 2, but got tuple of length %d" % len(m))
        for x in m:
            if not isinstance(x, str):
                raise TypeError("argument 'merges': '%s' object cannot be converted to 'PyString'" % type(x).__name__)
            flat.append(x.encode("utf-8"))
    return items, flat


def models_limits() -> dict:
    """The engine's tier bounds and the cap on a word's symbols (ctok_models_limits); extension."""
    t1, t2, cap = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    _n.lib.ctok_models_limits(ctypes.byref(t1), ctypes.byref(t2), ctypes.byref(cap))
    return {"tier1": int(t1.value), "tier2": int(t2.value), "max_word_symbols": int(cap.value)}


class _Model:
    """What the three models share: the vocab, the handle and the batch calls."""

    _abi = ""  # "wl", "cbpe", "blbpe"

    def _set_vocab(self, vocab, ids):
        self._vocab = dict(zip(vocab.keys(), ids))
        self._vocab_r = {}
        for k in sorted(self._vocab, key=lambda s: s.encode("utf-8"), reverse=True):
            self._vocab_r[self._vocab[k]] = k  # among strings that share an id, the smallest keeps it

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_n, "lib", None) if _n is not None else None  # (None at interpreter teardown)
        if h and lib is not None:
            getattr(lib, "ctok_%s_model_destroy" % self._abi)(h)
            self._h = None

    def encode_batch_flat(self, texts):
        """(ids: uint32 array, offsets: uint64 array[len(texts) + 1]) of a batch; extension."""
        from . import pack_texts
        buf, off = pack_texts(texts)
        n = len(off) - 1
        ids, toff = ctypes.POINTER(ctypes.c_uint32)(), ctypes.POINTER(ctypes.c_uint64)()
        rc = getattr(_n.lib, "ctok_%s_model_encode_batch" % self._abi)(self._h, buf.ctypes.data, off.ctypes.data, n,
                                                                      ctypes.byref(ids), ctypes.byref(toff))
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
        if not isinstance(text, str):
            raise TypeError("argument 'text': '%s' object cannot be converted to 'PyString'" % type(text).__name__)
        return self.encode_batch([text])[0]

    def _tokens(self, ids):
        if isinstance(ids, (str, bytes)):
            raise TypeError("argument 'ids': Can't extract `str` to `Vec`")
        return [t for t in (self._vocab_r.get(_uint("ids", i, 0xFFFFFFFF)) for i in ids) if t is not None]

    def stage_ms(self) -> list:
        """HIP-event times of the last encode call by stage (ctok_models_stage_ms); extension."""
        out = (ctypes.c_double * 4)()
        rc = _n.lib.ctok_models_stage_ms(self._h, out)
        if rc:
            _raise(rc)
        return list(out)

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


class WordLevelModel(_Model):
    """WordLevelModel(vocab, unk_token="<unk>") -- src/bindings/models.rs:98-104."""

    _abi = "wl"

    def __init__(self, vocab, unk_token="<unk>", device=0):
        keys, ids = _vocab_arg(vocab)
        unk = _string("unk_token", unk_token)
        self._set_vocab(vocab, ids)
        self.device = device
        blob, off = _pack(keys)
        idv = np.asarray(ids, dtype=np.uint32)
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_wl_model_create(blob.ctypes.data, off.ctypes.data, idv.ctypes.data, len(keys), unk, device,
                                         ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def decode(self, ids) -> str:
        """src/models.rs:340-346: the known ids' strings joined by a space."""
        return " ".join(self._tokens(ids))


class CharBpeModel(_Model):
    """CharBpeModel(vocab, merges, end_of_word_suffix="</w>", unk_token="<unk>") --
    src/bindings/models.rs:137-148."""

    _abi = "cbpe"

    def __init__(self, vocab, merges, end_of_word_suffix="</w>", unk_token="<unk>", device=0):
        keys, ids = _vocab_arg(vocab)
        pairs, flat = _merges_arg(merges)
        suffix = _string("end_of_word_suffix", end_of_word_suffix)
        unk = _string("unk_token", unk_token)
        self._set_vocab(vocab, ids)
        self._merges = [tuple(p) for p in pairs]
        self._suffix = end_of_word_suffix
        self.device = device
        blob, off = _pack(keys)
        mblob, moff = _pack(flat)
        idv = np.asarray(ids, dtype=np.uint32)
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_cbpe_model_create(blob.ctypes.data, off.ctypes.data, idv.ctypes.data, len(keys), mblob.ctypes.data,
                                           moff.ctypes.data, len(flat), suffix, unk, device, ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def decode(self, ids) -> str:
        """src/models.rs:708-725: a token that ends with the suffix gives the token without it and a
        space (with an empty suffix every token does); then str::trim_end."""
        out = []
        for t in self._tokens(ids):
            if t.endswith(self._suffix):
                out.append(t[:len(t) - len(self._suffix)])
                out.append(" ")
            else:
                out.append(t)
        return "".join(out).rstrip(_WHITE_SPACE)

    def decode_batch(self, batch) -> list:
        """decode of every id list, in one pass over the batch on the GPU: Decoder.bpe(suffix) over the
        model's id -> token map, bound at the first call; extension."""
        dec = getattr(self, "_decoder", None)
        if dec is None:
            from .decoders import Decoder
            dec = Decoder.bpe(self._suffix, device=self.device)
            dec.set_vocab(self._vocab_r)
            self._decoder = dec
        return dec.decode_ids_batch(batch)


class ByteLevelBpeModel(_Model):
    """ByteLevelBpeModel(vocab, merges, unk_token="<unk>", add_prefix_space=True) --
    src/bindings/models.rs:181-192."""

    _abi = "blbpe"

    def __init__(self, vocab, merges, unk_token="<unk>", add_prefix_space=True, device=0):
        keys, ids = _vocab_arg(vocab)
        pairs, flat = _merges_arg(merges)
        unk = _string("unk_token", unk_token)
        if not isinstance(add_prefix_space, (bool, np.bool_)):
            raise TypeError("argument 'add_prefix_space': '%s' object cannot be converted to 'PyBool'"
                            % type(add_prefix_space).__name__)
        self._set_vocab(vocab, ids)
        self._merges = [tuple(p) for p in pairs]
        self.device = device
        blob, off = _pack(keys)
        mblob, moff = _pack(flat)
        idv = np.asarray(ids, dtype=np.uint32)
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_blbpe_model_create(blob.ctypes.data, off.ctypes.data, idv.ctypes.data, len(keys), mblob.ctypes.data,
                                            moff.ctypes.data, len(flat), unk, 1 if add_prefix_space else 0, device,
                                            ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def decode(self, ids) -> str:
        """src/models.rs:560-568: the tokens' chars back to bytes (chars outside the byte map are
        dropped), then String::from_utf8_lossy."""
        raw = bytes(_BYTE_DECODER[c] for t in self._tokens(ids) for c in t if c in _BYTE_DECODER)
        return from_utf8_lossy(raw)
