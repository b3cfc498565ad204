"""`complexity_tokenizer.Decoder` (reference src/bindings/components.rs:231-292 over
src/decoders.rs:30-243) on the GPU, through include/ctok_decoder.h.

The seven constructors and `decode(tokens)` are the reference's.  A decoder is a program of steps that
a whole batch of token lists goes through on the device in one call (csrc/decoder.hip), quirks
included: `wordpiece` puts a space before a token only when the result so far is non-empty and cleans
up with eight `str::replace` passes, `bpe` trims trailing white space, `byte_level` keeps ASCII outside
the byte map, drops every other char outside it and ends with `from_utf8_lossy`, and in a sequence
every step after the first sees its document as one token.  There is no CPU fallback: without a HIP
device the constructors raise DeviceError.  A batch whose input, or any step's output, reaches 4 GiB
raises RuntimeError.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as _n
from .bpe_trainer import _raise
from .normalizers import _bool_arg, _str_arg
from .pretokenizers import _char_arg
from .wordpiece import _uint

_KINDS = {"byte_level": 0, "metaspace": 1, "wordpiece": 2, "bpe": 3, "ctc": 4, "fuse": 5, "strip": 6, "replace": 7}
_MAX_ID = 1 << 27
_NO_ENTRY = 0xFFFFFFFF


def _tokens_arg(name, tokens):
    """PyO3 `Vec<String>`: a non-str sequence of str."""
    if isinstance(tokens, str):
        raise TypeError("argument '%s': Can't extract `str` to `Vec`" % name)
    if isinstance(tokens, (bytes, bytearray)):
        raise TypeError("argument '%s': '%s' object cannot be converted to 'PyString'" % (name, type(tokens).__name__))
    try:
        out = list(tokens)
    except TypeError:
        raise TypeError("argument '%s': '%s' object cannot be converted to 'Sequence'" % (name, type(tokens).__name__)) from None
    for t in out:
        if not isinstance(t, str):
            raise TypeError("argument '%s': '%s' object cannot be converted to 'PyString'" % (name, type(t).__name__))
    return out


def _batch_arg(name, batch):
    if isinstance(batch, (str, bytes, bytearray)):
        raise TypeError("argument '%s': Can't extract `str` to `Vec`" % name)
    try:
        return list(batch)
    except TypeError:
        raise TypeError("argument '%s': '%s' object cannot be converted to 'Sequence'" % (name, type(batch).__name__)) from None


def _unpack(text, off) -> list:
    raw, o = text.tobytes(), off.tolist()
    return [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]


class Decoder:
    """A decoder; made by the static constructors, as in the reference."""

    def __init__(self, steps, device=0, repr_="Decoder"):
        # steps: [(kind, flags, a: bytes, b: bytes, cp, start, stop)] of include/ctok_decoder.h
        self._steps = list(steps)
        self._repr = repr_
        self.device = device
        self.last_stats = {}
        self._has_vocab = False
        arr = (_n.DecStep * max(len(self._steps), 1))()
        keep = []
        for i, (kind, flags, a, b, cp, start, stop) in enumerate(self._steps):
            ba, bb = ctypes.create_string_buffer(a, len(a) + 1), ctypes.create_string_buffer(b, len(b) + 1)
            keep += [ba, bb]
            arr[i] = _n.DecStep(kind, flags, ctypes.cast(ba, ctypes.c_void_p), len(a), ctypes.cast(bb, ctypes.c_void_p), len(b), cp,
                                start, stop)
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_decoder_create(arr, len(self._steps), device, ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_n, "lib", None) if _n is not None else None  # (None at interpreter teardown)
        if h and lib is not None:
            lib.ctok_decoder_destroy(h)
            self._h = None

    def __repr__(self):
        return self._repr

    # ---- the reference's constructors (src/bindings/components.rs:239-287) --------------------------------

    @staticmethod
    def byte_level(device=0) -> "Decoder":
        """The tokens joined, every char of the GPT-2 byte map to its byte, any other ASCII char to
        itself, every other char dropped; then String::from_utf8_lossy."""
        return Decoder([(_KINDS["byte_level"], 0, b"", b"", 0, 0, 0)], device, "Decoder.byte_level()")

    @staticmethod
    def metaspace(replacement="▁", add_prefix_space=True, device=0) -> "Decoder":
        """The tokens joined, every replacement a ' '; with add_prefix_space one leading ' ' dropped."""
        cp = _char_arg("replacement", replacement)
        f = 1 if _bool_arg("add_prefix_space", add_prefix_space) else 0
        return Decoder([(_KINDS["metaspace"], f, b"", b"", cp, 0, 0)], device, "Decoder.metaspace(%r, %r)" % (replacement, add_prefix_space))

    @staticmethod
    def wordpiece(prefix="##", cleanup=True, device=0) -> "Decoder":
        """A token that starts with the prefix is appended without it, any other after a ' ' when the
        result so far is non-empty; cleanup: ' .' ' ,' ' !' ' ?' ' :' ' ;' " '" "' " lose their space, in
        that order."""
        a = _str_arg("prefix", prefix)
        f = 1 if _bool_arg("cleanup", cleanup) else 0
        return Decoder([(_KINDS["wordpiece"], f, a, b"", 0, 0, 0)], device, "Decoder.wordpiece(%r, %r)" % (prefix, cleanup))

    @staticmethod
    def bpe(suffix="</w>", device=0) -> "Decoder":
        """A token that ends with the suffix gives the token without it and a ' '; then str::trim_end."""
        a = _str_arg("suffix", suffix)
        return Decoder([(_KINDS["bpe"], 0, a, b"", 0, 0, 0)], device, "Decoder.bpe(%r)" % (suffix,))

    @staticmethod
    def ctc(pad_token="<pad>", word_delimiter_token=None, device=0) -> "Decoder":
        """Pad tokens dropped, the delimiter a ' ', a token that repeats the one before it dropped."""
        a = _str_arg("pad_token", pad_token)
        b = b"" if word_delimiter_token is None else _str_arg("word_delimiter_token", word_delimiter_token)
        f = 0 if word_delimiter_token is None else 1
        return Decoder([(_KINDS["ctc"], f, a, b, 0, 0, 0)], device, "Decoder.ctc(%r, %r)" % (pad_token, word_delimiter_token))

    @staticmethod
    def fuse(device=0) -> "Decoder":
        return Decoder([(_KINDS["fuse"], 0, b"", b"", 0, 0, 0)], device, "Decoder.fuse()")

    @staticmethod
    def strip(content=" ", start=0, stop=0, device=0) -> "Decoder":
        """The tokens joined, at most `start` copies of content off the front and then `stop` off the back."""
        cp = _char_arg("content", content)
        start = _uint("start", start, 0xFFFFFFFFFFFFFFFF)
        stop = _uint("stop", stop, 0xFFFFFFFFFFFFFFFF)
        return Decoder([(_KINDS["strip"], 0, b"", b"", cp, start, stop)], device, "Decoder.strip(%r, %r, %r)" % (content, start, stop))

    # ---- extensions --------------------------------------------------------------------------------------

    @staticmethod
    def replace(pattern, replacement, device=0) -> "Decoder":
        """Decoder::Replace of the reference's enum, which its Python class does not reach: the tokens
        joined, then str::replace with the literal pattern (no regex); extension."""
        a = _str_arg("pattern", pattern)
        b = _str_arg("replacement", replacement)
        return Decoder([(_KINDS["replace"], 0, a, b, 0, 0, 0)], device, "Decoder.replace(%r, %r)" % (pattern, replacement))

    @staticmethod
    def sequence(decoders, device=0) -> "Decoder":
        """Decoder::Sequence: after every decoder each document is one token, its text (nested
        sequences are flattened; the empty sequence is fuse); extension."""
        if isinstance(decoders, (str, bytes)):
            raise TypeError("argument 'decoders': Can't extract `str` to `Vec`")
        steps, names = [], []
        for d in decoders:
            if not isinstance(d, Decoder):
                raise TypeError("argument 'decoders': '%s' object cannot be converted to 'Decoder'" % type(d).__name__)
            steps += d._steps
            names.append(repr(d))
        if not steps:
            steps = [(_KINDS["fuse"], 0, b"", b"", 0, 0, 0)]
        return Decoder(steps, device, "Decoder.sequence([%s])" % ", ".join(names))

    def decode(self, tokens) -> str:
        """src/bindings/components.rs:289-291"""
        return self.decode_batch([_tokens_arg("tokens", tokens)])[0]

    def decode_batch(self, batch) -> list:
        """decode of every token list, the whole program in one device call; extension."""
        docs = [_tokens_arg("batch", t) for t in _batch_arg("batch", batch)]
        flat = [t.encode("utf-8") for d in docs for t in d]
        tok_off = np.zeros(len(flat) + 1, dtype=np.uint64)
        if flat:
            np.cumsum([len(t) for t in flat], out=tok_off[1:])
        doc_tok = np.zeros(len(docs) + 1, dtype=np.uint64)
        if docs:
            np.cumsum([len(d) for d in docs], out=doc_tok[1:])
        text, off = self.decode_packed(np.frombuffer(b"".join(flat), dtype=np.uint8), tok_off, doc_tok)
        return _unpack(text, off)

    def _run(self, call, n_docs, guess):
        text_off = np.zeros(n_docs + 1, dtype=np.uint64)
        nb = ctypes.c_uint64()
        text = np.empty(guess, dtype=np.uint8)
        rc = call(text.ctypes.data, guess, text_off.ctypes.data, ctypes.byref(nb))
        if rc == _n.CTOK_E_CAPACITY and nb.value > guess:
            # the guess was too small: the library says what it needs and keeps the result on the device
            cap = int(nb.value)
            text = np.empty(cap, dtype=np.uint8)
            rc = _n.lib.ctok_decoder_fetch(self._h, text.ctypes.data, cap, text_off.ctypes.data, ctypes.byref(nb))
        if rc:
            _raise(rc)
        self._read_stats()
        return text[:int(nb.value)], text_off

    def decode_packed(self, tokens_u8, tok_off_u64, doc_tok_u64):
        """(uint8 text, uint64 text_off[n_docs + 1]) of a packed batch: token j is
        tokens_u8[tok_off[j]:tok_off[j + 1]] (UTF-8), document i owns tokens doc_tok[i] .. doc_tok[i + 1] --
        the layout PreTokenizer.pre_tokenize_packed returns; extension."""
        tokens = np.ascontiguousarray(tokens_u8, dtype=np.uint8)
        tok_off = np.ascontiguousarray(tok_off_u64, dtype=np.uint64)
        doc_tok = np.ascontiguousarray(doc_tok_u64, dtype=np.uint64)
        if tokens.ndim != 1 or tok_off.ndim != 1 or doc_tok.ndim != 1 or tok_off.size < 1 or doc_tok.size < 1:
            raise ValueError("decode_packed: the arrays must be 1-D, the offsets with n + 1 entries")
        n_docs = doc_tok.size - 1
        if int(doc_tok[n_docs]) != tok_off.size - 1:
            raise ValueError("decode_packed: doc_tok must end at the number of tokens")
        if int(tok_off[-1]) > tokens.size:
            raise ValueError("decode_packed: the offsets reach past the tokens")
        return self._run(lambda t, cap, o, nb: _n.lib.ctok_decoder_run(self._h, tokens.ctypes.data, tok_off.ctypes.data,
                                                                     doc_tok.ctypes.data, n_docs, t, cap, o, nb),
                         n_docs, int(tok_off[-1]) + int(tok_off.size) + 64)

    def decode_packed_device(self, tokens_ptr, tok_off_ptr, doc_tok_ptr, n_docs, n_tokens, n_bytes, text_ptr, text_cap,
                             text_off_ptr, stream=0):
        """The same over raw device pointers (ints; e.g. torch tensors' data_ptr()) of this decoder's
        device, ordered on the HIP stream `stream` (0: the default stream).  text_ptr has room for
        text_cap bytes, text_off_ptr for n_docs + 1 uint64.  Returns the bytes; raises BufferError
        carrying `.needed_bytes` when the capacity is too small, with nothing written.  The bytes are
        taken as they are (what is not UTF-8 passes through as one-byte units).  Returns after the work
        is done; extension."""
        nb = ctypes.c_uint64()
        rc = _n.lib.ctok_decoder_run_device(self._h, tokens_ptr, tok_off_ptr, doc_tok_ptr, n_docs, n_tokens, n_bytes, text_ptr,
                                            text_cap, text_off_ptr, ctypes.byref(nb), stream)
        if rc == _n.CTOK_E_CAPACITY and nb.value > text_cap:
            e = BufferError("decode_packed_device: the texts need %d bytes, the capacity is %d" % (nb.value, text_cap))
            e.needed_bytes = int(nb.value)
            raise e
        if rc:
            _raise(rc)
        self._read_stats()
        return int(nb.value)

    def set_vocab(self, id_to_token) -> None:
        """The id -> token map of decode_ids_*: a dict[int, str] or a sequence of str indexed by id,
        uploaded once as a dense (offset, length) table and a byte pool; extension."""
        if isinstance(id_to_token, dict):
            items = [(_uint("id_to_token", k, 0xFFFFFFFF), v) for k, v in id_to_token.items()]
        else:
            items = list(enumerate(_tokens_arg("id_to_token", id_to_token)))
        for _, v in items:
            if not isinstance(v, str):
                raise TypeError("argument 'id_to_token': '%s' object cannot be converted to 'PyString'" % type(v).__name__)
        n = max((k for k, _ in items), default=-1) + 1
        if n > _MAX_ID:
            _n.lib.ctok_decoder_set_vocab(self._h, None, 0, None, None, n)  # (sets the message)
            _raise(_n.CTOK_E_CAPACITY)
        off = np.zeros(n, dtype=np.uint32)
        length = np.full(n, _NO_ENTRY, dtype=np.uint32)
        pool, at = [], 0
        for k, v in items:
            raw = v.encode("utf-8")
            off[k], length[k] = at, len(raw)
            pool.append(raw)
            at += len(raw)
            if at >= 1 << 32:
                break
        blob = np.frombuffer(b"".join(pool), dtype=np.uint8) if at < 1 << 32 else np.zeros(0, dtype=np.uint8)
        rc = _n.lib.ctok_decoder_set_vocab(self._h, blob.ctypes.data, at, off.ctypes.data, length.ctypes.data, n)
        if rc:
            _raise(rc)
        self._has_vocab = True

    def decode_ids_batch(self, batch) -> list:
        """decode of every id list through the vocabulary of set_vocab; an id with no entry is
        skipped; extension."""
        docs = []
        for ids in _batch_arg("batch", batch):
            if isinstance(ids, (str, bytes)):
                raise TypeError("argument 'batch': Can't extract `str` to `Vec`")
            docs.append([_uint("ids", i, 0xFFFFFFFF) for i in ids])
        off = np.zeros(len(docs) + 1, dtype=np.uint64)
        if docs:
            np.cumsum([len(d) for d in docs], out=off[1:])
        flat = np.fromiter((i for d in docs for i in d), dtype=np.uint32, count=int(off[-1]))
        return _unpack(*self.decode_ids_packed(flat, off))

    def decode_ids_packed(self, ids_u32, ids_off_u64):
        """(uint8 text, uint64 text_off[n_docs + 1]) of packed ids: document i owns
        ids[ids_off[i]:ids_off[i + 1]]; extension."""
        if not self._has_vocab:
            raise ValueError("decode_ids: no vocabulary, call set_vocab first")
        ids = np.ascontiguousarray(ids_u32, dtype=np.uint32)
        off = np.ascontiguousarray(ids_off_u64, dtype=np.uint64)
        if ids.ndim != 1 or off.ndim != 1 or off.size < 1:
            raise ValueError("decode_ids_packed: ids_u32 and ids_off_u64 must be 1-D, ids_off_u64 with n + 1 entries")
        n_docs = off.size - 1
        if int(off[n_docs]) > ids.size:
            raise ValueError("decode_ids_packed: the offsets reach past the ids")
        return self._run(lambda t, cap, o, nb: _n.lib.ctok_decoder_run_ids(self._h, ids.ctypes.data, off.ctypes.data, n_docs, t, cap,
                                                                         o, nb),
                         n_docs, 8 * int(ids.size) + 64)

    def _read_stats(self):
        info = _n.DecInfo()
        n = ctypes.c_uint64()
        _n.lib.ctok_decoder_stats(self._h, ctypes.byref(info))
        _n.lib.ctok_decoder_stage_ms(self._h, None, 0, ctypes.byref(n))
        ms = (ctypes.c_double * max(int(n.value), 1))()
        _n.lib.ctok_decoder_stage_ms(self._h, ms, int(n.value), ctypes.byref(n))
        self.last_stats = {k: int(getattr(info, k)) for k, _ in info._fields_}
        self.last_stats["stages"] = [(_n.lib.ctok_decoder_stage_name(self._h, i).decode(), ms[i]) for i in range(int(n.value))]
