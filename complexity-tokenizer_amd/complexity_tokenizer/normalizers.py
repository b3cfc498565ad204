"""`complexity_tokenizer.Normalizer` (reference src/bindings/components.rs:15-87 over
src/normalizers.rs:43-202) on the GPU, through include/ctok_normalizer.h.

The ten constructors and `normalize(text)` are the reference's.  A normaliser is a program of steps
that a whole batch goes through on the device in one call (csrc/normalize.hip, csrc/lowercase.hip):
the four Unicode normal forms, Lowercase, Strip, StripAccents, Replace, the BERT normaliser and
Precompiled, bit-exact with the reference's definitions under the Unicode 13.0 data of
csrc/gen/normalize_data.h.  There is no CPU fallback: without a HIP device the constructors raise
DeviceError.  Two refusals the reference does not have: a batch whose input, or any step's output,
reaches 4 GiB raises RuntimeError, and a program of more than 1024 primitive steps raises
UnsupportedConfigError.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

from . import _native as _n
from .bpe_trainer import _raise

_KINDS = {"nfc": 0, "nfd": 1, "nfkc": 2, "nfkd": 3, "lowercase": 4, "strip": 5, "strip_accents": 6, "replace": 7,
          "prepend": 8, "append": 9, "bert": 10, "precompiled": 11}


def _str_arg(name, v):
    if not isinstance(v, str):
        raise TypeError("argument '%s': '%s' object cannot be converted to 'PyString'" % (name, type(v).__name__))
    return v.encode("utf-8")


def _bool_arg(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise TypeError("argument '%s': '%s' object cannot be converted to 'PyBool'" % (name, type(v).__name__))
    return bool(v)


def _charsmap_arg(charsmap):
    """PyO3 `Vec<(String, String)>`: a non-str sequence of 2-tuples of str."""
    if isinstance(charsmap, (str, bytes)):
        raise TypeError("argument 'charsmap': Can't extract `str` to `Vec`")
    try:
        items = list(charsmap)
    except TypeError:
        raise TypeError("argument 'charsmap': '%s' object cannot be converted to 'Sequence'" % type(charsmap).__name__) from None
    out = []
    for m in items:
        if not isinstance(m, tuple):
            raise TypeError("argument 'charsmap': '%s' object cannot be converted to 'PyTuple'" % type(m).__name__)
        if len(m) != 2:
            raise ValueError("argument 'charsmap': expected tuple of length 2, but got tuple of length %d" % len(m))
        out.append((_str_arg("charsmap", m[0]), _str_arg("charsmap", m[1])))
    return out


class Normalizer:
    """A text normaliser; made by the static constructors, as in the reference."""

    def __init__(self, steps, device=0, repr_="Normalizer"):
        # steps: [(kind, flags, a: bytes, b: bytes)] of include/ctok_normalizer.h
        self._steps = list(steps)
        self._repr = repr_
        self.device = device
        self.last_stats = {}
        arr = (_n.NormStep * max(len(self._steps), 1))()
        keep = []
        for i, (kind, flags, a, b) in enumerate(self._steps):
            ba, bb = ctypes.create_string_buffer(a, len(a) + 1), ctypes.create_string_buffer(b, len(b) + 1)
            keep += [ba, bb]
            arr[i] = _n.NormStep(kind, flags, ctypes.cast(ba, ctypes.c_void_p), len(a), ctypes.cast(bb, ctypes.c_void_p), len(b))
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_normalizer_create(arr, len(self._steps), device, ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_n, "lib", None) if _n is not None else None  # (None at interpreter teardown)
        if h and lib is not None:
            lib.ctok_normalizer_destroy(h)
            self._h = None

    def __repr__(self):
        return self._repr

    # ---- the reference's constructors (src/bindings/components.rs:24-80) ---------------------------------

    @staticmethod
    def nfc(device=0) -> "Normalizer":
        return Normalizer([(_KINDS["nfc"], 0, b"", b"")], device, "Normalizer.nfc()")

    @staticmethod
    def nfd(device=0) -> "Normalizer":
        return Normalizer([(_KINDS["nfd"], 0, b"", b"")], device, "Normalizer.nfd()")

    @staticmethod
    def nfkc(device=0) -> "Normalizer":
        return Normalizer([(_KINDS["nfkc"], 0, b"", b"")], device, "Normalizer.nfkc()")

    @staticmethod
    def nfkd(device=0) -> "Normalizer":
        return Normalizer([(_KINDS["nfkd"], 0, b"", b"")], device, "Normalizer.nfkd()")

    @staticmethod
    def lowercase(device=0) -> "Normalizer":
        return Normalizer([(_KINDS["lowercase"], 0, b"", b"")], device, "Normalizer.lowercase()")

    @staticmethod
    def strip(device=0) -> "Normalizer":
        return Normalizer([(_KINDS["strip"], 0, b"", b"")], device, "Normalizer.strip()")

    @staticmethod
    def strip_accents(device=0) -> "Normalizer":
        return Normalizer([(_KINDS["strip_accents"], 0, b"", b"")], device, "Normalizer.strip_accents()")

    @staticmethod
    def replace(pattern, replacement, device=0) -> "Normalizer":
        """str::replace with a literal pattern; an empty pattern inserts the replacement before every
        char and at the end."""
        a, b = _str_arg("pattern", pattern), _str_arg("replacement", replacement)
        return Normalizer([(_KINDS["replace"], 0, a, b)], device, "Normalizer.replace(%r, %r)" % (pattern, replacement))

    @staticmethod
    def bert(clean_text=True, handle_chinese_chars=True, strip_accents=None, lowercase=True, device=0) -> "Normalizer":
        """clean_text, handle_chinese_chars, NFC (always), the StripAccents rule if strip_accents (None:
        if lowercase), lowercase -- in this order (src/normalizers.rs:59-92)."""
        flags = (1 if _bool_arg("clean_text", clean_text) else 0) | (2 if _bool_arg("handle_chinese_chars", handle_chinese_chars) else 0)
        if strip_accents is not None:
            flags |= 16 if _bool_arg("strip_accents", strip_accents) else 8
        flags |= 4 if _bool_arg("lowercase", lowercase) else 0
        return Normalizer([(_KINDS["bert"], flags, b"", b"")], device,
                          "Normalizer.bert(%r, %r, %r, %r)" % (clean_text, handle_chinese_chars, strip_accents, lowercase))

    @staticmethod
    def precompiled(charsmap, device=0) -> "Normalizer":
        """One replace per (from, to) entry, in list order, each over the whole result of the one before."""
        entries = _charsmap_arg(charsmap)
        blob = b"".join(struct.pack("<II", len(f), len(t)) + f + t for f, t in entries)
        return Normalizer([(_KINDS["precompiled"], 0, blob, b"")], device, "Normalizer.precompiled(<%d entries>)" % len(entries))

    # ---- extensions --------------------------------------------------------------------------------------

    @staticmethod
    def prepend(s, device=0) -> "Normalizer":
        """Normalizer::Prepend of the reference's enum, which its Python class does not reach; extension."""
        return Normalizer([(_KINDS["prepend"], 0, _str_arg("s", s), b"")], device, "Normalizer.prepend(%r)" % (s,))

    @staticmethod
    def append(s, device=0) -> "Normalizer":
        """Normalizer::Append of the reference's enum, which its Python class does not reach; extension."""
        return Normalizer([(_KINDS["append"], 0, _str_arg("s", s), b"")], device, "Normalizer.append(%r)" % (s,))

    @staticmethod
    def sequence(normalizers, device=0) -> "Normalizer":
        """Normalizer::Sequence: the normalisers one after another (nested sequences are flattened);
        extension."""
        if isinstance(normalizers, (str, bytes)):
            raise TypeError("argument 'normalizers': Can't extract `str` to `Vec`")
        steps, names = [], []
        for n in normalizers:
            if not isinstance(n, Normalizer):
                raise TypeError("argument 'normalizers': '%s' object cannot be converted to 'Normalizer'" % type(n).__name__)
            steps += n._steps
            names.append(repr(n))
        return Normalizer(steps, device, "Normalizer.sequence([%s])" % ", ".join(names))

    def normalize(self, text) -> str:
        """src/bindings/components.rs:83-85"""
        if not isinstance(text, str):
            raise TypeError("argument 'text': '%s' object cannot be converted to 'PyString'" % type(text).__name__)
        return self.normalize_batch([text])[0]

    def normalize_batch(self, texts) -> list:
        """normalize of every text, the whole program in one device call; extension."""
        from . import pack_texts
        buf, off = pack_texts(texts)
        out, out_off = self.normalize_packed(buf, off)
        raw, o = out.tobytes(), out_off.tolist()
        return [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]

    def normalize_packed(self, text_u8, off_u64):
        """(uint8 bytes, uint64 offsets[n + 1]) of a packed batch (text i = text_u8[off[i]:off[i + 1]],
        UTF-8), the whole program in one device call; extension."""
        text = np.ascontiguousarray(text_u8, dtype=np.uint8)
        off = np.ascontiguousarray(off_u64, dtype=np.uint64)
        if off.ndim != 1 or off.size < 1 or text.ndim != 1:
            raise ValueError("normalize_packed: text_u8 and off_u64 must be 1-D, off_u64 with n + 1 entries")
        n = off.size - 1
        if int(off[n]) > text.size:
            raise ValueError("normalize_packed: the offsets reach past the text")
        out_off = np.zeros(n + 1, dtype=np.uint64)
        cap = int(off[n]) + 64  # (most programs shrink or keep the text; the library says what it needs)
        for _ in range(2):
            out = np.empty(cap, dtype=np.uint8)
            rc = _n.lib.ctok_normalizer_run(self._h, text.ctypes.data, off.ctypes.data, n, out.ctypes.data, cap,
                                            out_off.ctypes.data)
            if rc != _n.CTOK_E_CAPACITY or int(out_off[n]) <= cap:
                break
            cap = int(out_off[n])
        if rc:
            _raise(rc)
        self._read_stats()
        return out[:int(out_off[n])], out_off

    def normalize_packed_device(self, text_ptr, off_ptr, n_texts, n_bytes, out_ptr, out_cap, out_off_ptr, stream=0) -> int:
        """The same over raw device pointers (ints; e.g. torch tensors' data_ptr()) of this
        normaliser's device, ordered on the HIP stream `stream` (0: the default stream; e.g.
        torch.cuda.Stream.cuda_stream).  out_ptr has room for out_cap bytes, out_off_ptr for
        n_texts + 1 uint64.  Returns the output's bytes; raises BufferError carrying the needed size
        as `.needed` when out_cap is too small, with nothing written.  The bytes are taken as they
        are (what is not UTF-8 passes through).  Returns after the work is done; extension."""
        needed = ctypes.c_uint64()
        rc = _n.lib.ctok_normalizer_run_device(self._h, text_ptr, off_ptr, n_texts, n_bytes, out_ptr, out_cap, out_off_ptr,
                                               ctypes.byref(needed), stream)
        if rc == _n.CTOK_E_CAPACITY and needed.value > out_cap:
            e = BufferError("normalize_packed_device: the output needs %d bytes, out_cap is %d" % (needed.value, out_cap))
            e.needed = int(needed.value)
            raise e
        if rc:
            _raise(rc)
        self._read_stats()
        return int(needed.value)

    def _read_stats(self):
        info = _n.NormInfo()
        n = ctypes.c_uint64()
        _n.lib.ctok_normalizer_stats(self._h, ctypes.byref(info))
        _n.lib.ctok_normalizer_stage_ms(self._h, None, 0, ctypes.byref(n))
        ms = (ctypes.c_double * max(int(n.value), 1))()
        _n.lib.ctok_normalizer_stage_ms(self._h, ms, int(n.value), ctypes.byref(n))
        self.last_stats = {k: int(getattr(info, k)) for k, _ in info._fields_}
        self.last_stats["stages"] = [(_n.lib.ctok_normalizer_stage_name(self._h, i).decode(), ms[i]) for i in range(int(n.value))]
