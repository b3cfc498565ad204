"""`complexity_tokenizer.PreTokenizer` (reference src/bindings/components.rs:89-173 over
src/pretokenizers.rs:69-594) on the GPU, through include/ctok_pretokenizer.h.

The ten constructors and `pre_tokenize(text)` are the reference's.  A pre-tokenizer is a program of
steps that a whole batch goes through on the device in one call (csrc/pretok.hip), every step over
every word of the step before, quirks included: `punctuation`, `digits`, `gpt2` and `split` keep
whitespace, `punctuation` and `bert` use the reference's fixed range list, `unicode_scripts` its own
12-way table, and `split` hands an empty text on as one empty word.  There is no CPU fallback:
without a HIP device the constructors raise DeviceError.  A `split` pattern the Rust regex crate
rejects is the identity, as in the reference; one it compiles runs when it is a literal or one class
atom (`\\s \\S \\d \\D \\p{L} \\P{L} \\p{N} \\P{N}` or a bracket class of at most 32 items) with an optional
`+`, and raises UnsupportedConfigError otherwise, unless `split(..., regex=True)` asks for the general
engine: then a pattern of literals, `.`, those class atoms, concatenation, `|`, groups and
`? * + {n} {n,} {n,m}` (greedy or lazy) that cannot match the empty string runs as a DFA on the
device, leftmost-first as the crate matches (`split_plan` says how a pattern would run, `limits` what
bounds the engine).  A batch whose input, or any step's output, reaches
4 GiB raises RuntimeError.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as _n
from .bpe_trainer import _raise
from .normalizers import _bool_arg, _str_arg

_KINDS = {"whitespace": 0, "whitespace_split": 1, "byte_level": 2, "metaspace": 3, "punctuation": 4, "digits": 5, "gpt2": 6,
          "bert": 7, "char_delimiter_split": 8, "unicode_scripts": 9, "split": 10}
_BEHAVIORS = {"Removed": 0, "Isolated": 1, "MergedWithPrevious": 2, "MergedWithNext": 3, "Contiguous": 4}
_REGEX = 16  # CTOK_PRETOK_REGEX
_GATES = ("rejected", "literal", "class", "unsupported", "dfa")


def _char_arg(name, v):
    """PyO3 `char`: a str of exactly one code point."""
    if not isinstance(v, str):
        raise TypeError("argument '%s': '%s' object cannot be converted to 'PyString'" % (name, type(v).__name__))
    if len(v) != 1:
        raise ValueError("argument '%s': expected a string of length 1" % name)
    v.encode("utf-8")  # (a lone surrogate is no char: UnicodeEncodeError, a ValueError)
    return ord(v)


class PreTokenizer:
    """A pre-tokenizer; made by the static constructors, as in the reference."""

    def __init__(self, steps, device=0, repr_="PreTokenizer"):
        # steps: [(kind, flags, a: bytes, cp)] of include/ctok_pretokenizer.h
        self._steps = list(steps)
        self._repr = repr_
        self.device = device
        self.last_stats = {}
        arr = (_n.PretokStep * max(len(self._steps), 1))()
        keep = []
        for i, (kind, flags, a, cp) in enumerate(self._steps):
            ba = ctypes.create_string_buffer(a, len(a) + 1)
            keep.append(ba)
            arr[i] = _n.PretokStep(kind, flags, ctypes.cast(ba, ctypes.c_void_p), len(a), cp)
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_pretokenizer_create(arr, len(self._steps), device, ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_n, "lib", None) if _n is not None else None  # (None at interpreter teardown)
        if h and lib is not None:
            lib.ctok_pretokenizer_destroy(h)
            self._h = None

    def __repr__(self):
        return self._repr

    # ---- the reference's constructors (src/bindings/components.rs:97-168) --------------------------------

    @staticmethod
    def whitespace(device=0) -> "PreTokenizer":
        return PreTokenizer([(_KINDS["whitespace"], 0, b"", 0)], device, "PreTokenizer.whitespace()")

    @staticmethod
    def byte_level(add_prefix_space=False, device=0) -> "PreTokenizer":
        """A ' ' before a non-empty text that does not start with one, the GPT-2 split without
        look-ahead, every byte through bytes_to_unicode."""
        f = 1 if _bool_arg("add_prefix_space", add_prefix_space) else 0
        return PreTokenizer([(_KINDS["byte_level"], f, b"", 0)], device, "PreTokenizer.byte_level(%r)" % (add_prefix_space,))

    @staticmethod
    def metaspace(replacement="▁", add_prefix_space=True, device=0) -> "PreTokenizer":
        """The replacement before every word it is given, ' ' becomes the replacement, then a split
        on whitespace other than the replacement."""
        cp = _char_arg("replacement", replacement)
        f = 1 if _bool_arg("add_prefix_space", add_prefix_space) else 0
        return PreTokenizer([(_KINDS["metaspace"], f, b"", cp)], device, "PreTokenizer.metaspace(%r, %r)" % (replacement, add_prefix_space))

    @staticmethod
    def punctuation(device=0) -> "PreTokenizer":
        return PreTokenizer([(_KINDS["punctuation"], 0, b"", 0)], device, "PreTokenizer.punctuation()")

    @staticmethod
    def digits(individual_digits=False, device=0) -> "PreTokenizer":
        f = 1 if _bool_arg("individual_digits", individual_digits) else 0
        return PreTokenizer([(_KINDS["digits"], f, b"", 0)], device, "PreTokenizer.digits(%r)" % (individual_digits,))

    @staticmethod
    def gpt2(device=0) -> "PreTokenizer":
        return PreTokenizer([(_KINDS["gpt2"], 0, b"", 0)], device, "PreTokenizer.gpt2()")

    @staticmethod
    def bert(device=0) -> "PreTokenizer":
        return PreTokenizer([(_KINDS["bert"], 0, b"", 0)], device, "PreTokenizer.bert()")

    @staticmethod
    def char_delimiter_split(delimiter, device=0) -> "PreTokenizer":
        cp = _char_arg("delimiter", delimiter)
        return PreTokenizer([(_KINDS["char_delimiter_split"], 0, b"", cp)], device, "PreTokenizer.char_delimiter_split(%r)" % (delimiter,))

    @staticmethod
    def unicode_scripts(device=0) -> "PreTokenizer":
        return PreTokenizer([(_KINDS["unicode_scripts"], 0, b"", 0)], device, "PreTokenizer.unicode_scripts()")

    @staticmethod
    def split(pattern, behavior="Removed", invert=False, device=0, *, regex=False) -> "PreTokenizer":
        """SplitWithBehavior; a behavior string that names none means Removed (components.rs:154-160).
        regex=True (extension): a pattern that is neither a literal nor a class atom runs as a DFA
        where the engine takes it (see `split_plan`); a literal or class atom keeps its path."""
        a = _str_arg("pattern", pattern)
        if not isinstance(behavior, str):
            raise TypeError("argument 'behavior': '%s' object cannot be converted to 'PyString'" % type(behavior).__name__)
        f = _BEHAVIORS.get(behavior, 0) | (8 if _bool_arg("invert", invert) else 0) | (_REGEX if _bool_arg("regex", regex) else 0)
        return PreTokenizer([(_KINDS["split"], f, a, 0)], device,
                            "PreTokenizer.split(%r, %r, %r%s)" % (pattern, behavior, invert, ", regex=True" if regex else ""))

    # ---- extensions --------------------------------------------------------------------------------------

    @staticmethod
    def whitespace_split(device=0) -> "PreTokenizer":
        """PreTokenizer::WhitespaceSplit of the reference's enum, which its Python class does not reach; extension."""
        return PreTokenizer([(_KINDS["whitespace_split"], 0, b"", 0)], device, "PreTokenizer.whitespace_split()")

    @staticmethod
    def sequence(pretokenizers, device=0) -> "PreTokenizer":
        """PreTokenizer::Sequence: every pre-tokenizer over every word of the one before (nested
        sequences are flattened); extension."""
        if isinstance(pretokenizers, (str, bytes)):
            raise TypeError("argument 'pretokenizers': Can't extract `str` to `Vec`")
        steps, names = [], []
        for p in pretokenizers:
            if not isinstance(p, PreTokenizer):
                raise TypeError("argument 'pretokenizers': '%s' object cannot be converted to 'PreTokenizer'" % type(p).__name__)
            steps += p._steps
            names.append(repr(p))
        return PreTokenizer(steps, device, "PreTokenizer.sequence([%s])" % ", ".join(names))

    @staticmethod
    def split_plan(pattern) -> dict:
        """How `split(pattern, ..., regex=True)` would run, without a device: `gate` is "rejected" (the
        Rust crate refuses the pattern: the identity), "literal", "class", "dfa" or "unsupported" (with
        `reason` naming the refused construct); for "dfa" the symbols, states and NFA states of the
        compiled pattern, whether its matches are unbounded (`cyclic`: `limits()["max_regex_run"]` then
        applies), else the longest match in code points, and where the kernels keep the table; extension."""
        a = _str_arg("pattern", pattern)
        info = _n.PretokSplitInfo()
        rc = _n.lib.ctok_pretok_split_plan(a, len(a), ctypes.byref(info))
        if rc:
            _raise(rc)
        return {"gate": _GATES[info.gate], "n_symbols": info.n_symbols, "n_states": info.n_states, "n_nfa": info.n_nfa,
                "cyclic": bool(info.cyclic), "longest_match": int(info.longest_match), "table_bytes": int(info.table_bytes),
                "table_in_lds": bool(info.table_in_lds), "reason": info.reason.decode("utf-8", "replace")}

    @staticmethod
    def limits() -> dict:
        """The bounds of the `regex=True` engine: `max_regex_run` (the code points a match of a pattern
        with unbounded matches may run inside one word; CTOK_PRETOK_MAX_REGEX_RUN lowers it), the
        compiler's caps and the kernels' table threshold and scan tiles; extension."""
        lim = _n.PretokLimits()
        rc = _n.lib.ctok_pretok_limits(ctypes.byref(lim))
        if rc:
            _raise(rc)
        return {k: int(getattr(lim, k)) for k, _ in lim._fields_}

    def _with_regex(self) -> "PreTokenizer":
        """This pre-tokenizer with regex=True on every `split`."""
        steps = [(k, f | _REGEX if k == _KINDS["split"] else f, a, cp) for k, f, a, cp in self._steps]
        if steps == self._steps:
            return self
        return PreTokenizer(steps, self.device, self._repr + ".with_regex()")

    def pre_tokenize(self, text) -> list:
        """src/bindings/components.rs:170-172"""
        if not isinstance(text, str):
            raise TypeError("argument 'text': '%s' object cannot be converted to 'PyString'" % type(text).__name__)
        return self.pre_tokenize_batch([text])[0]

    def pre_tokenize_batch(self, texts) -> list:
        """pre_tokenize of every text, the whole program in one device call; extension."""
        from . import pack_texts
        buf, off = pack_texts(texts)
        words, word_off, text_word = self.pre_tokenize_packed(buf, off)
        raw, wo, tw = words.tobytes(), word_off.tolist(), text_word.tolist()
        return [[raw[wo[j]:wo[j + 1]].decode("utf-8") for j in range(tw[i], tw[i + 1])] for i in range(len(tw) - 1)]

    def pre_tokenize_packed(self, text_u8, off_u64):
        """(uint8 words, uint64 word_off[n_words + 1], uint64 text_word[n_texts + 1]) of a packed batch
        (text i = text_u8[off[i]:off[i + 1]], UTF-8): word j is words[word_off[j]:word_off[j + 1]], text i
        owns words text_word[i] .. text_word[i + 1]; extension."""
        text = np.ascontiguousarray(text_u8, dtype=np.uint8)
        off = np.ascontiguousarray(off_u64, dtype=np.uint64)
        if off.ndim != 1 or off.size < 1 or text.ndim != 1:
            raise ValueError("pre_tokenize_packed: text_u8 and off_u64 must be 1-D, off_u64 with n + 1 entries")
        n = off.size - 1
        if int(off[n]) > text.size:
            raise ValueError("pre_tokenize_packed: the offsets reach past the text")
        text_word = np.zeros(n + 1, dtype=np.uint64)
        nb, nw = ctypes.c_uint64(), ctypes.c_uint64()
        cap_b, cap_w = int(off[n]) + 64, int(off[n]) // 2 + n + 64  # (the library says what it needs)
        for _ in range(2):
            words = np.empty(cap_b, dtype=np.uint8)
            word_off = np.zeros(cap_w + 1, dtype=np.uint64)
            rc = _n.lib.ctok_pretokenizer_run(self._h, text.ctypes.data, off.ctypes.data, n, words.ctypes.data, cap_b,
                                              word_off.ctypes.data, cap_w, text_word.ctypes.data, ctypes.byref(nb), ctypes.byref(nw))
            if rc != _n.CTOK_E_CAPACITY or (nb.value <= cap_b and nw.value <= cap_w):
                break
            cap_b, cap_w = max(cap_b, int(nb.value)), max(cap_w, int(nw.value))
        if rc:
            _raise(rc)
        self._read_stats()
        return words[:int(nb.value)], word_off[:int(nw.value) + 1], text_word

    def pre_tokenize_packed_device(self, text_ptr, off_ptr, n_texts, n_bytes, words_ptr, words_cap, word_off_ptr, word_cap,
                                   text_word_ptr, stream=0):
        """The same over raw device pointers (ints; e.g. torch tensors' data_ptr()) of this
        pre-tokenizer's device, ordered on the HIP stream `stream` (0: the default stream).  words_ptr
        has room for words_cap bytes, word_off_ptr for word_cap + 1 uint64, text_word_ptr for
        n_texts + 1.  Returns (bytes, words); raises BufferError carrying `.needed_bytes` and
        `.needed_words` when a capacity is too small, with nothing written.  The bytes are taken as
        they are (what is not UTF-8 passes through).  Returns after the work is done; extension."""
        nb, nw = ctypes.c_uint64(), ctypes.c_uint64()
        rc = _n.lib.ctok_pretokenizer_run_device(self._h, text_ptr, off_ptr, n_texts, n_bytes, words_ptr, words_cap, word_off_ptr,
                                                 word_cap, text_word_ptr, ctypes.byref(nb), ctypes.byref(nw), stream)
        if rc == _n.CTOK_E_CAPACITY and (nb.value > words_cap or nw.value > word_cap):
            e = BufferError("pre_tokenize_packed_device: the words need %d bytes and %d offsets, the capacities are %d and %d"
                            % (nb.value, nw.value, words_cap, word_cap))
            e.needed_bytes, e.needed_words = int(nb.value), int(nw.value)
            raise e
        if rc:
            _raise(rc)
        self._read_stats()
        return int(nb.value), int(nw.value)

    def _read_stats(self):
        info = _n.PretokInfo()
        n = ctypes.c_uint64()
        _n.lib.ctok_pretokenizer_stats(self._h, ctypes.byref(info))
        _n.lib.ctok_pretokenizer_stage_ms(self._h, None, 0, ctypes.byref(n))
        ms = (ctypes.c_double * max(int(n.value), 1))()
        _n.lib.ctok_pretokenizer_stage_ms(self._h, ms, int(n.value), ctypes.byref(n))
        self.last_stats = {k: int(getattr(info, k)) for k, _ in info._fields_}
        self.last_stats["stages"] = [(_n.lib.ctok_pretokenizer_stage_name(self._h, i).decode(), ms[i]) for i in range(int(n.value))]
