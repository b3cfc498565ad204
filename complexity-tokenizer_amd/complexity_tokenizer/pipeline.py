"""`PipelineTokenizer`: a BPE tokenizer.json with any normaliser, pre-tokenizer, decoder and
post-processor -- the reference's HuggingFaceTokenizer (src/huggingface/mod.rs:247-334, :551-613,
:711-769, :1080-1101 over src/huggingface/parsing.rs:10-364 and src/bpe.rs:52-153) -- on the GPU, through
include/ctok_pipeline.h.

`Tokenizer` runs the fused ByteLevel path and refuses every other file; this class chains the
stand-alone stages on the device instead: Normalizer -> PreTokenizer -> the id-keyed word BPE with the
added-token loop inside every word (csrc/wordbpe.hip), without a trip through host memory.  Decode
goes through the loaded Decoder (`Decoder.fuse()` when the file names none) over the vocabulary's
strings.  The quirks are the reference's: a char without a one-char vocab string is dropped, a pair's
new id is the filtered merge list's entry at the pair's unfiltered rank, and a pair whose rank is past
that list raises PanicException as soon as it stands adjacent in a word.  There is no CPU fallback.
Refusals the reference does not have are listed in include/ctok_pipeline.h.
"""
from __future__ import annotations

import ctypes
import json

import numpy as np

from . import _native as _n
from . import _as_str, _as_str_list, _extract_str_list, _raise, _split_lists, _split_pairs, pack_ids, pack_texts
from .decoders import Decoder
from .encoding import BatchEncoding, Encoding
from .models import _WHITE_SPACE
from .normalizers import Normalizer
from .postprocessors import PostProcessor
from .pretokenizers import PreTokenizer

# ---- src/huggingface/parsing.rs as a pure function -------------------------------------------------------


def _named(value):
    """A component that names its type: (object, type); else None, the default arm of parsing.rs."""
    if not isinstance(value, dict) or "type" not in value:
        return None
    return value, value["type"] if isinstance(value["type"], str) else ""


def _get(obj, key, kind, default):
    v = obj.get(key)
    if kind is int:
        return v if type(v) is int and 0 <= v < 1 << 64 else default  # serde_json as_u64
    return v if isinstance(v, kind) else default


def _first_char(obj, key, default):
    v = obj.get(key)
    return v[0] if isinstance(v, str) and len(v) > 0 else default


def _members(obj, key, parse):
    """A Sequence: members that parse to none are skipped; no array, or nothing left, is none."""
    v = obj.get(key)
    if not isinstance(v, list):
        return None
    kept = []
    for m in v:
        p = parse(m)
        if p is not None:
            kept.append(p)
    return ("sequence", kept) if kept else None


def _parse_normalizer(value):
    named = _named(value)
    if named is None:
        return ("nfc",)
    obj, t = named
    simple = {"NFC": "nfc", "NFD": "nfd", "NFKC": "nfkc", "NFKD": "nfkd", "Lowercase": "lowercase", "Strip": "strip",
              "StripAccents": "strip_accents"}
    if t in simple:
        return (simple[t],)
    if t == "Replace":
        pattern = obj.get("pattern")
        return ("replace", _get(pattern, "String", str, "") if isinstance(pattern, dict) else "", _get(obj, "content", str, ""))
    if t == "Prepend":
        return ("prepend", _get(obj, "prepend", str, ""))
    if t == "Sequence":
        return _members(obj, "normalizers", _parse_normalizer)
    if t == "BertNormalizer":
        return ("bert", _get(obj, "clean_text", bool, True), _get(obj, "handle_chinese_chars", bool, True),
                _get(obj, "strip_accents", bool, None), _get(obj, "lowercase", bool, True))
    if t == "Precompiled":
        # the reference keeps the charsmap string as one (s, s) entry: a replace of s by itself
        s = obj.get("precompiled_charsmap")
        return ("precompiled", [(s, s)] if isinstance(s, str) else [])
    return None


def _parse_pre_tokenizer(value):
    named = _named(value)
    if named is None:
        return ("byte_level", False)
    obj, t = named
    simple = {"Whitespace": "whitespace", "WhitespaceSplit": "whitespace_split", "Punctuation": "punctuation",
              "BertPreTokenizer": "bert", "UnicodeScripts": "unicode_scripts"}
    if t in simple:
        return (simple[t],)
    if t == "ByteLevel":
        return ("byte_level", _get(obj, "add_prefix_space", bool, False))
    if t == "Metaspace":
        return ("metaspace", _first_char(obj, "replacement", "▁"), _get(obj, "add_prefix_space", bool, True))
    if t == "CharDelimiterSplit":
        return ("char_delimiter_split", _first_char(obj, "delimiter", " "))
    if t == "Digits":
        return ("digits", _get(obj, "individual_digits", bool, False))
    if t == "Split":
        pattern = obj.get("pattern")
        behavior = _get(obj, "behavior", str, "Removed")
        if behavior not in ("Isolated", "MergedWithPrevious", "MergedWithNext", "Contiguous"):
            behavior = "Removed"
        return ("split", _get(pattern, "Regex", str, "") if isinstance(pattern, dict) else "", behavior, _get(obj, "invert", bool, False))
    if t == "Sequence":
        return _members(obj, "pretokenizers", _parse_pre_tokenizer)
    return None


def _parse_decoder(value):
    named = _named(value)
    if named is None:
        return ("byte_level",)
    obj, t = named
    if t == "ByteLevel":
        return ("byte_level",)
    if t == "Metaspace":
        return ("metaspace", _first_char(obj, "replacement", "▁"), _get(obj, "add_prefix_space", bool, True))
    if t == "WordPiece":
        return ("wordpiece", _get(obj, "prefix", str, "##"), _get(obj, "cleanup", bool, True))
    if t == "BPE":
        return ("bpe", _get(obj, "suffix", str, "</w>"))
    if t == "CTC":
        return ("ctc", _get(obj, "pad_token", str, "<pad>"), _get(obj, "word_delimiter_token", str, None))
    if t == "Fuse":
        return ("fuse",)
    if t == "Strip":
        return ("strip", _first_char(obj, "content", " "), _get(obj, "start", int, 0), _get(obj, "stop", int, 0))
    if t == "Sequence":
        return _members(obj, "decoders", _parse_decoder)
    return None


def _template_string(items):
    parts = []
    for item in items:
        if not isinstance(item, dict):
            continue
        if "SpecialToken" in item:
            inner = item["SpecialToken"]
            tid = inner.get("id") if isinstance(inner, dict) else None
            if isinstance(tid, str):
                parts.append(tid)
        elif "Sequence" in item:
            inner = item["Sequence"]
            sid = inner.get("id") if isinstance(inner, dict) else None
            if isinstance(sid, str):
                parts.append("$" + sid)
    return " ".join(parts)


def _parse_post_processor(value, special):
    named = _named(value)
    if named is None:
        return None
    obj, t = named
    if t == "TemplateProcessing":
        single, pair = obj.get("single"), obj.get("pair")
        return ("template", _template_string(single) if isinstance(single, list) else "<s> $A </s>",
                _template_string(pair) if isinstance(pair, list) else None, [(k, v) for k, v in special.items()])
    if t == "RobertaProcessing":
        return ("roberta", ("<s>", special.get("<s>", 0)), ("</s>", special.get("</s>", 2)), False)
    if t == "BertProcessing":
        return ("bert", ("[CLS]", special.get("[CLS]", 101)), ("[SEP]", special.get("[SEP]", 102)))
    return None


def _parse_merges(items):
    """deserialize_merges (mod.rs:56-101): strings as they are, arrays of two strings joined by ' ',
    anything else skipped; then only what splits into exactly two parts at ' ' (mod.rs:252-264)."""
    if not isinstance(items, list):
        raise IOError("invalid type for `merges`: a sequence of strings or arrays of two strings expected")
    out = []
    for item in items:
        if isinstance(item, list):
            if len(item) != 2 or not isinstance(item[0], str) or not isinstance(item[1], str):
                continue
            item = item[0] + " " + item[1]
        elif not isinstance(item, str):
            continue
        parts = item.split(" ")
        if len(parts) == 2:
            out.append((parts[0], parts[1]))
    return out


def parse_tokenizer_json(obj) -> dict:
    """The rules of from_tokenizer_json_with_config and parsing.rs over a parsed tokenizer.json, with no
    device: a spec of constructor calls.  `vocab` {str: id}, `merges` [(left, right)], `added_tokens`
    [dict], and the four components as nested tuples named after the constructors of Normalizer,
    PreTokenizer, Decoder and PostProcessor -- ("nfkc",), ("metaspace", "▁", True), ("sequence", [...])
    -- or None where the reference has none."""
    if not isinstance(obj, dict) or not isinstance(obj.get("model"), dict):
        raise IOError("missing field `model`")
    model = obj["model"]
    vocab = model.get("vocab")
    if not isinstance(vocab, dict):
        raise IOError("missing field `vocab`")
    for k, v in vocab.items():
        if type(v) is not int or not 0 <= v < 1 << 32:
            raise IOError("invalid value for vocab entry %r, expected u32" % (k,))
    added = []
    for t in obj.get("added_tokens") or []:
        if not isinstance(t, dict) or type(t.get("id")) is not int or not isinstance(t.get("content"), str) \
                or not isinstance(t.get("special"), bool):
            raise IOError("invalid added token: `id` (u32), `content` (string) and `special` (boolean) are required")
        added.append(dict(id=t["id"], content=t["content"], special=t["special"], single_word=_get(t, "single_word", bool, False),
                          lstrip=_get(t, "lstrip", bool, False), rstrip=_get(t, "rstrip", bool, False),
                          normalized=_get(t, "normalized", bool, False)))
    special = {}
    for t in added:
        if t["special"]:
            special[t["content"]] = t["id"]
    return {"vocab": dict(vocab), "merges": _parse_merges(model.get("merges", [])), "added_tokens": added,
            "normalizer": _parse_normalizer(obj.get("normalizer")), "pre_tokenizer": _parse_pre_tokenizer(obj.get("pre_tokenizer")),
            "decoder": _parse_decoder(obj.get("decoder")), "post_processor": _parse_post_processor(obj.get("post_processor"), special)}


def _build(cls, spec, device, regex_split=False):
    """The component object of a spec tuple (None stays None).  regex_split: every `split` of a
    PreTokenizer is made with regex=True."""
    if spec is None:
        return None
    kind = spec[0]
    if kind == "sequence":
        return cls.sequence([_build(cls, s, device, regex_split) for s in spec[1]], device=device)
    if cls is PreTokenizer and kind == "split" and regex_split:
        return PreTokenizer.split(*spec[1:], device=device, regex=True)
    if cls is PostProcessor:
        if kind == "template":
            return PostProcessor.template(spec[1], spec[2], list(spec[3]), device=device)
        if kind == "bert":
            return PostProcessor.bert(spec[1][0], spec[1][1], spec[2][0], spec[2][1], device=device)
        return PostProcessor.roberta(spec[1][0], spec[1][1], spec[2][0], spec[2][1], spec[3], device=device)
    return getattr(cls, kind)(*spec[1:], device=device)


_CLEANUP = ((" .", "."), (" ,", ","), (" !", "!"), (" ?", "?"), (" :", ":"), (" ;", ";"), ('" ', '"'), (' "', '"'), ("' ", "'"),
            (" '", "'"), ("( ", "("), (" )", ")"), ("[ ", "["), (" ]", "]"), (" - ", "-"))
_WS_TABLE = {ord(c): " " for c in _WHITE_SPACE}


def _clean_up(text: str) -> str:
    """clean_up_tokenization_spaces (mod.rs:749-769): fifteen replaces, then split_whitespace with
    Rust's white-space set, joined by ' '.  Host string work."""
    for a, b in _CLEANUP:
        text = text.replace(a, b)
    return " ".join(w for w in text.translate(_WS_TABLE).split(" ") if w)


class PipelineTokenizer:
    """A BPE tokenizer with any normaliser and pre-tokenizer whose encode runs on an MI355X."""

    def __init__(self, vocab, merges, normalizer, pre_tokenizer, decoder, post_processor, added_tokens, device):
        self._vocab = dict(vocab)
        self._id_to_token = {v: k for k, v in self._vocab.items()}
        self._normalizer, self._pre_tokenizer, self._decoder, self._post_processor = normalizer, pre_tokenizer, decoder, post_processor
        self._added = [dict(t) for t in added_tokens]
        self._special = {t["content"]: t["id"] for t in self._added if t.get("special", False)}
        self._special_ids = None
        self._decode_with = None
        self.device = device
        self.last_stats = None
        self._model_max_length = 512  # from_tokenizer_json without a tokenizer_config.json (mod.rs:226)
        self._padding_side = self._truncation_side = "right"  # mod.rs:325-326
        keys = [k.encode("utf-8") for k in self._vocab]
        ms = [s.encode("utf-8") for ab in merges for s in ab]
        ab = [t["content"].encode("utf-8") for t in self._added]

        def packed(items):
            off = np.zeros(len(items) + 1, dtype=np.uint64)
            if items:
                np.cumsum([len(x) for x in items], out=off[1:])
            return np.frombuffer(b"".join(items) + b"\0" * 16, dtype=np.uint8), off

        vb, voff = packed(keys)
        mb, moff = packed(ms)
        abb, aoff = packed(ab)
        vid = np.asarray(list(self._vocab.values()) + [0], dtype=np.uint32)
        aid = np.asarray([int(t["id"]) for t in self._added] + [0], dtype=np.uint32)
        bits = {"special": 1, "single_word": 2, "lstrip": 4, "rstrip": 8, "normalized": 16}
        afl = np.asarray([sum(v for k, v in bits.items() if t.get(k, False)) for t in self._added] + [0], dtype=np.uint8)
        tb = _n.PipelineTables(vb.ctypes.data, voff.ctypes.data, vid.ctypes.data, len(keys), mb.ctypes.data, moff.ctypes.data, len(ms),
                               abb.ctypes.data, aoff.ctypes.data, aid.ctypes.data, afl.ctypes.data, len(ab))
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_pipeline_create(ctypes.byref(tb), normalizer._h if normalizer is not None else None,
                                         pre_tokenizer._h if pre_tokenizer is not None else None, device, ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_n, "lib", None) if _n is not None else None  # (None at interpreter teardown)
        if h and lib is not None:
            lib.ctok_pipeline_destroy(h)
            self._h = None

    def __repr__(self):
        return "PipelineTokenizer(vocab_size=%d, normalizer=%r, pre_tokenizer=%r, device=%d)" % (
            self.vocab_size, self._normalizer, self._pre_tokenizer, self.device)

    # ------------------------------------------------------------------ constructors
    @staticmethod
    def from_components(vocab, merges, normalizer=None, pre_tokenizer=None, decoder=None, post_processor=None, added_tokens=(),
                        device=None, regex_split=False) -> "PipelineTokenizer":
        """vocab {token: id}; merges [(left, right)] in rank order; the components are Normalizer,
        PreTokenizer, Decoder and PostProcessor objects or None (no normaliser; the whole text is one
        word; the vocab strings joined; no post-processor); added_tokens are dicts with the
        tokenizer.json fields.  All components must be on one device (ValueError otherwise).
        regex_split: every `split` of the pre-tokenizer runs as PreTokenizer.split(..., regex=True)."""
        for name, c, cls in (("normalizer", normalizer, Normalizer), ("pre_tokenizer", pre_tokenizer, PreTokenizer),
                             ("decoder", decoder, Decoder), ("post_processor", post_processor, PostProcessor)):
            if c is not None and not isinstance(c, cls):
                raise TypeError("argument '%s': '%s' object cannot be converted to '%s'" % (name, type(c).__name__, cls.__name__))
        if regex_split and pre_tokenizer is not None:
            pre_tokenizer = pre_tokenizer._with_regex()
        devs = {c.device for c in (normalizer, pre_tokenizer, decoder, post_processor) if c is not None}
        if device is not None:
            devs.add(int(device))
        if len(devs) > 1:
            raise ValueError("from_components: the components are on devices %s; all must be on one" % sorted(devs))
        merges = [(a, b) for a, b in merges]
        for a, b in merges:
            if not isinstance(a, str) or not isinstance(b, str):
                raise TypeError("argument 'merges': expected pairs of str")
        added = []
        for t in added_tokens:
            if not isinstance(t, dict) or "id" not in t or not isinstance(t.get("content"), str):
                raise TypeError("argument 'added_tokens': expected dicts with `id` and `content`")
            added.append(t)
        return PipelineTokenizer(vocab, merges, normalizer, pre_tokenizer, decoder, post_processor, added, devs.pop() if devs else 0)

    @staticmethod
    def from_spec(spec: dict, device: int = 0, regex_split: bool = False) -> "PipelineTokenizer":
        """From what parse_tokenizer_json returns.  A `split` pattern PreTokenizer cannot run raises
        UnsupportedConfigError, as it does there; regex_split=True makes every `split` with regex=True,
        so that a general pattern runs where PreTokenizer's engine takes it."""
        return PipelineTokenizer.from_components(
            spec["vocab"], spec["merges"], _build(Normalizer, spec["normalizer"], device),
            _build(PreTokenizer, spec["pre_tokenizer"], device, regex_split),
            _build(Decoder, spec["decoder"], device), _build(PostProcessor, spec["post_processor"], device), spec["added_tokens"], device)

    @staticmethod
    def from_str(json_text: str, device: int = 0, regex_split: bool = False) -> "PipelineTokenizer":
        """HuggingFaceTokenizer::from_str (mod.rs:168-173)."""
        try:
            obj = json.loads(json_text)
        except ValueError as e:
            raise IOError(str(e)) from None
        return PipelineTokenizer.from_spec(parse_tokenizer_json(obj), device, regex_split)

    @staticmethod
    def from_file(path: str, device: int = 0, regex_split: bool = False) -> "PipelineTokenizer":
        """HuggingFaceTokenizer::from_file (mod.rs:159-166)."""
        with open(path, "r", encoding="utf-8") as f:
            return PipelineTokenizer.from_str(f.read(), device, regex_split)

    # ------------------------------------------------------------------ getters
    @property
    def vocab_size(self) -> int:
        return len(self._vocab)

    def token_to_id(self, token: str):
        return self._vocab.get(token)

    def id_to_token(self, id: int):
        return self._id_to_token.get(id)

    @property
    def special_tokens(self) -> dict:
        return dict(self._special)

    @property
    def normalizer(self):
        return self._normalizer

    @property
    def pre_tokenizer(self):
        return self._pre_tokenizer

    @property
    def decoder(self):
        return self._decoder

    @property
    def post_processor(self):
        """The loaded PostProcessor or None: chain it with process_packed / process_padded over what
        encode_batch_flat returns."""
        return self._post_processor

    @staticmethod
    def limits(handle=None) -> dict:
        lim = _n.PipelineLimits()
        _n.lib.ctok_pipeline_limits(handle, ctypes.byref(lim))
        return {k: int(getattr(lim, k)) for k, _ in lim._fields_}

    # ------------------------------------------------------------------ encode
    def _read_stats(self):
        ms = (ctypes.c_double * _n.CTOK_PIPELINE_STAGES)()
        info = _n.PipelineInfo()
        _n.lib.ctok_pipeline_stage_ms(self._h, ms)
        _n.lib.ctok_pipeline_stats(self._h, ctypes.byref(info))
        st = {k: int(getattr(info, k)) for k, _ in info._fields_}
        st["stages"] = [(_n.lib.ctok_pipeline_stage_name(i).decode(), ms[i]) for i in range(_n.CTOK_PIPELINE_STAGES)]
        self.last_stats = st

    def encode_packed(self, text, off, tokenize: bool = False):
        """A packed batch (uint8 UTF-8 buffer, uint64 offsets[D + 1]) -> (ids uint32[T], tok_off uint64[D + 1])."""
        text = np.ascontiguousarray(text, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        if off.ndim != 1 or off.size < 1 or text.ndim != 1:
            raise ValueError("encode_packed: text and off must be 1-D, off with n + 1 entries")
        n = off.size - 1
        if int(off[n]) > text.size:
            raise ValueError("encode_packed: the offsets reach past the text")
        ids_p, off_p = ctypes.c_void_p(), ctypes.c_void_p()
        rc = _n.lib.ctok_pipeline_encode_batch(self._h, text.ctypes.data, off.ctypes.data, n, _n.CTOK_PIPELINE_TOKENIZE if tokenize else 0,
                                               ctypes.byref(ids_p), ctypes.byref(off_p))
        if rc:
            _raise(rc)
        self._read_stats()
        tok_off = np.ctypeslib.as_array(ctypes.cast(off_p, ctypes.POINTER(ctypes.c_uint64)), shape=(n + 1,)).copy()
        total = int(tok_off[n])
        ids = np.ctypeslib.as_array(ctypes.cast(ids_p, ctypes.POINTER(ctypes.c_uint32)), shape=(total,)).copy() if total \
            else np.zeros(0, dtype=np.uint32)
        return ids, tok_off

    def encode_packed_device(self, d_text: int, d_off: int, n_docs: int, n_bytes: int, d_ids: int, ids_cap: int, d_tok_off: int,
                             stream: int = 0, tokenize: bool = False) -> int:
        """The same over raw device pointers (ints; e.g. torch tensors' data_ptr()) of this tokenizer's
        device, ordered on the HIP stream `stream` (0: the default stream).  d_ids has room for ids_cap
        uint32, d_tok_off for n_docs + 1 uint64.  Returns the number of ids; raises BufferError carrying
        `.needed` when ids_cap is too small, with nothing written.  The bytes are taken as they are.
        Returns after the work is done."""
        need = ctypes.c_uint64()
        rc = _n.lib.ctok_pipeline_encode_batch_device(self._h, d_text, d_off, n_docs, n_bytes, _n.CTOK_PIPELINE_TOKENIZE if tokenize else 0,
                                                      d_ids, ids_cap, d_tok_off, ctypes.byref(need), stream)
        if rc == _n.CTOK_E_CAPACITY and need.value > ids_cap:
            e = BufferError("encode_packed_device: the ids need %d entries, ids_cap is %d" % (need.value, ids_cap))
            e.needed = int(need.value)
            raise e
        if rc:
            _raise(rc)
        self._read_stats()
        return int(need.value)

    def encode_batch_flat(self, texts):
        """list[str] -> (ids uint32[T], tok_off uint64[D + 1])"""
        text, off = pack_texts(texts)
        return self.encode_packed(text, off)

    def encode_batch(self, texts) -> list:
        """mod.rs:694-696"""
        return _split_lists(*self.encode_batch_flat(texts))

    def encode(self, text: str) -> list:
        """mod.rs:551-613"""
        if not isinstance(text, str):
            raise TypeError("'%s' object cannot be converted to 'PyString'" % type(text).__name__)
        return self.encode_batch([text])[0]

    def tokenize_batch(self, texts) -> list:
        text, off = pack_texts(texts)
        ids, tok_off = self.encode_packed(text, off, tokenize=True)
        names = self._id_to_token
        ids, o = ids.tolist(), tok_off.tolist()
        return [[names[i] for i in ids[o[d]:o[d + 1]] if i in names] for d in range(len(o) - 1)]

    def tokenize(self, text: str) -> list:
        """mod.rs:1080-1101: the word BPE without the added-token loop, as vocab strings; an id
        without a vocab string is dropped."""
        if not isinstance(text, str):
            raise TypeError("'%s' object cannot be converted to 'PyString'" % type(text).__name__)
        return self.tokenize_batch([text])[0]

    # ------------------------------------------------------------------ Encodings
    # (src/bindings/tokenizer.rs:33-201, :259-367 -> src/huggingface/mod.rs:340-545).  Ids, offsets, word
    # ids, type ids and the special mask of a whole batch come from one call of
    # ctok_pipeline_encode_encodings; truncation and padding are Encoding's list methods.

    @property
    def model_max_length(self) -> int:
        return self._model_max_length

    @model_max_length.setter
    def model_max_length(self, value: int):
        if type(value) is not int or value < 0:
            raise TypeError("model_max_length: expected a non-negative int")
        self._model_max_length = value

    @property
    def padding_side(self) -> str:
        return self._padding_side

    @padding_side.setter
    def padding_side(self, value: str):
        self._padding_side = _as_str(value)

    @property
    def truncation_side(self) -> str:
        """Stored and returned; the reference's truncation never reads it either."""
        return self._truncation_side

    @truncation_side.setter
    def truncation_side(self, value: str):
        self._truncation_side = _as_str(value)

    @staticmethod
    def encoding_limits(handle=None) -> dict:
        lim = _n.PipelineEncodingLimits()
        _n.lib.ctok_pipeline_encoding_limits(handle, ctypes.byref(lim))
        return {k: int(getattr(lim, k)) for k, _ in lim._fields_}

    def _read_encoding_stats(self):
        self._read_stats()
        ms = (ctypes.c_double * _n.CTOK_PIPELINE_ENCODING_STAGES)()
        info = _n.PipelineEncodingInfo()
        _n.lib.ctok_pipeline_encoding_stage_ms(self._h, ms)
        _n.lib.ctok_pipeline_encoding_stats(self._h, ctypes.byref(info))
        self.last_stats["encoding"] = {k: int(getattr(info, k)) for k, _ in info._fields_}
        self.last_stats["encoding_stages"] = [(_n.lib.ctok_pipeline_encoding_stage_name(i).decode(), ms[i])
                                              for i in range(_n.CTOK_PIPELINE_ENCODING_STAGES)]

    def encode_encodings_flat(self, texts, pairs=None) -> dict:
        """Extension: the batch's Encoding fields as flat arrays from one call on the GPU.  Row r is
        texts[r] (and pairs[r]).  ids, type_ids, special_tokens_mask: uint32, row r at row_off[r] ..
        row_off[r + 1] (the processed row); offsets uint64 [n, 2] and word_ids uint32 [n], row r at
        seq_off[r] .. seq_off[r + 1] (one entry per id before the post-processor, seq_ids, each relative
        to its own text); n_a[r] of them are texts[r]'s."""
        texts = _as_str_list(texts)
        text, off = pack_texts(texts)
        rows = len(texts)
        ptext = poff = None
        if pairs is not None:
            pairs = _as_str_list(pairs)
            if len(pairs) != rows:
                raise ValueError("pairs must have one entry per text")
            ptext, poff = pack_texts(pairs)
        out = _n.PipelineEncodings()
        pp = self._post_processor._h if self._post_processor is not None else None
        rc = _n.lib.ctok_pipeline_encode_encodings(self._h, text.ctypes.data, off.ctypes.data, rows,
                                                   ptext.ctypes.data if ptext is not None else None,
                                                   poff.ctypes.data if poff is not None else None, pp, ctypes.byref(out))
        if rc:
            _raise(rc)
        self._read_encoding_stats()

        def arr(ptr, ctype, dtype, n):
            if not n:
                return np.zeros(0, dtype=dtype)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(n,)).copy()

        row_off = arr(out.row_off, ctypes.c_uint64, np.uint64, rows + 1)
        seq_off = arr(out.seq_off, ctypes.c_uint64, np.uint64, rows + 1)
        cells, n = int(row_off[rows]), int(seq_off[rows])
        return {"ids": arr(out.ids, ctypes.c_uint32, np.uint32, cells), "type_ids": arr(out.type_ids, ctypes.c_uint32, np.uint32, cells),
                "special_tokens_mask": arr(out.special_tokens_mask, ctypes.c_uint32, np.uint32, cells), "row_off": row_off,
                "offsets": arr(out.offsets, ctypes.c_uint64, np.uint64, 2 * n).reshape(-1, 2),
                "word_ids": arr(out.word_ids, ctypes.c_uint32, np.uint32, n), "seq_ids": arr(out.seq_ids, ctypes.c_uint32, np.uint32, n),
                "seq_off": seq_off,
                "n_a": arr(out.n_a, ctypes.c_uint64, np.uint64, rows)}

    def encode_encodings_device(self, d_text: int, d_off: int, n_rows: int, n_bytes: int, *, d_ids: int, d_type_ids: int, d_special: int,
                                cells_cap: int, d_row_off: int, d_offsets: int, d_word_ids: int, ids_cap: int, d_seq_off: int, d_n_a: int,
                                d_seq_ids: int = 0, pairs: bool = False, stream: int = 0):
        """Extension: the same over raw device pointers (ints; e.g. torch tensors' data_ptr()) of this
        tokenizer's device, ordered on the HIP stream `stream` (0: the default stream).  With pairs the
        sequences are interleaved: 2r is row r's text, 2r + 1 its pair, and d_off has 2 * n_rows + 1
        entries.  d_ids, d_type_ids and d_special hold cells_cap uint32, d_offsets 2 * ids_cap uint64,
        d_word_ids and d_seq_ids (0: not wanted) ids_cap uint32, d_row_off and d_seq_off n_rows + 1 uint64, d_n_a n_rows uint64.
        Returns (cells, ids); raises BufferError carrying `.needed` = (cells, ids) when a capacity is too
        small, with nothing written.  The bytes are taken as they are.  Returns after the work is done."""
        out = _n.PipelineEncodingsDevice(d_ids or None, d_type_ids or None, d_special or None, cells_cap, d_row_off or None,
                                         d_offsets or None, d_word_ids or None, d_seq_ids or None, ids_cap, d_seq_off or None, d_n_a or None, 0, 0)
        pp = self._post_processor._h if self._post_processor is not None else None
        rc = _n.lib.ctok_pipeline_encode_encodings_device(self._h, d_text or None, d_off or None, n_rows, 1 if pairs else 0, n_bytes, pp,
                                                          ctypes.byref(out), stream or None)
        if rc == _n.CTOK_E_CAPACITY and (out.n_cells > cells_cap or out.n_ids > ids_cap):
            e = BufferError("encode_encodings_device: %d cells and %d ids are needed, the capacities are %d and %d"
                            % (out.n_cells, out.n_ids, cells_cap, ids_cap))
            e.needed = (int(out.n_cells), int(out.n_ids))
            raise e
        if rc:
            _raise(rc)
        self._read_encoding_stats()
        return int(out.n_cells), int(out.n_ids)

    # ------------------------------------------------------------------ padded batches and stride windows as arrays
    # (include/ctok_pipeline.h "Padded batches and overflowing stride windows": truncation, the windows and the
    # padding run on the device over what the Encoding call left there; csrc/pipeline_win.hip)

    def _window_opts(self, what, windows, truncation, max_length, stride, add_special_tokens, pairs, padding, pad_left, pad_id, want=0):
        ml = int(max_length) if max_length is not None else self._model_max_length
        stride = int(stride)
        if ml < 0 or stride < 0 or (windows and stride >= ml):
            raise ValueError("%s: stride must be smaller than max_length (the reference loops forever)" % what)
        f = (_n.CTOK_P_ADD_SPECIAL if add_special_tokens else 0) | (_n.CTOK_P_PAIRS if pairs else 0)
        f |= (_n.CTOK_P_TRUNCATE | _n.CTOK_P_WINDOWS) if windows else (_n.CTOK_P_TRUNCATE if truncation else 0)
        if padding == "longest":
            f |= _n.CTOK_P_PAD_LONGEST
        elif padding == "max_length":
            f |= _n.CTOK_P_PAD_TO_MAX
        elif padding is not None:
            raise ValueError("%s: padding must be None, 'longest' or 'max_length'" % what)
        if pad_left is None:
            pad_left = self._padding_side == "left"
        f |= (_n.CTOK_P_PAD_LEFT if pad_left else 0) | (_n.CTOK_P_PAD_ID if pad_id is not None else 0)
        return _n.PipelineWindowOpts(f, int(pad_id or 0), ml, stride, want)

    def _read_window_stats(self):
        self._read_encoding_stats()
        ms = (ctypes.c_double * _n.CTOK_PIPELINE_WINDOW_STAGES)()
        info = _n.PipelineWindowInfo()
        _n.lib.ctok_pipeline_window_stage_ms(self._h, ms)
        _n.lib.ctok_pipeline_window_stats(self._h, ctypes.byref(info))
        self.last_stats["windows"] = {k: int(getattr(info, k)) for k, _ in info._fields_}
        self.last_stats["window_stages"] = [(_n.lib.ctok_pipeline_window_stage_name(i).decode(), ms[i])
                                            for i in range(_n.CTOK_PIPELINE_WINDOW_STAGES)]

    def _windows(self, what, windows, texts, pairs, truncation, max_length, stride, add_special_tokens, padding, pad_left, pad_id,
                 return_offsets, return_word_ids, return_sequence_ids):
        want = (_n.CTOK_PIPELINE_WIN_OFFSETS if return_offsets else 0) | (_n.CTOK_PIPELINE_WIN_WORD_IDS if return_word_ids else 0) \
            | (_n.CTOK_PIPELINE_WIN_SEQUENCE_IDS if return_sequence_ids else 0)
        opts = self._window_opts(what, windows, truncation, max_length, stride, add_special_tokens, pairs is not None, padding, pad_left,
                                 pad_id, want)
        texts = _as_str_list(texts)
        text, off = pack_texts(texts)
        rows = len(texts)
        ptext = poff = None
        if pairs is not None:
            pairs = _as_str_list(pairs)
            if len(pairs) != rows:
                raise ValueError("pairs must have one entry per text")
            ptext, poff = pack_texts(pairs)
        out = _n.PipelineWindows()
        pp = self._post_processor._h if self._post_processor is not None else None
        rc = _n.lib.ctok_pipeline_encode_windows(self._h, text.ctypes.data, off.ctypes.data, rows,
                                                 ptext.ctypes.data if ptext is not None else None,
                                                 poff.ctypes.data if poff is not None else None, pp, ctypes.byref(opts), ctypes.byref(out))
        if rc:
            _raise(rc)
        self._read_window_stats()
        n, w = int(out.n_windows), int(out.width)

        def arr(ptr, ctype, dtype, count, shape):
            if not count:
                return np.zeros(shape, dtype=dtype)
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ctype)), shape=(count,)).copy().reshape(shape)

        def cells(ptr):
            return arr(ptr, ctypes.c_uint32, np.uint32, n * w, (n, w))

        def rec(ptr, ctype=ctypes.c_uint64, dtype=np.uint64):
            return arr(ptr, ctype, dtype, n, (n,)).astype(np.int64)

        res = {"input_ids": cells(out.ids), "attention_mask": cells(out.attention_mask), "token_type_ids": cells(out.type_ids),
               "special_tokens_mask": cells(out.special_tokens_mask), "row_len": rec(out.win_len)}
        if windows:
            res["overflow_to_sample_mapping"] = rec(out.win_row, ctypes.c_uint32, np.uint32)
            res["window_start"] = rec(out.win_start)
            res["row_window"] = arr(out.row_win, ctypes.c_uint64, np.uint64, rows + 1, (rows + 1,)).astype(np.int64)
        if return_offsets:
            res["offset_mapping"] = arr(out.offsets, ctypes.c_uint64, np.uint64, 2 * n * w, (n, w, 2))
        if return_word_ids:
            res["word_ids"] = cells(out.word_ids)
        if return_offsets or return_word_ids:
            res["offsets_len"] = rec(out.win_off_len)
        if return_sequence_ids:
            res["sequence_ids"] = cells(out.sequence_ids)
            res["sequence_len"] = rec(out.win_seq_len)
        return res

    def encode_padded(self, texts, pairs=None, *, add_special_tokens: bool = True, truncation: bool = False, max_length: int | None = None,
                      padding: str | None = None, pad_left: bool | None = None, pad_id: int | None = None, return_offsets: bool = False,
                      return_word_ids: bool = False, return_sequence_ids: bool = False) -> dict:
        """Extension: what `__call__` computes, as [rows, width] arrays from one call on the GPU.  A row
        longer than max_length (None: model_max_length) is cut to it when truncation is set; padding is
        None, "longest" or "max_length", on the left with pad_left (None: padding_side == "left"); pad_id
        None is the reference's choice ([PAD], then <pad>, then 0).  Returns uint32 input_ids,
        attention_mask, token_type_ids, special_tokens_mask and int64 row_len [rows] (the row's Encoding
        length); cells past it hold padding values.  On request offset_mapping uint64 [rows, width, 2],
        word_ids and sequence_ids uint32 [rows, width] with offsets_len / sequence_len: the lists as the
        reference leaves them -- one entry per id before the post-processor, not realigned by truncation or
        padding -- from cell 0; past a list's end (0, 0) and 0xFFFFFFFF, which is also None inside
        sequence_ids.  Raises PanicException where `__call__` does: a row cut between its token count and
        its id count."""
        return self._windows("encode_padded", False, texts, pairs, truncation, max_length, 0, add_special_tokens, padding, pad_left, pad_id,
                             return_offsets, return_word_ids, return_sequence_ids)

    def encode_windows(self, texts, pairs=None, *, max_length: int | None = None, stride: int = 0, add_special_tokens: bool = True,
                       padding: str | None = None, pad_left: bool | None = None, pad_id: int | None = None, return_offsets: bool = False,
                       return_word_ids: bool = False, return_sequence_ids: bool = False) -> dict:
        """Extension: the batch cut into overflowing stride windows on the GPU
        (Encoding::truncate_with_stride).  A row of P > max_length ids becomes 1 + ceil((P - max_length) /
        (max_length - stride)) windows, the truncated main encoding first and its `overflowing` list after it;
        only the main window is padded.  The keys of encode_padded, [n_windows, ...] each, and int64
        overflow_to_sample_mapping, window_start [n_windows] and row_window [rows + 1] as
        Tokenizer.encode_windows returns them.  stride >= max_length raises ValueError.  A row that overflows
        with fewer tokens than ids raises PanicException, as the reference panics slicing `tokens`: after a
        post-processor that adds ids, and with add_special_tokens=False when the row holds an added token
        whose id is not in the vocab."""
        return self._windows("encode_windows", True, texts, pairs, True, max_length, stride, add_special_tokens, padding, pad_left, pad_id,
                             return_offsets, return_word_ids, return_sequence_ids)

    def encode_windows_device(self, d_text: int, d_off: int, n_rows: int, n_bytes: int, *, d_ids: int, cap: int, d_win_len: int,
                              d_win_row: int, win_cap: int, d_row_win: int, max_length: int | None = None, stride: int = 0,
                              windows: bool = True, truncation: bool = True, d_attention: int = 0, d_type_ids: int = 0, d_special: int = 0,
                              d_offsets: int = 0, d_word_ids: int = 0, d_sequence_ids: int = 0, d_win_start: int = 0,
                              d_win_off_len: int = 0, d_win_seq_len: int = 0, pairs: bool = False, add_special_tokens: bool = True,
                              padding: str | None = None, pad_left: bool | None = None, pad_id: int | None = None, stream: int = 0):
        """Extension: encode_windows (windows=False: encode_padded) over raw device pointers (ints; e.g.
        torch tensors' data_ptr()) of this tokenizer's device, ordered on the HIP stream `stream` (0: the
        default stream).  With pairs the sequences are interleaved and d_off has 2 * n_rows + 1 entries.
        d_ids and the other uint32 arrays hold cap cells, d_offsets 2 * cap uint64; d_win_len (uint64),
        d_win_row (uint32) and the other uint64 records win_cap entries; d_row_win n_rows + 1 uint64.  0 for
        an output that is not wanted, among all but d_ids, d_win_len, d_win_row and d_row_win.  Returns
        (n_windows, width); raises BufferError carrying `.needed` = (n_windows, width) when a capacity is
        too small, with d_row_win filled and nothing else written.  The bytes are taken as they are.
        Returns after the work is done."""
        opts = self._window_opts("encode_windows_device", windows, truncation, max_length, stride, add_special_tokens, pairs, padding,
                                 pad_left, pad_id)
        out = _n.PipelineWindowsDevice(d_ids or None, d_attention or None, d_type_ids or None, d_special or None, d_offsets or None,
                                       d_word_ids or None, d_sequence_ids or None, cap, d_win_len or None, d_win_row or None,
                                       d_win_start or None, d_win_off_len or None, d_win_seq_len or None, win_cap, d_row_win or None, 0, 0)
        pp = self._post_processor._h if self._post_processor is not None else None
        rc = _n.lib.ctok_pipeline_encode_windows_device(self._h, d_text or None, d_off or None, n_rows, n_bytes, pp, ctypes.byref(opts),
                                                        ctypes.byref(out), stream or None)
        if rc == _n.CTOK_E_CAPACITY and (out.n_windows > win_cap or out.n_windows * out.width > cap):
            e = BufferError("encode_windows_device: %d windows of width %d are needed, the capacities are %d cells and %d windows"
                            % (out.n_windows, out.width, cap, win_cap))
            e.needed = (int(out.n_windows), int(out.width))
            raise e
        if rc:
            _raise(rc)
        self._read_window_stats()
        return int(out.n_windows), int(out.width)

    def _pad_id_token(self):
        """mod.rs:505-510"""
        pid = self._special.get("[PAD]", self._special.get("<pad>", 0))
        return pid, self._id_to_token.get(pid, "<pad>")

    def _to_encodings(self, texts, pairs=None, add_special_tokens=True) -> list:
        """Encodings before truncation and padding: encode_to_encoding / encode_pair_to_encoding
        (mod.rs:340-392), or with add_special_tokens=False Encoding::from_ids over encode() (+ merge for a
        pair, src/bindings/tokenizer.rs:64-97): no offsets, no word ids, and `tokens` without the ids that
        have no vocab string.  One GPU call either way."""
        names = self._id_to_token
        rows = len(texts)
        if not add_special_tokens:
            docs = [x for ab in zip(texts, pairs) for x in ab] if pairs is not None else list(texts)
            ids, tok_off = self.encode_batch_flat(docs)
            ids, o = ids.tolist(), tok_off.tolist()
            k = 2 if pairs is not None else 1
            encs = []
            for r in range(rows):
                a, m, b = o[k * r], o[k * r + 1], o[k * r + k]
                row = ids[a:b]
                types = [0] * (m - a) + [1] * (b - m)
                encs.append(Encoding(row, types, [names[i] for i in row if i in names], [1] * (b - a), [0] * (b - a), [], [], list(types)))
            return encs
        f = self.encode_encodings_flat(texts, pairs)
        ids, types, special = f["ids"].tolist(), f["type_ids"].tolist(), f["special_tokens_mask"].tolist()
        offsets, wids = f["offsets"].tolist(), f["word_ids"].tolist()
        ro, so, na = f["row_off"].tolist(), f["seq_off"].tolist(), f["n_a"].tolist()
        flat = f["seq_ids"].tolist()
        encs = []
        for r in range(rows):
            a, b, c, d = ro[r], ro[r + 1], so[r], so[r + 1]
            n = d - c
            # one token string per id before the post-processor, "" outside the vocab (mod.rs:410); the
            # post-processor extends neither tokens nor offsets, word ids and sequence ids (mod.rs:378-386)
            toks = [names.get(i, "") for i in flat[c:d]]
            encs.append(Encoding(ids[a:b], types[a:b], toks, [1] * (b - a), special[a:b], [tuple(x) for x in offsets[c:d]], wids[c:d],
                                 [0] * na[r] + [1] * (n - na[r])))
        return encs

    def encode_to_encoding(self, text: str) -> Encoding:
        """src/bindings/tokenizer.rs:298-300 -> mod.rs:340-342"""
        return self._to_encodings([_as_str(text)])[0]

    def encode_plus(self, text: str) -> Encoding:
        """src/bindings/tokenizer.rs:258-260"""
        return self.encode_to_encoding(text)

    def encode_pair_to_encoding(self, text: str, text_pair: str) -> Encoding:
        """src/bindings/tokenizer.rs:302-304 -> mod.rs:344-346"""
        return self._to_encodings([_as_str(text)], [_as_str(text_pair)])[0]

    def encode_with_truncation(self, text: str, text_pair: str | None = None, max_length: int = 512, stride: int = 0) -> Encoding:
        """src/bindings/tokenizer.rs:306-318 -> mod.rs:348-392"""
        enc = self.encode_pair_to_encoding(text, text_pair) if text_pair is not None else self.encode_to_encoding(text)
        if len(enc) > max_length:
            enc.truncate_with_stride(max_length, stride)
        return enc

    def encode_batch_to_encoding(self, texts) -> list:
        """src/bindings/tokenizer.rs:320-326 -> mod.rs:483-485"""
        return self._to_encodings(_as_str_list(texts))

    def batch_encode_plus(self, texts) -> list:
        """src/bindings/tokenizer.rs:262-269"""
        return self.encode_batch_to_encoding(texts)

    def encode_batch_pairs_to_encoding(self, pairs) -> list:
        """src/bindings/tokenizer.rs:328-336 -> mod.rs:487-491"""
        a, b = _split_pairs(pairs)
        return self._to_encodings(a, b)

    def _pad_all(self, encs, max_length, pad_left):
        target = max_length if max_length is not None else max((len(e) for e in encs), default=0)
        pid, ptok = self._pad_id_token()
        for e in encs:
            e.pad(target, pid, ptok, pad_left)
        return encs

    def encode_batch_with_padding(self, texts, max_length: int | None = None, pad_left: bool = False) -> list:
        """src/bindings/tokenizer.rs:338-350 -> mod.rs:493-517 (no truncation)"""
        return self._pad_all(self.encode_batch_to_encoding(texts), max_length, pad_left)

    def encode_batch_pairs_with_padding(self, pairs, max_length: int | None = None, pad_left: bool = False) -> list:
        """src/bindings/tokenizer.rs:352-367 -> mod.rs:519-543"""
        return self._pad_all(self.encode_batch_pairs_to_encoding(pairs), max_length, pad_left)

    def __call__(self, text, text_pair=None, add_special_tokens: bool = True, padding: str | None = None, truncation: bool = False,
                 max_length: int | None = None, stride: int = 0, return_attention_mask: bool = True, return_token_type_ids: bool = True,
                 return_offsets_mapping: bool = False, return_special_tokens_mask: bool = False) -> BatchEncoding:
        """src/bindings/tokenizer.rs:33-201"""
        flags = (return_attention_mask, return_token_type_ids, return_offsets_mapping, return_special_tokens_mask)
        max_len = max_length if max_length is not None else self._model_max_length
        batch = _extract_str_list(text)
        if batch is not None:
            pairs = _extract_str_list(text_pair) if text_pair is not None else None
            if pairs is not None:
                m = min(len(batch), len(pairs))  # Iterator::zip
                batch, pairs = batch[:m], pairs[:m]
            encs = self._to_encodings(batch, pairs, add_special_tokens)
        elif isinstance(text, str):
            pair = text_pair if isinstance(text_pair, str) else None
            encs = self._to_encodings([text], [pair] if pair is not None else None, add_special_tokens)
        else:
            raise TypeError("Expected str or List[str]")
        if truncation:
            for e in encs:
                if len(e) > max_len:
                    if stride > 0:
                        e.truncate_with_stride(max_len, stride)
                    else:
                        e.truncate(max_len)
        if padding is not None:
            # (a str input pads to its own length: the longest of a batch of one)
            target = max_len if padding == "max_length" else max((len(e) for e in encs), default=0)
            pid, ptok = self._pad_id_token()
            left = padding == "left" or self._padding_side == "left"
            for e in encs:
                e.pad(target, pid, ptok, left)
        return BatchEncoding(encs, *flags)

    # ------------------------------------------------------------------ decode
    def _decoder_with_vocab(self):
        if self._decode_with is None:
            dec = self._decoder
            if dec is None:
                dec = Decoder.fuse(device=self.device)  # BpeTokenizer::decode: the vocab strings joined
            elif dec._has_vocab:
                dec = Decoder(dec._steps, dec.device, repr(dec))  # (the caller's decoder keeps its own vocabulary)
            dec.set_vocab(self._id_to_token)
            self._decode_with = dec
        return self._decode_with

    def decode_batch_with_options(self, batch, skip_special_tokens: bool = False, clean_up_tokenization_spaces: bool = True) -> list:
        """decode_impl (mod.rs:711-747) of every id list: optionally without the ids whose vocab string
        is a special token, ids without a vocab string dropped, the decoder on the device, then
        optionally the clean-up."""
        ids, off = pack_ids(batch)
        if skip_special_tokens and self._special:
            if self._special_ids is None:
                self._special_ids = np.asarray(sorted(i for i, t in self._id_to_token.items() if t in self._special), dtype=np.uint32)
            keep = ~np.isin(ids, self._special_ids)
            kept_before = np.concatenate(([0], np.cumsum(keep, dtype=np.uint64)))
            ids, off = ids[keep], kept_before[off.astype(np.int64)].astype(np.uint64)
        dec = self._decoder_with_vocab()
        text, text_off = dec.decode_ids_packed(ids, off)
        raw, o = text.tobytes(), text_off.tolist()
        out = [raw[o[i]:o[i + 1]].decode("utf-8") for i in range(len(o) - 1)]
        return [_clean_up(t) for t in out] if clean_up_tokenization_spaces else out

    def decode_batch(self, batch) -> list:
        """mod.rs:771-773"""
        return self.decode_batch_with_options(batch, False, True)

    def decode_with_options(self, ids, skip_special_tokens: bool = False, clean_up_tokenization_spaces: bool = True) -> str:
        """mod.rs:702-709"""
        if isinstance(ids, (str, bytes)):
            raise TypeError("Can't extract `str` to `Vec`")
        return self.decode_batch_with_options([ids], skip_special_tokens, clean_up_tokenization_spaces)[0]

    def decode(self, ids) -> str:
        """mod.rs:698-700"""
        return self.decode_with_options(ids, False, True)
