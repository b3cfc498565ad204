"""TEST INFRASTRUCTURE ONLY -- the reference's HuggingFaceTokenizer with any normaliser, pre-tokenizer
and decoder, restated by composing what the suite already has:

  oracle/ref_py.py        RefTokenizer.bpe / _find_added_token / _encode_word / clean-up (src/bpe.rs:52-153,
                          src/huggingface/mod.rs:566-675, :749-769), used unchanged through a subclass
  tests/normalizer_ref    Normalizer::normalize      tests/pretok_ref    PreTokenizer::pre_tokenize
  tests/decoder_ref       Decoder::decode            tests/postproc_ref  PostProcessor::process

New here are only the rules of src/huggingface/parsing.rs:10-364 (the component specs are the tuples
of those modules) and the glue of from_tokenizer_json_with_config, encode, tokenize and decode_impl
(mod.rs:247-334, :551-613, :1080-1101, :711-747).  The product never imports this module.
"""
from oracle import ref_py
from oracle.ref_py import PanicException, UnsupportedConfig  # noqa: F401  (re-exported for the tests)
from tests import decoder_ref, normalizer_ref, postproc_ref, pretok_ref

_MISSING = object()


def _typed(value):
    """(obj, type string) of a component that names a type; None for the default arm (parsing.rs: no
    value, not an object, or no "type")."""
    if isinstance(value, dict) and "type" in value:
        t = value["type"]
        return value, (t if isinstance(t, str) else "")
    return None


def _str(obj, key, default):
    v = obj.get(key)
    return v if isinstance(v, str) else default


def _bool(obj, key, default):
    v = obj.get(key)
    return v if isinstance(v, bool) else default


def _char(obj, key, default):
    v = obj.get(key)
    return v[0] if isinstance(v, str) and v else default


def _u64(obj, key):
    v = obj.get(key)
    return v if isinstance(v, int) and not isinstance(v, bool) and 0 <= v < 1 << 64 else 0


def _sequence(obj, key, parse):
    items = obj.get(key)
    if not isinstance(items, list):
        return None
    parsed = [p for p in (parse(i) for i in items) if p is not None]
    return ("sequence", parsed) if parsed else None


def parse_normalizer(value):
    """parsing.rs:10-90"""
    tv = _typed(value)
    if tv is None:
        return ("nfc",)
    obj, t = tv
    if t in ("NFC", "NFD", "NFKC", "NFKD", "Lowercase", "Strip"):
        return (t.lower(),)
    if t == "StripAccents":
        return ("strip_accents",)
    if t == "Replace":
        pat = obj.get("pattern")
        pat = pat.get("String") if isinstance(pat, dict) else None
        return ("replace", pat if isinstance(pat, str) else "", _str(obj, "content", ""))
    if t == "Prepend":
        return ("prepend", _str(obj, "prepend", ""))
    if t == "Sequence":
        return _sequence(obj, "normalizers", parse_normalizer)
    if t == "BertNormalizer":
        sa = obj.get("strip_accents")
        return ("bert", _bool(obj, "clean_text", True), _bool(obj, "handle_chinese_chars", True), sa if isinstance(sa, bool) else None,
                _bool(obj, "lowercase", True))
    if t == "Precompiled":
        s = obj.get("precompiled_charsmap")
        return ("precompiled", [(s, s)] if isinstance(s, str) else [])  # (x -> x: the identity it is in the reference)
    return None


_BEHAVIORS = ("Isolated", "MergedWithPrevious", "MergedWithNext", "Contiguous")


def parse_pre_tokenizer(value):
    """parsing.rs:92-190"""
    tv = _typed(value)
    if tv is None:
        return ("byte_level", False)
    obj, t = tv
    if t == "ByteLevel":
        return ("byte_level", _bool(obj, "add_prefix_space", False))
    if t == "Metaspace":
        return ("metaspace", _char(obj, "replacement", "▁"), _bool(obj, "add_prefix_space", True))
    if t == "Whitespace":
        return ("whitespace",)
    if t == "WhitespaceSplit":
        return ("whitespace_split",)
    if t == "Punctuation":
        return ("punctuation",)
    if t == "BertPreTokenizer":
        return ("bert",)
    if t == "CharDelimiterSplit":
        return ("char_delimiter_split", _char(obj, "delimiter", " "))
    if t == "UnicodeScripts":
        return ("unicode_scripts",)
    if t == "Digits":
        return ("digits", _bool(obj, "individual_digits", False))
    if t == "Split":
        pat = obj.get("pattern")
        pat = pat.get("Regex") if isinstance(pat, dict) else None
        beh = obj.get("behavior")
        return ("split", pat if isinstance(pat, str) else "", beh if beh in _BEHAVIORS else "Removed", _bool(obj, "invert", False))
    if t == "Sequence":
        return _sequence(obj, "pretokenizers", parse_pre_tokenizer)
    return None


def parse_decoder(value):
    """parsing.rs:272-364"""
    tv = _typed(value)
    if tv is None:
        return ("byte_level",)
    obj, t = tv
    if t == "ByteLevel":
        return ("byte_level",)
    if t == "Metaspace":
        return ("metaspace", _char(obj, "replacement", "▁"), _bool(obj, "add_prefix_space", True))
    if t == "WordPiece":
        return ("wordpiece", _str(obj, "prefix", "##"), _bool(obj, "cleanup", True))
    if t == "BPE":
        return ("bpe", _str(obj, "suffix", "</w>"))
    if t == "CTC":
        wd = obj.get("word_delimiter_token")
        return ("ctc", _str(obj, "pad_token", "<pad>"), wd if isinstance(wd, str) else None)
    if t == "Fuse":
        return ("fuse",)
    if t == "Strip":
        return ("strip", _char(obj, "content", " "), _u64(obj, "start"), _u64(obj, "stop"))
    if t == "Sequence":
        return _sequence(obj, "decoders", parse_decoder)
    return None


def _template(arr):
    """template_from_array, parsing.rs:248-269"""
    out = []
    for item in arr:
        if not isinstance(item, dict):
            continue
        if "SpecialToken" in item:
            sp = item["SpecialToken"]
            v = sp.get("id") if isinstance(sp, dict) else None
            if isinstance(v, str):
                out.append(v)
            continue  # (the arm returns, also with no id)
        if "Sequence" in item:
            sq = item["Sequence"]
            v = sq.get("id") if isinstance(sq, dict) else None
            if isinstance(v, str):
                out.append("$" + v)
    return " ".join(out)


def parse_post_processor(value, special_tokens):
    """parsing.rs:193-245; special_tokens: {content: id} of the special added tokens, in the file's
    order (the reference's HashMap order is not defined; only which tokens a template names matters)"""
    tv = _typed(value)
    if tv is None:
        return None
    obj, t = tv
    if t == "TemplateProcessing":
        single = obj.get("single")
        pair = obj.get("pair")
        return ("template", _template(single) if isinstance(single, list) else "<s> $A </s>",
                _template(pair) if isinstance(pair, list) else None, list(special_tokens.items()))
    if t == "RobertaProcessing":
        return ("roberta", ("<s>", special_tokens.get("<s>", 0)), ("</s>", special_tokens.get("</s>", 2)), False)
    if t == "BertProcessing":
        return ("bert", ("[CLS]", special_tokens.get("[CLS]", 101)), ("[SEP]", special_tokens.get("[SEP]", 102)))
    return None


def parse_merges(items):
    """deserialize_merges (mod.rs:56-101), then the split at ' ' (mod.rs:252-264)"""
    out = []
    for m in ref_py.deserialize_merges(items):
        parts = m.split(" ")
        if len(parts) == 2:
            out.append((parts[0], parts[1]))
    return out


def parse_tokenizer_json(obj):
    """the whole file as a spec: what PipelineTokenizer.from_components takes"""
    model = obj["model"]
    added = [dict(id=t["id"], content=t["content"], special=t["special"], single_word=t.get("single_word", False),
                  lstrip=t.get("lstrip", False), rstrip=t.get("rstrip", False), normalized=t.get("normalized", False))
             for t in obj.get("added_tokens", [])]
    special = {}
    for t in added:
        if t["special"]:
            special[t["content"]] = t["id"]
    return dict(vocab=dict(model["vocab"]), merges=parse_merges(model.get("merges", [])), added_tokens=added,
                normalizer=parse_normalizer(obj.get("normalizer")), pre_tokenizer=parse_pre_tokenizer(obj.get("pre_tokenizer")),
                decoder=parse_decoder(obj.get("decoder")), post_processor=parse_post_processor(obj.get("post_processor"), special))


class PipelineRef(ref_py.RefTokenizer):
    """HuggingFaceTokenizer over a spec.  bpe, _find_added_token and _encode_word are RefTokenizer's."""

    def __init__(self, vocab, merges, normalizer=None, pre_tokenizer=None, decoder=None, post_processor=None, added_tokens=()):
        # BpeTokenizer::new, src/bpe.rs:52-79 (as RefTokenizer.__init__ states it)
        self.vocab = dict(vocab)
        self.merge_ranks = {}
        self.merge_new_ids = []
        for rank, (a, b) in enumerate(merges):
            if a in self.vocab and b in self.vocab and a + b in self.vocab:
                self.merge_ranks[(self.vocab[a], self.vocab[b])] = rank
                self.merge_new_ids.append(self.vocab[a + b])
        self.added_tokens, self.added_cfg, self.special_tokens = {}, {}, {}
        for t in added_tokens:
            self.added_tokens[t["content"]] = t["id"]
            self.added_cfg[t["content"]] = dict(single_word=t.get("single_word", False), lstrip=t.get("lstrip", False),
                                                rstrip=t.get("rstrip", False))
            if t.get("special", False):
                self.special_tokens[t["content"]] = t["id"]
        self.normalizer, self.pre_tokenizer, self.decoder, self.post_processor = normalizer, pre_tokenizer, decoder, post_processor
        self.id_to_token_map = {v: k for k, v in self.vocab.items()}

    @classmethod
    def from_json(cls, obj):
        return cls(**parse_tokenizer_json(obj))

    def words(self, text):
        normalized = text if self.normalizer is None else normalizer_ref.normalize(self.normalizer, text)
        return [normalized] if self.pre_tokenizer is None else pretok_ref.pre_tokenize(self.pre_tokenizer, normalized)

    def encode(self, text):
        """mod.rs:551-613"""
        out = []
        for w in self.words(text):
            out.extend(self._encode_word(w))
        return out

    def tokenize(self, text):
        """mod.rs:1080-1101: no added-token loop; ids without a vocab string are dropped"""
        out = []
        for w in self.words(text):
            out.extend(self.id_to_token_map[i] for i in self.bpe(w) if i in self.id_to_token_map)
        return out

    def decode_with_options(self, ids, skip_special_tokens=False, clean_up_tokenization_spaces=True):
        """decode_impl, mod.rs:711-747"""
        if skip_special_tokens:
            ids = [i for i in ids if not (i in self.id_to_token_map and self.id_to_token_map[i] in self.special_tokens)]
        toks = [self.id_to_token_map[i] for i in ids if i in self.id_to_token_map]
        text = "".join(toks) if self.decoder is None else decoder_ref.decode(self.decoder, toks)
        return ref_py.clean_up_tokenization_spaces_(text) if clean_up_tokenization_spaces else text

    def process(self, ids, pair_ids=None):
        return list(ids) if self.post_processor is None else postproc_ref.process(self.post_processor, ids, pair_ids)
