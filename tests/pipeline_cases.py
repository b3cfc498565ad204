"""The table of tokenizer specs and texts of the PipelineTokenizer suites (tests/test_pipeline_cpu.py,
tests/test_gpu_pipeline.py).  A spec is what tests/pipeline_ref.PipelineRef takes: vocab, merges, the
component tuples of the *_ref modules and the added tokens.  Pure data and seeded generators: no
device, no product import."""
import random

ABC = {"a": 0, "b": 1, "c": 2, "ab": 3, "bc": 4, "abc": 5, "aa": 6, "aaaa": 7}


def spec(vocab, merges, normalizer=None, pre_tokenizer=None, decoder=None, post_processor=None, added_tokens=()):
    return dict(vocab=dict(vocab), merges=list(merges), normalizer=normalizer, pre_tokenizer=pre_tokenizer, decoder=decoder,
                post_processor=post_processor, added_tokens=[dict(t) for t in added_tokens])


def added(content, id, special=False, single_word=False, lstrip=False, rstrip=False):
    return dict(id=id, content=content, special=special, single_word=single_word, lstrip=lstrip, rstrip=rstrip, normalized=False)


def chain(levels):
    """The worst case of the merge loop: "a", "aa", "aaaa", ... (2^levels) under (a, a), (aa, aa), ...;
    "b" never merges."""
    vocab = {"b": 0}
    for k in range(levels + 1):
        vocab["a" * (1 << k)] = k + 1
    return vocab, [("a" * (1 << k), "a" * (1 << k)) for k in range(levels)]


# filtered = [aa, cb, cbb]: (a, a) has rank 1 and so the new id of "cb"; (c, b) has rank 2 and the new id of
# "cbb"; (cb, b) has rank 3 >= 3 and panics -- a a b -> cb b makes it adjacent only after a merge
LATE = ({"a": 0, "b": 1, "c": 2, "aa": 3, "cb": 4, "cbb": 5}, [("q", "q"), ("a", "a"), ("c", "b"), ("cb", "b")])
# filtered = [ab, bc]: (a, b) has rank 1 and bc's id, (b, c) has rank 2 >= 2 and panics
SHIFT = (ABC, [("x", "y"), ("a", "b"), ("b", "c")])

CHARS = {"a": 0, "b": 1, "é": 2, "中": 3, "😀": 4, "é中": 5, "中😀": 6, "aé": 7, "é中😀": 8, "ab": 9, " ": 10}
CHAR_MERGES = [("é", "中"), ("中", "😀"), ("a", "é"), ("é中", "😀"), ("a", "b")]

AT = [added("<s>", 100, special=True), added("<s>>", 101), added("[X]", 102, special=True), added("<é>", 103)]
FLAGS = [added("<w>", 100, single_word=True), added("<l>", 101, lstrip=True), added("<r>", 102, rstrip=True),
         added("<lr>", 103, lstrip=True, rstrip=True)]

# name -> (spec, texts); none of these texts panics
CASES = {
    "aaa": (spec(ABC, [("a", "a")], pre_tokenizer=("whitespace",)), ["aaa", "aaaa a aa", "", "   ", "a"]),
    "chain": (spec(*chain(4), pre_tokenizer=("whitespace",)), ["a" * n for n in (1, 2, 3, 5, 15, 16, 17, 31)] + ["aab aaaab b"]),
    "duplicate": (spec(ABC, [("a", "b"), ("b", "c"), ("a", "b")], pre_tokenizer=("whitespace",)), ["abc", "ab bc cab abab"]),
    "shift": (spec(*SHIFT, pre_tokenizer=("whitespace",)), ["ab", "abab cb ba", "a b c"]),
    "late": (spec(*LATE, pre_tokenizer=("whitespace",)), ["aa", "cb", "aa cb b a", "aaa"]),
    "shared_id": (spec({"a": 0, "A": 0, "b": 1, "ab": 2, "Ab": 3}, [("a", "b"), ("A", "b")], pre_tokenizer=("whitespace",)),
                  ["ab Ab aAb", "bA"]),
    "chars": (spec(CHARS, CHAR_MERGES, pre_tokenizer=("whitespace",)),
              ["aé中😀b", "é", "中😀", "😀😀", "xyz", "?!", "a?é", "é?中", "áb", "ab é中😀 aé中 zzz", "", " "]),
    "no_pretok": (spec(CHARS, CHAR_MERGES), ["a b", "aé 中😀", "", " ", "zzz"]),
    "added": (spec(ABC, [("a", "b")], pre_tokenizer=("whitespace",), added_tokens=AT),
              ["<s>ab", "ab<s>ab", "ab[X]", "<s>[X]", "<s><s>", "a<s>>b", "<s", "a<é>b <é>", "[X]<s>>[X] ab<s> <s>ab", "<<s>>", ""]),
    "flags": (spec(ABC, [("a", "b")], added_tokens=FLAGS),
              ["a <w> b", "a<w> <w>", "<w>a", "é<w>", "1<w>", "<w>", "_<w>_", "a <l>b", "a<l>b", "<l>b", "a　<l>", "a<r> b", "a<r>b",
               "a<r>", "a <lr> b", "a <lr>b", "a<lr> b", "<lr>", "ab <w> <l><r> ab", "a<l> <l>", "b<r>b<r> "]),
    "flags_ws": (spec(ABC, [("a", "b")], pre_tokenizer=("whitespace",), added_tokens=FLAGS),
                 ["a <w> b", "a<w> <w>", "a <l>b", "a<r> b", "x<w>y <w>"]),
    "many_added": (spec(ABC, [("a", "b")], pre_tokenizer=("whitespace",),
                        added_tokens=[added("<t%d>" % i, 1000 + i, special=i < 4) for i in range(300)]),
                   ["<t0>ab<t299>", "ab<t17><t170>c <t3", "<t29><t2>9", "abc"]),
}


def fuzz_added(seed, n_texts=160):
    """Added tokens that overlap, prefix and contain each other over a five-char alphabet, with seeded
    flags, and seeded texts over the same alphabet: the first-occurrence rule and the three checks meet
    in every combination."""
    rng = random.Random(seed)
    contents = ["<a>", "<a", "a>", "<<", ">>", "b", "ab ", " <", "<a><", "a", "<b>", "> <", "é"]
    toks = [added(c, 200 + i, single_word=rng.random() < 0.4, lstrip=rng.random() < 0.3, rstrip=rng.random() < 0.3)
            for i, c in enumerate(contents)]
    alphabet = ["<", ">", "a", "b", " ", "c", "é", "1"]
    texts = ["".join(rng.choice(alphabet) for _ in range(rng.randrange(1, 14))) for _ in range(n_texts)]
    return spec(dict(ABC, **{" ": 8, "<": 9, ">": 10, "<a": 11}), [("a", "b"), ("<", "a"), ("b", "c")], added_tokens=toks), texts


CASES["fuzz_added_1"] = fuzz_added(31)
CASES["fuzz_added_2"] = fuzz_added(32)

# name -> (spec, texts, the text that panics, len, rank): one bad pair per case
PANICS = {
    "first_scan": (spec(*SHIFT, pre_tokenizer=("whitespace",)), ["bc"], 0, 2, 2),
    "not_best": (spec(*SHIFT, pre_tokenizer=("whitespace",)), ["ab ab", "a aabc", "cb"], 1, 2, 2),
    "clean_around": (spec(*SHIFT, pre_tokenizer=("whitespace",)), ["ab", "ba cb", "abab bc", "ab", "cb"], 2, 2, 2),
    "after_merge": (spec(*LATE, pre_tokenizer=("whitespace",)), ["aa cb", "b aab", "aa"], 1, 3, 3),
    "after_merge_inside": (spec(*LATE, pre_tokenizer=("whitespace",)), ["a", "cb baab"], 1, 3, 3),
}

ALPHABET = list("abcdefghijklmnopqrstuvwxyz0123456789") + ["é", "ß", "中", "文", "▁", "Ġ", "😀", "_", "-", "'"]
NOISE = list("ABCDEFXYW?!.,;") + ["É", "Ａ", "ﬁ", "é", "　", "\t", "\n", "日", "🙂"]


def random_vocab(seed, n_merges=260, invalid=0):
    """About 300 entries: the alphabet, then merges of random existing tokens.  `invalid` merges have a
    result outside the vocab, so every later pair's new id shifts; as many guard merges over "Z" strings,
    which no text holds, take the ranks past the filtered list."""
    rng = random.Random(seed)
    vocab = {c: i for i, c in enumerate(ALPHABET)}
    toks = list(ALPHABET)
    merges = []
    bad = set(rng.sample(range(n_merges // 4), invalid)) if invalid else set()
    tries = 0
    while len(merges) < n_merges and tries < 100000:
        tries += 1
        a, b = rng.choice(toks), rng.choice(toks)
        if a + b in vocab or len(a + b) > 12 or (a, b) in merges:
            continue
        merges.append((a, b))
        if len(merges) - 1 in bad:
            continue
        vocab[a + b] = len(vocab)
        toks.append(a + b)
        if rng.random() < 0.3:  # favour what can occur: extend a recent token again
            toks.append(a + b)
    for i in range(invalid):
        z = "Z" * (1 << i)
        vocab.setdefault(z, len(vocab))
        vocab[z + z] = len(vocab)
        merges.append((z, z))
    return vocab, merges


def random_texts(seed, n, vocab=None, max_words=12):
    """Seeded texts over the alphabet, vocab strings, noise chars and white space."""
    rng = random.Random(seed)
    keys = [k for k in (vocab or {}) if "Z" not in k] or ALPHABET
    out = []
    for _ in range(n):
        words = []
        for _ in range(rng.randrange(max_words + 1)):
            parts = []
            for _ in range(rng.randrange(1, 5)):
                r = rng.random()
                parts.append(rng.choice(keys) if r < 0.6 else rng.choice(ALPHABET) if r < 0.9 else rng.choice(NOISE))
            words.append("".join(parts))
        seps = [rng.choice([" ", " ", " ", "  ", "\n", "\t", " - ", ", "]) for _ in words]
        out.append("".join(w + s for w, s in zip(words, seps)) if rng.random() < 0.5 else " ".join(words))
    return out


def pipelines():
    """name -> (spec, texts): the end-to-end pipelines over one seeded vocabulary."""
    vocab, merges = random_vocab(11)
    texts = random_texts(12, 60, vocab)
    vocab = dict(vocab, **{"[CLS]": 5000, "<mask>": 5001})  # special tokens' strings in the vocab: what decode may skip
    texts = texts +["", " ", "　", "ÉCOLE ＡＢc ﬁn", "Hello, World! 中文 test-case it's"]
    sp = [added("[CLS]", 900, special=True), added("[SEP]", 901, special=True), added("<mask>", 902, special=True, lstrip=True)]
    more = ["[CLS] ab [SEP]", "x<mask>y <mask> [CLS][SEP]"]
    return {
        "nfkc_lower_whitespace": (spec(vocab, merges, ("sequence", [("nfkc",), ("lowercase",)]), ("whitespace",), ("fuse",), None, sp),
                                  texts + more),
        "bert_bert": (spec(vocab, merges, ("bert", True, True, None, True), ("bert",), ("wordpiece", "##", True),
                           ("bert", ("[CLS]", 900), ("[SEP]", 901)), sp), texts + more),
        "none_metaspace": (spec(vocab, merges, None, ("metaspace", "▁", True), ("metaspace", "▁", True), None, sp), texts + more),
        "strip_chardelim": (spec(vocab, merges, ("strip",), ("char_delimiter_split", "-"), None, None, sp), texts + more),
        "random_clean": (spec(vocab, merges, ("nfc",), ("whitespace",)), random_texts(13, 200, vocab)),
        "random_shifted": (spec(*random_vocab(21, invalid=3), normalizer=None, pre_tokenizer=("whitespace",)),
                           random_texts(22, 200, random_vocab(21, invalid=3)[0])),
    }


def tokenizer_json(sp, components):
    """A tokenizer.json object of a spec: `components` holds the four JSON component values (a key left
    out stays out of the file); merges alternate between the two forms."""
    obj = {"version": "1.0", "model": {"type": "BPE", "vocab": dict(sp["vocab"]),
                                       "merges": [a + " " + b if i % 2 else [a, b] for i, (a, b) in enumerate(sp["merges"])]},
           "added_tokens": [dict(t) for t in sp["added_tokens"]]}
    obj.update(components)
    return obj


# ---- specs written as tokenizer.json: the path from_file / from_str take -----------------------------------

_NORM_TYPES = {"nfc": "NFC", "nfd": "NFD", "nfkc": "NFKC", "nfkd": "NFKD", "lowercase": "Lowercase", "strip": "Strip",
               "strip_accents": "StripAccents"}
_PRETOK_TYPES = {"whitespace": "Whitespace", "whitespace_split": "WhitespaceSplit", "punctuation": "Punctuation", "bert": "BertPreTokenizer",
                 "unicode_scripts": "UnicodeScripts"}


def normalizer_json(n):
    kind = n[0]
    if kind in _NORM_TYPES:
        return {"type": _NORM_TYPES[kind]}
    if kind == "replace":
        return {"type": "Replace", "pattern": {"String": n[1]}, "content": n[2]}
    if kind == "prepend":
        return {"type": "Prepend", "prepend": n[1]}
    if kind == "bert":
        obj = {"type": "BertNormalizer", "clean_text": n[1], "handle_chinese_chars": n[2], "lowercase": n[4]}
        if n[3] is not None:
            obj["strip_accents"] = n[3]
        return obj
    if kind == "precompiled":
        return {"type": "Precompiled", "precompiled_charsmap": n[1][0][0]} if n[1] else {"type": "Precompiled"}
    assert kind == "sequence", kind
    return {"type": "Sequence", "normalizers": [normalizer_json(m) for m in n[1]]}


def pre_tokenizer_json(p):
    kind = p[0]
    if kind in _PRETOK_TYPES:
        return {"type": _PRETOK_TYPES[kind]}
    if kind == "byte_level":
        return {"type": "ByteLevel", "add_prefix_space": p[1]}
    if kind == "metaspace":
        return {"type": "Metaspace", "replacement": p[1], "add_prefix_space": p[2]}
    if kind == "char_delimiter_split":
        return {"type": "CharDelimiterSplit", "delimiter": p[1]}
    if kind == "digits":
        return {"type": "Digits", "individual_digits": p[1]}
    if kind == "split":
        return {"type": "Split", "pattern": {"Regex": p[1]}, "behavior": p[2], "invert": p[3]}
    assert kind == "sequence", kind
    return {"type": "Sequence", "pretokenizers": [pre_tokenizer_json(m) for m in p[1]]}


def decoder_json(d):
    kind = d[0]
    if kind == "byte_level":
        return {"type": "ByteLevel"}
    if kind == "metaspace":
        return {"type": "Metaspace", "replacement": d[1], "add_prefix_space": d[2]}
    if kind == "wordpiece":
        return {"type": "WordPiece", "prefix": d[1], "cleanup": d[2]}
    if kind == "bpe":
        return {"type": "BPE", "suffix": d[1]}
    if kind == "ctc":
        obj = {"type": "CTC", "pad_token": d[1]}
        if d[2] is not None:
            obj["word_delimiter_token"] = d[2]
        return obj
    if kind == "fuse":
        return {"type": "Fuse"}
    if kind == "strip":
        return {"type": "Strip", "content": d[1], "start": d[2], "stop": d[3]}
    assert kind == "sequence", kind
    return {"type": "Sequence", "decoders": [decoder_json(m) for m in d[1]]}


def _template_items(template):
    return [{"Sequence": {"id": w[1:], "type_id": 0}} if w.startswith("$") else {"SpecialToken": {"id": w, "type_id": 0}}
            for w in template.split(" ") if w]


def post_processor_json(p):
    if p[0] == "template":
        obj = {"type": "TemplateProcessing", "single": _template_items(p[1])}
        if p[2] is not None:
            obj["pair"] = _template_items(p[2])
        return obj
    return {"type": {"bert": "BertProcessing", "roberta": "RobertaProcessing"}[p[0]]}


def spec_json(sp):
    """The tokenizer.json of a spec: a component that is None is written as an unknown type, which is how
    the reference reads `none` (a key left out would be the default)."""
    none = {"type": "None"}
    return tokenizer_json(sp, {
        "normalizer": none if sp["normalizer"] is None else normalizer_json(sp["normalizer"]),
        "pre_tokenizer": none if sp["pre_tokenizer"] is None else pre_tokenizer_json(sp["pre_tokenizer"]),
        "decoder": none if sp["decoder"] is None else decoder_json(sp["decoder"]),
        "post_processor": none if sp["post_processor"] is None else post_processor_json(sp["post_processor"])})


def json_pipelines():
    """name -> (tokenizer.json object, texts): pipelines() and three more that reach the constructors those do
    not (Precompiled, Replace, Prepend, StripAccents, the normal forms; Punctuation, Digits, UnicodeScripts,
    WhitespaceSplit, ByteLevel with the prefix space; CTC, BPE, Strip, Fuse; Roberta and a template with a pair)."""
    out = {name: (spec_json(sp), texts) for name, (sp, texts) in pipelines().items()}
    vocab, merges = random_vocab(11)
    vocab = dict(vocab, **{"<s>": 5000, "</s>": 5001, "<pad>": 5002, "|": 5003})
    texts = random_texts(14, 40, vocab) + ["", "Ａｂc 12 x3y ÉCOLE ﬁn <s>ab</s>", "ab``cd 中文abc кириллица 7"]
    sp = [added("<s>", 950, special=True), added("</s>", 951, special=True), added("<pad>", 952, special=True, rstrip=True)]
    out["precompiled_digits_ctc_roberta"] = (spec_json(spec(
        vocab, merges, ("sequence", [("precompiled", [("ALQAAACAAAAA", "ALQAAACAAAAA")]), ("nfkd",), ("strip_accents",), ("replace", "``", "\""),
                                     ("lowercase",)]),
        ("sequence", [("whitespace_split",), ("punctuation",), ("digits", True)]), ("ctc", "<pad>", "|"),
        ("roberta", ("<s>", 950), ("</s>", 951), False), sp)), texts)
    out["prepend_scripts_bpe_template"] = (spec_json(spec(
        vocab, merges, ("sequence", [("nfd",), ("prepend", "_"), ("nfc",)]), ("sequence", [("unicode_scripts",), ("digits", False)]),
        ("sequence", [("bpe", "_"), ("strip", "_", 1, 0), ("fuse",)]),
        ("template", "<s> $A </s>", "<s> $A </s> $B </s>", [("<s>", 950), ("</s>", 951), ("<pad>", 952)]), sp)), texts)
    out["bytelevel_prefix_space"] = (spec_json(spec(
        vocab, merges, ("nfkc",), ("byte_level", True), ("byte_level",), None, sp)), texts)
    return out
