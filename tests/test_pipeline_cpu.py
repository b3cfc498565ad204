"""The host side of PipelineTokenizer on the CPU: parse_tokenizer_json against the parser of
tests/pipeline_ref.py over every default / unknown-type / empty-Sequence / null combination of the four
components and both merges forms; and csrc/wordbpe_compile.cpp with the scalar loops of
csrc/wordbpe_hd.h, which the kernels share, by tools/wordbpe_check.cpp built with g++ -- its hard-coded
cases (the duplicate-pair rank, the rank shift after an invalid merge, the panic mark, two vocab strings
sharing an id) and the case table of tests/pipeline_cases.py with the oracle's answers.  No GPU."""
import ctypes
import itertools
import os
import struct
import subprocess

import pytest

from complexity_tokenizer import PipelineTokenizer, parse_tokenizer_json
from complexity_tokenizer import _native as _n
from tests import pipeline_cases as pc
from tests import pipeline_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ABSENT = object()
# per component: left out, null, an object without "type", an unknown type, a type that is no string, an
# empty Sequence, a Sequence of unknown members, a Sequence with one member that parses, a plain member
VARIANTS = {
    "normalizer": ("normalizers", [{"type": "NFKC"}, {"type": "Lowercase"}],
                   [{"type": "BertNormalizer", "strip_accents": False, "clean_text": 1}, {"type": "Precompiled", "precompiled_charsmap": "AAEC"},
                    {"type": "Replace", "pattern": {"String": "``"}, "content": "\""}, {"type": "Prepend", "prepend": "▁"},
                    {"type": "StripAccents"}, {"type": "Strip"}, {"type": "NFD"}, {"type": "NFKD"}, {"type": "NFC"}]),
    "pre_tokenizer": ("pretokenizers", [{"type": "Whitespace"}, {"type": "Digits", "individual_digits": True}],
                      [{"type": "Metaspace", "replacement": "_", "add_prefix_space": False}, {"type": "Metaspace"},
                       {"type": "ByteLevel", "add_prefix_space": True}, {"type": "CharDelimiterSplit", "delimiter": "-|"},
                       {"type": "CharDelimiterSplit"}, {"type": "Split", "pattern": {"Regex": "\\s+"}, "behavior": "Isolated", "invert": True},
                       {"type": "Split", "pattern": {"String": " "}, "behavior": "Nope"}, {"type": "BertPreTokenizer"},
                       {"type": "Punctuation"}, {"type": "UnicodeScripts"}, {"type": "WhitespaceSplit"}, {"type": "Digits"}]),
    "decoder": ("decoders", [{"type": "Fuse"}, {"type": "Strip", "content": " ", "start": 1, "stop": 0}],
                [{"type": "WordPiece"}, {"type": "WordPiece", "prefix": "@@", "cleanup": False}, {"type": "BPE"}, {"type": "BPE", "suffix": "_"},
                 {"type": "CTC"}, {"type": "CTC", "pad_token": "[P]", "word_delimiter_token": "|"}, {"type": "Metaspace", "replacement": ""},
                 {"type": "Strip", "start": True, "stop": 1.5}, {"type": "Strip", "content": "", "start": -1}, {"type": "ByteLevel"},
                 {"type": "Replace", "pattern": {"String": "a"}, "content": "b"}]),
    "post_processor": ("processors", [],
                       [{"type": "TemplateProcessing", "single": [{"SpecialToken": {"id": "[CLS]", "type_id": 0}}, {"Sequence": {"id": "A", "type_id": 0}},
                                                                   {"SpecialToken": {"id": "[SEP]"}}, {"SpecialToken": {"id": 3}}, {"Other": 1}, "x"],
                         "pair": [{"Sequence": {"id": "A"}}, {"Sequence": {"id": "B"}}]},
                        {"type": "TemplateProcessing"}, {"type": "TemplateProcessing", "single": "x", "pair": None},
                        {"type": "RobertaProcessing"}, {"type": "BertProcessing"}, {"type": "ByteLevel"}]),
}


def values_of(key):
    member_key, good, plain = VARIANTS[key]
    seq = lambda members: {"type": "Sequence", member_key: members}  # noqa: E731
    return [ABSENT, None, {"no_type": 1}, [], "NFC", {"type": "Unknown"}, {"type": 7}, {"type": None}, seq([]), {"type": "Sequence"},
            {"type": "Sequence", member_key: {"type": "NFC"}}, seq([{"type": "Unknown"}, {"type": 3}]),
            seq([{"type": "Unknown"}] + good[:1] + [None]), seq(good + [seq(good[1:] + [{"type": "Unknown"}]), seq([])])] + plain


def test_parse_every_component_combination():
    sp = pc.spec(pc.ABC, [("a", "b"), ("b", "c")], added_tokens=[pc.added("[CLS]", 7, special=True), pc.added("<s>", 8, special=True),
                                                                  pc.added("plain", 9)])
    keys = list(VARIANTS)
    # the head of every component's list (defaults, unknown types, sequences) against each other in full ...
    heads = [values_of(k)[:14] for k in keys]
    combos = list(itertools.product(*[h[::3] + h[1:2] for h in heads]))
    # ... and every value of each component once, the others left out
    for i, k in enumerate(keys):
        for v in values_of(k):
            combos.append(tuple(v if j == i else ABSENT for j in range(len(keys))))
    assert len(combos) > 1000
    for combo in combos:
        obj = pc.tokenizer_json(sp, {k: v for k, v in zip(keys, combo) if v is not ABSENT})
        got, want = parse_tokenizer_json(obj), pr.parse_tokenizer_json(obj)
        assert got == want, (combo, got, want)
        assert got["merges"] == [("a", "b"), ("b", "c")]


def test_parse_defaults_by_hand():
    sp = pc.spec(pc.ABC, [])
    got = parse_tokenizer_json(pc.tokenizer_json(sp, {}))
    assert (got["normalizer"], got["pre_tokenizer"], got["decoder"], got["post_processor"]) == (("nfc",), ("byte_level", False), ("byte_level",), None)
    none = {"type": "Unknown"}
    got = parse_tokenizer_json(pc.tokenizer_json(sp, {"normalizer": none, "pre_tokenizer": none, "decoder": none, "post_processor": none}))
    assert (got["normalizer"], got["pre_tokenizer"], got["decoder"], got["post_processor"]) == (None, None, None, None)
    seq = {"type": "Sequence", "normalizers": [none], "pretokenizers": [none], "decoders": [none]}
    got = parse_tokenizer_json(pc.tokenizer_json(sp, {"normalizer": seq, "pre_tokenizer": seq, "decoder": seq}))
    assert (got["normalizer"], got["pre_tokenizer"], got["decoder"]) == (None, None, None)
    got = parse_tokenizer_json(pc.tokenizer_json(sp, {"normalizer": None, "pre_tokenizer": None, "decoder": None, "post_processor": None}))
    assert (got["normalizer"], got["pre_tokenizer"], got["decoder"], got["post_processor"]) == (("nfc",), ("byte_level", False), ("byte_level",), None)


def test_parse_merges_forms():
    for merges, want in (
            (["a b", "b c"], [("a", "b"), ("b", "c")]),
            ([["a", "b"], ["b", "c"]], [("a", "b"), ("b", "c")]),
            (["a b", ["b", "c"], "abc", "a b c", " a", "a ", ["x"], ["x", "y", "z"], ["x", 1], 5, None, ["p q", "r"], ["", ""]],
             [("a", "b"), ("b", "c"), ("", "a"), ("a", ""), ("", "")])):
        obj = {"model": {"vocab": dict(pc.ABC), "merges": merges}}
        assert parse_tokenizer_json(obj)["merges"] == want == pr.parse_tokenizer_json(obj)["merges"]
    assert parse_tokenizer_json({"model": {"vocab": {}}})["merges"] == []
    for bad in ({}, {"model": {}}, {"model": {"vocab": {"a": -1}}}, {"model": {"vocab": {"a": "1"}}}, {"model": {"vocab": {}, "merges": "a b"}},
                {"model": {"vocab": {}}, "added_tokens": [{"id": 1, "content": "x"}]}):
        with pytest.raises(IOError):
            parse_tokenizer_json(bad)


def test_specs_written_as_json_parse_back():
    """tests/pipeline_cases.spec_json is the inverse of the parser: what the GPU suite loads from tokenizer.json
    is the spec it means to load"""
    for name, (sp, _) in pc.pipelines().items():
        got = parse_tokenizer_json(pc.spec_json(sp))
        for k in ("vocab", "merges", "normalizer", "pre_tokenizer", "decoder", "added_tokens"):
            assert got[k] == sp[k], (name, k)
        if sp["post_processor"] is not None:
            assert got["post_processor"][0] == sp["post_processor"][0] and got["post_processor"][1:3] == sp["post_processor"][1:3]
    kinds = set()
    for name, (obj, texts) in pc.json_pipelines().items():
        got = parse_tokenizer_json(obj)
        assert got == pr.parse_tokenizer_json(obj), name

        def walk(t):
            if t is not None:
                kinds.add(t[0])
                for m in (t[1] if t[0] == "sequence" else []):
                    walk(m)
        for k in ("normalizer", "pre_tokenizer", "decoder", "post_processor"):
            walk(got[k])
    assert {"bert", "metaspace", "char_delimiter_split", "strip", "ctc", "precompiled", "roberta", "template", "wordpiece", "bpe", "fuse",
            "byte_level", "nfkc", "nfkd", "nfd", "nfc", "lowercase", "strip_accents", "replace", "prepend", "whitespace",
            "whitespace_split", "punctuation", "digits", "unicode_scripts"} <= kinds


def _s(b):
    return struct.pack("<I", len(b)) + b


def case_file():
    """the case table as tools/wordbpe_check.cpp reads it, with pipeline_ref's answer per word"""
    out, n_words = [], 0
    table = [(sp, texts, None) for sp, texts in list(pc.CASES.values()) + list(pc.pipelines().values())]
    table += [(sp, texts, bad) for sp, texts, bad, _, _ in pc.PANICS.values()]
    for sp, texts, bad in table:
        r = pr.PipelineRef(**sp)
        rec = [struct.pack("<I", len(sp["vocab"]))] + [_s(k.encode()) + struct.pack("<I", v) for k, v in sp["vocab"].items()]
        rec += [struct.pack("<I", len(sp["merges"]))] + [_s(a.encode()) + _s(b.encode()) for a, b in sp["merges"]]
        rec.append(struct.pack("<I", len(sp["added_tokens"])))
        for t in sp["added_tokens"]:
            flags = (1 if t["single_word"] else 0) | (2 if t["lstrip"] else 0) | (4 if t["rstrip"] else 0)
            rec.append(_s(t["content"].encode()) + struct.pack("<II", t["id"], flags))
        words = []
        for text in texts:
            for w in r.words(text):
                for tokenize in (0, 1):
                    try:
                        ids, panics = (r.bpe(w) if tokenize else r._encode_word(w)), 0
                    except pr.PanicException as e:
                        parts = str(e).split()
                        ids, panics = [int(parts[7]), int(parts[-1])], 1  # "... the len is N but the index is R"
                    words.append(_s(w.encode()) + struct.pack("<III", tokenize, panics, len(ids)) + struct.pack("<%dI" % len(ids), *ids))
        rec.append(struct.pack("<I", len(words)))
        n_words += len(words)
        out.append(b"".join(rec + words))
    return struct.pack("<I", len(out)) + b"".join(out), n_words


def test_wordbpe_check(tmp_path):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "wordbpe_check.cpp")
    exe = str(tmp_path / "wordbpe_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    blob, n_words = case_file()
    assert n_words > 5000
    path = tmp_path / "cases.bin"
    path.write_bytes(blob)
    r = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr
    assert "%d words" % n_words in r.stderr


def test_create_without_a_device_reports_it():
    """the C ABI loads; create either works or says that there is no device; the limits are stated"""
    assert {"ctok_pipeline_create", "ctok_pipeline_encode_batch", "ctok_pipeline_encode_batch_device", "ctok_pipeline_stage_ms",
            "ctok_pipeline_stage_name", "ctok_pipeline_limits"} <= set(_n.SIGS)
    lim = PipelineTokenizer.limits()
    assert 0 < lim["tier1"] < lim["tier2"] < lim["max_word_symbols"] and lim["max_merges"] == 1 << 24
    assert lim["max_added_tokens"] >= 300 and lim["max_flagged_word_bytes"] > 0
    assert [_n.lib.ctok_pipeline_stage_name(i) for i in range(7)] == [b"normalize", b"pre_tokenize", b"segments", b"symbols", b"merges",
                                                                       b"emit", b""]
    try:
        PipelineTokenizer.from_components(pc.ABC, [("a", "b")])
    except RuntimeError as e:  # DeviceError
        assert "no HIP device" in str(e)
    # refused at load, before any device is touched
    from complexity_tokenizer import UnsupportedConfigError
    with pytest.raises(UnsupportedConfigError, match="empty content"):
        PipelineTokenizer.from_components(pc.ABC, [], added_tokens=[pc.added("", 9)])
    with pytest.raises(UnsupportedConfigError, match="at most 1024"):
        PipelineTokenizer.from_components(pc.ABC, [], added_tokens=[pc.added("<%d>" % i, i) for i in range(1025)])
    with pytest.raises(UnsupportedConfigError, match="share a first byte hold 32896 bytes"):
        PipelineTokenizer.from_components(pc.ABC, [], added_tokens=[pc.added("<" * 255 + chr(0x100 + i), i) for i in range(128)])
    assert lim["max_added_group_bytes"] == 1 << 15 and lim["max_flagged_word_bytes"] == 1 << 20 and lim["max_batch_bytes"] < 1 << 32
    with pytest.raises(UnsupportedConfigError, match="4294967295"):
        PipelineTokenizer.from_components({"a": 0xFFFFFFFF}, [])
    h = ctypes.c_void_p()
    assert _n.lib.ctok_pipeline_create(None, None, None, 0, ctypes.byref(h)) == _n.CTOK_E_ARG and not h.value
