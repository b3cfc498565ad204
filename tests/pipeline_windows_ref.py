"""TEST INFRASTRUCTURE ONLY -- the array form of PipelineTokenizer.encode_padded / encode_windows from the
reference's lists: PipelineEncodingRef.encode_to_encoding / encode_from_ids, then RefEncoding.truncate,
truncate_with_stride and pad, by the recipe of RefTokenizer.call (oracle/ref_py.py:415-436).  Mode "cut"
drops the remainder encoding.  The product never imports this module.

Also the worlds and inputs that tests/test_gpu_pipeline_windows.py runs on the GPU, so that
tests/test_pipeline_windows_ref_cpu.py can confirm on the CPU which of them the reference panics on.
"""
import numpy as np

from tests import pipeline_cases as pc
from tests.pipeline_encoding_ref import PanicException, PipelineEncodingRef

NONE = 0xFFFFFFFF

ABQ = {"a": 0, "b": 1, "c": 2, "q": 3, "r": 4, "x": 5, "ab": 6, "[CLS]": 7, "[SEP]": 8, "<s>": 9, "</s>": 10}
SPECIAL = [pc.added("[CLS]", 7, special=True), pc.added("[SEP]", 8, special=True), pc.added("<s>", 9, special=True),
           pc.added("</s>", 10, special=True), pc.added("<pad>", 11, special=True)]
BERT = ("bert", ("[CLS]", 7), ("[SEP]", 8))
ROBERTA = ("roberta", ("<s>", 9), ("</s>", 10), False)
NOTHING = ("template", "$A", None, [])  # a template that adds nothing
LETTERS = "abcqrx"


def world_spec(vocab=ABQ, merges=(("a", "b"),), normalizer=None, pre_tokenizer=("whitespace",), post_processor=None, added=SPECIAL):
    return pc.spec(vocab, list(merges), normalizer, pre_tokenizer, None, post_processor, added)


def row(n, shift=0):
    """a text of n one-letter words: n ids, no merge"""
    return " ".join(LETTERS[(i + shift) % len(LETTERS)] for i in range(n))


def boundary_cases():
    """(m, stride, texts): rows at every length where a window begins or ends"""
    out = []
    for m in (1, 2, 63, 64, 65, 256, 257):
        for stride in sorted({0, 1, m - 1}):
            if stride >= m:
                continue
            lens = sorted({0, 1, m - 1, m, m + 1, 2 * m - stride, 2 * m - stride + 1})
            out.append((m, stride, [row(n, i) for i, n in enumerate(lens)]))
    return out


def many_windows_texts():
    """one row of 5,000 ids next to 3,000 short rows, with empty rows first, last and in the middle"""
    texts = [""] + [row(i % 5, i) for i in range(1500)] + ["", row(5000), ""] + [row(1 + i % 4, i) for i in range(1500)] + [""]
    return texts


def windows_ref(ref, texts, pairs=None, *, mode, max_length=None, stride=0, add_special_tokens=True, padding=None, pad_left=False,
                pad_id=None):
    """mode None (no truncation), "cut" or "windows".  A dict of arrays, or the PanicException of the lowest row."""
    m = max_length if max_length is not None else ref.model_max_length
    try:
        if add_special_tokens:
            encs = [ref.encode_to_encoding(t, pairs[i] if pairs is not None else None) for i, t in enumerate(texts)]
        else:
            encs = [ref.encode_from_ids(t, pairs[i] if pairs is not None else None) for i, t in enumerate(texts)]
        for e in encs:
            if mode is not None and len(e.ids) > m:
                if mode == "windows":
                    e.truncate_with_stride(m, stride)
                else:
                    e.truncate(m)
                    e.overflowing = []
    except PanicException as exc:
        return exc
    target = 0
    if padding is not None:
        target = m if padding == "max_length" else max((len(e.ids) for e in encs), default=0)
        pid, ptok = ref.pad_id_token()
        if pad_id is not None:
            pid = pad_id
        for e in encs:
            e.pad(target, pid, ptok, pad_left)
    else:
        pid = pad_id if pad_id is not None else ref.pad_id_token()[0]
    wins, rows_of, starts, row_window = [], [], [], [0]
    for r, e in enumerate(encs):
        for k, w in enumerate([e] + e.overflowing):
            wins.append(w)
            rows_of.append(r)
            starts.append(k * (m - stride) if k else 0)
        row_window.append(len(wins))
    n = len(wins)
    width = max([len(w.ids) for w in wins] + [target if n else 0])

    def cells(field, fill):
        a = np.full((n, width), fill, dtype=np.uint32)
        for i, w in enumerate(wins):
            v = [NONE if x is None else x for x in getattr(w, field)]
            a[i, :len(v)] = v
        return a

    offs = np.zeros((n, width, 2), dtype=np.uint64)
    for i, w in enumerate(wins):
        if w.offsets:
            offs[i, :len(w.offsets)] = w.offsets
    i64 = lambda v: np.asarray(v, dtype=np.int64)  # noqa: E731
    return {"input_ids": cells("ids", pid), "attention_mask": cells("attention_mask", 0), "token_type_ids": cells("type_ids", 0),
            "special_tokens_mask": cells("special_tokens_mask", 1), "row_len": i64([len(w.ids) for w in wins]),
            "overflow_to_sample_mapping": i64(rows_of), "window_start": i64(starts), "row_window": i64(row_window),
            "offset_mapping": offs, "word_ids": cells("word_ids", NONE), "offsets_len": i64([len(w.offsets) for w in wins]),
            "sequence_ids": cells("sequence_ids", NONE), "sequence_len": i64([len(w.sequence_ids) for w in wins])}


def make_ref(**kw):
    return PipelineEncodingRef(**world_spec(**kw))
