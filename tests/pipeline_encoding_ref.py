"""TEST INFRASTRUCTURE ONLY -- the reference's Encoding path (src/huggingface/mod.rs:340-480) for a
tokenizer with any normaliser and pre-tokenizer, by composing what the suite already has:

  tests/pipeline_ref.PipelineRef       words (normalise, pre-tokenize), bpe, process
  oracle/ref_py.RefTokenizer           words_with_offsets, encode_from_ids, pad_id_token, call, RefEncoding

New here: encode_single_to_encoding over PipelineRef.words, encode_to_encoding over PipelineRef.process,
and find_work, the work of the word search as include/ctok_pipeline.h defines it.  The product never
imports this module.
"""
from oracle import ref_py
from oracle.ref_py import PanicException, RefEncoding  # noqa: F401  (re-exported for the tests)
from tests import pipeline_ref


class PipelineEncodingRef(pipeline_ref.PipelineRef):
    model_max_length = 512

    def encode_single_to_encoding(self, text, type_id):
        """mod.rs:395-443: the spans first (pre_tokenize_with_offsets panics before any word is
        encoded), then bpe.encode per word, no added-token loop"""
        ids, offsets, word_ids = [], [], []
        for wi, (w, ws, we) in enumerate(self.words_with_offsets(self.words(text), text)):
            pos = ws
            for i in self.bpe(w):
                ids.append(i)
                end = min(pos + len(self.id_to_token_map.get(i, "").encode("utf-8")), we)
                offsets.append((pos, end))
                pos = end
                word_ids.append(wi)
        toks = [self.id_to_token_map.get(i, "") for i in ids]
        n = len(ids)
        return RefEncoding(ids, [type_id] * n, toks, [1] * n, [0] * n, [type_id] * n, offsets, word_ids)

    def encode_to_encoding(self, text, pair=None):
        """encode_to_encoding_impl, mod.rs:358-392: the post-processor in the single form, also for a pair"""
        enc = self.encode_single_to_encoding(text, 0)
        if pair is not None:
            enc.merge(self.encode_single_to_encoding(pair, 1), 1)
        processed = self.process(enc.ids)
        added = len(processed) - len(enc.ids)
        if added < 0:
            raise PanicException("attempt to subtract with overflow")
        enc.ids = processed
        enc.attention_mask += [1] * added
        enc.special_tokens_mask += [1] * added
        enc.type_ids += [0] * added
        sp = set(self.special_tokens.values())
        enc.special_tokens_mask = [1 if i in sp else m for i, m in zip(enc.ids, enc.special_tokens_mask)]
        return enc


def find_work(words, original):
    """The work of pre_tokenize_with_offsets over one sequence: with s where a word's search starts, L
    the text's bytes and m the needle's, pos - s + m on a hit and L - s on a miss, added up."""
    o = original.encode("utf-8")
    work, s = 0, 0
    for w in words:
        trimmed = w.lstrip("Ġ▁")
        needle = (trimmed if trimmed else w).encode("utf-8")
        pos = o.find(needle, s)
        if pos >= 0:
            work += pos - s + len(needle)
            s = pos + len(needle)
        else:
            work += len(o) - s
            s = min(s + len(w.encode("utf-8")), len(o))
    return work


def enc_dict(e):
    """an Encoding of the product as RefEncoding.as_dict gives it"""
    return {"ids": list(e.ids), "type_ids": list(e.type_ids), "tokens": list(e.tokens), "attention_mask": list(e.attention_mask),
            "special_tokens_mask": list(e.special_tokens_mask), "sequence_ids": list(e.sequence_ids),
            "offsets": [tuple(x) for x in e.offsets], "word_ids": list(e.word_ids), "overflowing": [enc_dict(o) for o in e.overflowing]}
