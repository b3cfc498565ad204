"""A literal restatement of the reference's src/postprocessors.rs (Complexity-ML/complexity-tokenizer
v0.3.3) in Python: the char walk of template_process, Sequence's take() of the pair, the pop loop of
truncate's longest_first, pad, and the substring count of added_tokens_*.  What the GPU class and the
CPU check of csrc/postproc_hd.h are compared with.

A processor is a tuple:
  ("template", single, pair_or_None, [(token, id), ...])
  ("bert", (cls_token, cls_id), (sep_token, sep_id))
  ("roberta", (bos_token, bos_id), (eos_token, eos_id), add_prefix_space)
  ("sequence", [processor, ...])
"""
import struct

# char::is_whitespace: the White_Space property (str.strip() would also take U+001C..U+001F)
WHITE_SPACE = set([0x20, 0x85, 0xA0, 0x1680, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000]) | set(range(0x09, 0x0E)) | set(range(0x2000, 0x200B))

DEFAULT = ("template", "<s> $A </s>", "<s> $A </s> $B </s>", [("<s>", 2), ("</s>", 0)])


def _trim(s):
    lo, hi = 0, len(s)
    while lo < hi and ord(s[lo]) in WHITE_SPACE:
        lo += 1
    while hi > lo and ord(s[hi - 1]) in WHITE_SPACE:
        hi -= 1
    return s[lo:hi]


def template_process(ids, pair_ids, single, pair, special_tokens):
    """postprocessors.rs:88-148"""
    template = (pair if pair is not None else single) if pair_ids is not None else single
    result = []
    i = 0
    chars = list(template)
    while i < len(chars):
        if chars[i] == "$" and i + 1 < len(chars):
            if chars[i + 1] == "A":
                result.extend(ids)
                i += 2
            elif chars[i + 1] == "B":
                if pair_ids is not None:
                    result.extend(pair_ids)
                i += 2
            else:
                i += 1
        elif chars[i] == "<" or chars[i] == "[":
            end_char = ">" if chars[i] == "<" else "]"
            start = i
            while i < len(chars) and chars[i] != end_char:
                i += 1
            if i < len(chars):
                i += 1
            token = _trim("".join(chars[start:i]))
            for t, id_ in special_tokens:
                if t == token:
                    result.append(id_)
                    break
        else:
            i += 1
    return result


def bert_process(ids, pair_ids, cls, sep):
    """:151-167"""
    result = [cls[1]]
    result.extend(ids)
    result.append(sep[1])
    if pair_ids is not None:
        result.extend(pair_ids)
        result.append(sep[1])
    return result


def roberta_process(ids, pair_ids, bos, eos):
    """:170-187"""
    result = [bos[1]]
    result.extend(ids)
    result.append(eos[1])
    if pair_ids is not None:
        result.append(eos[1])
        result.extend(pair_ids)
        result.append(eos[1])
    return result


def process(p, ids, pair_ids=None):
    """PostProcessor::process, :34-54"""
    ids = list(ids)
    pair_ids = None if pair_ids is None else list(pair_ids)
    if p[0] == "template":
        return template_process(ids, pair_ids, p[1], p[2], p[3])
    if p[0] == "bert":
        return bert_process(ids, pair_ids, p[1], p[2])
    if p[0] == "roberta":
        return roberta_process(ids, pair_ids, p[1], p[2])
    if p[0] == "sequence":
        result, pair_result = ids, pair_ids
        for q in p[1]:
            taken, pair_result = pair_result, None  # pair_result.take()
            result = process(q, result, taken)
        return result
    raise ValueError(p[0])


def count_special_tokens(template, special_tokens):
    """:190-195"""
    return sum(1 for t, _ in special_tokens if t in template)


def added_tokens_single(p):
    if p[0] == "template":
        return count_special_tokens(p[1], p[3])
    if p[0] in ("bert", "roberta"):
        return 2
    return sum(added_tokens_single(q) for q in p[1])


def added_tokens_pair(p):
    if p[0] == "template":
        return count_special_tokens(p[2], p[3]) if p[2] is not None else 0
    if p[0] == "bert":
        return 3
    if p[0] == "roberta":
        return 4
    return sum(added_tokens_pair(q) for q in p[1])


def truncate(ids, pair_ids, max_length, strategy):
    """:209-254, in place as there; pair_ids None: no pair"""
    total_len = len(ids) + (len(pair_ids) if pair_ids is not None else 0)
    if total_len <= max_length:
        return
    to_remove = total_len - max_length
    if strategy == "only_first":
        remove = min(to_remove, len(ids))
        del ids[len(ids) - remove:]
    elif strategy == "only_second":
        if pair_ids is not None:
            remove = min(to_remove, len(pair_ids))
            del pair_ids[len(pair_ids) - remove:]
    elif strategy == "longest_first":
        remaining = to_remove
        while remaining > 0:
            ids_len = len(ids)
            pair_len = len(pair_ids) if pair_ids is not None else 0
            if ids_len >= pair_len and ids_len > 0:
                ids.pop()
                remaining -= 1
            elif pair_ids is not None:
                if pair_ids:
                    pair_ids.pop()
                    remaining -= 1
            else:
                break
    else:
        raise ValueError(strategy)


def pad(ids, target_length, pad_token_id, pad_left):
    """:266-280; the padded list"""
    if len(ids) >= target_length:
        return list(ids)
    fill = [pad_token_id] * (target_length - len(ids))
    return fill + list(ids) if pad_left else list(ids) + fill


# ---- the masks, which the reference does not have: every id with where it came from ---------------------

A, B, SPECIAL, PAD = 0, 1, 2, 3


def process_tagged(p, ids, pair_ids=None):
    """process over (id, source) cells: the sources of the ids of process(p, ids, pair_ids)"""
    a = [(i, A) for i in ids]
    b = None if pair_ids is None else [(i, B) for i in pair_ids]
    return _tagged(p, a, b)


def _tagged(p, a, b):
    if p[0] == "template":
        return template_process(a, b, p[1], p[2], [(t, (i, SPECIAL)) for t, i in p[3]])
    if p[0] == "bert":
        return bert_process(a, b, (p[1][0], (p[1][1], SPECIAL)), (p[2][0], (p[2][1], SPECIAL)))
    if p[0] == "roberta":
        return roberta_process(a, b, (p[1][0], (p[1][1], SPECIAL)), (p[2][0], (p[2][1], SPECIAL)))
    result, pair_result = a, b
    for q in p[1]:
        taken, pair_result = pair_result, None
        result = _tagged(q, result, taken)
    return result


def process_padded(p, batch, pairs=None, truncate_to=None, strategy="longest_first", pad_to=None, pad_id=0, pad_left=False):
    """truncate, process, pad over a batch, in the order of the free functions: the dict of lists of
    rows that PostProcessor.process_padded returns as arrays.  A cell copied from the first sequence is
    (1, 0, 0) in attention_mask, token_type_ids, special_tokens_mask, one from the pair (1, 1, 0), an
    inserted id (1, 0, 1), padding (0, 0, 1)."""
    pairs = [None] * len(batch) if pairs is None else pairs
    rows = []
    for ids, pr in zip(batch, pairs):
        ids = list(ids)
        pr = None if pr is None else list(pr)
        if truncate_to is not None:
            truncate(ids, pr, truncate_to, strategy)
        rows.append(process_tagged(p, ids, pr))
    longest = max([len(r) for r in rows], default=0)
    width = longest if pad_to in (None, "longest") else max(longest, pad_to)
    out = {"input_ids": [], "attention_mask": [], "token_type_ids": [], "special_tokens_mask": [], "row_len": [len(r) for r in rows],
           "width": width}
    for r in rows:
        cells = pad(r, width, (pad_id, PAD), pad_left)
        out["input_ids"].append([c[0] for c in cells])
        out["attention_mask"].append([int(c[1] != PAD) for c in cells])
        out["token_type_ids"].append([int(c[1] == B) for c in cells])
        out["special_tokens_mask"].append([int(c[1] in (SPECIAL, PAD)) for c in cells])
    return out


# ---- the CPU check's input (tools/postproc_check.cpp) and the GPU class ---------------------------------

STRATEGIES = {"only_first": 0, "only_second": 1, "longest_first": 2}


def flatten(p):
    """the steps of a processor, nested sequences flattened (the pair goes to the first step only,
    so a nested sequence is its steps in place)"""
    if p[0] == "sequence":
        return [s for q in p[1] for s in flatten(q)]
    return [p]


def pack_steps(p):
    """u64 n_steps, per step {u32 kind, flags, id_a, id_b; u64 single_len, pair_len, n_tok; single; pair;
    per token {u64 len; u32 id; bytes}}"""
    steps = flatten(p)
    out = [struct.pack("<Q", len(steps))]
    for s in steps:
        if s[0] == "template":
            single, pair = s[1].encode(), (s[2] or "").encode()
            out.append(struct.pack("<IIIIQQQ", 0, 1 if s[2] is not None else 0, 0, 0, len(single), len(pair), len(s[3])))
            out += [single, pair]
            for t, i in s[3]:
                raw = t.encode()
                out += [struct.pack("<QI", len(raw), i), raw]
        else:
            out.append(struct.pack("<IIIIQQQ", 1 if s[0] == "bert" else 2, 0, s[1][1], s[2][1], 0, 0, 0))
    return b"".join(out)


def to_postprocessor(p):
    from complexity_tokenizer import PostProcessor

    if p[0] == "template":
        return PostProcessor.template(p[1], p[2], list(p[3]))
    if p[0] == "bert":
        return PostProcessor.bert(p[1][0], p[1][1], p[2][0], p[2][1])
    if p[0] == "roberta":
        return PostProcessor.roberta(p[1][0], p[1][1], p[2][0], p[2][1], p[3])
    return PostProcessor.sequence([to_postprocessor(q) for q in p[1]])
