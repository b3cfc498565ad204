"""The reference's Decoder (src/decoders.rs:30-243) restated in plain Python, for the tests of
complexity_tokenizer.Decoder and of csrc/decoder_hd.h.

A decoder is a tuple: ("byte_level",), ("metaspace", replacement, add_prefix_space),
("wordpiece", prefix, cleanup), ("bpe", suffix), ("ctc", pad_token, word_delimiter_token or None),
("fuse",), ("strip", content, start, stop), ("replace", pattern, replacement) and
("sequence", [decoder, ...]).  `str.replace` stands for Rust's str::replace (both take the leftmost
non-overlapping matches, and both put the replacement around every code point for an empty pattern),
`rstrip(WHITE_SPACE)` for str::trim_end and `bytes.decode("utf-8", "replace")` for
String::from_utf8_lossy (both replace every maximal invalid subpart by one U+FFFD).
"""
import struct

# char::is_whitespace: the 25 White_Space code points
WHITE_SPACE = "".join(chr(c) for c in ([0x09, 0x0A, 0x0B, 0x0C, 0x0D, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B))
                                       + [0x2028, 0x2029, 0x202F, 0x205F, 0x3000]))
KINDS = {"byte_level": 0, "metaspace": 1, "wordpiece": 2, "bpe": 3, "ctc": 4, "fuse": 5, "strip": 6, "replace": 7}
CLEANUP = ((" .", "."), (" ,", ","), (" !", "!"), (" ?", "?"), (" :", ":"), (" ;", ";"), (" '", "'"), ("' ", "'"))


def unicode_to_bytes():
    """:70-91, the reverse of bytes_to_unicode"""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAD)) + list(range(0xAE, 0x100))
    cs = list(bs)
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return {chr(c): b for c, b in zip(cs, bs)}


_BYTE_OF = unicode_to_bytes()


def byte_level(tokens):  # :94-119
    out = bytearray()
    for ch in "".join(tokens):
        if ch == "Ġ":
            out.append(0x20)
        elif ch in _BYTE_OF:
            out.append(_BYTE_OF[ch])
        elif ord(ch) < 0x80:
            out.append(ord(ch))
    return bytes(out).decode("utf-8", "replace")


def metaspace(tokens, replacement, add_prefix_space):  # :122-131
    result = "".join(tokens).replace(replacement, " ")
    if add_prefix_space and result.startswith(" "):
        result = result[1:]
    return result


def wordpiece(tokens, prefix, cleanup):  # :134-162
    result = ""
    for token in tokens:
        if token.startswith(prefix):
            result += token[len(prefix):]
        else:
            if result:
                result += " "
            result += token
    if cleanup:
        for a, b in CLEANUP:
            result = result.replace(a, b)
    return result


def bpe(tokens, suffix):  # :165-178
    result = ""
    for token in tokens:
        if token.endswith(suffix):
            result += token[:len(token) - len(suffix)] + " "
        else:
            result += token
    return result.rstrip(WHITE_SPACE)


def ctc(tokens, pad_token, word_delimiter_token):  # :182-210
    result, prev = [], None
    for token in tokens:
        if token == pad_token:
            prev = None
            continue
        if word_delimiter_token is not None and token == word_delimiter_token:
            result.append(" ")
            prev = None
            continue
        if prev != token:
            result.append(token)
        prev = token
    return "".join(result)


def strip(tokens, content, start, stop):  # :218-243
    result = "".join(tokens)
    for _ in range(min(start, len(result))):
        if not result.startswith(content):
            break
        result = result[len(content):]
    for _ in range(min(stop, len(result))):
        if not result.endswith(content):
            break
        result = result[:len(result) - len(content)]
    return result


def decode(dec, tokens):
    kind = dec[0]
    if kind == "byte_level":
        return byte_level(tokens)
    if kind == "metaspace":
        return metaspace(tokens, dec[1], dec[2])
    if kind == "wordpiece":
        return wordpiece(tokens, dec[1], dec[2])
    if kind == "bpe":
        return bpe(tokens, dec[1])
    if kind == "ctc":
        return ctc(tokens, dec[1], dec[2])
    if kind == "fuse":
        return "".join(tokens)
    if kind == "strip":
        return strip(tokens, dec[1], dec[2], dec[3])
    if kind == "replace":
        return "".join(tokens).replace(dec[1], dec[2])
    if kind == "sequence":  # :57-64
        result = list(tokens)
        for sub in dec[1]:
            result = [decode(sub, result)]
        return "".join(result)
    raise ValueError(kind)


def flat_steps(dec):
    """(kind, flags, a: bytes, b: bytes, cp, start, stop) of include/ctok_decoder.h, sequences flattened
    (the empty sequence is fuse)"""
    kind = dec[0]
    if kind == "sequence":
        return [s for sub in dec[1] for s in flat_steps(sub)] or [(KINDS["fuse"], 0, b"", b"", 0, 0, 0)]
    if kind == "metaspace":
        return [(KINDS[kind], 1 if dec[2] else 0, b"", b"", ord(dec[1]), 0, 0)]
    if kind == "wordpiece":
        return [(KINDS[kind], 1 if dec[2] else 0, dec[1].encode("utf-8"), b"", 0, 0, 0)]
    if kind == "bpe":
        return [(KINDS[kind], 0, dec[1].encode("utf-8"), b"", 0, 0, 0)]
    if kind == "ctc":
        return [(KINDS[kind], 0 if dec[2] is None else 1, dec[1].encode("utf-8"), (dec[2] or "").encode("utf-8"), 0, 0, 0)]
    if kind == "strip":
        return [(KINDS[kind], 0, b"", b"", ord(dec[1]), dec[2], dec[3])]
    if kind == "replace":
        return [(KINDS[kind], 0, dec[1].encode("utf-8"), dec[2].encode("utf-8"), 0, 0, 0)]
    return [(KINDS[kind], 0, b"", b"", 0, 0, 0)]


def pack_steps(dec):
    """the program as tools/decoder_check.cpp reads it"""
    prog = flat_steps(dec)
    return struct.pack("<Q", len(prog)) + b"".join(
        struct.pack("<IIIQQQQ", k, f, cp, start, stop, len(a), len(b)) + a + b for k, f, a, b, cp, start, stop in prog)


def to_decoder(dec, device=0):
    from complexity_tokenizer import Decoder as D
    kind = dec[0]
    if kind == "sequence":
        return D.sequence([to_decoder(sub, device) for sub in dec[1]], device=device)
    return getattr(D, kind)(*dec[1:], device=device)
