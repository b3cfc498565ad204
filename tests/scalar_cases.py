"""Inputs and expected ids for the every-scalar, word-straddle, tile-edge and NFC-window tests of
the fused encode path (tests/test_scalar_cases_cpu.py ties them to the C oracle,
tests/test_gpu_scalars.py runs them on the GPU).  Generators only: nothing here touches a device.

The probe tokenizer makes ids readable as bytes.  Its vocab is the 256 byte chars with id = byte;
for each prefix P of PREFIXES (index pi) and each UTF-8 lead byte 0xC2..0xF4 it holds one merge
(char(P), char(lead)) whose token has the id 256 + pi * 51 + (lead - 0xC2).  The normalizer is null
(= NFC) and the pre-tokenizer ByteLevel, so the ids of a document spell the bytes of its NFC form,
and a merged first token shows that P and the following non-ASCII character fell into one piece:
P = "a" joins a letter, "1" a number, "!" any other non-space, a tab a whitespace character.  That
is the class k_segment gave the character.

Closed-form rule (rule_ids; vectorised in expected()): N = NFC(doc), with " " in front when
add_prefix_space is set and N is non-empty and does not start with " ".  The ids are N's bytes,
except that when P stands at index 0 (1 behind the added space), the next character is non-ASCII
and its class (classes()) equals pi, P's byte and the lead byte become the merged id.
"""
import functools
import unicodedata

import numpy as np
import regex

from tests import toys

NCP = 0x110000
PREFIXES = [b"a", b"1", b"!", b"\t"]
SUFFIXES = [b"a", b"1", b"!", b"\t\t"]  # what follows X in the suffix documents (the second tab is context)
LEAD0, N_LEADS = 0xC2, 0xF4 - 0xC2 + 1  # 51 lead bytes
SUFFIX_ID0 = 256 + 4 * N_LEADS  # 460: the first suffix-merged id
TILE = 3968  # k_segment's tile: 62 words of 64 bytes


# ------------------------------------------------------------------------------- tokenizers
def probe_obj(add_prefix_space=False, suffixes=False):
    """The probe tokenizer.  suffixes: also one merge (char(tail), char(S)) for each continuation
    byte 0x80..0xBF and each first byte S of SUFFIXES, with the id 460 + si * 64 + (tail - 0x80): a
    merged token behind X shows that X's last byte and the following character fell into one
    piece, that is the class the device gave X's last byte (the (P, lead) merges show only the
    class of its first).  The class of a code point whose lead byte lies in the previous 64-byte
    word comes from a route of its own in k_segment (lead_cont) and covers just those last bytes."""
    bm = toys.byte_map()
    vocab = {bm[b]: b for b in range(256)}
    merges = []
    for pi, p in enumerate(PREFIXES):
        for lead in range(LEAD0, LEAD0 + N_LEADS):
            vocab[bm[p[0]] + bm[lead]] = 256 + pi * N_LEADS + (lead - LEAD0)
            merges.append((bm[p[0]], bm[lead]))
    if suffixes:
        for si, sfx in enumerate(SUFFIXES):
            for tail in range(0x80, 0xC0):
                vocab[bm[tail] + bm[sfx[0]]] = SUFFIX_ID0 + si * 64 + (tail - 0x80)
                merges.append((bm[tail], bm[sfx[0]]))
    return toys.tok_json(vocab, merges, pre_tokenizer={"type": "ByteLevel", "add_prefix_space": bool(add_prefix_space),
                                                       "trim_offsets": True, "use_regex": True})


def bytes_obj(add_prefix_space=False):
    """The 256 byte chars, id = byte, no merge: ids are the bytes of the normalised text."""
    bm = toys.byte_map()
    return toys.tok_json({bm[b]: b for b in range(256)}, [],
                         pre_tokenizer={"type": "ByteLevel", "add_prefix_space": bool(add_prefix_space),
                                        "trim_offsets": True, "use_regex": True})


# ------------------------------------------------------------------- scalars, classes, flags
@functools.lru_cache(None)
def scalars():
    """Every Unicode scalar value, ascending (1,112,064)."""
    return np.concatenate([np.arange(0, 0xD800), np.arange(0xE000, NCP)]).astype(np.int64)


@functools.lru_cache(None)
def classes():
    """int8[NCP]: the probe's class of a code point, from the `regex` module (the pre-tokenizer's
    classes): \\p{L} -> 0, else \\p{N} -> 1, else \\s -> 3, else 2 (the index of the prefix that
    joins it)."""
    text = "".join(map(chr, range(NCP)))
    out = np.full(NCP, 2, dtype=np.int8)
    for pat, v in ((r"\s", 3), (r"\p{N}", 1), (r"\p{L}", 0)):
        out[[m.start() for m in regex.finditer(pat, text)]] = v
    return out


@functools.lru_cache(None)
def flags():
    """bool[NCP]: NFC may touch the code point: NFC changes it, or its combining class is not 0,
    or it is the second element of a primary composite, or a Hangul V / T jamo (derived from
    `unicodedata` as tests/test_unicode_tables.py derives NFC_QC)."""
    f = np.zeros(NCP, dtype=bool)
    for cp in scalars().tolist():
        c = chr(cp)
        stable = unicodedata.normalize("NFC", c) == c
        if not stable or unicodedata.combining(c):
            f[cp] = True
        d = unicodedata.decomposition(c)
        if stable and d and not d.startswith("<"):
            parts = d.split()
            if len(parts) == 2:
                f[int(parts[1], 16)] = True
    f[0x1161:0x1176] = True
    f[0x11A8:0x11C3] = True
    return f


def flagged_scalars():
    return np.flatnonzero(flags()).astype(np.int64)


def inert_scalars():
    sc = scalars()
    return sc[~flags()[sc]]


def has_flagged(s: str) -> bool:
    f = flags()
    return any(f[ord(c)] for c in s)


@functools.lru_cache(None)
def run_edges():
    """The first and last scalar of every run of equal (class, flag) over the ascending scalars."""
    sc = scalars()
    key = classes()[sc].astype(np.int64) * 2 + flags()[sc]
    ch = np.flatnonzero(key[1:] != key[:-1])
    e = np.zeros(len(sc), dtype=bool)
    e[0] = e[-1] = True
    e[ch] = True
    e[ch + 1] = True
    return sc[e]


@functools.lru_cache(None)
def subset():
    """Run edges, every flagged scalar and every 61st scalar (23,239), ascending."""
    sc = scalars()
    keep = np.zeros(NCP, dtype=bool)
    keep[run_edges()] = True
    keep[flagged_scalars()] = True
    keep[sc[::61]] = True
    return np.flatnonzero(keep).astype(np.int64)


# --------------------------------------------------------------------------- packed batches
def utf8_matrix(cps):
    """(uint8[n, 4], int64[n]): the UTF-8 bytes of each scalar, left-aligned, and their count."""
    c = np.asarray(cps, dtype=np.int64)
    n = 1 + (c >= 0x80) + (c >= 0x800) + (c >= 0x10000)
    u = np.zeros((len(c), 4), dtype=np.uint8)
    m1, m2, m3, m4 = n == 1, n == 2, n == 3, n == 4
    u[m1, 0] = c[m1]
    u[m2, 0] = 0xC0 | (c[m2] >> 6)
    u[m2, 1] = 0x80 | (c[m2] & 63)
    u[m3, 0] = 0xE0 | (c[m3] >> 12)
    u[m3, 1] = 0x80 | ((c[m3] >> 6) & 63)
    u[m3, 2] = 0x80 | (c[m3] & 63)
    u[m4, 0] = 0xF0 | (c[m4] >> 18)
    u[m4, 1] = 0x80 | ((c[m4] >> 12) & 63)
    u[m4, 2] = 0x80 | ((c[m4] >> 6) & 63)
    u[m4, 3] = 0x80 | (c[m4] & 63)
    return u, n.astype(np.int64)


def _flatten(rows, counts):
    """Row-major concatenation of rows[i, :counts[i]] and the offsets (uint64[n + 1])."""
    keep = np.arange(rows.shape[1])[None, :] < counts[:, None]
    off = np.zeros(len(counts) + 1, dtype=np.uint64)
    np.cumsum(counts, out=off[1:])
    return rows[keep], off


def pack(docs):
    """bytes documents -> (uint8 text with 64 spare zero bytes behind it, uint64 offsets)."""
    off = np.zeros(len(docs) + 1, dtype=np.uint64)
    np.cumsum([len(d) for d in docs], out=off[1:])
    return np.frombuffer(b"".join(docs) + b"\0" * 64, dtype=np.uint8), off


def px_docs(cps, prefixes=range(4)):
    """The documents P + X, prefix-major (all X behind PREFIXES[0], then PREFIXES[1], ...), packed."""
    u, n = utf8_matrix(cps)
    texts, lens = [], []
    for pi in prefixes:
        rows = np.empty((len(n), 5), dtype=np.uint8)
        rows[:, 0] = PREFIXES[pi][0]
        rows[:, 1:] = u
        t, _ = _flatten(rows, n + 1)
        texts.append(t)
        lens.append(n + 1)
    off = np.zeros(sum(map(len, lens)) + 1, dtype=np.uint64)
    np.cumsum(np.concatenate(lens), out=off[1:])
    return np.concatenate(texts + [np.zeros(64, dtype=np.uint8)]), off


def rule_ids(doc: str, pi: int, add_prefix_space=False):
    """The closed-form rule for one document (see the module docstring)."""
    n = unicodedata.normalize("NFC", doc)
    k = 0
    if add_prefix_space and n and not n.startswith(" "):
        n, k = " " + n, 1
    ids = list(n.encode("utf-8"))
    p = PREFIXES[pi].decode()
    if n[k:k + 1] == p and len(n) > k + 1 and ord(n[k + 1]) >= 0x80 and classes()[ord(n[k + 1])] == pi:
        ids[k:k + 2] = [256 + pi * N_LEADS + (ids[k + 1] - LEAD0)]
    return ids


def expected(cps, add_prefix_space=False, prefixes=range(4)):
    """(ids uint32[T], tok_off uint64[D + 1]) of px_docs(cps, prefixes) by the closed-form rule.
    Vectorised: a document whose X is unflagged is left alone by NFC, so its ids follow from X's
    UTF-8 bytes and class; only the documents of flagged X go through rule_ids one by one."""
    c = np.asarray(cps, dtype=np.int64)
    u, n = utf8_matrix(c)
    cl, fl = classes()[c], flags()[c]
    fidx = np.flatnonzero(fl)
    sp = 1 if add_prefix_space else 0
    all_ids, all_cnt = [], []
    for pi in prefixes:
        special = [rule_ids(PREFIXES[pi].decode() + chr(c[i]), pi, add_prefix_space) for i in fidx.tolist()]
        width = max([6] + [len(s) for s in special])
        rows = np.zeros((len(c), width), dtype=np.uint32)
        merged = (c >= 0x80) & (cl == pi)
        cnt = sp + 1 + n - merged
        rows[:, 0] = 0x20  # (overwritten just below without the prefix space)
        k = sp
        rows[:, k] = PREFIXES[pi][0]
        for j in range(4):  # X's bytes behind P, or one slot earlier with the lead merged into P's
            dst = k + 1 + j - merged.astype(np.int64)
            ok = j < n
            rows[np.flatnonzero(ok), dst[ok]] = u[ok, j]
        mrow = np.flatnonzero(merged)
        rows[mrow, k] = 256 + pi * N_LEADS + (u[mrow, 0].astype(np.uint32) - LEAD0)
        for i, s in zip(fidx.tolist(), special):
            rows[i, :len(s)] = s
            cnt[i] = len(s)
        ids, _ = _flatten(rows, cnt)
        all_ids.append(ids)
        all_cnt.append(cnt)
    tok_off = np.zeros(sum(map(len, all_cnt)) + 1, dtype=np.uint64)
    np.cumsum(np.concatenate(all_cnt), out=tok_off[1:])
    return np.concatenate(all_ids), tok_off


def merged_counts(ids):
    """How many merged first tokens each prefix has in ids."""
    m = ids[ids >= 256].astype(np.int64) - 256
    return [int(((m // N_LEADS) == pi).sum()) for pi in range(4)]


# ------------------------------------------------------------- 64-byte documents and straddles
def alternating(cps):
    """cps reordered so that flagged and unflagged scalars alternate for as long as both last."""
    c = np.asarray(cps, dtype=np.int64)
    f = flags()[c]
    a, b = c[f], c[~f]
    k = min(len(a), len(b))
    head = np.empty(2 * k, dtype=np.int64)
    head[0::2] = a[:k]
    head[1::2] = b[:k]
    return np.concatenate([head, a[k:], b[k:]])


def word_docs(cps, prefixes=range(4), lead_bytes=0, suffix=False):
    """64-byte documents P + X + "x" * (63 - len(X)), prefix-major, behind one leading document of
    lead_bytes "x" (none when 0), packed.  With lead_bytes = 0 every document is one 64-byte word.
    suffix: SUFFIXES[pi] stands right behind X (P + X + S + "x" ...), for probe_obj(suffixes=True)."""
    u, n = utf8_matrix(cps)
    blocks = []
    for pi in prefixes:
        rows = np.full((len(n), 64), ord("x"), dtype=np.uint8)
        rows[:, 0] = PREFIXES[pi][0]
        for j in range(4):
            ok = j < n
            rows[ok, 1 + j] = u[ok, j]
        if suffix:
            for j, b in enumerate(SUFFIXES[pi]):
                rows[np.arange(len(n)), 1 + n + j] = b
        blocks.append(rows.reshape(-1))
    nd = len(n) * len(list(prefixes))
    lens = [lead_bytes] * (1 if lead_bytes else 0) + [64] * nd
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    np.cumsum(lens, out=off[1:])
    text = np.concatenate([np.full(lead_bytes, ord("x"), dtype=np.uint8)] + blocks + [np.zeros(64, dtype=np.uint8)])
    return text, off


@functools.lru_cache(None)
def tile_representatives():
    """One scalar per (class, UTF-8 length 2 / 3 / 4, flagged / unflagged) combination that exists:
    the lowest one."""
    sc = scalars()
    sc = sc[sc >= 0x80]
    _, n = utf8_matrix(sc)
    key = (classes()[sc].astype(np.int64) * 8 + n) * 2 + flags()[sc]
    _, first = np.unique(key, return_index=True)
    return sc[np.sort(first)]


def tile_edge_docs():
    """(docs, placed): for each representative X, each prefix, back = 1, 2, 3 and both placements,
    one block of exactly three tiles (3 * TILE bytes) of documents in which X's lead byte falls
    `back` bytes before the block's byte TILE and before its byte 2 * TILE: in the middle of a
    document and with P + X as the document's last bytes, each without and with SUFFIXES[pi] behind X.  The blocks follow one another in
    one batch that starts at byte 0, so every block's edges are tile edges.  The rest is short ASCII
    documents.  placed: [(byte position of the lead byte, code point)]."""
    fill = b"the quick brown fox jumps over 12 lazy dogs, twice! "
    docs, placed, pos = [], [], 0
    for cp in tile_representatives().tolist():
        x = chr(cp).encode()
        for p, sfx in zip(PREFIXES, SUFFIXES):
            for back in (1, 2, 3):
                for at_end, sx in ((False, b""), (True, b""), (False, sfx), (True, sfx)):
                    start = pos
                    for edge in (start + TILE, start + 2 * TILE):
                        lead = edge - back  # X's lead byte; P one byte before it
                        while lead - 1 - pos > 200:
                            k = 37 + (pos % 23)
                            docs.append((fill * 2)[:k])
                            pos += k
                        body = (fill * 5)[:lead - 1 - pos] + p + x + sx + (b"" if at_end else b" tail of the document")
                        docs.append(body)
                        placed.append((lead, cp))
                        pos += len(body)
                    while pos < start + 3 * TILE:
                        k = min(41 + (pos % 19), start + 3 * TILE - pos)
                        docs.append((fill * 2)[:k])
                        pos += k
    return docs, placed


# --------------------------------------------------------------------------- NFC scenarios
EXPANSIONS = [0x0344, 0x0958, 0x0F73, 0xFB2C, 0x1D15E, 0x1D160, 0x1D1BB, 0x2F800, 0xF900]
SBASE, LBASE, VBASE, TBASE = 0xAC00, 0x1100, 0x1161, 0x11A7
_LV = [(0, 0), (7, 9), (18, 20)]  # (L index, V index) of the three LV syllables used with every T


def _mark_run(n, descending):
    a, b = "\u0301", "\u0323"  # classes 230 and 220
    s = "".join((a if i % 2 == 0 else b) for i in range(n))
    if descending:
        s = a * (n // 2) + b * (n - n // 2)
    return "a" + s


@functools.lru_cache(None)
def nfc_scenarios():
    """[(kind, string)]; kind "plain" or one of "expansion", "hangul_t", "run" (the kinds that
    get every fill length 0..66)."""
    out = []
    sc = scalars().tolist()
    for cp in sc:
        if SBASE <= cp < SBASE + 11172:
            continue
        c = chr(cp)
        d = unicodedata.normalize("NFD", c)
        if d != c:
            out.append(("plain", d))
            out.append(("plain", c))
    for cp in sc:  # two-part canonical decompositions, composition exclusions included
        d = unicodedata.decomposition(chr(cp))
        if d and not d.startswith("<"):
            parts = d.split()
            if len(parts) == 2:
                out.append(("plain", chr(int(parts[0], 16)) + chr(int(parts[1], 16))))
    for li in range(19):
        for vi in range(21):
            out.append(("plain", chr(LBASE + li) + chr(VBASE + vi)))
    for ti in range(1, 28):
        for li, vi in _LV:
            lv = SBASE + (li * 21 + vi) * 28
            out.append(("hangul_t", chr(lv) + chr(TBASE + ti)))
            out.append(("hangul_t", chr(LBASE + li) + chr(VBASE + vi) + chr(TBASE + ti)))
            out.append(("hangul_t", chr(lv + 1 + (ti % 27)) + chr(TBASE + ti)))  # LVT + T: stays
    lowest = {}
    for cp in sc:
        cc = unicodedata.combining(chr(cp))
        if cc and cc not in lowest:
            lowest[cc] = chr(cp)
    marks = [lowest[cc] for cc in sorted(lowest)]
    assert len(marks) == 55
    for m1 in marks:
        for m2 in marks:
            out.append(("plain", "a" + m1 + m2))
            out.append(("plain", "e" + m1 + m2 + "\u0301"))
    for cp in EXPANSIONS:
        out.append(("expansion", chr(cp) * 40))
    out.append(("plain", "\u0301\u0323"))       # only marks
    out.append(("plain", "\u0323\u0301abc"))    # starts with a mark
    out.append(("end", "abce\u0301"))           # ends inside a segment (no trailing "y")
    out.append(("end", "abc\u1100\u1161"))
    for n in (64, 256):
        out.append(("run", _mark_run(n, False)))
        out.append(("run", _mark_run(n, True)))
    return out


def _drop_leading_starter(s):
    """s without its first character when that one is a stable starter (not flagged)."""
    return s[1:] if s and not flags()[ord(s[0])] else s


@functools.lru_cache(None)
def nfc_window_docs():
    """Every scenario under every layout: a list of str documents fill + scenario + "y" ("end"
    scenarios without the "y": the document ends inside the segment).

    * fill = "x" * s, s in {0, 60, 61, 62, 63, 64}, every scenario;
    * fill = "x" * s for every s in 0..66: every 10th scenario and all expansion, Hangul-T, end and
      run scenarios;
    * fill = U+4E00 * 21 + "x" * r and U+1F600 * 15 + "x" * (r + 1), r in 0..3, every scenario: a
      stable 3- or 4-byte character across the 64-byte window's end, and the character before the
      scenario in the previous window;
    * fill = "x" * 62 + "e" and "x" * 63 + "e" with the scenario's leading stable starter dropped:
      the second puts the boundary that nfc_doc pops at lane 63 of a window without an unstable
      code point and the unstable one at lane 0 of the next.
    """
    scen = nfc_scenarios()
    docs = []

    def add(fill, kind, s):
        docs.append(fill + s + ("" if kind == "end" else "y"))

    for i, (kind, s) in enumerate(scen):
        for n in (0, 60, 61, 62, 63, 64):
            add("x" * n, kind, s)
        if i % 10 == 0 or kind != "plain":
            for n in range(67):
                add("x" * n, kind, s)
        for r in range(4):
            add("\u4e00" * 21 + "x" * r, kind, s)
            add("\U0001f600" * 15 + "x" * (r + 1), kind, s)
        t = _drop_leading_starter(s)
        add("x" * 62 + "e", kind, t)
        add("x" * 63 + "e", kind, t)
    return docs


def nfc_expected(docs, add_prefix_space=False):
    """(text, off, ids, tok_off) for the no-merge byte tokenizer: ids are the bytes of NFC(doc),
    behind " " when add_prefix_space is set and the result is non-empty and starts with no " "."""
    raw = [d.encode() for d in docs]
    want = []
    for d in docs:
        n = unicodedata.normalize("NFC", d)
        if add_prefix_space and n and not n.startswith(" "):
            n = " " + n
        want.append(n.encode())
    text, off = pack(raw)
    wt, woff = pack(want)
    return text, off, wt[:int(woff[-1])].astype(np.uint32), woff
