#!/usr/bin/env python3
"""Writes csrc/gen/normalize_data.h: the tables of csrc/normalize_hd.h (UAX #15 normalisation).

Everything comes from this interpreter's unicodedata:
  - the full canonical and full compatibility decomposition of a code point is its
    unicodedata.decomposition() mapping applied recursively (Hangul syllables are algorithmic and
    not in the tables); both are checked against unicodedata.normalize("NFD" / "NFKD");
  - the combining class is unicodedata.combining();
  - a primary composite is a code point whose one-level canonical decomposition "a b" composes
    back to it under NFC (which leaves out singletons, the composition exclusions and the
    non-starter decompositions);
  - per form one "stable" bit: combining class 0 and quick check Yes.  Quick check No is
    normalize(form, c) != c; Maybe (the C forms only) is the set of second code points of the
    primary composites plus the Hangul V and T jamo.
Usage: gen_normalize_tables.py [out.h]
"""
import os
import sys
import unicodedata

SCALARS = [c for c in range(0x110000) if not 0xD800 <= c < 0xE000]
S_BASE, L_BASE, V_BASE, T_BASE = 0xAC00, 0x1100, 0x1161, 0x11A7
L_COUNT, V_COUNT, T_COUNT = 19, 21, 28
S_COUNT = L_COUNT * V_COUNT * T_COUNT
RUN_SHIFT = 8  # the property runs are indexed per 2^RUN_SHIFT code points,
INDEXED = 0x30000  # below this code point (above it lie a handful of runs)

# bits of a property word above the combining class (csrc/normalize_hd.h)
P_HAS_D, P_HAS_K, P_SECOND = 1 << 8, 1 << 9, 1 << 10
P_STABLE = {"NFC": 1 << 11, "NFD": 1 << 12, "NFKC": 1 << 13, "NFKD": 1 << 14}
P_K_IS_D = 1 << 15  # the compatibility decomposition is the canonical one


def one_level(c):
    """(mapping, is_compat) of unicodedata.decomposition, or None"""
    d = unicodedata.decomposition(chr(c))
    if not d:
        return None
    parts = d.split()
    compat = parts[0].startswith("<")
    if compat:
        parts = parts[1:]
    return [int(p, 16) for p in parts], compat


def full(c, compat):
    m = one_level(c)
    if m is None or (m[1] and not compat):
        return [c]
    out = []
    for x in m[0]:
        out += full(x, compat)
    return out


def tables():
    decomp_d, decomp_k = {}, {}
    for c in SCALARS:
        if S_BASE <= c < S_BASE + S_COUNT:
            continue
        d, k = full(c, False), full(c, True)
        if d != [c]:
            decomp_d[c] = d
        if k != [c]:
            decomp_k[c] = k
    pairs = {}
    for c in SCALARS:
        m = one_level(c)
        if m is None or m[1] or len(m[0]) != 2:
            continue
        a, b = m[0]
        if unicodedata.normalize("NFC", chr(a) + chr(b)) == chr(c):
            assert (a, b) not in pairs
            pairs[(a, b)] = c
    seconds = {b for _, b in pairs} | set(range(V_BASE, V_BASE + V_COUNT)) | set(range(T_BASE + 1, T_BASE + T_COUNT))
    props = {}
    for c in SCALARS:
        ch = chr(c)
        p = unicodedata.combining(ch)
        if c in decomp_d:
            p |= P_HAS_D
        if c in decomp_k:
            p |= P_HAS_K
        if c in seconds:
            p |= P_SECOND
        if unicodedata.combining(ch) == 0:
            for form, bit in P_STABLE.items():
                maybe = form in ("NFC", "NFKC") and c in seconds
                if unicodedata.normalize(form, ch) == ch and not maybe:
                    p |= bit
        props[c] = p
    return decomp_d, decomp_k, pairs, props


def facts(decomp_d, decomp_k):
    """The expansion facts DESIGN.md 4.6g records; every kernel sizes its output by a count pass,
    so they are documentation, asserted here."""
    def hangul(c):
        if not S_BASE <= c < S_BASE + S_COUNT:
            return None
        s = c - S_BASE
        out = [L_BASE + s // (V_COUNT * T_COUNT), V_BASE + s % (V_COUNT * T_COUNT) // T_COUNT]
        if s % T_COUNT:
            out.append(T_BASE + s % T_COUNT)
        return out
    f = {}
    for name, table, form in (("nfd", decomp_d, "NFD"), ("nfkd", decomp_k, "NFKD")):
        most, most_c, ratio = 1, 0, 1.0
        for c in SCALARS:
            d = hangul(c) or table.get(c, [c])
            assert "".join(map(chr, d)) == unicodedata.normalize(form, chr(c)), hex(c)
            if len(d) > most:
                most, most_c = len(d), c
            ratio = max(ratio, len("".join(map(chr, d)).encode()) / len(chr(c).encode()))
        f[name] = (most, most_c, ratio)
    for form in ("NFC", "NFKC"):
        f[form.lower()] = max(len(unicodedata.normalize(form, chr(c))) for c in SCALARS), \
            max(len(unicodedata.normalize(form, chr(c)).encode()) / len(chr(c).encode()) for c in SCALARS)
    assert f["nfd"] == (4, 0x1F82, 3.0), f["nfd"]
    assert f["nfkd"] == (18, 0xFDFA, 11.0), f["nfkd"]
    assert f["nfc"][1] <= 3.0 and f["nfkc"] == (18, 11.0), (f["nfc"], f["nfkc"])
    return f


def emit(ctype, name, vals, per_line=32):
    lines = ["NZ_DATA_ATTR static const %s %s[%d] = {" % (ctype, name, len(vals))]
    for i in range(0, len(vals), per_line):
        lines.append(",".join("%d" % v for v in vals[i:i + per_line]) + ",")
    lines.append("};")
    return "\n".join(lines)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "csrc", "gen", "normalize_data.h")
    decomp_d, decomp_k, pairs, props = tables()
    facts(decomp_d, decomp_k)
    # The compatibility table holds only what differs from the canonical one (P_K_IS_D marks the
    # rest).  One pool of code points serves both: the longest decompositions go in first and a
    # decomposition found inside what is already there is not stored again.  An entry is
    # (code point, offset << 5 | length).
    only_k = {c: k for c, k in decomp_k.items() if decomp_d.get(c) != k}
    for c in decomp_k:
        if c not in only_k:
            props[c] |= P_K_IS_D
    # ... and not the single code points whose targets run on as they do (fullwidth forms, mathematical
    # alphabets, ...): nz_kr_* holds such ranges of 3 and more as (first, count, first target)
    ranges = []
    for c in sorted(c for c, k in only_k.items() if len(k) == 1):
        if ranges and ranges[-1][0] + ranges[-1][1] == c and ranges[-1][2] + ranges[-1][1] == only_k[c][0]:
            ranges[-1][1] += 1
        else:
            ranges.append([c, 1, only_k[c][0]])
    ranges = [r for r in ranges if r[1] >= 3]
    for first, count, _ in ranges:
        for c in range(first, first + count):
            del only_k[c]
    pool = ""
    for key in sorted({tuple(v) for t in (decomp_d, only_k) for v in t.values()}, key=lambda k: (-len(k), k)):
        if "".join(map(chr, key)) not in pool:
            pool += "".join(map(chr, key))

    def entries(table):
        cps = sorted(table)
        assert all(len(table[c]) < 32 for c in cps)
        return cps, [pool.index("".join(map(chr, table[c]))) << 5 | len(table[c]) for c in cps]

    d_cp, d_loc = entries(decomp_d)
    k_cp, k_loc = entries(only_k)
    # the properties as runs of equal words: run r covers [nz_run_start[r], nz_run_start[r + 1]);
    # nz_run_index[c >> RUN_SHIFT] is the run that covers the first code point of c's block
    run_start, run_val, index = [], [], []
    for c in range(0x110000):
        v = props.get(c, 0)
        if not run_val or run_val[-1] != v:
            run_start.append(c)
            run_val.append(v)
        if c % (1 << RUN_SHIFT) == 0 and c <= INDEXED:
            index.append(len(run_val) - 1)
    index.append(len(run_val) - 1)  # (the blocks' ends: index[b + 1]; the last block is all the rest)
    keys = sorted(pairs)
    text = "\n".join([
        "/* Generated by tools/gen_normalize_tables.py from unicodedata (Unicode %s); do not edit." % unicodedata.unidata_version,
        " * nz_run_*: per code point, combining class | has canonical | has compatibility decomposition |",
        " *   second of a composition | stable under NFC, NFD, NFKC, NFKD | compatibility = canonical,",
        " *   as %d runs of equal words with an index per %d code points below U+%X;" % (len(run_val), 1 << RUN_SHIFT, INDEXED),
        " * nz_d_* / nz_k_* / nz_kr_*: the %d full canonical decompositions and, of the %d full compatibility" % (
            len(d_cp), len(decomp_k)),
        " *   ones, the %d that differ from them and lie in none of the %d ranges of singles (Hangul is" % (len(k_cp), len(ranges)),
        " *   algorithmic), each offset << 5 | length into nz_pool;",
        " * nz_comp_*: the %d primary composites, by (first << 21 | second). */" % len(keys),
        "#pragma once",
        "#include <stdint.h>",
        "#ifndef NZ_DATA_ATTR",
        "#define NZ_DATA_ATTR",
        "#endif",
        "#define NZ_RUN_SHIFT %d" % RUN_SHIFT,
        "#define NZ_N_INDEXED %d" % (INDEXED >> RUN_SHIFT),
        "#define NZ_N_RUNS %d" % len(run_val),
        "#define NZ_N_D %d" % len(d_cp),
        "#define NZ_N_K %d" % len(k_cp),
        "#define NZ_N_KR %d" % len(ranges),
        "#define NZ_N_COMP %d" % len(keys),
        "#define NZ_N_POOL %d" % len(pool),
        emit("uint16_t", "nz_run_index", index),
        emit("uint32_t", "nz_run_start", run_start),
        emit("uint16_t", "nz_run_val", run_val),
        emit("uint32_t", "nz_d_cp", d_cp),
        emit("uint32_t", "nz_d_loc", d_loc),
        emit("uint32_t", "nz_k_cp", k_cp),
        emit("uint32_t", "nz_k_loc", k_loc),
        emit("uint32_t", "nz_kr_first", [r[0] for r in ranges]),
        emit("uint16_t", "nz_kr_count", [r[1] for r in ranges]),
        emit("uint32_t", "nz_kr_to", [r[2] for r in ranges]),
        emit("uint32_t", "nz_pool", [ord(ch) for ch in pool]),
        emit("uint64_t", "nz_comp_key", [a << 21 | b for a, b in keys], 16),
        emit("uint32_t", "nz_comp_to", [pairs[k] for k in keys]),
        "",
    ])
    with open(out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
