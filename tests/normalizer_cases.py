"""The batches both Normalizer test files run: tests/test_normalize_cpu.py through the CPU build of
csrc/normalize_hd.h, tests/test_gpu_normalizer.py through the kernels.  CASES maps a name to a function
that returns (normaliser tuple of tests/normalizer_ref.py, list of texts).  The shapes are the
smallest at which a step can still go wrong: a span is 64 input bytes, a wavefront 64 lanes."""
import itertools
import random

from tests import normalizer_ref as ref

SCALARS = [c for c in range(0x110000) if not 0xD800 <= c < 0xE000]
FORMS = ("nfc", "nfd", "nfkc", "nfkd")
MARKS = "\u0315\u0300\u0323"  # classes 232, 230, 220: in the wrong order
WS25 = "".join(chr(c) for c in sorted(ref.WHITE_SPACE))
BERT_DEFAULT = ("bert", True, True, None, True)

MIXED = ["Hello\u4e16\u754c", "  CAF\u00c9  ", "\u0130stanbul", "e\u0301", "\x00a\x1fb\x7f\x85c\u00a0d\u2028e\u3000", "\u0391\u03a3 \u0391\u03a3\u0391", "\ud55c\uae00 \u1112\u1161\u11ab",
         "\ufb01le \ufdfa", "", "a" + MARKS, "\tTab\nNew\rCR\x0b\x0c", "\U00020000x\uf900\u4e00\u3400y", "na\u00efve caf\u00e9",
         "\u0591\u05d0\u0591", "A\u030a\u0323", "x" * 63 + "\u00e9" + "\u0301" * 3, "\u01c5 \u1e9b\u0323", "   ", "\u212b\u2126\u212a"]

CASES = {}


def case(f):
    CASES[f.__name__] = f
    return f


def _shapes(c):
    ch = chr(c)
    return [ch, "x" + ch, ch + "x", ch * 70, ("ab" + ch) * 40]


def _scalars(norm):
    return lambda: (norm, [chr(c) for c in SCALARS])


def _lengths(norm):
    def f():
        cps = [c for c in SCALARS if len(ref.normalize(norm, chr(c)).encode()) != len(chr(c).encode())]
        return norm, [t for c in cps for t in _shapes(c)]
    return f


for _n in [(k,) for k in FORMS] + [("strip_accents",), BERT_DEFAULT]:
    CASES["scalars_" + _n[0]] = _scalars(_n)
for _n in [(k,) for k in FORMS] + [("strip_accents",)]:
    CASES["lengths_" + _n[0]] = _lengths(_n)


@case
def fdfa_nfkd():
    return ("nfkd",), ["\ufdfa" * 200, "x" + "\ufdfa" * 200]


@case
def fdfa_nfkc():
    return ("nfkc",), ["\ufdfa" * 200, "x" + "\ufdfa" * 200]


def _syllables():
    return [chr(c) for c in range(0xAC00, 0xAC00 + 11172, 97)]


@case
def hangul_nfd():
    s = _syllables()
    return ("nfd",), s + ["".join(s), "x".join(s)]


@case
def hangul_nfc():
    s = [ref.normalize(("nfd",), x) for x in _syllables()]
    jamo = "".join(chr(0x1100 + i % 19) + chr(0x1161 + i % 21) + chr(0x11A8 + i % 27) for i in range(400))
    return ("nfc",), s + ["".join(s), jamo, "\u1100" + "\u1161" * 300, "\u1161\u11a8" * 100, "\u1100\u1161" * 100 + "\u11a8" * 70,
                          "\uac00\u11a7\uac00\u11a8\uac01\u11a8"]


def _marks_at_offsets():
    # marks in the wrong order at byte offsets 55..70: across a span boundary and a 64-byte window
    return ["x" * k + "a" + MARKS + "b" for k in range(55, 71)] + ["\u00e9" * k + "a" + MARKS * 3 for k in range(27, 35)]


for _k in FORMS:
    CASES["marks_across_spans_" + _k] = (lambda k: lambda: ((k,), _marks_at_offsets()))(_k)


@case
def long_run_nfd():
    return ("nfd",), ["a" + MARKS * 20000]


@case
def long_run_nfkc():
    return ("nfkc",), ["a" + MARKS * 20000]


def _boundaries():
    return [["e", "\u0301", "", "", "e\u0301", "", "a", MARKS, "\u1100", "\u1161", "\u11a8"], ["", "", ""], [], [""],
            ["", "\u00e9", ""]]


for _i in range(len(_boundaries())):
    for _k in ("nfc", "nfkd", "lowercase", "strip", "strip_accents"):
        CASES["boundaries_%d_%s" % (_i, _k)] = (lambda i, k: lambda: ((k,), _boundaries()[i]))(_i, _k)
    CASES["boundaries_%d_bert" % _i] = (lambda i: lambda: (BERT_DEFAULT, _boundaries()[i]))(_i)
    CASES["boundaries_%d_affix" % _i] = (lambda i: lambda: (
        ("sequence", [("prepend", "\u2581"), ("append", "</s>"), ("replace", "", "-"), ("replace", "-", "")]), _boundaries()[i]))(_i)
    CASES["boundaries_%d_insert" % _i] = (lambda i: lambda: (("replace", "", "\u00b7"), _boundaries()[i]))(_i)


@case
def strip_sets():
    edge = WS25 + "\x1c\x1d\x1e\x1f\u200b"
    texts = [edge + "a b" + edge, WS25 + "a" + WS25, WS25, " ", "", "\x1c a \x1c", "\u200b x \u200b", " " * 100, "x" * 70 + " " * 70,
             " " * 70 + "x" * 70, "\u3000" * 30 + "\u00e9" + "\u2003" * 30]
    texts += [chr(c) + "x" + chr(c) for c in sorted(ref.WHITE_SPACE) + [0x1C, 0x1D, 0x1E, 0x1F, 0x200B]]
    return ("strip",), texts


def _runs(ch):
    return [ch * n for n in list(range(10)) + [63, 64, 65, 10001]]


@case
def replace_self_overlap():
    return ("replace", "aa", "b"), _runs("a") + ["aaaaa", "xaaax" * 30]


@case
def replace_self_overlap_long():
    return ("replace", "abab", "<>"), _runs("ab") + ["ababa" * 50, "abab"]


@case
def replace_across_spans():
    return ("replace", "needle", "N"), ["x" * k + "needle" + "y" * 9 for k in range(56, 67)] + ["needl", "needle", "eedle"]


@case
def replace_longer_than_text():
    return ("replace", "x" * 100, "y"), ["x" * 99, "", "x", "x" * 100, "x" * 201]


@case
def replace_multibyte():
    return ("replace", "\u00e9\u4e16", "\U0001f600\u00df"), ["\u00e9\u4e16", "a\u00e9\u4e16b" * 20, "\u00e9", "\u4e16\u00e9", "\u00e9\u4e16" * 70, "\u00e9\u4e16\u4e16"]


@case
def replace_empty_pattern():
    return ("replace", "", "-"), ["abc", "", "\u00e9\u4e16\U0001f600", "x" * 130]


@case
def replace_empty_replacement():
    return ("replace", "ab", ""), ["ab", "abab", "aabb", "xaby" * 40, "", "a", "b"]


@case
def replace_not_into_next_text():
    # "ab" + "c" would match across the boundary; "abc" inside one text does
    return ("replace", "abc", "!"), ["ab", "c", "a", "bc", "", "abc", "ab", "", "c", "xabc"]


def _bert_options():
    return list(itertools.product((True, False), (True, False), (None, True, False), (True, False)))


for _i, _o in enumerate(_bert_options()):
    CASES["bert_%02d" % _i] = (lambda o: lambda: (("bert",) + o, MIXED))(_o)


@case
def precompiled_chain():
    # the second entry matches what the first one wrote, the third what the second one wrote
    return ("precompiled", [("\ufb01", "fi"), ("fi", "F"), ("Fl", "#"), ("", ""), ("zz", "z")]), ["\ufb01le", "fifi\ufb01", "zzzz", "", "Fle"]


ALL_KINDS = ("sequence", [("nfd",), ("nfkd",), ("nfc",), ("nfkc",), ("lowercase",), ("strip",), ("strip_accents",),
                          ("replace", "e", "E"), ("prepend", "<"), ("append", ">"), BERT_DEFAULT,
                          ("precompiled", [("<", "["), (">", "]")]), ("sequence", [("strip",), ("replace", "", ".")])])


@case
def sequence_of_all_kinds():
    return ALL_KINDS, MIXED


@case
def bert_sequence_of_the_reference():
    return ("sequence", [("nfc",), ("lowercase",), ("strip_accents",), ("strip",)]), MIXED


POOLS = {
    "ascii": list(range(0x20, 0x7F)),
    "marks": [0x61, 0x65, 0x41, 0x300, 0x301, 0x315, 0x323, 0x327, 0x328, 0x338, 0x345, 0x591, 0x5B0, 0xF71, 0xF72, 0xF74, 0x1DC0, 0x20D0, 0xFE20,
              0x1AB0, 0x3099, 0x93C, 0x94D],
    "composing": [0x1100, 0x1161, 0x11A8, 0x11A7, 0xAC00, 0xAC01, 0x1112, 0x1175, 0x11C2, 0x9C7, 0x9BE, 0x9D7, 0xB47, 0xB56, 0xB3E, 0x1025,
                  0x102E, 0x3B1, 0x3A9, 0x301, 0x342, 0x345, 0x308, 0x1F00, 0x1F80, 0x212B, 0x2126, 0x41, 0x30A, 0x323],
    "compat": [0xFDFA, 0xFB01, 0x2460, 0x33A7, 0x3300, 0xFF21, 0x1D400, 0x2F800, 0xF900, 0xA0, 0xAA, 0xBC, 0x2026, 0x2003, 0x3000, 0x1E9B,
               0x323, 0x307, 0x1C4, 0x1C5, 0x132, 0x149, 0x17F],
    "bert": [0x0, 0x9, 0xA, 0xD, 0x1F, 0x20, 0x7F, 0x85, 0x9F, 0xA0, 0x2028, 0x3000, 0x4E00, 0x9FFF, 0x3400, 0x20000, 0xF900, 0x2FA1F, 0x41,
             0xC9, 0x130, 0x3A3, 0x301, 0x1C, 0x200B],
    "any": SCALARS,
}


def random_texts(pool, seed, n=3000):
    rng = random.Random(seed)
    cps = POOLS[pool]
    return ["".join(chr(rng.choice(cps)) for _ in range(rng.randrange(0, 40))) for _ in range(n)]
