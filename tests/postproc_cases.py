"""The processors and batches that the PostProcessor's CPU check (tests/test_postproc_cpu.py) and its
GPU tests (tests/test_gpu_postproc.py) share.  A processor is a tuple of tests/postproc_ref.py."""
import random

SPECIALS = [("[CLS]", 101), ("[SEP]", 102), ("<s>", 0), ("</s>", 0xFFFFFFFF), ("<pad>", 7), ("s", 9), ("[CLS]", 55)]

BERT = ("bert", ("[CLS]", 101), ("[SEP]", 102))
ROBERTA = ("roberta", ("<s>", 0), ("</s>", 2), False)
BERT_TEMPLATE = ("template", "[CLS]:0 $A:0 [SEP]:0", "[CLS]:0 $A:0 [SEP]:0 $B:1 [SEP]:1", SPECIALS)
DEFAULT = ("template", "<s> $A </s>", "<s> $A </s> $B </s>", [("<s>", 2), ("</s>", 0)])

# (processor, ids, pair, expected), every expected output written out by hand from postprocessors.rs:34-195
QUIRKS = [
    # the template walk
    (("template", "$A", None, []), [1, 2], None, [1, 2]),
    (("template", "$A $B", None, []), [1, 2], [3], [1, 2, 3]),  # pair=None: the single template, which has a $B
    (("template", "$A", None, []), [1, 2], [3], [1, 2]),  # the single template drops the pair
    (("template", "$A $B", "$B $A", []), [1], None, [1]),  # a $B without a pair adds nothing
    (("template", "$A $B", "$B $A", []), [1], [2], [2, 1]),
    (("template", "$C$A$", None, []), [1], None, [1]),  # $ before another char, and as the last char: only the $ is skipped
    (("template", "$$A", None, []), [1], None, [1]),  # the first $ is skipped, the second begins $A
    (("template", "$", None, []), [1], None, []),
    (("template", "", None, []), [1], [2], []),
    (("template", "[CLS]:0 $A:0 [SEP]:0 $B:1 [SEP]:1", None, SPECIALS), [5], [6], [101, 5, 102, 6, 102]),  # other chars are skipped
    (("template", "<$A>", None, [("<$A>", 4)]), [1], None, [4]),  # a token, copies nothing
    (("template", "<$A>", None, []), [1], None, []),
    (("template", "<s> $A <unk>", None, SPECIALS), [1], None, [0, 1]),  # an unknown token adds nothing
    (("template", "[CLS] $A", None, SPECIALS), [1], None, [101, 1]),  # the first equal string wins (101, not 55)
    (("template", "s $A s", None, SPECIALS), [1], None, [1]),  # a special token that begins with neither < nor [ never matches
    (("template", "$A <pad", None, [("<pad", 3)]), [1], None, [1, 3]),  # no closing char: to the end of the template
    (("template", "$A <pad \t 　", None, [("<pad", 3)]), [1], None, [1, 3]),  # ... and then trimmed (Unicode trim)
    (("template", "$A <pad \x1f", None, [("<pad", 3)]), [1], None, [1]),  # U+001F is not White_Space
    (("template", "$A < s>", None, [("< s>", 3), ("<s>", 0)]), [1], None, [1, 3]),  # a closed token keeps its inner spaces
    (("template", "<a]> $A [b>] $A", None, [("<a]>", 1), ("[b>]", 2)]), [9], None, [1, 9, 2, 9]),  # each opener has its own closer
    (("template", "é$Aé<é>", None, [("<é>", 8)]), [1], None, [1, 8]),  # char by char, not byte by byte
    (("template", "$A $A", None, []), [1, 2], None, [1, 2, 1, 2]),
    (("template", "$B $B", "$B <s> $B", SPECIALS), [1], [2, 3], [2, 3, 0, 2, 3]),
    # ids are the whole u32 range
    (("template", "</s> $A <s>", None, SPECIALS), [0, 0xFFFFFFFF, 0xFFFFFFFE], None, [0xFFFFFFFF, 0, 0xFFFFFFFF, 0xFFFFFFFE, 0]),
    # the fixed processors
    (BERT, [1, 2, 3], None, [101, 1, 2, 3, 102]),
    (BERT, [1], [2], [101, 1, 102, 2, 102]),
    (BERT, [1], [], [101, 1, 102, 102]),  # a pair that is present but empty is not an absent one
    (BERT, [], None, [101, 102]),
    (ROBERTA, [1, 2, 3], None, [0, 1, 2, 3, 2]),
    (ROBERTA, [1], [5], [0, 1, 2, 2, 5, 2]),
    (ROBERTA, [], [], [0, 2, 2, 2]),
    (DEFAULT, [5], [], [2, 5, 0, 0]),  # the pair template is chosen
    (DEFAULT, [5], None, [2, 5, 0]),
    # Sequence: the pair goes to the first processor only
    (("sequence", []), [1, 2], [3], [1, 2]),  # the empty Sequence returns ids and drops the pair
    (("sequence", [BERT, ROBERTA]), [1], [2], [0, 101, 1, 102, 2, 102, 2]),
    (("sequence", [ROBERTA, BERT]), [1], None, [101, 0, 1, 2, 102]),
    (("sequence", [("template", "$A", None, []), BERT]), [1], [2], [101, 1, 102]),  # the first dropped the pair, Bert sees none
    (("sequence", [("sequence", [BERT]), ("sequence", [("sequence", [DEFAULT])])]), [1], [2], [2, 101, 1, 102, 2, 102, 0]),  # nested ones flatten
    (("sequence", [BERT, ("template", "$A $B <s> $A", "$B", SPECIALS)]), [1], [2], [101, 1, 102, 2, 102, 0, 101, 1, 102, 2, 102]),
]

# every processor the batches run under
EVERY = []
for _p in [BERT, ROBERTA, BERT_TEMPLATE, DEFAULT] + [q[0] for q in QUIRKS]:
    if _p not in EVERY:
        EVERY.append(_p)

QUIRK_ROWS = [([], None), ([], []), ([1], None), ([1], []), ([], [2]), ([0, 0xFFFFFFFF], [0xFFFFFFFF, 0, 5]), ([1, 2, 3], None),
              ([4, 5, 6, 7], [8]), (list(range(70)), list(range(100, 130)))]


def flat_list(n_items):
    """a processor whose flat lists have n_items items each, made of all three kinds: steps of "$A $A"
    double a list, a last step adds the rest"""
    assert n_items >= 1
    sp = [("<s>", 11), ("[x]", 0xFFFFFFFF)]
    if n_items == 1:
        return ("template", "$A", None, sp)
    if n_items == 2:
        return ("template", "<s> $A", "[x] $B", sp)
    steps = [("template", "<s> $A", "$B $A", sp)]  # 2 items
    n = 2
    while n * 2 <= n_items:
        steps.append(("template", "$A $A", None, sp))
        n *= 2
    rest = n_items - n
    if rest:
        steps.append(("template", "$A" + " [x]" * rest, None, sp))
    return ("sequence", steps)


def random_rows(seed, n_rows, max_len=9):
    """rows with mixed None / [] / non-empty pairs, and ids 0 and 0xFFFFFFFF among them"""
    rng = random.Random(seed)
    pool = [0, 0xFFFFFFFF, 1, 2, 101, 102, 0x7FFFFFFF, 0x80000000, 12345]
    batch, pairs = [], []
    for _ in range(n_rows):
        batch.append([rng.choice(pool) for _ in range(rng.randrange(0, max_len))])
        k = rng.randrange(3)
        pairs.append(None if k == 0 else [] if k == 1 else [rng.choice(pool) for _ in range(rng.randrange(1, max_len))])
    return batch, pairs
