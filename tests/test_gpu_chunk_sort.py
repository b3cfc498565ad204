"""The merge passes' chunk order (csrc/chunk_sort_hd.h, class_pass in kernels.hip) against the C
oracle, bit-exact, with every value of its switch (CTOK_CHUNK_SORT, read by every call: bits 0..2
the exact-length order of the <= 8 B, 9..16 B and 17..32 B pass, bit 3 the walk direction): the
order in which a chunk's pieces are merged may not show in the output.

Tables and arms: gpt2_50k in both CTOK_SHORT_PACKED arms and all three CTOK_MID_PACKED arms (the
packed tiers, the 17..32 B pass inside k_bpe_short or in k_bpe_mid<2>), and llama3_128k (the
register tiers, the wide sort buffer), all through the same class_pass.

Inputs (tests/chunk_sort_cases.py; their list sizes per chunk are checked on the CPU in
tests/test_chunk_sort_cpu.py): random lowercase words, so nearly every piece is a list entry --
<= 8 B lists above, between and below the sort buffer's capacities (sorted prefix plus the rest in
list order), 9..16 B lists below and above the smallest one, 17..32 B pieces sparse over 300 tiles
and dense, one length only per class, and a text shorter than a tile."""
import json

import numpy as np
import pytest

from complexity_tokenizer import Tokenizer
from datagen import corpus
from oracle import ref_c
from tests import chunk_sort_cases
from tests.packed_cases import env as _env
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

MODES = [None] + [str(m) for m in range(16)]  # (None: the default)

# (table, CTOK_SHORT_PACKED, CTOK_MID_PACKED)
ARMS = [("gpt2", sp, mp) for sp in (None, "0") for mp in ("0", "1", "2")] + [("llama3", None, None)]
ARM_IDS = ["%s-short%s-mid%s" % (n, "_off" if sp else "", mp or "") for n, sp, mp in ARMS]


@pytest.fixture(scope="module")
def cases(gpt2_path, llama3_path):
    """table -> (tokenizer JSON text, {input: (packed text, offsets, oracle ids, oracle offsets)});
    each oracle result computed once and shared by the arms."""
    ins = chunk_sort_cases.inputs()
    packed = {k: corpus.pack([d.encode() for d in docs]) for k, docs in ins.items()}
    cache = {}

    def get(name):
        if name not in cache:
            with open(gpt2_path if name == "gpt2" else llama3_path) as f:
                obj = json.load(f)
            ref = ref_c.RefC(obj)
            cache[name] = (json.dumps(obj), {k: (t, o) + tuple(ref.encode_packed(t, o)) for k, (t, o) in packed.items()})
        return cache[name]

    return get


@pytest.mark.parametrize("name,short_packed,mid_packed", ARMS, ids=ARM_IDS)
def test_every_order_vs_oracle(cases, name, short_packed, mid_packed):
    js, inputs = cases(name)
    with _env("CTOK_SHORT_PACKED", short_packed), _env("CTOK_MID_PACKED", mid_packed):
        tok = Tokenizer.from_str(js)
        for key, (text, off, ref_ids, ref_off) in inputs.items():
            work = None
            for mode in MODES:
                with _env("CTOK_CHUNK_SORT", mode):
                    ids, toff = tok.encode_packed(text, off, timing=True)
                    st = tok.last_stats
                assert_same(ids, toff, ref_ids, ref_off)
                # the same pieces through the same passes, whatever the order
                w = (tuple(st["class_bytes"]), tuple(st["class_ids"]))
                work = work or w
                assert w == work, (key, mode, w, work)
            cls = {"c0": 0, "c1": 1, "c2": 2}.get(key[:2])
            if cls is not None:
                assert work[0][cls] > 0 and work[1][cls] > 0, (key, work)
        # the tiers that ran (known once the device tables are made: the first call)
        p = tok.table_props
        assert p["narrow"] == (name == "gpt2")
        assert p["dev_short_packed"] == (name == "gpt2" and short_packed is None)
        if p["dev_short_packed"]:
            assert p["dev_mid_packed"] == int(mid_packed)


def test_two_calls_same_output(cases):
    """No state of one chunk or call leaks into the next (the bucket counters, the sorted prefix):
    two calls on one tokenizer agree, in the default order and in the one least like it."""
    js, inputs = cases("gpt2")
    tok = Tokenizer.from_str(js)
    for key in ("c0_over", "c1_over", "c2_sparse"):
        text, off, ref_ids, ref_off = inputs[key]
        for mode in (None, "15"):
            with _env("CTOK_CHUNK_SORT", mode):
                a_ids, a_off = tok.encode_packed(text, off)
                b_ids, b_off = tok.encode_packed(text, off)
            assert np.array_equal(a_ids, b_ids) and np.array_equal(a_off, b_off)
            assert_same(b_ids, b_off, ref_ids, ref_off)
