"""The 9..16 B pass of k_bpe_short by either 16-slot tier, against the C oracle: the packed tier
(tokens and pair values as u16 pairs, csrc/merge_packed_hd.h; taken on narrow compact tables whose
values all fit 16 bits, as the gpt2_50k fixture's) and the 16 + 16 register tier
(CTOK_SHORT_PACKED=0, read when the tokenizer's device tables are made; also what a table that
fails the property gets: the shuffled-merges table, whose values are ranks, and the 128k-vocabulary
llama3 fixture).  A few thousand pieces of every length 9..16 B in a few hundred short documents:
words over the fixture's common letters (deep merges), periodic strings (equal pairs repeated, so
the leftmost rule decides), digit runs, consonant strings (they stop merging above 8 tokens) and
one document whose 9..16 B pieces lie across pre-tokenizer tile ends."""
import json

import numpy as np
import pytest

from complexity_tokenizer import Tokenizer
from datagen import corpus
from oracle import ref_c
from tests import packed_cases, toys
from tests.packed_cases import env as _env
from tests.test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu


def _docs(seed):
    return packed_cases.docs(seed, 9, 17, 40)


@pytest.fixture(scope="module")
def batch():
    return corpus.pack([d.encode() for d in _docs(16)])


@pytest.fixture(scope="module")
def tables(gpt2_path, llama3_path):
    """name -> (tokenizer JSON text, oracle ids, oracle offsets); each oracle result computed once."""
    cache = {}

    def get(name, text, off):
        if name not in cache:
            with open(llama3_path if name == "llama3" else gpt2_path) as f:
                obj = json.load(f)
            if name == "shuffled":
                obj = toys.shuffled_merges(obj, seed=16)
            ids, toff = ref_c.RefC(obj).encode_packed(text, off)
            cache[name] = (json.dumps(obj), ids, toff)
        return cache[name]

    return get


@pytest.mark.parametrize("packed", [None, "0"], ids=["default", "packed_off"])
@pytest.mark.parametrize("name", ["gpt2", "shuffled", "llama3"])
def test_short_tiers_vs_oracle(batch, tables, name, packed):
    text, off = batch
    js, ref_ids, ref_off = tables(name, text, off)
    with _env("CTOK_SHORT_PACKED", packed):
        tok = Tokenizer.from_str(js)
        ids, toff = tok.encode_packed(text, off, timing=True)
        st = tok.last_stats
    # the tier that ran (Tokenizer.table_props): packed for the gpt2 table unless switched off
    p = tok.table_props
    assert p["short_packed"] == (name == "gpt2") and p["narrow"] == (name != "llama3")
    assert p["dev_short_packed"] == (name == "gpt2" and packed is None)
    assert_same(ids, toff, ref_ids, ref_off)
    # the 9..16 B class did the work: 320 documents x at least 7 letter pieces of >= 9 bytes
    assert st["class_bytes"][1] > 20000 and st["class_ids"][1] > 0


def test_two_calls_same_output(batch, tables):
    """No state of one piece or call leaks into the next: two calls on one tokenizer agree (and
    with the oracle)."""
    text, off = batch
    js, ref_ids, ref_off = tables("gpt2", text, off)
    with _env("CTOK_SHORT_PACKED", None):
        tok = Tokenizer.from_str(js)
        a_ids, a_off = tok.encode_packed(text, off)
        b_ids, b_off = tok.encode_packed(text, off)
    assert tok.table_props["dev_short_packed"]
    assert np.array_equal(a_ids, b_ids) and np.array_equal(a_off, b_off)
    assert_same(b_ids, b_off, ref_ids, ref_off)
