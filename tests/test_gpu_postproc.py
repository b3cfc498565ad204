"""GPU parity of complexity_tokenizer.PostProcessor (csrc/postproc.hip) against the restatement of the
reference's src/postprocessors.rs (tests/postproc_ref.py).  Exact equality of ids and masks everywhere;
the processors and batches are those of tests/postproc_cases.py, which tests/test_postproc_cpu.py runs
through the CPU build of the same rules first.  A workgroup's tile is 256 cells (csrc/postproc_internal.h
kThreads), a wave 64 lanes, and the scan of the rows' lengths takes another path from 4,097 rows on."""
import numpy as np
import pytest

from complexity_tokenizer import Decoder, PostProcessor, WordPieceModel
from tests import postproc_cases as pc
from tests import postproc_ref as ref

pytestmark = pytest.mark.gpu

TILE = 256
WAVE = 64
NAMES = ("input_ids", "attention_mask", "token_type_ids", "special_tokens_mask")


def want_rows(p, batch, pairs=None):
    return [ref.process(p, ids, None if pairs is None else pairs[i]) for i, ids in enumerate(batch)]


def pack(rows):
    off = np.cumsum([0] + [len(r or []) for r in rows]).astype(np.uint64)
    return np.array([i for r in rows for i in (r or [])], dtype=np.uint32), off


def unpack(ids, off):
    flat, o = ids.tolist(), off.tolist()
    return [flat[o[i]:o[i + 1]] for i in range(len(o) - 1)]


def padded_lists(got):
    out = {k: got[k].tolist() for k in NAMES}
    out["row_len"] = got["row_len"].tolist()
    out["width"] = got["input_ids"].shape[1]
    return out


def on_device(d, batch, pairs=None, slack=0, **kw):
    """process_packed_device over torch tensors; (rows, the tensors of the output)"""
    import torch
    dev = torch.device("cuda", 0)

    def to_dev(a, as_type):
        return torch.from_numpy(a.view(as_type).copy()).to(dev)

    ids, off = pack(batch)
    t = {"ids": to_dev(ids, np.int32), "off": to_dev(off, np.int64)}
    args = {}
    if pairs is not None:
        pids, poff = pack(pairs)
        t["pids"], t["poff"] = to_dev(pids, np.int32), to_dev(poff, np.int64)
        t["has"] = torch.from_numpy(np.array([p is not None for p in pairs], dtype=np.uint8)).to(dev)
        args = dict(pair_ids_ptr=t["pids"].data_ptr(), pair_off_ptr=t["poff"].data_ptr(), has_pair_ptr=t["has"].data_ptr(),
                    n_pair_ids=int(pids.size))
    total = sum(len(r) for r in kw.pop("want"))
    out = torch.full((total + slack + 1,), -2, dtype=torch.int32, device=dev)
    out_off = torch.full((len(batch) + 2,), -7, dtype=torch.int64, device=dev)
    n = d.process_packed_device(t["ids"].data_ptr(), t["off"].data_ptr(), len(batch), int(ids.size), out.data_ptr(), total + slack,
                                out_off.data_ptr(), **args, **kw)
    torch.cuda.synchronize()
    o, oo = out.cpu().numpy(), out_off.cpu().numpy()
    assert n == total and bool((o[n:] == -2).all()) and oo[-1] == -7  # nothing past out[n) and out_off[n_rows]
    return unpack(o[:n].view(np.uint32), oo[:-1].view(np.uint64))


def check(p, batch, pairs=None, made=None, device_too=False):
    d = made or ref.to_postprocessor(p)
    want = want_rows(p, batch, pairs)
    got = d.process_batch(batch, pairs)
    bad = [i for i in range(len(batch)) if got[i] != want[i]]
    assert len(got) == len(batch) and not bad, (p, len(bad), batch[bad[0]][:20], got[bad[0]][:40], want[bad[0]][:40])
    if device_too:
        assert on_device(d, batch, pairs, want=want) == want, p
    return d


def check_padded(p, batch, pairs=None, made=None, **kw):
    d = made or ref.to_postprocessor(p)
    got = padded_lists(d.process_padded(batch, pairs, **kw))
    want = ref.process_padded(p, batch, pairs, **kw)
    for k in want:
        assert got[k] == want[k], (p, kw, k)
    return d


def test_quirk_table():
    for p, ids, pair, want in pc.QUIRKS:
        d = ref.to_postprocessor(p)
        assert d.process(ids, pair) == want == d.process_batch([ids], [pair])[0], (p, ids, pair)
        assert d.process(np.array(ids, dtype=np.uint32), pair) == want


@pytest.mark.parametrize("i", range(len(pc.EVERY)))
def test_every_entry_under_every_processor(i):
    p = pc.EVERY[i]
    batch, pairs = [r[0] for r in pc.QUIRK_ROWS], [r[1] for r in pc.QUIRK_ROWS]
    d = check(p, batch, pairs, device_too=True)
    want = want_rows(p, batch, pairs)
    for ids, pr, w in zip(batch, pairs, want):  # process is the batch of one
        assert d.process(ids, pr) == w
    has = np.array([pr is not None for pr in pairs], dtype=np.uint8)
    assert unpack(*d.process_packed(*pack(batch), *pack(pairs), has)) == want
    assert unpack(*d.process_packed(*pack(batch))) == want_rows(p, batch) == d.process_batch(batch)
    full = [pr or [] for pr in pairs]
    assert unpack(*d.process_packed(*pack(batch), *pack(full))) == want_rows(p, batch, full)  # has_pair=None: every row has a pair
    for pad_left in (False, True):
        check_padded(p, batch, pairs, d, pad_left=pad_left, pad_id=0xFFFFFFFF)
        check_padded(p, batch, pairs, d, pad_left=pad_left, truncate_to=5, strategy="longest_first", pad_to=3)
    got = d.process_padded(pack(batch), pack(pairs) + (has,), pad_to="longest")  # the packed form of the same
    assert padded_lists(got) == padded_lists(d.process_padded(batch, pairs, pad_to="longest"))


@pytest.mark.parametrize("seed", range(3))
def test_seeded_random_batches(seed):
    batch, pairs = pc.random_rows(seed, 700, 40)
    for p in pc.EVERY[seed::3]:
        d = check(p, batch, pairs, device_too=(seed == 0))
        check_padded(p, batch, pairs, d, pad_left=bool(seed & 1), pad_id=9)


@pytest.mark.parametrize("strategy", ["only_first", "only_second", "longest_first"])
def test_truncation_against_the_pop_loop(strategy):
    batch, pairs = [], []
    for na in range(13):
        for nb in [None] + list(range(13)):
            batch.append(list(range(1, na + 1)))
            pairs.append(None if nb is None else list(range(100, 100 + nb)))
    p = ("template", "$A <s> $B", "$B <s> $A", [("<s>", 0)])
    d = ref.to_postprocessor(p)
    for to in range(26):
        check_padded(p, batch, pairs, d, truncate_to=to, strategy=strategy)
    want = []
    for ids, pr in zip(batch, pairs):
        ids, pr = list(ids), (None if pr is None else list(pr))
        ref.truncate(ids, pr, 7, strategy)
        want.append(ref.process(p, ids, pr))
    assert on_device(d, batch, pairs, want=want, truncate_to=7, strategy=strategy) == want


@pytest.mark.parametrize("n_rows", [0, 1, 255, 256, 257])
def test_rows_around_a_workgroup(n_rows):
    batch, pairs = pc.random_rows(n_rows, n_rows, 6)
    for p in (pc.BERT, pc.DEFAULT, ("sequence", [])):
        d = check(p, batch, pairs, device_too=True)
        check(p, batch, None, d, device_too=True)
        check(p, [[]] * n_rows, None, d)
        check(p, [[5]] * n_rows, None, d)
        check_padded(p, batch, pairs, d, pad_to="longest")
        check_padded(p, batch, pairs, d, pad_to=40, pad_left=True)
    assert d.process_padded([[]] * n_rows)["input_ids"].shape == (n_rows, 0)
    assert d.process_padded([[]] * n_rows, pad_to=3)["input_ids"].tolist() == [[0, 0, 0]] * n_rows


def test_empty_rows_at_the_start_the_middle_and_the_end():
    p = ("template", "$A $B", None, [])  # rows of no cells at all
    batch = [[], [], [1, 2, 3], [], [], [], [4] * 300, [], [5], [], []]
    pairs = [None, [], None, [], None, None, [6] * 300, None, None, [], None]
    for q in (p, pc.BERT):
        d = check(q, batch, pairs, device_too=True)
        for pad_left in (False, True):
            check_padded(q, batch, pairs, d, pad_left=pad_left, pad_id=8)


@pytest.mark.parametrize("at", [WAVE, TILE, 3 * TILE])
def test_rows_that_straddle_a_boundary(at):
    """A row whose output lies on both sides of cell `at` of the ragged output (a 64-lane boundary, a
    256-cell workgroup boundary), with rows before and after it, empty ones among them."""
    p = pc.BERT_TEMPLATE  # a row without a pair has 2 + na cells, one with a pair 3 + na + nb
    for before, na, nb in ((at - 1, 0, None), (at - 2, 1, []), (at - 30, 40, [1] * 40), (at - 3, 1, [7]), (at - 1, 300, [2] * 300)):
        # `before` cells in front: rows of 3 cells, one that makes up the rest, and an empty row (2 cells) last
        k, rem = (before - 2) // 3, (before - 2) % 3
        lead = [[9]] * (k - 1) + [[9] * (rem + 1)] + [[]]
        batch = lead + [list(range(50, 50 + na))] + [[3], []]
        pairs = [None] * len(lead) + [nb] + [None, []]
        want = want_rows(p, batch, pairs)
        off = np.cumsum([0] + [len(r) for r in want])
        i = len(lead)
        assert off[i] == before < at < off[i + 1], (before, off[i], off[i + 1])  # the row's cells lie on both sides
        d = check(p, batch, pairs, device_too=True)
        check_padded(p, batch, pairs, d)
    # the matrix form: a row of the flat [rows, width] cells across `at`, for widths that do not divide it
    for width in (at // 2 + 1, at - 1, at + 1):
        batch = [[1] * (width - 2), [2], [], [3] * (width - 2)]
        assert any(r * width < at < (r + 1) * width for r in range(len(batch)))
        for pad_left in (False, True):
            d = check_padded(pc.BERT, batch, None, pad_to=width, pad_left=pad_left, pad_id=6)
            assert d.last_stats["width"] == width


def test_one_long_row_copied_twice():
    p = ("template", "$A $A", None, [])
    ids = list(range(1000))
    d = check(p, [ids], None, device_too=True)
    assert d.process(ids) == ids + ids
    check(p, [ids, [], ids[:3]], [None, [1], None], d, device_too=True)
    check_padded(p, [ids, [7]], None, d, pad_left=True)


@pytest.mark.parametrize("width", [63, 64, 65, 255, 256, 257])
def test_widths_around_a_wave_and_a_workgroup(width):
    batch = [[1] * (width - 2), [], [2] * 5, [3] * (width - 3), [4]]
    pairs = [None, [], [6] * 3, None, None]
    for pad_left in (False, True):
        d = check_padded(pc.BERT, batch, pairs, pad_to="longest", pad_left=pad_left, pad_id=0xFFFFFFFF)
        assert d.last_stats["width"] == width
        check_padded(pc.BERT, [[1], [2, 3]], [None, [4]], d, pad_to=width, pad_left=pad_left)
        assert d.last_stats["width"] == width


@pytest.mark.parametrize("n", [1, 2, 64, 65, 4096])
def test_flat_lists(n):
    p = pc.flat_list(n)
    batch = [[], [7], [1, 2, 3], [0xFFFFFFFF], []]
    pairs = [None, [], [4, 5], None, [6]]
    d = check(p, batch, pairs, device_too=True)
    assert (d.last_stats["items_single"], d.last_stats["items_pair"]) == (n, n)
    check_padded(p, batch, pairs, d, pad_left=True, pad_id=5)


def test_a_flat_list_of_4097_items_is_refused():
    for p in (pc.flat_list(4097), ("sequence", [("template", "$A $A", None, [])] * 13)):
        with pytest.raises(RuntimeError, match="4096"):  # CTOK_E_CAPACITY, at create
            ref.to_postprocessor(p)
    with pytest.raises(RuntimeError, match="4097 items"):
        PostProcessor.template("$A " * 4097)
    assert PostProcessor.sequence([PostProcessor.template("$A $A")] * 10).process([5]) == [5] * 1024


def test_a_scan_of_more_than_one_block():
    n_rows = 4096 + 5  # scan_u64 takes 4,096 entries a block
    batch, pairs = pc.random_rows(3, n_rows, 5)
    d = check(pc.ROBERTA, batch, pairs, device_too=True)
    check_padded(pc.ROBERTA, batch, pairs, d, pad_left=True)


def test_a_workgroup_that_takes_a_run_of_tiles():
    """From 2,048 tiles on (524,288 ids) a workgroup of the ragged write takes more than one tile, and
    the last workgroups may have none."""
    import random
    rng = random.Random(8)
    batch = [[rng.randrange(1 << 32)] * rng.choice((0, 0, 1, 90, 255, 256, 700)) for _ in range(5300)]
    pairs = [None if i % 3 == 0 else [i] * (i % 5) for i in range(len(batch))]
    want = want_rows(pc.ROBERTA, batch, pairs)
    assert sum(len(r) for r in want) > 3 * 2048 * TILE // 2  # two tiles a workgroup, and workgroups without one
    d = ref.to_postprocessor(pc.ROBERTA)
    has = np.array([pr is not None for pr in pairs], dtype=np.uint8)
    assert unpack(*d.process_packed(*pack(batch), *pack(pairs), has)) == want
    assert on_device(d, batch, pairs, want=want) == want


def test_pair_present_but_empty_against_pair_absent():
    with_pair = ("template", "<s> $A", "<s> $A </s> $B </s>", [("<s>", 1), ("</s>", 2)])
    batch = [[5], [5], [5, 6], [], []]
    pairs = [None, [], [7], [], None]
    d = check(pc.BERT, batch, pairs, device_too=True)
    assert d.process_batch(batch, pairs) == [[101, 5, 102], [101, 5, 102, 102], [101, 5, 6, 102, 7, 102], [101, 102, 102], [101, 102]]
    d = check(with_pair, batch, pairs, device_too=True)
    assert d.process_batch(batch, pairs) == [[1, 5], [1, 5, 2, 2], [1, 5, 6, 2, 7, 2], [1, 2, 2], [1]]
    got = d.process_padded(batch, pairs)
    assert got["token_type_ids"].tolist()[2] == [0, 0, 0, 0, 1, 0] and got["row_len"].tolist() == [2, 4, 6, 3, 1]


def test_capacity_is_refused_without_the_allocation():
    """One row of 2^20 ids under 4096 $A items is exactly 2^32 ids: refused after the count, nothing
    written, and the handle goes on."""
    import torch
    d = PostProcessor.sequence([PostProcessor.template("$A $A")] * 12)
    n = 1 << 20
    dev = torch.device("cuda", 0)
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    off = torch.tensor([0, n], dtype=torch.int64, device=dev)
    out = torch.full((1024,), -2, dtype=torch.int32, device=dev)
    out_off = torch.full((2,), -7, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="2\\^32"):
        d.process_packed_device(ids.data_ptr(), off.data_ptr(), 1, n, out.data_ptr(), 1024, out_off.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == -2).all()) and bool((out_off == -7).all())
    with pytest.raises(ValueError):
        d.fetch_packed()
    with pytest.raises(RuntimeError, match="2\\^32"):
        d.process_packed(np.zeros(n, dtype=np.uint32), np.array([0, n], dtype=np.uint64))
    with pytest.raises(RuntimeError, match="2\\^32"):  # 2^16 rows of 2^16 cells
        PostProcessor.sequence([]).process_padded([[]] * (1 << 16), pad_to=1 << 16)
    assert d.process([3]) == [3] * 4096


def test_exact_capacity_on_the_device_entry():
    import torch
    p = pc.BERT_TEMPLATE
    d = ref.to_postprocessor(p)
    batch, pairs = pc.random_rows(5, 300, 30)
    want = want_rows(p, batch, pairs)
    total = sum(len(r) for r in want)
    assert on_device(d, batch, pairs, want=want) == want  # the capacity is exactly the ids; the guards are checked there
    dev = torch.device("cuda", 0)
    ids, off = pack(batch)
    pids, poff = pack(pairs)
    t_ids, t_off = torch.from_numpy(ids.view(np.int32).copy()).to(dev), torch.from_numpy(off.view(np.int64).copy()).to(dev)
    t_pids, t_poff = torch.from_numpy(pids.view(np.int32).copy()).to(dev), torch.from_numpy(poff.view(np.int64).copy()).to(dev)
    t_has = torch.from_numpy(np.array([pr is not None for pr in pairs], dtype=np.uint8)).to(dev)
    out = torch.full((total + 8,), -2, dtype=torch.int32, device=dev)
    out_off = torch.full((len(batch) + 1,), -7, dtype=torch.int64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    stream.synchronize()
    torch.cuda.synchronize()
    for cap in (0, total - 1):  # one id short: the needed size comes back and nothing is written
        with pytest.raises(BufferError) as e:
            d.process_packed_device(t_ids.data_ptr(), t_off.data_ptr(), len(batch), int(ids.size), out.data_ptr(), cap, out_off.data_ptr(),
                                    t_pids.data_ptr(), t_poff.data_ptr(), t_has.data_ptr(), int(pids.size), stream=stream.cuda_stream)
        assert e.value.needed_ids == total
        torch.cuda.synchronize()
        assert bool((out == -2).all()) and bool((out_off == -7).all())
        assert unpack(*d.fetch_packed()) == want  # the whole result, without a second run
    # ids 4-byte and offsets 8-byte aligned, refused at the entry
    for bad in (dict(ids=1), dict(out=2), dict(off=4), dict(out_off=4)):
        with pytest.raises(ValueError, match="aligned"):
            d.process_packed_device(t_ids.data_ptr() + bad.get("ids", 0), t_off.data_ptr() + bad.get("off", 0), len(batch), int(ids.size),
                                    out.data_ptr() + bad.get("out", 0), total, out_off.data_ptr() + bad.get("out_off", 0))
    bad_off = torch.tensor([0, 5, 3, int(ids.size)], dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="order"):  # CTOK_E_ARG: the offsets decrease
        d.process_packed_device(t_ids.data_ptr(), bad_off.data_ptr(), 3, int(ids.size), out.data_ptr(), total, out_off.data_ptr())
    with pytest.raises(ValueError, match="order"):  # they do not end at n_ids
        d.process_packed_device(t_ids.data_ptr(), t_off.data_ptr(), len(batch), int(ids.size) + 1, out.data_ptr(), total, out_off.data_ptr())
    torch.cuda.synchronize()
    assert bool((out == -2).all()) and bool((out_off == -7).all())


def test_an_output_larger_than_the_first_guess_is_fetched():
    p = ("sequence", [("template", "$A $A", None, [])] * 8)
    d = check(p, [list(range(100)), [], [1]], None)
    assert d.last_stats["ids_out"] == 256 * 101 > d.last_stats["ids_in"] + 8 * 3 + 64
    check_padded(p, [list(range(100)), [], [1]], None, d)
    assert d.process([2]) == [2] * 256  # (and the handle goes on)
    assert [s[0] for s in d.last_stats["stages"]] == ["count", "scan", "write"]


def test_the_chain_from_a_model_and_back():
    vocab = {"[UNK]": 0, "[CLS]": 1, "[SEP]": 2, "un": 3, "##able": 4, "##a": 5, "b": 6, "hello": 7, "##s": 8, "é": 9}
    m = WordPieceModel(vocab)
    texts = ["unable hello", "", "hellos b é", "zzz unables", "b"]
    ids, off = m.encode_batch_flat(texts)
    d = PostProcessor.bert("[CLS]", 1, "[SEP]", 2)
    out, out_off = d.process_packed(ids, off)
    rows = unpack(out, out_off)
    assert rows == [[1] + r + [2] for r in m.encode_batch(texts)]
    dec = Decoder.wordpiece("##", cleanup=False)
    dec.set_vocab({i: t for t, i in vocab.items() if i > 2})  # the special tokens have no entry: skipped
    text, text_off = dec.decode_ids_packed(out, out_off)
    raw, o = text.tobytes(), text_off.tolist()
    got = [raw[o[i]:o[i + 1]].decode() for i in range(len(texts))]
    assert got == [m.decode([i for i in r if i > 2]) for r in rows]
    assert got[0] == "unable hello" and got[2] == "hellos b é"
    # a pair of encodings: the second half of the batch as the pairs of the first
    a, b = m.encode_batch(texts[:2]), m.encode_batch(texts[2:4])
    got = d.process_padded(a, b, truncate_to=4, strategy="only_second", pad_to="longest")
    assert got["input_ids"].tolist() == ref.process_padded(pc.BERT[:1] + (("[CLS]", 1), ("[SEP]", 2)), a, b, truncate_to=4,
                                                           strategy="only_second")["input_ids"]


def test_names_defaults_and_arguments():
    d = PostProcessor.default()
    assert d.process([5]) == ref.process(ref.DEFAULT, [5]) == [2, 5, 0]
    assert d.process([5], [6]) == [2, 5, 0, 6, 0] and (d.added_tokens_single(), d.added_tokens_pair()) == (2, 2)
    r = PostProcessor.roberta("<s>", 0, "</s>", 2)
    assert r.add_prefix_space is False and PostProcessor.roberta("<s>", 0, "</s>", 2, True).process([1]) == r.process([1]) == [0, 1, 2]
    assert (r.added_tokens_single(), r.added_tokens_pair()) == (2, 4)
    b = PostProcessor.bert("[CLS]", 101, "[SEP]", 102)
    assert (b.added_tokens_single(), b.added_tokens_pair()) == (2, 3)
    t = PostProcessor.template("<s> $A", "<s>", [("s", 1), ("", 2), ("$A", 3), ("> $", 4), ("s", 5)])
    assert (t.added_tokens_single(), t.added_tokens_pair()) == (5, 3)
    assert PostProcessor.template("<s> $A", None, [("<s>", 1)]).added_tokens_pair() == 0
    s = PostProcessor.sequence([b, r, PostProcessor.sequence([d])])
    assert (s.added_tokens_single(), s.added_tokens_pair()) == (6, 9)
    assert s.process([1], [2]) == ref.process(("sequence", [pc.BERT, pc.ROBERTA, ref.DEFAULT]), [1], [2])
    assert PostProcessor.sequence([]).process([1, 2], [3]) == [1, 2]
    assert PostProcessor.template("$A").process([0, 0xFFFFFFFF]) == [0, 0xFFFFFFFF]
    for call, err in ((lambda: b.process(["a"]), TypeError), (lambda: b.process([1.5]), TypeError), (lambda: b.process([-1]), OverflowError),
                      (lambda: b.process([1 << 32]), OverflowError), (lambda: b.process("12"), TypeError), (lambda: b.process(5), TypeError),
                      (lambda: b.process([1], [None]), TypeError), (lambda: b.process_batch([[1]], [[1 << 32]]), OverflowError),
                      (lambda: PostProcessor.bert("a", "1", "b", 2), TypeError), (lambda: PostProcessor.bert("a", 1, "b", 1 << 32), OverflowError),
                      (lambda: PostProcessor.bert(1, 1, "b", 2), TypeError), (lambda: PostProcessor.roberta("a", 1, "b", 2, 1), TypeError),
                      (lambda: PostProcessor.template("$A", None, [("a", -1)]), OverflowError),
                      (lambda: PostProcessor.template("$A", None, [["a", 1]]), TypeError), (lambda: PostProcessor.template(b"$A"), TypeError),
                      (lambda: PostProcessor.sequence([b, "x"]), TypeError), (lambda: b.process_batch([[1]], [None, None]), ValueError),
                      (lambda: b.process_padded([[1]], strategy="shortest"), ValueError),
                      (lambda: b.process_padded([[1]], truncate_to=-1), OverflowError)):
        with pytest.raises(err):
            call()
