"""tests/pipeline_windows_ref.py pinned on the CPU: the array form of the reference's truncate,
truncate_with_stride and pad against hand-written expectations -- the offsets that stay misaligned after a
BERT post-processor, the None prefix of sequence_ids on a left pad, the windows of a short row, the panics --
and the inputs that tests/test_gpu_pipeline_windows.py expects to run without a panic."""
import numpy as np

from tests import pipeline_windows_ref as wr
from tests.pipeline_encoding_ref import PanicException

N = wr.NONE


def test_bert_offsets_stay_misaligned():
    ref = wr.make_ref(post_processor=wr.BERT)
    got = wr.windows_ref(ref, ["a b"], mode=None, max_length=6, padding="max_length")
    assert got["input_ids"].tolist() == [[7, 0, 1, 8, 11, 11]] and got["attention_mask"].tolist() == [[1, 1, 1, 1, 0, 0]]
    assert got["special_tokens_mask"].tolist() == [[1, 0, 1, 1, 1, 1]] and got["token_type_ids"].tolist() == [[0] * 6]
    # two entries for four ids: cell 0 holds the span of "a" under [CLS]
    assert got["offset_mapping"].tolist() == [[[0, 1], [2, 3], [0, 0], [0, 0], [0, 0], [0, 0]]] and got["offsets_len"].tolist() == [2]
    assert got["word_ids"].tolist() == [[0, 1, N, N, N, N]]
    assert got["sequence_ids"].tolist() == [[0, 0, N, N, N, N]] and got["sequence_len"].tolist() == [4]  # two entries and two None
    assert got["row_len"].tolist() == [6] and got["row_window"].tolist() == [0, 1]
    # cut to three ids: three of the three entries stay, under [CLS] a b
    got = wr.windows_ref(ref, ["a b c", "a"], mode="cut", max_length=3)
    assert got["input_ids"].tolist() == [[7, 0, 1], [7, 0, 8]] and got["offset_mapping"][0].tolist() == [[0, 1], [2, 3], [4, 5]]
    assert got["offsets_len"].tolist() == [3, 1] and got["overflow_to_sample_mapping"].tolist() == [0, 1]


def test_left_pad_puts_none_in_front_of_sequence_ids_only():
    ref = wr.make_ref(post_processor=wr.BERT)
    got = wr.windows_ref(ref, ["a b"], ["x"], mode=None, max_length=7, padding="max_length", pad_left=True)
    assert got["input_ids"].tolist() == [[11, 11, 7, 0, 1, 5, 8]] and got["token_type_ids"].tolist() == [[0, 0, 0, 0, 1, 0, 0]]
    assert got["sequence_ids"].tolist() == [[N, N, 0, 0, 1, N, N]] and got["sequence_len"].tolist() == [5]
    assert got["offset_mapping"][0, :4].tolist() == [[0, 1], [2, 3], [0, 1], [0, 0]] and got["offsets_len"].tolist() == [3]
    assert got["word_ids"].tolist() == [[0, 1, 0, N, N, N, N]]
    got = wr.windows_ref(ref, ["a"], mode=None, padding="longest", pad_id=99)
    assert got["input_ids"].tolist() == [[7, 0, 8]]
    assert wr.windows_ref(ref, ["a", ""], mode=None, padding="longest", pad_id=99)["input_ids"].tolist() == [[7, 0, 8], [7, 8, 99]]


def test_windows_of_a_short_row():
    ref = wr.make_ref()
    got = wr.windows_ref(ref, ["a b c q r", "x"], mode="windows", max_length=2, stride=1, padding="max_length")
    assert got["input_ids"].tolist() == [[0, 1], [1, 2], [2, 3], [3, 4], [5, 11]]
    assert got["window_start"].tolist() == [0, 1, 2, 3, 0] and got["row_window"].tolist() == [0, 4, 5]
    assert got["overflow_to_sample_mapping"].tolist() == [0, 0, 0, 0, 1] and got["row_len"].tolist() == [2] * 5
    assert got["offset_mapping"][1].tolist() == [[2, 3], [4, 5]] and got["word_ids"][3].tolist() == [3, 4]
    assert got["sequence_len"].tolist() == [2, 2, 2, 2, 2] and got["sequence_ids"][4].tolist() == [0, N]
    got = wr.windows_ref(ref, ["a b c q r"], mode="windows", max_length=3, stride=0)
    assert got["input_ids"].tolist() == [[0, 1, 2], [3, 4, 11]] and got["row_len"].tolist() == [3, 2]  # the last window is not padded
    assert got["attention_mask"].tolist() == [[1, 1, 1], [1, 1, 0]] and got["special_tokens_mask"].tolist() == [[0, 0, 0], [0, 0, 1]]


def test_panics():
    ref = wr.make_ref(post_processor=wr.BERT)
    text = "a b c"  # n = 3, P = 5
    assert isinstance(wr.windows_ref(ref, [text], mode="cut", max_length=4), PanicException)
    for m in (1, 2, 3, 5, 6):
        assert isinstance(wr.windows_ref(ref, [text], mode="cut", max_length=m), dict), m
    for m in (1, 2, 3, 4):
        assert isinstance(wr.windows_ref(ref, [text], mode="windows", max_length=m), PanicException), m
    assert isinstance(wr.windows_ref(ref, [text], mode="windows", max_length=5), dict)
    # an added token whose id is outside the vocab has no token string
    ref = wr.make_ref(added=wr.SPECIAL + [wr.pc.added("<n>", 50)])
    assert isinstance(wr.windows_ref(ref, ["a <n> b"], mode="cut", max_length=2, add_special_tokens=False), dict)
    assert isinstance(wr.windows_ref(ref, ["<n> <n> b"], mode="cut", max_length=2, add_special_tokens=False), PanicException)
    assert isinstance(wr.windows_ref(ref, ["a <n> b"], mode="windows", max_length=2, add_special_tokens=False), PanicException)


def test_gpu_inputs_that_must_not_panic():
    ref = wr.make_ref()
    for m, stride, texts in wr.boundary_cases():
        got = wr.windows_ref(ref, texts, mode="windows", max_length=m, stride=stride)
        assert isinstance(got, dict), (m, stride)
        step = m - stride
        lens = [len(t.split()) for t in texts]
        assert np.diff(got["row_window"]).tolist() == [1 if p <= m else 1 + -(-(p - m) // step) for p in lens]
    got = wr.windows_ref(ref, wr.many_windows_texts(), mode="windows", max_length=2, stride=1)
    assert isinstance(got, dict) and got["row_window"][-1] > 4999 + 3000 and int(np.diff(got["row_window"]).max()) == 4999
    for pp in (wr.BERT, wr.ROBERTA, wr.NOTHING):
        ref = wr.make_ref(post_processor=pp)
        assert isinstance(wr.windows_ref(ref, ["a b c", "", "x"], mode="windows", max_length=5, stride=2), dict)
        assert isinstance(wr.windows_ref(ref, ["a b c", "", "x"], mode="cut", max_length=5), dict)
