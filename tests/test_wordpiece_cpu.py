"""CPU tests of complexity_tokenizer.WordPieceTrainer and WordPieceModel: the reference's signatures
(src/bindings/trainers.rs:102-134, src/bindings/models.rs:16-29), argument errors in the style of
BpeTrainer's, the C ABI's exports, the host-only methods and the loud failure without a device.
No GPU."""
import ctypes
import inspect
import os

import pytest

import complexity_tokenizer
from complexity_tokenizer import DeviceError, WordPieceModel, WordPieceTrainer
from complexity_tokenizer import _native as _n
from tests.wordpiece_ref import RefWordPieceModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signatures_are_the_references():
    assert "WordPieceTrainer" in complexity_tokenizer.__all__ and "WordPieceModel" in complexity_tokenizer.__all__
    p = inspect.signature(WordPieceTrainer.__init__).parameters
    assert list(p)[1:] == ["vocab_size", "min_frequency", "special_tokens", "continuing_subword_prefix",
                           "max_input_chars_per_word", "device"]
    assert [p[k].default for k in list(p)[1:]] == [30000, 2, None, "##", 100, 0]
    p = inspect.signature(WordPieceModel.__init__).parameters
    assert list(p)[1:] == ["vocab", "continuing_subword_prefix", "unk_token", "max_input_chars_per_word", "device"]
    assert [p[k].default for k in list(p)[2:]] == ["##", "[UNK]", 100, 0]
    for name in ("train", "train_from_iterator", "train_words", "word_counts", "merges", "stats", "pair_counts"):
        assert callable(getattr(WordPieceTrainer, name))
    for name in ("encode", "decode", "token_to_id", "id_to_token", "encode_batch", "encode_batch_flat", "get_vocab"):
        assert callable(getattr(WordPieceModel, name))
    # the getter is the vocab's size, not the target (src/bindings/trainers.rs:149-152)
    assert WordPieceTrainer(vocab_size=500).vocab_size == 0


def test_argument_errors():
    with pytest.raises(TypeError):
        WordPieceTrainer(vocab_size="10")
    with pytest.raises(TypeError):
        WordPieceTrainer(min_frequency=2.0)
    with pytest.raises(TypeError):
        WordPieceTrainer(vocab_size=True)
    with pytest.raises(OverflowError):
        WordPieceTrainer(min_frequency=-1)
    with pytest.raises(OverflowError):
        WordPieceTrainer(min_frequency=1 << 32)
    with pytest.raises(OverflowError):
        WordPieceTrainer(vocab_size=1 << 64)
    with pytest.raises(OverflowError):
        WordPieceTrainer(max_input_chars_per_word=-1)
    with pytest.raises(TypeError):
        WordPieceTrainer(special_tokens="[UNK]")
    with pytest.raises(TypeError):
        WordPieceTrainer(special_tokens=["[UNK]", 3])
    with pytest.raises(TypeError):
        WordPieceTrainer(continuing_subword_prefix=None)
    with pytest.raises(TypeError):
        WordPieceTrainer(continuing_subword_prefix=b"##")
    with pytest.raises(ValueError):
        WordPieceTrainer(continuing_subword_prefix="#\0")
    with pytest.raises(TypeError):
        WordPieceTrainer().train_from_iterator("one text")
    with pytest.raises(TypeError):
        WordPieceTrainer().train("one_file.txt")
    with pytest.raises(TypeError):
        WordPieceTrainer().train_words({b"ab": 1})
    with pytest.raises(OverflowError):
        WordPieceTrainer().train_words({"ab": 1 << 32})
    with pytest.raises(IOError):
        WordPieceTrainer().train([os.path.join(ROOT, "no", "such", "file.txt")])
    with pytest.raises(TypeError):
        WordPieceModel(["a"])
    with pytest.raises(TypeError):
        WordPieceModel({3: 1})
    with pytest.raises(TypeError):
        WordPieceModel({"a": "1"})
    with pytest.raises(OverflowError):
        WordPieceModel({"a": 1 << 32})
    with pytest.raises(TypeError):
        WordPieceModel({"a": 1}, unk_token=None)
    with pytest.raises(TypeError):
        WordPieceModel({"a": 1}).encode(b"a")
    with pytest.raises(ValueError):
        WordPieceModel({"a": 0xFFFFFFFF})  # (the one id the device keeps for "no match")


def test_train_reads_lines_before_it_needs_a_device(tmp_path):
    p = tmp_path / "bad.txt"
    p.write_bytes(b"ok\n\xff\xfe\n")
    with pytest.raises(IOError):
        WordPieceTrainer().train([str(p)])


def test_exports_and_header():
    lib = ctypes.CDLL(_n.LIB_PATH)
    with open(os.path.join(ROOT, "include", "ctok_wordpiece.h")) as f:
        header = f.read()
    names = [n for n in _n.SIGS if n.startswith("ctok_wp_") or n == "ctok_lowercase"]
    assert len(names) == 16
    for name in names:
        assert hasattr(lib, name) and name + "(" in header, name
    # the conventions are stated where the C ABI is declared
    for words in ("ascending code point", "smallest (key(a), key(b))", "2^31 +", "smallest\n *     string by UTF-8 bytes"):
        assert words in header, words


def test_null_arguments_are_refused():
    h = ctypes.c_void_p()
    assert _n.lib.ctok_wp_trainer_create(None, ctypes.byref(h)) == _n.CTOK_E_ARG
    cfg = _n.WpTrainerConfig(vocab_size=10, min_frequency=1, n_special=0, continuing_subword_prefix=None)
    assert _n.lib.ctok_wp_trainer_create(ctypes.byref(cfg), ctypes.byref(h)) == _n.CTOK_E_ARG
    cfg = _n.WpTrainerConfig(vocab_size=10, min_frequency=1, n_special=0, continuing_subword_prefix=b"\xff")
    assert _n.lib.ctok_wp_trainer_create(ctypes.byref(cfg), ctypes.byref(h)) == _n.CTOK_E_ARG
    t = WordPieceTrainer()
    assert _n.lib.ctok_wp_trainer_train(t._h, None, None, 1) == _n.CTOK_E_ARG
    assert _n.lib.ctok_wp_trainer_count(None, None, None, 0) == _n.CTOK_E_ARG
    assert _n.lib.ctok_wp_trainer_train_words(t._h, None, None, None, 1) == _n.CTOK_E_ARG
    assert _n.lib.ctok_wp_trainer_stats(t._h, None) == _n.CTOK_E_ARG
    assert _n.lib.ctok_wp_trainer_result(t._h, None, None, None) == _n.CTOK_E_ARG
    assert _n.lib.ctok_wp_trainer_vocab_size(None) == 0 and _n.lib.ctok_wp_model_vocab_size(None) == 0
    _n.lib.ctok_wp_trainer_destroy(None)
    _n.lib.ctok_wp_model_destroy(None)
    assert _n.lib.ctok_wp_model_create(None, None, None, 1, b"##", b"[UNK]", 100, 0, ctypes.byref(h)) == _n.CTOK_E_ARG
    assert _n.lib.ctok_wp_model_create(None, None, None, 0, None, b"[UNK]", 100, 0, ctypes.byref(h)) == _n.CTOK_E_ARG
    assert _n.lib.ctok_wp_model_create(None, None, None, 0, b"##", b"[UNK]", 100, 0, None) == _n.CTOK_E_ARG
    m = WordPieceModel({"a": 1})
    assert _n.lib.ctok_wp_model_encode_batch(m._h, None, None, 1, None, None) == _n.CTOK_E_ARG
    assert _n.lib.ctok_lowercase(None, None, 1, 0, None, 0, None) == _n.CTOK_E_ARG
    # a vocab string given twice, a string that is not UTF-8
    off = (ctypes.c_uint64 * 3)(0, 1, 2)
    ids = (ctypes.c_uint32 * 2)(1, 2)
    assert _n.lib.ctok_wp_model_create(b"aa", off, ids, 2, b"##", b"[UNK]", 100, 0, ctypes.byref(h)) == _n.CTOK_E_ARG
    assert _n.lib.ctok_wp_model_create(b"a\xff", off, ids, 2, b"##", b"[UNK]", 100, 0, ctypes.byref(h)) == _n.CTOK_E_ARG
    out_off = (ctypes.c_uint64 * 2)()
    out = (ctypes.c_uint8 * 8)()
    assert _n.lib.ctok_lowercase(b"\xc3", (ctypes.c_uint64 * 2)(0, 1), 1, 0, out, 8, out_off) == _n.CTOK_E_ARG


def test_before_training_everything_is_empty():
    t = WordPieceTrainer(vocab_size=100)
    assert t.merges() == [] and t.pair_counts() == {} and t.get_vocab() == {} and t.tokens() == {}
    st = t.stats()
    assert st["merges"] == 0 and st["rebuilds"] == 0 and st["table_capacity"] == 0


def test_model_host_methods_follow_the_oracle():
    vocab = {"[UNK]": 0, "play": 1, "##ing": 2, "##ed": 3, "b": 7, "a": 7, "##": 9}
    m, r = WordPieceModel(vocab), RefWordPieceModel(vocab)
    assert m.vocab_size == r.vocab_size() == 7 and m.get_vocab() == vocab
    for ids in ([1, 2], [1, 3, 1], [2, 1], [99, 1, 99, 2], [], [7, 7], [9, 1], [9, 9, 2, 0]):
        assert m.decode(ids) == r.decode(ids), ids
    assert m.id_to_token(7) == "a" and m.id_to_token(99) is None
    assert m.token_to_id("##ing") == 2 and m.token_to_id("ing") is None
    m, r = WordPieceModel(vocab, ""), RefWordPieceModel(vocab, "")
    assert m.decode([1, 2, 0]) == r.decode([1, 2, 0]) == "play##ing[UNK]"


def test_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(DeviceError):
        WordPieceTrainer(vocab_size=50, min_frequency=1).train_from_iterator(["hello world"])
    with pytest.raises(DeviceError):
        WordPieceTrainer(vocab_size=50, min_frequency=1).train_words({"ab": 2})
    with pytest.raises(DeviceError):
        WordPieceTrainer().word_counts(["hello world"])
    with pytest.raises(DeviceError):
        WordPieceModel({"a": 1}).encode("a")
    from complexity_tokenizer.wordpiece import lowercase
    with pytest.raises(DeviceError):
        lowercase(["ABC"])
