"""CPU tests of complexity_tokenizer.BpeTrainer: the reference's signature and getters
(src/bindings/trainers.rs:226-279), its argument errors in the style of Trainer's, the C ABI's
exports, and the loud failure without a device.  No GPU."""
import ctypes
import inspect
import os

import pytest

import complexity_tokenizer
from complexity_tokenizer import BpeTrainer, DeviceError
from complexity_tokenizer import _native as _n

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signature_is_the_references():
    assert "BpeTrainer" in complexity_tokenizer.__all__
    p = inspect.signature(BpeTrainer.__init__).parameters
    assert list(p)[1:] == ["vocab_size", "min_frequency", "special_tokens", "show_progress", "end_of_word_suffix",
                           "continuing_subword_prefix", "device"]
    assert [p[k].default for k in list(p)[1:]] == [30000, 2, None, True, None, None, 0]
    t = BpeTrainer()
    assert t.vocab_size == 30000 and t.min_frequency == 2
    t = BpeTrainer(10000, 5, ["<s>"], False, "</w>", "##")
    assert t.vocab_size == 10000 and t.min_frequency == 5  # src/bpe_trainer.rs:513-524
    assert not hasattr(t, "initial_alphabet") and not hasattr(t, "limit_alphabet")


def test_argument_errors():
    with pytest.raises(TypeError):
        BpeTrainer(vocab_size="10")
    with pytest.raises(TypeError):
        BpeTrainer(min_frequency=2.0)
    with pytest.raises(TypeError):
        BpeTrainer(vocab_size=True)
    with pytest.raises(OverflowError):
        BpeTrainer(min_frequency=-1)
    with pytest.raises(OverflowError):
        BpeTrainer(vocab_size=-1)
    with pytest.raises(OverflowError):
        BpeTrainer(min_frequency=1 << 32)
    with pytest.raises(OverflowError):
        BpeTrainer(vocab_size=1 << 64)
    with pytest.raises(TypeError):
        BpeTrainer(special_tokens="<s>")
    with pytest.raises(TypeError):
        BpeTrainer(special_tokens=["<s>", 3])
    with pytest.raises(TypeError):
        BpeTrainer(end_of_word_suffix=3)
    with pytest.raises(TypeError):
        BpeTrainer(continuing_subword_prefix=b"##")
    with pytest.raises(TypeError):
        BpeTrainer().train("one text")
    with pytest.raises(TypeError):
        BpeTrainer().train_words({b"ab": 1})
    with pytest.raises(OverflowError):
        BpeTrainer().train_words({"ab": 1 << 32})


def test_exports_and_header():
    lib = ctypes.CDLL(_n.LIB_PATH)
    with open(os.path.join(ROOT, "include", "ctok_bpe_trainer.h")) as f:
        header = f.read()
    names = [n for n in _n.SIGS if n.startswith("ctok_bpe_trainer_")]
    assert len(names) == 12
    for name in names:
        assert hasattr(lib, name) and name + "(" in header, name
    # the two conventions are stated where the C ABI is declared
    assert "ascending code point" in header and "smallest (symbol id of first" in header


def test_null_arguments_are_refused():
    h = ctypes.c_void_p()
    assert _n.lib.ctok_bpe_trainer_create(None, ctypes.byref(h)) == _n.CTOK_E_ARG
    t = BpeTrainer()
    assert _n.lib.ctok_bpe_trainer_train(t._h, None, None, 1) == _n.CTOK_E_ARG
    assert _n.lib.ctok_bpe_trainer_train_words(t._h, None, None, None, 1) == _n.CTOK_E_ARG
    assert _n.lib.ctok_bpe_trainer_stats(t._h, None) == _n.CTOK_E_ARG
    assert _n.lib.ctok_bpe_trainer_vocab_size(None) == 0 and _n.lib.ctok_bpe_trainer_num_merges(None) == 0
    _n.lib.ctok_bpe_trainer_destroy(None)


def test_before_training_everything_is_empty():
    t = BpeTrainer(vocab_size=100)
    assert t.symbols() == [] and t.pair_counts() == {}
    st = t.stats()
    assert st["merges"] == 0 and st["rebuilds"] == 0 and st["table_capacity"] == 0
    assert _n.lib.ctok_bpe_trainer_vocab_size(t._h) == 0


def test_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(DeviceError):
        BpeTrainer(vocab_size=50, min_frequency=1).train(["hello world"])
    with pytest.raises(DeviceError):
        BpeTrainer(vocab_size=50, min_frequency=1).train_words({"ab": 2})
    with pytest.raises(DeviceError):
        BpeTrainer().word_counts(["hello world"])
