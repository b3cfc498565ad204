"""GPU parity of complexity_tokenizer.Normalizer (csrc/normalize.hip, csrc/lowercase.hip) against the
restatement of the reference's src/normalizers.rs (tests/normalizer_ref.py).  Exact equality
everywhere; the batches are those of tests/normalizer_cases.py, which tests/test_normalize_cpu.py runs
through the CPU build of the same header first (the 60,000-mark run among them, with its step count)."""
import numpy as np
import pytest

from complexity_tokenizer import Normalizer, WordPieceModel
from tests import normalizer_cases as nc
from tests import normalizer_ref as ref
from tests.wordpiece_ref import RefWordPieceModel

pytestmark = pytest.mark.gpu


def check(norm, texts):
    nz = ref.to_normalizer(norm)
    got = nz.normalize_batch(texts)
    assert len(got) == len(texts)
    bad = [i for i, t in enumerate(texts) if got[i] != ref.normalize(norm, t)]
    assert not bad, (norm, len(bad), texts[bad[0]], got[bad[0]], ref.normalize(norm, texts[bad[0]]))
    return nz


@pytest.mark.parametrize("name", sorted(nc.CASES))
def test_case(name):
    norm, texts = nc.CASES[name]()
    check(norm, texts)


@pytest.mark.parametrize("pool", sorted(nc.POOLS))
def test_seeded_random_strings(pool):
    texts = nc.random_texts(pool, 20262, 1500)
    for norm in [(k,) for k in nc.FORMS] + [("strip_accents",), nc.BERT_DEFAULT, nc.ALL_KINDS]:
        check(norm, texts)


def test_normalize_is_the_batch_of_one():
    for norm in [("nfkc",), nc.BERT_DEFAULT, nc.ALL_KINDS, ("replace", "", "-"), ("strip",)]:
        nz = ref.to_normalizer(norm)
        for t in nc.MIXED:
            one = nz.normalize(t)
            assert one == nz.normalize_batch([t])[0] == ref.normalize(norm, t), (norm, t, one)


def test_a_step_that_changes_nothing_is_not_copied():
    nz = Normalizer.sequence([Normalizer.nfc(), Normalizer.lowercase(), Normalizer.strip()])
    assert nz.normalize_batch(["plain ascii", "already lower"]) == ["plain ascii", "already lower"]
    st = nz.last_stats
    assert st["steps"] == 5 and st["steps_changed"] == 0 and st["bytes_out"] == st["bytes_in"] == 24
    assert [n for n, _ in st["stages"]] == ["decompose", "reorder", "compose", "lowercase", "strip"]
    assert nz.normalize_batch(["\u00c9 "]) == ["\u00e9"]
    assert nz.last_stats["steps_changed"] == 4  # decompose, compose, lowercase, strip


def test_packed_and_argument_errors():
    nz = Normalizer.nfkd()
    out, off = nz.normalize_packed(np.frombuffer("\ufdfa\u00e9".encode(), dtype=np.uint8), np.array([0, 3, 5], dtype=np.uint64))
    want = [ref.normalize(("nfkd",), "\ufdfa").encode(), "e\u0301".encode()]
    assert off.tolist() == [0, len(want[0]), len(want[0]) + 3] and out.tobytes() == b"".join(want)
    with pytest.raises(ValueError):  # CTOK_E_ARG: not UTF-8
        nz.normalize_packed(np.array([0xC3, 0x28], dtype=np.uint8), np.array([0, 2], dtype=np.uint64))
    with pytest.raises(TypeError):
        nz.normalize(b"bytes")
    with pytest.raises(TypeError):
        nz.normalize_batch("a bare str")
    with pytest.raises(TypeError):
        Normalizer.replace("a", 1)
    with pytest.raises(TypeError):
        Normalizer.bert(lowercase=1)
    with pytest.raises(TypeError):
        Normalizer.precompiled("ab")
    with pytest.raises(ValueError):
        Normalizer.precompiled([("a", "b", "c")])
    with pytest.raises(TypeError):
        Normalizer.sequence([Normalizer.nfc(), "nfc"])


def test_too_many_steps_is_refused():
    from complexity_tokenizer import UnsupportedConfigError
    assert Normalizer.precompiled([("a", "b")] * 1024).normalize("a") == "b"
    with pytest.raises(UnsupportedConfigError):
        Normalizer.precompiled([("a", "b")] * 1025)


def test_device_pointers_on_a_side_stream():
    import torch
    norm = nc.ALL_KINDS
    nz = ref.to_normalizer(norm)
    texts = nc.MIXED + nc.random_texts("compat", 7, 300)
    want_out, want_off = nz.normalize_packed(*_pack(texts))
    raw, off = _pack(texts)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_text = torch.from_numpy(np.concatenate([raw, np.zeros(16, dtype=np.uint8)])).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        cap = int(want_off[-1])
        d_out = torch.full((cap + 32,), 0xAB, dtype=torch.uint8, device=dev)
        d_out_off = torch.zeros(len(texts) + 1, dtype=torch.int64, device=dev)
        stream.synchronize()
        # too small by one byte: the needed size comes back and nothing is written
        with pytest.raises(BufferError) as e:
            nz.normalize_packed_device(d_text.data_ptr(), d_off.data_ptr(), len(texts), int(off[-1]), d_out.data_ptr(), cap - 1,
                                       d_out_off.data_ptr(), stream.cuda_stream)
        assert e.value.needed == cap
        assert bool((d_out == 0xAB).all())
        n = nz.normalize_packed_device(d_text.data_ptr(), d_off.data_ptr(), len(texts), int(off[-1]), d_out.data_ptr(), cap,
                                       d_out_off.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    assert n == cap
    got = d_out.cpu().numpy()
    assert got[:cap].tobytes() == want_out.tobytes() and bool((got[cap:] == 0xAB).all())
    assert d_out_off.cpu().numpy().view(np.uint64).tolist() == want_off.tolist()
    body = want_out.tobytes()
    assert [body[int(want_off[i]):int(want_off[i + 1])].decode() for i in range(len(texts))] == [ref.normalize(norm, t) for t in texts]


def _pack(texts):
    raw = [t.encode() for t in texts]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw), dtype=np.uint8), off


def test_in_front_of_the_wordpiece_model():
    """Normalizer.sequence([nfkc, lowercase]) then WordPieceModel.encode_batch: the host step the
    models' "no normaliser runs" left to the caller, on the device."""
    vocab = {t: i for i, t in enumerate(["[UNK]", "fi", "##le", "##s", "caf", "##e\u0301", "##\u00e9", "h2", "##o", "i", "##\u0307",
                                         "\u0635\u0644\u0649", "x", "##x"])}
    texts = ["\ufb01les CAF\u00c9", "H\u2082O \u0130x", "\ufdfa xX", "", "Cafe\u0301\u3000\ufb01"]
    norm = ("sequence", [("nfkc",), ("lowercase",)])
    got = WordPieceModel(vocab).encode_batch(ref.to_normalizer(norm).normalize_batch(texts))
    model = RefWordPieceModel(vocab)
    want = [model.encode(ref.normalize(norm, t)) for t in texts]
    assert got == want
    assert want[0] == [vocab["fi"], vocab["##le"], vocab["##s"], vocab["caf"], vocab["##\u00e9"]]
