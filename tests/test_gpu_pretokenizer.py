"""GPU parity of complexity_tokenizer.PreTokenizer (csrc/pretok.hip) against the restatement of the
reference's src/pretokenizers.rs (tests/pretok_ref.py).  Exact equality of word lists everywhere; the
batches are those of tests/pretok_cases.py, which tests/test_pretok_cpu.py runs through the CPU build
of the same rules first."""
import numpy as np
import pytest

from complexity_tokenizer import Normalizer, PreTokenizer, UnsupportedConfigError, WordPieceModel
from tests import pretok_cases as pc
from tests import pretok_ref as ref
from tests.wordpiece_ref import RefWordPieceModel

pytestmark = pytest.mark.gpu


def check(pt, texts, made=None):
    p = made or ref.to_pretokenizer(pt)
    got = p.pre_tokenize_batch(texts)
    assert len(got) == len(texts)
    bad = [i for i, t in enumerate(texts) if got[i] != ref.pre_tokenize(pt, t)]
    assert not bad, (pt, len(bad), texts[bad[0]][:80], got[bad[0]][:8], ref.pre_tokenize(pt, texts[bad[0]])[:8])
    return p


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_case(name):
    pt, texts = pc.CASES[name]()
    check(pt, texts)


@pytest.mark.parametrize("i", range(len(pc.EVERY)))
def test_quirks_under_every_pre_tokenizer(i):
    pt = pc.EVERY[i]
    p = check(pt, pc.QUIRKS + pc.ADJACENT)
    for t in pc.QUIRKS[:12]:  # pre_tokenize is the batch of one
        assert p.pre_tokenize(t) == p.pre_tokenize_batch([t])[0] == ref.pre_tokenize(pt, t), (pt, t)


# every behaviour and `invert`, over literals, class atoms and runs of them
RANDOM_SPLITS = [("split", r"\s", "Removed", False), ("split", "aa", "Removed", True), ("split", r"\d+", "Isolated", False),
                 ("split", "ab", "Isolated", True), ("split", r"\p{L}+", "MergedWithPrevious", False), ("split", "!", "MergedWithPrevious", False),
                 ("split", r"[^\s\p{L}\p{N}]", "MergedWithNext", False), ("split", "aa", "MergedWithNext", False),
                 ("split", r"\d", "Contiguous", False), ("split", "a", "Contiguous", False), ("split", r"\p{L}+", "Removed", False),
                 ("split", "a", "Removed", False)]


@pytest.mark.parametrize("pool", sorted(pc.POOLS))
def test_seeded_random_strings(pool):
    texts = pc.random_texts(pool, 20264, 1500, 200)
    for pt in pc.SINGLE + RANDOM_SPLITS + pc.SEQUENCES:
        check(pt, texts)


def test_the_empty_batch():
    for pt in (("bert",), ("byte_level", True), ("split", "a", "Removed", False)):
        p = ref.to_pretokenizer(pt)
        assert p.pre_tokenize_batch([]) == []
        words, word_off, text_word = p.pre_tokenize_packed(np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.uint64))
        assert words.size == 0 and word_off.tolist() == [0] and text_word.tolist() == [0]


def _pack(texts):
    raw = [t.encode() for t in texts]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    return np.frombuffer(b"".join(raw), dtype=np.uint8), off


def test_packed_form_is_the_batch_form():
    texts = pc.QUIRKS + pc.random_texts("mixed_scripts", 3, 200)
    for pt in (("bert",), ("byte_level", True), pc.SEQUENCES[2], ("sequence", [("split", "a", "Removed", False), ("metaspace", "▁", True)])):
        p = ref.to_pretokenizer(pt)
        words, word_off, text_word = p.pre_tokenize_packed(*_pack(texts))
        raw, wo, tw = words.tobytes(), word_off.tolist(), text_word.tolist()
        assert tw[0] == 0 and tw[-1] == len(wo) - 1 and wo[-1] == len(raw) and wo == sorted(wo)
        got = [[raw[wo[j]:wo[j + 1]].decode() for j in range(tw[i], tw[i + 1])] for i in range(len(texts))]
        assert got == p.pre_tokenize_batch(texts) == [ref.pre_tokenize(pt, t) for t in texts]


def test_stats_tell_splitters_from_rewriters():
    p = PreTokenizer.sequence([PreTokenizer.whitespace(), PreTokenizer.punctuation(), PreTokenizer.digits(True),
                               PreTokenizer.split(r"\d", "Contiguous"), PreTokenizer.unicode_scripts()])
    assert p.pre_tokenize_batch(["ab, c1", "d"]) == [["ab", ",", "c", "1"], ["d"]]
    st = p.last_stats
    assert st["steps"] == 5 and st["steps_rewriting"] == 0 and st["bytes_peak"] == st["bytes_in"] == 7
    assert st["words"] == 5 and st["bytes_out"] == 6
    assert [n for n, _ in st["stages"]] == ["whitespace", "punctuation", "digits", "split", "unicode_scripts", "gather"]
    p = PreTokenizer.sequence([PreTokenizer.whitespace(), PreTokenizer.byte_level()])
    assert p.pre_tokenize_batch(["é x"]) == [["Ã©", "x"]]
    st = p.last_stats
    assert st["steps_rewriting"] == 1 and st["bytes_in"] == 4 and st["bytes_out"] == 5 and st["words"] == 2


UNSUPPORTED = ["", "a|b", "(a)", ".", "^a", "a$", r"\w", r"\w+", r"\bfoo", "a*", "a?", r"\s*", r"\s+?", r"\d{2}", "(?i)a", r"\s\s",
               "[a-z][0-9]", "[[:alpha:]]", r"\p{Lu}"]


@pytest.mark.parametrize("pattern", UNSUPPORTED)
def test_unsupported_patterns_are_refused(pattern):
    with pytest.raises(UnsupportedConfigError) as e:
        PreTokenizer.split(pattern, "Isolated")
    assert pattern in str(e.value)


def test_argument_errors():
    for bad in ("", "ab", "▁▁"):
        with pytest.raises(ValueError):
            PreTokenizer.metaspace(bad)
        with pytest.raises(ValueError):
            PreTokenizer.char_delimiter_split(bad)
    for bad in (1, b"_", None):
        with pytest.raises(TypeError):
            PreTokenizer.metaspace(bad)
        with pytest.raises(TypeError):
            PreTokenizer.char_delimiter_split(bad)
    with pytest.raises(TypeError):
        PreTokenizer.byte_level(1)
    with pytest.raises(TypeError):
        PreTokenizer.metaspace("_", "yes")
    with pytest.raises(TypeError):
        PreTokenizer.digits(None)
    with pytest.raises(TypeError):
        PreTokenizer.split(b"a")
    with pytest.raises(TypeError):
        PreTokenizer.split("a", 1)
    with pytest.raises(TypeError):
        PreTokenizer.split("a", "Removed", 0)
    with pytest.raises(TypeError):
        PreTokenizer.sequence("ab")
    with pytest.raises(TypeError):
        PreTokenizer.sequence([PreTokenizer.bert(), "bert"])
    p = PreTokenizer.bert()
    with pytest.raises(TypeError):
        p.pre_tokenize(b"bytes")
    with pytest.raises(TypeError):
        p.pre_tokenize_batch("a bare str")
    with pytest.raises(ValueError):  # CTOK_E_ARG: not UTF-8
        p.pre_tokenize_packed(np.array([0xC3, 0x28], dtype=np.uint8), np.array([0, 2], dtype=np.uint64))
    assert repr(PreTokenizer.sequence([PreTokenizer.digits(True), PreTokenizer.split("a")])) == \
        "PreTokenizer.sequence([PreTokenizer.digits(True), PreTokenizer.split('a', 'Removed', False)])"


def test_device_pointers_on_a_side_stream():
    import torch
    pt = ("sequence", [("split", "q", "Removed", True), ("metaspace", "▁", True), ("unicode_scripts",)])
    p = ref.to_pretokenizer(pt)
    texts = pc.QUIRKS + pc.random_texts("mixed_scripts", 7, 300)
    want_words, want_off, want_tw = p.pre_tokenize_packed(*_pack(texts))
    raw, off = _pack(texts)
    nb, nw = int(want_words.size), int(want_off.size) - 1
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_text = torch.from_numpy(raw.copy()).to(dev)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev)
        d_words = torch.full((nb + 32,), 0xAB, dtype=torch.uint8, device=dev)
        d_woff = torch.full((nw + 1 + 8,), -7, dtype=torch.int64, device=dev)
        d_tw = torch.full((len(texts) + 1,), -7, dtype=torch.int64, device=dev)
        stream.synchronize()
        args = (d_text.data_ptr(), d_off.data_ptr(), len(texts), int(off[-1]), d_words.data_ptr())
        for cap_b, cap_w in ((nb - 1, nw), (nb, nw - 1)):  # a byte short, a word short: nothing is written
            with pytest.raises(BufferError) as e:
                p.pre_tokenize_packed_device(*args, cap_b, d_woff.data_ptr(), cap_w, d_tw.data_ptr(), stream.cuda_stream)
            assert (e.value.needed_bytes, e.value.needed_words) == (nb, nw)
            assert bool((d_words == 0xAB).all()) and bool((d_woff == -7).all()) and bool((d_tw == -7).all())
        got = p.pre_tokenize_packed_device(*args, nb, d_woff.data_ptr(), nw, d_tw.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    assert got == (nb, nw)
    words = d_words.cpu().numpy()
    assert words[:nb].tobytes() == want_words.tobytes() and bool((words[nb:] == 0xAB).all())
    woff = d_woff.cpu().numpy()
    assert woff[:nw + 1].view(np.uint64).tolist() == want_off.tolist() and bool((woff[nw + 1:] == -7).all())
    assert d_tw.cpu().numpy().view(np.uint64).tolist() == want_tw.tolist()
    body, wo, tw = want_words.tobytes(), want_off.tolist(), want_tw.tolist()
    assert [[body[wo[j]:wo[j + 1]].decode() for j in range(tw[i], tw[i + 1])] for i in range(len(texts))] == \
        [ref.pre_tokenize(pt, t) for t in texts]


def test_device_path_takes_ill_formed_bytes():
    """The device entry takes bytes as they are.  Words never cross texts, so a text that is UTF-8
    gives what the restatement gives whatever its neighbours hold, and every word is a slice of
    its own text under a pure splitter."""
    import random

    import torch
    rng = random.Random(11)
    raw = [bytes(rng.choice([0x61, 0x20, 0x27, 0x73, 0x31, 0x2C, 0xC3, 0xA9, 0xE2, 0x80, 0x83, 0xE3, 0xF0, 0x9F, 0xED, 0xA0, 0xC0, 0xF4])
                 for _ in range(rng.randrange(0, 14))) for _ in range(2000)]
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    np.cumsum([len(r) for r in raw], out=off[1:])
    nb = int(off[-1])
    dev = torch.device("cuda", 0)
    d_text = torch.from_numpy(np.frombuffer(b"".join(raw), dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    for pt in (("bert",), ("gpt2",), ("unicode_scripts",), ("split", r"\S+", "Removed", False), ("byte_level", True),
               ("metaspace", "▁", True)):
        p = ref.to_pretokenizer(pt)
        cap_b, cap_w = 4 * nb + 4 * len(raw), nb + len(raw)
        d_words = torch.zeros(cap_b, dtype=torch.uint8, device=dev)
        d_woff = torch.zeros(cap_w + 1, dtype=torch.int64, device=dev)
        d_tw = torch.zeros(len(raw) + 1, dtype=torch.int64, device=dev)
        n_b, n_w = p.pre_tokenize_packed_device(d_text.data_ptr(), d_off.data_ptr(), len(raw), nb, d_words.data_ptr(), cap_b,
                                                d_woff.data_ptr(), cap_w, d_tw.data_ptr())
        body, wo, tw = d_words.cpu().numpy()[:n_b].tobytes(), d_woff.cpu().numpy()[:n_w + 1].tolist(), d_tw.cpu().numpy().tolist()
        assert tw[0] == 0 and tw[-1] == n_w and wo[0] == 0 and wo[-1] == n_b
        for i, t in enumerate(raw):
            words = [body[wo[j]:wo[j + 1]] for j in range(tw[i], tw[i + 1])]
            try:
                s = t.decode("utf-8")
            except UnicodeDecodeError:
                if pt[0] not in ("byte_level", "metaspace"):
                    at = 0
                    for w in words:  # slices of the text, in order
                        at = t.index(w, at) + len(w)
                continue
            assert [w.decode("utf-8") for w in words] == ref.pre_tokenize(pt, s), (pt, t)


def test_in_front_of_the_wordpiece_model():
    """Normalizer.bert() then PreTokenizer.bert() then WordPieceModel.encode_batch: `bert` words hold
    no whitespace, so the words joined by ' ' are what the model splits again."""
    from tests import normalizer_ref
    vocab = {t: i for i, t in enumerate(["[UNK]", "hello", ",", "world", "!", "世", "界", "un", "##aff", "##able", "cafe", "2", "##0",
                                         "##2", "##4", "-", "x"])}
    texts = ["Hello, WORLD!", "世界unaffable", "Café 2024", "", "x-x 　x", "¿x?"]
    norm = ("bert", True, True, None, True)
    normed = normalizer_ref.to_normalizer(norm).normalize_batch(texts)
    assert normed == [normalizer_ref.normalize(norm, t) for t in texts]
    words = PreTokenizer.bert().pre_tokenize_batch(normed)
    want_words = [ref.pre_tokenize(("bert",), t) for t in normed]
    assert words == want_words
    got = WordPieceModel(vocab).encode_batch([" ".join(w) for w in words])
    model = RefWordPieceModel(vocab)
    assert got == [model.encode(" ".join(w)) for w in want_words]
    assert got[0] == [vocab["hello"], vocab[","], vocab["world"], vocab["!"]]
    assert got[1] == [vocab["世"], vocab["界"], vocab["un"], vocab["##aff"], vocab["##able"]]
