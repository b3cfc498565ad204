"""The end of the text, and what else include/ctok.h says about the buffers of the device entry
points ("Buffers of the device entry points" there), pinned on the GPU.  Bit-exact against the
Python oracle everywhere; the inputs are those of tests/text_tail_cases.py, whose claims
tests/test_text_tail_cpu.py checks first (above all that the tails are live: a kernel that looked
past n_bytes would give other ids).

a. "The 16 bytes after the text ... must be readable device memory", "What those bytes hold changes
   no result": every case under every tail through ctok_encode_batch_device and a handful through
   ctok_encode_windows_device.
b. "ids_cap may be exactly the number of ids: nothing past ids[n_tokens) and tok_off[n_docs] is
   written", and on CTOK_E_CAPACITY "tok_off is complete, tok_off[n_docs] holds the number of ids
   needed ..., ids[0 .. ids_cap) hold the first ids_cap ids, and nothing past them is written".
c. The library's own text buffers (pad_in_text, the chunk buffers, norm_text, sub_text): "a result
   does not depend on what an earlier call left in them".
d. "d_utf8 must be 16-byte aligned when n_bytes > 0, and d_ids of the decode 4-byte aligned when
   n_ids > 0: CTOK_E_ARG otherwise, checked at the entry, before any device is used, so a refused call
   launches nothing and writes nothing".
(tests/test_text_tail_cpu.py holds the header to these words.)
e. ctok_normalizer.h / ctok_pretokenizer.h / ctok_decoder.h: "no byte outside the buffers is read" --
   inputs that are views at odd byte offsets into poisoned memory, outputs at exact capacity.

No test here goes near memory that may not be read: only the content past the end varies.
"""
import ctypes
import json

import numpy as np
import pytest

from complexity_tokenizer import PanicException, Tokenizer, pack_texts
from complexity_tokenizer import _native as _n
from tests import decoder_cases as dcs
from tests import decoder_ref, normalizer_ref, pretok_ref
from tests import normalizer_cases as ncs
from tests import pretok_cases as pcs
from tests import text_tail_cases as ttc

pytestmark = pytest.mark.gpu

G = 8                       # guard elements in front of and behind every output
S32 = 0x5A5A5A5A            # sentinel of the u32 outputs
S64 = 0x5A5A5A5A5A5A5A5A    # and of the u64 ones
S8 = 0xAB
SHORT_DOCS = ["Short one.", ""]  # in front of a case's text in the three-document layout
WIN_M, WIN_S = 16, 4


def dev():
    import torch
    return torch.device("cuda", 0)


def filled(n, value, dtype):
    import torch
    return torch.full((n,), value, dtype=dtype, device=dev())


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def text_tensor(body, tail, at=0):
    """body at byte `at` of a tensor that holds the tail's bytes everywhere else, 16 of them after
    the body; the tensor's base is 16-byte aligned."""
    import torch
    assert len(tail) == ttc.PAD
    buf = np.frombuffer((tail * (at // ttc.PAD + 1))[:at] + body + tail, dtype=np.uint8).copy()
    t = torch.from_numpy(buf).to(dev())
    assert t.data_ptr() % 16 == 0
    return t


def offsets_of(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    np.cumsum(lengths, out=off[1:])
    return off


class World:
    """One variant: its Tokenizer, its oracle, its cases and the expected ids of each layout."""

    def __init__(self, base, variant):
        obj = ttc.variant_json(base, variant)
        self.variant, self.obj = variant, obj
        self.tok = self.fresh()
        self.orc = ttc.Oracle(obj)
        self.cases = ttc.cases(variant)
        self.by_name = {c["name"]: c for c in self.cases}
        self._zero = {}

    def fresh(self):
        tok = Tokenizer.from_str(json.dumps(self.obj))
        tok.device = 0
        return tok

    def docs(self, case, layout):
        return [case["text"]] if layout == "one" else SHORT_DOCS + [case["text"]]

    def want(self, docs):
        rows = [self.orc.encode(d) for d in docs]
        return np.asarray([i for r in rows for i in r], dtype=np.uint32), offsets_of([len(r) for r in rows])

    def device(self, docs, tail, ids_cap=None, tok=None):
        """ctok_encode_batch_device on docs + tail -> (ntok or the exception, ids with guards, tok_off
        with guards, ids_cap)."""
        import torch
        raw = [d.encode() for d in docs]
        off = offsets_of([len(r) for r in raw])
        B = int(off[-1])
        d_text = text_tensor(b"".join(raw), ttc.TAILS[tail])
        d_off = torch.from_numpy(off.view(np.int64)).to(dev())
        cap = B + 2 * len(docs) + 16 if ids_cap is None else ids_cap
        d_ids = filled(cap + 2 * G, S32, torch.int32)
        d_toff = filled(len(docs) + 1 + 2 * G, S64, torch.int64)
        try:
            n = (tok or self.tok).encode_packed_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), B, d_ids[G:].data_ptr(), cap,
                                                       d_toff[G:].data_ptr())
        except RuntimeError as e:
            n = e
        torch.cuda.synchronize(dev())
        return n, u32(d_ids), u64(d_toff), cap

    def zero(self, case, layout):
        key = (case["name"], layout)
        if key not in self._zero:
            n, ids, toff, cap = self.device(self.docs(case, layout), "zeros")
            self._zero[key] = (n, ids.tobytes(), toff.tobytes())
        return self._zero[key]


@pytest.fixture(scope="module")
def worlds(gpt2_path):
    with open(gpt2_path) as f:
        base = json.load(f)
    made = {}

    def get(variant):
        if variant not in made:
            made[variant] = World(base, variant)
        return made[variant]
    return get


def outside_untouched(arr, n, sentinel):
    """arr = guard + n written elements + the rest: only [G, G + n) may differ from the sentinel."""
    return bool((arr[:G] == sentinel).all()) and bool((arr[G + n:] == sentinel).all())


# ----------------------------------------------------------------------------- a. poisoned tail

@pytest.mark.parametrize("variant", ttc.VARIANTS)
@pytest.mark.parametrize("tail", list(ttc.TAILS))
def test_poisoned_tail_device_entry(worlds, variant, tail):
    """include/ctok.h: "What those bytes hold changes no result -- they need not be zero, and nothing
    past n_bytes + 16 is read."  Every case as one document and as the last of three (one of them empty): ids and
    tok_off equal the oracle's for the text alone and those of the zero tail."""
    w = worlds(variant)
    bad = []
    for c in w.cases:
        for layout in ("one", "three"):
            docs = w.docs(c, layout)
            want_ids, want_off = w.want(docs)
            n, ids, toff, cap = w.device(docs, tail)
            ok = (n == len(want_ids) and np.array_equal(ids[G:G + n], want_ids) and np.array_equal(toff[G:G + len(docs) + 1], want_off)
                  and outside_untouched(ids, n, S32) and outside_untouched(toff, len(docs) + 1, S64))
            same = (n, ids.tobytes(), toff.tobytes()) == w.zero(c, layout)
            if not (ok and same):
                bad.append((c["name"], layout, "oracle" if not ok else "zero tail"))
    assert not bad, "%s, tail %s: %d calls differ, first %r" % (variant, tail, len(bad), bad[:8])


def oracle_windows(rows, m, s):
    """include/ctok.h ctok_encode_windows: a row of P > m ids is 1 + ceil((P - m) / (m - s)) windows,
    window k the positions [k (m - s), min(k (m - s) + m, P))."""
    wins, win_row, row_win = [], [], [0]
    for r, ids in enumerate(rows):
        P = len(ids)
        n = 1 if P <= m else 1 + -(-(P - m) // (m - s))
        for k in range(n):
            wins.append(ids[k * (m - s):min(k * (m - s) + m, P)])
            win_row.append(r)
        row_win.append(len(wins))
    return wins, win_row, row_win


def windows_device(w, docs, tail):
    import torch
    rows = [w.orc.encode(d) for d in docs]
    wins, win_row, row_win = oracle_windows(rows, WIN_M, WIN_S)
    n, width = len(wins), max(len(x) for x in wins)
    raw = [d.encode() for d in docs]
    off = offsets_of([len(r) for r in raw])
    d_text = text_tensor(b"".join(raw), ttc.TAILS[tail])
    d_off = torch.from_numpy(off.view(np.int64)).to(dev())
    d_ids = filled(n * width + 2 * G, S32, torch.int32)
    d_len = filled(n + 2 * G, S64, torch.int64)
    d_row = filled(n + 2 * G, S32, torch.int32)
    d_row_win = filled(len(docs) + 1 + 2 * G, S64, torch.int64)
    got = w.tok.encode_windows_device(d_text.data_ptr(), d_off.data_ptr(), len(docs), int(off[-1]), max_length=WIN_M, stride=WIN_S,
                                      d_ids=d_ids[G:].data_ptr(), cap=n * width, d_win_len=d_len[G:].data_ptr(),
                                      d_win_row=d_row[G:].data_ptr(), win_cap=n, d_row_win=d_row_win[G:].data_ptr(),
                                      add_special_tokens=False)
    torch.cuda.synchronize(dev())
    assert got == (n, width)
    ids, lens, rws, rw = u32(d_ids), u64(d_len), u32(d_row), u64(d_row_win)
    assert lens[G:G + n].tolist() == [len(x) for x in wins] and rws[G:G + n].tolist() == win_row
    assert rw[G:G + len(docs) + 1].tolist() == row_win
    cells = ids[G:G + n * width].reshape(n, width)
    for k, x in enumerate(wins):
        assert cells[k, :len(x)].tolist() == x, k
    assert outside_untouched(ids, n * width, S32) and outside_untouched(lens, n, S64)
    assert outside_untouched(rws, n, S32) and outside_untouched(rw, len(docs) + 1, S64)
    return ids.tobytes(), lens.tobytes(), rws.tobytes(), rw.tobytes()


@pytest.mark.parametrize("variant", ttc.VARIANTS)
def test_poisoned_tail_windows_device_entry(worlds, variant):
    """The same rule at ctok_encode_windows_device (the padded encode's front): windows, their
    lengths and rows as the oracle's ids cut by the header's formula, at exact capacities, and
    every output bit for bit what the zero tail gives."""
    w = worlds(variant)
    for name in ttc.WINDOWS:
        docs = w.docs(w.by_name[name], "three")
        zero = windows_device(w, docs, "zeros")
        for tail in ttc.TAILS:
            assert windows_device(w, docs, tail) == zero, (variant, name, tail)


# ----------------------------------------------------------------------------- b. exact capacity

def host_call(tok, docs, ids_cap):
    """ctok_encode_batch with ids inside a sentinel-filled array -> (rc, ids with guards, tok_off)."""
    text, off = pack_texts(docs)
    ids = np.full(ids_cap + 2 * G, S32, dtype=np.uint32)
    toff = np.full(len(docs) + 1 + 2 * G, S64, dtype=np.uint64)
    ex = tok._host_exec(False)
    rc = _n.lib.ctok_encode_batch(tok._h, text.ctypes.data, off.ctypes.data, len(docs), ids[G:].ctypes.data, ids_cap,
                                  toff[G:].ctypes.data, ctypes.byref(ex), None)
    return rc, ids, toff


@pytest.mark.parametrize("variant", ttc.VARIANTS)
def test_exact_capacity_and_canaries(worlds, variant):
    """include/ctok.h: "ids_cap may be exactly the number of ids: nothing past ids[n_tokens) and
    tok_off[n_docs] is written", and on CTOK_E_CAPACITY "tok_off is complete, tok_off[n_docs] holds the
    number of ids needed ..., ids[0 .. ids_cap) hold the first ids_cap ids, and nothing past them is
    written ... the next call is an ordinary call".  Token
    counts of 0, 1 and 7 mod 8 in every length class (k_emit's 8-id stores, k_wire16 and the host's
    widening work in eights), through the device entry and through ctok_encode_batch."""
    w = worlds(variant)
    picked = ttc.capacity_cases(variant, lambda text: len(w.orc.encode(text)))
    assert {(c["cls"], r) for c, r in picked} == {(k, r) for k in (0, 1, 2, 3, "long") for r in (0, 1, 7)}
    for c, r in picked:
        for layout in ("one", "three"):
            docs = w.docs(c, layout)
            want_ids, want_off = w.want(docs)
            nt, nd = len(want_ids), len(docs)
            assert len(w.orc.encode(c["text"])) % 8 == r
            what = (variant, c["name"], layout)
            # exactly enough
            n, ids, toff, cap = w.device(docs, "ff", ids_cap=nt)
            assert n == nt and np.array_equal(ids[G:G + nt], want_ids) and np.array_equal(toff[G:G + nd + 1], want_off), what
            assert outside_untouched(ids, nt, S32) and outside_untouched(toff, nd + 1, S64), what
            # one short
            n, ids, toff, cap = w.device(docs, "ff", ids_cap=nt - 1)
            assert isinstance(n, RuntimeError) and "ctok error %d" % _n.CTOK_E_CAPACITY in str(n) and "ids_cap too small" in str(n), what
            assert outside_untouched(ids, nt - 1, S32) and outside_untouched(toff, nd + 1, S64), what
            assert np.array_equal(toff[G:G + nd + 1], want_off) and np.array_equal(ids[G:G + nt - 1], want_ids[:nt - 1]), what
            # the next call on the same object is correct
            n, ids, toff, cap = w.device(docs, "ff", ids_cap=nt)
            assert n == nt and np.array_equal(ids[G:G + nt], want_ids) and np.array_equal(toff[G:G + nd + 1], want_off), what
        # host buffers: ctok_encode_batch (the 16-bit wire and its widening)
        docs = w.docs(c, "three")
        want_ids, want_off = w.want(docs)
        nt, nd = len(want_ids), len(docs)
        rc, ids, toff = host_call(w.tok, docs, nt)
        assert rc == _n.CTOK_OK and np.array_equal(ids[G:G + nt], want_ids) and np.array_equal(toff[G:G + nd + 1], want_off)
        assert outside_untouched(ids, nt, S32) and outside_untouched(toff, nd + 1, S64)
        rc, ids, toff = host_call(w.tok, docs, nt - 1)
        assert rc == _n.CTOK_E_CAPACITY and int(toff[G + nd]) == nt and np.array_equal(toff[G:G + nd + 1], want_off)
        assert outside_untouched(ids, nt - 1, S32) and outside_untouched(toff, nd + 1, S64)
        rc, ids, toff = host_call(w.tok, docs, nt)
        assert rc == _n.CTOK_OK and np.array_equal(ids[G:G + nt], want_ids)


# ----------------------------------------------------------------------------- c. call history

def host_results(tok, docs):
    """The four host entries on docs, in a comparable form."""
    ids, toff = tok.encode_packed(*pack_texts(docs))
    stats = dict(tok.last_stats)
    pad = tok.encode_padded(docs, add_special_tokens=False, padding="longest")
    win = tok.encode_windows(docs, max_length=WIN_M, stride=WIN_S, add_special_tokens=False)
    try:
        offs = tok.encode_offsets(docs)
    except PanicException as e:  # (where the reference's walk panics: the same on both objects)
        offs = str(e)
    return {"packed": (ids.tolist(), toff.tolist()),
            "padded": {k: v.tolist() for k, v in pad.items()},
            "windows": {k: v.tolist() for k, v in win.items()},
            "offsets": offs}, stats


def poison(tok, docs):
    """Every host entry on docs: what it stages and normalises stays in the library's buffers."""
    tok.encode_packed(*pack_texts(docs))
    tok.encode_padded(docs, add_special_tokens=False, padding="longest")
    tok.encode_windows(docs, max_length=WIN_M, stride=WIN_S, add_special_tokens=False)
    try:
        tok.encode_offsets(docs)
    except PanicException:
        pass


HISTORY_RUNS = [("plain", "splice"), ("plain", "rerun"), ("nfc", "splice"), ("nfc", "rerun"), ("prefix_space", "splice"), ("raw", "splice")]


@pytest.mark.parametrize("variant,mode", HISTORY_RUNS)
def test_call_history_host_entries(worlds, monkeypatch, variant, mode):
    """The library's own text buffers: the staged text (pad_in_text, the chunk buffers) and the
    spliced sub-batch (sub_text) get 16 zero bytes after them, the normalised text (norm_text) does
    not -- include/ctok.h: "a result does not depend on what an earlier call left in them".  Each
    case is encoded by every host entry after a longer call that left letters, then the second half
    of a split "e-acute", exactly where the case's staged and normalised texts end; the results equal
    those of a Tokenizer that never saw a longer text, and the oracle's.  Every batch holds a
    document NFC changes: a speculating call (plain, nfc) re-encodes it through sub_text and
    norm_text (the switches of test_gpu_parity.py test_nfc_splice_positions: CTOK_NFC_RERUN=1
    normalises the whole batch instead), prefix_space always runs on norm_text."""
    if mode == "rerun":
        monkeypatch.setenv("CTOK_NFC_RERUN", "1")
    w = worlds(variant)
    tok, clean = w.fresh(), w.fresh()
    cs = sorted((w.by_name[n] for n in ttc.HISTORY), key=lambda c: c["B"])
    for c in cs:  # (ascending: `clean` never holds a longer text than the one it encodes)
        docs = ["An ascii document.", ttc.MARK_DOC + c["text"]]
        want_clean, _ = host_results(clean, docs)
        rows = [w.orc.encode(d) for d in docs]
        assert want_clean["packed"] == ([i for r in rows for i in r], offsets_of([len(r) for r in rows]).tolist()), c["name"]
        for split in (False, True):
            poison(tok, ttc.poison_docs(docs, split))
            got, st = host_results(tok, docs)
            for entry in got:
                assert got[entry] == want_clean[entry], (variant, mode, c["name"], split, entry)
            bytes_in = sum(len(d.encode()) for d in docs)
            bytes_norm = sum(w.orc.n_bytes(d) for d in docs)
            assert st["bytes_in"] == bytes_in
            if variant == "raw":
                assert st["nfc_docs"] == 0 and st["bytes_norm"] == bytes_in == bytes_norm
            elif variant == "prefix_space" or mode == "rerun":  # the whole batch on norm_text
                assert 1 <= st["nfc_docs"] <= 2 and st["bytes_norm"] == bytes_norm != bytes_in
            else:  # the pass on the staged text, the flagged documents again through sub_text and norm_text
                assert 1 <= st["nfc_docs"] <= 2 and st["bytes_norm"] == bytes_in


# ----------------------------------------------------------------------------- d. alignment

@pytest.mark.parametrize("variant", ttc.VARIANTS)
def test_misaligned_pointers_are_refused_and_nothing_runs(worlds, variant):
    """include/ctok.h: "d_utf8 must be 16-byte aligned when n_bytes > 0, and d_ids of the decode
    4-byte aligned when n_ids > 0: CTOK_E_ARG otherwise, checked at the entry, before any device is
    used, so a refused call launches nothing and writes nothing" (for an NFC or prefix-space tokenizer
    k_nfc_check and k_norm would otherwise read the text first).  The refused calls leave the
    sentinel-filled outputs as they were and the object encodes and decodes correctly afterwards."""
    import torch
    w = worlds(variant)
    docs = w.docs(w.by_name["c16@65"], "three")
    raw = [d.encode() for d in docs]
    off = offsets_of([len(r) for r in raw])
    B, nd = int(off[-1]), len(docs)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev())
    want_ids, want_off = w.want(docs)
    for at in (1, 4, 8):
        d_text = text_tensor(b"".join(raw), ttc.TAILS["a"], at=at)
        d_ids = filled(B + 64, S32, torch.int32)
        d_toff = filled(nd + 1 + 2 * G, S64, torch.int64)
        d_len, d_row_win = filled(64, S64, torch.int64), filled(nd + 1, S64, torch.int64)
        d_row = filled(64, S32, torch.int32)
        with pytest.raises(ValueError, match="16-byte aligned"):
            w.tok.encode_packed_device(d_text.data_ptr() + at, d_off.data_ptr(), nd, B, d_ids.data_ptr(), B + 64, d_toff.data_ptr())
        with pytest.raises(ValueError, match="16-byte aligned"):
            w.tok.encode_windows_device(d_text.data_ptr() + at, d_off.data_ptr(), nd, B, max_length=WIN_M, stride=WIN_S,
                                        d_ids=d_ids.data_ptr(), cap=B + 64, d_win_len=d_len.data_ptr(), d_win_row=d_row.data_ptr(),
                                        win_cap=64, d_row_win=d_row_win.data_ptr(), add_special_tokens=False)
        torch.cuda.synchronize(dev())
        assert bool((d_ids == S32).all()) and bool((d_toff == S64).all()) and bool((d_len == S64).all())
        assert bool((d_row == S32).all()) and bool((d_row_win == S64).all())
        n, ids, toff, cap = w.device(docs, "a")
        assert n == len(want_ids) and np.array_equal(ids[G:G + n], want_ids) and np.array_equal(toff[G:G + nd + 1], want_off)
    # decode: ids two bytes off
    nt = len(want_ids)
    d_ids = torch.from_numpy(np.concatenate([want_ids, np.full(1, S32, np.uint32)]).view(np.int32)).to(dev())
    d_toff = torch.from_numpy(want_off.view(np.int64)).to(dev())
    cap = 4 * nt + 64
    d_out = filled(cap, S8, torch.uint8)
    d_out_off = filled(nd + 1, S64, torch.int64)
    with pytest.raises(ValueError, match="4-byte aligned"):
        w.tok.decode_packed_device(d_ids.data_ptr() + 2, d_toff.data_ptr(), nd, nt, d_out.data_ptr(), cap, d_out_off.data_ptr())
    torch.cuda.synchronize(dev())
    assert bool((d_out == S8).all()) and bool((d_out_off == S64).all())
    nb = w.tok.decode_packed_device(d_ids.data_ptr(), d_toff.data_ptr(), nd, nt, d_out.data_ptr(), cap, d_out_off.data_ptr())
    torch.cuda.synchronize(dev())
    body, o = d_out.cpu().numpy()[:nb].tobytes(), u64(d_out_off).tolist()
    rows = [w.orc.encode(d) for d in docs]
    assert [body[o[i]:o[i + 1]].decode() for i in range(nd)] == [w.orc.py.decode(r) for r in rows]
    assert bool((d_out[nb:] == S8).all())


# ----------------------------------------------------------------------------- e. views, newer components

VIEW_AT = [0, 1, 3, 13]


def view_runs():
    for tail in ttc.TAILS:
        for at in VIEW_AT:
            yield tail, at


NORMALIZERS = [("nfc",), ("nfkc",), ncs.ALL_KINDS]
# the batch's last text ends where a poisoned tail could compose with it: an e (U+0301 follows in one
# tail), a Hangul lead + vowel (a trailing consonant would compose) and a lone lead jamo
NORM_ENDS = ["ends in e", "lead and vowel \u1100\u1161", "lead jamo \u1100"]


@pytest.mark.parametrize("norm", NORMALIZERS, ids=lambda n: n[0])
def test_normalizer_device_views(norm):
    """ctok_normalizer.h: "no byte outside the buffers is read" -- the input a view at byte offsets 0,
    1, 3 and 13 of memory that holds a poisoned tail everywhere else (no spare zero after it), the
    output at exact capacity between sentinels; equal to tests/normalizer_ref.py."""
    import torch
    nz = normalizer_ref.to_normalizer(norm)
    for end in NORM_ENDS:
        texts = ncs.MIXED + [end]
        raw = [t.encode() for t in texts]
        off = offsets_of([len(r) for r in raw])
        want = [normalizer_ref.normalize(norm, t).encode() for t in texts]
        want_off, nb = offsets_of([len(x) for x in want]), sum(len(x) for x in want)
        d_off = torch.from_numpy(off.view(np.int64)).to(dev())
        for tail, at in view_runs():
            d_text = text_tensor(b"".join(raw), ttc.TAILS[tail], at=at)
            d_out = filled(nb + 2 * 16, S8, torch.uint8)
            d_out_off = filled(len(texts) + 1 + 2 * G, S64, torch.int64)
            n = nz.normalize_packed_device(d_text.data_ptr() + at, d_off.data_ptr(), len(texts), int(off[-1]), d_out[16:].data_ptr(), nb,
                                           d_out_off[G:].data_ptr())
            torch.cuda.synchronize(dev())
            out, oo = d_out.cpu().numpy(), u64(d_out_off)
            what = (norm[0], end, tail, at)
            assert n == nb and out[16:16 + nb].tobytes() == b"".join(want), what
            assert oo[G:G + len(texts) + 1].tolist() == want_off.tolist(), what
            assert bool((out[:16] == S8).all()) and bool((out[16 + nb:] == S8).all()) and outside_untouched(oo, len(texts) + 1, S64), what


PRETOKENIZERS = [("gpt2",), ("bert",), ("sequence", [("split", "q", "Removed", True), ("metaspace", "\u2581", True), ("unicode_scripts",)])]


@pytest.mark.parametrize("pt", PRETOKENIZERS, ids=lambda p: p[0])
def test_pretokenizer_device_views(pt):
    """ctok_pretokenizer.h: "no byte outside the buffers is read"; words, word offsets and the texts'
    first words at exact capacities, equal to tests/pretok_ref.py."""
    import torch
    p = pretok_ref.to_pretokenizer(pt)
    texts = pcs.QUIRKS + pcs.random_texts("mixed_scripts", 7, 100)
    raw = [t.encode() for t in texts]
    off = offsets_of([len(r) for r in raw])
    words = [[x.encode() for x in pretok_ref.pre_tokenize(pt, t)] for t in texts]
    flat = [x for ws in words for x in ws]
    want_woff, want_tw = offsets_of([len(x) for x in flat]), offsets_of([len(ws) for ws in words])
    nb, nw = sum(len(x) for x in flat), len(flat)
    d_off = torch.from_numpy(off.view(np.int64)).to(dev())
    for tail, at in view_runs():
        d_text = text_tensor(b"".join(raw), ttc.TAILS[tail], at=at)
        d_words = filled(nb + 2 * 16, S8, torch.uint8)
        d_woff = filled(nw + 1 + 2 * G, S64, torch.int64)
        d_tw = filled(len(texts) + 1 + 2 * G, S64, torch.int64)
        got = p.pre_tokenize_packed_device(d_text.data_ptr() + at, d_off.data_ptr(), len(texts), int(off[-1]), d_words[16:].data_ptr(), nb,
                                           d_woff[G:].data_ptr(), nw, d_tw[G:].data_ptr())
        torch.cuda.synchronize(dev())
        out, wo, tw = d_words.cpu().numpy(), u64(d_woff), u64(d_tw)
        what = (pt[0], tail, at)
        assert got == (nb, nw) and out[16:16 + nb].tobytes() == b"".join(flat), what
        assert wo[G:G + nw + 1].tolist() == want_woff.tolist() and tw[G:G + len(texts) + 1].tolist() == want_tw.tolist(), what
        assert bool((out[:16] == S8).all()) and bool((out[16 + nb:] == S8).all()), what
        assert outside_untouched(wo, nw + 1, S64) and outside_untouched(tw, len(texts) + 1, S64), what


DECODERS = [("byte_level",), ("wordpiece", "##", True), ("sequence", [("wordpiece", "##", True), ("replace", "a", "\u00e9\u00e9"), ("strip", " ", 1, 1)])]


@pytest.mark.parametrize("dec", DECODERS, ids=lambda d: d[0])
def test_decoder_device_views(dec):
    """ctok_decoder.h: "no byte outside the buffers is read"; the text at exact capacity, equal to
    tests/decoder_ref.py."""
    import torch
    d = decoder_ref.to_decoder(dec)
    docs = dcs.QUIRKS + dcs.random_token_lists("mixed", 7, 100, 60)
    flat = [t.encode() for doc in docs for t in doc]
    tok_off, doc_tok = offsets_of([len(t) for t in flat]), offsets_of([len(doc) for doc in docs])
    want = [decoder_ref.decode(dec, doc).encode() for doc in docs]
    want_off, nb = offsets_of([len(x) for x in want]), sum(len(x) for x in want)
    d_tok_off = torch.from_numpy(tok_off.view(np.int64)).to(dev())
    d_doc_tok = torch.from_numpy(doc_tok.view(np.int64)).to(dev())
    for tail, at in view_runs():
        d_raw = text_tensor(b"".join(flat), ttc.TAILS[tail], at=at)
        d_text = filled(nb + 2 * 16, S8, torch.uint8)
        d_off = filled(len(docs) + 1 + 2 * G, S64, torch.int64)
        n = d.decode_packed_device(d_raw.data_ptr() + at, d_tok_off.data_ptr(), d_doc_tok.data_ptr(), len(docs), len(flat), int(tok_off[-1]),
                                   d_text[16:].data_ptr(), nb, d_off[G:].data_ptr())
        torch.cuda.synchronize(dev())
        out, oo = d_text.cpu().numpy(), u64(d_off)
        what = (dec[0], tail, at)
        assert n == nb and out[16:16 + nb].tobytes() == b"".join(want), what
        assert oo[G:G + len(docs) + 1].tolist() == want_off.tolist(), what
        assert bool((out[:16] == S8).all()) and bool((out[16 + nb:] == S8).all()) and outside_untouched(oo, len(docs) + 1, S64), what
