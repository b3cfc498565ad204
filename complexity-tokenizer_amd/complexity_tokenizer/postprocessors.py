"""`complexity_tokenizer.PostProcessor` (reference src/bindings/components.rs:175-229 over
src/postprocessors.rs:34-280) on the GPU, through include/ctok_postprocessor.h.

The three constructors, `process(ids, pair_ids=None)` and `added_tokens_single / _pair` are the
reference's.  A post-processor is a program of steps, compiled once into two flat lists of items (copy
the first sequence, copy the pair, insert one id), that a whole batch of rows goes through on the
device in one call (csrc/postproc.hip), quirks included: the template is walked char by char, `<` and
`[` open a token that runs through the first `>` or `]`, an unknown token adds nothing, a pair under a
template without a `$B` is dropped, a pair that is present but empty is not an absent one, and a
sequence hands the pair to its first processor only.  Ids are the whole u32 range.  There is no CPU
fallback: without a HIP device the constructors raise DeviceError.  A batch whose output reaches 2^32
ids raises RuntimeError.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as _n
from .bpe_trainer import _raise
from .normalizers import _bool_arg, _str_arg
from .wordpiece import _uint

_STRATEGIES = {"only_first": 0, "only_second": 1, "longest_first": 2}
_U32 = 0xFFFFFFFF
_USIZE = 0xFFFFFFFFFFFFFFFF


def _ids_arg(name, ids):
    """PyO3 `Vec<u32>`: a non-str sequence of ints in 0..2**32-1."""
    if isinstance(ids, str):
        raise TypeError("argument '%s': Can't extract `str` to `Vec`" % name)
    if isinstance(ids, np.ndarray) and ids.dtype == np.uint32 and ids.ndim == 1:
        return ids
    try:
        out = list(ids)
    except TypeError:
        raise TypeError("argument '%s': '%s' object cannot be converted to 'Sequence'" % (name, type(ids).__name__)) from None
    return [_uint(name, i, _U32) for i in out]


def _specials_arg(special_tokens):
    """PyO3 `Vec<(String, u32)>`: a non-str sequence of 2-tuples."""
    if isinstance(special_tokens, (str, bytes)):
        raise TypeError("argument 'special_tokens': Can't extract `str` to `Vec`")
    try:
        items = list(special_tokens)
    except TypeError:
        raise TypeError("argument 'special_tokens': '%s' object cannot be converted to 'Sequence'" % type(special_tokens).__name__) from None
    out = []
    for it in items:
        if not isinstance(it, tuple):
            raise TypeError("argument 'special_tokens': '%s' object cannot be converted to 'PyTuple'" % type(it).__name__)
        if len(it) != 2:
            raise ValueError("argument 'special_tokens': expected tuple of length 2, but got tuple of length %d" % len(it))
        if not isinstance(it[0], str):
            raise TypeError("argument 'special_tokens': '%s' object cannot be converted to 'PyString'" % type(it[0]).__name__)
        out.append((it[0], _uint("special_tokens", it[1], _U32)))
    return out


def _rows_arg(name, batch):
    if isinstance(batch, (str, bytes, bytearray)):
        raise TypeError("argument '%s': Can't extract `str` to `Vec`" % name)
    try:
        return list(batch)
    except TypeError:
        raise TypeError("argument '%s': '%s' object cannot be converted to 'Sequence'" % (name, type(batch).__name__)) from None


def _pack_rows(rows):
    off = np.zeros(len(rows) + 1, dtype=np.uint64)
    if rows:
        np.cumsum([len(r) for r in rows], out=off[1:])
    flat = np.empty(int(off[-1]), dtype=np.uint32)
    at = 0
    for r in rows:
        flat[at:at + len(r)] = r
        at += len(r)
    return flat, off


def _ptr(a):
    return a.ctypes.data if a is not None else None


class PostProcessor:
    """A post-processor; made by the static constructors, as in the reference."""

    def __init__(self, steps, added, device=0, repr_="PostProcessor"):
        # steps: [("template", single: str, pair: str | None, [(token: str, id)]) | ("bert" | "roberta", id_a, id_b)]
        self._steps = list(steps)
        self._added = added
        self._repr = repr_
        self.device = device
        self.last_stats = {}
        arr = (_n.PpStep * max(len(self._steps), 1))()
        keep = []
        for i, st in enumerate(self._steps):
            if st[0] == "template":
                single, pair = st[1].encode("utf-8"), (st[2] or "").encode("utf-8")
                toks = [t.encode("utf-8") for t, _ in st[3]]
                blob = np.frombuffer(b"".join(toks) + b"\0", dtype=np.uint8)
                off = np.zeros(len(toks) + 1, dtype=np.uint64)
                if toks:
                    np.cumsum([len(t) for t in toks], out=off[1:])
                ids = np.array([i_ for _, i_ in st[3]] + [0], dtype=np.uint32)
                bs, bp = ctypes.create_string_buffer(single, len(single) + 1), ctypes.create_string_buffer(pair, len(pair) + 1)
                keep += [blob, off, ids, bs, bp]
                arr[i] = _n.PpStep(0, 1 if st[2] is not None else 0, ctypes.cast(bs, ctypes.c_void_p), len(single),
                                   ctypes.cast(bp, ctypes.c_void_p), len(pair), blob.ctypes.data, off.ctypes.data, ids.ctypes.data,
                                   len(toks), 0, 0)
            else:
                arr[i] = _n.PpStep(1 if st[0] == "bert" else 2, 0, None, 0, None, 0, None, None, None, 0, st[1], st[2])
        h = ctypes.c_void_p()
        rc = _n.lib.ctok_postprocessor_create(arr, len(self._steps), device, ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h

    def __del__(self):
        h = getattr(self, "_h", None)
        lib = getattr(_n, "lib", None) if _n is not None else None  # (None at interpreter teardown)
        if h and lib is not None:
            lib.ctok_postprocessor_destroy(h)
            self._h = None

    def __repr__(self):
        return self._repr

    # ---- the reference's constructors (src/bindings/components.rs:183-215) --------------------------------

    @staticmethod
    def bert(cls_token, cls_id, sep_token, sep_id, device=0) -> "PostProcessor":
        """cls ids sep, and pair sep when there is a pair."""
        _str_arg("cls_token", cls_token)
        cls_id = _uint("cls_id", cls_id, _U32)
        _str_arg("sep_token", sep_token)
        sep_id = _uint("sep_id", sep_id, _U32)
        return PostProcessor([("bert", cls_id, sep_id)], (2, 3), device,
                             "PostProcessor.bert(%r, %r, %r, %r)" % (cls_token, cls_id, sep_token, sep_id))

    @staticmethod
    def roberta(bos_token, bos_id, eos_token, eos_id, add_prefix_space=False, device=0) -> "PostProcessor":
        """bos ids eos, and eos pair eos when there is a pair; add_prefix_space is stored and ignored,
        as in the reference."""
        _str_arg("bos_token", bos_token)
        bos_id = _uint("bos_id", bos_id, _U32)
        _str_arg("eos_token", eos_token)
        eos_id = _uint("eos_id", eos_id, _U32)
        aps = _bool_arg("add_prefix_space", add_prefix_space)
        pp = PostProcessor([("roberta", bos_id, eos_id)], (2, 4), device,
                           "PostProcessor.roberta(%r, %r, %r, %r, %r)" % (bos_token, bos_id, eos_token, eos_id, aps))
        pp.add_prefix_space = aps
        return pp

    @staticmethod
    def template(single, pair=None, special_tokens=(), device=0) -> "PostProcessor":
        """The template walked char by char: `$A` copies the ids, `$B` the pair if there is one, a
        `$` before any other char or at the end is skipped alone, `<` or `[` opens a token that runs
        through the first `>` or `]` (without one: to the end, then trimmed) and adds the id of the
        first equal entry of special_tokens, or nothing; every other char is skipped.  A pair uses
        `pair`, or `single` when pair is None."""
        _str_arg("single", single)
        if pair is not None:
            _str_arg("pair", pair)
        sp = _specials_arg(special_tokens)
        added = (sum(1 for t, _ in sp if t in single), sum(1 for t, _ in sp if t in pair) if pair is not None else 0)
        return PostProcessor([("template", single, pair, sp)], added, device, "PostProcessor.template(%r, %r, %r)" % (single, pair, sp))

    def process(self, ids, pair_ids=None) -> list:
        """src/bindings/components.rs:217-220"""
        ids = _ids_arg("ids", ids)
        pair = None if pair_ids is None else _ids_arg("pair_ids", pair_ids)
        return self._process_rows([ids], [pair])[0]

    def added_tokens_single(self) -> int:
        """The special_tokens entries whose string occurs in the single template (not the occurrences;
        a duplicated entry counts each time), 2 for bert and roberta, the sum for a sequence."""
        return self._added[0]

    def added_tokens_pair(self) -> int:
        """The same for the pair template, 0 without one; 3 for bert, 4 for roberta."""
        return self._added[1]

    # ---- extensions --------------------------------------------------------------------------------------

    @staticmethod
    def sequence(processors, device=0) -> "PostProcessor":
        """PostProcessor::Sequence of the reference's enum, which its Python class does not reach: the
        pair goes to the first processor only, every later one sees the result so far alone (nested
        sequences therefore flatten; the empty sequence returns the ids and drops the pair); extension."""
        if isinstance(processors, (str, bytes)):
            raise TypeError("argument 'processors': Can't extract `str` to `Vec`")
        steps, names, a, b = [], [], 0, 0
        for p in processors:
            if not isinstance(p, PostProcessor):
                raise TypeError("argument 'processors': '%s' object cannot be converted to 'PostProcessor'" % type(p).__name__)
            steps += p._steps
            names.append(repr(p))
            a += p._added[0]
            b += p._added[1]
        return PostProcessor(steps, (a, b), device, "PostProcessor.sequence([%s])" % ", ".join(names))

    @staticmethod
    def default(device=0) -> "PostProcessor":
        """default_postprocessor(), postprocessors.rs:283-292: `<s> $A </s>` / `<s> $A </s> $B </s>`
        with ids 2 and 0; extension."""
        pp = PostProcessor.template("<s> $A </s>", "<s> $A </s> $B </s>", [("<s>", 2), ("</s>", 0)], device)
        pp._repr = "PostProcessor.default()"
        return pp

    def _process_rows(self, rows, pairs):
        ids, off = _pack_rows(rows)
        if all(p is None for p in pairs):
            out, out_off = self.process_packed(ids, off)
        else:
            pair_ids, pair_off = _pack_rows([[] if p is None else p for p in pairs])
            has = np.array([p is not None for p in pairs], dtype=np.uint8)
            out, out_off = self.process_packed(ids, off, pair_ids, pair_off, has)
        flat, o = out.tolist(), out_off.tolist()
        return [flat[o[i]:o[i + 1]] for i in range(len(rows))]

    def _rows_and_pairs(self, batch, pairs):
        rows = [_ids_arg("batch", r) for r in _rows_arg("batch", batch)]
        if pairs is None:
            return rows, [None] * len(rows)
        prs = [None if p is None else _ids_arg("pairs", p) for p in _rows_arg("pairs", pairs)]
        if len(prs) != len(rows):
            raise ValueError("pairs must have an entry (a list or None) for every row of batch")
        return rows, prs

    def process_batch(self, batch, pairs=None) -> list:
        """process of every row, the whole batch in one device call; pairs[i] may be None; extension."""
        return self._process_rows(*self._rows_and_pairs(batch, pairs))

    @staticmethod
    def _packed_args(who, ids_u32, off_u64, pair_ids, pair_off, has_pair):
        ids = np.ascontiguousarray(ids_u32, dtype=np.uint32)
        off = np.ascontiguousarray(off_u64, dtype=np.uint64)
        if ids.ndim != 1 or off.ndim != 1 or off.size < 1:
            raise ValueError(who + ": ids_u32 and off_u64 must be 1-D, off_u64 with n + 1 entries")
        n = off.size - 1
        if int(off[n]) > ids.size:
            raise ValueError(who + ": the offsets reach past the ids")
        if pair_off is None:
            if pair_ids is not None or has_pair is not None:
                raise ValueError(who + ": pair_ids and has_pair need pair_off")
            return ids, off, None, None, None
        pids = np.ascontiguousarray(np.zeros(0, dtype=np.uint32) if pair_ids is None else pair_ids, dtype=np.uint32)
        poff = np.ascontiguousarray(pair_off, dtype=np.uint64)
        if pids.ndim != 1 or poff.ndim != 1 or poff.size != n + 1:
            raise ValueError(who + ": pair_ids and pair_off must be 1-D, pair_off with n + 1 entries")
        if n and int(poff.max()) > pids.size:
            raise ValueError(who + ": the pair offsets reach past the pair ids")
        has = None
        if has_pair is not None:
            has = np.ascontiguousarray(has_pair, dtype=np.uint8)
            if has.ndim != 1 or has.size != n:
                raise ValueError(who + ": has_pair must have an entry for every row")
        return ids, off, pids, poff, has

    def _run(self, packed, opts, guess):
        ids, off, pids, poff, has = packed
        n = off.size - 1
        b = _n.PpBatch(_ptr(ids), _ptr(off), _ptr(pids), _ptr(poff), _ptr(has), n)
        padded = bool(opts.padded)

        def outputs(cap):
            arrs = [np.empty(cap, dtype=np.uint32) for _ in range(4 if padded else 1)]
            out_off = np.zeros(n + 1, dtype=np.uint64)
            row_len = np.zeros(n, dtype=np.uint32)
            o = _n.PpOut(arrs[0].ctypes.data, cap, out_off.ctypes.data, *([a.ctypes.data for a in arrs[1:]] if padded else [None] * 3),
                         row_len.ctypes.data, 0, 0)
            return arrs, out_off, row_len, o

        arrs, out_off, row_len, o = outputs(guess)
        rc = _n.lib.ctok_postprocessor_run(self._h, ctypes.byref(b), ctypes.byref(opts), ctypes.byref(o))
        if rc == _n.CTOK_E_CAPACITY and o.n_ids > guess:
            # the guess was too small: the library says what it needs and keeps the result on the device
            arrs, out_off, row_len, o = outputs(int(o.n_ids))
            rc = _n.lib.ctok_postprocessor_fetch(self._h, ctypes.byref(o))
        if rc:
            _raise(rc)
        self._read_stats()
        return [a[:int(o.n_ids)] for a in arrs], out_off, row_len, int(o.width)

    def process_packed(self, ids_u32, off_u64, pair_ids=None, pair_off=None, has_pair=None):
        """(uint32 ids, uint64 off[n + 1]) of a packed batch: row i owns ids_u32[off[i]:off[i + 1]] -- the
        layout the models' encode_batch_flat returns -- and, when has_pair[i] (uint8) is not 0,
        pair_ids[pair_off[i]:pair_off[i + 1]].  has_pair=None with pair_off given: every row has a pair;
        extension."""
        packed = self._packed_args("process_packed", ids_u32, off_u64, pair_ids, pair_off, has_pair)
        n = packed[1].size - 1
        guess = int(packed[0].size) + (int(packed[2].size) if packed[2] is not None else 0) + 8 * n + 64
        arrs, out_off, _, _ = self._run(packed, _n.PpOpts(), guess)
        return arrs[0], out_off

    def process_padded(self, batch_or_packed, pairs=None, truncate_to=None, strategy="longest_first", pad_to=None, pad_id=0,
                       pad_left=False) -> dict:
        """truncate, process and pad over a batch, in the order of the reference's free functions
        (postprocessors.rs:209-280): `[rows, width]` uint32 arrays input_ids, attention_mask,
        token_type_ids, special_tokens_mask, and row_len.

        batch_or_packed is a list of id lists with pairs a list of id lists or None per row, or a tuple
        (ids_u32, off_u64) with pairs a tuple (pair_ids, pair_off[, has_pair]) as for process_packed.

        truncate_to bounds len(ids) + len(pair) of the *input* sequences, not the processed row: the
        caller subtracts added_tokens_single() or added_tokens_pair() from the length the model takes.
        only_first removes from the end of the first sequence, only_second from the pair (nothing from
        a row without one), longest_first one id at a time from the first sequence while it is not
        the shorter one, else from the pair.  pad_to="longest" pads to the longest processed row; an int
        leaves longer rows as they are, so width = max(longest row, pad_to); with None the cells past a
        row's end are filled like padding all the same.  A cell copied from the first sequence is
        (1, 0, 0) in the three masks, one copied from the pair (1, 1, 0), an id the program inserted
        (1, 0, 1), padding (0, 0, 1) with pad_id; extension."""
        if isinstance(batch_or_packed, tuple):
            if len(batch_or_packed) != 2:
                raise ValueError("process_padded: a packed batch is (ids_u32, off_u64)")
            pr = (None, None, None) if pairs is None else tuple(pairs) + (None,) * (3 - len(pairs))
            packed = self._packed_args("process_padded", batch_or_packed[0], batch_or_packed[1], pr[0], pr[1], pr[2])
        else:
            rows, prs = self._rows_and_pairs(batch_or_packed, pairs)
            ids, off = _pack_rows(rows)
            if all(p is None for p in prs):
                packed = (ids, off, None, None, None)
            else:
                pids, poff = _pack_rows([[] if p is None else p for p in prs])
                packed = (ids, off, pids, poff, np.array([p is not None for p in prs], dtype=np.uint8))
        if strategy not in _STRATEGIES:
            raise ValueError("strategy must be 'only_first', 'only_second' or 'longest_first'")
        opts = _n.PpOpts()
        if truncate_to is not None:
            opts.truncate, opts.truncate_to = 1, _uint("truncate_to", truncate_to, _USIZE)
        opts.strategy = _STRATEGIES[strategy]
        opts.padded = 1
        opts.pad_left = 1 if _bool_arg("pad_left", pad_left) else 0
        if pad_to is not None and pad_to != "longest":
            opts.pad_to = _uint("pad_to", pad_to, _USIZE)
        opts.pad_id = _uint("pad_id", pad_id, _U32)
        n = packed[1].size - 1
        longest = int(np.diff(packed[1]).max()) if n else 0
        if packed[3] is not None and n:
            longest += int(np.diff(packed[3].astype(np.int64)).max(initial=0))
        guess = min(n * max(longest + 8, min(int(opts.pad_to), 1 << 20)), 1 << 26) + 64  # (else: fetch)
        arrs, _, row_len, width = self._run(packed, opts, guess)
        names = ("input_ids", "attention_mask", "token_type_ids", "special_tokens_mask")
        out = {k: a.reshape(n, width) for k, a in zip(names, arrs)}
        out["row_len"] = row_len
        return out

    def process_packed_device(self, ids_ptr, off_ptr, n_rows, n_ids, out_ptr, out_cap, out_off_ptr, pair_ids_ptr=0, pair_off_ptr=0,
                              has_pair_ptr=0, n_pair_ids=0, truncate_to=None, strategy="longest_first", stream=0):
        """process_packed over raw device pointers (ints; e.g. torch tensors' data_ptr()) of this
        post-processor's device, ordered on the HIP stream `stream` (0: the default stream); n_ids =
        off[n_rows], n_pair_ids = pair_off[n_rows].  out_ptr has room for out_cap uint32, out_off_ptr for
        n_rows + 1 uint64; ids must be 4-byte and offsets 8-byte aligned.  Returns the number of ids;
        raises BufferError carrying `.needed_ids` when the capacity is too small, with nothing written --
        fetch_packed() then returns the result without a second run.  Returns after the work is done;
        extension."""
        if strategy not in _STRATEGIES:
            raise ValueError("strategy must be 'only_first', 'only_second' or 'longest_first'")
        opts = _n.PpOpts()
        if truncate_to is not None:
            opts.truncate, opts.truncate_to = 1, _uint("truncate_to", truncate_to, _USIZE)
        opts.strategy = _STRATEGIES[strategy]
        b = _n.PpBatch(ids_ptr or None, off_ptr or None, pair_ids_ptr or None, pair_off_ptr or None, has_pair_ptr or None, n_rows)
        n = ctypes.c_uint64()
        self._fetch_rows = None
        rc = _n.lib.ctok_postprocessor_run_device(self._h, ctypes.byref(b), n_ids, n_pair_ids, ctypes.byref(opts), out_ptr or None,
                                                  out_cap, out_off_ptr or None, ctypes.byref(n), stream or None)
        if rc == _n.CTOK_E_CAPACITY and n.value > out_cap:
            self._fetch_rows = (n_rows, int(n.value))
            e = BufferError("process_packed_device: the result needs %d ids, the capacity is %d" % (n.value, out_cap))
            e.needed_ids = int(n.value)
            raise e
        if rc:
            _raise(rc)
        self._read_stats()
        return int(n.value)

    def fetch_packed(self):
        """(uint32 ids, uint64 off) of the process_packed_device call that raised BufferError, which the
        library kept on the device; extension."""
        if getattr(self, "_fetch_rows", None) is None:
            raise ValueError("fetch_packed: no result to fetch")
        n_rows, n = self._fetch_rows
        ids = np.empty(n, dtype=np.uint32)
        off = np.zeros(n_rows + 1, dtype=np.uint64)
        o = _n.PpOut(ids.ctypes.data, n, off.ctypes.data, None, None, None, None, 0, 0)
        rc = _n.lib.ctok_postprocessor_fetch(self._h, ctypes.byref(o))
        if rc:
            _raise(rc)
        return ids, off

    def _read_stats(self):
        info = _n.PpInfo()
        n = ctypes.c_uint64()
        _n.lib.ctok_postprocessor_stats(self._h, ctypes.byref(info))
        _n.lib.ctok_postprocessor_stage_ms(self._h, None, 0, ctypes.byref(n))
        ms = (ctypes.c_double * max(int(n.value), 1))()
        _n.lib.ctok_postprocessor_stage_ms(self._h, ms, int(n.value), ctypes.byref(n))
        self.last_stats = {k: int(getattr(info, k)) for k, _ in info._fields_}
        self.last_stats["stages"] = [(_n.lib.ctok_postprocessor_stage_name(self._h, i).decode(), ms[i]) for i in range(int(n.value))]
