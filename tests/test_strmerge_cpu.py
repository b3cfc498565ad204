"""The host side of the string-keyed merge engine checked on the CPU: csrc/strmerge_compile.cpp
(interning, the foreign symbol, the pair table, the id map) and the merge loop of
csrc/strmerge_hd.h that the kernels share, by tools/strmerge_check.cpp, built with g++ and run.
Where the shared library loads, the create calls of include/ctok_models.h either succeed or
report that there is no device.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_strmerge_check(tmp_path):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "strmerge_check.cpp")
    exe = str(tmp_path / "strmerge_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def _create(n, vocab, merges=(), *args):
    keys = [k.encode() for k in vocab]
    blob = np.frombuffer(b"".join(keys) + b"\0" * 16, dtype=np.uint8)
    off = np.zeros(len(keys) + 1, dtype=np.uint64)
    np.cumsum([len(k) for k in keys], out=off[1:])
    ids = np.asarray(list(vocab.values()) + [0], dtype=np.uint32)
    h = ctypes.c_void_p()
    if n.__name__ == "ctok_wl_model_create":
        return n(blob.ctypes.data, off.ctypes.data, ids.ctypes.data, len(keys), *args, ctypes.byref(h)), h
    ms = [m.encode() for m in merges]
    mblob = np.frombuffer(b"".join(ms) + b"\0" * 16, dtype=np.uint8)
    moff = np.zeros(len(ms) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in ms], out=moff[1:])
    return n(blob.ctypes.data, off.ctypes.data, ids.ctypes.data, len(keys), mblob.ctypes.data, moff.ctypes.data, len(ms),
             *args, ctypes.byref(h)), h


def test_create_without_a_device_reports_it():
    from complexity_tokenizer import _native as _n
    lib = _n.lib
    vocab = {"<unk>": 0, "a": 1, "b": 2}
    calls = [(lib.ctok_wl_model_create, lib.ctok_wl_model_destroy, (), (b"<unk>", 0)),
             (lib.ctok_cbpe_model_create, lib.ctok_cbpe_model_destroy, ("a", "b"), (b"</w>", b"<unk>", 0)),
             (lib.ctok_blbpe_model_create, lib.ctok_blbpe_model_destroy, ("a", "b"), (b"<unk>", 1, 0))]
    for create, destroy, merges, args in calls:
        rc, h = _create(create, vocab, merges, *args)
        assert rc in (_n.CTOK_OK, _n.CTOK_E_DEVICE), _n.last_error()
        if rc == _n.CTOK_OK:
            destroy(h)
        else:
            assert not h.value and _n.last_error()
    # an odd merge array is an argument error before any device is touched
    rc, h = _create(lib.ctok_cbpe_model_create, vocab, ("a", "b", "c"), b"</w>", b"<unk>", 0)
    assert rc == _n.CTOK_E_ARG and "odd" in _n.last_error()
    t1, t2, cap = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    lib.ctok_models_limits(ctypes.byref(t1), ctypes.byref(t2), ctypes.byref(cap))
    assert 0 < t1.value < t2.value < cap.value
