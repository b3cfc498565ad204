"""The stride-window arithmetic (csrc/window_hd.h: windows of a row, bounds of window k) against
values written out by hand: tools/window_check.cpp built with g++ and run.  And the parts of
ctok_encode_windows that need no device: a stride the reference would loop on forever is refused
before any device is touched, and the library exports the two calls.  No GPU."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from complexity_tokenizer import Tokenizer, pack_texts
from complexity_tokenizer import _native as _n
from tests import toys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_arithmetic(tmp_path):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "window_check.cpp")
    exe = str(tmp_path / "window_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_exports_the_window_calls():
    lib = ctypes.CDLL(_n.LIB_PATH)
    for name in ("ctok_encode_windows", "ctok_encode_windows_device"):
        assert hasattr(lib, name) and name in _n.SIGS, name
    assert _n.CTOK_P_WINDOWS == 256
    with open(os.path.join(ROOT, "include", "ctok.h")) as f:
        assert "#define CTOK_P_WINDOWS 256u" in f.read()


@pytest.fixture(scope="module")
def tok():
    return Tokenizer.from_str(json.dumps(toys.tok_json({c: i for i, c in enumerate(toys.byte_chars())}, [])))


@pytest.mark.parametrize("max_length,stride", [(4, 4), (4, 5), (1, 1), (0, 0), (0, 3), (512, 2 ** 40)])
def test_stride_not_below_max_length_is_refused(tok, max_length, stride):
    """stride >= max_length (max_length 0 included) never ends in the reference: CTOK_E_ARG from
    both calls and ValueError from Python, with or without a device (an encode on a host without
    one fails with CTOK_E_DEVICE, so the check comes first)."""
    text, off = pack_texts(["aaaaaaaaaa", "b"])
    row_win = np.zeros(3, dtype=np.uint64)
    n_out, w_out = ctypes.c_uint64(), ctypes.c_uint64()
    opts = _n.PadOpts(_n.CTOK_P_ADD_SPECIAL, 0, max_length)
    rc = _n.lib.ctok_encode_windows(tok._h, text.ctypes.data, off.ctypes.data, 2, ctypes.byref(opts), stride, None, None,
                                    None, None, 0, None, None, None, 0, row_win.ctypes.data, ctypes.byref(n_out),
                                    ctypes.byref(w_out), None, None)
    assert rc == _n.CTOK_E_ARG and "stride" in _n.last_error()
    # (the device call checks its options before it looks at the buffers: no device pointer is needed)
    rc = _n.lib.ctok_encode_windows_device(tok._h, None, off.ctypes.data, 2, 0, ctypes.byref(opts), stride, None, None,
                                           None, None, 0, None, None, None, 0, row_win.ctypes.data, ctypes.byref(n_out),
                                           ctypes.byref(w_out), None, None)
    assert rc == _n.CTOK_E_ARG and "stride" in _n.last_error()
    with pytest.raises(ValueError, match="stride"):
        tok.encode_windows(["aaaaaaaaaa", "b"], max_length=max_length, stride=stride)


def test_null_arguments_are_refused(tok):
    opts = _n.PadOpts(0, 0, 4)
    n_out = ctypes.c_uint64()
    rc = _n.lib.ctok_encode_windows(tok._h, None, None, 0, ctypes.byref(opts), 1, None, None, None, None, 0, None, None,
                                    None, 0, None, ctypes.byref(n_out), ctypes.byref(n_out), None, None)
    assert rc == _n.CTOK_E_ARG
