"""The host+device headers of the classic BPE trainer checked on the CPU: csrc/ws_split_hd.h (the
White_Space split behind k_ws_bits) against a split on the explicit 25-code-point set, and
csrc/pair_best_hd.h (the order k_pair_best picks by) against hand-written cases.  The checks are
tools/ws_split_check.cpp and tools/pair_best_check.cpp, built with g++ and run.  No GPU."""
import os
import subprocess

import pytest

from tests import bpe_trainer_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("tool", ["ws_split_check", "pair_best_check"])
def test_header_check(tmp_path, tool):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", tool + ".cpp")
    exe = str(tmp_path / tool)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_the_25_code_points_are_rusts_white_space():
    """The check and the restatement split on one set: the 25 code points tests/test_unicode_tables.py
    pins as Rust's White_Space, which is the `regex` module's \\s where that module is present."""
    import re
    with open(os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "ws_split_check.cpp")) as f:
        src = f.read()
    body = re.search(r"kWs\[25\] = \{([^}]*)\}", src).group(1)
    assert {chr(int(x, 16)) for x in re.findall(r"0x([0-9A-Fa-f]+)", body)} == bpe_trainer_ref.WHITE_SPACE
    rust_ws = [0x9, 0xA, 0xB, 0xC, 0xD, 0x20, 0x85, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) + \
              [0x2028, 0x2029, 0x202F, 0x205F, 0x3000]
    assert sorted(map(ord, bpe_trainer_ref.WHITE_SPACE)) == rust_ws
    # not Python's str.split(): U+001C-001F split there and not here; U+200B splits nowhere
    assert "a\x1cb".split() == ["a", "b"] and bpe_trainer_ref.split_whitespace("a\x1cb") == ["a\x1cb"]
    assert bpe_trainer_ref.split_whitespace("a\u200bb") == ["a\u200bb"]
    assert bpe_trainer_ref.split_whitespace(" a\u3000b\u0085 ") == ["a", "b"]
    assert bpe_trainer_ref.split_whitespace("") == [] and bpe_trainer_ref.split_whitespace(" \n") == []
