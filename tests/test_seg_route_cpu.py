"""k_segment's mask gathers and slot-front functions on the host (CPU only):
complexity-tokenizer_amd/tools/seg_route_check.cpp, a stand-alone program, compares the
dot-product pack8 with the multiply form it replaced and the word-domain doc-start bits with the
per-piece definition.
Built and run plain and under -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "seg_route_check.cpp")
PARTS = ["pack8 ok", "doc bits ok", "all ok"]


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_seg_route_check(tmp_path, flags):
    exe = str(tmp_path / "seg_route_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for part in PARTS:
        assert part in r.stdout, r.stdout
