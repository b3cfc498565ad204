"""The packed 16-slot merge tier's step (csrc/merge16_hd.h: min-find, L / R extraction, slot move,
value update, hand-off encoding) on the host against a scalar model of the register tier:
tools/merge16_check.cpp built with g++ and run.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merge16_packed_step(tmp_path):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "merge16_check.cpp")
    exe = str(tmp_path / "merge16_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
