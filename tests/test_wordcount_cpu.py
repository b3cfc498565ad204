"""The word-counting kernels' pure functions (csrc/wordcount_hd.h: slot descriptor pack / unpack,
length clipping, hash, byte compare) on the host: tools/wordcount_check.cpp built with g++ and run.
No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wordcount_pure_functions(tmp_path):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "wordcount_check.cpp")
    exe = str(tmp_path / "wordcount_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
