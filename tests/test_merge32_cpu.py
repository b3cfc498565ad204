"""The packed 32-slot merge tier's step (csrc/merge32_hd.h) on the host against a scalar model of
the register tier (merge_slots<32>), across the hand-offs to the packed 16-slot step and to the
8-slot tier's keys: tools/merge32_check.cpp built with g++ and run.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merge32_packed_step(tmp_path):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "merge32_check.cpp")
    exe = str(tmp_path / "merge32_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
