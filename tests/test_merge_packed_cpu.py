"""The packed merge tiers' step (csrc/merge_packed_hd.h: min-find, L / R extraction, slot move,
value update) for 16 and for 32 slots on the host against a scalar model of the register tier
(merge_slots<16>, merge_slots<32>), across the hand-offs from 32 to 16 slots and to the 8-slot
tier's keys: tools/merge_packed_check.cpp built with g++ and run.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_merge_packed_step(tmp_path):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "merge_packed_check.cpp")
    exe = str(tmp_path / "merge_packed_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", src, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
