"""An encode call's numeric decisions (csrc/call_plan.h: list capacities, the pass plan from
k_segment's report, the outcome from the final counters) against values written out by hand:
tools/call_plan_check.cpp built with g++ and run.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_call_plan(tmp_path):
    src = os.path.join(ROOT, "complexity-tokenizer_amd", "tools", "call_plan_check.cpp")
    exe = str(tmp_path / "call_plan_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", src, "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
