"""tests/native/x80_device_check.hip, built next to varigraph_amd/csrc/vg_x80.h alone (flags of varigraph_amd/build.py): the driver of
test_x80_cases_cpu.py (--host: no HIP call) and test_gpu_x80.py (the divergent, uniform and chain kernels)."""
import json
import os
import subprocess

from varigraph_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("x80_mul", "x80_add", "x80_div", "n80_mul", "n80_add", "n80_sum", "n80_div", "n80_muladd", "n80_from_to")


def build_harness(outdir):
    exe = os.path.join(str(outdir), "x80_device_check")
    subprocess.run([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", build.CSRC,
                    os.path.join(ROOT, "tests", "native", "x80_device_check.hip"), "-o", exe], check=True, cwd=ROOT, timeout=600)
    return exe


def run_harness(exe, args, timeout=300):
    """-> (exit status, {(function, mode): the JSON object it printed}, stderr)"""
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)
    lines = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    return r.returncode, {(d["function"], d["mode"]): d for d in lines}, r.stderr
