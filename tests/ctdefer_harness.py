"""tests/native/ctdefer_check.hip, built next to varigraph_amd/csrc/vgmi_ctdefer.hip alone (flags of varigraph_amd/build.py): the
driver of test_ctdefer_cpu.py (geometry, no HIP call) and test_gpu_ctdefer.py (the scatter and accumulate kernels on seeded records)."""
import json
import os
import subprocess

from varigraph_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("VGMI_CT_DEFER", "VGMI_CT_DEFER_MIN", "VGMI_CT_DEFER_CAP", "VGMI_CT_DEFER_ROOM")


def build_harness(outdir):
    exe = os.path.join(str(outdir), "ctdefer_check")
    subprocess.run([build._hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", build.CSRC,
                    os.path.join(ROOT, "tests", "native", "ctdefer_check.hip"), os.path.join(build.CSRC, "vgmi_ctdefer.hip"), "-o", exe],
                   check=True, cwd=ROOT, timeout=600)
    return exe


def run_harness(exe, args, env=None, timeout=300):
    """-> (exit status, the JSON objects it printed, stderr); the deferral knobs of the caller's environment do not reach it"""
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env or {})
    r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, env=e, timeout=timeout)
    return r.returncode, [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")], r.stderr
