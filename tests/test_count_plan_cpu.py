"""The count plan (csrc/vgmi_count_plan.h: which launches count a read block and where the fast kernel's rows end) against a plain
model of the four decision trees launch_count used to hold."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_count_plan_equals_the_model_of_the_four_decision_trees(tmp_path):
    """tests/native/count_plan_check.cpp under AddressSanitizer + UBSan, a stand-alone program: count_plan against the model over every
    combination of a context's flags that adopt_image can produce, odd and even k, the block's length on the host and on the device, and
    block sizes on both sides of every row boundary up to 2^32 + 5; vg_row_split against the rows' coverage lane by lane (emit_from is
    the first end the rows do not cover and never lies behind the block); the host's split against the one the kernels derive."""
    exe = str(tmp_path / "count_plan_check")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-Wall", "-I",
                        os.path.join(ROOT, "varigraph_amd", "csrc"), os.path.join(ROOT, "tests", "native", "count_plan_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("count plan identical to the model"), (r.stdout[-1000:], r.stderr[-2000:])
