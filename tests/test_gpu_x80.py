"""csrc/vg_x80.h as the device compiles and runs it (tests/native/x80_device_check.hip) against the x87 unit of the host, on the cases of
tests/native/x80_cases.h: one case per lane (fast-path and fallback lanes side by side in a wavefront), one case per wavefront (the
operands uniform, all 64 lanes' results checked), and 120-term chains  r += s * o  one per lane.  The cases are seeded: the class counts
of every device mode are those of the host mode (tests/test_x80_cases_cpu.py holds each of them above zero)."""
import pytest

import x80_harness as xh

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = xh.build_harness(tmp_path_factory.mktemp("x80_device_check"))
    status, lines, err = xh.run_harness(exe, ["--host", "--divergent", "--uniform", "--chains"])
    assert status in (0, 1), (status, err[-2000:])      # 1: mismatches, which the tests below report by function; 2: a HIP error
    return lines


@pytest.mark.parametrize("mode", ["divergent", "uniform"])
@pytest.mark.parametrize("function", xh.FUNCTIONS)
def test_device_equals_x87(lines, function, mode):
    d, host = lines[(function, mode)], lines[(function, "host")]
    assert d["mismatches"] == 0, d["first"]
    assert d["cases"] == host["cases"] > 0 and d["skipped"] == host["skipped"]
    assert d["classes"] == host["classes"] and all(count > 0 for count in d["classes"].values())


def test_chains_on_the_device_equal_x87(lines):
    d = lines[("chains", "chains")]
    assert d["mismatches"] == 0, d["first"]
    assert d["cases"] == lines[("chains", "host")]["cases"] > 0 and lines[("chains", "host")]["mismatches"] == 0
