"""The operands of tests/native/x80_cases.h reach what they claim to reach, shown without a GPU: x80_device_check --host sends every
case through the host pass's compile of csrc/vg_x80.h, compares with the x87 unit, and counts per function how many cases fell into each
class of rounding, operand and alignment (counted from the operands and the x87 results, not with vg_x80.h).  Every class a function can
reach has cases; test_gpu_x80.py sends the same cases through the device's compile."""
import pytest

import x80_harness as xh


@pytest.fixture(scope="module")
def host_lines(tmp_path_factory):
    exe = xh.build_harness(tmp_path_factory.mktemp("x80_device_check"))
    status, lines, err = xh.run_harness(exe, ["--host"])
    assert status == 0, (status, err[-2000:])
    return lines


@pytest.mark.parametrize("function", xh.FUNCTIONS + ("chains",))
def test_host_pass_equals_x87_and_every_class_has_cases(host_lines, function):
    d = host_lines[(function, "host")]
    assert d["mismatches"] == 0, d["first"]
    assert d["cases"] > 0
    empty = [name for name, count in d["classes"].items() if count <= 0]
    assert not empty, empty
    if function != "chains":
        assert len(d["classes"]) >= 3
    if not function.endswith("div"):
        assert d["skipped"] == 0        # only a division by zero or a quotient that overflows is no case


def test_the_functions_of_one_operation_saw_the_same_cases(host_lines):
    for group in (("x80_mul", "n80_mul"), ("x80_add", "n80_add", "n80_sum"), ("x80_div", "n80_div")):
        first = host_lines[(group[0], "host")]
        for other in group[1:]:
            assert host_lines[(other, "host")]["classes"] == first["classes"] and host_lines[(other, "host")]["cases"] == first["cases"]
