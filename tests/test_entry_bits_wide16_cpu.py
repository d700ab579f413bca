"""The host's reading of a node-list entry from the graph's bit vectors beyond 32 bytes (csrc/host/entry_bits.hpp: eight words per mask) --
what a diploid sample over a panel of 255 to 511 haplotypes prunes and checks sequences by."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_readings_beyond_32_bytes_equal_a_literal_model(tmp_path):
    """tests/native/entry_bits_wide16_check.cpp under AddressSanitizer + UBSan, a stand-alone program: words_of over 1 to 64 bytes (8 from 33
    on), and carried_bytes / meets_bytes at 33, 40, 41, 63 and 64 bytes against a model with one bool per haplotype -- ids 255, 256 and
    8 bl - 2 in the selections, both sides of every word boundary, entries whose only set bit is the flag; entries and masks are allocated
    at their exact sizes, so a read past either is a report."""
    exe = str(tmp_path / "entry_bits_wide16_check")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-I",
                        os.path.join(ROOT, "varigraph_amd", "csrc", "host"), os.path.join(ROOT, "tests", "native", "entry_bits_wide16_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("entry readings identical"), (r.stdout[-1000:], r.stderr[-2000:])
