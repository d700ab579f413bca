#!/usr/bin/env python3
"""The reference's find_most_likely_depth (src/genotype.cpp:1136-1158) over its whole domain, recorded: oracle/_ref/ref_harness (the
unmodified reference + oracle/ref_harness.cpp) `depthrule` calls GENOTYPE::find_most_likely_depth for every h 0..8, c 0..255 and f 1..255
at each average and interval of tests/depth_rule_cases.py's CASES -- the interval GENOTYPE::calculate_poisson_interval's own unless the
case names one.  Writes depth_rule.npz: names, ave_bits (the float's bits), lower, upper (the doubles the harness used) and tables
(cases, 9, 256, 255) uint8 [h, c, f - 1], every f.  Run in the build container after `make -C oracle ref`."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
HARNESS = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "ref_harness")

from depth_rule_cases import CASES, H_MAX, N_C, N_F      # noqa: E402


def _bits64(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def main():
    names, ave_bits, lower, upper, tables = [], [], [], [], []
    with tempfile.TemporaryDirectory() as work:
        out = os.path.join(work, "table.bin")
        for name, ave, interval in CASES:
            bits = int(np.float32(ave).view(np.uint32))
            args = [HARNESS, "depthrule", f"{bits:08x}", out]
            if interval is not None:
                args += [f"{_bits64(interval[0]):016x}", f"{_bits64(interval[1]):016x}"]
            said = dict(ln.split() for ln in subprocess.run(args, check=True, capture_output=True, text=True).stdout.splitlines())
            assert int(said["ave_bits"], 16) == bits
            lo, up = (struct.unpack("<d", struct.pack("<Q", int(said[k], 16)))[0] for k in ("lower_bits", "upper_bits"))
            assert interval is None or (lo, up) == tuple(interval)
            t = np.fromfile(out, dtype=np.uint8)
            assert t.size == (H_MAX + 1) * N_C * N_F
            names.append(name)
            ave_bits.append(bits)
            lower.append(lo)
            upper.append(up)
            tables.append(t.reshape(H_MAX + 1, N_C, N_F))
            print(name, f"{bits:08x}", lo, up)
    path = os.path.join(HERE, "depth_rule.npz")
    np.savez_compressed(path, names=np.array(names), ave_bits=np.array(ave_bits, dtype=np.uint32), lower=np.array(lower, dtype=np.float64),
                        upper=np.array(upper, dtype=np.float64), tables=np.stack(tables))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
