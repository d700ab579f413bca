"""Masks over the places of a window's list turned into W-word masks over haplotype ids (csrc/host/id_masks.hpp): what a polyploid sample
over a panel of 48 to 254 haplotypes hands the device as reference-allele masks and sequence fixes, and the bound on such samples."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_place_masks_become_id_masks_as_a_literal_model_has_them(tmp_path):
    """tests/native/id_masks_check.cpp under AddressSanitizer + UBSan, a stand-alone program: places_to_ids against a model with one
    bool per haplotype at 7, 8, 9, 16, 17 and 32 bytes of haplotype bits -- lists of 1 to 64 haplotypes that hold ids 0, 63, 64, 127, 128 and
    8 bit_len - 2 where the width has them, every place, no place, places beyond the list, a second mask or-ed into the same words; the words
    are allocated at exactly W, so a write past them is a report -- and wide_ploidy_sample at both sides of each of its bounds."""
    exe = str(tmp_path / "id_masks_check")
    r = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17", "-I",
                        os.path.join(ROOT, "varigraph_amd", "csrc", "host"), os.path.join(ROOT, "tests", "native", "id_masks_check.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("id masks identical"), (r.stdout[-1000:], r.stderr[-2000:])
