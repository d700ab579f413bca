"""bench.py's bookkeeping and the bench-only library, without a GPU (round 6).

* `measured_traffic`: a committed counter profile is reported as `roofline.traffic` only for the code it was measured on (sha256 of the
  library or of its sources), the kernel named and a launch of the same size -- VERDICT r5 "weak" #5 found constants of earlier builds there.
* libvgsynth.so (csrc/bench/vgsynth.h): the synthetic workloads have a library of their own; the product ABI no longer exports them."""
import ctypes
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_traffic_is_reported_for_the_code_it_was_measured_on_only(bench, tmp_path, monkeypatch):
    from varigraph_amd import build
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    rec = {"reads_per_launch": 24_000_000, "kernel": "vgk::countkc_defer_kernel<27u>", "bytes_per_launch": 123, "libvgmi_sha256": "aa", "source_sha256": "bb"}
    (prof / "hbm_traffic_c3.json").write_text(json.dumps(rec))
    monkeypatch.setattr(build, "lib_digest", lambda: "aa")
    monkeypatch.setattr(build, "source_digest", lambda: "zz")
    assert bench.measured_traffic("c3", 24_000_000, "vgk::countkc_defer_kernel<27u>")[0] == 123          # the library's sha256 matches
    monkeypatch.setattr(build, "lib_digest", lambda: "other")
    monkeypatch.setattr(build, "source_digest", lambda: "bb")
    assert bench.measured_traffic("c3", 24_000_000, "vgk::countkc_defer_kernel<27u>")[0] == 123          # ... or the sources' does
    monkeypatch.setattr(build, "source_digest", lambda: "zz")
    assert bench.measured_traffic("c3", 24_000_000, "vgk::countkc_defer_kernel<27u>") == (None, None)    # another build
    monkeypatch.setattr(build, "lib_digest", lambda: "aa")
    assert bench.measured_traffic("c3", 24_000_000, "vgk::count27c_kernel") == (None, None)              # another kernel
    assert bench.measured_traffic("c3", 12_000_000, "vgk::countkc_defer_kernel<27u>") == (None, None)    # another launch
    assert bench.measured_traffic("c5", 24_000_000, None) == (None, None)                                 # no file
    (prof / "hbm_traffic.json").write_text(json.dumps(dict(rec, kernel="vgk::count27s_kernel<true, 27u>", reads_per_launch=100_000_000)))
    assert bench.measured_traffic("c2", 100_000_000, "vgk::count27s_kernel<true, 27u>")[0] == 123


def test_source_digest_names_the_sources_of_the_library():
    from varigraph_amd import build
    a, b = build.source_digest(), build.source_digest()
    assert a == b and len(a) == 64
    assert all(os.path.exists(os.path.join(build.CSRC, f)) for f in build.VGMI_SOURCES)
    assert {"vgmi_api.cpp", "vgmi_api_table.cpp", "vgmi_api_rccl.cpp", "vgmi_api_fastq.cpp", "vgmi_api_bloom.cpp", "vgmi_api_hmm.cpp", "vgmi_ctdefer.hip"} <= set(build.VGMI_SOURCES)


def test_synthetic_workloads_have_a_library_of_their_own():
    from varigraph_amd import build, synthlib, vgmi
    build.build_synth()
    lib = ctypes.CDLL(synthlib.LIB_PATH)
    for name in ("vgs_reads_device", "vgs_reads_host", "vgs_reference_host", "vgs_snp_keys_host"):
        assert hasattr(lib, name)
    product = ctypes.CDLL(vgmi.LIB_PATH)
    for name in ("vgmi_synth_reads_device", "vgmi_synth_reads_host", "vgmi_synth_reference_host", "vgmi_synth_snp_keys_host", "vgs_reads_host"):
        with pytest.raises(AttributeError):
            getattr(product, name)
    assert "synth" not in open(os.path.join(ROOT, "include", "vgmi.h")).read().replace("libvgsynth", "").replace("vgsynth.h", "").replace("synthetic", "")
    # the generator is a pure function of (seed, read, base): any piece of a block equals the same reads drawn alone
    ref = synthlib.reference(7, 5000)
    whole = synthlib.reads_host(3, 0, 64, 150, [ref, ref[::-1].copy()])
    part = synthlib.reads_host(3, 20, 10, 150, [ref, ref[::-1].copy()])
    assert np.array_equal(whole[20 * 151:30 * 151], part) and set(np.unique(whole)) <= set(b"ACGTN\n")
    with pytest.raises(RuntimeError):
        synthlib.reads_host(3, 0, 4, 150, [ref[:100]])          # a haplotype shorter than the insert


@pytest.mark.parametrize("which,n,rx,summary", [("c3", 24_000_000, "count27|countkc|ctd_", "r6_c3_rocprofv3_summary.txt"), ("c5", 100_000_000, "count27|countkc|ctd_", "r6_c5_rocprofv3_summary.txt"),
                                               ("c2", 100_000_000, "count27|countkc|ctd_", "r6_rocprofv3_summary.txt"), ("bloom", 59_999_974, "bb_|rows_kernel", "r6_bloom_rocprofv3_summary.txt")])
def test_committed_traffic_files_follow_from_the_committed_rocprofv3_summaries(which, n, rx, summary, tmp_path):
    """profiles/hbm_traffic*.json are what tools/make_traffic_json_r6.py makes of the round's committed rocprofv3 summaries (kernel table + FETCH_SIZE /
    WRITE_SIZE / request counters per kernel of the count pass): every figure of `roofline.traffic` can be recomputed from profiles/ alone."""
    import shutil
    import subprocess
    name = {"c2": "hbm_traffic.json"}.get(which, f"hbm_traffic_{which}.json")
    want = json.load(open(os.path.join(ROOT, "profiles", name)))
    shutil.copy(os.path.join(ROOT, "profiles", summary), tmp_path / "summary.txt")
    (tmp_path / "libvgmi.sha256").write_text(want["libvgmi_sha256"] + "\n")
    (tmp_path / "source.sha256").write_text((want.get("source_sha256") or "") + "\n")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_traffic_json_r6.py"), which, str(n), str(tmp_path), rx], check=True, capture_output=True)
    got = json.load(open(tmp_path / "traffic.json"))
    for key in ("reads_per_launch", "kernel", "bytes_per_launch", "breakdown_bytes", "kernel_table", "count_pass_us_per_launch_rocprofv3", "libvgmi_sha256"):
        assert got[key] == want[key], key
    # ... and the pass the profile timed is the pass the committed bench line timed (same library; another box: within a fifth)
    line = json.loads(open(os.path.join(ROOT, "profiles", "r6_bench_n1.json")).read())
    assert line["library"]["libvgmi_sha256"] == want["libvgmi_sha256"]
    live_ms = {"c2": line["roofline"]["kernel_ms"], "c3": line["c3"]["roofline"]["kernel_ms"], "c5": line["c5"]["roofline"]["kernel_ms"], "bloom": line["bloom"]["add_seconds"] * 1e3}[which]
    assert abs(want["count_pass_us_per_launch_rocprofv3"] / 1e3 - live_ms) / live_ms < 0.2, (want["count_pass_us_per_launch_rocprofv3"], live_ms)
    traffic = {"c2": line["roofline"]["traffic"], "c3": line["c3"]["roofline"]["traffic"], "c5": line["c5"]["roofline"]["traffic"], "bloom": line["bloom"]["roofline"]["traffic"]}[which]
    assert traffic == want["bytes_per_launch"]


def test_dump_outputs_writes_exact_float64_arrays_within_the_limit(bench, tmp_path, monkeypatch):
    """--dump-outputs: every array the timed path hands back, as <name>.npy in float64, values unchanged; more than the limit is refused."""
    import torch
    cov = torch.tensor([0, 1, 255, 7], dtype=torch.uint8)
    hist = torch.tensor([3, 0, 2 ** 40], dtype=torch.int64)
    bench.dump_outputs(str(tmp_path / "out"), {"cov": cov, "hist": hist})
    assert sorted(os.listdir(tmp_path / "out")) == ["cov.npy", "hist.npy"]
    got = np.load(tmp_path / "out" / "cov.npy")
    assert got.dtype == np.float64 and np.array_equal(got, cov.numpy().astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "out" / "hist.npy"), hist.numpy().astype(np.float64))
    bench.dump_outputs(str(tmp_path / "out"), {"cov": cov}, "_rank1")
    assert (tmp_path / "out" / "cov_rank1.npy").exists()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 8 * 4 - 1)
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "big"), {"cov": cov})
    assert not (tmp_path / "big").exists()
