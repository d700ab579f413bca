"""The command line over cohorts of 130, 160 and 255 diploid samples -- 261, 321 and 511 haplotypes, 33, 41 and 64 bytes of haplotype bits per
entry, eight words on the device -- against the deterministic build of the reference, byte for byte, with the log saying which path ran;
and what stays out (65 bytes, -n above 16, a polyploid sample) keeping the pool.  The generator is test_gpu_hmm_wide's: 150 kb, 250 sites,
seed 4, indel_frac 0.1, 25 000 read pairs per sample with read seeds 8 + i, --granularity 0.04, -t 6."""
import re
import shutil

import pytest

from test_gpu_hmm_wide import BITS, SELECTED, _cohort, _genotype

pytestmark = pytest.mark.gpu
GRAN = ["--granularity", "0.04"]      # windows of 40 kb: four of them


@pytest.fixture(scope="module")
def cohort130(tmp_path_factory):
    """130 diploid samples: 261 haplotypes, 33 bytes.  Four sites in ten are insertions of 60..300 bp (`--sv` needs them); reads of samples 3,
    7 and 129 -- the last one's own haplotypes have ids above 255, beyond what a byte holds."""
    work = str(tmp_path_factory.mktemp("wide16_cli"))
    graph, cfg = _cohort(work, 130, (3, 7, 129), 0.4)
    yield work, graph, cfg
    shutil.rmtree(work, ignore_errors=True)


CASES = {"n15": (["-n", "15"], 1), "n16": (["-n", "16"], 1), "n16_hom": (["-n", "16", "-g", "hom"], 1), "n5_depth_3_samples": (["-n", "5", "--use-depth"], 3),
         "n5_sv": (["-n", "5", "--sv"], 1), "n5_hom": (["-n", "5", "-g", "hom"], 1), "fre_n5": (["-m", "fre", "-n", "5"], 1)}
# -n 16 with pairs of any two haplotypes is 136 genotypes, more than the 128 the emission kernel has lanes for: the pool, as at any width
ON_THE_POOL = {"n16"}


@pytest.mark.parametrize("case", sorted(CASES))
def test_command_line_over_261_haplotypes_on_the_selected_path_equals_the_reference(case, cohort130):
    """`varigraph-mi genotype` over the 261-haplotype graph, byte for byte the deterministic reference build's VCFs: -n 15; -n 16; -n 16 -g hom;
    -n 5 --use-depth with three samples in one run (the pruned lists carry over); -n 5 --sv; -n 5 -g hom; -m fre -n 5 -- each also with VGH_HMM_WIDE_DEVICE=0 (the pool), VGH_HMM_SELECT_DEVICE=0, VGH_DEVICE_TALLIES=0, VGH_HMM_FIX_DEVICE=0
    (flagged rows scored by the host's hidden_states, which reads the bit vectors) and VGH_HMM_FAKE_NOMEM=1 (the first sample takes the
    pool, the next ones start from the host's lists).  The default run's log carries the selected-path line for every window of every
    sample and the `haplotype bits on the device: 33 bytes` line once; with either of the first two knobs it carries neither.
    -n 16 is the exception in the log, not in the VCFs: a window's 16 haplotypes make 136 pairs, the emission kernel has 128 lanes (and the
    C ABI refuses n_gt 129), so under every knob the sample takes the pool and neither line appears -- what this asserts for it.  The 16
    places of a window's list (gt0 and the fixes use all 16 bits) go through the selected path with -n 16 -g hom: 16 genotypes.
    Reference VCF lines, counted on the CPU with the host twin of the read generator: -n 15: 189; -n 16: 189; -n 5 --use-depth: 189, 210,
    201; -n 5 --sv: 88; -n 5 -g hom: 152; -m fre -n 5: 189 (at least 50 each: the comparison must not be of empty files)."""
    from test_gpu_configs import CLI, ENV, REF
    work, graph, cfg = cohort130
    opts, n = CASES[case]
    opts = opts + GRAN
    timing = dict(ENV, VGH_TIMING="1")
    want, _ = _genotype(work, graph, cfg[:n], f"{case}_cpu", REF, opts, ENV)
    lines = [v.count(b"\n") for v in want]
    print(f"{case}: reference VCF lines {lines}")
    assert min(lines) >= 50, lines
    logs = {}
    for name, env in (("native", timing), ("pool", dict(timing, VGH_HMM_WIDE_DEVICE="0")), ("host_select", dict(timing, VGH_HMM_SELECT_DEVICE="0")),
                      ("host_tallies", dict(timing, VGH_DEVICE_TALLIES="0")), ("host_fixes", dict(timing, VGH_HMM_FIX_DEVICE="0")),
                      ("fake_nomem", dict(timing, VGH_HMM_FAKE_NOMEM="1"))):
        got, logs[name] = _genotype(work, graph, cfg[:n], f"{case}_{name}", CLI, opts, env)
        for i in range(n):
            assert got[i] == want[i], (case, name, i)
    if case in ON_THE_POOL:
        for name, log in logs.items():
            assert not re.search(SELECTED, log) and not re.search(BITS, log), name
        return
    for name in ("native", "host_tallies", "host_fixes"):
        seen = re.findall(SELECTED, logs[name])
        assert len(seen) == n and all(a == b and int(b) >= 4 for a, b in seen), (name, seen)
        assert re.findall(BITS, logs[name]) == ["33"], name
    for name in ("pool", "host_select"):
        assert not re.search(SELECTED, logs[name]) and not re.search(BITS, logs[name]), name
    # as if the device had no room for the first sample: it takes the pool, the others the selected path on the host's lists
    assert len(re.findall(SELECTED, logs["fake_nomem"])) == n - 1 and len(re.findall(BITS, logs["fake_nomem"])) == min(1, n - 1)


@pytest.mark.parametrize("n_samples,whos,bit_len", [(160, (3, 159), 41), (255, (3,), 64)], ids=["321_haplotypes", "511_haplotypes"])
def test_command_line_over_wider_cohorts_equals_the_reference(n_samples, whos, bit_len, tmp_path_factory):
    """160 diploid samples -- 321 haplotypes, 41 bytes: the first byte of the sixth word -- with reads of samples 3 and 159 in one run, and 255
    samples -- 511 haplotypes, 64 bytes, the flag at bit 511 -- with reads of sample 3; -n 5 --use-depth: the reference's VCFs byte for byte
    (200 and 196 lines; 213 lines when counted on the CPU), the selected path for every window of every sample, the entries' width once."""
    from test_gpu_configs import CLI, ENV, REF
    work = str(tmp_path_factory.mktemp(f"wide16_cli_{n_samples}"))
    try:
        graph, cfg = _cohort(work, n_samples, whos, 0.01)
        opts = ["-n", "5", "--use-depth"] + GRAN
        want, _ = _genotype(work, graph, cfg, "cpu", REF, opts, ENV)
        lines = [v.count(b"\n") for v in want]
        print(f"{n_samples} samples: reference VCF lines {lines}")
        assert min(lines) >= 50, lines
        got, log = _genotype(work, graph, cfg, "native", CLI, opts, dict(ENV, VGH_TIMING="1"))
        for i in range(len(cfg)):
            assert got[i] == want[i], i
        seen = re.findall(SELECTED, log)
        assert len(seen) == len(cfg) and all(a == b and int(b) >= 4 for a, b in seen), seen
        assert re.findall(BITS, log) == [str(bit_len)]
    finally:
        shutil.rmtree(work, ignore_errors=True)


def _keeps_the_pool(work, graph, cfg, tag, opts, env):
    from test_gpu_configs import CLI, ENV, REF
    want, _ = _genotype(work, graph, cfg, tag + "_cpu", REF, opts + GRAN, ENV)
    lines = want[0].count(b"\n")
    print(f"{tag}: reference VCF lines {lines}")
    assert lines >= 50, lines
    got, log = _genotype(work, graph, cfg, tag, CLI, opts + GRAN, dict(ENV, VGH_TIMING="1", **env))
    assert got[0] == want[0], tag
    assert not re.search(SELECTED, log) and not re.search(BITS, log), tag
    assert "HMM thread-seconds: selection" in log and "host thread-seconds around the device" not in log, tag


def test_65_bytes_of_haplotype_bits_keep_the_pool(tmp_path_factory):
    """256 diploid samples -- 513 haplotypes, 65 bytes, one more than eight words hold -- with -n 5 --use-depth: the pool, as before; no
    selected-path line, no haplotype bits on the device, the reference's VCF byte for byte (193 lines when counted on the CPU)."""
    work = str(tmp_path_factory.mktemp("wide16_cli_256"))
    try:
        graph, cfg = _cohort(work, 256, (3,), 0.01)
        _keeps_the_pool(work, graph, cfg, "pool_65_bytes", ["-n", "5", "--use-depth"], {})
    finally:
        shutil.rmtree(work, ignore_errors=True)


@pytest.mark.parametrize("opts,env", [(["-n", "28"], {}), (["--sample-ploidy", "4", "-n", "5"], {"VGH_HMM_WIDE_PLOIDY_DEVICE": "1"})], ids=["n28", "tetraploid_n5"])
def test_what_stays_out_of_scope_over_261_haplotypes_keeps_the_pool(opts, env, cohort130):
    """-n above 16, and a polyploid sample even when VGH_HMM_WIDE_PLOIDY_DEVICE=1 asks (that opt-in ends at 32 bytes), keep the pool over the
    33-byte graph: no selected-path line, no haplotype bits on the device, the reference's VCF byte for byte."""
    work, graph, cfg = cohort130
    _keeps_the_pool(work, graph, cfg[:1], "pool_" + "_".join(o.strip("-") for o in opts), opts, env)
