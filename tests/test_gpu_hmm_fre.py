"""The HMM under `-m fre` on the device: transitions by haplotype frequency (src/genotype.cpp:1196-1215, 1297-1316).  Both transition
probabilities are zero there and a term of a node's sum is  (prev_p * obs_g) * score[hap_g[0]] * ... * score[hap_g[ploidy - 1]]  in x87
`long double`, the scores being the window's normalised gamma draws (doubles).  hmm_recursion_fre_kernel (vgmi_hmm.hip) against that loop in
numpy.longdouble, bit for bit; vgmi_hmm_part_calls_fre through an emission part against the posterior in numpy.longdouble; the refusals."""
import itertools
import re

import numpy as np
import pytest

from varigraph_amd import vgmi

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _model_chain(freq, obs_rows, restart, uniform):
    """freq: (n, ploidy) longdouble.  All genotypes at once, the previous entries in their order, the factors in haplotype order."""
    n, ploidy = freq.shape
    out = np.zeros((len(obs_rows), n), dtype=LD)
    prev = None
    for s, o in enumerate(obs_rows):
        if restart[s] or prev is None:
            r = LD(0) + o
        else:
            r = np.zeros(n, dtype=LD)
            for p in range(n):
                t = prev[p] * o
                for q in range(ploidy):
                    t = t * freq[:, q]
                r = r + t
        total = LD(0)
        for g in range(n):
            total = total + r[g]
        out[s] = r / total if total > 0 else uniform
        prev = out[s]
    return out


def _tables(rng, n_hap, genotypes):
    """Three tables of factors, (3, n_gt, ploidy) longdouble from doubles: normalised gamma draws; the same with one haplotype without
    support (score exactly 0.0); one haplotype at 1e-300 and one at 0.0 -- products that are subnormal or zero, and with few enough
    haplotypes a node whose every genotype is zero."""
    draws = rng.gamma(rng.integers(1, 400, size=n_hap).astype(np.float64) + 1.0, 1.0)
    t0 = draws / draws.sum()
    t1 = t0.copy()
    t1[n_hap // 2] = 0.0
    t2 = t0.copy()
    t2[0] = 1e-300
    t2[n_hap - 1] = 0.0
    gt = np.array(genotypes)
    return np.stack([t[gt] for t in (t0, t1, t2)]).astype(LD)


def _scores(rng, n_rows, n):
    """Emission scores as test_gpu_hmm.py draws them: a few plausible genotypes, the rest far down, beyond the normal range, exact zeros."""
    expo = rng.choice([0, -20, -300, -2000, -4800, -4940, -4960], size=(n_rows, n), p=[.15, .2, .25, .2, .1, .05, .05])
    obs = (rng.random((n_rows, n)).astype(LD) + LD(0.01)) * np.power(LD(10), expo.astype(LD))
    obs[rng.random((n_rows, n)) < 0.02] = 0
    obs[7] = 0                                           # a node whose scores are all zero: the uniform fallback
    return obs


@pytest.mark.parametrize("ploidy,n_gt,waves", [(2, 120, 4), (2, 120, 2), (2, 128, 2), (2, 65, 2), (2, 15, 4), (2, 1, 4), (3, 6, 4), (4, 5, 2)])
def test_recursion_by_haplotype_frequency_equals_x87(ploidy, n_gt, waves, monkeypatch):
    """(2, 65, 2): a wavefront boundary inside the list; (2, 128, 2): every lane of both wavefronts; (2, 1, 4): three idle wavefronts."""
    monkeypatch.setenv("VGMI_HMM_WAVES", str(waves))
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    rng = np.random.default_rng(ploidy * 1000 + n_gt * 4 + waves)
    n_hap = 2
    while len(list(itertools.combinations_with_replacement(range(n_hap), ploidy))) < n_gt:
        n_hap += 1
    genotypes = list(itertools.combinations_with_replacement(range(n_hap), ploidy))[:n_gt]
    n = len(genotypes)
    assert n == n_gt
    freq = _tables(rng, n_hap, genotypes)
    n_tables, n_rows = 3, 40
    obs = _scores(rng, n_rows, n)
    steps_row, steps_restart, chains = [], [], []
    for w in range(n_tables):
        for direction in (1, -1):
            rows = list(range(n_rows))[::direction][w:]
            first = len(steps_row)
            for i, r in enumerate(rows):
                steps_row.append(r)
                steps_restart.append(1 if i == 0 or (i % 13 == 5) else 0)
            chains.append((first, len(rows), w))
    uniform = LD(1) / LD(n)
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        got = ctx.hmm_recursion_fre(freq, obs, steps_row, steps_restart, uniform, chains, ploidy)
    finally:
        ctx.close()
    n_uniform = 0
    for first, count, w in chains:
        want = _model_chain(freq[w], [obs[r] for r in steps_row[first:first + count]], steps_restart[first:first + count], uniform)
        g = got[first:first + count]
        assert np.array_equal(g, want), (ploidy, w, int(np.argmax((g != want).any(axis=1))))
        n_uniform += int((g == uniform).all(axis=1).sum())
    assert (got > 0).any() and n_uniform >= 1
    if n > 1:
        assert (got == 0).any()


def _posterior_model(a, b, gid_r, order_r):
    """posterior() of the host (src/genotype.cpp:1387-1522) in long double, as test_gpu_hmm.py models it: (prob, winner), None: no call."""
    n = a.size
    den = LD(0)
    for g in range(n):
        den = den + a[g] * b[g]
    if den == 0:
        return None
    post = (a * b) / den
    sums = {}
    for g in range(n):
        sums[gid_r[g]] = sums.get(gid_r[g], LD(0)) + post[g]
    best, best_id = LD(-1), None
    for k in order_r:
        if k == 0xFF:
            break
        if sums[k] > best:
            best, best_id = sums[k], k
    mx, win = LD(0), 0xFFFFFFFF
    for g in range(n):
        if gid_r[g] == best_id and mx < post[g]:
            mx, win = post[g], g
    return best, win


def test_part_calls_by_haplotype_frequency_equal_the_host_posterior():
    """vgmi_hmm_part_calls_fre on an emission part (15 genotypes, 20 rows): the scores never leave the device between the emission kernel and
    the recursion; prob and winner equal the posterior on alpha / beta of the model above, computed from the scores the part hands out."""
    assert np.finfo(LD).nmant == 63
    rng = np.random.default_rng(4242)
    n_hap, bit_len = 5, 2
    used = np.arange(n_hap, dtype=np.uint8)
    pairs = list(itertools.combinations_with_replacement(range(n_hap), 2))
    pos_a = np.array([a for a, _ in pairs], dtype=np.uint8)
    pos_b = np.array([b for _, b in pairs], dtype=np.uint8)
    n_gt = len(pairs)
    assert n_gt == 15
    ave = np.float32(23.5)
    lower, upper = float(ave) - 1.96 * float(np.sqrt(np.float64(ave))), float(ave) + 1.96 * float(np.sqrt(np.float64(ave)))
    tables = (rng.random(768).astype(LD) + LD(0.05)) * np.power(LD(10), rng.integers(-40, 1, size=768).astype(LD))
    n_rows = 20
    counts = rng.integers(1, 40, size=n_rows)
    entry_begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    n_entries = int(counts.sum())
    f = rng.choice([1, 1, 2, 3], size=n_entries).astype(np.uint64)
    bits = rng.integers(1, 1 << n_hap, size=n_entries).astype(np.uint64)
    bits |= rng.integers(0, 2, size=n_entries).astype(np.uint64) << np.uint64(8 * bit_len - 1)
    cov = rng.choice([0, 1, 5, 14, 15, 20, 23, 24, 30, 60], size=n_entries).astype(np.uint8)
    entries = (f << np.uint64(8)) | (bits << np.uint64(16))
    gt0 = rng.integers(0, 1 << n_hap, size=n_rows).astype(np.uint16)
    draws = rng.gamma(rng.integers(1, 400, size=n_hap).astype(np.float64) + 1.0, 1.0)
    score = draws / draws.sum()
    score[3] = 0.0                                       # a haplotype without support
    freq = score[np.array(pairs)].astype(LD)[None]
    row = np.concatenate([np.arange(n_rows), np.arange(n_rows)[::-1]]).astype(np.uint32)
    restart = np.zeros(2 * n_rows, dtype=np.uint8)
    restart[0] = restart[n_rows] = 1
    gid = rng.integers(0, 4, size=(n_rows, n_gt)).astype(np.uint8)
    order = np.full((n_rows, n_gt), 0xFF, dtype=np.uint8)
    for r in range(n_rows):
        ids = np.unique(gid[r])
        order[r, :ids.size] = rng.permutation(ids)
    fwd = np.arange(n_rows, dtype=np.uint64)
    bwd = (n_rows + (n_rows - 1 - np.arange(n_rows))).astype(np.uint64)
    uniform = LD(1) / LD(n_gt)
    calls = dict(ploidy=2, freq=freq, row=row, restart=restart, uniform=uniform, chains=[(0, n_rows, 0), (n_rows, n_rows, 0)], gid=gid, order=order,
                 fwd=fwd, bwd=bwd)
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        obs, _, _, ((prob, winner),) = ctx.hmm_emissions(entries, cov, used, pos_a, pos_b, (1 << n_hap) - 1, bit_len, ave, lower, upper, tables, entry_begin,
                                                         counts, gt0, calls=calls)
    finally:
        ctx.close()
    ab = np.concatenate([_model_chain(freq[0], [obs[r] for r in row[:n_rows]], restart[:n_rows], uniform),
                         _model_chain(freq[0], [obs[r] for r in row[n_rows:]], restart[n_rows:], uniform)])
    n_called = 0
    for r in range(n_rows):
        want = _posterior_model(ab[fwd[r]], ab[bwd[r]], gid[r], order[r])
        if want is None:
            assert winner[r] == 0xFFFFFFFF
            continue
        assert winner[r] == want[1] and prob[r] == want[0], r
        n_called += want[1] != 0xFFFFFFFF
    assert n_called > n_rows // 2


def test_refusals_leave_the_context_usable():
    """Every refusal of vgmi_hmm_recursion_fre is VGMI_E_INVALID, and the context serves a valid call after each."""
    rng = np.random.default_rng(9)
    ploidy, n_hap = 2, 4
    genotypes = list(itertools.combinations_with_replacement(range(n_hap), ploidy))
    n = len(genotypes)
    draws = rng.gamma(50.0, 1.0, size=n_hap)
    freq = (draws / draws.sum())[np.array(genotypes)].astype(LD)[None]
    n_rows = 6
    obs = (rng.random((n_rows, n)).astype(LD) + LD(0.01)) * np.power(LD(10), rng.integers(-300, 1, size=(n_rows, n)).astype(LD))
    row = list(range(n_rows))
    restart = [1] + [0] * (n_rows - 1)
    uniform = LD(1) / LD(n)
    chains = [(0, n_rows, 0)]
    want = _model_chain(freq[0], obs, restart, uniform)
    wide = np.tile(freq[:, :1], (1, 129, 1))

    def refused(**kw):
        a = dict(freq=freq, obs=obs, row=row, restart=restart, uniform=uniform, chains=chains, ploidy=ploidy)
        a.update(kw)
        with pytest.raises(vgmi.VgmiError) as e:
            ctx.hmm_recursion_fre(**a)
        assert e.value.code == vgmi.E_INVALID, kw.keys()
        assert np.array_equal(ctx.hmm_recursion_fre(freq, obs, row, restart, uniform, chains, ploidy), want)

    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        refused(ploidy=1, freq=freq[:, :, :1])
        refused(ploidy=5, freq=np.tile(freq[:, :, :1], (1, 1, 5)))
        refused(obs=np.zeros((n_rows, 129), dtype=LD), freq=wide)      # more than 128 genotypes
        refused(obs=np.zeros((n_rows, 0), dtype=LD))                   # none
        refused(n_tables=0)
        refused(freq=None, n_tables=1)
        refused(chains=[(0, n_rows, 1)])                               # a table that is not there
        refused(chains=[(0, n_rows + 1, 0)])                           # a chain beyond the steps
        refused(row=[0, 1, 2, 3, 4, n_rows])                           # a step beyond the rows
    finally:
        ctx.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------------
FRE_LINE = r"HMM transitions by haplotype frequency on the device: (\d+) windows"


def _genotype(exe, cohort, work, opts, n_samples=1, env_more=None, gpu=True):
    """`genotype` on a committed cohort (the same reads for every sample of the run): (exit status, stderr, the samples' VCFs)."""
    import gzip
    import os
    from conftest import GOLDEN
    from test_gpu_configs import ENV, _run
    d = os.path.join(GOLDEN, cohort)
    os.makedirs(work, exist_ok=True)
    graph = os.path.join(work, "graph.bin")
    open(graph, "wb").write(gzip.open(os.path.join(d, "graph.bin.gz"), "rb").read())
    fq = [os.path.join(d, f"reads_{i}.fq.gz") for i in (1, 2)]
    open(os.path.join(work, "samples.cfg"), "w").write("".join(f"sample{s} " + " ".join(fq) + "\n" for s in range(n_samples)))
    env = dict(ENV, **(env_more or {}))      # (ENV pins VGH_RANDOM_DEVICE_VALUE=20241022)
    r = _run([exe, "genotype", "--load-graph", graph, "-s", "samples.cfg", "-t", "4"] + (["--gpu", "0", "--buffer", "8"] if gpu else []) + opts, cwd=work,
             capture_output=True, text=True, env=env, timeout=300)
    vcfs = []
    if r.returncode == 0:
        vcfs = [gzip.open(os.path.join(work, f"sample{s}.varigraph.vcf.gz"), "rb").read() for s in range(n_samples)]
    return r.returncode, r.stderr, vcfs


CLI_CASES = [
    # cohort, options, samples in the run, the committed VCF, samples the log line is due for, more environment
    ("cohort_sv", ["-m", "fre"], 1, "expected_fre.vcf", 1, {}),                                   # whole panel, 7 haplotypes
    ("cohort_snp", ["-m", "fre", "-n", "5"], 1, "expected_fre_n5.vcf", 1, {}),                      # haplotypes selected per window
    ("cohort_snp", ["-m", "fre", "-n", "5"], 3, None, 3, {}),                                       # ... each sample from the lists the last one pruned
    ("cohort_snp", ["-m", "fre", "-n", "5", "--sv"], 1, None, 1, {}),
    ("cohort_snp", ["-m", "fre", "-n", "5", "-g", "hom"], 1, None, 1, {}),
    ("cohort_tetra", ["--sample-ploidy", "4", "-m", "fre", "--use-depth"], 1, None, 1, {}),        # whole panel, 13 haplotypes, blocks of four
    ("cohort_snp", ["-m", "fre", "-n", "5"], 3, None, 2, {"VGH_HMM_FAKE_NOMEM": "1"}),              # the first sample is refused the device
]


@pytest.mark.parametrize("cohort,opts,n_samples,committed,n_lines,env_more", CLI_CASES,
                         ids=["sv_panel", "snp_n5", "snp_n5_x3", "snp_n5_sv", "snp_n5_hom", "tetra_panel", "snp_n5_x3_first_refused"])
def test_command_line_by_haplotype_frequency_on_the_device_equals_the_reference(cohort, opts, n_samples, committed, n_lines, env_more, tmp_path):
    """`varigraph-mi genotype -m fre`: every VCF is the deterministic reference build's byte for byte, and the bytes VGH_HMM_FRE_DEVICE=0 (the
    host's recursion) writes; the committed VCF where there is one, GQ aside.  The VGH_TIMING log names the new recursion once per sample
    that takes it, and never with the knob off."""
    import os
    from conftest import GOLDEN
    from test_gpu_configs import CLI, REF, _need_binaries
    from test_gpu_integration import _strip_gq
    _need_binaries()
    rc, err, dev = _genotype(CLI, cohort, str(tmp_path / "device"), opts, n_samples, dict(env_more, VGH_TIMING="1"))
    assert rc == 0, err[-2000:]
    rc, err_host, host = _genotype(CLI, cohort, str(tmp_path / "host"), opts, n_samples, dict(env_more, VGH_TIMING="1", VGH_HMM_FRE_DEVICE="0"))
    assert rc == 0, err_host[-2000:]
    rc, err_ref, ref = _genotype(REF, cohort, str(tmp_path / "cpu"), opts, n_samples, gpu=False)
    assert rc == 0, err_ref[-2000:]
    for s in range(n_samples):
        assert dev[s] == ref[s], (opts, s)
        assert dev[s] == host[s], (opts, s, "VGH_HMM_FRE_DEVICE=0")
    if "--sv" not in opts:
        assert min(v.count(b"\n") for v in ref) > 20
    if committed:
        want = open(os.path.join(GOLDEN, cohort, committed), "rb").read()
        assert _strip_gq(dev[0]) == _strip_gq(want)
    seen = re.findall(FRE_LINE, err)
    assert len(seen) == n_lines, err[-3000:]
    if "--sv" not in opts:      # (cohort_snp has no allele of 50 bases: under --sv the path is taken and no window has a row)
        assert all(int(w) >= 1 for w in seen), seen
    assert not re.search(FRE_LINE, err_host)


def test_command_line_polyploid_with_selection_keeps_the_host_path(tmp_path):
    """`--sample-ploidy 4 -m fre -n 5`: a window's blocks name haplotypes that were not drawn and have no score.  The reference stops there
    ("does not exist in 'hapIdxScoreMap'"), and this build keeps doing the same, on the host: no log line, the exit status and the last line
    of VGH_HMM_FRE_DEVICE=0."""
    from test_gpu_configs import CLI, REF, _need_binaries
    _need_binaries()
    opts = ["--sample-ploidy", "4", "-m", "fre", "-n", "5"]
    rc, err, _ = _genotype(CLI, "cohort_tetra", str(tmp_path / "device"), opts, 1, {"VGH_TIMING": "1"})
    rc_host, err_host, _ = _genotype(CLI, "cohort_tetra", str(tmp_path / "host"), opts, 1, {"VGH_TIMING": "1", "VGH_HMM_FRE_DEVICE": "0"})
    rc_ref, err_ref, _ = _genotype(REF, "cohort_tetra", str(tmp_path / "cpu"), opts, 1, gpu=False)
    assert not re.search(FRE_LINE, err) and not re.search(FRE_LINE, err_host)
    assert rc == rc_host
    assert err.strip().splitlines()[-1] == err_host.strip().splitlines()[-1]
    assert rc_ref != 0 and rc != 0
    assert "does not exist in 'hapIdxScoreMap'" in err_ref and "does not exist in 'hapIdxScoreMap'" in err
