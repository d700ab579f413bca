"""Haplotypes selected per window on the device (`-n` below the number of haplotypes of the graph, a diploid sample): the alive state of
the node lists, the support sums the draw is weighted by, the emission scores with the reference's prune (src/genotype.cpp:673-686,
815-818) and the calls' tallies -- each against the same computation spelled out in numpy (products in numpy.longdouble, the x87 format,
bit for bit) -- and the command line against the deterministic build of the reference."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from varigraph_amd import vgmi

pytestmark = pytest.mark.gpu
LD = np.longdouble
AVE = np.float32(23.5)
LOWER = float(AVE) - 1.96 * float(np.sqrt(np.float64(AVE)))
UPPER = float(AVE) + 1.96 * float(np.sqrt(np.float64(AVE)))


def _mld(h, c, ff):
    """most_likely_depth (src/genotype.cpp:1118-1145) in the host's float / double steps"""
    if ff == 1:
        return c
    cf = np.float32(c)
    if h > 0 and cf > AVE * np.float32(h):
        return int(AVE * np.float32(h)) & 0xFF
    if h == 0 and cf > AVE:
        return 0 if float(ff) > float(cf) / UPPER else int(cf / np.float32(ff)) & 0xFF
    if h == 0:
        return int(cf / np.float32(ff)) & 0xFF
    return c


def _model_emissions(f, bits, cov, alive, bit_len, pairs, win_used, tables, entry_begin, counts, row_win, gt0, fixes=None, prune=True):
    """hidden_states(filter = true) + observable_states over the rows' ranges: returns (obs, n_kept, flags); `alive` is pruned in place.
    fixes: {(row, j): mask} -- haplotypes (bits over the window's places) taken off entry j of the row's range."""
    n_gt = len(pairs)
    pa = np.array([a for a, _ in pairs])
    pb = np.array([b for _, b in pairs])
    obs = np.ones((len(counts), n_gt), dtype=LD)
    n_kept = np.zeros(len(counts), dtype=np.uint32)
    flags = np.zeros(len(counts), dtype=np.uint8)
    for r in range(len(counts)):
        used = [int(h) for h in win_used[row_win[r]]]
        top_mask = 0
        for h in used:
            top_mask |= 1 << h
        prod = np.ones(n_gt, dtype=LD)
        for jj in range(int(counts[r])):
            j = int(entry_begin[r]) + jj
            if not alive[j]:
                continue
            c, ff, b = int(cov[j]), int(f[j]), int(bits[j])
            if b & top_mask == 0:
                if prune:
                    alive[j] = 0
                continue
            n_kept[r] += 1
            last = (b >> (8 * bit_len - 1)) & 1
            in_interval = last == 1 and LOWER <= c <= UPPER
            one = np.array([1 if (in_interval and (int(gt0[r]) >> p) & 1) else (b >> h) & 1 for p, h in enumerate(used)])
            if c < LOWER and ff >= 2 and one.any():
                flags[r] |= 1
            if fixes and (r, jj) in fixes:
                one = np.array([0 if (fixes[(r, jj)] >> p) & 1 else o for p, o in enumerate(one)])
            fj = 2 if (last == 1 and ff == 1) else ff
            t = np.array([tables[h * 256 + _mld(h, c, fj)] for h in (0, 1, 2)], dtype=LD)
            prod = prod * t[one[pa] + one[pb]]
        obs[r] = prod
    return obs, n_kept, flags


def _panel(rng, n_hap, bit_len, n_rows, density=0.15, fixed=None):
    counts = rng.integers(0, 71, size=n_rows)
    for r, n in (fixed or {}).items():
        counts[r] = n
    entry_begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    n_entries = int(counts.sum())
    f = rng.choice([1, 1, 1, 2, 3, 4], size=n_entries).astype(np.uint64)
    bits = np.zeros(n_entries, dtype=np.uint64)
    for h in range(n_hap):
        bits |= (rng.random(n_entries) < density).astype(np.uint64) << np.uint64(h)
    bits |= rng.integers(0, 2, size=n_entries).astype(np.uint64) << np.uint64(8 * bit_len - 1)
    cov = rng.choice([0, 1, 5, 14, 15, 20, 23, 24, 30, 33, 34, 60, 255], size=n_entries).astype(np.uint8)
    return counts, entry_begin, f, bits, cov


@pytest.mark.parametrize("bit_len,n_hap,n_used", [(2, 9, 5), (2, 15, 15), (3, 23, 5), (3, 23, 15), (6, 47, 5), (6, 47, 15)])
def test_emissions_with_selection_equal_the_host_arithmetic_and_prune_for_good(bit_len, n_hap, n_used):
    """vgmi_hmm_emissions_select against the numpy model, bit for bit: three windows with different haplotypes (ids below 16, 16..31 and
    from 32 up -- a 32-bit shift would lose them), ~40 rows each of 0..70 entries, a row whose entries all die, rows with entries dead on
    entry, a row with a carried under-covered multi-copy k-mer (flag bit 0) that a second launch scores again (vgmi_hmm_part_fix_rows,
    fix_j = places in the row's range), the alive bytes afterwards; then the next sample on the same context with another selection: it
    scores the lists the first one pruned, and what the first selection killed stays dead whoever carries it now.
    (Nine haplotypes cannot lend fifteen: with two bytes of haplotype bits the 120-genotype case runs on a panel of fifteen.)"""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    rng = np.random.default_rng(1000 * bit_len + n_used)
    n_windows, per_window = 3, 40
    n_rows = n_windows * per_window
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, fixed={3: 20, 50: 30, 90: 25})
    row_win = np.repeat(np.arange(n_windows), per_window).astype(np.uint32)

    def selection():
        sel = []
        for w in range(n_windows):      # every window holds a haplotype near the top of the panel
            others = [h for h in range(n_hap) if h != n_hap - 1 - w]
            sel.append(sorted([n_hap - 1 - w] + list(rng.choice(others, size=n_used - 1, replace=False))))
        return np.array(sel, dtype=np.uint8)
    win_used = selection()
    assert bit_len < 3 or (win_used >= 16).any()
    assert bit_len < 6 or ((win_used >= 32).any() and ((win_used >= 16) & (win_used < 32)).any())
    masks = np.array([sum(1 << int(h) for h in u) for u in win_used], dtype=np.uint64)
    pairs = list(itertools.combinations_with_replacement(range(n_used), 2))
    assert len(pairs) == (15 if n_used == 5 else 120)
    gt0 = rng.integers(0, 1 << n_used, size=n_rows).astype(np.uint16)
    tables = (rng.random(768).astype(LD) + LD(0.05)) * np.power(LD(10), rng.integers(-300, 1, size=768).astype(LD))
    # row 3: no entry carries a haplotype of its window (n_kept = 0); row 50: half its entries dead on entry; row 90: entry 2 is an
    # under-covered multi-copy k-mer that the window's first two haplotypes carry
    counts_l = counts.tolist()
    e3 = slice(int(entry_begin[3]), int(entry_begin[3]) + counts_l[3])
    bits[e3] &= ~masks[0]
    alive0 = (rng.random(f.size) < 0.9).astype(np.uint8)
    alive0[int(entry_begin[50]):int(entry_begin[50]) + counts_l[50]:2] = 0
    j90 = int(entry_begin[90]) + 2
    alive0[j90] = 1
    cov[j90], f[j90] = 1, 2
    bits[j90] |= (np.uint64(1) << np.uint64(win_used[2][0])) | (np.uint64(1) << np.uint64(win_used[2][1]))
    gt0[90] = 0
    entries = (f << np.uint64(8)) | (bits << np.uint64(16))
    fixes = {(90, 2): 0b01}
    win_used2 = selection()

    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload(entries, cov, alive0)
        obs, n_kept, flags = ctx.hmm_emissions_select([a for a, _ in pairs], [b for _, b in pairs], win_used, masks, bit_len, AVE, LOWER, UPPER, tables,
                                                      entry_begin, counts, row_win, gt0)
        alive1 = ctx.hmm_alive_fetch()
        # the same selection once more with the flagged row scored again: nothing further dies, the other rows keep their scores
        obs_f, n_kept_f, flags_f = ctx.hmm_emissions_select([a for a, _ in pairs], [b for _, b in pairs], win_used, masks, bit_len, AVE, LOWER, UPPER,
                                                            tables, entry_begin, counts, row_win, gt0, fixes=([90], [0, 1], [2], [fixes[(90, 2)]]))
        alive1b = ctx.hmm_alive_fetch()
        # the next sample: other haplotypes per window, the lists as the first sample left them
        masks2 = np.array([sum(1 << int(h) for h in u) for u in win_used2], dtype=np.uint64)
        obs2, n_kept2, flags2 = ctx.hmm_emissions_select([a for a, _ in pairs], [b for _, b in pairs], win_used2, masks2, bit_len, AVE, LOWER, UPPER,
                                                         tables, entry_begin, counts, row_win, gt0)
        alive2 = ctx.hmm_alive_fetch()
    finally:
        ctx.close()

    m_alive = alive0.copy()
    want, want_kept, want_flags = _model_emissions(f, bits, cov, m_alive, bit_len, pairs, win_used, tables, entry_begin, counts, row_win, gt0)
    assert np.array_equal(n_kept, want_kept) and np.array_equal(flags, want_flags)
    for r in range(n_rows):
        assert np.array_equal(obs[r], want[r]), (r, int(np.argmax(obs[r] != want[r])))
    assert np.array_equal(alive1, m_alive)
    assert n_kept[3] == 0 and not alive1[e3].any() and (obs[3] == 1).all()
    assert flags[90] & 1 and not (flags & 2).any()
    assert 0 < (alive0 != alive1).sum() and (n_kept > 0).sum() > n_rows // 2 and (obs == 0).any() and (obs > 0).any()

    want_f, _, _ = _model_emissions(f, bits, cov, m_alive, bit_len, pairs, win_used, tables, entry_begin, counts, row_win, gt0, fixes=fixes)
    assert np.array_equal(alive1b, alive1) and np.array_equal(n_kept_f, n_kept) and np.array_equal(flags_f, flags)
    for r in range(n_rows):
        assert np.array_equal(obs_f[r], want_f[r]), r
    assert not np.array_equal(obs_f[90], obs[90]) and np.array_equal(np.delete(obs_f, 90, axis=0), np.delete(obs, 90, axis=0))

    killed = (alive0 == 1) & (alive1 == 0)
    revived_if_forgotten = sum(1 for j in np.flatnonzero(killed)
                               if int(bits[j]) & int(masks2[row_win[np.searchsorted(entry_begin, j, side="right") - 1]]))
    assert revived_if_forgotten > 0 or n_used == n_hap, "no entry would tell a persistent prune from a fresh one"
    want2, want_kept2, want_flags2 = _model_emissions(f, bits, cov, m_alive, bit_len, pairs, win_used2, tables, entry_begin, counts, row_win, gt0)
    assert np.array_equal(n_kept2, want_kept2) and np.array_equal(flags2, want_flags2)
    for r in range(n_rows):
        assert np.array_equal(obs2[r], want2[r]), (r, int(np.argmax(obs2[r] != want2[r])))
    assert np.array_equal(alive2, m_alive) and not alive2[killed].any() and n_kept2[3] == 0


def test_support_sums_equal_the_host_loop():
    """vgmi_hmm_support against src/genotype.cpp:500-560 in numpy: entries with c <= 1, with multiplicity > 1 and dead entries do not
    count, a window without rows reads zero, windows that change inside a workgroup's rows, and one row of 300 entries at coverage 255
    that one haplotype carries throughout (76 500: a 16-bit sum would wrap)."""
    rng = np.random.default_rng(4242)
    bit_len, n_hap = 3, 23
    rows_of = [70, 30, 0, 50]
    n_windows = len(rows_of)
    row_win = np.repeat(np.arange(n_windows), rows_of).astype(np.uint32)
    n_rows = row_win.size
    counts = rng.integers(0, 71, size=n_rows)
    big = 120                                  # a row of the last window
    counts[big] = 300
    entry_begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    n_entries = int(counts.sum())
    f = rng.choice([0, 1, 1, 2, 3], size=n_entries).astype(np.uint64)
    bits = np.zeros(n_entries, dtype=np.uint64)
    for h in range(n_hap):
        bits |= (rng.random(n_entries) < 0.3).astype(np.uint64) << np.uint64(h)
    bits |= rng.integers(0, 2, size=n_entries).astype(np.uint64) << np.uint64(8 * bit_len - 1)      # the last bit is no haplotype
    cov = rng.choice([0, 1, 2, 5, 40, 255], size=n_entries).astype(np.uint8)
    alive = (rng.random(n_entries) < 0.8).astype(np.uint8)
    eb = slice(int(entry_begin[big]), int(entry_begin[big]) + 300)
    f[eb], cov[eb], alive[eb] = 1, 255, 1
    bits[eb] |= np.uint64(1 << 7)
    entries = (f << np.uint64(8)) | (bits << np.uint64(16))
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload(entries, cov, alive)
        got = ctx.hmm_support(n_hap, n_windows, entry_begin, counts, row_win)
        none = ctx.hmm_support(n_hap, 2, entry_begin[:0], counts[:0], row_win[:0])
    finally:
        ctx.close()
    want = np.zeros((n_windows, n_hap), dtype=np.uint64)
    seen = {"low": 0, "multi": 0, "dead": 0}
    for r in range(n_rows):
        for j in range(int(entry_begin[r]), int(entry_begin[r]) + int(counts[r])):
            if not alive[j]:
                seen["dead"] += 1
                continue
            if cov[j] <= 1:
                seen["low"] += 1
                continue
            if f[j] > 1:
                seen["multi"] += 1
                continue
            for h in range(n_hap):
                if (int(bits[j]) >> h) & 1:
                    want[row_win[r], h] += int(cov[j])
    assert min(seen.values()) > 50
    assert np.array_equal(got.astype(np.uint64), want)
    assert want[3, 7] >= 76500 and not want[2].any() and want[0].all() and want[1].all()
    assert none.shape == (2, n_hap) and not none.any()


def test_tallies_with_selection_equal_the_host_walk():
    """vgmi_hmm_tallies_select against posterior()'s tallies (src/genotype.cpp:1387-1414) on pruned lists: the called pair's haplotypes
    stand at other places in other windows, a row without a call (winner 0xFFFFFFFF) reads zeros, dead entries count for nothing --
    not for the single-copy k-mers either."""
    rng = np.random.default_rng(99)
    bit_len, n_hap, n_used, n_windows, per_window = 6, 47, 5, 3, 100
    n_rows = n_windows * per_window
    counts = rng.integers(0, 71, size=n_rows)
    counts[7] = 400                                         # more than 255 single-copy k-mers: the count stops at 255
    entry_begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    n_entries = int(counts.sum())
    f = rng.choice([0, 1, 1, 2, 3], size=n_entries).astype(np.uint64)
    f[int(entry_begin[7]):int(entry_begin[7]) + 400] = 1
    bits = rng.integers(0, 1 << 47, size=n_entries, dtype=np.uint64) & rng.integers(0, 1 << 47, size=n_entries, dtype=np.uint64)
    cov = rng.integers(0, 256, size=n_entries).astype(np.uint8)
    alive = (rng.random(n_entries) < 0.7).astype(np.uint8)
    alive[int(entry_begin[7]):int(entry_begin[7]) + 400] = 1
    entries = (f << np.uint64(8)) | (bits << np.uint64(16))
    row_win = np.repeat(np.arange(n_windows), per_window).astype(np.uint32)
    win_used = np.array([[0, 5, 17, 33, 46], [1, 16, 31, 32, 45], [2, 3, 4, 15, 40]], dtype=np.uint8)
    pairs = list(itertools.combinations_with_replacement(range(n_used), 2))
    n_gt = len(pairs)
    winner = rng.integers(0, n_gt, size=n_rows).astype(np.uint32)
    winner[::9] = 0xFFFFFFFF
    winner[7] = 3
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload(entries, cov, alive)
        out, uniq = ctx.hmm_tallies_select(entry_begin, counts, row_win, winner, [a for a, _ in pairs], [b for _, b in pairs], win_used)
    finally:
        ctx.close()
    n_dead_unique = 0
    for r in range(n_rows):
        want, u = [0, 0, 0, 0], 0
        if winner[r] < n_gt:
            ha, hb = (int(win_used[row_win[r]][p]) for p in pairs[winner[r]])
            for j in range(int(entry_begin[r]), int(entry_begin[r]) + int(counts[r])):
                if not alive[j]:
                    n_dead_unique += f[j] <= 1
                    continue
                if f[j] <= 1 and u < 255:
                    u += 1
                if (int(bits[j]) >> ha) & 1:
                    want[0] += 1
                    want[1] += int(cov[j])
                if (int(bits[j]) >> hb) & 1:
                    want[2] += 1
                    want[3] += int(cov[j])
        assert out[r].tolist() == want and uniq[r] == u, r
    assert uniq[7] == 255 and n_dead_unique > 100 and not out[::9].any() and out[1::9].any()


# ---- the command line: a cohort of 6 diploid samples (12 haplotypes + the reference), -n 5 ---------------------------------------
@pytest.fixture(scope="module")
def select_cohort(tmp_path_factory):
    """200 kb, 1 500 sites (one in ten a short indel, four in ten an insertion of 60..300 bp: `--sv` has hundreds of sites to call), the
    graph built once, reads of three individuals at ~30x; three samples in one samples.cfg: the second and third see pruned lists."""
    import shutil
    from test_gpu_configs import CLI, ENV, _need_binaries, _write_fastq
    from varigraph_amd import synth
    _need_binaries()
    work = str(tmp_path_factory.mktemp("select_cli"))
    ref = synth.make_reference(200_000)
    variants, gts = synth.make_cohort(ref, 1500, n_samples=6, ploidy=2, seed=15, indel_frac=0.1, sv_frac=0.4)
    fa, vcf = os.path.join(work, "ref.fa"), os.path.join(work, "in.vcf")
    synth.write_fasta(fa, "chr1", ref)
    synth.write_vcf(vcf, "chr1", len(ref), variants, gts, 6, 2)
    graph = os.path.join(work, "graph.bin")
    r = subprocess.run([CLI, "construct", "-r", fa, "-v", vcf, "--save-graph", graph, "-t", "16", "--gpu", "0"], cwd=work, capture_output=True, text=True,
                       env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    cfg = ""
    for i, who in enumerate((0, 2, 4)):
        fq = _write_fastq(os.path.join(work, f"s{i}"), synth.sample_haplotypes(ref, variants, gts, who, 2), 20_000, seed=70 + i)
        cfg += f"ind{i} " + " ".join(fq) + "\n"
    yield work, graph, cfg
    shutil.rmtree(work, ignore_errors=True)


@pytest.mark.parametrize("extra", [[], ["--sv"], ["-g", "hom"]], ids=["het", "sv", "hom"])
def test_command_line_with_selection_on_the_device_equals_the_reference(extra, select_cohort):
    """`varigraph-mi genotype -n 5 --use-depth` over a 13-haplotype graph, three samples in one run: every VCF is the deterministic
    reference build's byte for byte, the VGH_TIMING log shows the emissions on the device with haplotypes selected per window for every
    window of all three samples, and VGH_HMM_SELECT_DEVICE=0 (the host's preparation) writes the same bytes.  The reference's VCFs hold
    at least 200 lines each ("a few hundred": an empty result must not pass).  VGH_HMM_FIX_DEVICE=0 (flagged nodes scored by the host: 50 to
    58 per sample of this cohort, 1 to 3 under --sv; none of them is scored again on the device in a default run) and VGH_DEVICE_TALLIES=0
    (the calls' tallies walked by the host) keep the selection on the device and write the same bytes."""
    from test_gpu_configs import CLI, ENV, REF, _run, _vcf
    work, graph, cfg = select_cohort
    opts = ["-n", "5", "--use-depth", "--granularity", "0.05"] + extra      # 50 kb windows: four of them
    tag = "_".join(extra).replace("-", "") or "het"
    outs, logs = {}, {}
    for name, exe, more, env in (("cpu", REF, [], ENV), ("native", CLI, ["--gpu", "0"], dict(ENV, VGH_TIMING="1")),
                                 ("host", CLI, ["--gpu", "0"], dict(ENV, VGH_TIMING="1", VGH_HMM_SELECT_DEVICE="0")),
                                 ("host_fixes", CLI, ["--gpu", "0"], dict(ENV, VGH_TIMING="1", VGH_HMM_FIX_DEVICE="0")),
                                 ("host_tallies", CLI, ["--gpu", "0"], dict(ENV, VGH_TIMING="1", VGH_DEVICE_TALLIES="0"))):
        d = os.path.join(work, f"{name}_{tag}")
        os.makedirs(d, exist_ok=True)
        open(os.path.join(d, "samples.cfg"), "w").write(cfg)
        r = _run([exe, "genotype", "--load-graph", graph, "-s", "samples.cfg", "-t", "6"] + opts + more, cwd=d, capture_output=True, text=True, env=env,
                 timeout=600)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        outs[name] = [_vcf(d, f"ind{i}") for i in range(3)]
        logs[name] = r.stderr
    lines = [v.count(b"\n") for v in outs["cpu"]]
    print(f"-n 5 {' '.join(extra)}: reference VCF lines {lines}")
    assert min(lines) >= 200, lines
    assert outs["cpu"][0] != outs["cpu"][1] != outs["cpu"][2]
    for i in range(3):
        assert outs["native"][i] == outs["cpu"][i], (extra, i)
        assert outs["host"][i] == outs["cpu"][i], (extra, i, "VGH_HMM_SELECT_DEVICE=0")
        # the flagged nodes scored by the host instead of a second launch; the calls' tallies walked by the host
        assert outs["host_fixes"][i] == outs["cpu"][i], (extra, i, "VGH_HMM_FIX_DEVICE=0")
        assert outs["host_tallies"][i] == outs["cpu"][i], (extra, i, "VGH_DEVICE_TALLIES=0")
    for name in ("native", "host_fixes", "host_tallies"):
        seen = re.findall(r"HMM emissions on the device: .*haplotypes selected per window for (\d+) of (\d+) windows", logs[name])
        assert len(seen) == 3 and all(a == b and int(b) >= 4 for a, b in seen), (name, seen)
    scored = {name: [tuple(map(int, m)) for m in re.findall(r"(\d+) nodes scored by the host, (\d+) scored again on the device", logs[name])]
              for name in ("native", "host_fixes")}
    print(f"-n 5 {' '.join(extra)}: nodes scored by the host / again on the device, per sample: {scored}")
    assert "haplotypes selected per window" not in logs["host"]
