"""Haplotypes selected per window on the device for a POLYPLOID sample (`--sample-ploidy` 3 or 4, `-n` below the number of haplotypes of
the graph): every window has its own genotype list -- the blocks of `ploidy` consecutive haplotypes that hold a drawn haplotype
(src/genotype.cpp:846-873) -- so the emission kernel takes the lists by haplotype id and 64-bit masks over ids.  The kernel against the
same computation spelled out in numpy (products in numpy.longdouble, the x87 format, bit for bit), and the command line against the
deterministic build of the reference."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from varigraph_amd import vgmi
from test_gpu_hmm_select import AVE, LD, LOWER, UPPER, _mld, _panel

pytestmark = pytest.mark.gpu


def _blocks(top, ploidy, max_hap):
    """haplotype_combinations for ploidy > 2: per drawn haplotype its block, ids above max_hap read 0; the sorted set of them"""
    out = set()
    for h in top:
        if h == 0:
            out.add((0,) * ploidy)
            continue
        first = (math.ceil(h / ploidy) - 1) * ploidy + 1
        out.add(tuple(x if x <= max_hap else 0 for x in range(first, first + ploidy)))
    return sorted(out)


def _model(f, bits, cov, alive, bit_len, win_n, win_haps, win_top, tables, entry_begin, counts, row_win, gt0, fixes=None):
    """hidden_states(filter = true) + observable_states with a genotype list per window: returns (obs, n_kept, flags); `alive` is pruned
    in place.  fixes: {(row, j): mask over haplotype ids} taken off entry j of the row's range.  Scores beyond a window's count are zero."""
    n_gt = win_haps.shape[1]
    obs = np.zeros((len(counts), n_gt), dtype=LD)
    n_kept = np.zeros(len(counts), dtype=np.uint32)
    flags = np.zeros(len(counts), dtype=np.uint8)
    for r in range(len(counts)):
        w = int(row_win[r])
        n = int(win_n[w])
        haps = win_haps[w, :n].astype(np.int64)
        used_mask = 0
        for h in haps.ravel():
            used_mask |= 1 << int(h)
        top_mask = int(win_top[w])
        prod = np.ones(n, dtype=LD)
        for jj in range(int(counts[r])):
            j = int(entry_begin[r]) + jj
            if not alive[j]:
                continue
            c, ff, b = int(cov[j]), int(f[j]), int(bits[j])
            if b & top_mask == 0:
                alive[j] = 0
                continue
            n_kept[r] += 1
            last = (b >> (8 * bit_len - 1)) & 1
            in_interval = last == 1 and LOWER <= c <= UPPER
            om = (b | (int(gt0[r]) if in_interval else 0)) & used_mask
            if c < LOWER and ff >= 2 and om:
                flags[r] |= 1
            if fixes and (r, jj) in fixes:
                om &= ~fixes[(r, jj)]
            fj = 2 if (last == 1 and ff == 1) else ff
            h = np.array([sum((om >> int(x)) & 1 for x in gt) for gt in haps])      # repeats count each time
            prod = prod * np.array([tables[int(x) * 256 + _mld(int(x), c, fj)] for x in h], dtype=LD)
        obs[r, :n] = prod
    return obs, n_kept, flags


@pytest.mark.parametrize("n_drawn", [1, 5, 15])
@pytest.mark.parametrize("bit_len,n_hap", [(2, 15), (6, 47)])
@pytest.mark.parametrize("ploidy", [3, 4])
def test_emissions_with_a_genotype_list_per_window_equal_the_host_arithmetic(ploidy, bit_len, n_hap, n_drawn):
    """vgmi_hmm_emissions_select_ploidy against the numpy model, bit for bit -- scores, n_kept, flags, alive bytes -- in ONE call over six
    windows: a random draw, a draw with haplotype 0 (the all-zero block), a draw with the last haplotype (n_hap - 1 is no multiple of the
    ploidy: a truncated block, haplotype 0 repeated in it), two drawn haplotypes in one block, a single drawn haplotype (one genotype),
    and a second random draw; their lists have different lengths (-n > 1).  ~35 rows each of 0..70 entries: a row of zero entries, a row
    that loses every entry, a row half of whose entries are dead on entry, and a flagged row (a carried under-covered multi-copy k-mer)
    that a second launch scores again with a fix mask that clears the panel's last haplotype (id 46 with six bytes of bits: above 15).
    A second call on the same rows sees the first call's prune; a third with other draws scores what is left."""
    assert np.finfo(LD).nmant == 63, "numpy.longdouble is not the x87 format here"
    rng = np.random.default_rng(100 * ploidy + 10 * bit_len + n_drawn)
    max_hap = n_hap - 1
    assert max_hap % ploidy != 0 and max_hap == 8 * bit_len - 2
    per_window = 35

    def draws():
        def some(k, must=()):
            pool = [h for h in range(n_hap) if h not in must]
            return sorted(list(must) + [int(x) for x in rng.choice(pool, size=max(0, k - len(must)), replace=False)])
        return [some(n_drawn), some(n_drawn, (0,)), some(n_drawn, (max_hap,)), some(n_drawn, (1, 2) if n_drawn > 1 else (1,)), [5], some(n_drawn)]

    def windows(tops):
        lists = [_blocks(t, ploidy, max_hap) for t in tops]
        n_gt = max(len(x) for x in lists)
        win_haps = np.zeros((len(tops), n_gt, ploidy), dtype=np.uint8)
        for w, x in enumerate(lists):
            win_haps[w, :len(x)] = np.array(x, dtype=np.uint8)
        return (np.array([len(x) for x in lists], dtype=np.uint32), win_haps,
                np.array([sum(1 << h for h in t) for t in tops], dtype=np.uint64), lists)

    tops = draws()
    n_windows = len(tops)
    n_rows = n_windows * per_window
    win_n, win_haps, win_top, lists = windows(tops)
    assert (0,) * ploidy in lists[1] and any(0 in gt and max_hap in gt for gt in lists[2]) and win_n[4] == 1
    assert n_drawn == 1 or (len(set(win_n.tolist())) > 1 and win_n[3] < n_drawn), win_n
    zero_row, lost_row, dead_row, flag_row = 2, per_window + 3, 3 * per_window + 5, 2 * per_window + 7
    counts, entry_begin, f, bits, cov = _panel(rng, n_hap, bit_len, n_rows, fixed={zero_row: 0, lost_row: 20, dead_row: 30, flag_row: 25})
    row_win = np.repeat(np.arange(n_windows), per_window).astype(np.uint32)
    gt0 = rng.integers(0, 1 << n_hap, size=n_rows, dtype=np.uint64)
    tables = (rng.random(256 * (ploidy + 1)).astype(LD) + LD(0.05)) * np.power(LD(10), rng.integers(-300, 1, size=256 * (ploidy + 1)).astype(LD))
    counts_l = counts.tolist()
    e_lost = slice(int(entry_begin[lost_row]), int(entry_begin[lost_row]) + counts_l[lost_row])
    bits[e_lost] &= ~win_top[1]
    alive0 = (rng.random(f.size) < 0.9).astype(np.uint8)
    alive0[int(entry_begin[dead_row]):int(entry_begin[dead_row]) + counts_l[dead_row]:2] = 0
    alive0[int(entry_begin[dead_row]) + 1] = 1      # (one of the living is carried by the window's draw for certain)
    bits[int(entry_begin[dead_row]) + 1] |= win_top[3]
    # the flagged row (window 2, whose draw holds the last haplotype): entry 2 is under-covered, multi-copy and carried by the last
    # haplotype alone among those of its block; the sequence check takes it off
    jf = int(entry_begin[flag_row]) + 2
    alive0[jf] = 1
    cov[jf], f[jf] = 1, 2
    last_block = next(gt for gt in lists[2] if max_hap in gt)
    bits[jf] &= ~np.uint64(sum(1 << h for h in set(last_block)))
    bits[jf] |= np.uint64(1) << np.uint64(max_hap)
    gt0[flag_row] = 0
    entries = (f << np.uint64(8)) | (bits << np.uint64(16))
    fixes = {(flag_row, 2): 1 << max_hap}
    tops2 = draws()
    win_n2, win_haps2, win_top2, _ = windows(tops2)

    def call(ctx, wn, wh, wt, fx=None):
        return ctx.hmm_emissions_select_ploidy(ploidy, wn, wh, wt, bit_len, AVE, LOWER, UPPER, tables, entry_begin, counts, row_win, gt0, fixes=fx)

    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload(entries, cov, alive0)
        obs, n_kept, flags = call(ctx, win_n, win_haps, win_top)
        alive1 = ctx.hmm_alive_fetch()
        obs_f, n_kept_f, flags_f = call(ctx, win_n, win_haps, win_top, ([flag_row], [0, 1], [2], [fixes[(flag_row, 2)]]))
        alive1b = ctx.hmm_alive_fetch()
        obs2, n_kept2, flags2 = call(ctx, win_n2, win_haps2, win_top2)
        alive2 = ctx.hmm_alive_fetch()
    finally:
        ctx.close()

    m_alive = alive0.copy()
    want, want_kept, want_flags = _model(f, bits, cov, m_alive, bit_len, win_n, win_haps, win_top, tables, entry_begin, counts, row_win, gt0)
    assert np.array_equal(n_kept, want_kept) and np.array_equal(flags, want_flags)
    for r in range(n_rows):
        assert np.array_equal(obs[r], want[r]), (r, int(np.argmax(obs[r] != want[r])))
    assert np.array_equal(alive1, m_alive)
    assert n_kept[zero_row] == 0 and (obs[zero_row, :win_n[0]] == 1).all()
    assert n_kept[lost_row] == 0 and not alive1[e_lost].any() and (obs[lost_row, :win_n[1]] == 1).all()
    assert 0 < n_kept[dead_row] <= counts_l[dead_row] // 2
    assert flags[flag_row] & 1 and not (flags & 2).any()
    for w in range(n_windows):      # lanes beyond a window's count: zero scores
        assert not obs[row_win == w][:, win_n[w]:].any()
    assert 0 < (alive0 != alive1).sum() and (n_kept > 0).sum() > n_rows // 2 and (obs > 0).any()

    # the same lists once more with the flagged row scored again: nothing further dies, the other rows keep their scores
    want_f, _, _ = _model(f, bits, cov, m_alive, bit_len, win_n, win_haps, win_top, tables, entry_begin, counts, row_win, gt0, fixes=fixes)
    assert np.array_equal(alive1b, alive1) and np.array_equal(n_kept_f, n_kept) and np.array_equal(flags_f, flags)
    for r in range(n_rows):
        assert np.array_equal(obs_f[r], want_f[r]), r
    assert not np.array_equal(obs_f[flag_row], obs[flag_row]) and np.array_equal(np.delete(obs_f, flag_row, axis=0), np.delete(obs, flag_row, axis=0))

    # other draws: the lists as the first call left them
    want2, want_kept2, want_flags2 = _model(f, bits, cov, m_alive, bit_len, win_n2, win_haps2, win_top2, tables, entry_begin, counts, row_win, gt0)
    assert np.array_equal(n_kept2, want_kept2) and np.array_equal(flags2, want_flags2)
    for r in range(n_rows):
        assert np.array_equal(obs2[r], want2[r]), (r, int(np.argmax(obs2[r] != want2[r])))
    killed = (alive0 == 1) & (alive1 == 0)
    assert np.array_equal(alive2, m_alive) and not alive2[killed].any() and n_kept2[lost_row] == 0


# ---- the command line: a cohort of 4 tetraploid samples (16 haplotypes + the reference) --------------------------------------------
@pytest.fixture(scope="module")
def polyploid_cohort(tmp_path_factory):
    """200 kb, 1 500 sites (one in ten a short indel, four in ten an insertion of 60..300 bp), `--vcf-ploidy 4`: 17 haplotypes, and 16
    is no multiple of 3.  Reads of three individuals at ~30x, three samples in one samples.cfg: the second and third see pruned lists."""
    import shutil
    from test_gpu_configs import CLI, ENV, _need_binaries, _write_fastq
    from varigraph_amd import synth
    _need_binaries()
    work = str(tmp_path_factory.mktemp("select_ploidy_cli"))
    ref = synth.make_reference(200_000)
    variants, gts = synth.make_cohort(ref, 1500, n_samples=4, ploidy=4, seed=19, indel_frac=0.1, sv_frac=0.4)
    fa, vcf = os.path.join(work, "ref.fa"), os.path.join(work, "in.vcf")
    synth.write_fasta(fa, "chr1", ref)
    synth.write_vcf(vcf, "chr1", len(ref), variants, gts, 4, 4)
    graph = os.path.join(work, "graph.bin")
    r = subprocess.run([CLI, "construct", "-r", fa, "-v", vcf, "--save-graph", graph, "-t", "16", "--gpu", "0", "--vcf-ploidy", "4"], cwd=work,
                       capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    cfg = ""
    for i, who in enumerate((0, 1, 3)):
        fq = _write_fastq(os.path.join(work, f"s{i}"), synth.sample_haplotypes(ref, variants, gts, who, 4), 20_000, seed=170 + i)
        cfg += f"ind{i} " + " ".join(fq) + "\n"
    yield work, graph, cfg
    shutil.rmtree(work, ignore_errors=True)


@pytest.mark.parametrize("opts", [["--sample-ploidy", "4", "-n", "5"], ["--sample-ploidy", "3", "-n", "4"], ["--sample-ploidy", "4", "-n", "5", "--sv"],
                                  ["--sample-ploidy", "4", "-n", "5", "-g", "hom"]], ids=["p4n5", "p3n4", "p4n5sv", "p4n5hom"])
def test_command_line_polyploid_with_selection_on_the_device_equals_the_reference(opts, polyploid_cohort):
    """`varigraph-mi genotype --sample-ploidy P -n N --use-depth` over a 17-haplotype graph, 20 windows of 10 kb, three samples in one
    run: every VCF is the deterministic reference build's byte for byte (at least 100 lines each: an empty result must not pass), the
    VGH_TIMING log shows every window of all three samples on the device, VGH_HMM_SELECT_DEVICE=0 (today's path, no such log line),
    VGH_HMM_FIX_DEVICE=0 and VGH_DEVICE_TALLIES=0 write the same bytes, and so does a run whose first sample was refused the device
    (VGH_HMM_FAKE_NOMEM=1: it takes the pool, the host prunes its lists, the next two samples start from those on the device)."""
    from test_gpu_configs import CLI, ENV, REF, _run, _vcf
    work, graph, cfg = polyploid_cohort
    opts = opts + ["--use-depth", "--granularity", "0.01"]
    tag = "_".join(o.strip("-") for o in opts[:6])
    outs, logs = {}, {}
    for name, exe, more, env in (("cpu", REF, [], ENV), ("native", CLI, ["--gpu", "0"], dict(ENV, VGH_TIMING="1")),
                                 ("host", CLI, ["--gpu", "0"], dict(ENV, VGH_TIMING="1", VGH_HMM_SELECT_DEVICE="0")),
                                 ("host_fixes", CLI, ["--gpu", "0"], dict(ENV, VGH_TIMING="1", VGH_HMM_FIX_DEVICE="0")),
                                 ("host_tallies", CLI, ["--gpu", "0"], dict(ENV, VGH_TIMING="1", VGH_DEVICE_TALLIES="0")),
                                 ("host_first", CLI, ["--gpu", "0"], dict(ENV, VGH_TIMING="1", VGH_HMM_FAKE_NOMEM="1"))):
        d = os.path.join(work, f"{name}_{tag}")
        os.makedirs(d, exist_ok=True)
        open(os.path.join(d, "samples.cfg"), "w").write(cfg)
        r = _run([exe, "genotype", "--load-graph", graph, "-s", "samples.cfg", "-t", "6"] + opts + more, cwd=d, capture_output=True, text=True, env=env,
                 timeout=600)
        assert r.returncode == 0, (name, r.stderr[-2000:])
        outs[name] = [_vcf(d, f"ind{i}") for i in range(3)]
        logs[name] = r.stderr
    lines = [v.count(b"\n") for v in outs["cpu"]]
    print(f"{' '.join(opts)}: reference VCF lines {lines}")
    assert min(lines) >= 100, lines
    assert outs["cpu"][0] != outs["cpu"][1] != outs["cpu"][2]
    for name in ("native", "host", "host_fixes", "host_tallies", "host_first"):
        for i in range(3):
            assert outs[name][i] == outs["cpu"][i], (opts, name, i)
    device_line = r"HMM emissions on the device: .*haplotypes selected per window for (\d+) of (\d+) windows"
    for name in ("native", "host_fixes", "host_tallies"):
        seen = re.findall(device_line, logs[name])
        assert len(seen) == 3 and all(a == b and int(b) >= 20 for a, b in seen), (name, seen)
    seen = re.findall(device_line, logs["host_first"])
    assert len(seen) == 2 and all(a == b and int(b) >= 20 for a, b in seen), seen
    scored = {name: [tuple(map(int, m)) for m in re.findall(r"(\d+) nodes scored by the host, (\d+) scored again on the device", logs[name])]
              for name in ("native", "host_fixes")}
    print(f"{' '.join(opts)}: nodes scored by the host / again on the device, per sample: {scored}")
    assert "haplotypes selected per window" not in logs["host"]
