"""The tallies of a polyploid call on the device (vgmi_hmm_tallies_ploidy: ploidy 3 and 4): the kernel against posterior()'s tallies
(src/genotype.cpp:1387-1414) spelled out in numpy -- 32-bit integer sums, so every number is exact --, the refusals, and the command line on
both device emission paths (whole panel, haplotypes selected per window) against the committed fixture, the deterministic build of the
reference and the host's walk (VGH_DEVICE_TALLIES=0)."""
import gzip
import os
import re

import numpy as np
import pytest

from test_gpu_hmm_select_ploidy import polyploid_cohort      # noqa: F401  (that module's fixture: 17 haplotypes, three samples in one run)
from varigraph_amd import vgmi

pytestmark = pytest.mark.gpu

N_HAP, N_GT, PER_WINDOW = 47, 5, 70
WIN_N_GT = [1, 3, 5, 5]
TALLY_LINE = r"HMM tallies on the device: (\d+) rows, ploidy (\d+)"


def _model(ploidy, f, bits, cov, alive, win_n_gt, win_haps, win_sel_mask, entry_begin, counts, row_win, winner):
    """alive None: every entry counts"""
    n_rows = len(counts)
    out = np.zeros((n_rows, 2 * ploidy), dtype=np.uint32)
    uniq = np.zeros(n_rows, dtype=np.uint8)
    for r in range(n_rows):
        w, g = int(row_win[r]), int(winner[r])
        if g >= win_n_gt[w]:
            continue
        ids = [int(h) for h in win_haps[w][g]]
        ok = [h < 64 and (int(win_sel_mask[w]) >> h) & 1 == 1 for h in ids]
        u = 0
        for j in range(int(entry_begin[r]), int(entry_begin[r]) + int(counts[r])):
            if alive is not None and not alive[j]:
                continue
            if f[j] <= 1 and u < 255:
                u += 1
            for q in range(ploidy):
                if ok[q] and (int(bits[j]) >> ids[q]) & 1:
                    out[r, 2 * q] += 1
                    out[r, 2 * q + 1] += int(cov[j])
        uniq[r] = u
    return out, uniq


def _case(ploidy):
    """four windows of 70 rows with 1, 3, 5 and 5 genotypes; 47 haplotypes in 6 bytes of bits"""
    rng = np.random.default_rng(4100 + ploidy)
    n_windows = len(WIN_N_GT)
    n_rows = n_windows * PER_WINDOW                          # 280: 17 workgroups of 16 rows and a half
    counts = rng.integers(0, 71, size=n_rows)
    counts[[3, 4, 75, 279]] = 0
    counts[7] = 400
    counts[10], counts[11] = 64, 65
    special = [71, 73, 141, 142, 143, 211]                   # rows whose genotype is set below: none a multiple of 9
    counts[special] = rng.integers(20, 71, size=len(special))
    entry_begin = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
    n_entries = int(counts.sum())
    f = rng.choice([0, 1, 1, 2, 3], size=n_entries).astype(np.uint64)
    bits = rng.integers(0, 1 << 47, size=n_entries, dtype=np.uint64) | rng.integers(0, 1 << 47, size=n_entries, dtype=np.uint64)
    cov = rng.integers(0, 256, size=n_entries).astype(np.uint8)
    alive = (rng.random(n_entries) < 0.7).astype(np.uint8)
    lo = int(entry_begin[7])
    f[lo:lo + 400], cov[lo:lo + 400], alive[lo:lo + 400] = 1, 255, 1
    bits[lo:lo + 400] |= np.uint64(1)                        # haplotype 0 carries all 400
    entries = (f << np.uint64(8)) | (bits << np.uint64(16))
    row_win = np.repeat(np.arange(n_windows), PER_WINDOW).astype(np.uint32)

    def blk(a):
        return tuple(range(a, a + ploidy))
    zero, rep = (0,) * ploidy, (0,) * (ploidy - 1) + (5,)
    lists = [[zero, blk(20), blk(24), blk(28), blk(32)],
             [rep, blk(5), blk(9), blk(13), blk(36)],
             [blk(1), blk(13), blk(17), blk(47 - ploidy), zero],
             [blk(47 - ploidy), blk(33), rep, blk(1), blk(9)]]
    win_haps = np.array(lists, dtype=np.uint8)
    assert win_haps.shape == (n_windows, N_GT, ploidy) and win_haps.max() == 46
    masks = []
    for w in range(n_windows):
        m = 0
        for g in range(WIN_N_GT[w]):
            for h in lists[w][g]:
                m |= 1 << h
        masks.append(m)
    masks[2] &= ~(1 << 18)                                   # window 2, genotype 2 = 17, 18, 19 ..: 18 was not drawn
    win_sel_mask = np.array(masks, dtype=np.uint64)
    winner = rng.integers(0, N_GT, size=n_rows).astype(np.uint32)      # (windows 0 and 1 have fewer: those rows read zeros)
    winner[::9] = 0xFFFFFFFF
    winner[7] = 0
    winner[10], winner[11] = 0, 0
    winner[71], winner[73] = 0, 4                            # window 1: (0, .., 0, 5); 4 < n_gt but >= the window's 3
    winner[141], winner[142], winner[143] = 2, 3, 4          # window 2: an id outside the mask; id 46; the all-zero block
    winner[211] = 0                                          # window 3: id 46
    return dict(f=f, bits=bits, cov=cov, alive=alive, entries=entries, entry_begin=entry_begin, counts=counts, row_win=row_win, win_haps=win_haps,
                win_sel_mask=win_sel_mask, winner=winner)


@pytest.mark.parametrize("ploidy", [3, 4])
def test_tallies_of_a_polyploid_call_equal_the_host_walk(ploidy):
    """Every number of every row against the model: rows without entries, of 64 and of 65 entries (one turn of a wavefront, one and a
    lane), 400 single-copy k-mers of coverage 255 (unique stops at 255, the sum passes 16 bits), dead entries that count for nothing,
    rows without a call, a winner beyond its window's count, genotypes that repeat an id, an id that was not drawn, id 46.  Then the
    whole-panel form: one window, every haplotype selected, no alive bytes -- the dead entries count."""
    c = _case(ploidy)
    n_rows = len(c["counts"])
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        ctx.hmm_entries_upload(c["entries"], c["cov"], c["alive"])
        out, uniq = ctx.hmm_tallies_ploidy(ploidy, c["win_haps"], c["win_sel_mask"], c["entry_begin"], c["counts"], c["winner"], row_win=c["row_win"],
                                           win_n_gt=WIN_N_GT, use_alive=True)
        panel_haps = c["win_haps"][2:3]
        all_haps = np.array([(1 << N_HAP) - 1], dtype=np.uint64)
        out_p, uniq_p = ctx.hmm_tallies_ploidy(ploidy, panel_haps, all_haps, c["entry_begin"], c["counts"], c["winner"], use_alive=False)
    finally:
        ctx.close()
    assert out.shape == (n_rows, 2 * ploidy) and out.dtype == np.uint32 and uniq.shape == (n_rows,) and uniq.dtype == np.uint8
    want, want_u = _model(ploidy, c["f"], c["bits"], c["cov"], c["alive"], WIN_N_GT, c["win_haps"], c["win_sel_mask"], c["entry_begin"], c["counts"],
                          c["row_win"], c["winner"])
    bad = np.flatnonzero((out != want).any(axis=1) | (uniq != want_u))
    assert bad.size == 0, (bad[:10], out[bad[:3]], want[bad[:3]], uniq[bad[:3]], want_u[bad[:3]])
    # the cases the issue names are in the data, and read as they must
    assert uniq[7] == 255 and out[7].tolist() == [400, 102_000] * ploidy
    assert c["counts"][10] == 64 and c["counts"][11] == 65 and out[10].any() and out[11].any()
    assert not out[::9].any() and not uniq[::9].any() and out[1::9].any()
    assert not out[73].any() and uniq[73] == 0 and c["winner"][73] < N_GT
    beyond = c["winner"][:PER_WINDOW] < N_GT
    assert (c["winner"][:PER_WINDOW][beyond] >= 1).sum() > 20 and not out[:PER_WINDOW][c["winner"][:PER_WINDOW] >= 1].any()
    assert len(set(out[71, 0:2 * ploidy - 2:2])) == 1 and out[71, 0] > 0 and out[71, 2 * ploidy - 2] > 0         # (0, .., 0, 5): every place tallied
    assert out[141, 0] > 0 and out[141, 2:4].tolist() == [0, 0] and out[141, 4] > 0                                   # 18 was not drawn
    assert out[142, 2 * ploidy - 2] > 0 and out[211, 2 * ploidy - 2] > 0                                              # id 46
    assert len(set(out[143, 0::2])) == 1 and len(set(out[143, 1::2])) == 1 and out[143, 0] > 0                         # the all-zero block
    dead = c["alive"] == 0
    assert 0.25 < dead.mean() < 0.35
    # the whole-panel form
    want_p, want_pu = _model(ploidy, c["f"], c["bits"], c["cov"], None, [N_GT], panel_haps, all_haps, c["entry_begin"], c["counts"],
                             np.zeros(n_rows, dtype=np.uint32), c["winner"])
    assert np.array_equal(out_p, want_p) and np.array_equal(uniq_p, want_pu)
    alive_only, _ = _model(ploidy, c["f"], c["bits"], c["cov"], c["alive"], [N_GT], panel_haps, all_haps, c["entry_begin"], c["counts"],
                           np.zeros(n_rows, dtype=np.uint32), c["winner"])
    assert int(out_p[:, 0::2].sum()) > int(alive_only[:, 0::2].sum()) and not out_p[::9].any()


def test_refusals_leave_the_context_usable():
    """ploidy 5, 129 genotypes, a row in a window that does not exist, a window with more genotypes than the lists are wide, a call before
    the entries are there: each an error, and the valid call that follows answers as before."""
    c = _case(4)
    args = (c["win_haps"], c["win_sel_mask"], c["entry_begin"], c["counts"], c["winner"])
    want, want_u = _model(4, c["f"], c["bits"], c["cov"], c["alive"], WIN_N_GT, c["win_haps"], c["win_sel_mask"], c["entry_begin"], c["counts"], c["row_win"],
                          c["winner"])
    ctx = vgmi.Context(0, buffer_mib=16)
    try:
        with pytest.raises(vgmi.VgmiError) as e:
            ctx.hmm_tallies_ploidy(4, *args, row_win=c["row_win"], win_n_gt=WIN_N_GT)
        assert e.value.code == -4                             # VGMI_E_STATE: nothing uploaded
        ctx.hmm_entries_upload(c["entries"], c["cov"], c["alive"])

        def valid():
            out, uniq = ctx.hmm_tallies_ploidy(4, *args, row_win=c["row_win"], win_n_gt=WIN_N_GT)
            assert np.array_equal(out, want) and np.array_equal(uniq, want_u)
        valid()
        haps5 = np.zeros((4, N_GT, 5), dtype=np.uint8)
        haps129 = np.zeros((4, 129, 4), dtype=np.uint8)
        row_win_bad = c["row_win"].copy()
        row_win_bad[200] = 4
        for bad in (lambda: ctx.hmm_tallies_ploidy(5, haps5, *args[1:], row_win=c["row_win"], win_n_gt=WIN_N_GT),
                    lambda: ctx.hmm_tallies_ploidy(4, haps129, *args[1:], row_win=c["row_win"], win_n_gt=WIN_N_GT),
                    lambda: ctx.hmm_tallies_ploidy(4, *args, row_win=row_win_bad, win_n_gt=WIN_N_GT),
                    lambda: ctx.hmm_tallies_ploidy(4, *args, row_win=c["row_win"], win_n_gt=[1, 3, 6, 5])):
            with pytest.raises(vgmi.VgmiError) as e:
                bad()
            assert e.value.code == -1                         # VGMI_E_INVALID
            valid()
    finally:
        ctx.close()


def test_command_line_whole_panel_tetraploid_is_tallied_on_the_device(tmp_path):
    """tests/golden/cohort_tetra has 13 haplotypes: the default -n 15 selects them all, the whole-panel device path.  The VCF is the
    committed one (GQ aside: x87 transcendentals differ between CPU vendors), the VGH_TIMING log says the calls were tallied on the device,
    and VGH_DEVICE_TALLIES=0 -- the host's walk -- writes the same bytes without that line."""
    from conftest import GOLDEN
    from test_gpu_integration import CLI, _missing, _run, _strip_gq
    if not os.path.exists(CLI):
        _missing("varigraph-mi not built (python -m varigraph_amd.build)")
    d = os.path.join(GOLDEN, "cohort_tetra")
    graph = tmp_path / "graph.bin"
    graph.write_bytes(gzip.open(os.path.join(d, "graph.bin.gz"), "rb").read())
    fq = [os.path.join(d, f"reads_{i}.fq.gz") for i in (1, 2)]
    got, logs = {}, {}
    for name, more in (("device", {}), ("host", {"VGH_DEVICE_TALLIES": "0"})):
        work = tmp_path / name
        work.mkdir()
        (work / "samples.cfg").write_text("sample0 " + " ".join(fq) + "\n")
        env = dict(os.environ, VGH_RANDOM_DEVICE_VALUE="20241022", VGH_TIMING="1", **more)
        r = _run([CLI, "genotype", "--load-graph", str(graph), "-s", "samples.cfg", "-t", "4", "--gpu", "0", "--buffer", "8", "--sample-ploidy", "4",
                  "--use-depth"], cwd=work, capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got[name] = gzip.open(work / "sample0.varigraph.vcf.gz", "rb").read()
        logs[name] = r.stderr
    want = open(os.path.join(d, "expected_p4_use_depth.vcf"), "rb").read()
    assert _strip_gq(got["device"]) == _strip_gq(want)
    seen = re.findall(TALLY_LINE, logs["device"])
    assert len(seen) == 1 and int(seen[0][0]) > 0 and seen[0][1] == "4", logs["device"][-2000:]
    assert got["host"] == got["device"]
    assert not re.search(TALLY_LINE, logs["host"])


@pytest.mark.parametrize("opts", [["--sample-ploidy", "4", "-n", "5"], ["--sample-ploidy", "3", "-n", "4", "--sv"]], ids=["p4n5", "p3n4sv"])
def test_command_line_polyploid_with_selection_is_tallied_on_the_device(opts, polyploid_cohort):      # noqa: F811
    """Three samples in one run, haplotypes selected per window: every VCF is the deterministic reference build's byte for byte (at least
    100 lines each), with the device's tallies, with the host's walk (VGH_DEVICE_TALLIES=0) and when the first sample was refused the device
    (VGH_HMM_FAKE_NOMEM=1: it takes the pool, the next two start from the host's lists); the log names the device's tallies once per sample
    that had them."""
    from test_gpu_configs import CLI, ENV, REF, _run, _vcf
    work, graph, cfg = polyploid_cohort
    ploidy = opts[1]
    opts = opts + ["--use-depth", "--granularity", "0.01"]
    tag = "tally_" + "_".join(o.strip("-") for o in opts[:6])
    outs, logs = {}, {}
    for name, exe, more, env in (("cpu", REF, [], ENV), ("native", CLI, ["--gpu", "0"], dict(ENV, VGH_TIMING="1")),
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
    for name in ("native", "host_tallies", "host_first"):
        for i in range(3):
            assert outs[name][i] == outs["cpu"][i], (opts, name, i)
    seen = {name: re.findall(TALLY_LINE, logs[name]) for name in logs}
    print(f"{' '.join(opts)}: rows tallied on the device per sample: {seen}")
    assert len(seen["native"]) == 3 and all(int(rows) > 0 and p == ploidy for rows, p in seen["native"]), seen
    assert seen["host_tallies"] == [] and seen["cpu"] == []
    assert len(seen["host_first"]) == 2 and all(int(rows) > 0 and p == ploidy for rows, p in seen["host_first"]), seen
