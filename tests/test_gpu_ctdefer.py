"""Deferred counter updates of the context-table count kernels (varigraph_amd/csrc/vgmi_ctdefer.hip) under test (-m gpu).

(a) ctd_scatter_kernel / ctd_accumulate_kernel by themselves, on seeded records, against a plain 64-bit loop on the host
    (tests/native/ctdefer_check.hip): the region geometries the product's own graphs do not reach -- regions of 32 768 counters, more
    regions than accumulate workgroups, odd region sizes, the 256-counter clamp, the largest table served, rooms and a record buffer that
    overflow, a scratch used twice.
(b) countkc_defer_kernel<K> + those two through the C ABI against the oracle, where the matrix of test_gpu_parity.py does not go: small
    graphs (k = 26, 28), reads that pile onto few counters, launches that add up on a scratch that grows, a table replaced on a live
    context.  Every case asserts through Context.ctable_defer_info() that its launches deferred: a silent fall-back checks nothing.
Everything is integer work: equality is exact."""
import numpy as np
import pytest

import oracle_lib as o
import test_gpu_parity as parity
from conftest import block_from_seqs
from ctdefer_harness import build_harness, run_harness
from varigraph_amd import vgmi

pytestmark = pytest.mark.gpu

DEFER = {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_harness(tmp_path_factory.mktemp("ctdefer"))


def _n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


# ----------------------------------------------------------------------------- (a) the two kernels behind the row loop
# case -> launches it makes
CASES = {"uniform-32768": 1, "two-rounds": 1, "max-table": 1, "tiny": 2, "pile-up": 1, "rooms-of-8": 1, "cursor": 4, "reuse": 2}


@pytest.mark.parametrize("case", list(CASES))
def test_scatter_and_accumulate_match_a_plain_loop(exe, case):
    """Every counter after launch_ctd_apply == its seeded start value + what a loop over the records adds, and the words behind the
    last counter are untouched.  The harness exits non-zero on the first HIP error, on any difference and when a case does not reach
    what it is for (pile-up / rooms-of-8: no room overflowed)."""
    rc, out, err = run_harness(exe, ["apply", case], timeout=600)
    for line in out:
        print(line)
    assert rc == 0, (rc, err, [x.get("first") for x in out])
    assert len(out) == CASES[case] and all(x["differences"] == 0 for x in out), out
    n_cu = out[0]["n_cu"]
    assert all(x["n_wg"] == n_cu & ~1 for x in out)
    shape = [(x["n_counts"], x["n_bins"], x["region"]) for x in out]
    if case == "tiny":
        assert [x["n_counts"] for x in out] == [300, 5000] and all(x["region"] == 256 for x in out), shape
        assert (out[0]["n_bins"], out[1]["n_bins"]) == (2, 20)
    elif case == "max-table":
        assert shape == [(67_108_864, 2048, 32768)]
    elif n_cu == 256:
        want = {"uniform-32768": (8_388_608, 256, 32768), "two-rounds": (8_388_609, 512, 16385), "pile-up": (8_388_608, 256, 32768),
                "reuse": (8_388_609, 512, 16385), "rooms-of-8": (1_800_000, 256, 7032), "cursor": (1_800_000, 256, 7032)}[case]
        assert all(s == want for s in shape), shape
    if case in ("two-rounds", "reuse", "max-table"):
        assert all(x["n_bins"] > n_cu for x in out)      # a workgroup of the accumulate kernel goes round its loop again
    if case == "tiny":
        assert all(x["n_bins"] < n_cu for x in out)
    if case in ("pile-up", "rooms-of-8"):
        assert out[0]["rooms_overflowed"] > 0 and out[0]["fullest_room"] > out[0]["room"], out
    if case == "rooms-of-8":
        assert out[0]["room"] == 8
    if case == "cursor":
        cap = out[0]["cap"]
        assert cap == 40448 and [(x["cursor"], x["applied"]) for x in out] == [(0, 0), (256, 256), (cap, cap), (cap + 768, cap)], out
        assert out[0]["increments"] == 0 and out[0]["records_binned"] == 0
    if case == "reuse":
        assert out[1]["applied"] < out[0]["applied"] // 10 and out[1]["records_binned"] < out[0]["records_binned"] // 10, out
    assert all(x["increments"] > 0 for x in out if x["applied"])


# ----------------------------------------------------------------------------- (b) through the C ABI, against the oracle
def _submit_device(c, block, n_reads, k):
    """One launch over the block resident on the device (even k: the reads' offsets come with the block)."""
    import torch
    d = torch.from_numpy(block).cuda()
    d_off = None
    if k % 2 == 0:
        d_off = torch.from_numpy(np.concatenate([[0], np.flatnonzero(block == 10) + 1]).astype(np.int64)).cuda()
        assert d_off.numel() == n_reads + 1
    c.reads_submit_device(d, block.size, n_reads, d_off)
    torch.cuda.synchronize()
    return d, d_off      # (alive until the caller has fetched the counters)


def _deferred_since(c, before, launches):
    di = c.ctable_defer_info()
    assert (di["deferred_launches"] - before["deferred_launches"], di["plain_launches"] - before["plain_launches"]) == (launches, 0), (before, di)
    return di


@pytest.mark.parametrize("kind", ["plain", "repeats"])
@pytest.mark.parametrize("k", [26, 28])
def test_small_graph_deferred_matches_oracle(kind, k, monkeypatch):
    """k = 26 / 28 take the context table at any size: a table of a few ten thousand counters is cut into regions of 256 (the clamp), fewer
    than there are CUs, so the accumulate kernel's grid is the number of regions.  The graphs and reads of
    test_small_graph_other_odd_k_fast_path_matches_oracle, host-staged pieces and one device-resident launch."""
    for name, val in DEFER.items():
        monkeypatch.setenv(name, val)
    rng = np.random.default_rng({"plain": 1, "repeats": 2}[kind] + k)
    keys, haps = parity._small_graph(kind, rng, k)
    assert 1000 < keys.size <= 65536, keys.size
    n_reads = 60_000
    block = vgmi.synth_reads_host(23 + k, 0, n_reads, 150, haps)
    t = o.Table(keys)
    t.count_block(block, k)
    want = t.counts()
    c = vgmi.Context(0, buffer_mib=16)
    try:
        c.table_upload(keys, k)
        assert c.ctable_info()["n_buckets"] > 0
        before = c.ctable_defer_info()
        c.counts_reset()
        cuts = [0, 16 * 1000, 16 * 1000 + 16 * 37, n_reads]
        for a, e in zip(cuts[:-1], cuts[1:]):
            c.reads_submit(block[a * 151:e * 151], e - a)
        cov, _, _ = c.counts_finish()
        assert np.array_equal(cov, want), (kind, k, int((cov != want).sum()))
        di = _deferred_since(c, before, 3)
        assert di["deferred_launches"] > 0 and di["region"] == 256 and 1 <= di["n_bins"] < _n_cu(), di
        assert di["n_bins"] * 256 >= keys.size
        c.counts_reset()
        keep = _submit_device(c, block, n_reads, k)
        cov_d, _, _ = c.counts_finish()
        del keep
        assert np.array_equal(cov_d, want), (kind, k, "device")
        _deferred_since(c, di, 1)
        assert int(cov.astype(np.int64).sum()) > 50_000
    finally:
        c.close()


_PILE_UP = {}


def _pile_up_case(k):
    """The large-graph matrix's graph; 100 000 ordinary reads plus 40 000 copies of each of three reads of the other haplotype that cross SNP
    sites, one of them reverse-complemented: their runs pile onto three stretches of counters, which saturate."""
    if k not in _PILE_UP:
        keys, ref, hap1, pos = parity._large_graph(k)
        n_reads = 100_000
        block = vgmi.synth_reads_host(9, 0, n_reads, 150, [ref, hap1])
        comp = np.zeros(256, dtype=np.uint8)
        comp[list(b"ACGT")] = list(b"TGCA")
        hot = [hap1[int(p) - 70:int(p) + 80] for p in (pos[1000], pos[33_000], pos[65_000])]
        hot[1] = comp[hot[1][::-1]]
        hot = block_from_seqs([h.tobytes() for h in hot])
        assert hot.size == 3 * 151
        piled = np.tile(hot, 40_000)
        # ordinary reads in front, between and behind
        block = np.concatenate([block[: 30_000 * 151], piled[: piled.size // 2], block[30_000 * 151:], piled[piled.size // 2:]])
        n_reads += 120_000
        t = o.Table(keys)
        t.count_block(block, k)
        _PILE_UP[k] = (keys, block, n_reads, t.counts())
    return _PILE_UP[k]


@pytest.mark.parametrize("k", [27, 28])
def test_large_graph_pile_up_and_saturation_deferred(k, monkeypatch):
    """Reads that pile onto a few counters: whole tiles of the scatter kernel go to one region (rooms overflow into plain atomics), the
    regions' sums pass the read-out clamp of 255 by far, and the rest of the table is counted as ever.  Default rooms."""
    for name, val in DEFER.items():
        monkeypatch.setenv(name, val)
    keys, block, n_reads, want = _pile_up_case(k)
    assert (want == 255).sum() > 100 and ((want > 0) & (want < 255)).sum() > 100_000
    c = vgmi.Context(0, buffer_mib=16)
    try:
        c.table_upload(keys, k)
        before = c.ctable_defer_info()
        c.counts_reset()
        c.reads_submit(block, n_reads)
        cov, _, _ = c.counts_finish()
        assert np.array_equal(cov, want), int((cov != want).sum())
        launches = c.count_kernel_ms()[1]
        assert launches >= 2
        di = _deferred_since(c, before, launches)
        c.counts_reset()
        keep = _submit_device(c, block, n_reads, k)
        cov2, _, _ = c.counts_finish()
        del keep
        assert np.array_equal(cov2, want), int((cov2 != want).sum())
        _deferred_since(c, di, 1)
    finally:
        c.close()


@pytest.mark.parametrize("k", [27, 24])
def test_launches_add_up_on_a_scratch_that_grows(k, monkeypatch):
    """One context, no reset in between: a 20 000-read block, the 300 000-read block (the stream's scratch is replaced by a larger one), the
    first again (a launch with far fewer records on the large scratch) == the oracle over the three."""
    for name, val in DEFER.items():
        monkeypatch.setenv(name, val)
    keys, block, n_reads, _ = parity._large_graph_case(k)
    small_reads = 20_000
    small = block[: small_reads * 151]
    assert small[-1] == 10
    t = o.Table(keys)
    for b in (small, block, small):
        t.count_block(b, k)
    want = t.counts()
    c = vgmi.Context(0, buffer_mib=16)
    try:
        c.table_upload(keys, k)
        before = c.ctable_defer_info()
        c.counts_reset()
        keep, caps = [], []
        for b, n in ((small, small_reads), (block, n_reads), (small, small_reads)):
            keep.append(_submit_device(c, b, n, k))
            caps.append(c.ctable_defer_info()["cap"])
        cov, _, _ = c.counts_finish()
        del keep
        assert np.array_equal(cov, want), int((cov != want).sum())
        _deferred_since(c, before, 3)
        assert caps[0] < caps[1] and caps[2] == caps[0], caps
        assert c.read_base() == 150 * 2 * small_reads + int((block != 10).sum())
    finally:
        c.close()


def test_table_replaced_on_a_live_context(monkeypatch):
    """The per-stream scratch survives vgmi_table_upload: the k = 27 graph, then the k = 22 graph (other counters, other regions) in the same
    context, then the k = 27 graph again -- each laid out anew on what the one before left there."""
    for name, val in DEFER.items():
        monkeypatch.setenv(name, val)
    c = vgmi.Context(0, buffer_mib=16)
    try:
        shapes = []
        for k in (27, 22, 27):
            keys, block, n_reads, want = parity._large_graph_case(k)
            c.table_upload(keys, k)
            before = c.ctable_defer_info()
            c.counts_reset()
            keep = _submit_device(c, block, n_reads, k)
            cov, _, _ = c.counts_finish()
            del keep
            assert np.array_equal(cov, want), (k, int((cov != want).sum()))
            di = _deferred_since(c, before, 1)
            assert di["n_bins"] * di["region"] >= keys.size
            shapes.append((di["n_bins"], di["region"]))
        assert shapes[0] == shapes[2] and shapes[1] != shapes[0], shapes
    finally:
        c.close()
