"""Position counters of the small-graph path-table drain (PathView::PC, VGMI_PT_POSCOUNT): the drain adds a run's hits
to cells indexed by path position, the read-out sums them with the hash table's counters.  Every test compares ALL counters with the
oracle, bit for bit; VGMI_PT_POSCOUNT=0 (the increments on the hash table's counters, as before) is the A/B reference."""
import os

import numpy as np
import pytest

import oracle_lib as o
from conftest import GOLDEN, get_cohort
from varigraph_amd import vgmi

pytestmark = pytest.mark.gpu

_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTNacgtn", b"TGCANtgcan"):
    _COMP[_a] = _b


def _rc(seq):
    return _COMP[np.frombuffer(bytes(seq), dtype=np.uint8)][::-1].tobytes()


def _block(reads):
    return np.frombuffer(b"".join(bytes(r) + b"\n" for r in reads), dtype=np.uint8).copy()


def _want(keys, k, *blocks):
    t = o.Table(keys)
    for b in blocks:
        t.count_block(b, k)
    return t.counts()


class _Ctx:
    """A fresh context with the keys uploaded, the knob set while the table (and with it the path table) is built."""

    def __init__(self, keys, k, knob_on=True):
        old = os.environ.get("VGMI_PT_POSCOUNT")
        if knob_on:
            os.environ.pop("VGMI_PT_POSCOUNT", None)
        else:
            os.environ["VGMI_PT_POSCOUNT"] = "0"
        try:
            self.c = vgmi.Context(0, buffer_mib=16)
            self.c.table_upload(keys, k)
        finally:
            if old is None:
                os.environ.pop("VGMI_PT_POSCOUNT", None)
            else:
                os.environ["VGMI_PT_POSCOUNT"] = old

    def __enter__(self):
        return self.c

    def __exit__(self, *a):
        self.c.close()


def _count(c, block, n_reads, pieces=1, reset=True):
    """The block in `pieces` submits (cut at read boundaries), no reset in between; all counters."""
    if reset:
        c.counts_reset()
    nl = np.flatnonzero(block == 10)
    assert nl.size == n_reads
    cuts = [0] + [int(nl[(i * n_reads) // pieces - 1]) + 1 for i in range(1, pieces)] + [block.size]
    rd = [0] + [(i * n_reads) // pieces for i in range(1, pieces)] + [n_reads]
    for a, e, ra, re_ in zip(cuts[:-1], cuts[1:], rd[:-1], rd[1:]):
        c.reads_submit(block[a:e], re_ - ra)
    return c.counts_finish()[0]


@pytest.fixture(scope="module")
def c1():
    """The C1 graph, the two haplotypes of its sample 0, 2e5 reads over both strands and their oracle counters (computed once)."""
    co = get_cohort("c1")
    haps = co.haplotypes()
    n = 200_000
    block = vgmi.synth_reads_host(90125, 0, n, 150, haps)
    sites = np.array([int(l.split("\t")[1]) - 1 for l in open(os.path.join(GOLDEN, "c1", "in.vcf")) if not l.startswith("#")])
    alts = [l.split("\t")[4].encode() for l in open(os.path.join(GOLDEN, "c1", "in.vcf")) if not l.startswith("#")]
    from varigraph_amd import synth
    ref = synth.make_reference(co.meta["ref_len"], seed=co.meta["ref_seed"])
    return dict(keys=co.graph.keys, k=co.k, haps=haps, block=block, n=n, want=_want(co.graph.keys, co.k, block), sites=sites, alts=alts, ref=ref)


def test_unsaturated_sample_equals_oracle_and_the_hash_table_counters(c1):
    with _Ctx(c1["keys"], c1["k"]) as c:
        on = _count(c, c1["block"], c1["n"])
    assert np.array_equal(on, c1["want"]), int((on != c1["want"]).sum())
    assert 0 < on.max() < 255 and int(on.astype(np.int64).sum()) > 200_000
    with _Ctx(c1["keys"], c1["k"], knob_on=False) as c:
        off = _count(c, c1["block"], c1["n"])
    assert np.array_equal(off, on)


def _site_read(c1, i, start, length=150, alt=True):
    seq = c1["ref"][start:start + length].copy()
    at = int(c1["sites"][i]) - start
    if alt and 0 <= at < seq.size:
        seq[at] = c1["alts"][i][0]
    return seq.tobytes()


def test_duplicates_in_one_instruction_and_the_crossing(c1):
    """One read across a SNP site and its reverse complement, alternating, 300 times: every lane of an instruction adds to the same
    cells, the hit k-mers end at exactly 255 (the crossing falls inside the position counters: the fast kernel takes all but the
    ragged end of the block), a second launch on top leaves them there, and a reset brings the first result back."""
    i = 500
    r = _site_read(c1, i, int(c1["sites"][i]) - 70)
    block = _block([r, _rc(r)] * 150)
    want = _want(c1["keys"], c1["k"], block)
    assert set(np.unique(want)) == {0, 255} and 27 <= int((want == 255).sum()) <= 124
    for knob_on in (True, False):
        with _Ctx(c1["keys"], c1["k"], knob_on) as c:
            first = _count(c, block, 300)
            assert np.array_equal(first, want), (knob_on, int((first != want).sum()))
            again = _count(c, block, 300, reset=False)
            assert np.array_equal(again, want), (knob_on, int((again != want).sum()))
            back = _count(c, block, 300)
            assert np.array_equal(back, want)
            # ... and below the clamp after the reset: 100 reads, every hit k-mer at exactly 100
            some = _count(c, block[:151 * 100], 100)
            assert np.array_equal(some, _want(c1["keys"], c1["k"], block[:151 * 100])) and set(np.unique(some)) == {0, 100}


def test_partial_masks(c1):
    """Runs that hit only some of their windows: reads that start and end inside a unitig (every offset against the site, several
    lengths), a non-base inside the run, and reads through two SNPs less than 27 bp apart (four allele combinations: places 2 and 3 of
    the index entry) -- both strands, in the rows of the fast kernel."""
    sites, ref = c1["sites"], c1["ref"]
    close = np.flatnonzero(np.diff(sites) < 27)
    assert close.size >= 1      # (C1: 64172 / 64197 and 797515 / 797541)
    rng = np.random.default_rng(11)
    reads = []
    for i in rng.choice(np.arange(5, sites.size - 5), size=60, replace=False):      # (not the first sites: a read starts 149 bases in front)
        for alt in (False, True):
            for start in range(int(sites[i]) - 149, int(sites[i]) + 1, 9):
                length = int(rng.choice([150, 150, 97, 61, 40]))
                reads.append(_site_read(c1, int(i), start + (150 - length) * int(rng.integers(0, 2)), length, alt))
    for i in close:
        for a0 in (False, True):
            for a1 in (False, True):
                lo = int(sites[i]) - 200
                seq = ref[lo:lo + 500].copy()
                if a0:
                    seq[sites[i] - lo] = c1["alts"][i][0]
                if a1:
                    seq[sites[i + 1] - lo] = c1["alts"][i + 1][0]
                for start in range(60, 200 + int(sites[i + 1] - sites[i]) - 8, 7):
                    reads.append(seq[start:start + 150].tobytes())
    reads = [r if j % 2 == 0 else _rc(r) for j, r in enumerate(reads)]
    with_n = []
    for r in reads:
        b = bytearray(r)
        b[int(rng.integers(0, len(b)))] = ord("N")
        with_n.append(bytes(b))
    reads = reads + with_n
    reads = [reads[j] for j in rng.permutation(len(reads))]
    assert 4000 < len(reads) < 20_000
    block = _block(reads)
    want = _want(c1["keys"], c1["k"], block)
    assert int(want.astype(np.int64).sum()) > 30_000 and 0 < want.max() < 255, (int(want.astype(np.int64).sum()), int(want.max()))
    with _Ctx(c1["keys"], c1["k"]) as c:
        got = _count(c, block, len(reads))
    assert np.array_equal(got, want), int((got != want).sum())
    with _Ctx(c1["keys"], c1["k"], knob_on=False) as c:
        assert np.array_equal(_count(c, block, len(reads)), want)


def test_several_pieces_give_one_result(c1):
    with _Ctx(c1["keys"], c1["k"]) as c:
        for pieces in (1, 3, 7):
            got = _count(c, c1["block"], c1["n"], pieces=pieces)
            assert np.array_equal(got, c1["want"]), (pieces, int((got != c1["want"]).sum()))


def test_counters_travel_as_the_sum_of_both_cells(c1):
    """Export, reset, import, finish == the direct finish; more reads on top of an import, exported == the oracle on the concatenation."""
    import torch
    keys, k = c1["keys"], c1["k"]
    half = 100_000
    b0, b1 = c1["block"][:151 * half], c1["block"][151 * half:]
    # deep k-mers too: the crossing read of the test above, so the clamp matters
    r = _site_read(c1, 500, int(c1["sites"][500]) - 70)
    deep = _block([r, _rc(r)] * 100)
    b0 = np.concatenate([b0, deep])
    b1 = np.concatenate([b1, deep])
    want0 = _want(keys, k, b0)
    want01 = _want(keys, k, b0, b1)
    assert (want01 == 255).any() and not (want0 == 255).any()
    with _Ctx(keys, k) as c:
        direct = _count(c, b0, half + 200)
        assert np.array_equal(direct, want0)
        ext = torch.empty(keys.size, dtype=torch.int32, device="cuda")
        c.counts_export_device(ext)
        assert np.array_equal(ext.cpu().numpy().astype(np.int64), want0.astype(np.int64))
        c.counts_reset()
        assert not c.counts_finish()[0].any()
        c.counts_import_device(ext)
        assert np.array_equal(c.counts_finish()[0], want0)
        got = _count(c, b1, half + 200, reset=False)
        assert np.array_equal(got, want01), int((got != want01).sum())
        c.counts_export_device(ext)
        assert np.array_equal(np.minimum(ext.cpu().numpy().astype(np.int64), 255), want01.astype(np.int64))
        # an import replaces what both cells held
        c.counts_import_device(torch.zeros_like(ext))
        assert not c.counts_finish()[0].any()


def _snp_graph(k, seed):
    """A 100 kb reference with a SNP per kilobase, two haplotypes (the C2 shape, small: the LDS-resident fast path of every k)."""
    from varigraph_amd import synth
    rng = np.random.default_rng(seed)
    ref = synth.make_reference(100_000, seed=seed)
    pos = np.sort(rng.choice(np.arange(100, ref.size - 100), size=100, replace=False))
    alts = synth._ACGT[(synth._CODE[ref[pos]] + rng.integers(1, 4, size=pos.size)) % 4]
    hap1 = ref.copy()
    hap1[pos] = alts
    return np.unique(vgmi.synth_snp_keys(ref, pos, alts, k)), [ref, hap1], pos


@pytest.mark.parametrize("k", [21, 22])
def test_other_k_unsaturated_and_crossing(k):
    """k = 21: 8 windows per run on the grid of 8.  k = 22: even k, the debit pass in front of the fast kernel (its debits stand in
    counts[slot] while the drain adds to the position counters: the read-out is the sum of both, mod 2^32) -- the crossing read starts
    with two k-mers that are their own reverse complement, the shapes that pass looks for (the reads built to be debited, saturated:
    test_small_graph_even_k_run_counter_lag_is_taken_back in test_gpu_parity.py)."""
    keys, haps, pos = _snp_graph(k, 40 + k)
    rng = np.random.default_rng(k)
    body = haps[1][pos[50] - 60:pos[50] + 60].tobytes()
    if k % 2 == 0:
        h0, h1 = (bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=k // 2)) for _ in range(2))
        r = h0 + _rc(h0) + h1 + _rc(h1) + body      # (the key set holds its windows)
        keys = np.unique(np.concatenate([keys, o.sketch(r, k), o.sketch(r[1:], k), o.sketch(b"G" + r, k)]))
        keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
    else:
        r = body
    assert 1000 < keys.size <= 65536
    n = 40_000
    shallow = vgmi.synth_reads_host(7 + k, 0, n, 150, haps)
    crossing = _block([r, _rc(r)] * 150)
    want_s = _want(keys, k, shallow)
    want_c = _want(keys, k, crossing)
    assert 0 < want_s.max() < 255 and (want_c == 255).any()
    got = {}
    for knob_on in (True, False):
        with _Ctx(keys, k, knob_on) as c:
            got[knob_on] = (_count(c, shallow, n, pieces=3), _count(c, crossing, 300), _count(c, crossing, 300, reset=False))
    want_cc = _want(keys, k, crossing, crossing)
    for knob_on in (True, False):
        s, c1_, c2_ = got[knob_on]
        assert np.array_equal(s, want_s), (k, knob_on, int((s != want_s).sum()))
        assert np.array_equal(c1_, want_c), (k, knob_on, int((c1_ != want_c).sum()), c1_[c1_ != want_c][:8], want_c[c1_ != want_c][:8])
        assert np.array_equal(c2_, want_cc), (k, knob_on, int((c2_ != want_cc).sum()))
