"""Done buckets of the small-graph path table (PathView::BKT .. DONE, VGMI_PT_DONE): the count kernel drops a
candidate run whose index bucket is done -- every k-mer the run's windows could equal has reached the clamp.  Every test compares ALL
counters with the oracle, bit for bit, gives the same counters with VGMI_PT_DONE=0, and asks vgmi_pt_done_check, which recomputes
the property from the index, the k-mer-start bits and the saturation bits alone: no bucket is marked done that is not fully saturated,
and (the stream idle) none that is fully saturated is left unmarked."""
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


def _clamped(*terms):
    """min(255, sum of times x counters): what submits of blocks whose single-pass counters are known add up to"""
    s = sum(int(times) * c.astype(np.int64) for times, c in terms)
    return np.minimum(s, 255).astype(np.uint8)


class _Ctx:
    """A fresh context with the keys uploaded, the knobs set while the table (and with it the path table) is built."""

    def __init__(self, keys, k, done=True, env=None):
        knobs = dict(env or {})
        knobs["VGMI_PT_DONE"] = None if done else "0"
        old = {n: os.environ.get(n) for n in knobs}
        for n, v in knobs.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
        try:
            self.c = vgmi.Context(0, buffer_mib=16)
            self.c.table_upload(keys, k)
        finally:
            for n, v in old.items():
                if v is None:
                    os.environ.pop(n, None)
                else:
                    os.environ[n] = v

    def __enter__(self):
        return self.c

    def __exit__(self, *a):
        self.c.close()


def _submit(c, block, times=1):
    n = int((block == 10).sum())
    for _ in range(times):
        c.reads_submit(block, n)
    return c.counts_finish()[0]


def _check(c, done=True):
    """(can become done, marked done) once the two violation counts have been looked at"""
    can, marked, wrong, missed = c.pt_done_check()
    assert wrong == 0, (can, marked, wrong, missed)
    if done:
        assert missed == 0, (can, marked, wrong, missed)
    else:
        assert marked == 0
    assert marked <= can
    return can, marked


@pytest.fixture(scope="module")
def c1():
    """The C1 graph, the two haplotypes of its sample 0, 2e5 reads over both strands and their oracle counters (computed once)."""
    co = get_cohort("c1")
    haps = co.haplotypes()
    n = 200_000
    block = vgmi.synth_reads_host(90125, 0, n, 150, haps)
    vcf = [l.split("\t") for l in open(os.path.join(GOLDEN, "c1", "in.vcf")) if not l.startswith("#")]
    sites = np.array([int(f[1]) - 1 for f in vcf])
    alts = [f[4].encode() for f in vcf]
    from varigraph_amd import synth
    ref = synth.make_reference(co.meta["ref_len"], seed=co.meta["ref_seed"])
    want = _want(co.graph.keys, co.k, block)
    assert 0 < want.max() < 255
    return dict(keys=co.graph.keys, k=co.k, block=block, want=want, sites=sites, alts=alts, ref=ref)


def _saturate_across_launches(keys, k, block, want, done, env=None):
    """Ten submits without a reset; submits up to 260, where every k-mer the block holds at all has passed the clamp; one more; a reset
    and one pass.  Returns the counters after each part and the done count of the saturated graph.

    (Ten submits of a block whose deepest k-mer stands at 24 after one pass -- the 2e5-read C1 block -- take no counter to 255: ten
    times the single-pass counters is what they are compared with, no bucket can be done then and the check must say so.  The graph
    saturates at 255 submits; the block stays on the device for them.)"""
    import torch
    n = int((block == 10).sum())
    d_block = torch.from_numpy(block).cuda()
    d_off = None
    if k % 2 == 0:      # even k counts read by read: where the reads start
        off = np.concatenate([[0], np.flatnonzero(block == 10) + 1]).astype(np.int64)
        d_off = torch.from_numpy(off).cuda()
    with _Ctx(keys, k, done, env) as c:
        def more(times):
            for _ in range(times):
                c.reads_submit_device(d_block, d_block.numel(), n, d_off)
            return c.counts_finish()[0]
        c.counts_reset()
        ten = more(10)
        assert np.array_equal(ten, _clamped((10, want))), int((ten != _clamped((10, want))).sum())
        assert _check(c, done)[1] == 0 or (ten == 255).any()
        deep = more(250)
        assert np.array_equal(deep, _clamped((260, want))) and set(np.unique(deep)) <= {0, 255}
        can, marked = _check(c, done)
        if done:
            assert 0 < marked <= can
        assert np.array_equal(more(1), deep)
        assert _check(c, done) == (can, marked)
        c.counts_reset()
        assert _check(c, done)[1] == 0
        one = _submit(c, block)
        assert np.array_equal(one, want), int((one != want).sum())
        assert _check(c, done)[1] == 0
        return ten, deep, one, marked


@pytest.mark.parametrize("env", [{}, {"VGMI_PT_POSCOUNT": "0"}], ids=["position-counters", "hash-table-counters"])
def test_whole_graph_saturates_across_launches(c1, env):
    on = _saturate_across_launches(c1["keys"], c1["k"], c1["block"], c1["want"], True, env)
    off = _saturate_across_launches(c1["keys"], c1["k"], c1["block"], c1["want"], False, env)
    assert all(np.array_equal(a, b) for a, b in zip(on[:3], off[:3]))
    assert on[3] > 10_000      # (most of the 7e4 twelve-mers of the graph: only the buckets of the six k-mers the sample lacks, and the flagged ones, stay open)


def _site_read(c1, i, start, length=150, alt=True, also=None):
    seq = c1["ref"][start:start + length].copy()
    for j, a in ((i, alt),) + ((also,) if also else ()):
        at = int(c1["sites"][j]) - start
        if a and 0 <= at < seq.size:
            seq[at] = c1["alts"][j][0]
    return seq.tobytes()


def test_partial_saturation_leaves_the_other_allele_counting(c1):
    """300 reads over one SNP site with the reference allele (both strands): the buckets of 12-mers that lie on the reference allele
    alone become done, those with a place on either allele do not -- the check finds none marked with an unsaturated k-mer under it.
    Reads with the alternative allele then count exactly, at that site and at two sites less than 27 bp apart (four places an entry)."""
    sites = c1["sites"]
    i = 500
    close = int(np.flatnonzero(np.diff(sites) < 27)[0])      # (C1: 64172 / 64197)
    first = []
    for j, also in ((i, None), (close, (close + 1, False))):
        r = _site_read(c1, j, int(sites[j]) - 70, alt=False, also=also)
        first += [r, _rc(r)] * 150
    second = []
    for a0, a1 in ((True, False), (False, True), (True, True)):
        r = _site_read(c1, close, int(sites[close]) - 70, alt=a0, also=(close + 1, a1))
        second += [r, _rc(r)] * 20
    r = _site_read(c1, i, int(sites[i]) - 70, alt=True)
    second += [r, _rc(r)] * 50
    b1, b2 = _block(first), _block(second)
    want1, want12 = _want(c1["keys"], c1["k"], b1), _want(c1["keys"], c1["k"], b1, b2)
    assert set(np.unique(want1)) == {0, 255} and {40, 100} <= set(np.unique(want12))
    got = {}
    for done in (True, False):
        with _Ctx(c1["keys"], c1["k"], done) as c:
            c.counts_reset()
            g1 = _submit(c, b1)
            can, marked = _check(c, done)
            if done:
                # a site's 12-mers: 12 on each allele alone, the others (15 a side) on both; nothing else of the graph is saturated
                assert 0 < marked <= 2 * 2 * 12 + 4
            g2 = _submit(c, b2)
            _check(c, done)
            got[done] = (g1, g2)
        assert np.array_equal(got[done][0], want1), (done, int((got[done][0] != want1).sum()))
        assert np.array_equal(got[done][1], want12), (done, int((got[done][1] != want12).sum()))


def _snp_graph(k, seed):
    """A 100 kb reference with a SNP per kilobase, two haplotypes (the C2 shape, small: the LDS-resident fast path of every k)."""
    from varigraph_amd import synth
    rng = np.random.default_rng(seed)
    ref = synth.make_reference(100_000, seed=seed)
    pos = np.sort(rng.choice(np.arange(100, ref.size - 100), size=100, replace=False))
    alts = synth._ACGT[(synth._CODE[ref[pos]] + rng.integers(1, 4, size=pos.size)) % 4]
    hap1 = ref.copy()
    hap1[pos] = alts
    return np.unique(vgmi.synth_snp_keys(ref, pos, alts, k)), [ref, hap1]


def test_k21_saturates_across_launches():
    """Eight windows a run, two grid positions a lane."""
    keys, haps = _snp_graph(21, 61)
    block = vgmi.synth_reads_host(28, 0, 40_000, 150, haps)
    want = _want(keys, 21, block)
    assert 0 < want.max() < 255
    on = _saturate_across_launches(keys, 21, block, want, True)
    off = _saturate_across_launches(keys, 21, block, want, False)
    assert all(np.array_equal(a, b) for a, b in zip(on[:3], off[:3])) and on[3] > 100


def test_even_k_saturates_across_launches():
    co = get_cohort("cohort_k22")
    block = vgmi.synth_reads_host(29, 0, 40_000, 150, co.haplotypes())
    want = _want(co.graph.keys, co.k, block)
    assert co.k == 22 and 0 < want.max() < 255
    on = _saturate_across_launches(co.graph.keys, co.k, block, want, True)
    off = _saturate_across_launches(co.graph.keys, co.k, block, want, False)
    assert all(np.array_equal(a, b) for a, b in zip(on[:3], off[:3])) and on[3] > 100


def test_even_k_debited_kmers_keep_their_buckets_open():
    """Even k: a read whose bases behind a non-base complete, with the stale bases in front of it, a window that is its own reverse
    complement loses its next k-mer in the reference, and the debit pass takes that k-mer back ahead of the fast kernel.  While debits
    stand in its counter the k-mer is never flagged, however deep the sample: its buckets stay open, and it goes on being counted."""
    co = get_cohort("cohort_k22")
    k, hap = co.k, co.haplotypes()[0]
    body = hap[3000:3120].tobytes()
    rng = np.random.default_rng(5)
    lead = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=30))
    debited = lead + _rc(body[:k // 2]) + b"N" + body      # behind the N: rc(h) of the stale h in front of it, k / 2 bases in
    keys = np.unique(np.concatenate([co.graph.keys, o.sketch(body, k)]))
    keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
    block = _block([debited] * 300 + [body, _rc(body)] * 100)
    want = _want(keys, k, block)
    lost = int(np.searchsorted(keys, o.sketch(body[:k], k)[0]))      # the first k-mer behind the N: 300 times in the stream, never emitted there
    assert want[lost] == 200 and (want == 255).sum() >= 90
    got = {}
    for done in (True, False):
        with _Ctx(keys, k, done) as c:
            c.counts_reset()
            got[done] = _submit(c, block)
            can, marked = _check(c, done)
            again = _submit(c, block)
            _check(c, done)
            assert np.array_equal(again, _clamped((2, want)))
        assert np.array_equal(got[done], want), (done, int((got[done] != want).sum()))


def test_saturation_from_the_generic_kernel_and_the_slow_path():
    """Bits of SB set by other code than the fast kernel's counters: a block shorter than a pair of rows goes through the generic kernel
    alone (table_count), and the runs of 12-mers with more than four places go through the hash table window by window (slow_count)."""
    from varigraph_amd import synth
    rng = np.random.default_rng(2)
    unit = synth.make_reference(300, seed=5)      # 120 diverged copies of one element: 12-mers with dozens of places, overfull buckets
    ref = np.tile(unit, 120)
    mut = rng.random(ref.size) < 0.03
    ref[mut] = synth._ACGT[(synth._CODE[ref[mut]] + rng.integers(1, 4, size=int(mut.sum()))) % 4]
    pos = np.sort(rng.choice(np.arange(100, ref.size - 100), size=900, replace=False))
    alts = synth._ACGT[(synth._CODE[ref[pos]] + rng.integers(1, 4, size=900)) % 4]
    keys = np.unique(vgmi.synth_snp_keys(ref, pos, alts, 27))
    hap1 = ref.copy()
    hap1[pos] = alts
    assert 1000 < keys.size <= 65536
    large = vgmi.synth_reads_host(23, 0, 20_000, 150, [ref, hap1])
    small = large[:12 * 151]
    assert small.size < 2048
    w_small, w_large = _want(keys, 27, small), _want(keys, 27, large)
    got = {}
    for done in (True, False):
        with _Ctx(keys, 27, done) as c:
            c.counts_reset()
            a = _submit(c, small, 300)
            _check(c, done)
            b = _submit(c, large)
            _check(c, done)
            d = _submit(c, large, 9)
            can, marked = _check(c, done)
            got[done] = (a, b, d)
            if done:
                assert 0 < marked < can
    for done in (True, False):
        for g, w in zip(got[done], (_clamped((300, w_small)), _clamped((300, w_small), (1, w_large)), _clamped((300, w_small), (10, w_large)))):
            assert np.array_equal(g, w), (done, int((g != w).sum()))


def test_generic_kernel_alone_on_c1_then_a_large_block(c1):
    i = 500
    r = _site_read(c1, i, int(c1["sites"][i]) - 70)
    small = _block([r, _rc(r)] * 6)
    assert small.size < 2048
    w_small = _want(c1["keys"], c1["k"], small)
    for done in (True, False):
        with _Ctx(c1["keys"], c1["k"], done) as c:
            c.counts_reset()
            a = _submit(c, small, 300)
            can, marked = _check(c, done)
            if done:
                assert 0 < marked <= 2 * 12 + 2      # (the alternative allele's own 12-mers)
            b = _submit(c, c1["block"])
            _check(c, done)
        assert np.array_equal(a, _clamped((300, w_small)))
        assert np.array_equal(b, _clamped((300, w_small), (1, c1["want"])))


def test_round_trips(c1):
    """Export, reset, import, finish == the direct finish (the buckets' state is per sample and starts again); a context cloned from one
    that holds a deep sample starts with no bucket done."""
    import torch
    keys, k = c1["keys"], c1["k"]
    d_block = torch.from_numpy(c1["block"]).cuda()

    def deep_sample(c):
        c.counts_reset()
        for _ in range(60):
            c.reads_submit_device(d_block, d_block.numel(), 200_000)
        return c.counts_finish()[0]

    with _Ctx(keys, k) as c:
        direct = deep_sample(c)
        assert np.array_equal(direct, _clamped((60, c1["want"])))
        can, marked = _check(c)
        assert marked > 0
        ext = torch.empty(keys.size, dtype=torch.int32, device="cuda")
        c.counts_export_device(ext)
        c.counts_reset()
        assert _check(c)[1] == 0 and not c.counts_finish()[0].any()
        c.counts_import_device(ext)
        assert np.array_equal(c.counts_finish()[0], direct)
        assert np.array_equal(_submit(c, c1["block"]), _clamped((61, c1["want"])))
        _check(c)
        deep_sample(c)
        c2 = vgmi.Context(0, buffer_mib=16)
        try:
            c2.table_clone_from(c)
            assert c2.pt_done_check()[:3] == (can, 0, 0)
            c2.counts_reset()
            assert np.array_equal(_submit(c2, c1["block"]), c1["want"])
            assert _check(c2)[1] == 0
        finally:
            c2.close()
