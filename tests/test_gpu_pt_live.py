"""The live filter of the small-graph count kernel (VGMI_PT_LIVE, VGMI_PT_LIVE_BYTES): deep into a sample the scan probes
an image of the 12-mer grid filter that holds only the 12-mers of buckets not yet done, rebuilt at L, 4 L, 16 L, ... bytes; a block that
crosses a due point is cut there at a boundary of row pairs.  Every case compares ALL counters with the oracle, bit for bit, and with a
VGMI_PT_LIVE=0 context, and asks vgmi_pt_live_check and vgmi_pt_done_check after every submit: no live 12-mer is missing from the
image in use and the image has no bit the static filter lacks -- always.  L is 4096 bytes unless a case says otherwise."""
import os

import numpy as np
import pytest

import oracle_lib as o
from conftest import get_cohort
from varigraph_amd import synth, vgmi

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
    s = sum(int(times) * c.astype(np.int64) for times, c in terms)
    return np.minimum(s, 255).astype(np.uint8)


class _Ctx:
    """A fresh context with the keys uploaded, the knobs set while the table (and with it the path table) is built."""

    def __init__(self, keys, k, live=True, unit=4096, buffer_mib=16):
        knobs = {"VGMI_PT_DONE": None, "VGMI_PT_LIVE": None if live else "0", "VGMI_PT_LIVE_BYTES": str(unit)}
        old = {n: os.environ.get(n) for n in knobs}
        for n, v in knobs.items():
            if v is None:
                os.environ.pop(n, None)
            else:
                os.environ[n] = v
        try:
            self.c = vgmi.Context(0, buffer_mib=buffer_mib)
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


def _check(c):
    """(the image's bits, builds that made a new image) once both checkers' violation counts have been looked at"""
    missing, foreign, bits, builds = c.pt_live_check()
    assert missing == 0 and foreign == 0, (missing, foreign, bits, builds)
    can, marked, wrong, missed = c.pt_done_check()
    assert wrong == 0 and missed == 0 and marked <= can, (can, marked, wrong, missed)
    return bits, builds


def _off(block):
    return np.concatenate([[0], np.flatnonzero(block == 10) + 1]).astype(np.uint64)


def _submit(c, block, times=1, k=27):
    """host blocks (vgmi_reads_submit), the checks after every one"""
    n = int((block == 10).sum())
    for _ in range(times):
        c.reads_submit(block, n, _off(block) if k % 2 == 0 else None)
        _check(c)
    return c.counts_finish()[0]


class _Dev:
    """a block resident on the device, submitted with its length on the host (vgmi_reads_submit_device)"""

    def __init__(self, block, k):
        import torch
        self.n = int((block == 10).sum())
        self.d = torch.from_numpy(block).cuda()
        self.off = torch.from_numpy(_off(block).astype(np.int64)).cuda() if k % 2 == 0 else None

    def submit(self, c, times=1, check=True):
        for _ in range(times):
            c.reads_submit_device(self.d, self.d.numel(), self.n, self.off)
            if check:
                _check(c)
        return c.counts_finish()[0]


def _static_bits(keys, k):
    with _Ctx(keys, k, live=False) as c:
        missing, foreign, bits, builds = c.pt_live_check()      # (no image in use: the static filter is the image)
        assert (missing, foreign, builds) == (0, 0, 0) and bits > 0
        return bits


# ---- the failure this can introduce: a live 12-mer missing from the image ----

_CODE = {65: 0, 67: 1, 71: 2, 84: 3}


def _canon12(s):
    f = 0
    for ch in bytes(s):
        f = f << 2 | _CODE[ch]
    r = 0
    for ch in bytes(s)[::-1]:
        r = r << 2 | (3 - _CODE[ch])
    return min(f, r)


def _bucket(cx, log2):
    h = cx * 0x9E3779B1 & 0xFFFFFFFF
    h ^= h >> 15
    h = h * 0x85EBCA77 & 0xFFFFFFFF
    h ^= h >> 13
    return h >> (32 - log2)


def _two_sites(plant):
    """A 6 kb reference with SNP sites A and B.  plant: None; 'places' -- the 12-mer around B's alternative allele stands next to six
    further sites as well (more than four places: its runs take the hash table, its bucket is flagged); 'third' -- two other 12-mers of
    the graph share that 12-mer's index bucket (a bucket with a third 12-mer: flagged).  Returns keys, the two blocks and the number of
    index buckets the graph's 12-mers hash to."""
    rng = np.random.default_rng(17)
    ref = synth.make_reference(6000, seed=23)
    A, B = 1000, 2000
    alt = lambda p: synth._ACGT[(synth._CODE[ref[p]] + 1) % 4]
    altB = alt(B)
    M = ref[B - 6:B + 6].copy()
    M[6] = altB
    extra = [3000 + 300 * i for i in range(6)]
    if plant is not None:
        words = []
        if plant == "places":
            words = [M] * 6
        elif plant == "third":
            want_b = _bucket(_canon12(M.tobytes()), 13)
            while len(words) < 2:
                w = synth._ACGT[rng.integers(0, 4, size=12)]
                if _bucket(_canon12(w.tobytes()), 13) == want_b and _canon12(w.tobytes()) != _canon12(M.tobytes()):
                    words.append(w)
        while len(words) < 6:
            words.append(synth._ACGT[rng.integers(0, 4, size=12)])
        for p, w in zip(extra, words):
            ref[p - 16:p - 4] = w      # within the k-mers across the site at p
    pos = np.array([A, B] + (extra if plant is not None else []))
    alts = np.array([alt(p) for p in pos], dtype=np.uint8)
    keys = np.unique(vgmi.synth_snp_keys(ref, pos, alts, 27))
    assert keys.size <= 1024      # (8 192 index buckets: what _bucket assumes)
    hapA, hapB = ref.copy(), ref.copy()
    hapA[A] = alts[0]
    hapB[B] = altB
    for j, p in enumerate(extra if plant is not None else []):
        hapA[p] = alts[2 + j]
    # the first sample never carries B's alternative allele; forward reads tile the reference every 10 bases and the other haplotype every
    # 75: the k-mers of the one reach the clamp within 17 submits (in front of the refresh at 4 MiB), those of the other within 128 (16 MiB)
    first = [h[s:s + 150].tobytes() for h, step in ((ref, 10), (hapA, 75)) for s in range(0, ref.size - 150, step)]
    r = hapB[B - 70:B + 80].tobytes()
    second = [r, _rc(r)] * 20 + [hapB[B - 26:B + 40].tobytes()] * 3
    buckets = set()
    for p, a in zip(pos, alts):
        for allele in (ref[p], a):
            h = ref[p - 26:p + 27].copy()
            h[26] = allele
            buckets |= {_bucket(_canon12(h[i:i + 12].tobytes()), 13) for i in range(42)}
    return keys, _block(first), _block(second), len(buckets)


@pytest.mark.parametrize("plant", [None, "places", "third"], ids=["plain", "more-than-four-places", "third-12-mer-in-the-bucket"])
def test_an_allele_the_deep_sample_never_carried_is_counted_from_zero(plant):
    """260 submits of reads without site B's alternative allele: everything else saturates, refreshes happen at 4 KiB, 16 KiB, ..., 16 MiB (the
    block is 100 KB: cuts inside it), two of them behind new done buckets.  Reads with the allele then count its k-mers from 0 upward, exactly."""
    keys, b1, b2, n_buckets = _two_sites(plant)
    w1, w2 = _want(keys, 27, b1), _want(keys, 27, b2)
    only2 = (w1 == 0) & (w2 > 0)
    assert only2.sum() == 27 and (w1[w1 > 0] >= 1).all() and b1.size > 8 * 2048
    got = {}
    for live in (True, False):
        with _Ctx(keys, 27, live) as c:
            c.counts_reset()
            d1 = _Dev(b1, 27)
            deep = d1.submit(c, 260)
            assert np.array_equal(deep, _clamped((260, w1))) and set(np.unique(deep)) <= {0, 255}
            bits, builds = _check(c)
            if live:
                assert builds >= 2
            after = _submit(c, b2)
            assert np.array_equal(after, _clamped((260, w1), (1, w2))), int((after != _clamped((260, w1), (1, w2))).sum())
            assert np.array_equal(after[only2], w2[only2])
            again = _submit(c, b2, 2)
            assert np.array_equal(again, _clamped((260, w1), (3, w2)))
            got[live] = (deep, after, again, c.pt_done_check()[0])
    assert all(np.array_equal(a, b) for a, b in zip(got[True][:3], got[False][:3]))
    # the planted 12-mers did flag their bucket (and the copies' neighbours theirs): those can never become done
    assert got[True][3] < n_buckets if plant is not None else got[True][3] == n_buckets, (got[True][3], n_buckets)


# ---- cuts ----

def _dense_graph(seed, length=6000):
    """a SNP every 25 bases: every 27-mer of both haplotypes is a graph k-mer"""
    rng = np.random.default_rng(seed)
    ref = synth.make_reference(length, seed=seed)
    pos = np.arange(30, length - 30, 25)
    alts = synth._ACGT[(synth._CODE[ref[pos]] + rng.integers(1, 4, size=pos.size)) % 4]
    hap1 = ref.copy()
    hap1[pos] = alts
    return np.unique(vgmi.synth_snp_keys(ref, pos, alts, 27)), [ref, hap1]


@pytest.fixture(scope="module")
def dense():
    keys, haps = _dense_graph(41)
    assert 5000 < keys.size <= 65536
    return dict(keys=keys, haps=haps)


@pytest.mark.parametrize("pairs", [2, 3, 4, 5, 64])
def test_cuts(dense, pairs):
    """Blocks of `pairs` pairs of rows and a ragged tail, reads of 150 bases (a read lies across every boundary of pairs), with L placed
    so that the first cut falls after pair 1, before the last pair, and nowhere (the due point in the last pair or the ragged tail: no
    pair behind the cut; beyond the block: nothing due).  Around both cuts an `N` and a newline within 27 bytes either side."""
    keys, haps = dense["keys"], dense["haps"]
    rng = np.random.default_rng(pairs)
    n_bytes = pairs * 2048 + 700
    reads = []
    while sum(len(r) + 1 for r in reads) < n_bytes:
        h = haps[int(rng.integers(0, 2))]
        s = int(rng.integers(0, h.size - 150))
        r = h[s:s + 150].tobytes()
        reads.append(_rc(r) if rng.integers(0, 2) else r)
    plain = _block(reads)[:n_bytes].copy()
    plain[-1] = 10
    if plain[-2] == 10:
        plain[-2] = ord("A")
    marked = plain.copy()
    for cut in {2048, (pairs - 1) * 2048}:
        for at, ch in ((cut - 20, ord("N")), (cut + 9, ord("N")), (cut - 7, 10), (cut + 22, 10)):
            while 10 in marked[at - 1:at + 2]:      # (no empty read)
                at -= 2
            marked[at] = ch
    units = [2048, (pairs - 1) * 2048, pairs * 2048 - 100, pairs * 2048 + 300, n_bytes + 5000]
    for block in (plain, marked):
        assert (np.diff(np.flatnonzero(block == 10)) > 1).all()
        w = _want(keys, 27, block)
        assert w.max() > 0
        with _Ctx(keys, 27, live=False) as c:
            c.counts_reset()
            off = _submit(c, block, 2)
        assert np.array_equal(off, _clamped((2, w)))
        for unit in units:
            with _Ctx(keys, 27, unit=unit) as c:
                c.counts_reset()
                one = _submit(c, block)
                assert np.array_equal(one, w), (unit, int((one != w).sum()))
                two = _submit(c, block)
                assert np.array_equal(two, off), (unit, int((two != off).sum()))


# ---- C1: unsaturated, saturated, lifecycle ----

@pytest.fixture(scope="module")
def c1():
    co = get_cohort("c1")
    block = vgmi.synth_reads_host(90125, 0, 200_000, 150, co.haplotypes())
    want = _want(co.graph.keys, co.k, block)
    assert 0 < want.max() < 255
    return dict(keys=co.graph.keys, k=co.k, block=block, want=want, static=_static_bits(co.graph.keys, co.k))


def test_unsaturated_sample_keeps_the_static_filter(c1):
    """Ten submits take no counter to the clamp: every refresh finds the number of done buckets unchanged and builds nothing."""
    with _Ctx(c1["keys"], c1["k"]) as c:
        c.counts_reset()
        d = _Dev(c1["block"], c1["k"])
        ten = d.submit(c, 10)
        assert np.array_equal(ten, _clamped((10, c1["want"])))
        assert _check(c) == (c1["static"], 0)


def test_saturated_sample_and_lifecycle(c1):
    """260 submits: the image shrinks to the few live 12-mers, the counters are the oracle's clamped values (L: _deep_unit).  After a reset the static
    filter is back; export / reset / import / finish equals the direct finish; a clone gets no image from its source."""
    import torch
    keys, k, want = c1["keys"], c1["k"], c1["want"]
    d = _Dev(c1["block"], k)
    got = {}
    for live in (True, False):
        with _Ctx(keys, k, live, unit=_deep_unit(c1["block"])) as c:
            c.counts_reset()
            deep = d.submit(c, 260)
            assert np.array_equal(deep, _clamped((260, want)))
            bits, builds = _check(c)
            if live:
                assert builds >= 1 and bits < c1["static"] // 20, (bits, builds, c1["static"])
            else:
                assert (bits, builds) == (c1["static"], 0)
            ext = torch.empty(keys.size, dtype=torch.int32, device="cuda")
            c.counts_export_device(ext)
            c.counts_reset()
            assert _check(c) == (c1["static"], 0) and not c.counts_finish()[0].any()
            c.counts_import_device(ext)
            assert np.array_equal(c.counts_finish()[0], deep)
            assert _check(c) == (c1["static"], 0)
            more = d.submit(c, 1)
            assert np.array_equal(more, deep)
            c.counts_reset()
            one = d.submit(c, 1)
            assert np.array_equal(one, want)
            d.submit(c, 259, check=False)
            c2 = vgmi.Context(0, buffer_mib=16)
            try:
                c2.table_clone_from(c)
                assert c2.pt_live_check() == (0, 0, c1["static"], 0)
                c2.counts_reset()
                assert np.array_equal(d.submit(c2, 1), want)
            finally:
                c2.close()
            got[live] = (deep, more, one)
    assert all(np.array_equal(a, b) for a, b in zip(got[True], got[False]))


# ---- other k ----

def _snp_graph(k, seed):
    rng = np.random.default_rng(seed)
    ref = synth.make_reference(100_000, seed=seed)
    pos = np.sort(rng.choice(np.arange(100, ref.size - 100), size=100, replace=False))
    alts = synth._ACGT[(synth._CODE[ref[pos]] + rng.integers(1, 4, size=pos.size)) % 4]
    hap1 = ref.copy()
    hap1[pos] = alts
    return np.unique(vgmi.synth_snp_keys(ref, pos, alts, k)), [ref, hap1]


def _deep_unit(block):
    """L for a sample of 260 submits of `block`: refreshes fall due a few pairs of rows in front of the end of submit 4, 16, 64 and 256 (cuts
    inside those blocks) -- the last one looks at a graph saturated all over.  (With L = 4096 the eight images are used up within the first
    64 MiB, before anything has reached the clamp.)"""
    return 4 * block.size - 10240


def _saturating_sequence(keys, k, block, want):
    d = _Dev(block, k)
    got = {}
    for live in (True, False):
        with _Ctx(keys, k, live, unit=_deep_unit(block)) as c:
            c.counts_reset()
            ten = d.submit(c, 10)
            deep = d.submit(c, 250)
            bits, builds = _check(c)
            more = d.submit(c, 1)
            c.counts_reset()
            one = d.submit(c, 1)
            got[live] = (ten, deep, more, one, bits, builds)
    for live in (True, False):
        ten, deep, more, one = got[live][:4]
        assert np.array_equal(ten, _clamped((10, want))) and np.array_equal(deep, _clamped((260, want)))
        assert np.array_equal(more, deep) and np.array_equal(one, want)
    return got


def test_k21_grid_of_8():
    keys, haps = _snp_graph(21, 61)
    block = vgmi.synth_reads_host(28, 0, 40_000, 150, haps)
    want = _want(keys, 21, block)
    assert 0 < want.max() < 255
    got = _saturating_sequence(keys, 21, block, want)
    assert got[True][5] >= 1 and got[True][4] < got[False][4]


def test_k22_debited_kmers_keep_their_buckets_live():
    """Even k: while debits stand in a k-mer's counter it is never flagged, however deep the sample -- its buckets are never done, its
    12-mers stay in every image, and it goes on being counted exactly."""
    co = get_cohort("cohort_k22")
    k, hap = co.k, co.haplotypes()[0]
    body = hap[3000:3120].tobytes()
    rng = np.random.default_rng(5)
    lead = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=30))
    debited = lead + _rc(body[:k // 2]) + b"N" + body
    keys = np.unique(np.concatenate([co.graph.keys, o.sketch(body, k)]))
    keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
    block = _block([debited] * 300 + [body, _rc(body)] * 100)
    want = _want(keys, k, block)
    lost = int(np.searchsorted(keys, o.sketch(body[:k], k)[0]))
    assert want[lost] == 200 and (want == 255).sum() >= 90 and block.size > 16 * 2048
    got = {}
    for live in (True, False):
        with _Ctx(keys, k, live) as c:
            c.counts_reset()
            a = _submit(c, block, k=k)
            bits, builds = _check(c)
            b = _submit(c, block, k=k)
            got[live] = (a, b)
            if live:
                assert builds >= 1
        assert np.array_equal(got[live][0], want), (live, int((got[live][0] != want).sum()))
        assert np.array_equal(got[live][1], _clamped((2, want)))
    block2 = vgmi.synth_reads_host(29, 0, 40_000, 150, co.haplotypes())
    want2 = _want(co.graph.keys, k, block2)
    assert 0 < want2.max() < 255
    _saturating_sequence(co.graph.keys, k, block2, want2)


# ---- the device-length path and two streams ----

@pytest.fixture(scope="module")
def deep_small(dense):
    """26 000 reads over the 6 kb dense graph: one pass takes a quarter of the k-mers to the clamp, a second one nearly all"""
    block = vgmi.synth_reads_host(77, 0, 26_000, 150, dense["haps"])
    want = _want(dense["keys"], 27, block)
    assert (want >= 128).mean() > 0.8 and (want == 255).mean() > 0.2
    return dict(block=block, want=want)


def test_device_side_fastq_reader(dense, deep_small):
    """The block's length lives in device memory: no cut, a due refresh runs behind the block -- between the chunks of the file."""
    keys, block, want = dense["keys"], deep_small["block"], deep_small["want"]
    reads = bytes(block).split(b"\n")[:-1]
    text = b"".join(b"@r\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for r in reads)
    got = {}
    for live in (True, False):
        with _Ctx(keys, 27, live) as c:
            c.counts_reset()
            for _ in range(5):      # (the refresh at 16 MiB of chunk bounds comes behind two passes or so: most k-mers are at the clamp by then)
                st = c.fastq_text(text, piece=1 << 20)
                assert st["n_records"] == len(reads) and not st["stopped"] and st["tail"] == b""
                bits, builds = _check(c)
            got[live] = c.counts_finish()[0]
            if live:
                assert builds >= 1
        assert np.array_equal(got[live], _clamped((5, want))), (live, int((got[live] != _clamped((5, want))).sum()))


def test_two_staging_streams(dense, deep_small):
    """vgmi_reads_submit from host memory with a 1 MiB staging buffer: the 4 MB block goes in pieces that alternate the two staging
    streams, refreshes fall due in between, and a piece is handed images built on the other stream."""
    keys, block, want = dense["keys"], deep_small["block"], deep_small["want"]
    assert block.size > 3 << 20
    got = {}
    for live in (True, False):
        with _Ctx(keys, 27, live, buffer_mib=1) as c:
            c.counts_reset()
            got[live] = _submit(c, block, 5)      # (19.6 MB: the refresh at 16 MiB finds nearly every bucket done)
            bits, builds = _check(c)
            if live:
                assert builds >= 1
    with _Ctx(keys, 27) as c:
        c.counts_reset()
        one_block = _Dev(block, 27).submit(c, 5)
    assert np.array_equal(got[True], _clamped((5, want)))
    assert np.array_equal(got[True], got[False]) and np.array_equal(got[True], one_block)
