"""Odd k at the count kernels' row geometry, on every path of the count plan (csrc/vgmi_count_plan.h), with the block's length on the
device (fastq_text: the device-side reader) and on the host (reads_submit).  One context per path; the knobs that choose a path are
read when the context is made and the table uploaded.  The reads are slices of the genome whose k-mers are keys, so every window is a
key and an end that is missed or counted twice at a row boundary moves a counter.  Expected counters are the oracle's."""
import functools

import numpy as np
import pytest

import even_k_cases as E
import oracle_lib as o
from varigraph_amd import vgmi

pytestmark = pytest.mark.gpu

# name: (k, more than 65 536 keys, knobs, context table)
PATHS = {
    "3-count27s": (27, False, {}, False),
    "4-count27s-k21": (21, False, {}, False),
    "1-count27-lds-filter": (27, False, {"VGMI_GRID12": "0"}, False),
    "0-generic": (27, False, {"VGMI_GENERIC_KERNEL": "1"}, False),
    "2-context-table-k21": (21, True, {}, True),
    "2-context-table-k27": (27, True, {}, True),
    "1-count27-global-filter": (27, True, {"VGMI_XTABLE": "0"}, False),
}
# packed block sizes in bytes (None: one read only): around single 768-byte rows, pairs of them and pairs of 1 024-byte rows
SIZES = [None, 700, 767, 768, 769, 1535, 1536, 1537, 2047, 2048, 2049, 3072, 4096, 6154]

_ctx = {}


class _Set:
    pass


@functools.lru_cache(maxsize=None)
def _keys(k, big):
    """(genome, keys): the k-mers of a 2 400-base genome; big: plus the sketch of 90 000 random bases, as even_k_cases.make builds it"""
    rng = np.random.default_rng(4000 + k + (7 if big else 0))
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    s = _Set()
    s.genome = acgt[rng.integers(0, 4, size=2400)].tobytes()
    sets = [o.sketch(s.genome, k)] + ([o.sketch(acgt[rng.integers(0, 4, size=90_000)].tobytes(), k)] if big else [])
    keys = np.unique(np.concatenate(sets))
    s.keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
    assert (s.keys.size > 65536) == big
    return s


def _reads(s, size):
    return [s.genome[100:210]] if size is None else E.fit(s, [], size)


@functools.lru_cache(maxsize=None)
def _want(k, big, size):
    s = _keys(k, big)
    reads = _reads(s, size)
    block = E.block_of(reads)
    assert size is None or block.size == size
    t = o.Table(s.keys)
    hits, read_bases = t.count_block(block, k)
    want = t.counts()
    # (checked on the CPU before the sizes were fixed: a counter at the clamp would hide a double count)
    assert want.any() and want.max() < 255 and hits == int(want.sum()), (k, big, size)
    return reads, block, want, read_bases


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def _context(name):
    k, big, knobs, ctable = PATHS[name]
    if name not in _ctx:
        with pytest.MonkeyPatch.context() as mp:
            for var in ("VGMI_GRID12", "VGMI_GENERIC_KERNEL", "VGMI_XTABLE", "VGMI_CTABLE", "VGMI_CTABLE_K", "VGMI_SMALLK", "VGMI_WIDE_SLOTS"):
                mp.delenv(var, raising=False)
            for var, val in knobs.items():
                mp.setenv(var, val)
            c = vgmi.Context(0, buffer_mib=16)
            c.table_upload(_keys(k, big).keys, k)
        assert (c.ctable_info()["n_buckets"] > 0) == ctable, name
        _ctx[name] = c
    return _ctx[name]


@pytest.mark.parametrize("name", list(PATHS))
def test_odd_k_at_the_row_geometry(name, monkeypatch):
    monkeypatch.delenv("VGMI_FASTQ_CHUNK_KB", raising=False)
    k, big = PATHS[name][:2]
    ctx = _context(name)
    for size in SIZES:
        reads, block, want, read_bases = _want(k, big, size)
        ctx.counts_reset()
        r = ctx.fastq_text(E.fastq(reads))
        cov, _, _ = ctx.counts_finish()
        assert (r["n_records"], r["n_bases"], r["stopped"], r["tail"]) == (len(reads), read_bases, False, b""), (name, size)
        bad = np.flatnonzero(cov != want)
        assert bad.size == 0, (name, size, "device length", int(bad.size), bad[:5], cov[bad[:5]], want[bad[:5]])
        ctx.counts_reset()
        ctx.reads_submit(block, len(reads))
        cov, _, _ = ctx.counts_finish()
        bad = np.flatnonzero(cov != want)
        assert bad.size == 0, (name, size, "host length", int(bad.size), bad[:5], cov[bad[:5]], want[bad[:5]])
