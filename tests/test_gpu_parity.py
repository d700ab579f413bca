"""GPU parity tests (-m gpu): the HIP path through the C ABI (include/vgmi.h) against
 (a) the golden vectors dumped from the real reference and (b) the oracle on seeded inputs.
Bit-exact: everything on this path is integer work."""
import json
import os

import numpy as np
import pytest

import oracle_lib as o
from conftest import GOLDEN, block_from_seqs, get_cohort
from varigraph_amd import vgmi

pytestmark = pytest.mark.gpu

KATS = json.load(open(os.path.join(GOLDEN, "kats.json")))
BLOOM = json.load(open(os.path.join(GOLDEN, "bloom.json")))
NOKEY = np.uint64(0xFFFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def ctx():
    c = vgmi.Context(0, buffer_mib=64)
    yield c
    c.close()


# ----------------------------------------------------------------------------- K1 emitter
@pytest.mark.parametrize("case", KATS["sketch"], ids=lambda c: f"k{c['k']}")
def test_sketch_keys_match_reference_traces(ctx, case):
    """Ordered key list per read == reference kmer_sketch_fastq trace (odd k: row kernel, even k:
    sequential kernel), including lower case, U, N, raw 0..3 bytes, short reads, palindromes."""
    k = case["k"]
    seqs = [bytes.fromhex(t["seq_hex"]) for t in case["traces"]]
    block = block_from_seqs(seqs)
    keys = ctx.sketch_keys(block, len(seqs), k)
    start = 0
    for s, t in zip(seqs, case["traces"]):
        got = keys[start:start + len(s)]
        got = got[got != NOKEY]
        want = np.array([int(x, 16) for x in t["keys"]], dtype=np.uint64)
        assert np.array_equal(got, want), (k, s)
        assert keys[start + len(s)] == NOKEY
        start += len(s) + 1


@pytest.mark.parametrize("k", [1, 3, 5, 11, 21, 25, 27])
def test_sketch_keys_positions_random_block(ctx, k):
    """Per-position keys on a ragged random block spanning many 1 KiB rows and wave ranges."""
    rng = np.random.default_rng(k)
    alphabet = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTacgtNnU", dtype=np.uint8)
    seqs = [alphabet[rng.integers(0, alphabet.size, size=int(n))].tobytes()
            for n in rng.integers(1, 400, size=600)]
    block = block_from_seqs(seqs)
    got = ctx.sketch_keys(block, len(seqs), k)
    want = o.sketch_block_positions(block, k)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k", [2, 6, 22, 28])
def test_sketch_keys_even_k_random_block(ctx, k):
    rng = np.random.default_rng(100 + k)
    alphabet = np.frombuffer(b"ACGTACGTACGTNacgt", dtype=np.uint8)
    seqs = [alphabet[rng.integers(0, alphabet.size, size=int(n))].tobytes()
            for n in rng.integers(1, 300, size=200)]
    block = block_from_seqs(seqs)
    got = ctx.sketch_keys(block, len(seqs), k)
    want = o.sketch_block_positions(block, k)
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------- K1+K2 counting
def _upload(ctx, cohort, nodes=False, flags=False):
    g = cohort.graph
    ctx.table_upload(g.keys, cohort.k)
    if nodes:
        order = np.argsort(g.keys)
        off = [0]
        idx = []
        for name, start, kh in cohort.ref_nodes:
            pos = order[np.searchsorted(g.keys[order], kh)]
            assert np.array_equal(g.keys[pos], kh)
            idx.append(pos)
            off.append(off[-1] + len(kh))
        ctx.nodes_upload(np.array(off, dtype=np.uint64),
                         np.concatenate(idx).astype(np.uint32) if idx else np.zeros(0, np.uint32))
    if flags:
        ctx.flags_upload(_hom_flags(g))


def _hom_flags(g):
    """sample-independent predicate of Varigraph::get_hom_kmer (src/varigraph.cpp:263-287)"""
    n = g.keys.size
    flag = np.zeros(n, dtype=np.uint8)
    bits = np.unpackbits(g.bitvec.view(np.uint8), axis=1, bitorder="little")
    p = g.vcf_ploidy
    for s in range((g.hap_num - 1) // p):
        cols = [1 + s * p + h for h in range(p)]
        flag |= bits[:, cols].all(axis=1).astype(np.uint8)
    flag &= (g.f <= 1).astype(np.uint8)
    return flag


def test_cohort_counts_match_reference(ctx, cohort):
    """c[] after the HIP path == c[] dumped from the reference FastqKmer::build_fastq_index."""
    _upload(ctx, cohort, nodes=True, flags=True)
    ctx.counts_reset()
    block = cohort.block()
    ctx.reads_submit(block, cohort.n_reads)
    cov, cov_node, hist = ctx.counts_finish(nodes=True, hist=True)
    want = cohort.ref_c_in_graph_order()
    assert np.array_equal(cov, want)
    assert ctx.read_base() == cohort.ref_read_base
    # per-node depth gather in the reference's node/k-mer order
    order = np.argsort(cohort.graph.keys)
    exp = []
    for _, _, kh in cohort.ref_nodes:
        exp.append(want[order[np.searchsorted(cohort.graph.keys[order], kh)]])
    exp = np.concatenate(exp) if exp else np.zeros(0, np.uint8)
    assert np.array_equal(cov_node, exp)
    assert hist.tolist() == cohort.meta["hist"]
    ms, launches = ctx.count_kernel_ms()
    assert launches >= 1 and ms > 0


def test_counts_chunked_host_submit_and_device_submit(cohort):
    """Small staging buffer (block is cut at read boundaries, two streams) and the device-resident
    entry point give the same counters."""
    import torch
    want = cohort.ref_c_in_graph_order()
    block = cohort.block()
    c = vgmi.Context(0, buffer_mib=1)
    try:
        c.table_upload(cohort.graph.keys, cohort.k)
        c.counts_reset()
        c.reads_submit(block, cohort.n_reads)
        cov, _, _ = c.counts_finish()
        assert np.array_equal(cov, want)
        # device-resident block (+ offsets for even k)
        c.counts_reset()
        d_block = torch.from_numpy(block).cuda()
        d_off = None
        if cohort.k % 2 == 0:
            nl = np.flatnonzero(block == 10)
            off = np.concatenate([[0], nl + 1]).astype(np.uint64)
            d_off = torch.from_numpy(off.view(np.int64)).cuda()
        c.reads_submit_device(d_block, block.size, cohort.n_reads, d_off)
        cov2, _, _ = c.counts_finish()
        assert np.array_equal(cov2, want)
        assert c.read_base() == cohort.ref_read_base
    finally:
        c.close()


def test_counts_reset_split_and_saturation(ctx):
    """reset zeroes; split submission == single submission; repeated blocks saturate at 255."""
    cohort = get_cohort("cohort_snp")
    _upload(ctx, cohort)
    block = cohort.block()
    want = cohort.ref_c_in_graph_order().astype(np.int64)
    nl = np.flatnonzero(block == 10)
    cut = int(nl[len(nl) // 3]) + 1
    ctx.counts_reset()
    ctx.reads_submit(block[:cut], len(nl) // 3 + 1)
    ctx.reads_submit(block[cut:], cohort.n_reads - (len(nl) // 3 + 1))
    cov, _, _ = ctx.counts_finish()
    assert np.array_equal(cov, want)
    ctx.counts_reset()
    cov0, _, _ = ctx.counts_finish()
    assert not cov0.any()
    reps = 40
    ctx.counts_reset()
    for _ in range(reps):
        ctx.reads_submit(block, cohort.n_reads)
    cov, _, _ = ctx.counts_finish()
    # per-key occurrences are not clamped in the reference dump only when < 255; use the oracle total
    t = o.Table(cohort.graph.keys)
    for _ in range(reps):
        t.count_block(block, cohort.k)
    assert np.array_equal(cov, t.counts())
    assert (cov == 255).any()


def test_table_export_import_roundtrip(ctx):
    import torch
    cohort = get_cohort("cohort_sv")
    _upload(ctx, cohort)
    nbytes = ctx.table_image_bytes()
    img = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ctx.table_export(img)
    c2 = vgmi.Context(0, buffer_mib=16)
    try:
        c2.table_import(img)
        assert c2.table_info() == ctx.table_info()
        c2.counts_reset()
        c2.reads_submit(cohort.block(), cohort.n_reads)
        cov, _, _ = c2.counts_finish()
        assert np.array_equal(cov, cohort.ref_c_in_graph_order())
    finally:
        c2.close()


def test_error_paths(ctx):
    cohort = get_cohort("cohort_snp")
    keys = cohort.graph.keys
    with pytest.raises(vgmi.VgmiError) as e:
        ctx.table_upload(np.concatenate([keys[:10], keys[:1]]), 27)
    assert e.value.code == vgmi.E_DUPLICATE_KEY
    with pytest.raises(vgmi.VgmiError) as e:
        ctx.table_upload(keys[:10], 25)          # low byte says 27
    assert e.value.code == vgmi.E_BAD_KEY
    with pytest.raises(vgmi.VgmiError) as e:
        ctx.table_upload(keys[:10], 29)
    assert e.value.code == vgmi.E_INVALID
    with pytest.raises(vgmi.VgmiError) as e:
        ctx.counts_reset()                        # failed uploads leave no table
    assert e.value.code == vgmi.E_STATE
    ctx.table_upload(keys, 27)
    ctx.counts_reset()
    # zero-length read: the reference aborts on assert(len > 0) (src/kmer.cpp:124)
    for bad in (b"ACGT\n\nACGT\n", b"\nACGT\n", b"ACGTN\n\n"):
        ctx.counts_reset()
        ctx.reads_submit(np.frombuffer(bad, dtype=np.uint8), bad.count(b"\n"))
        with pytest.raises(vgmi.VgmiError) as e:
            ctx.counts_finish()
        assert e.value.code == vgmi.E_EMPTY_READ
    # 'N' right before the separator is NOT an empty read
    ctx.counts_reset()
    ok = b"ACGTN\nNN\nN\nACGT\n"
    ctx.reads_submit(np.frombuffer(ok, dtype=np.uint8), 4)
    ctx.counts_finish()
    with pytest.raises(vgmi.VgmiError) as e:
        ctx.reads_submit(np.frombuffer(b"ACGT", dtype=np.uint8), 1)   # no trailing '\n'
    assert e.value.code == vgmi.E_INVALID


def test_empty_table_and_tiny_inputs(ctx):
    ctx.table_upload(np.zeros(0, dtype=np.uint64), 27)
    ctx.counts_reset()
    ctx.reads_submit(np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGT\n", dtype=np.uint8), 1)
    cov, _, _ = ctx.counts_finish()
    assert cov.size == 0
    key = o.sketch(b"ACGTACGTTGCAAGCTTAGCGATCGAT", 27)
    ctx.table_upload(key, 27)
    ctx.counts_reset()
    ctx.reads_submit(np.frombuffer(b"ACGTACGTTGCAAGCTTAGCGATCGAT\nATCGATCGCTAAGCTTGCAACGTACGT\nAC\n", dtype=np.uint8), 3)
    cov, _, _ = ctx.counts_finish()
    assert cov.tolist() == [2]     # forward and reverse-complement read hit the same canonical key


# ----------------------------------------------------------------------------- Bloom (K3/K4)
@pytest.mark.parametrize("case", BLOOM, ids=lambda c: c["name"])
def test_bloom_filter_matches_reference(ctx, case):
    want = np.load(os.path.join(GOLDEN, f"bloom_{case['name']}_filter.npy"))
    m, nh = vgmi.bloom_params(case["n"], 0.01)
    assert (m, nh) == (case["m"], case["n_hash"])
    ctx.bloom_create(m, nh, np.array([int(s, 16) for s in case["seeds"]], dtype=np.uint64))
    for s in case["seqs"]:
        ctx.bloom_add_seq(np.frombuffer(s.encode(), dtype=np.uint8), case["k"])
    got = ctx.bloom_fetch()
    assert np.array_equal(got, want)
    mn, nz = ctx.bloom_query(np.array([int(x, 16) for x in case["query_keys"]], dtype=np.uint64))
    assert mn.tolist() == case["query_count"]
    assert nz.tolist() == case["query_find"]


@pytest.mark.parametrize("k", [27, 12])
def test_bloom_saturation_and_oracle(ctx, k):
    """A repetitive 200 kb sequence drives counters to the 255 clamp; bytes must equal the oracle's."""
    rng = np.random.default_rng(3)
    unit = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=300)]
    seq = np.concatenate([np.tile(unit, 400), np.frombuffer(b"NNN", dtype=np.uint8),
                          np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=80000)]])
    n = seq.size - k + 1
    m, nh = vgmi.bloom_params(n, 0.01)
    seeds = rng.integers(1, 1 << 63, size=nh).astype(np.uint64)
    ctx.bloom_create(m, nh, seeds)
    ctx.bloom_add_seq(seq, k)
    got = ctx.bloom_fetch()
    want = np.zeros(m, dtype=np.uint8)
    o.bloom_add_seq(want, seeds, seq, k)
    assert np.array_equal(got, want)
    assert (got == 255).any()


def test_bloom_binned_form_matches_oracle(ctx):
    """Sequences of 4 Mi bases and more go through the binned form (vgmi_bloom_bin.hip: positions partitioned by 128 KiB chunk of
    the filter, counters bumped in LDS): random bases, a tandem repeat that drives counters to the 255 clamp, N runs; the bytes must
    equal the oracle's (BloomFilter::add, src/counting_bloom_filter.cpp:28-36)."""
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    unit = acgt[rng.integers(0, 4, size=300)]
    seq = np.concatenate([acgt[rng.integers(0, 4, size=2_500_000)], np.tile(unit, 400), np.frombuffer(b"NNNNN", dtype=np.uint8),
                          acgt[rng.integers(0, 4, size=2_400_000)], np.frombuffer(b"N", dtype=np.uint8), acgt[rng.integers(0, 4, size=100_000)]])
    assert seq.size >= 4 << 20
    k = 27
    m, nh = vgmi.bloom_params(seq.size - k + 1, 0.01)
    seeds = rng.integers(1, 1 << 63, size=nh).astype(np.uint64)
    ctx.bloom_create(m, nh, seeds)
    ctx.bloom_add_seq(seq, k)
    ctx.bloom_add_seq(seq[:4_500_000], k)        # a second call onto the counters of the first
    got = ctx.bloom_fetch()
    want = np.zeros(m, dtype=np.uint8)
    o.bloom_add_seq(want, seeds, seq, k)
    o.bloom_add_seq(want, seeds, seq[:4_500_000], k)
    assert np.array_equal(got, want)
    assert (got == 255).any()


@pytest.mark.parametrize("shape", ["many_bins", "wide_bins"])
def test_bloom_binned_form_large_filter_geometries(ctx, shape):
    """The binned form's two levels at the geometries of large filters: `many_bins` -- a 1 GB filter (a 1.1e8-k-mer genome's), 125
    level-1 bins of 64 chunks, fed 12 Mb; `wide_bins` -- level-1 bins of 512 chunks (what a whole-genome filter of 28.8 GB takes),
    forced onto a small filter.  Bytes equal the oracle's."""
    rng = np.random.default_rng(21)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    k = 27
    if shape == "many_bins":
        seq = acgt[rng.integers(0, 4, size=12_000_000)]
        m, nh = vgmi.bloom_params(110_000_000, 0.01)
        env = {}
    else:
        seq = np.concatenate([acgt[rng.integers(0, 4, size=4_400_000)], np.tile(acgt[rng.integers(0, 4, size=200)], 600)])
        m, nh = vgmi.bloom_params(seq.size - k + 1, 0.01)
        env = {"VGMI_BLOOM_SUB": "512"}
    seeds = rng.integers(1, 1 << 63, size=nh).astype(np.uint64)
    old = {kk: os.environ.get(kk) for kk in env}
    os.environ.update(env)
    try:
        ctx.bloom_create(m, nh, seeds)
        ctx.bloom_add_seq(seq, k)
        got = ctx.bloom_fetch()
    finally:
        for kk, v in old.items():
            if v is None:
                os.environ.pop(kk, None)
            else:
                os.environ[kk] = v
    want = np.zeros(m, dtype=np.uint8)
    o.bloom_add_seq(want, seeds, seq, k)
    assert np.array_equal(got, want)


def test_bloom_binned_form_one_kmer_everywhere(ctx):
    """One k-mer repeated through the whole call lands in seven chunks: their room runs out, nothing is applied, the direct form
    redoes the call -- seven counters at 255, everything else as the random tail leaves it."""
    rng = np.random.default_rng(12)
    seq = np.concatenate([np.full(4_300_000, ord("A"), dtype=np.uint8), np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=50_000)]])
    k = 27
    m, nh = vgmi.bloom_params(seq.size - k + 1, 0.01)
    seeds = rng.integers(1, 1 << 63, size=nh).astype(np.uint64)
    ctx.bloom_create(m, nh, seeds)
    ctx.bloom_add_seq(seq, k)
    got = ctx.bloom_fetch()
    want = np.zeros(m, dtype=np.uint8)
    o.bloom_add_seq(want, seeds, seq, k)
    assert np.array_equal(got, want)


# ----------------------------------------------------------------------------- tooling
def test_synth_device_equals_host(ctx):
    import torch
    cohort = get_cohort("cohort_sv")
    haps = cohort.haplotypes()
    cat = np.concatenate(haps)
    off = np.concatenate([[0], np.cumsum([len(h) for h in haps])]).astype(np.uint64)
    n_reads, L = 5000, 150
    host = vgmi.synth_reads_host(77, 123, n_reads, L, haps)
    d_cat = torch.from_numpy(cat).cuda()
    d_out = torch.empty(n_reads * (L + 1), dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(77, 123, n_reads, L, d_cat, off, d_out)
    assert np.array_equal(d_out.cpu().numpy(), host)


def test_large_block_properties(ctx):
    """4 M reads of the C1/C2 workload generated on the device: the counters must equal the oracle's on a
    64 k-read prefix submitted alone, be invariant under splitting the block, and be monotone in the input."""
    import torch
    cohort = get_cohort("c1")
    haps = cohort.haplotypes()
    cat = np.concatenate(haps)
    off = np.concatenate([[0], np.cumsum([len(h) for h in haps])]).astype(np.uint64)
    n_reads, L = 4_000_000, 150
    d_cat = torch.from_numpy(cat).cuda()
    d_out = torch.empty(n_reads * (L + 1), dtype=torch.uint8, device="cuda")
    ctx.synth_reads_device(2024, 0, n_reads, L, d_cat, off, d_out)
    ctx.table_upload(cohort.graph.keys, 27)
    ctx.counts_reset()
    ctx.reads_submit_device(d_out, d_out.numel(), n_reads)
    full, _, _ = ctx.counts_finish()
    # split at a multiple of 16 bytes that is a read boundary: 16 reads * 151 B
    cut_reads = 16 * 100_003
    cut = cut_reads * (L + 1)
    ctx.counts_reset()
    ctx.reads_submit_device(d_out, cut, cut_reads)
    ctx.reads_submit_device(d_out[cut:], d_out.numel() - cut, n_reads - cut_reads)
    split, _, _ = ctx.counts_finish()
    assert np.array_equal(full, split)
    pre_reads = 65536
    ctx.counts_reset()
    ctx.reads_submit_device(d_out, pre_reads * (L + 1), pre_reads)
    pre, _, _ = ctx.counts_finish()
    t = o.Table(cohort.graph.keys)
    t.count_block(d_out[: pre_reads * (L + 1)].cpu().numpy(), 27)
    assert np.array_equal(pre, t.counts())
    assert (full >= pre).all()
    assert ctx.read_base() == pre_reads * L


# ----------------------------------------------------------------------------- host pipeline (C++)
@pytest.mark.parametrize("name", ["cohort_snp", "cohort_sv", "cohort_k22", "cohort_tetra"])
@pytest.mark.parametrize("use_depth", [False, True])
def test_sample_pipeline_fastq_to_coverage(name, use_depth):
    """FastqKmerHip::build_fastq_index over the fixture's FASTQ.gz files (C++ reader threads ->
    pinned staging -> HIP) + coverage statistics == the reference's counters, ReadDepth_,
    homCoverage and hapKmerCoverage_ (bit patterns of the floats)."""
    from varigraph_amd import host
    cohort = get_cohort(name)
    m = cohort.meta
    g = host.Graph(os.path.join(cohort.dir, "graph.bin.gz"))
    c = vgmi.Context(0, buffer_mib=1)   # small staging buffer: blocks are cut and double-buffered
    try:
        g.upload(c)
        fq = [os.path.join(cohort.dir, f"reads_{i}.fq.gz") for i in (1, 2)]
        cov, cov_node, hist, st = g.sample_count(c, fq, threads=2, sample_ploidy=m["sample_ploidy"], use_depth=use_depth)
        want = cohort.ref_c_in_graph_order()
        assert np.array_equal(cov, want)
        a = g.arrays()
        assert np.array_equal(cov_node, want[a["node_key_index"]])
        assert hist.tolist() == m["hist"]
        assert st["read_base"] == cohort.ref_read_base and st["n_reads"] == cohort.n_reads
        assert np.float32(st["read_depth"]).view(np.uint32) == int(m["read_depth_bits"], 16)
        assert st["max_coverage"] == int(m["max_cov"])
        pre = "use_depth_" if use_depth else ""
        assert st["hom_coverage"] == int(m[pre + "hom_cov"])
        assert np.float32(st["hap_kmer_coverage"]).view(np.uint32) == int(m[pre + "hap_kmer_cov_bits"], 16)
    finally:
        c.close()
        g.close()


def test_sample_pipeline_rejects_empty_read(tmp_path):
    from varigraph_amd import host
    cohort = get_cohort("cohort_snp")
    p = tmp_path / "bad.fq"
    p.write_bytes(b"@r1\nACGTACGTACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIIIIIIIIIII\n@r2\n\n+\n\n")
    g = host.Graph(os.path.join(cohort.dir, "graph.bin.gz"))
    c = vgmi.Context(0)
    try:
        g.upload(c)
        with pytest.raises(vgmi.VgmiError) as e:
            g.sample_count(c, [str(p)])
        assert e.value.code == vgmi.E_EMPTY_READ
    finally:
        c.close()
        g.close()


@pytest.mark.parametrize("k", [27, 21])
def test_dense_hits_overflow_path(ctx, k):
    """Reads made only of graph k-mers: every row overflows the per-wave pass ring, which must
    fall back to the step-at-a-time path and still count exactly (also exercises saturation)."""
    rng = np.random.default_rng(5 + k)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, size=3000)]
    keys = np.unique(o.sketch(genome.tobytes(), k))
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    seqs = []
    for _ in range(6000):
        s = int(rng.integers(0, genome.size - 150))
        r = genome[s:s + 150]
        if rng.random() < 0.5:
            r = comp[r[::-1]]
        seqs.append(r.tobytes())
    block = block_from_seqs(seqs)
    ctx.table_upload(keys, k)
    ctx.counts_reset()
    ctx.reads_submit(block, len(seqs))
    cov, _, _ = ctx.counts_finish()
    t = o.Table(keys)
    t.count_block(block, k)
    assert np.array_equal(cov, t.counts())
    assert (cov == 255).any()


def test_saturation_flags_cleared_by_reset(ctx):
    """Compact table format (k = 27, small graph): a counter that reaches the 255 clamp gets its slot flagged so
    that later hits skip their atomic.  The flag is per-sample state: after vgmi_counts_reset a shallow sample must
    count exactly again, and a deep one must saturate exactly again."""
    k = 27
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, size=2000)]
    keys = np.unique(o.sketch(genome.tobytes(), k))

    def sample(n, seed):
        r = np.random.default_rng(seed)
        return [genome[s:s + 150].tobytes() for s in r.integers(0, genome.size - 150, size=n)]

    deep, shallow = sample(20000, 1), sample(300, 2)
    ctx.table_upload(keys, k)
    for seqs in (deep, shallow, deep):
        block = block_from_seqs(seqs)
        ctx.counts_reset()
        ctx.reads_submit(block, len(seqs))
        cov, _, _ = ctx.counts_finish()
        t = o.Table(keys)
        t.count_block(block, k)
        assert np.array_equal(cov, t.counts())
        if seqs is deep:
            assert (cov == 255).mean() > 0.9   # all but the k-mers at the very ends of the little genome
        else:
            assert cov.max() < 255 and cov.sum() > 0


def test_saturation_flags_do_not_travel_with_the_table_image(ctx):
    """The slot array is part of the table image: an image exported (or cloned) after a deep sample carries that sample's
    saturation flags, which the importer has no list of -- its first reset must sweep them away, or hits on those
    k-mers would skip their atomics for good."""
    import torch
    k = 27
    rng = np.random.default_rng(78)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, size=2000)]
    keys = np.unique(o.sketch(genome.tobytes(), k))
    r = np.random.default_rng(3)
    deep = block_from_seqs([genome[s:s + 150].tobytes() for s in r.integers(0, genome.size - 150, size=20000)])
    shallow = block_from_seqs([genome[s:s + 150].tobytes() for s in r.integers(0, genome.size - 150, size=300)])
    ctx.table_upload(keys, k)
    ctx.counts_reset()
    ctx.reads_submit(deep, 20000)
    cov, _, _ = ctx.counts_finish()
    assert (cov == 255).mean() > 0.9
    img = torch.empty(ctx.table_image_bytes(), dtype=torch.uint8, device="cuda")
    ctx.table_export(img)
    t = o.Table(keys)
    t.count_block(shallow, k)
    for how in ("import", "clone"):
        other = vgmi.Context(0, buffer_mib=16)
        try:
            if how == "import":
                other.table_import(img)
            else:
                other.table_clone_from(ctx)
            other.counts_reset()
            other.reads_submit(shallow, 300)
            got, _, _ = other.counts_finish()
        finally:
            other.close()
        assert np.array_equal(got, t.counts()), how


# ----------------------------------------------------------------------------- large graphs (global grid bitmap)
_LARGE_GRAPH_CASES = {}


def _large_graph(k):
    """The 4 Mb / 66 000-SNP graph of the large-graph matrix: (keys, reference, the other haplotype, SNP positions)."""
    from varigraph_amd import synth
    G, V = 4_000_000, 66_000
    ref = synth.make_reference(G, seed=4242)
    rng = np.random.default_rng(17)
    pos = np.sort(rng.choice(np.arange(100, G - 100), size=V, replace=False))
    alts = synth._ACGT[(synth._CODE[ref[pos]] + rng.integers(1, 4, size=V)) % 4]
    keys = synth.snp_kmer_keys(ref, pos, alts, k=k)
    assert keys.size > 200_000
    hap1 = ref.copy()
    hap1[pos] = alts
    return keys, ref, hap1, pos


def _large_graph_case(k):
    """Keys, read block and the oracle's counters of the large-graph matrix: they depend on k only, so every variant of a k shares them."""
    if k not in _LARGE_GRAPH_CASES:
        keys, ref, hap1, _ = _large_graph(k)
        n_reads = 300_000
        block = vgmi.synth_reads_host(5, 0, n_reads, 150, [ref, hap1])
        # sprinkle ragged reads so the stream is not 151-periodic and ends in a partial row
        extra = block_from_seqs([hap1[i:i + L].tobytes() for i, L in ((1000, 31), (5000, 27), (9000, 200), (77, 26), (123456, 64))])
        block = np.concatenate([block, extra])
        n_reads += 5
        t = o.Table(keys)
        t.count_block(block, k)
        _LARGE_GRAPH_CASES[k] = (keys, block, n_reads, t.counts())
    return _LARGE_GRAPH_CASES[k]


@pytest.mark.parametrize("k,placement", [(27, None), (25, None), (23, None), (21, None), (19, None), (24, None), (22, None), (20, None), (26, None), (28, None), (28, {"VGMI_CTABLE_LOAD": "90"}), (28, {"VGMI_CT_DEFER": "0"}), (25, {"VGMI_CTABLE_K": "0"}),
                                         (21, {"VGMI_CTABLE_LOAD": "90"}), (23, {"VGMI_CTABLE_LOAD": "10"}), (27, {"VGMI_XTABLE": "0"}), (27, {"VGMI_XTABLE": "0", "VGMI_LOCALITY": "0"}),
                                         (27, {"VGMI_XTABLE": "0", "VGMI_LOCALITY": "3"}),
                                         (27, {"VGMI_WIDE_SLOTS": "1"}), (27, {"VGMI_WIDE_SLOTS": "1", "VGMI_DENSE_COUNTS": "1"}),
                                         (27, {"VGMI_WIDE_SLOTS": "1", "VGMI_LOCALITY": "0"}),
                                         (27, {"VGMI_XTABLE": "0", "VGMI_SLOT_ORDER": "1", "VGMI_LOCALITY": "6"}),
                                         (27, {"VGMI_CTABLE": "0"}), (27, {"VGMI_CTABLE": "0", "VGMI_XTABLE_ORDER": "0"}),
                                         (27, {"VGMI_CTABLE": "0", "VGMI_XTABLE_LOAD": "60"}), (27, {"VGMI_CTABLE_LOAD": "90"}),
                                         (27, {"VGMI_CTABLE_LOAD": "10"}),
                                         (27, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0"}), (25, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0"}),
                                         (22, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0"}), (19, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0"}),
                                         (27, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0", "VGMI_CT_DEFER_CAP": "40000"}),
                                         (27, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0", "VGMI_CT_DEFER_ROOM": "500"}),
                                         (27, {"VGMI_CT_DEFER": "0"}),
                                         (28, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0"}), (26, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0"}),
                                         (24, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0"}), (23, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0"}),
                                         (21, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0"}), (20, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0"}),
                                         (28, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0", "VGMI_CT_DEFER_CAP": "40000"}),
                                         (24, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0", "VGMI_CT_DEFER_CAP": "40000"}),
                                         (28, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0", "VGMI_CT_DEFER_ROOM": "500"}),
                                         (21, {"VGMI_CT_DEFER": "1", "VGMI_CT_DEFER_MIN": "0", "VGMI_CT_DEFER_ROOM": "500"})],
                         ids=["k27", "k25", "k23", "k21", "k19", "k24", "k22", "k20", "k26", "k28", "k28-context-table-crowded", "k28-counts-in-the-row-loop", "k25-generic-kernel", "k21-context-table-crowded", "k23-context-table-sparse", "k27-minimiser-buckets", "k27-random-homes", "k27-buckets-of-8", "k27-16-byte-slots",
                              "k27-16-byte-slots-dense-counters", "k27-16-byte-slots-random-homes", "k27-slots-by-minimiser-offset",
                              "k27-grid-table", "k27-grid-table-ids-by-key-index", "k27-grid-table-crowded", "k27-context-table-crowded",
                              "k27-context-table-sparse", "k27-deferred-counts", "k25-deferred-counts", "k22-deferred-counts", "k19-deferred-counts",
                              "k27-deferred-counts-buffer-fills-up", "k27-deferred-counts-rooms-fill-up", "k27-counts-in-the-row-loop",
                              "k28-deferred-counts", "k26-deferred-counts", "k24-deferred-counts", "k23-deferred-counts", "k21-deferred-counts", "k20-deferred-counts",
                              "k28-deferred-counts-buffer-fills-up", "k24-deferred-counts-buffer-fills-up", "k28-deferred-counts-rooms-fill-up",
                              "k21-deferred-counts-rooms-fill-up"])
def test_large_graph_grid_variant_matches_oracle(k, placement, monkeypatch):
    """> 65 536 keys: k = 27 takes count27c_kernel over the context table (default since round 4; path-ordered counter ids), with
    VGMI_CTABLE=0 count27x_kernel over round 2's grid-16-mer table, with
    VGMI_XTABLE=0 count27_kernel<global grid bitmap> over the minimiser-bucket table (+ generic tail row either way); k = 19 .. 25
    the context table with flanks of k - 16 bases and countkc_kernel<K> (round 5: a 16-mer looked up every 6 or 4 bases), with
    VGMI_CTABLE_K=0 the generic rows_kernel with the global blocked-Bloom prefilter.  Dense SNPs (1 per 60 bp) give ~35 %
    hit rate: exercises ring pressure, re-queued collision probes and unsaturated counters.  The k = 27 table has
    8-byte slots in minimiser buckets with per-slot counters by default; the other formats and placements stay covered.
    Round 6: VGMI_CT_DEFER=1 -- the context-table kernels write their runs of hits out and two kernels behind them count them by counter
    region in LDS (vgmi_ctdefer.hip); also with a record buffer and with rooms far too small (the rest is counted by plain atomics).
    Every countkc_defer_kernel<K> (k = 19 .. 28) is in the matrix, k = 28, 24 and 21 also with a buffer / rooms that fill up; the cases that
    set VGMI_CT_DEFER check through vgmi_ctable_defer_info that every launch took the path they are about."""
    import torch
    for name, val in (placement or {}).items():
        monkeypatch.setenv(name, val)
    keys, block, n_reads, want = _large_graph_case(k)
    deferred = bool(placement) and placement.get("VGMI_CT_DEFER") == "1"
    in_row_loop = bool(placement) and placement.get("VGMI_CT_DEFER") == "0"
    c = vgmi.Context(0, buffer_mib=16)
    try:
        c.table_upload(keys, k)
        info = c.table_info()
        assert info["n_keys"] == keys.size
        if k != 27:
            x = c.ctable_info()
            if placement and placement.get("VGMI_CTABLE_K") == "0":
                assert x["n_buckets"] == 0, x
            else:      # (k = 28, round 6: a unitig's first and last sixteen-mer have no window an entry of 11 + 16 + 11 bases can hold)
                assert x["n_buckets"] > 0 and x["n_entries"] == keys.size + (10 if k == 28 else k - 16) * x["n_unitigs"], x
        c.counts_reset()
        c.reads_submit(block, n_reads)               # chunked through the 16 MiB staging buffers
        cov, _, _ = c.counts_finish()
        assert np.array_equal(cov, want)
        assert want.sum() > 5_000_000 and want.max() > 8
        # which kernels counted: a deferral that fell back to the row loop (or the reverse) would be green and check nothing
        launches, di = c.count_kernel_ms()[1], c.ctable_defer_info()
        assert launches >= 2
        if deferred:
            assert (di["deferred_launches"], di["plain_launches"]) == (launches, 0), di
            assert di["n_bins"] * di["region"] >= keys.size and di["n_bins"] >= 2, di
            if "VGMI_CT_DEFER_CAP" in placement:
                assert di["cap"] == 40448, di
            if "VGMI_CT_DEFER_ROOM" in placement:
                assert di["room"] == 501, di
        elif in_row_loop:
            assert (di["deferred_launches"], di["plain_launches"]) == (0, launches), di
        # device-resident single launch gives the same
        c.counts_reset()
        d = torch.from_numpy(block).cuda()
        d_off = None
        if k % 2 == 0:      # even k: the reads' offsets come with the block
            d_off = torch.from_numpy(np.concatenate([[0], np.flatnonzero(block == 10) + 1]).astype(np.int64)).cuda()
            assert d_off.numel() == n_reads + 1
        c.reads_submit_device(d, block.size, n_reads, d_off)
        cov2, _, _ = c.counts_finish()
        assert np.array_equal(cov2, want)
        dj = c.ctable_defer_info()
        if deferred:
            assert (dj["deferred_launches"], dj["plain_launches"]) == (di["deferred_launches"] + 1, 0), dj
        elif in_row_loop:
            assert (dj["deferred_launches"], dj["plain_launches"]) == (0, di["plain_launches"] + 1), dj
    finally:
        c.close()


@pytest.mark.parametrize("form,crowded,k", [("ctable", False, 27), ("ctable", True, 27), ("xtable", False, 27), ("xtable", True, 27),
                                           ("ctable", False, 25), ("ctable", True, 21), ("ctable", False, 19), ("ctable-deferred", False, 27), ("ctable-deferred", True, 23), ("ctable", False, 28), ("ctable", True, 28)],
                         ids=["context-table", "context-table-crowded", "grid-table", "grid-table-crowded", "context-table-k25",
                              "context-table-crowded-k21", "context-table-k19", "context-table-deferred-counts", "context-table-crowded-k23-deferred-counts", "context-table-k28", "context-table-crowded-k28"])
def test_repeat_rich_graph_matches_oracle(form, crowded, k, monkeypatch):
    """A reference made of thousands of diverged copies of one 400-bp element: every 16-mer of the element sits in hundreds
    of different contexts / graph k-mers, far more than its home bucket (line) of the context table (grid-16-mer table) and the
    ones behind it hold.  Those k-mers must be served by the exact overflow table, and nothing may be matched by less than every base."""
    if form == "xtable":
        monkeypatch.setenv("VGMI_CTABLE", "0")
    if form == "ctable-deferred":      # (round 6: reads of a repeat pile onto few counter regions)
        monkeypatch.setenv("VGMI_CT_DEFER", "1")
        monkeypatch.setenv("VGMI_CT_DEFER_MIN", "0")
    if crowded:
        monkeypatch.setenv("VGMI_XTABLE_LOAD", "60")
        monkeypatch.setenv("VGMI_CTABLE_LOAD", "80")
    from varigraph_amd import synth
    rng = np.random.default_rng(99)
    unit = synth.make_reference(400, seed=31)
    copies = 6000
    ref = np.tile(unit, copies)
    mut = rng.random(ref.size) < 0.02                       # 2 % divergence between copies
    ref[mut] = synth._ACGT[(synth._CODE[ref[mut]] + rng.integers(1, 4, size=int(mut.sum()))) % 4]
    G = ref.size
    V = 60_000
    pos = np.sort(rng.choice(np.arange(100, G - 100), size=V, replace=False))
    alts = synth._ACGT[(synth._CODE[ref[pos]] + rng.integers(1, 4, size=V)) % 4]
    keys = np.unique(vgmi.synth_snp_keys(ref, pos, alts, k))
    assert keys.size > 200_000
    hap1 = ref.copy()
    hap1[pos] = alts
    n_reads = 120_000
    block = vgmi.synth_reads_host(11, 0, n_reads, 150, [ref, hap1])
    c = vgmi.Context(0, buffer_mib=16)
    try:
        c.table_upload(keys, k)
        if form == "xtable":
            x = c.xtable_info()
            assert x["n_lines"] > 0 and x["overflow_pairs"] > 1000, x
        else:
            x = c.ctable_info()
            assert x["n_buckets"] > 0 and x["overflow_kmers"] > 1000 and c.xtable_info()["n_lines"] == 0, x
        c.counts_reset()
        c.reads_submit(block, n_reads)
        cov, _, _ = c.counts_finish()
        t = o.Table(keys)
        t.count_block(block, k)
        assert np.array_equal(cov, t.counts())
        assert int(cov.astype(np.int64).sum()) > 1_000_000
    finally:
        c.close()


def test_make_mbf_matches_reference_whole_genome_bloom(ctx, tmp_path):
    """vgh_make_mbf (FASTA -> device Bloom, seeds as the reference draws them for the det build's
    random_device value) == the reference's build_fasta_index + make_mbf, byte for byte (sha256)."""
    import hashlib
    import importlib.util
    from varigraph_amd import host
    spec = importlib.util.spec_from_file_location("mg", os.path.join(GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    fa = str(tmp_path / "mbf.fa")
    mg.mbf_fasta(fa)
    for c in json.load(open(os.path.join(GOLDEN, "mbf.json"))):
        gs, m, nh = host.make_mbf(ctx, fa, c["k"], seeds=None, random_device_value=c["random_device_value"])
        assert (gs, m, nh) == (c["genome_size"], c["m"], c["n_hash"])
        filt = ctx.bloom_fetch()
        assert hashlib.sha256(filt.tobytes()).hexdigest() == c["sha256"]
        # BloomFilter::save's file: size, number of hashes, the 64-bit seeds, the counters -- and back through load_file
        path = str(tmp_path / ("mbf_%d.bin" % c["k"]))
        ctx.bloom_save_file(path)
        data = open(path, "rb").read()
        head = c["m"].to_bytes(8, "little") + c["n_hash"].to_bytes(4, "little") + b"".join(int(x, 16).to_bytes(8, "little") for x in c["seeds"])
        assert data[:len(head)] == head and data[len(head):] == filt.tobytes()
        other = vgmi.Context(0, buffer_mib=16)
        try:
            other.bloom_load_file(path)
            assert np.array_equal(other.bloom_fetch(), filt)
        finally:
            other.close()


def test_full_size_c2_properties(ctx):
    """BASELINE.json configs[1] at full size: 1e8 reads (50 M pairs) of the C2 workload, generated on the
    device.  Size-independent properties: (1) one launch == five ragged sub-launches, (2) the first
    2 M reads alone equal the oracle, (3) counters are monotone in the input, (4) at 15 000x coverage
    every graph k-mer carried by the sequenced sample's two haplotypes is saturated at 255."""
    import torch
    cohort = get_cohort("c1")
    haps = cohort.haplotypes()
    cat = np.concatenate(haps)
    off = np.concatenate([[0], np.cumsum([len(h) for h in haps])]).astype(np.uint64)
    n_reads, L = 100_000_000, 150
    d_cat = torch.from_numpy(cat).cuda()
    d_out = torch.empty(n_reads * (L + 1), dtype=torch.uint8, device="cuda")
    for first in range(0, n_reads, 10_000_000):
        ctx.synth_reads_device(1000, first, 10_000_000, L, d_cat, off, d_out[first * (L + 1):])
    keys = cohort.graph.keys
    ctx.table_upload(keys, 27)
    ctx.counts_reset()
    ctx.reads_submit_device(d_out, d_out.numel(), n_reads)
    full, _, _ = ctx.counts_finish()
    assert ctx.read_base() == n_reads * L
    # (1) ragged split at read boundaries that are multiples of 16 reads (keeps 16-byte alignment)
    cuts = [0, 16 * 1_000_003, 16 * 2_500_001, 16 * 2_500_002, 16 * 5_999_999, n_reads]
    ctx.counts_reset()
    for a, b in zip(cuts[:-1], cuts[1:]):
        ctx.reads_submit_device(d_out[a * (L + 1):], (b - a) * (L + 1), b - a)
    split, _, _ = ctx.counts_finish()
    assert np.array_equal(full, split)
    # (2) prefix against the oracle
    pre = 2_000_000
    ctx.counts_reset()
    ctx.reads_submit_device(d_out, pre * (L + 1), pre)
    part, _, _ = ctx.counts_finish()
    t = o.Table(keys)
    t.count_block(d_out[: pre * (L + 1)].cpu().numpy(), 27)
    assert np.array_equal(part, t.counts())
    # (3) monotone
    assert (full >= part).all()
    # (4) saturation of the sample's own k-mers
    hk = np.unique(np.concatenate([o.sketch(h.tobytes(), 27) for h in haps]))
    on_sample = np.isin(keys, hk)
    assert on_sample.sum() > 0.9 * keys.size
    assert (full[on_sample] == 255).all()


@pytest.mark.parametrize("name", ["cohort_snp", "c1"])
def test_read_sharded_sample_sums_to_single_gpu_result(name):
    """Strong-scaling mode: two contexts count the two halves of one sample, their raw counters are
    summed (what the RCCL all-reduce does across ranks) and imported: clamped result == single pass."""
    import torch
    cohort = get_cohort(name)
    block = cohort.block()
    if name == "cohort_snp":
        block = np.tile(block, 30)           # push some counters past 255 so the clamp matters
        n_reads = cohort.n_reads * 30
    else:
        n_reads = cohort.n_reads
    nl = np.flatnonzero(block == 10)
    half = int(nl[len(nl) // 2]) + 1
    a, b = vgmi.Context(0, buffer_mib=16), vgmi.Context(0, buffer_mib=16)
    try:
        for c in (a, b):
            c.table_upload(cohort.graph.keys, cohort.k)
            c.counts_reset()
        a.reads_submit(block, n_reads)
        want, _, _ = a.counts_finish()
        a.counts_reset()
        a.reads_submit(block[:half], len(nl) // 2 + 1)
        b.reads_submit(block[half:], n_reads - (len(nl) // 2 + 1))
        ta = torch.empty(cohort.graph.keys.size, dtype=torch.int32, device="cuda")
        tb = torch.empty_like(ta)
        a.counts_finish()                    # drain the staged kernels before exporting
        b.counts_finish()
        a.counts_export_device(ta)
        b.counts_export_device(tb)
        tot = ta + tb
        for c in (a, b):
            c.counts_import_device(tot)
            got, _, _ = c.counts_finish()
            assert np.array_equal(got, want)
        if name == "cohort_snp":
            assert (want == 255).any()
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("table_mul,wide", [("8", False), ("2", False), ("2", True)])
def test_every_kmer_counted_once_at_any_alignment(table_mul, wide, monkeypatch):
    """A 400-base sequence whose k-mers are all graph k-mers, placed at assorted stream offsets (row
    boundaries, wave-range boundaries, the last positions before the ragged tail): every k-mer must be
    counted exactly once.  Regression for (a) the flush of a wave that owns a single row while probes
    collide in the table (re-queue path; load factor 0.5 makes collisions frequent) and (b) k-mers
    ending in the last <= 11 positions of the last complete row (no grid offset left in the fast
    kernel's rows: they belong to the generic tail launch).  Offsets straddle the 768-byte rows and the
    1536-byte row pairs of the k = 27 kernel; `wide` forces the 16-byte slot format, which a small k = 27 graph
    only gets through the generic kernel."""
    monkeypatch.setenv("VGMI_TABLE_MUL", table_mul)
    if wide:
        monkeypatch.setenv("VGMI_WIDE_SLOTS", "1")
    rng = np.random.default_rng(1)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    S = acgt[rng.integers(0, 4, size=400)].tobytes()
    keys_pos = o.sketch(S, 27)
    uk, inv = np.unique(keys_pos, return_inverse=True)
    want = np.bincount(inv, minlength=uk.size).astype(np.uint8)
    c = vgmi.Context(0)
    try:
        c.table_upload(uk, 27)
        for pre in [0, 1, 5, 13, 100, 340, 366, 367, 368, 379, 623, 624, 635, 760, 767, 1000, 1019, 1130, 1135, 1136,
                    1147, 1500, 1535, 1536, 2047, 3000, 5000]:
            for post in [0, 3000]:
                filler = (b"N" * pre + b"\n") if pre else b""
                tail = (b"N" * post + b"\n") if post else b""
                blk = np.frombuffer(filler + S + b"\n" + tail, dtype=np.uint8)
                c.counts_reset()
                c.reads_submit(blk, 1 + (1 if pre else 0) + (1 if post else 0))
                cov, _, _ = c.counts_finish()
                assert np.array_equal(cov, want), (pre, post, int((cov != want).sum()))
    finally:
        c.close()


@pytest.mark.parametrize("k", [4, 12, 22, 28])
def test_bloom_even_k_segmented_matches_sequential_oracle(ctx, k):
    """Even k: emission depends on history (palindromic k-mers do not advance l, a non-base resets l but not the
    registers, src/kmer.cpp:134,145).  The device splits a chromosome into 1 KiB segments and rebuilds the state by
    look-back (bloom_even_kernel); the oracle runs the reference's sequential loop.  The sequence is built to hurt:
    N runs that end exactly on / just before / just after segment borders, runs longer than a segment, single Ns every
    few bases (stale register bits), long palindromic stretches (ACGT..., AT..., poly-A/T), lower case and other bytes."""
    rng = np.random.default_rng(100 + k)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)

    def rand(n):
        return acgt[rng.integers(0, 4, size=n)]

    def lit(b, n=1):
        return np.tile(np.frombuffer(b, dtype=np.uint8), n)

    parts = [rand(5), lit(b"N"), rand(k - 1), lit(b"N"), rand(k), lit(b"N"), rand(3 * k)]
    parts += [lit(b"ACGT", 700), rand(50), lit(b"AT", 900), lit(b"N"), lit(b"AT", 40), rand(7), lit(b"A", 1500), lit(b"T", 1500)]
    for border_shift in (-2, -1, 0, 1, 2):   # an N run ending around a multiple of 1024
        cur = sum(p.size for p in parts)
        pad = (-cur) % 1024 + 1024 + border_shift - 9
        parts += [rand(pad), lit(b"N", 9), rand(k // 2), lit(b"n"), rand(2 * k + 3)]
    parts += [rand(300), lit(b"N", 3000), rand(k - 1), lit(b"N", 1100), rand(4000)]
    sprinkled = rand(6000)
    sprinkled[rng.choice(6000, size=900, replace=False)] = ord("N")
    parts += [sprinkled, np.frombuffer(b"acgtRYKM-*", dtype=np.uint8), rand(2500)]
    for _ in range(30):   # exact reverse-complement palindromes of length k dropped into random sequence
        h = rand(k // 2)
        comp = np.array([{65: 84, 67: 71, 71: 67, 84: 65}[x] for x in h[::-1]], dtype=np.uint8)
        parts += [rand(int(rng.integers(1, 3 * k))), h, comp]
    parts += [rand(20000)]
    seq = np.concatenate(parts)
    n = max(1, seq.size - k + 1)
    m, nh = vgmi.bloom_params(n, 0.01)
    seeds = rng.integers(1, 1 << 63, size=nh).astype(np.uint64)
    ctx.bloom_create(m, nh, seeds)
    ctx.bloom_add_seq(seq, k)
    got = ctx.bloom_fetch()
    want = np.zeros(m, dtype=np.uint8)
    o.bloom_add_seq(want, seeds, seq, k)
    assert want.sum() > 0
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------
# Small graphs (<= 65 536 k-mers): count27s_kernel and the path table (vgmi_ptable.hip).  The golden cohorts above run through
# the default (12-mer grid + path table) in every test of this file; these add the shapes the path table has rare paths for and
# keep the two A/B variants (hash-table drain, round 2's 16-mer kernel) in the matrix.
def _small_graph(kind, rng, k=27):
    from varigraph_amd import synth
    if kind == "repeats":
        # 120 diverged copies of one 300-bp element: every 12-mer of the element has dozens of places (> 4: the run goes to the
        # hash table window by window) and the index buckets of neighbouring 12-mers fill up
        unit = synth.make_reference(300, seed=5)
        ref = np.tile(unit, 120)
        mut = rng.random(ref.size) < 0.03
        ref[mut] = synth._ACGT[(synth._CODE[ref[mut]] + rng.integers(1, 4, size=int(mut.sum()))) % 4]
        n_var = 900
    elif kind == "dense-sites":
        # a SNP every ~12 bp: every k-mer spans two or three sites, chains are short, 12-mers have three and four places
        ref = synth.make_reference(20_000, seed=6)
        n_var = 1100
    else:   # "plain": one SNP per kilobase (the C2 shape)
        ref = synth.make_reference(400_000, seed=7)
        n_var = 400
    pos = np.sort(rng.choice(np.arange(100, ref.size - 100), size=n_var, replace=False))
    alts = synth._ACGT[(synth._CODE[ref[pos]] + rng.integers(1, 4, size=n_var)) % 4]
    keys = np.unique(vgmi.synth_snp_keys(ref, pos, alts, k))
    hap1 = ref.copy()
    hap1[pos] = alts
    return keys, [ref, hap1]


@pytest.mark.parametrize("kind", ["plain", "repeats", "dense-sites"])
@pytest.mark.parametrize("variant", [{}, {"VGMI_PTABLE": "0"}, {"VGMI_GRID12": "0"}], ids=["path-table", "hash-drain", "grid16-round2"])
def test_small_graph_variants_match_oracle(kind, variant, monkeypatch):
    for k_, v_ in variant.items():
        monkeypatch.setenv(k_, v_)
    rng = np.random.default_rng({"plain": 1, "repeats": 2, "dense-sites": 3}[kind])
    keys, haps = _small_graph(kind, rng)
    assert 1000 < keys.size <= 65536, keys.size
    n_reads = 60_000
    block = vgmi.synth_reads_host(23, 0, n_reads, 150, haps)
    # reads with non-bases and lower case on top (validity masks, both strands come from the generator already)
    b2 = block.copy()
    idx = rng.choice(b2.size, size=3000, replace=False)
    idx = idx[b2[idx] != 10]
    b2[idx[:1500]] = ord("N")
    b2[idx[1500:]] |= 0x20
    c = vgmi.Context(0, buffer_mib=16)
    try:
        c.table_upload(keys, 27)
        t = o.Table(keys)
        for blk in (block, b2):
            c.counts_reset()
            # ragged pieces: the fast kernel takes whole pairs of rows, the generic kernel the ends
            cuts = [0, 16 * 1000, 16 * 1000 + 16 * 37, n_reads]
            for a, e in zip(cuts[:-1], cuts[1:]):
                c.reads_submit(blk[a * 151:e * 151], e - a)
            cov, _, _ = c.counts_finish()
            t.reset()
            t.count_block(blk, 27)
            assert np.array_equal(cov, t.counts()), (kind, variant)
        assert int(cov.astype(np.int64).sum()) > 50_000
    finally:
        c.close()


@pytest.mark.parametrize("variant", [("small", {}), ("large", {}), ("large", {"VGMI_WIDE_SLOTS": "1", "VGMI_XTABLE": "0"}), ("k25", {})],
                         ids=["small-graph", "large-graph", "large-graph-16-byte-slots", "k25"])
def test_table_lookup_returns_the_index_of_every_key(variant, monkeypatch):
    """vgmi_table_lookup == graph2node's find (src/construct_index.cpp:710-751): keys of the set map to their index in the uploaded
    array, whatever order they are asked in; k-mers the graph does not hold, keys of another k and malformed keys map to 0xFFFFFFFF.
    The counters are not touched (a sample counted before the lookups reads out the same after them)."""
    from varigraph_amd import synth
    size, env = variant
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    rng = np.random.default_rng(21)
    k = 25 if size == "k25" else 27
    if size == "small":
        keys, haps = _small_graph("plain", rng)
    else:
        G, V = 2_000_000, 30_000
        ref = synth.make_reference(G, seed=99)
        pos = np.sort(rng.choice(np.arange(100, G - 100), size=V, replace=False))
        alts = synth._ACGT[(synth._CODE[ref[pos]] + rng.integers(1, 4, size=V)) % 4]
        keys = np.unique(synth.snp_kmer_keys(ref, pos, alts, k=k))
        hap1 = ref.copy()
        hap1[pos] = alts
        haps = [ref, hap1]
        assert keys.size > 65_536
    keys = keys[rng.permutation(keys.size)]             # the uploaded order is the index
    absent = np.unique(o.sketch(synth._ACGT[rng.integers(0, 4, size=20_000)].tobytes(), k))
    absent = absent[~np.isin(absent, keys)]
    assert absent.size > 10_000
    other_k = (keys[:100] & ~np.uint64(0xFF)) | np.uint64(k - 2)
    too_wide = keys[:100] | (np.uint64(1) << np.uint64(8 + 2 * k))
    asked = np.concatenate([keys, absent, other_k, too_wide, keys[:1000]])
    want = np.concatenate([np.arange(keys.size, dtype=np.uint32), np.full(absent.size + 200, 0xFFFFFFFF, dtype=np.uint32),
                           np.arange(1000, dtype=np.uint32)])
    order = rng.permutation(asked.size)
    c = vgmi.Context(0, buffer_mib=16)
    try:
        c.table_upload(keys, k)
        block = vgmi.synth_reads_host(3, 0, 20_000, 150, haps)
        c.counts_reset()
        c.reads_submit(block, 20_000)
        got = c.table_lookup(asked[order])
        assert np.array_equal(got, want[order]), int((got != want[order]).sum())
        assert c.table_lookup(np.empty(0, dtype=np.uint64)).size == 0
        cov, _, _ = c.counts_finish()
        t = o.Table(keys)
        t.count_block(block, k)
        assert np.array_equal(cov, t.counts())
    finally:
        c.close()


def _low_complexity_sequence(rng):
    """What a unitig layout can trip over: homopolymers (a k-mer that follows itself), short tandem repeats (k-mers on cycles:
    no chain end to start a walk from), an inverted repeat (12-mers that are their own reverse complement across the centre,
    k-mers next to their own reverse complement), 12-mers with more than four places, and one element in both orientations."""
    from varigraph_amd import synth
    comp = {65: 84, 67: 71, 71: 67, 84: 65}

    def rc(a):
        return np.array([comp[int(x)] for x in a[::-1]], dtype=np.uint8)

    def lit(s, times=1):
        return np.frombuffer((s * times).encode(), dtype=np.uint8).copy()

    r = lambda n, seed: synth._ACGT[rng.integers(0, 4, size=n)]     # (make_reference's seeds are offsets into one stream)
    x = r(70, 11)
    unit30, unit13, elem = r(30, 12), r(13, 13), r(200, 14)
    twelve = r(12, 15)
    spread = np.concatenate([np.concatenate([r(45, 100 + i), twelve]) for i in range(7)])     # one 12-mer at seven places
    parts = [r(1500, 16), lit("A", 100), r(80, 17), lit("AC", 60), r(80, 18), lit("ACG", 40), r(80, 19), lit("T", 64),
             r(80, 20), x, rc(x), r(80, 21), np.tile(unit30, 8), r(80, 22), np.tile(unit13, 10), r(80, 23), spread,
             r(80, 24), elem, r(300, 25), rc(elem), r(1500, 26)]
    return np.concatenate(parts)


@pytest.mark.parametrize("variant", [{}, {"VGMI_PTABLE": "0"}], ids=["path-table", "hash-drain"])
def test_small_graph_low_complexity_keys_match_oracle(variant, monkeypatch):
    for k_, v_ in variant.items():
        monkeypatch.setenv(k_, v_)
    rng = np.random.default_rng(9)
    seq = _low_complexity_sequence(rng)
    keys = np.unique(o.sketch(seq, 27))
    assert 3000 < keys.size <= 65536, keys.size
    from varigraph_amd import synth
    other = seq.copy()                          # reads of a diverged copy leave and re-enter the chains everywhere
    mut = rng.random(other.size) < 0.02
    other[mut] = synth._ACGT[(synth._CODE[other[mut]] + rng.integers(1, 4, size=int(mut.sum()))) % 4]
    n_reads = 40_000
    block = vgmi.synth_reads_host(31, 0, n_reads, 150, [seq, other])
    c = vgmi.Context(0, buffer_mib=16)
    try:
        c.table_upload(keys, 27)
        c.counts_reset()
        c.reads_submit(block, n_reads)
        cov, _, _ = c.counts_finish()
        t = o.Table(keys)
        t.count_block(block, 27)
        want = t.counts()
        assert np.array_equal(cov, want), (variant, int((cov != want).sum()))
        assert (cov == 255).any() and (cov < 255).any() and int(cov.astype(np.int64).sum()) > 500_000
    finally:
        c.close()


def test_small_graph_saturation_through_the_path_table():
    """Deep coverage of a tiny graph: every counter passes 254 -> 255 under contention from all wavefronts, the saturation
    bits of both places and the hash table's flag are set by exactly that increment, later hits skip their atomic, and a reset
    clears all of it (a shallow sample afterwards counts from zero)."""
    rng = np.random.default_rng(3)
    keys, haps = _small_graph("dense-sites", rng)
    n_reads = 3_000_000                        # 20 kb x 2 haplotypes: ~11 000 x
    c = vgmi.Context(0, buffer_mib=64)
    try:
        import torch
        c.table_upload(keys, 27)
        off = np.array([0, haps[0].size, haps[0].size + haps[1].size], dtype=np.uint64)
        d_cat = torch.from_numpy(np.concatenate(haps)).cuda()
        d_block = torch.empty(n_reads * 151, dtype=torch.uint8, device="cuda")
        c.synth_reads_device(77, 0, n_reads, 150, d_cat, off, d_block)
        c.counts_reset()
        c.reads_submit_device(d_block, d_block.numel(), n_reads)
        deep, _, _ = c.counts_finish()
        pre = 40_000
        small = d_block[: pre * 151].cpu().numpy()
        t = o.Table(keys)
        t.count_block(d_block.cpu().numpy(), 27)
        assert np.array_equal(deep, t.counts())
        assert (deep == 255).mean() > 0.4      # (keys pairing an allele with a neighbouring site's other allele are not on the sample)
        c.counts_reset()
        c.reads_submit(small, pre)
        shallow, _, _ = c.counts_finish()
        t.reset()
        t.count_block(small, 27)
        assert np.array_equal(shallow, t.counts()) and shallow.max() < 255
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------------------------
# Round 5: small graphs of odd k = 19 .. 25 through count27s_kernel<true, K> (the grid of 8: two grid 12-mers per lane and row, runs of
# K + 7 bases, 8 windows each) and the path table laid out for k.  VGMI_SMALLK=0 keeps the generic row kernel: the A/B reference.
@pytest.mark.parametrize("kind", ["plain", "repeats", "dense-sites"])
@pytest.mark.parametrize("k", [19, 21, 23, 25, 20, 22, 24, 26, 28])      # (26, 28: k + 7 bases do not fit a run -- the context table at any size, flanks of 10 / 11)
def test_small_graph_other_odd_k_fast_path_matches_oracle(kind, k):
    rng = np.random.default_rng({"plain": 1, "repeats": 2, "dense-sites": 3}[kind] + k)
    keys, haps = _small_graph(kind, rng, k)
    assert 1000 < keys.size <= 65536, keys.size
    n_reads = 60_000
    block = vgmi.synth_reads_host(23 + k, 0, n_reads, 150, haps)
    b2 = block.copy()
    idx = rng.choice(b2.size, size=3000, replace=False)
    idx = idx[b2[idx] != 10]
    b2[idx[:1500]] = ord("N")
    b2[idx[1500:]] |= 0x20
    c = vgmi.Context(0, buffer_mib=16)
    try:
        import torch
        c.table_upload(keys, k)
        assert (c.ctable_info()["n_buckets"] > 0) == (k in (26, 28))
        t = o.Table(keys)
        for blk in (block, b2):
            c.counts_reset()
            cuts = [0, 16 * 1000, 16 * 1000 + 16 * 37, n_reads]
            for a, e in zip(cuts[:-1], cuts[1:]):
                c.reads_submit(blk[a * 151:e * 151], e - a)
            cov, _, _ = c.counts_finish()
            t.reset()
            t.count_block(blk, k)
            want = t.counts()
            assert np.array_equal(cov, want), (kind, k, int((cov != want).sum()))
            # the same block resident on the device (the kernel reads its length from device memory on the FASTQ path; here the host's)
            c.counts_reset()
            d = torch.from_numpy(blk).cuda()
            d_off = (torch.arange(n_reads + 1, dtype=torch.int64, device="cuda") * 151) if k % 2 == 0 else None
            c.reads_submit_device(d, d.numel(), n_reads, d_off)
            cov_d, _, _ = c.counts_finish()
            assert np.array_equal(cov_d, want), (kind, k, "device")
        assert int(cov.astype(np.int64).sum()) > 50_000
        ms, launches = c.count_kernel_ms()
        assert launches > 0
    finally:
        c.close()


@pytest.mark.parametrize("k", [19, 25])
def test_small_graph_other_odd_k_every_kmer_counted_once_at_any_alignment(k):
    """The alignment matrix of test_every_kmer_counted_once_at_any_alignment for the grid of 8: a 400-base sequence whose k-mers are
    all graph k-mers at assorted stream offsets -- row and row-pair boundaries, the last positions in front of the ragged tail (the
    fast kernel covers every end inside its complete row pairs, the generic kernel starts at the first byte behind them)."""
    rng = np.random.default_rng(k)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    S = acgt[rng.integers(0, 4, size=400)].tobytes()
    keys_pos = o.sketch(S, k)
    uk, inv = np.unique(keys_pos, return_inverse=True)
    want = np.bincount(inv, minlength=uk.size).astype(np.uint8)
    c = vgmi.Context(0)
    try:
        c.table_upload(uk, k)
        for pre in [0, 1, 5, 7, 8, 9, 13, 100, 1000, 1019, 1023, 1024, 1025, 1500, 1630, 1640, 1647, 1648, 1649, 2040, 2047, 2048, 2049, 3000, 4090, 5000]:
            for post in [0, 3000]:
                filler = (b"N" * pre + b"\n") if pre else b""
                tail = (b"N" * post + b"\n") if post else b""
                blk = np.frombuffer(filler + S + b"\n" + tail, dtype=np.uint8)
                c.counts_reset()
                c.reads_submit(blk, 1 + (1 if pre else 0) + (1 if post else 0))
                cov, _, _ = c.counts_finish()
                assert np.array_equal(cov, want), (k, pre, post, int((cov != want).sum()))
    finally:
        c.close()


@pytest.mark.parametrize("k", [21, 23])
def test_small_graph_other_odd_k_low_complexity_and_saturation(k, monkeypatch):
    """Homopolymers, dinucleotide repeats, an element and its reverse complement: 12-mers with many places, palindromic 12-mers, k-mers
    next to their own reverse complement -- and enough reads that counters pass 254 -> 255 (saturation bits at both places of the
    path table, cleared by the reset).  The generic row kernel on the same table (VGMI_GENERIC_KERNEL through force_generic) agrees."""
    rng = np.random.default_rng(9 + k)
    seq = _low_complexity_sequence(rng)
    keys = np.unique(o.sketch(seq, k))
    assert 3000 < keys.size <= 65536, keys.size
    from varigraph_amd import synth
    other = seq.copy()
    mut = rng.random(other.size) < 0.02
    other[mut] = synth._ACGT[(synth._CODE[other[mut]] + rng.integers(1, 4, size=int(mut.sum()))) % 4]
    n_reads = 40_000
    block = vgmi.synth_reads_host(31 + k, 0, n_reads, 150, [seq, other])
    c = vgmi.Context(0, buffer_mib=16)
    try:
        c.table_upload(keys, k)
        t = o.Table(keys)
        t.count_block(block, k)
        want = t.counts()
        for rep in range(2):      # the second pass starts from a reset: saturation flags of the first are gone
            c.counts_reset()
            c.reads_submit(block, n_reads)
            cov, _, _ = c.counts_finish()
            assert np.array_equal(cov, want), (k, rep, int((cov != want).sum()))
        assert (cov == 255).any() and (cov < 255).any() and int(cov.astype(np.int64).sum()) > 500_000
        c.counts_reset()
        c.reads_submit(block[:151 * 2000], 2000)
        shallow, _, _ = c.counts_finish()
        t.reset()
        t.count_block(block[:151 * 2000], k)
        assert np.array_equal(shallow, t.counts())
    finally:
        c.close()
    monkeypatch.setenv("VGMI_SMALLK", "0")
    c = vgmi.Context(0, buffer_mib=16)
    try:
        c.table_upload(keys, k)
        c.counts_reset()
        c.reads_submit(block, n_reads)
        cov, _, _ = c.counts_finish()
        assert np.array_equal(cov, want)
    finally:
        c.close()


@pytest.mark.parametrize("k,big", [(20, False), (22, False), (24, False), (20, True), (22, True), (24, True), (26, False), (26, True), (28, False), (28, True)],
                         ids=["20", "22", "24", "20-context-table", "22-context-table", "24-context-table", "26-context-table-small", "26-context-table", "28-context-table-small", "28-context-table"])
def test_small_graph_even_k_run_counter_lag_is_taken_back(k, big):
    """Even k on the fast path (round 5).  The reference does not advance its run counter on a window that is its own reverse
    complement (src/kmer.cpp:134, `continue` before `++l`), registers included that still hold bases from in front of a non-base or the
    zeros in front of the read (:145 resets l only): the windows with  run of bases >= k > l  are not emitted.  Reads built to meet
    that -- starting with T^(k/2) (the phantom window A^(k/2) T^(k/2)), starting with a k-mer that is its own reverse complement, the
    same behind an N, two of them in a row -- with a key set that HOLDS the suppressed windows (the same reads sketched from other
    start offsets), deep enough that counters saturate, in pieces that put the reads into the rows of the fast kernel and into its
    ragged tail.  Counters must be the literal state machine's (the oracle)."""
    rng = np.random.default_rng(100 + k)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = {65: 84, 67: 71, 71: 67, 84: 65}

    def rnd(n):
        return acgt[rng.integers(0, 4, size=n)].tobytes()

    pals = []

    def own_rc():
        h = rnd(k // 2)
        pals.append(h + bytes(comp[b] for b in reversed(h)))
        return pals[-1]

    genome = rnd(3000)
    specials = []
    for i in range(40):
        body = genome[50 * i:50 * i + 110]
        specials += [b"T" * (k // 2) + body, own_rc() + body, body[:30] + b"N" + own_rc() + body[30:], own_rc() + own_rc() + body,
                     body[:40] + b"N" + b"T" * (k // 2 - 3) + body[40:], b"A" * 5 + b"T" * (k // 2) + body, own_rc()[: k - 1] + b"N" + body,
                     body[:k + 3] + own_rc() + body[k + 3:],
                     # (the scan form of the pass: non-bases in a row, two within k bases of each other, one at the read's end, lower case)
                     body[:30] + b"NN" + own_rc() + body[30:], body[:20] + b"N" + own_rc()[:5] + b"n" + own_rc() + body[20:], body + b"N",
                     (body[:30] + b"N" + own_rc() + body[30:]).lower(), body[:35] + b"." + own_rc()[1:] + body[35:]]
    plain = [genome[s:s + 150] for s in rng.integers(0, len(genome) - 150, size=3000)]
    # the key set: every window the literal state machine emits for the reads, for the reads less their first base, and with a base in front
    keysets = [o.sketch(r, k) for r in specials] + [o.sketch(r[1:], k) for r in specials] + [o.sketch(b"G" + r, k) for r in specials] + [o.sketch(genome, k)]
    keys = np.unique(np.concatenate(keysets))
    keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
    # ... and the k-mers that are their own reverse complement as keys (a key set of another emitter may hold them; the reference never
    # emits such a window, so their counters stay zero: no bit in the path table, no window bit in the context table)
    from varigraph_amd import synth
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    pal_codes = np.array([sum(code[b] << (2 * (k - 1 - i)) for i, b in enumerate(q)) for q in pals[:60]], dtype=np.uint64)
    keys = np.unique(np.concatenate([keys, (synth.hash64_np(pal_codes, k) << np.uint64(8)) | np.uint64(k)]))
    assert 1000 < keys.size <= 65536
    if big:
        # the same on a graph of more than 65 536 k-mers: countkc_kernel<K> over the context table behind the same pass (its debits go to
        # the table's counters by id); the extra keys are the emitter's own for another random sequence
        keys = np.unique(np.concatenate([keys, o.sketch(rnd(90_000), k)]))
        keys = keys[keys != np.uint64(0xFFFFFFFFFFFFFFFF)]
        assert keys.size > 80_000
    reads = (specials * 12 + plain)
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    block = np.frombuffer(b"".join(r + b"\n" for r in reads), dtype=np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) + 1 for r in reads])]).astype(np.uint64)
    t = o.Table(keys)
    t.count_block(block, k)
    want = t.counts()
    c = vgmi.Context(0, buffer_mib=16)
    try:
        import torch
        c.table_upload(keys, k)
        d = torch.from_numpy(block).cuda()
        d_off = torch.from_numpy(off.astype(np.int64)).cuda()
        c.counts_reset()
        c.reads_submit_device(d, d.numel(), len(reads), d_off)
        cov, _, _ = c.counts_finish()
        assert np.array_equal(cov, want), (k, int((cov != want).sum()), np.flatnonzero(cov != want)[:5], cov[cov != want][:5], want[cov != want][:5])
        assert (c.ctable_info()["n_buckets"] > 0) == (big or k in (26, 28))
        # the literal kernel on the same keys (the A/B)
        import os
        knob = "VGMI_CTABLE_K" if big or k in (26, 28) else "VGMI_SMALLK"
        os.environ[knob] = "0"
        try:
            g = vgmi.Context(0, buffer_mib=16)
            g.table_upload(keys, k)
            assert g.ctable_info()["n_buckets"] == 0
            g.counts_reset()
            g.reads_submit_device(d, d.numel(), len(reads), d_off)
            cov_g, _, _ = g.counts_finish()
            g.close()
        finally:
            os.environ.pop(knob)
        assert np.array_equal(cov_g, want)
        # deep: the same reads 30 times over -- counters pass the clamp with debits and increments of many launches in flight
        c.counts_reset()
        for _ in range(30):
            c.reads_submit_device(d, d.numel(), len(reads), d_off)
        deep, _, _ = c.counts_finish()
        want_deep = np.minimum(255, want.astype(np.int64) * 30).astype(np.uint8)
        assert np.array_equal(deep, want_deep), int((deep != want_deep).sum())
        assert (want_deep == 255).any() and (want_deep < 255).any()
        # host submit in ragged pieces (read offsets made by the library)
        c.counts_reset()
        cuts = [0, 700, 701, 1500, len(reads)]
        for a, e in zip(cuts[:-1], cuts[1:]):
            c.reads_submit(block[int(off[a]):int(off[e])], e - a)
        cov_h, _, _ = c.counts_finish()
        assert np.array_equal(cov_h, want)
        if k == 22:
            # more non-bases in ONE launch than the pass's lists of positions hold (2^20 in all): the rest is walked where the scan finds it
            some = [r for r in reads if b"N" in r or b"n" in r or b"." in r]
            many = some * (1 + 1_600_000 // sum(r.count(b"N") + r.count(b"n") + r.count(b".") for r in some))
            block_m = np.frombuffer(b"".join(r + b"\n" for r in many), dtype=np.uint8)
            off_m = np.concatenate([[0], np.cumsum([len(r) + 1 for r in many])]).astype(np.int64)
            t2 = o.Table(keys)
            t2.count_block(block_m, k)
            c.counts_reset()
            dm = torch.from_numpy(block_m).cuda()
            c.reads_submit_device(dm, dm.numel(), len(many), torch.from_numpy(off_m).cuda())
            cov_m, _, _ = c.counts_finish()
            assert np.array_equal(cov_m, t2.counts())
    finally:
        c.close()
