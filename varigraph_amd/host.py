"""ctypes binding of include/vghost.h (libvghost.so): graph.bin reader, FASTA/Q reader and the
sample-counting driver (C++17 host side).  No fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import vgmi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvghost.so")
_lib = None


class GraphInfo(C.Structure):
    _fields_ = [("graph_base_num", C.c_uint64), ("genome_size", C.c_uint64), ("n_keys", C.c_uint64),
                ("bitlen", C.c_uint64), ("n_variant_nodes", C.c_uint64), ("n_node_entries", C.c_uint64),
                ("k", C.c_uint32), ("vcf_ploidy", C.c_uint32), ("hap_num", C.c_uint32), ("n_chromosomes", C.c_uint32)]


class SampleStats(C.Structure):
    _fields_ = [("read_base", C.c_uint64), ("n_reads", C.c_uint64), ("read_depth", C.c_float),
                ("hap_kmer_coverage", C.c_float), ("max_coverage", C.c_uint8), ("hom_coverage", C.c_uint8),
                ("seconds_total", C.c_double), ("seconds_kernel", C.c_double)]


class GenotypeConfig(C.Structure):
    _fields_ = [("sample_type", C.c_char_p), ("sample_ploidy", C.c_uint32), ("haploid_num", C.c_uint32),
                ("chr_len_thread", C.c_uint32), ("transition", C.c_char_p), ("sv_only", C.c_int), ("threads", C.c_uint32),
                ("min_gq", C.c_float)]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    vgmi.lib()  # libvgmi.so first (libvghost links against it)
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -m varigraph_amd.build`")
    l = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    l.vgh_last_error.restype = C.c_char_p
    l.vgh_graph_load.restype = C.c_int; l.vgh_graph_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    l.vgh_graph_free.restype = None; l.vgh_graph_free.argtypes = [vp]
    l.vgh_graph_get_info.restype = C.c_int; l.vgh_graph_get_info.argtypes = [vp, C.POINTER(GraphInfo)]
    for name in ("keys", "f", "bitvec", "hom_flag", "node_off", "node_key_index", "node_start", "node_chr"):
        fn = getattr(l, "vgh_graph_" + name)
        fn.restype = vp
        fn.argtypes = [vp]
    l.vgh_graph_chr_name.restype = C.c_char_p; l.vgh_graph_chr_name.argtypes = [vp, C.c_uint32]
    l.vgh_graph_upload.restype = C.c_int; l.vgh_graph_upload.argtypes = [vp, vp]
    l.vgh_fastx_read_all.restype = C.c_int64
    l.vgh_fastx_read_all.argtypes = [C.c_char_p, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
    l.vgh_fastx_read_all_mt.restype = C.c_int64
    l.vgh_fastx_read_all_mt.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64),
                                        C.c_char_p]
    l.vgh_sniff_input.restype = C.c_int
    l.vgh_sniff_input.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    l.vgh_bam_read_all.restype = C.c_int64
    l.vgh_bam_read_all.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
    l.vgh_free.restype = None; l.vgh_free.argtypes = [vp]
    l.vgh_sample_count.restype = C.c_int
    l.vgh_sample_count.argtypes = [vp, vp, C.POINTER(C.c_char_p), C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, vp, vp, vp,
                                   C.POINTER(SampleStats)]
    l.vgh_sample_count_q.restype = C.c_int
    l.vgh_sample_count_q.argtypes = l.vgh_sample_count.argtypes + [C.c_uint32, C.POINTER(C.c_uint64)]
    l.vgh_sample_count_s.restype = C.c_int
    l.vgh_sample_count_s.argtypes = l.vgh_sample_count.argtypes + [C.c_uint32, C.c_double, C.c_uint64, C.POINTER(C.c_uint64),
                                                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    l.vgh_reads_read_all_s.restype = C.c_int64
    l.vgh_reads_read_all_s.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64, C.c_uint64, C.POINTER(vp),
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    l.vgh_sample_count_f.restype = C.c_int
    l.vgh_sample_count_f.argtypes = l.vgh_sample_count.argtypes + [C.c_uint32, C.c_double, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                                                   C.c_char_p, C.c_double] + [C.POINTER(C.c_uint64)] * 5
    l.vgh_sample_count_r.restype = C.c_int
    l.vgh_sample_count_r.argtypes = l.vgh_sample_count.argtypes + [C.c_uint32, C.c_double, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                                                   C.c_char_p, C.c_double, C.c_char_p, C.c_char_p, C.c_int] + [C.POINTER(C.c_uint64)] * 5
    l.vgh_reads_read_all_r.restype = C.c_int64
    l.vgh_reads_read_all_r.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_char_p, C.c_double, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vp),
                                       C.POINTER(C.c_size_t)] + [C.POINTER(C.c_uint64)] * 5
    l.vgh_sample_count_l.restype = C.c_int
    l.vgh_sample_count_l.argtypes = l.vgh_sample_count.argtypes + [C.c_uint32, C.c_double, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                                                   C.c_char_p, C.c_double, C.c_char_p, C.c_char_p, C.c_int,
                                                                   C.POINTER(vgmi.ReadFilter)] + [C.POINTER(C.c_uint64)] * 6
    l.vgh_reads_read_all_l.restype = C.c_int64
    l.vgh_reads_read_all_l.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_char_p, C.c_double, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(vgmi.ReadFilter),
                                       C.POINTER(vp), C.POINTER(C.c_size_t)] + [C.POINTER(C.c_uint64)] * 6
    l.vgh_parse_quality_tenths.restype = C.c_int
    l.vgh_parse_quality_tenths.argtypes = [C.c_char_p, C.POINTER(C.c_uint32)]
    l.vgh_reads_read_all_f.restype = C.c_int64
    l.vgh_reads_read_all_f.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                       C.c_uint32, C.c_char_p, C.c_double, C.POINTER(vp), C.POINTER(C.c_size_t)] + [C.POINTER(C.c_uint64)] * 5
    l.vgh_reads_read_all_q.restype = C.c_int64
    l.vgh_reads_read_all_q.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64)]
    l.vgh_bloom_reference_seeds.restype = C.c_int
    l.vgh_bloom_reference_seeds.argtypes = [C.c_uint32, C.c_uint32, vp]
    l.vgh_make_mbf.restype = C.c_int
    l.vgh_make_mbf.argtypes = [vp, C.c_char_p, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    l.vgh_coverage_stats.restype = C.c_int
    l.vgh_coverage_stats.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(SampleStats)]
    l.vgh_genotype_config_default.restype = None; l.vgh_genotype_config_default.argtypes = [C.POINTER(GenotypeConfig)]
    l.vgh_genotyper_create.restype = C.c_int; l.vgh_genotyper_create.argtypes = [vp, C.POINTER(vp)]
    l.vgh_genotyper_free.restype = None; l.vgh_genotyper_free.argtypes = [vp]
    l.vgh_genotype.restype = C.c_int
    l.vgh_genotype.argtypes = [vp, vp, C.c_float, C.c_char_p, C.POINTER(GenotypeConfig), C.POINTER(vp), C.POINTER(C.c_size_t)]
    _lib = l
    return l


def _arr(ptr, n, dtype):
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype).copy()


class Graph:
    """A loaded graph.bin (host arrays stay in the C++ object; numpy copies on request)."""

    def __init__(self, path):
        self._l = lib()
        h = C.c_void_p()
        rc = self._l.vgh_graph_load(os.fsencode(path), C.byref(h))
        if rc:
            raise RuntimeError(self._l.vgh_last_error().decode())
        self._h = h
        info = GraphInfo()
        self._l.vgh_graph_get_info(h, C.byref(info))
        self.info = {f[0]: getattr(info, f[0]) for f in GraphInfo._fields_}

    def close(self):
        if getattr(self, "_h", None):
            self._l.vgh_graph_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def arrays(self):
        i = self.info
        l, h = self._l, self._h
        n, nv, ne = i["n_keys"], i["n_variant_nodes"], i["n_node_entries"]
        return {
            "k": i["k"], "vcf_ploidy": i["vcf_ploidy"], "hap_num": i["hap_num"], "genome_size": i["genome_size"],
            "keys": _arr(l.vgh_graph_keys(h), n, np.uint64),
            "f": _arr(l.vgh_graph_f(h), n, np.uint8),
            "bitvec": _arr(l.vgh_graph_bitvec(h), n * i["bitlen"], np.int8).reshape(n, i["bitlen"]),
            "hom_flag": _arr(l.vgh_graph_hom_flag(h), n, np.uint8),
            "node_off": _arr(l.vgh_graph_node_off(h), nv + 1, np.uint64),
            "node_key_index": _arr(l.vgh_graph_node_key_index(h), ne, np.uint32),
            "node_start": _arr(l.vgh_graph_node_start(h), nv, np.uint32),
            "node_chr": _arr(l.vgh_graph_node_chr(h), nv, np.uint32),
            "chr_names": [l.vgh_graph_chr_name(h, c).decode() for c in range(i["n_chromosomes"])],
        }

    def upload(self, ctx):
        rc = self._l.vgh_graph_upload(self._h, ctx._h)
        if rc:
            raise vgmi.VgmiError(rc, self._l.vgh_last_error().decode())
        ctx.n_keys = self.info["n_keys"]
        ctx.n_node_entries = self.info["n_node_entries"]

    def reads_index_save(self, path, cov, read_base):
        """FastqKmer::save_index: the reference's per-sample dump of the k-mer table."""
        cov = np.ascontiguousarray(cov, dtype=np.uint8)
        assert cov.size == self.info["n_keys"]
        self._l.vgh_reads_index_save.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p]
        if self._l.vgh_reads_index_save(self._h, vgmi._ptr(cov), int(read_base), os.fsencode(path)):
            raise RuntimeError(self._l.vgh_last_error().decode())

    def reads_index_load(self, path):
        cov = np.empty(self.info["n_keys"], dtype=np.uint8)
        rb = C.c_uint64()
        self._l.vgh_reads_index_load.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_uint64)]
        if self._l.vgh_reads_index_load(self._h, os.fsencode(path), vgmi._ptr(cov), C.byref(rb)):
            raise RuntimeError(self._l.vgh_last_error().decode())
        return cov, rb.value

    def sample_count(self, ctx, fastq_paths, threads=4, sample_ploidy=2, use_depth=False, require_depth=True, min_base_quality=0,
                     subsample=None, bam_filter=None, bam_regions=None, bam_regions_bed=None, bam_unplaced=False, read_filter=None):
        """FastqKmerHip::build_fastq_index + coverage statistics for one sample.  require_depth=False: a sample too thin
        for the coverage peak (the reference exits with "Failed to retrieve depth information") still returns its
        counters.  min_base_quality: bases of FASTQ / BAM reads whose quality is below it are counted as N (vgh_sample_count_q);
        stats["masked_bases"] = how many, device and host readers together.  subsample=(F, S): a seeded fraction of every file's
        reads is kept (vgh_sample_count_s); stats then has reads_seen and reads_kept, and n_reads / read_base are the kept reads'.
        bam_filter=dict(exclude=0x900, require=0, min_mapq=0, tag=None, min_value=0.0), any key optional: the read filter of BAM files
        (vgh_sample_count_f); stats then has bam_records and bam_reads.  bam_regions="NAME,NAME:BEG-END,...", bam_regions_bed=a BED
        file's path, bam_unplaced: the regions of BAM files (vgh_sample_count_r), alone or with bam_filter; stats has bam_records and
        bam_reads then too.  read_filter=dict(min_len, max_len, min_mean_q (tenths), lowq_below, lowq_max_pct), any key optional: the
        read filter by length and read quality (vgh_sample_count_l), with any of the above; stats then has read_filter_stats =
        (evaluated, short, long, low fraction, low mean).  Without it the calls are those of before."""
        i = self.info
        cov = np.empty(i["n_keys"], dtype=np.uint8)
        cov_node = np.empty(i["n_node_entries"], dtype=np.uint8)
        hist = np.zeros(256, dtype=np.uint64)
        st = SampleStats()
        arr = (C.c_char_p * len(fastq_paths))(*[os.fsencode(p) for p in fastq_paths])
        masked, seen, kept = C.c_uint64(), C.c_uint64(), C.c_uint64()
        recs, rds = C.c_uint64(), C.c_uint64()
        regions = bam_regions is not None or bam_regions_bed is not None or bam_unplaced
        rfs = (C.c_uint64 * 5)()
        if read_filter is not None:
            f, fs = bam_filter_args(bam_filter or {}), subsample if subsample is not None else (1.0, 0)
            rf = vgmi.read_filter_struct(read_filter)
            rc = self._l.vgh_sample_count_l(self._h, ctx._h, arr, len(fastq_paths), threads, sample_ploidy, int(use_depth),
                                            vgmi._ptr(cov), vgmi._ptr(cov_node), vgmi._ptr(hist), C.byref(st), min_base_quality,
                                            float(fs[0]), int(fs[1]), *f, *_region_args(bam_regions, bam_regions_bed), int(bool(bam_unplaced)),
                                            C.byref(rf), C.byref(seen), C.byref(kept), C.byref(masked), C.byref(recs), C.byref(rds), rfs)
        elif regions:
            f, fs = bam_filter_args(bam_filter or {}), subsample if subsample is not None else (1.0, 0)
            rc = self._l.vgh_sample_count_r(self._h, ctx._h, arr, len(fastq_paths), threads, sample_ploidy, int(use_depth),
                                            vgmi._ptr(cov), vgmi._ptr(cov_node), vgmi._ptr(hist), C.byref(st), min_base_quality,
                                            float(fs[0]), int(fs[1]), *f, _region_args(bam_regions, bam_regions_bed)[0],
                                            _region_args(bam_regions, bam_regions_bed)[1], int(bool(bam_unplaced)), C.byref(seen),
                                            C.byref(kept), C.byref(masked), C.byref(recs), C.byref(rds))
        elif bam_filter is not None:
            f, fs = bam_filter_args(bam_filter), subsample if subsample is not None else (1.0, 0)
            rc = self._l.vgh_sample_count_f(self._h, ctx._h, arr, len(fastq_paths), threads, sample_ploidy, int(use_depth),
                                            vgmi._ptr(cov), vgmi._ptr(cov_node), vgmi._ptr(hist), C.byref(st), min_base_quality,
                                            float(fs[0]), int(fs[1]), *f, C.byref(seen), C.byref(kept), C.byref(masked),
                                            C.byref(recs), C.byref(rds))
        elif subsample is not None:
            rc = self._l.vgh_sample_count_s(self._h, ctx._h, arr, len(fastq_paths), threads, sample_ploidy, int(use_depth),
                                            vgmi._ptr(cov), vgmi._ptr(cov_node), vgmi._ptr(hist), C.byref(st), min_base_quality,
                                            float(subsample[0]), int(subsample[1]), C.byref(seen), C.byref(kept), C.byref(masked))
        elif min_base_quality:
            rc = self._l.vgh_sample_count_q(self._h, ctx._h, arr, len(fastq_paths), threads, sample_ploidy, int(use_depth),
                                            vgmi._ptr(cov), vgmi._ptr(cov_node), vgmi._ptr(hist), C.byref(st), min_base_quality, C.byref(masked))
        else:
            rc = self._l.vgh_sample_count(self._h, ctx._h, arr, len(fastq_paths), threads, sample_ploidy, int(use_depth),
                                          vgmi._ptr(cov), vgmi._ptr(cov_node), vgmi._ptr(hist), C.byref(st))
        if rc and (require_depth or b"Failed to retrieve depth" not in self._l.vgh_last_error()):
            raise vgmi.VgmiError(rc, self._l.vgh_last_error().decode())
        stats = {f[0]: getattr(st, f[0]) for f in SampleStats._fields_}
        stats["masked_bases"] = masked.value
        if subsample is not None:
            stats["reads_seen"], stats["reads_kept"] = seen.value, kept.value
        if bam_filter is not None or regions:
            stats["bam_records"], stats["bam_reads"] = recs.value, rds.value
        if read_filter is not None:
            stats["read_filter_stats"] = tuple(int(v) for v in rfs)
        return cov, cov_node, hist, stats


def coverage_stats(hist, read_base, genome_size, sample_ploidy=2, use_depth=False):
    """ReadDepth_ / hapKmerCoverage_ / peaks from a masked coverage histogram (host arithmetic of the reference)."""
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    st = SampleStats()
    rc = lib().vgh_coverage_stats(hist.ctypes.data_as(C.c_void_p), int(read_base), int(genome_size), sample_ploidy,
                                  1 if use_depth else 0, C.byref(st))
    if rc:
        raise RuntimeError(lib().vgh_last_error().decode())
    return {f[0]: getattr(st, f[0]) for f in SampleStats._fields_}


class Genotyper:
    """Host HMM of `genotype` (include/vghost.h): keeps the per-node k-mer lists across samples like the reference."""

    def __init__(self, graph):
        self._l = lib()
        self._graph = graph   # keeps the C++ graph alive
        h = C.c_void_p()
        rc = self._l.vgh_genotyper_create(graph._h, C.byref(h))
        if rc:
            raise RuntimeError(self._l.vgh_last_error().decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._l.vgh_genotyper_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, cov, hap_kmer_coverage, sample_name, sample_type="het", sample_ploidy=2, haploid_num=15,
            granularity_bp=1000000, transition="rec", sv_only=False, threads=4, min_gq=0.0):
        """cov: c per key in graph.bin record order.  Returns the VCF text (bytes)."""
        cov = np.ascontiguousarray(cov, dtype=np.uint8)
        assert cov.size == self._graph.info["n_keys"]
        cfg = GenotypeConfig()
        self._l.vgh_genotype_config_default(C.byref(cfg))
        st, tr = sample_type.encode(), transition.encode()
        cfg.sample_type, cfg.transition = st, tr
        cfg.sample_ploidy, cfg.haploid_num, cfg.chr_len_thread = sample_ploidy, haploid_num, granularity_bp
        cfg.sv_only, cfg.threads, cfg.min_gq = int(sv_only), threads, min_gq
        out, n = C.c_void_p(), C.c_size_t()
        rc = self._l.vgh_genotype(self._h, cov.ctypes.data_as(C.c_void_p), C.c_float(hap_kmer_coverage),
                                  sample_name.encode(), C.byref(cfg), C.byref(out), C.byref(n))
        if rc:
            raise RuntimeError(self._l.vgh_last_error().decode())
        try:
            return C.string_at(out, n.value)
        finally:
            self._l.vgh_free(out)


def load_graph(path):
    """graph.bin -> dict of numpy arrays (keys, f, bitvec, hom_flag, node CSR, ...)."""
    g = Graph(path)
    try:
        return g.arrays()
    finally:
        g.close()


def write_vcf_gz(path, text, threads=1):
    """`text` (bytes) as block gzip, the way `varigraph-mi genotype` writes <sample>.varigraph.vcf.gz."""
    l = lib()
    l.vgh_write_vcf_gz.restype = C.c_int
    l.vgh_write_vcf_gz.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.c_uint32]
    if l.vgh_write_vcf_gz(os.fsencode(path), text, len(text), threads):
        raise RuntimeError(l.vgh_last_error().decode())


def fastx_read_all(path, decode_threads=1, with_kind=False):
    """All records of a FASTA/Q(.gz) file as a '\\n'-joined block (kseq_read semantics).  with_kind: also how the
    bytes were decoded ("plain" | "gzip" | "bgzf", csrc/host/byte_source.hpp)."""
    l = lib()
    p, n, rb = C.c_void_p(), C.c_size_t(), C.c_uint64()
    kind = C.create_string_buffer(8)
    cnt = l.vgh_fastx_read_all_mt(os.fsencode(path), decode_threads, C.byref(p), C.byref(n), C.byref(rb), kind)
    if cnt < 0:
        raise RuntimeError(l.vgh_last_error().decode())
    try:
        block = _arr(p.value, n.value, np.uint8)
    finally:
        l.vgh_free(p)
    if with_kind:
        return block, int(cnt), rb.value, kind.value.decode()
    return block, int(cnt), rb.value


def reads_read_all_q(path, min_base_quality, decode_threads=1):
    """A FASTA/Q or BAM file through the host reader with a minimum base quality (vgh_reads_read_all_q): (block, n_reads, read_base,
    masked_bases) -- the block fastx_read_all / bam_read_all give, with the bases below the bound as N."""
    l = lib()
    p, n, rb, mb = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64()
    cnt = l.vgh_reads_read_all_q(os.fsencode(path), decode_threads, min_base_quality, C.byref(p), C.byref(n), C.byref(rb), C.byref(mb))
    if cnt < 0:
        raise RuntimeError(l.vgh_last_error().decode())
    try:
        block = _arr(p.value, n.value, np.uint8)
    finally:
        l.vgh_free(p)
    return block, int(cnt), rb.value, mb.value


def reads_read_all_s(path, fraction, seed, first_number=0, min_base_quality=0, decode_threads=1):
    """A FASTA/Q or BAM file through the host reader with subsampling (vgh_reads_read_all_s): (block, n_kept, read_base, masked_bases,
    next_number) -- the block of reads_read_all_q with the dropped reads left out, the file's reads numbered from first_number."""
    l = lib()
    p, n, rb, mb, nx = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    cnt = l.vgh_reads_read_all_s(os.fsencode(path), decode_threads, min_base_quality, fraction, seed, first_number, C.byref(p), C.byref(n),
                                 C.byref(rb), C.byref(mb), C.byref(nx))
    if cnt < 0:
        raise RuntimeError(l.vgh_last_error().decode())
    try:
        block = _arr(p.value, n.value, np.uint8)
    finally:
        l.vgh_free(p)
    return block, int(cnt), rb.value, mb.value, nx.value


def bam_filter_args(bam_filter):
    """(exclude, require, min_mapq, tag, min_value) of a bam_filter dict as the C entries take them"""
    tag = bam_filter.get("tag")
    return (int(bam_filter.get("exclude", 0x900)), int(bam_filter.get("require", 0)), int(bam_filter.get("min_mapq", 0)),
            None if tag is None else (tag if isinstance(tag, bytes) else tag.encode()), float(bam_filter.get("min_value", 0.0)))


def reads_read_all_f(path, bam_filter, fraction=1.0, seed=11, first_number=0, min_base_quality=0, decode_threads=1):
    """A BAM (or FASTA/Q) file through the host reader with the read filter (vgh_reads_read_all_f): (block, n_kept, read_base,
    masked_bases, next_number, bam_records, bam_reads).  bam_filter: the dict of Graph.sample_count."""
    l = lib()
    p, n, rb, mb, nx, rc, rd = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    cnt = l.vgh_reads_read_all_f(os.fsencode(path), decode_threads, min_base_quality, fraction, seed, first_number, *bam_filter_args(bam_filter),
                                 C.byref(p), C.byref(n), C.byref(rb), C.byref(mb), C.byref(nx), C.byref(rc), C.byref(rd))
    if cnt < 0:
        raise RuntimeError(l.vgh_last_error().decode())
    try:
        block = _arr(p.value, n.value, np.uint8)
    finally:
        l.vgh_free(p)
    return block, int(cnt), rb.value, mb.value, nx.value, rc.value, rd.value


def _region_args(bam_regions, bam_regions_bed):
    """(list, bed) as the C entries take them: bam_regions a string or a sequence of items, bam_regions_bed a path; None stays NULL"""
    if bam_regions is not None and not isinstance(bam_regions, (str, bytes)):
        bam_regions = ",".join(bam_regions)
    return (None if bam_regions is None else os.fsencode(bam_regions), None if bam_regions_bed is None else os.fsencode(bam_regions_bed))


def reads_read_all_r(path, bam_regions=None, bam_regions_bed=None, bam_unplaced=False, bam_filter=None, fraction=1.0, seed=11, first_number=0,
                     min_base_quality=0, decode_threads=1):
    """A BAM (or FASTA/Q) file through the host reader with regions (vgh_reads_read_all_r), with or without the read filter: the
    tuple of reads_read_all_f."""
    l = lib()
    p, n, rb, mb, nx, rc, rd = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    cnt = l.vgh_reads_read_all_r(os.fsencode(path), decode_threads, min_base_quality, fraction, seed, first_number,
                                 *bam_filter_args(bam_filter or {}), *_region_args(bam_regions, bam_regions_bed), int(bool(bam_unplaced)),
                                 C.byref(p), C.byref(n), C.byref(rb), C.byref(mb), C.byref(nx), C.byref(rc), C.byref(rd))
    if cnt < 0:
        raise RuntimeError(l.vgh_last_error().decode())
    try:
        block = _arr(p.value, n.value, np.uint8)
    finally:
        l.vgh_free(p)
    return block, int(cnt), rb.value, mb.value, nx.value, rc.value, rd.value


def reads_read_all_l(path, read_filter, bam_regions=None, bam_regions_bed=None, bam_unplaced=False, bam_filter=None, fraction=1.0, seed=11,
                     first_number=0, min_base_quality=0, decode_threads=1):
    """A file through the host reader with the read filter by length and read quality (vgh_reads_read_all_l; read_filter: the dict of
    Graph.sample_count, or None), with or without the others: the tuple of reads_read_all_f + (read_filter_stats,), the 5 values
    (evaluated, short, long, low fraction, low mean)."""
    l = lib()
    p, n, rb, mb, nx, rc, rd = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    rfs = (C.c_uint64 * 5)()
    rf = None if read_filter is None else C.byref(vgmi.read_filter_struct(read_filter))
    cnt = l.vgh_reads_read_all_l(os.fsencode(path), decode_threads, min_base_quality, fraction, seed, first_number,
                                 *bam_filter_args(bam_filter or {}), *_region_args(bam_regions, bam_regions_bed), int(bool(bam_unplaced)), rf,
                                 C.byref(p), C.byref(n), C.byref(rb), C.byref(mb), C.byref(nx), C.byref(rc), C.byref(rd), rfs)
    if cnt < 0:
        raise RuntimeError(l.vgh_last_error().decode())
    try:
        block = _arr(p.value, n.value, np.uint8)
    finally:
        l.vgh_free(p)
    return block, int(cnt), rb.value, mb.value, nx.value, rc.value, rd.value, tuple(int(v) for v in rfs)


def parse_quality_tenths(text):
    """--min-read-quality's text as tenths (vgh_parse_quality_tenths); ValueError for what the CLI refuses"""
    l = lib()
    t = C.c_uint32()
    if l.vgh_parse_quality_tenths(os.fsencode(text), C.byref(t)):
        raise ValueError(l.vgh_last_error().decode())
    return t.value


def sniff_input(path):
    """What the device path makes of an input file, from its first bytes (vgh_sniff_input; no device involved):
    dict(kind, first_byte, bam, fasta)."""
    l = lib()
    kind = C.create_string_buffer(8)
    first, bam, fasta = C.c_int(), C.c_int(), C.c_int()
    if l.vgh_sniff_input(os.fsencode(path), kind, C.byref(first), C.byref(bam), C.byref(fasta)) != 0:
        raise RuntimeError(l.vgh_last_error().decode())
    return {"kind": kind.value.decode(), "first_byte": first.value, "bam": bool(bam.value), "fasta": bool(fasta.value)}


def bam_read_all(path, decode_threads=1):
    """The reads of a BAM / unaligned BAM file through the host decoder (csrc/host/bam_reader.hpp) as a '\\n'-joined block:
    (block, n_reads, read_base).  A malformed record raises RuntimeError naming its decompressed byte."""
    l = lib()
    p, n, rb = C.c_void_p(), C.c_size_t(), C.c_uint64()
    cnt = l.vgh_bam_read_all(os.fsencode(path), decode_threads, C.byref(p), C.byref(n), C.byref(rb))
    if cnt < 0:
        raise RuntimeError(l.vgh_last_error().decode())
    try:
        block = _arr(p.value, n.value, np.uint8)
    finally:
        l.vgh_free(p)
    return block, int(cnt), rb.value


def bloom_reference_seeds(random_device_value, n_hash):
    out = np.zeros(n_hash, dtype=np.uint64)
    rc = lib().vgh_bloom_reference_seeds(random_device_value, n_hash, vgmi._ptr(out))
    if rc:
        raise RuntimeError("vgh_bloom_reference_seeds")
    return out


def make_mbf(ctx, fasta_path, k, seeds=None, random_device_value=0):
    """build_fasta_index + make_mbf with the Bloom filter on the device; returns (genome_size, m, n_hash)."""
    l = lib()
    gs, m, nh = C.c_uint64(), C.c_uint64(), C.c_uint32()
    if seeds is not None:
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
    rc = l.vgh_make_mbf(ctx._h, os.fsencode(fasta_path), k, vgmi._ptr(seeds), 0 if seeds is None else seeds.size,
                        random_device_value, C.byref(gs), C.byref(m), C.byref(nh))
    if rc:
        raise vgmi.VgmiError(rc, l.vgh_last_error().decode())
    ctx._bloom_m = m.value
    return gs.value, m.value, nh.value
