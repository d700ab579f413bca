/*
 * vghost.h -- C API of the C++17 host side (libvghost.so): the callers and data formats either
 * side of the device hot path, restated from the reference for the MI355X build.
 *
 *   graph.bin reader + graph2node     ConstructIndex::load_index / graph2node
 *                                     (src/construct_index.cpp:911-1105, :710-751,1572-1603)
 *   FASTA/Q reader                    kseq_read semantics (include/kseq.h:192-232) as used by
 *                                     FastqKmer::fastq_file_open (src/fastq_kmer.cpp:65-187)
 *   sample counting driver            FastqKmer::build_fastq_index (src/fastq_kmer.cpp:41-52) over vgmi.h
 *   coverage statistics               Varigraph::kmer_read / cal_ave_cov_kmer / get_hom_kmer_c /
 *                                     cal_hap_kmer_cov (src/varigraph.cpp:185-243,308-362)
 *
 *   genotyping HMM + VCF text         GENOTYPE::genotype / for_bac_post_run / hidden_states / forward / backward /
 *                                     posterior / save (src/genotype.cpp), HaplotypeSelect (src/haplotype_select.cpp),
 *                                     find_node_up_down_seq (src/construct_index.cpp:1266-1549)
 *
 * The C++ classes behind it (GraphIndex, FastxReader, FastqKmerHip, Genotyper) are in
 * varigraph_amd/csrc/host/; INTEGRATION.md shows how they slot into the reference.
 */
#ifndef VGHOST_H
#define VGHOST_H
#include <stddef.h>
#include <stdint.h>

#include "vgmi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vgh_graph vgh_graph;

typedef struct vgh_graph_info {
    uint64_t graph_base_num;  /* mGraphBaseNum */
    uint64_t genome_size;     /* mGenomeSize after load(): sum of lengths of chromosomes in mVcfInfoMap (construct_index.cpp:959-960) */
    uint64_t n_keys;          /* mGraphKmerHashHapStrMap.size() */
    uint64_t bitlen;          /* BitVec bytes per key */
    uint64_t n_variant_nodes; /* nodes with hapGtVec.size() > 1 */
    uint64_t n_node_entries;  /* sum over variant nodes of kept k-mers (<= 128 each) */
    uint32_t k;               /* mKmerLen */
    uint32_t vcf_ploidy;      /* mVcfPloidy */
    uint32_t hap_num;         /* mHapNum */
    uint32_t n_chromosomes;
} vgh_graph_info;

const char *vgh_last_error(void);

/* graph.bin (plain or gzip) -> flat host arrays.  Key order = file record order. */
int vgh_graph_load(const char *path, vgh_graph **out);
void vgh_graph_free(vgh_graph *g);
int vgh_graph_get_info(const vgh_graph *g, vgh_graph_info *info);
const uint64_t *vgh_graph_keys(const vgh_graph *g);           /* n_keys */
const uint8_t *vgh_graph_f(const vgh_graph *g);               /* n_keys */
const int8_t *vgh_graph_bitvec(const vgh_graph *g);           /* n_keys * bitlen */
const uint8_t *vgh_graph_hom_flag(const vgh_graph *g);        /* n_keys; A8 predicate, see vgmi_flags_upload */
const uint64_t *vgh_graph_node_off(const vgh_graph *g);       /* n_variant_nodes + 1 */
const uint32_t *vgh_graph_node_key_index(const vgh_graph *g); /* n_node_entries, graph2node order */
const uint32_t *vgh_graph_node_start(const vgh_graph *g);     /* n_variant_nodes: nodeStart (1-based) */
const uint32_t *vgh_graph_node_chr(const vgh_graph *g);       /* n_variant_nodes: chromosome ordinal (lexicographic) */
const char *vgh_graph_chr_name(const vgh_graph *g, uint32_t chr);
/* table + node CSR + flags -> device context */
int vgh_graph_upload(const vgh_graph *g, vgmi_ctx *ctx);

/* The reference's per-sample dump of the k-mer table (FastqKmer::save_index / load_index, src/fastq_kmer.cpp:200-298; public but
 * never called by its CLI): u64 ReadBase, then every record of the graph's k-mer table as
 * u64 key | u8 c | u8 f | u64 bitLen | i8[bitLen] -- graph.bin's last section with the sample's coverage in c -- in the
 * iteration order of the reference's unordered_map after load_index (derived, csrc/host/stl_order_map.hpp).
 * save writes exactly the bytes the reference writes for the same counters; load accepts the records in any order (the
 * reference loads them into a map) and fails on a key the graph does not hold. cov: n_keys bytes in key order. */
int vgh_reads_index_save(const vgh_graph *g, const uint8_t *cov, uint64_t read_base, const char *path);
int vgh_reads_index_load(const vgh_graph *g, const char *path, uint8_t *cov, uint64_t *read_base);

/* FASTA/Q files -> '\n'-joined read block appended to a caller buffer (for tests of the parser).
 * Returns the number of reads, or <0.  *read_base gets sum(seq.l). */
int64_t vgh_fastx_read_all(const char *path, char **block_out, size_t *n_bytes_out, uint64_t *read_base);
/* same with `decode_threads` inflate workers for block-gzip (BGZF) input; source_kind (may be NULL) gets "plain",
 * "gzip" or "bgzf": how the bytes were decoded (csrc/host/byte_source.hpp) */
int64_t vgh_fastx_read_all_mt(const char *path, uint32_t decode_threads, char **block_out, size_t *n_bytes_out,
                              uint64_t *read_base, char source_kind[8]);
/* A BAM / unaligned BAM file through the host decoder (csrc/host/bam_reader.hpp): the same block of its reads (flag & 0x900 == 0,
 * l_seq > 0; SEQ decoded as stored).  Returns the number of reads, or <0 (vgh_last_error: "'<path>': not a valid BAM record at
 * decompressed byte N (<what>)", or a file that is not BAM).  *read_base gets sum(l_seq). */
int64_t vgh_bam_read_all(const char *path, uint32_t decode_threads, char **block_out, size_t *n_bytes_out, uint64_t *read_base);
/* A FASTA/Q or BAM file (by its content, as vgh_sample_count decides) through the host reader with a minimum base quality: the same
 * block with every base whose quality is below min_base_quality written as 'N' (the rule of vgmi_fastq_set_min_quality: FASTQ byte
 * < 33 + q, BAM QUAL[i] < q and no masking where QUAL[0] is 0xff, FASTA untouched).  *masked_bases (may be NULL) = bases masked;
 * *read_base as without the option.  VGMI_E_INVALID for min_base_quality > 93.  What the host legs of vgh_sample_count_q apply.
 * Like the two entries above, an entry for tests of the readers: the three share one loop, this one with the bound. */
int64_t vgh_reads_read_all_q(const char *path, uint32_t decode_threads, uint32_t min_base_quality, char **block_out, size_t *n_bytes_out,
                             uint64_t *read_base, uint64_t *masked_bases);
/* The same with subsampling (the rule of vgmi_fastq_set_subsample; fraction 1 = off): the file's reads are numbered first_number,
 * first_number + 1, ... in file order (FASTA/Q: the records; BAM: the records that pass the read filter) and the block holds the
 * kept ones only; *read_base and *masked_bases are theirs.  *next_number (may be NULL) = first_number + the reads numbered.  Returns
 * the number of kept reads.  VGMI_E_INVALID for a fraction that is NaN, <= 0 or > 1.  first_number > 0 is the host reader taking a
 * file over from the device: reading a whole file from number n gives what a reader that starts n reads into it would. */
int64_t vgh_reads_read_all_s(const char *path, uint32_t decode_threads, uint32_t min_base_quality, double fraction, uint64_t seed,
                             uint64_t first_number, char **block_out, size_t *n_bytes_out, uint64_t *read_base, uint64_t *masked_bases,
                             uint64_t *next_number);
/* The same with the read filter of BAM files (the rule of vgmi_fastq_set_bam_filter, which has the parameters' ranges; bam_tag NULL:
 * no tag bound; exclude 0x900, require 0, min_mapq 0, no tag: vgh_reads_read_all_s): a record the filter drops is not a read, and
 * subsampling numbers the reads that passed.  *bam_records, *bam_reads (may be NULL) = the valid records examined and the reads
 * among them, before subsampling.  A record whose auxiliary fields cannot be walked ends the call with "'<path>': not a valid BAM
 * record at decompressed byte N (auxiliary fields)".  A FASTA/Q file is read as without the filter.  VGMI_E_INVALID for a parameter
 * out of range. */
int64_t vgh_reads_read_all_f(const char *path, uint32_t decode_threads, uint32_t min_base_quality, double fraction, uint64_t seed,
                             uint64_t first_number, uint32_t bam_exclude, uint32_t bam_require, uint32_t bam_min_mapq, const char *bam_tag,
                             double bam_min_value, char **block_out, size_t *n_bytes_out, uint64_t *read_base, uint64_t *masked_bases,
                             uint64_t *next_number, uint64_t *bam_records, uint64_t *bam_reads);
/* The same with regions for BAM files (condition 5 of the rule, vgmi_fastq_set_bam_regions): bam_regions = a comma-separated list of
 * NAME, NAME:BEG or NAME:BEG-END (1-based inclusive; an item that is a reference name as a whole is that reference, else it is split
 * at its last ':'), bam_regions_bed = the path of a BED file (columns 1 to 3, 0-based half-open; empty lines and lines starting with
 * '#', "track" or "browser" skipped; lines whose name the header lacks skipped), either may be NULL, both are joined; bam_unplaced:
 * records with refID -1 pass.  Resolved against the file's own header.  Both NULL: vgh_reads_read_all_f.  VGMI_E_INVALID with
 * "'<path>': reference '<name>' of region '<item>' is not in the header", for a BED line with start >= end or a non-number (the
 * message names the line), for a list that comes out empty, and for bam_unplaced without regions. */
int64_t vgh_reads_read_all_r(const char *path, uint32_t decode_threads, uint32_t min_base_quality, double fraction, uint64_t seed,
                             uint64_t first_number, uint32_t bam_exclude, uint32_t bam_require, uint32_t bam_min_mapq, const char *bam_tag,
                             double bam_min_value, const char *bam_regions, const char *bam_regions_bed, int bam_unplaced, char **block_out,
                             size_t *n_bytes_out, uint64_t *read_base, uint64_t *masked_bases, uint64_t *next_number, uint64_t *bam_records,
                             uint64_t *bam_reads);
/* The same with the read filter by length and read quality (the rule of vgmi_fastq_set_read_filter, csrc/vgmi_read_filter.h), applied
 * behind subsampling on the file's own qualities: the block holds the reads that pass.  read_filter NULL or all zero:
 * vgh_reads_read_all_r.  read_filter_stats (may be NULL): 5 values -- the reads evaluated (those subsampling kept), then the reads
 * dropped as short, long, low fraction, low mean.  VGMI_E_INVALID, with the field's message, for a field out of range. */
int64_t vgh_reads_read_all_l(const char *path, uint32_t decode_threads, uint32_t min_base_quality, double fraction, uint64_t seed,
                             uint64_t first_number, uint32_t bam_exclude, uint32_t bam_require, uint32_t bam_min_mapq, const char *bam_tag,
                             double bam_min_value, const char *bam_regions, const char *bam_regions_bed, int bam_unplaced,
                             const vgmi_read_filter *read_filter, char **block_out, size_t *n_bytes_out, uint64_t *read_base,
                             uint64_t *masked_bases, uint64_t *next_number, uint64_t *bam_records, uint64_t *bam_reads,
                             uint64_t *read_filter_stats);
/* "Q" with at most one fractional digit as tenths of a Phred unit, from its characters alone (never through a double): "7" -> 70,
 * "7.5" -> 75; VGMI_E_INVALID for a sign, a leading zero in front of a digit, two fractional digits, anything above 93.0 or not a number. */
int vgh_parse_quality_tenths(const char *text, uint32_t *tenths);
/* What the device path of vgh_sample_count makes of an input file, from its first bytes (no device involved): kind = "plain" |
 * "gzip" | "bgzf"; first_byte = the first byte of its text (-1: it has none); bam = block gzip whose text starts with "BAM\1";
 * fasta = the text starts with '>' and goes to the device's FASTA parser (VGH_DEVICE_FASTA=0: never).  Any pointer may be NULL. */
int vgh_sniff_input(const char *path, char kind[8], int *first_byte, int *bam, int *fasta);
void vgh_free(void *p);
/* CRC-32 (gzip polynomial) of the ingest decoder, csrc/host/fast_inflate.hpp (for tests) */
uint32_t vgh_crc32(uint32_t crc, const void *data, size_t n);

/* construct side: ConstructIndex::build_fasta_index + make_mbf (src/construct_index.cpp:85-139,150-177)
 * with the Bloom filter on the device.  seeds == NULL: the seeds BloomFilter::_init_seeds
 * (src/counting_bloom_filter.cpp:80-87) would draw if std::random_device returned
 * random_device_value.  The filter stays in ctx (vgmi_bloom_fetch / vgmi_bloom_query). */
int vgh_bloom_reference_seeds(uint32_t random_device_value, uint32_t n_hash, uint64_t *seeds_out);
int vgh_make_mbf(vgmi_ctx *ctx, const char *fasta_path, uint32_t k, const uint64_t *seeds, uint32_t n_seeds,
                 uint32_t random_device_value, uint64_t *genome_size, uint64_t *m, uint32_t *n_hash);

typedef struct vgh_sample_stats {
    uint64_t read_base;       /* FastqKmer::mReadBase */
    uint64_t n_reads;
    float read_depth;         /* ReadDepth_ (varigraph.cpp:198) */
    float hap_kmer_coverage;  /* hapKmerCoverage_ (varigraph.cpp:360-362) */
    uint8_t max_coverage;     /* get_hom_kmer_c */
    uint8_t hom_coverage;     /* after the --use-depth override, if any */
    double seconds_total, seconds_kernel;
} vgh_sample_stats;

/* One sample: counts reset -> all fastq files -> finish + coverage statistics.
 * cov_out[n_keys], cov_node_out[n_node_entries], hist_out[256] may be NULL. */
int vgh_sample_count(const vgh_graph *g, vgmi_ctx *ctx, const char *const *fastq_paths, size_t n_files,
                     uint32_t threads, uint32_t sample_ploidy, int use_depth, uint8_t *cov_out,
                     uint8_t *cov_node_out, uint64_t *hist_out, vgh_sample_stats *stats);
/* The same with a minimum base quality (0..93; 0 = off, which is vgh_sample_count): a base of a FASTQ / BAM record whose quality is
 * below it is counted as 'N' -- by the device kernels (vgmi_fastq_set_min_quality) and, by the same rule, wherever the host reader
 * serves (a tail record, the stream behind an irregular record, a pipe, VGH_HOST_PARSE=1, ...).  read_base, n_reads and the depth
 * statistics are those of the unmasked files.  *masked_bases (may be NULL) = bases masked, device and host together. */
int vgh_sample_count_q(const vgh_graph *g, vgmi_ctx *ctx, const char *const *fastq_paths, size_t n_files,
                       uint32_t threads, uint32_t sample_ploidy, int use_depth, uint8_t *cov_out,
                       uint8_t *cov_node_out, uint64_t *hist_out, vgh_sample_stats *stats, uint32_t min_base_quality,
                       uint64_t *masked_bases);
/* The same with subsampling as well (genotype --subsample F --subsample-seed S): read i of every file -- numbered per file, in file
 * order -- is kept iff the rule of vgmi_fastq_set_subsample says so, on the device and, from the device's number on, wherever the
 * host reader serves; fraction 1 is off, which is vgh_sample_count_q.  A dropped read is not a read: read_base, n_reads and the depth
 * statistics are those of the kept reads.  *reads_seen, *reads_kept (may be NULL) = the files' reads and how many were counted;
 * *masked_bases as above, of the kept reads.  VGMI_E_INVALID for a fraction that is NaN, <= 0 or > 1. */
int vgh_sample_count_s(const vgh_graph *g, vgmi_ctx *ctx, const char *const *fastq_paths, size_t n_files,
                       uint32_t threads, uint32_t sample_ploidy, int use_depth, uint8_t *cov_out,
                       uint8_t *cov_node_out, uint64_t *hist_out, vgh_sample_stats *stats, uint32_t min_base_quality,
                       double fraction, uint64_t seed, uint64_t *reads_seen, uint64_t *reads_kept, uint64_t *masked_bases);
/* The same with the read filter of BAM files (genotype --bam-exclude-flags / --bam-require-flags / --bam-min-mapq / --bam-min-tag; the
 * rule and the parameters' ranges: vgmi_fastq_set_bam_filter): applied on the device and wherever the host decoder serves -- the
 * hand-over, pipes, VGH_HOST_PARSE=1, VGH_HOST_INFLATE=1.  A dropped record is not a read: subsampling numbers the reads that
 * passed, read_base, n_reads and the depth statistics are theirs.  FASTQ and FASTA files among the paths are untouched.  The default
 * parameters (0x900, 0, 0, NULL) are vgh_sample_count_s.  *bam_records, *bam_reads (may be NULL) = the BAM files' valid records
 * and the reads among them, the two readers' counts added.  A record whose auxiliary fields cannot be walked (tag bound only) ends
 * the call with the host decoder's error, "... (auxiliary fields)".  VGMI_E_INVALID for a parameter out of range. */
int vgh_sample_count_f(const vgh_graph *g, vgmi_ctx *ctx, const char *const *fastq_paths, size_t n_files,
                       uint32_t threads, uint32_t sample_ploidy, int use_depth, uint8_t *cov_out,
                       uint8_t *cov_node_out, uint64_t *hist_out, vgh_sample_stats *stats, uint32_t min_base_quality,
                       double fraction, uint64_t seed, uint32_t bam_exclude, uint32_t bam_require, uint32_t bam_min_mapq,
                       const char *bam_tag, double bam_min_value, uint64_t *reads_seen, uint64_t *reads_kept, uint64_t *masked_bases,
                       uint64_t *bam_records, uint64_t *bam_reads);
/* The same with regions for BAM files (genotype --bam-regions / --bam-regions-file / --bam-regions-unplaced; the grammar:
 * vgh_reads_read_all_r, the rule: vgmi_fastq_set_bam_regions): resolved against every BAM file's own header, decided on the device
 * and wherever the host decoder serves.  A record outside the regions is not a read, exactly as one the filter drops.  bam_regions
 * and bam_regions_bed both NULL: vgh_sample_count_f.  *bam_records, *bam_reads are filled with regions alone too. */
int vgh_sample_count_r(const vgh_graph *g, vgmi_ctx *ctx, const char *const *fastq_paths, size_t n_files,
                       uint32_t threads, uint32_t sample_ploidy, int use_depth, uint8_t *cov_out,
                       uint8_t *cov_node_out, uint64_t *hist_out, vgh_sample_stats *stats, uint32_t min_base_quality,
                       double fraction, uint64_t seed, uint32_t bam_exclude, uint32_t bam_require, uint32_t bam_min_mapq,
                       const char *bam_tag, double bam_min_value, const char *bam_regions, const char *bam_regions_bed, int bam_unplaced,
                       uint64_t *reads_seen, uint64_t *reads_kept, uint64_t *masked_bases, uint64_t *bam_records, uint64_t *bam_reads);
/* The same with the read filter by length and read quality (genotype --min-read-length / --max-read-length / --min-read-quality /
 * --max-low-quality; the rule: vgmi_fastq_set_read_filter): every file's reads that subsampling kept are evaluated, on the device
 * and wherever the host reader serves, and a read that fails is not a read.  A FASTA file takes the length tests through the host
 * reader.  read_filter NULL or all zero: vgh_sample_count_r.  read_filter_stats (may be NULL): 5 values as vgh_reads_read_all_l,
 * summed over the files. */
int vgh_sample_count_l(const vgh_graph *g, vgmi_ctx *ctx, const char *const *fastq_paths, size_t n_files,
                       uint32_t threads, uint32_t sample_ploidy, int use_depth, uint8_t *cov_out,
                       uint8_t *cov_node_out, uint64_t *hist_out, vgh_sample_stats *stats, uint32_t min_base_quality,
                       double fraction, uint64_t seed, uint32_t bam_exclude, uint32_t bam_require, uint32_t bam_min_mapq,
                       const char *bam_tag, double bam_min_value, const char *bam_regions, const char *bam_regions_bed, int bam_unplaced,
                       const vgmi_read_filter *read_filter, uint64_t *reads_seen, uint64_t *reads_kept, uint64_t *masked_bases,
                       uint64_t *bam_records, uint64_t *bam_reads, uint64_t *read_filter_stats);

/* Coverage statistics alone (Varigraph::kmer_read / cal_ave_cov_kmer): hist = masked coverage histogram
 * (vgmi_counts_finish).  Fills read_depth, hap_kmer_coverage, max_coverage, hom_coverage of *stats; returns
 * VGMI_E_STATE where the reference exits with "Failed to retrieve depth information". */
int vgh_coverage_stats(const uint64_t hist[256], uint64_t read_base, uint64_t genome_size, uint32_t sample_ploidy,
                       int use_depth, vgh_sample_stats *stats);

/* Genotyping HMM (host; x87 long double like the reference).  The object keeps the per-node k-mer lists, which the
 * forward pass prunes and which persist across samples exactly as in the reference (reset() does not restore them):
 * create one per graph, call vgh_genotype once per sample in `-s` order. */
typedef struct vgh_genotyper vgh_genotyper;
typedef struct vgh_genotype_config {   /* defaults of include/varigraph.hpp:49-68 via vgh_genotype_config_default */
    const char *sample_type;    /* -g: "het" | "hom" */
    uint32_t sample_ploidy;     /* --sample-ploidy */
    uint32_t haploid_num;       /* -n */
    uint32_t chr_len_thread;    /* --granularity, in bp */
    const char *transition;     /* -m: "rec" | "fre" */
    int sv_only;                /* --sv */
    uint32_t threads;           /* -t */
    float min_gq;               /* --min-support */
} vgh_genotype_config;
void vgh_genotype_config_default(vgh_genotype_config *cfg);
int vgh_genotyper_create(const vgh_graph *g, vgh_genotyper **out);
void vgh_genotyper_free(vgh_genotyper *gt);
/* cov: c of every key in graph.bin record order.  *vcf_text_out (vgh_free) = decompressed content of
 * <sample>.varigraph.vcf.gz. */
int vgh_genotype(vgh_genotyper *gt, const uint8_t *cov, float hap_kmer_coverage, const char *sample_name,
                 const vgh_genotype_config *cfg, char **vcf_text_out, size_t *n_bytes_out);
/* <sample>.varigraph.vcf.gz as `varigraph-mi genotype` writes it: block gzip (BGZF) of `text`, deflated by `threads`
 * workers; the decompressed bytes are what the reference's SAVE::save writes (src/save.cpp:11-30) */
int vgh_write_vcf_gz(const char *path, const char *text, size_t n_bytes, uint32_t threads);

#ifdef __cplusplus
}
#endif
#endif
