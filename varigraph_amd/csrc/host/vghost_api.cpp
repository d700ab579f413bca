// vghost_api.cpp -- C API of include/vghost.h over the C++ host classes
#include "vghost.h"

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>

#include "bam_reader.hpp"
#include "fastq_kmer_hip.hpp"
#include "fast_inflate.hpp"
#include "fastx_reader.hpp"
#include "genotyper.hpp"
#include "graph_index.hpp"
#include "make_mbf.hpp"

struct vgh_graph {
    vgh::GraphIndex g;
};
struct vgh_genotyper {
    vgh::Genotyper gt;
    explicit vgh_genotyper(const vgh::GraphIndex& g) : gt(g) {}
};

static thread_local std::string g_err;

namespace {
// every record of `rd` (FastxReader or BamReader) as a '\n'-joined block in malloc'ed memory, bases below quality q masked (0: none);
// the number of reads, or VGMI_E_NOMEM.  A sequence ends at its first NUL, read_base counts it whole (src/fastq_kmer.cpp:101 vs :105).
template <class Reader>
int64_t reads_block(Reader& rd, uint32_t q, char** block_out, size_t* n_bytes_out, uint64_t* read_base, uint64_t* masked_bases,
                    const vgh::SubsampleRule* sub = nullptr, uint64_t first_number = 0, uint64_t* next_number = nullptr,
                    const vgh::ReadFilterParams* rf = nullptr, uint64_t* rf_stats = nullptr)
{
    if (sub) rd.subsample(*sub, first_number);
    if (rf && rf->on) rd.read_filter(vgh::ReadFilterRule(*rf));
    std::string block;
    int64_t n = 0;
    uint64_t rb = 0, masked = 0;
    while (rd.next() >= 0) {
        if (q) masked += rd.mask_below(q);
        const std::string& s = rd.seq();
        block.append(s.data(), strnlen(s.data(), s.size()));
        block.push_back('\n');
        rb += s.size();
        ++n;
    }
    char* p = static_cast<char*>(malloc(block.size() ? block.size() : 1));
    if (!p) return VGMI_E_NOMEM;
    memcpy(p, block.data(), block.size());
    *block_out = p;
    *n_bytes_out = block.size();
    if (read_base) *read_base = rb;
    if (masked_bases) *masked_bases = masked;
    if (next_number) *next_number = sub && sub->on ? rd.next_number() : first_number + (uint64_t)n;      // (off: every read is kept, nothing numbers them)
    if (rf && rf->on && !(sub && sub->on) && next_number) *next_number = first_number + rd.read_filter().evaluated();
    if (rf_stats) {
        const vgh::ReadFilterRule& r = rd.read_filter();
        rf_stats[0] = rf && rf->on ? r.evaluated() : (uint64_t)n;
        for (int c = 1; c < 5; ++c) rf_stats[c] = r.n_class[c];
    }
    return n;
}
}  // namespace

extern "C" {

const char* vgh_last_error(void) { return g_err.c_str(); }

int vgh_graph_load(const char* path, vgh_graph** out)
{
    if (!path || !out) return VGMI_E_INVALID;
    *out = nullptr;
    try {
        auto* h = new vgh_graph();
        try {
            h->g.load(path);
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
        return VGMI_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

void vgh_graph_free(vgh_graph* g) { delete g; }

int vgh_reads_index_save(const vgh_graph* h, const uint8_t* cov, uint64_t read_base, const char* path)
{
    if (!h || !cov || !path) return VGMI_E_INVALID;
    try {
        h->g.save_reads_index(path, cov, read_base);
        return VGMI_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

int vgh_reads_index_load(const vgh_graph* h, const char* path, uint8_t* cov, uint64_t* read_base)
{
    if (!h || !cov || !path || !read_base) return VGMI_E_INVALID;
    try {
        h->g.load_reads_index(path, cov, *read_base);
        return VGMI_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

int vgh_graph_get_info(const vgh_graph* h, vgh_graph_info* info)
{
    if (!h || !info) return VGMI_E_INVALID;
    const vgh::GraphIndex& g = h->g;
    info->graph_base_num = g.graph_base_num;
    info->genome_size = g.genome_size;
    info->n_keys = g.keys.size();
    info->bitlen = g.bitlen;
    info->n_variant_nodes = g.node_off.size() - 1;
    info->n_node_entries = g.node_key_index.size();
    info->k = g.k;
    info->vcf_ploidy = g.vcf_ploidy;
    info->hap_num = g.hap_num;
    info->n_chromosomes = (uint32_t)g.chr_names.size();
    return VGMI_OK;
}

const uint64_t* vgh_graph_keys(const vgh_graph* h) { return h->g.keys.data(); }
const uint8_t* vgh_graph_f(const vgh_graph* h) { return h->g.f.data(); }
const int8_t* vgh_graph_bitvec(const vgh_graph* h) { return h->g.bitvec.data(); }
const uint8_t* vgh_graph_hom_flag(const vgh_graph* h) { return h->g.hom_flag.data(); }
const uint64_t* vgh_graph_node_off(const vgh_graph* h) { return h->g.node_off.data(); }
const uint32_t* vgh_graph_node_key_index(const vgh_graph* h) { return h->g.node_key_index.data(); }
const uint32_t* vgh_graph_node_start(const vgh_graph* h) { return h->g.node_start.data(); }
const uint32_t* vgh_graph_node_chr(const vgh_graph* h) { return h->g.node_chr.data(); }
const char* vgh_graph_chr_name(const vgh_graph* h, uint32_t chr)
{
    return chr < h->g.chr_names.size() ? h->g.chr_names[chr].c_str() : nullptr;
}

int vgh_graph_upload(const vgh_graph* h, vgmi_ctx* ctx)
{
    if (!h || !ctx) return VGMI_E_INVALID;
    int rc = h->g.upload(ctx);
    if (rc) g_err = vgmi_last_error(ctx);
    return rc;
}

int64_t vgh_fastx_read_all_mt(const char* path, uint32_t decode_threads, char** block_out, size_t* n_bytes_out,
                              uint64_t* read_base, char source_kind[8])
{
    if (!path || !block_out || !n_bytes_out) return VGMI_E_INVALID;
    try {
        vgh::FastxReader rd(path, decode_threads ? decode_threads : 1);
        if (source_kind) {
            strncpy(source_kind, rd.source_kind(), 7);
            source_kind[7] = 0;
        }
        return reads_block(rd, 0, block_out, n_bytes_out, read_base, nullptr);
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

int64_t vgh_bam_read_all(const char* path, uint32_t decode_threads, char** block_out, size_t* n_bytes_out, uint64_t* read_base)
{
    if (!path || !block_out || !n_bytes_out) return VGMI_E_INVALID;
    try {
        bool is_bam = false;
        std::unique_ptr<vgh::ByteSource> src = vgh::open_sniffed(path, decode_threads ? decode_threads : 1, is_bam);
        if (!is_bam) throw std::runtime_error(std::string("'") + path + "': not a BAM file (block gzip starting with BAM\\1)");
        vgh::BamReader rd(std::move(src), path);
        return reads_block(rd, 0, block_out, n_bytes_out, read_base, nullptr);
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

int64_t vgh_reads_read_all_q(const char* path, uint32_t decode_threads, uint32_t min_base_quality, char** block_out, size_t* n_bytes_out,
                             uint64_t* read_base, uint64_t* masked_bases)
{
    if (!path || !block_out || !n_bytes_out) return VGMI_E_INVALID;
    if (min_base_quality > 93) {
        g_err = "minimum base quality " + std::to_string(min_base_quality) + " is out of range (0..93, Phred+33)";
        return VGMI_E_INVALID;
    }
    try {
        bool is_bam = false;
        std::unique_ptr<vgh::ByteSource> src = vgh::open_sniffed(path, decode_threads ? decode_threads : 1, is_bam);
        if (is_bam) {
            vgh::BamReader rd(std::move(src), path);
            return reads_block(rd, min_base_quality, block_out, n_bytes_out, read_base, masked_bases);
        }
        vgh::FastxReader rd(std::move(src));
        return reads_block(rd, min_base_quality, block_out, n_bytes_out, read_base, masked_bases);
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

int64_t vgh_reads_read_all_s(const char* path, uint32_t decode_threads, uint32_t min_base_quality, double fraction, uint64_t seed,
                             uint64_t first_number, char** block_out, size_t* n_bytes_out, uint64_t* read_base, uint64_t* masked_bases,
                             uint64_t* next_number)
{
    if (!path || !block_out || !n_bytes_out) return VGMI_E_INVALID;
    if (min_base_quality > 93) {
        g_err = "minimum base quality " + std::to_string(min_base_quality) + " is out of range (0..93, Phred+33)";
        return VGMI_E_INVALID;
    }
    if (!vgh::subsample_fraction_valid(fraction)) {
        g_err = "subsampling fraction " + std::to_string(fraction) + " is out of range (0 < fraction <= 1)";
        return VGMI_E_INVALID;
    }
    try {
        const vgh::SubsampleRule rule(fraction, seed);
        bool is_bam = false;
        std::unique_ptr<vgh::ByteSource> src = vgh::open_sniffed(path, decode_threads ? decode_threads : 1, is_bam);
        if (is_bam) {
            vgh::BamReader rd(std::move(src), path);
            return reads_block(rd, min_base_quality, block_out, n_bytes_out, read_base, masked_bases, &rule, first_number, next_number);
        }
        vgh::FastxReader rd(std::move(src));
        return reads_block(rd, min_base_quality, block_out, n_bytes_out, read_base, masked_bases, &rule, first_number, next_number);
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

int64_t vgh_reads_read_all_f(const char* path, uint32_t decode_threads, uint32_t min_base_quality, double fraction, uint64_t seed,
                             uint64_t first_number, uint32_t bam_exclude, uint32_t bam_require, uint32_t bam_min_mapq, const char* bam_tag,
                             double bam_min_value, char** block_out, size_t* n_bytes_out, uint64_t* read_base, uint64_t* masked_bases,
                             uint64_t* next_number, uint64_t* bam_records, uint64_t* bam_reads)
{
    return vgh_reads_read_all_r(path, decode_threads, min_base_quality, fraction, seed, first_number, bam_exclude, bam_require, bam_min_mapq, bam_tag,
                                bam_min_value, nullptr, nullptr, 0, block_out, n_bytes_out, read_base, masked_bases, next_number, bam_records,
                                bam_reads);
}

int64_t vgh_reads_read_all_r(const char* path, uint32_t decode_threads, uint32_t min_base_quality, double fraction, uint64_t seed,
                             uint64_t first_number, uint32_t bam_exclude, uint32_t bam_require, uint32_t bam_min_mapq, const char* bam_tag,
                             double bam_min_value, const char* bam_regions, const char* bam_regions_bed, int bam_unplaced, char** block_out,
                             size_t* n_bytes_out, uint64_t* read_base, uint64_t* masked_bases, uint64_t* next_number, uint64_t* bam_records,
                             uint64_t* bam_reads)
{
    return vgh_reads_read_all_l(path, decode_threads, min_base_quality, fraction, seed, first_number, bam_exclude, bam_require, bam_min_mapq, bam_tag,
                                bam_min_value, bam_regions, bam_regions_bed, bam_unplaced, nullptr, block_out, n_bytes_out, read_base, masked_bases,
                                next_number, bam_records, bam_reads, nullptr);
}

int vgh_parse_quality_tenths(const char* text, uint32_t* tenths)
{
    if (!tenths) return VGMI_E_INVALID;
    if (!vgh::read_filter_parse_tenths(text, tenths)) {
        g_err = std::string("'") + (text ? text : "") + "' is not a quality of 0 to 93 with at most one fractional digit";
        return VGMI_E_INVALID;
    }
    return VGMI_OK;
}

int64_t vgh_reads_read_all_l(const char* path, uint32_t decode_threads, uint32_t min_base_quality, double fraction, uint64_t seed,
                             uint64_t first_number, uint32_t bam_exclude, uint32_t bam_require, uint32_t bam_min_mapq, const char* bam_tag,
                             double bam_min_value, const char* bam_regions, const char* bam_regions_bed, int bam_unplaced,
                             const vgmi_read_filter* read_filter, char** block_out, size_t* n_bytes_out, uint64_t* read_base,
                             uint64_t* masked_bases, uint64_t* next_number, uint64_t* bam_records, uint64_t* bam_reads, uint64_t* read_filter_stats)
{
    if (!path || !block_out || !n_bytes_out) return VGMI_E_INVALID;
    if (read_filter_stats) memset(read_filter_stats, 0, 5 * sizeof(uint64_t));
    vgh::ReadFilterParams rf = vgh::read_filter_params();
    if (read_filter) {
        if (const int bad = vgh::read_filter_invalid(read_filter->min_len, read_filter->max_len, read_filter->min_mean_q, read_filter->lowq_below,
                                                     read_filter->lowq_max_pct)) {
            g_err = vgh::read_filter_invalid_text(bad);
            return VGMI_E_INVALID;
        }
        rf = vgh::read_filter_params(read_filter->min_len, read_filter->max_len, read_filter->min_mean_q, read_filter->lowq_below, read_filter->lowq_max_pct);
    }
    if (bam_records) *bam_records = 0;
    if (bam_reads) *bam_reads = 0;
    if (min_base_quality > 93) {
        g_err = "minimum base quality " + std::to_string(min_base_quality) + " is out of range (0..93, Phred+33)";
        return VGMI_E_INVALID;
    }
    if (!vgh::subsample_fraction_valid(fraction)) {
        g_err = "subsampling fraction " + std::to_string(fraction) + " is out of range (0 < fraction <= 1)";
        return VGMI_E_INVALID;
    }
    if (const int bad = vgh::bam_filter_invalid(bam_exclude, bam_require, bam_min_mapq, bam_tag, bam_min_value)) {
        g_err = vgh::bam_filter_invalid_text(bad);
        return VGMI_E_INVALID;
    }
    vgh::BamRegionSpec reg;
    reg.list = bam_regions ? bam_regions : "";
    reg.bed = bam_regions_bed ? bam_regions_bed : "";
    reg.unplaced = bam_unplaced != 0;
    if (reg.unplaced && !reg.on()) {
        g_err = vgh::bam_regions_invalid_text(4);
        return VGMI_E_INVALID;
    }
    try {
        const vgh::SubsampleRule rule(fraction, seed);
        bool is_bam = false;
        std::unique_ptr<vgh::ByteSource> src = vgh::open_sniffed(path, decode_threads ? decode_threads : 1, is_bam);
        if (is_bam) {
            vgh::BamReader rd(std::move(src), path, reg.on());
            rd.filter(vgh::bam_filter_params(bam_exclude, bam_require, bam_min_mapq, bam_tag, bam_min_value));
            if (reg.on()) rd.regions(vgh::resolve_bam_regions(reg, rd.ref_names(), path), reg.unplaced);
            const int64_t n = reads_block(rd, min_base_quality, block_out, n_bytes_out, read_base, masked_bases, &rule, first_number, next_number, &rf,
                                          read_filter_stats);
            if (bam_records) *bam_records = rd.records();
            if (bam_reads) *bam_reads = rd.reads();
            return n;
        }
        vgh::FastxReader rd(std::move(src));
        return reads_block(rd, min_base_quality, block_out, n_bytes_out, read_base, masked_bases, &rule, first_number, next_number, &rf, read_filter_stats);
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

int vgh_sniff_input(const char* path, char kind[8], int* first_byte, int* bam, int* fasta)
{
    if (!path) return VGMI_E_INVALID;
    try {
        const vgh::InputSniff r = vgh::sniff_input(path);
        if (kind) {
            memset(kind, 0, 8);
            strncpy(kind, r.plain ? "plain" : r.bgzf ? "bgzf" : "gzip", 7);
        }
        if (first_byte) *first_byte = r.first_byte;
        if (bam) *bam = r.bam;
        if (fasta) *fasta = r.fasta;
        return VGMI_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

int64_t vgh_fastx_read_all(const char* path, char** block_out, size_t* n_bytes_out, uint64_t* read_base)
{
    return vgh_fastx_read_all_mt(path, 1, block_out, n_bytes_out, read_base, nullptr);
}

int vgh_write_vcf_gz(const char* path, const char* text, size_t n_bytes, uint32_t threads)
{
    if (!path || (!text && n_bytes)) return VGMI_E_INVALID;
    try {
        vgh::Genotyper::write_gz(path, std::string(text ? text : "", n_bytes), threads);
        return VGMI_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

void vgh_free(void* p) { free(p); }

uint32_t vgh_crc32(uint32_t crc, const void* data, size_t n) { return vgh::crc32_fast(crc, static_cast<const unsigned char*>(data), n); }

int vgh_bloom_reference_seeds(uint32_t random_device_value, uint32_t n_hash, uint64_t* seeds_out)
{
    if (!seeds_out) return VGMI_E_INVALID;
    const auto s = vgh::reference_bloom_seeds(random_device_value, n_hash);
    memcpy(seeds_out, s.data(), s.size() * 8);
    return VGMI_OK;
}

int vgh_make_mbf(vgmi_ctx* ctx, const char* fasta_path, uint32_t k, const uint64_t* seeds, uint32_t n_seeds,
                 uint32_t random_device_value, uint64_t* genome_size, uint64_t* m, uint32_t* n_hash)
{
    if (!ctx || !fasta_path) return VGMI_E_INVALID;
    try {
        std::vector<uint64_t> sv(seeds, seeds + (seeds ? n_seeds : 0));
        const vgh::MbfResult r = vgh::make_mbf(ctx, fasta_path, k, sv, random_device_value);
        if (genome_size) *genome_size = r.genome_size;
        if (m) *m = r.m;
        if (n_hash) *n_hash = r.n_hash;
        return VGMI_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

int vgh_sample_count(const vgh_graph* h, vgmi_ctx* ctx, const char* const* fastq_paths, size_t n_files, uint32_t threads,
                     uint32_t sample_ploidy, int use_depth, uint8_t* cov_out, uint8_t* cov_node_out, uint64_t* hist_out,
                     vgh_sample_stats* stats)
{
    return vgh_sample_count_q(h, ctx, fastq_paths, n_files, threads, sample_ploidy, use_depth, cov_out, cov_node_out, hist_out, stats, 0, nullptr);
}

int vgh_sample_count_q(const vgh_graph* h, vgmi_ctx* ctx, const char* const* fastq_paths, size_t n_files, uint32_t threads,
                       uint32_t sample_ploidy, int use_depth, uint8_t* cov_out, uint8_t* cov_node_out, uint64_t* hist_out,
                       vgh_sample_stats* stats, uint32_t min_base_quality, uint64_t* masked_bases)
{
    return vgh_sample_count_s(h, ctx, fastq_paths, n_files, threads, sample_ploidy, use_depth, cov_out, cov_node_out, hist_out, stats,
                              min_base_quality, 1.0, 0, nullptr, nullptr, masked_bases);
}

int vgh_sample_count_s(const vgh_graph* h, vgmi_ctx* ctx, const char* const* fastq_paths, size_t n_files, uint32_t threads,
                       uint32_t sample_ploidy, int use_depth, uint8_t* cov_out, uint8_t* cov_node_out, uint64_t* hist_out,
                       vgh_sample_stats* stats, uint32_t min_base_quality, double fraction, uint64_t seed, uint64_t* reads_seen,
                       uint64_t* reads_kept, uint64_t* masked_bases)
{
    return vgh_sample_count_f(h, ctx, fastq_paths, n_files, threads, sample_ploidy, use_depth, cov_out, cov_node_out, hist_out, stats,
                              min_base_quality, fraction, seed, 0x900u, 0, 0, nullptr, 0.0, reads_seen, reads_kept, masked_bases, nullptr, nullptr);
}

int vgh_sample_count_f(const vgh_graph* h, vgmi_ctx* ctx, const char* const* fastq_paths, size_t n_files, uint32_t threads,
                       uint32_t sample_ploidy, int use_depth, uint8_t* cov_out, uint8_t* cov_node_out, uint64_t* hist_out,
                       vgh_sample_stats* stats, uint32_t min_base_quality, double fraction, uint64_t seed, uint32_t bam_exclude,
                       uint32_t bam_require, uint32_t bam_min_mapq, const char* bam_tag, double bam_min_value, uint64_t* reads_seen,
                       uint64_t* reads_kept, uint64_t* masked_bases, uint64_t* bam_records, uint64_t* bam_reads)
{
    return vgh_sample_count_r(h, ctx, fastq_paths, n_files, threads, sample_ploidy, use_depth, cov_out, cov_node_out, hist_out, stats,
                              min_base_quality, fraction, seed, bam_exclude, bam_require, bam_min_mapq, bam_tag, bam_min_value, nullptr, nullptr, 0,
                              reads_seen, reads_kept, masked_bases, bam_records, bam_reads);
}

int vgh_sample_count_r(const vgh_graph* h, vgmi_ctx* ctx, const char* const* fastq_paths, size_t n_files, uint32_t threads,
                       uint32_t sample_ploidy, int use_depth, uint8_t* cov_out, uint8_t* cov_node_out, uint64_t* hist_out,
                       vgh_sample_stats* stats, uint32_t min_base_quality, double fraction, uint64_t seed, uint32_t bam_exclude,
                       uint32_t bam_require, uint32_t bam_min_mapq, const char* bam_tag, double bam_min_value, const char* bam_regions,
                       const char* bam_regions_bed, int bam_unplaced, uint64_t* reads_seen, uint64_t* reads_kept, uint64_t* masked_bases,
                       uint64_t* bam_records, uint64_t* bam_reads)
{
    return vgh_sample_count_l(h, ctx, fastq_paths, n_files, threads, sample_ploidy, use_depth, cov_out, cov_node_out, hist_out, stats,
                              min_base_quality, fraction, seed, bam_exclude, bam_require, bam_min_mapq, bam_tag, bam_min_value, bam_regions,
                              bam_regions_bed, bam_unplaced, nullptr, reads_seen, reads_kept, masked_bases, bam_records, bam_reads, nullptr);
}

int vgh_sample_count_l(const vgh_graph* h, vgmi_ctx* ctx, const char* const* fastq_paths, size_t n_files, uint32_t threads,
                       uint32_t sample_ploidy, int use_depth, uint8_t* cov_out, uint8_t* cov_node_out, uint64_t* hist_out,
                       vgh_sample_stats* stats, uint32_t min_base_quality, double fraction, uint64_t seed, uint32_t bam_exclude,
                       uint32_t bam_require, uint32_t bam_min_mapq, const char* bam_tag, double bam_min_value, const char* bam_regions,
                       const char* bam_regions_bed, int bam_unplaced, const vgmi_read_filter* read_filter, uint64_t* reads_seen,
                       uint64_t* reads_kept, uint64_t* masked_bases, uint64_t* bam_records, uint64_t* bam_reads, uint64_t* read_filter_stats)
{
    if (!h || !ctx || (!fastq_paths && n_files)) return VGMI_E_INVALID;
    if (read_filter_stats) memset(read_filter_stats, 0, 5 * sizeof(uint64_t));
    vgh::ReadFilterParams rf = vgh::read_filter_params();
    if (read_filter) {
        if (const int bad = vgh::read_filter_invalid(read_filter->min_len, read_filter->max_len, read_filter->min_mean_q, read_filter->lowq_below,
                                                     read_filter->lowq_max_pct)) {
            g_err = vgh::read_filter_invalid_text(bad);
            return VGMI_E_INVALID;
        }
        rf = vgh::read_filter_params(read_filter->min_len, read_filter->max_len, read_filter->min_mean_q, read_filter->lowq_below, read_filter->lowq_max_pct);
    }
    if (masked_bases) *masked_bases = 0;
    if (reads_seen) *reads_seen = 0;
    if (reads_kept) *reads_kept = 0;
    if (bam_records) *bam_records = 0;
    if (bam_reads) *bam_reads = 0;
    if (const int bad = vgh::bam_filter_invalid(bam_exclude, bam_require, bam_min_mapq, bam_tag, bam_min_value)) {
        g_err = vgh::bam_filter_invalid_text(bad);
        return VGMI_E_INVALID;
    }
    try {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<std::string> files(fastq_paths, fastq_paths + n_files);
        vgh::BamRegionSpec reg;
        reg.list = bam_regions ? bam_regions : "";
        reg.bed = bam_regions_bed ? bam_regions_bed : "";
        reg.unplaced = bam_unplaced != 0;
        vgh::FastqKmerHipL fk(ctx, files, h->g.k, threads, min_base_quality, fraction, seed,
                              vgh::bam_filter_params(bam_exclude, bam_require, bam_min_mapq, bam_tag, bam_min_value), reg, rf);
        fk.build_fastq_index_read_filter();
        if (read_filter_stats) {
            read_filter_stats[0] = fk.mReadNum;
            for (int c = 0; c < 4; ++c) read_filter_stats[0] += fk.mReadsDropped[c], read_filter_stats[c + 1] = fk.mReadsDropped[c];
        }
        if (masked_bases) *masked_bases = fk.mMaskedBases;
        if (reads_seen) *reads_seen = fk.mReadsSeen;
        if (reads_kept) *reads_kept = fk.mReadNum;
        if (bam_records) *bam_records = fk.mBamRecords;
        if (bam_reads) *bam_reads = fk.mBamReads;
        uint64_t hist[256];
        fk.fetch(cov_out, cov_node_out, hist);
        if (hist_out) memcpy(hist_out, hist, sizeof hist);
        if (stats) {
            memset(stats, 0, sizeof *stats);
            stats->read_base = fk.mReadBase;
            stats->n_reads = fk.mReadNum;
            vgh::CoverageStats cs;
            const bool ok = vgh::coverage_stats(hist, fk.mReadBase, h->g.genome_size, sample_ploidy, use_depth != 0, cs);
            stats->read_depth = cs.read_depth;
            stats->hap_kmer_coverage = cs.hap_kmer_coverage;
            stats->max_coverage = cs.max_coverage;
            stats->hom_coverage = cs.hom_coverage;
            stats->seconds_kernel = fk.kernel_seconds();
            stats->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (!ok) {
                g_err = "Failed to retrieve depth information of k-mers from the sequencing data. Please verify your data.";
                return VGMI_E_STATE;
            }
        }
        return VGMI_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        const std::string m = e.what();
        return m.find("empty read") != std::string::npos || m.find("zero-length") != std::string::npos ? VGMI_E_EMPTY_READ
                                                                                                       : VGMI_E_INVALID;
    }
}

int vgh_coverage_stats(const uint64_t hist[256], uint64_t read_base, uint64_t genome_size, uint32_t sample_ploidy,
                       int use_depth, vgh_sample_stats* stats)
{
    if (!hist || !stats) return VGMI_E_INVALID;
    vgh::CoverageStats cs;
    const bool ok = vgh::coverage_stats(hist, read_base, genome_size, sample_ploidy, use_depth != 0, cs);
    stats->read_base = read_base;
    stats->read_depth = cs.read_depth;
    stats->hap_kmer_coverage = cs.hap_kmer_coverage;
    stats->max_coverage = cs.max_coverage;
    stats->hom_coverage = cs.hom_coverage;
    if (!ok) {
        g_err = "Failed to retrieve depth information of k-mers from the sequencing data. Please verify your data.";
        return VGMI_E_STATE;
    }
    return VGMI_OK;
}

void vgh_genotype_config_default(vgh_genotype_config* cfg)
{
    if (!cfg) return;
    const vgh::GenotypeConfig d;
    cfg->sample_type = "het";
    cfg->sample_ploidy = d.sample_ploidy;
    cfg->haploid_num = d.haploid_num;
    cfg->chr_len_thread = d.chr_len_thread;
    cfg->transition = "rec";
    cfg->sv_only = d.sv_only;
    cfg->threads = d.threads;
    cfg->min_gq = d.min_gq;
}

int vgh_genotyper_create(const vgh_graph* g, vgh_genotyper** out)
{
    if (!g || !out) return VGMI_E_INVALID;
    *out = nullptr;
    try {
        *out = new vgh_genotyper(g->g);
        return VGMI_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

void vgh_genotyper_free(vgh_genotyper* gt) { delete gt; }

int vgh_genotype(vgh_genotyper* gt, const uint8_t* cov, float hap_kmer_coverage, const char* sample_name,
                 const vgh_genotype_config* cfg, char** vcf_text_out, size_t* n_bytes_out)
{
    if (!gt || !cov || !sample_name || !cfg || !vcf_text_out || !n_bytes_out) return VGMI_E_INVALID;
    try {
        vgh::GenotypeConfig c;
        if (cfg->sample_type) c.sample_type = cfg->sample_type;
        c.sample_ploidy = cfg->sample_ploidy;
        c.haploid_num = cfg->haploid_num;
        c.chr_len_thread = cfg->chr_len_thread;
        if (cfg->transition) c.transition = cfg->transition;
        c.sv_only = cfg->sv_only != 0;
        c.threads = cfg->threads ? cfg->threads : 1;
        c.min_gq = cfg->min_gq;
        const std::string text = gt->gt.run(cov, hap_kmer_coverage, sample_name, c);
        char* buf = static_cast<char*>(malloc(text.size() + 1));
        if (!buf) return VGMI_E_NOMEM;
        memcpy(buf, text.data(), text.size());
        buf[text.size()] = 0;
        *vcf_text_out = buf;
        *n_bytes_out = text.size();
        return VGMI_OK;
    } catch (const std::exception& e) {
        g_err = e.what();
        return VGMI_E_INVALID;
    }
}

}  // extern "C"
