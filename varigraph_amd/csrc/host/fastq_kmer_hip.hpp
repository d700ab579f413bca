// fastq_kmer_hip.hpp -- the MI355X twin of the reference's read-counting class.
//
// Reference seam:
//   FastqKmer(unordered_map<uint64_t,kmerCovFreBitVec>& table, const vector<string>& fastqs,
//             const uint32_t& k, const uint32_t& threads)          include/fastq_kmer.hpp:57-62
//   void build_fastq_index();  uint64_t mReadBase;                  include/fastq_kmer.hpp:42,73
//   FastqKmerKernel(..., int buffer); build_fastq_index_kernel()    include/fastq_kmer.cuh:15-36
// Post-condition kept: after build_fastq_index() every key's c == min(255, occurrences over all
// reads of all files) and mReadBase == sum of record lengths.  Here the table lives on the device
// behind a vgmi context (uploaded once per run from the graph index) instead of being borrowed as
// a host unordered_map; the counters are fetched with fetch() when the caller wants them.
//
// Pipeline: one parser thread per input file (up to `threads`), each filling read blocks
// ('\n'-joined sequences) that the calling thread hands to vgmi_reads_submit, which stages them
// through pinned memory on alternating HIP streams.  The reference parses on its main thread and
// runs files one after another (src/fastq_kmer.cpp:47-49); the result is order-independent.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../vgmi_bam_filter.h"
#include "bam_regions.hpp"
#include "../vgmi_read_filter.h"
#include "../vgmi_subsample.h"

struct vgmi_ctx;

namespace vgh {

class FastqKmerHip {
public:
    uint64_t mReadBase = 0;  // Sequencing file size (same name as the reference member)
    uint64_t mReadNum = 0;

    FastqKmerHip(vgmi_ctx* ctx, const std::vector<std::string>& fastqFileNameVec, uint32_t kmerLen,
                 uint32_t threads, size_t block_bytes = 32u << 20);

    // resets the device counters, streams every file through the device; throws std::runtime_error
    // on I/O errors, empty reads (reference: assert(len > 0)) and device errors
    void build_fastq_index();

    // c per key / per node entry / masked histogram (any may be null), see vgmi_counts_finish
    void fetch(uint8_t* cov, uint8_t* cov_node, uint64_t* hist256);

    double kernel_seconds() const { return kernel_s_; }

protected:
    // build_fastq_index with a minimum base quality (0: off); masked_bases gets the bases counted as 'N' for their quality
    void count_files(uint32_t min_base_quality, uint64_t& masked_bases);
    // ... and with a subsampling rule (off: count_files); reads_seen gets the files' reads, of which mReadNum were kept and counted
    void count_files_sampled(uint32_t min_base_quality, const SubsampleRule& sub, uint64_t& masked_bases, uint64_t& reads_seen);
    // ... and with a read filter for the BAM files (on == 0: count_files_sampled); bam_records / bam_reads get their records and the reads among them
    void count_files_filtered(uint32_t min_base_quality, const SubsampleRule& sub, const BamFilterParams& filter, uint64_t& masked_bases,
                              uint64_t& reads_seen, uint64_t& bam_records, uint64_t& bam_reads);
    // ... and with regions for the BAM files (regions.on() false: count_files_filtered); bed_skipped gets the BED lines whose reference a
    // file's header lacks, summed over the BAM files
    void count_files_regions(uint32_t min_base_quality, const SubsampleRule& sub, const BamFilterParams& filter, const BamRegionSpec& regions,
                             uint64_t& masked_bases, uint64_t& reads_seen, uint64_t& bam_records, uint64_t& bam_reads, uint64_t& bed_skipped);
    // ... and with a read filter by length and read quality for every file (read_filter.on == 0: count_files_regions); dropped gets the reads
    // it dropped: short, long, low fraction, low mean
    void count_files_read_filter(uint32_t min_base_quality, const SubsampleRule& sub, const BamFilterParams& filter, const BamRegionSpec& regions,
                                 const ReadFilterParams& read_filter, uint64_t& masked_bases, uint64_t& reads_seen, uint64_t& bam_records,
                                 uint64_t& bam_reads, uint64_t& bed_skipped, uint64_t dropped[4]);

private:
    vgmi_ctx* ctx_;
    std::vector<std::string> files_;
    uint32_t k_, threads_;
    size_t block_bytes_;
    double kernel_s_ = 0;
};

// FastqKmerHip with a minimum base quality (0..93; 0 = off): a base of a FASTQ / BAM record whose quality is below it is counted as
// 'N' (the rule of vgmi_fastq_set_min_quality, on the device and wherever the host reader serves); mReadBase and mReadNum do not
// change with it.  A class of its own: FastqKmerHip keeps its constructor and its size, so a program built against the earlier
// header -- the integration binary of integration/varigraph_hip.hpp -- runs against this library as it is.  Nothing of the base is
// hidden: the masked count has its own name, build_fastq_index_masked, and the inherited build_fastq_index stays what it is for
// every FastqKmerHip -- the count without a bound.
class FastqKmerHipQ : public FastqKmerHip {
public:
    uint64_t mMaskedBases = 0;  // bases counted as 'N' for their quality, device and host readers together

    // throws std::runtime_error for min_base_quality > 93
    FastqKmerHipQ(vgmi_ctx* ctx, const std::vector<std::string>& fastqFileNameVec, uint32_t kmerLen, uint32_t threads,
                  uint32_t min_base_quality = 0, size_t block_bytes = 32u << 20);

    // build_fastq_index with the bound applied; fills mMaskedBases
    void build_fastq_index_masked() { count_files(min_q_, mMaskedBases); }

private:
    uint32_t min_q_;
};

// FastqKmerHip with a minimum base quality and subsampling (genotype --subsample F --subsample-seed S; vgmi_subsample.h has the rule): a
// seeded fraction of every file's reads is kept, on the device and -- from the device's number on -- wherever the host reader
// serves, so a file counted partly by each gives one answer.  A dropped read is not a read: mReadBase and mReadNum are those of
// the kept reads, which is what the depth statistics take.  Fraction 1 is off and counts what FastqKmerHipQ counts.  A class of
// its own for FastqKmerHipQ's reason: FastqKmerHip keeps its constructor symbol and its size.
class FastqKmerHipS : public FastqKmerHip {
public:
    uint64_t mMaskedBases = 0;  // bases of the kept reads counted as 'N' for their quality
    uint64_t mReadsSeen = 0;    // the files' reads, kept or not (mReadNum: the kept ones)

    // throws std::runtime_error for min_base_quality > 93 and for a fraction that is NaN, <= 0 or > 1
    FastqKmerHipS(vgmi_ctx* ctx, const std::vector<std::string>& fastqFileNameVec, uint32_t kmerLen, uint32_t threads,
                  uint32_t min_base_quality, double fraction, uint64_t seed = 11, size_t block_bytes = 32u << 20);

    // build_fastq_index with the bound and the rule applied; fills mMaskedBases and mReadsSeen
    void build_fastq_index_sampled() { count_files_sampled(min_q_, rule_, mMaskedBases, mReadsSeen); }

private:
    uint32_t min_q_;
    SubsampleRule rule_;
};

// FastqKmerHipS with a read filter for BAM files (genotype --bam-exclude-flags / --bam-require-flags / --bam-min-mapq / --bam-min-tag;
// vgmi_bam_filter.h has the rule): a record the filter drops is not a read, on the device and wherever the host decoder serves;
// subsampling numbers the reads that passed.  FASTQ and FASTA files are untouched.  filter.on == 0 counts what FastqKmerHipS counts.  A
// class of its own for FastqKmerHipQ's reason.
class FastqKmerHipF : public FastqKmerHip {
public:
    uint64_t mMaskedBases = 0;  // bases of the kept reads counted as 'N' for their quality
    uint64_t mReadsSeen = 0;    // the files' reads, kept or not (mReadNum: the kept ones)
    uint64_t mBamRecords = 0;   // with a filter: the BAM files' valid records ...
    uint64_t mBamReads = 0;     // ... and the reads among them (before subsampling)

    // throws std::runtime_error for min_base_quality > 93 and for a fraction that is NaN, <= 0 or > 1; filter: bam_filter_params of valid parameters
    FastqKmerHipF(vgmi_ctx* ctx, const std::vector<std::string>& fastqFileNameVec, uint32_t kmerLen, uint32_t threads, uint32_t min_base_quality,
                  double fraction, uint64_t seed, const BamFilterParams& filter, size_t block_bytes = 32u << 20);

    void build_fastq_index_filtered() { count_files_filtered(min_q_, rule_, filt_, mMaskedBases, mReadsSeen, mBamRecords, mBamReads); }

private:
    uint32_t min_q_;
    SubsampleRule rule_;
    BamFilterParams filt_;
};

// FastqKmerHipF with regions for BAM files (genotype --bam-regions / --bam-regions-file / --bam-regions-unplaced; condition 5 of
// vgmi_bam_filter.h): resolved against every BAM file's own header, applied on the device and wherever the host decoder serves.  A
// reference of --bam-regions that a file's header lacks ends the count with that file's name.  regions.on() false counts what
// FastqKmerHipF counts.  A class of its own for FastqKmerHipQ's reason.
class FastqKmerHipR : public FastqKmerHip {
public:
    uint64_t mMaskedBases = 0;
    uint64_t mReadsSeen = 0;
    uint64_t mBamRecords = 0;   // with a filter or regions: the BAM files' valid records ...
    uint64_t mBamReads = 0;     // ... and the reads among them (before subsampling)
    uint64_t mBedSkipped = 0;   // BED lines whose reference a BAM file's header lacks

    // throws as FastqKmerHipF, and for regions.unplaced without a list or a BED file
    FastqKmerHipR(vgmi_ctx* ctx, const std::vector<std::string>& fastqFileNameVec, uint32_t kmerLen, uint32_t threads, uint32_t min_base_quality,
                  double fraction, uint64_t seed, const BamFilterParams& filter, const BamRegionSpec& regions, size_t block_bytes = 32u << 20);

    void build_fastq_index_regions()
    {
        count_files_regions(min_q_, rule_, filt_, reg_, mMaskedBases, mReadsSeen, mBamRecords, mBamReads, mBedSkipped);
    }

private:
    uint32_t min_q_;
    SubsampleRule rule_;
    BamFilterParams filt_;
    BamRegionSpec reg_;
};

// FastqKmerHipR with the read filter by length and read quality (genotype --min-read-length / --max-read-length / --min-read-quality /
// --max-low-quality; vgmi_read_filter.h has the rule): evaluated on the reads subsampling kept, on the device and wherever the host
// reader serves, on the file's own qualities.  A dropped read is not a read.  A FASTA file has no qualities: the length tests alone
// apply, through the host reader.  read_filter.on == 0 counts what FastqKmerHipR counts.  A class of its own for FastqKmerHipQ's reason.
class FastqKmerHipL : public FastqKmerHip {
public:
    uint64_t mMaskedBases = 0;
    uint64_t mReadsSeen = 0;
    uint64_t mBamRecords = 0;
    uint64_t mBamReads = 0;
    uint64_t mBedSkipped = 0;
    uint64_t mReadsDropped[4] = {0, 0, 0, 0};   // by the read filter: short, long, low fraction, low mean (evaluated = mReadNum + their sum)

    // throws as FastqKmerHipR, and for read_filter fields out of range (read_filter_invalid)
    FastqKmerHipL(vgmi_ctx* ctx, const std::vector<std::string>& fastqFileNameVec, uint32_t kmerLen, uint32_t threads, uint32_t min_base_quality,
                  double fraction, uint64_t seed, const BamFilterParams& filter, const BamRegionSpec& regions, const ReadFilterParams& read_filter,
                  size_t block_bytes = 32u << 20);

    void build_fastq_index_read_filter()
    {
        count_files_read_filter(min_q_, rule_, filt_, reg_, rf_, mMaskedBases, mReadsSeen, mBamRecords, mBamReads, mBedSkipped, mReadsDropped);
    }

private:
    uint32_t min_q_;
    SubsampleRule rule_;
    BamFilterParams filt_;
    BamRegionSpec reg_;
    ReadFilterParams rf_;
};

// What the device path makes of an input file, decided from its first bytes alone (no device involved): the container by the
// gzip magic and the 'BC' extra subfield of the first member, BAM by "BAM\1" at the start of a block-gzip file's text, FASTA by a
// text whose first byte is '>' (vgmi_fastq_open_fasta; VGH_DEVICE_FASTA=0: the FASTQ-mode parser, which hands a FASTA stream to
// the host reader at record 0).  first_byte: the text's first byte, -1 when it has none.  Throws like ByteSource::open.
struct InputSniff {
    bool plain = true, bgzf = false, bam = false, fasta = false;
    int first_byte = -1;
};
InputSniff sniff_input(const std::string& path);

// Coverage statistics that turn the counters into hapKmerCoverage_ (src/varigraph.cpp:198,220-243,
// 308-362).  Returns false where the reference exits with "Failed to retrieve depth information".
struct CoverageStats {
    float read_depth = 0, hap_kmer_coverage = 0;
    uint8_t max_coverage = 0, hom_coverage = 0;
};
bool coverage_stats(const uint64_t hist[256], uint64_t read_base, uint64_t genome_size, uint32_t sample_ploidy,
                    bool use_depth, CoverageStats& out);

}  // namespace vgh
