// bam_reader.hpp -- the reads of a BAM / unaligned BAM file (SAM spec 4.2) over a ByteSource: the host decoder of the BAM stream
// (vgmi_fastq_open_bam).  It takes the stream where the device cannot (a record it stops at, a damaged member, a pipe), it is the
// reader of the host-parse path (even k), and it is the yardstick of the device kernels (vgmi_bam.hip).
//   reads     records with flag & 0x900 == 0 (no secondary, no supplementary alignment) and l_seq > 0 -- what `samtools fastq`
//             writes by default; QC-fail, duplicate and unmapped records are reads too.  filter() configures the rule.
//   sequence  the 4-bit SEQ field through "=ACMGRSVTWYHKDBN", as stored (no reverse complement: the k-mers are canonical)
// A record that is not valid throws "'<path>': not a valid BAM record at decompressed byte N (<what>)", N = its first byte.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "bam_regions.hpp"
#include "byte_source.hpp"
#include "../vgmi_bam_filter.h"
#include "../vgmi_read_filter.h"
#include "../vgmi_subsample.h"

namespace vgh {

class BamReader {
public:
    // reads and checks the header; keep_refs: the references' names and lengths are kept (ref_names(), ref_lengths()) -- only where
    // regions are resolved against them, a header may hold millions of contigs
    BamReader(std::unique_ptr<ByteSource> src, const std::string& path, bool keep_refs = false);
    const std::vector<std::string>& ref_names() const { return ref_names_; }
    const std::vector<uint32_t>& ref_lengths() const { return ref_lengths_; }
    const std::string& path() const { return path_; }
    uint64_t header_bytes() const { return header_bytes_; }   // magic .. the last reference, in decompressed bytes
    int32_t n_ref() const { return n_ref_; }
    // passes over the stream up to decompressed byte `offset` (a record boundary at or behind the current position)
    void skip_to(uint64_t offset);

    // >= 0: sequence length (seq() holds it); -1: end of the data
    long next();
    // Subsampling (vgmi_subsample.h): the reads -- the records that pass the filter above; the others have no number -- that next() comes
    // to from here on are numbered first_number, first_number + 1, ... and the ones the rule drops are passed over undecoded.
    // first_number: 0 at the start of a file, the device's n_seen where this reader takes a stream over.
    void subsample(const SubsampleRule& rule, uint64_t first_number)
    {
        rule_ = rule;
        number_ = first_number;
    }
    uint64_t next_number() const { return number_; }
    // The read filter (vgmi_bam_filter.h; on == 0: the default above): from here on next() applies the configured rule in the default's
    // place, in front of subsampling.  A record whose auxiliary fields cannot be walked throws as the invalid record it is, "(auxiliary
    // fields)".  records() / reads(): valid records examined since, and the reads among them (before subsampling).
    void filter(const BamFilterParams& f) { filt_ = f; }
    // The region list (condition 5 of vgmi_bam_filter.h), normalised -- bam_regions_normalise, or resolve_bam_regions below; empty: no
    // region test.  It combines with filter().
    void regions(std::vector<BamInterval> list, bool unplaced)
    {
        regions_ = std::move(list);
        unplaced_ = unplaced && !regions_.empty();
    }
    // The read filter by length and read quality (vgmi_read_filter.h): applied behind subsampling on the record's QUAL bytes as stored (a
    // record whose QUAL[0] is 0xff passes both quality tests); a read it drops is passed over undecoded.  read_filter().n_class: the
    // evaluated reads by class ([0]: passed).
    void read_filter(const ReadFilterRule& rule) { rf_ = rule; }
    const ReadFilterRule& read_filter() const { return rf_; }
    uint64_t records() const { return records_; }
    uint64_t reads() const { return reads_; }
    const std::string& seq() const { return seq_; }
    const std::string& qual() const { return qual_; }   // the record's QUAL bytes as stored (l_seq of them; QUAL[0] == 0xff: none stored)
    // Minimum base quality q (the rule of vgmi_fastq_set_min_quality): base i of seq() becomes 'N' where QUAL[i] < q, in record order;
    // a record whose QUAL[0] is 0xff is not masked.  Returns the number of bases masked.
    uint64_t mask_below(uint32_t q);

private:
    bool fill(size_t n);   // at least n bytes buffered; false if the data ends first
    [[noreturn]] void bad(uint64_t at, const char* what) const;

    std::unique_ptr<ByteSource> src_;
    std::string path_;
    std::vector<unsigned char> buf_;
    size_t pos_ = 0;        // buf_[pos_] is decompressed byte off_
    uint64_t off_ = 0;
    uint64_t header_bytes_ = 0;
    int32_t n_ref_ = 0;
    std::string seq_, qual_;
    SubsampleRule rule_;
    uint64_t number_ = 0;
    BamFilterParams filt_ = bam_filter_params();
    uint64_t records_ = 0, reads_ = 0;
    std::vector<std::string> ref_names_;
    std::vector<uint32_t> ref_lengths_;
    std::vector<BamInterval> regions_;
    bool unplaced_ = false;
    ReadFilterRule rf_;
};

// the bytes of `path` as ByteSource::open delivers them; is_bam: block gzip whose text starts with "BAM\1" (decided from content)
std::unique_ptr<ByteSource> open_sniffed(const std::string& path, unsigned decode_threads, bool& is_bam);

}  // namespace vgh
