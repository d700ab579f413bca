// fastx_reader.hpp -- FASTA/FASTQ(.gz) record reader with the semantics of klib's kseq_read as
// the reference uses it (include/kseq.h:192-232 through FastqKmer::fastq_file_open,
// src/fastq_kmer.cpp:74-105):
//   * records start at the next '>' or '@'; the name ends at the first whitespace
//   * sequence = concatenation of the following lines up to a line starting with '>', '+' or '@'
//     (empty lines skipped, a trailing '\r' dropped per line when the sequence is longer than 1)
//   * FASTQ: the rest of the '+' line is skipped, quality lines are appended until they are at
//     least as long as the sequence; a length mismatch or a missing quality is a truncated record
//     (-2) and the reference's `while (kseq_read(ks) >= 0)` loop stops reading the file there
//   * the bytes come from a ByteSource (plain, gzip or block-gzip input, as gzopen would deliver them) whose
//     inflate runs on its own thread(s), `decode_threads` of them for block gzip
#pragma once
#include <cstdint>
#include <memory>
#include <string>

#include "byte_source.hpp"
#include "../vgmi_read_filter.h"
#include "../vgmi_subsample.h"

namespace vgh {

class FastxReader {
public:
    explicit FastxReader(const std::string& path, unsigned decode_threads = 1);  // throws std::runtime_error if it cannot open
    explicit FastxReader(std::unique_ptr<ByteSource> src);   // any byte stream, read from a record boundary on
    ~FastxReader();
    FastxReader(const FastxReader&) = delete;
    FastxReader& operator=(const FastxReader&) = delete;

    // >= 0: sequence length (seq() holds it); -1: end of file; -2: truncated quality
    long next() { return rule_.on || rf_.on() ? next_sampled() : next_record(); }      // (without a rule: the reader of before, one call)
    // Subsampling (vgmi_subsample.h): the records next() reads from here on are numbered first_number, first_number + 1, ... and the ones
    // the rule drops are passed over -- next() returns the kept ones only.  first_number is the file number of the next record: 0 at
    // the start of a file, the device's n_seen where this reader takes a stream over.  next_number(): the number the record after
    // the last one read would get (with a rule that is on: without one nothing is numbered).
    void subsample(const SubsampleRule& rule, uint64_t first_number)
    {
        rule_ = rule;
        number_ = first_number;
    }
    uint64_t next_number() const { return number_; }
    // The read filter (vgmi_read_filter.h): from here on next() applies the rule behind subsampling -- a record subsampling drops is not
    // evaluated -- on the record's own quality bytes, and returns the passing records only.  A FASTA record has no qualities: the length
    // tests alone apply.  read_filter().n_class: the evaluated records by class ([0]: passed).  A record of 2^31 bases or more under a
    // quality test throws: the rule's sums are exact below that, and such a record is a contig, not a read.
    void read_filter(const ReadFilterRule& rule) { rf_ = rule; }
    const ReadFilterRule& read_filter() const { return rf_; }
    const std::string& seq() const { return seq_; }
    const std::string& name() const { return name_; }  // up to the first whitespace of the header line
    const std::string& qual() const { return qual_; }  // the record's quality lines joined (empty for a FASTA record)
    // Minimum base quality q (the rule of vgmi_fastq_set_min_quality): base i of seq() becomes 'N' where quality byte i, as an unsigned
    // byte, is < 33 + q.  Returns the number of bases masked; a FASTA record has no qualities and stays as it is.
    uint64_t mask_below(uint32_t q);
    const char* source_kind() const { return src_->kind(); }

private:
    long next_record();   // next() without the rule
    long next_sampled();  // ... and with subsampling and / or a read filter: the next record they keep
    int getc();
    // append up to (not including) the next '\n' to s; returns false at EOF with nothing read
    bool get_line(std::string& s, bool append);

    bool refill();   // false at the end of the data
    bool skip_line();

    std::unique_ptr<ByteSource> src_;
    const unsigned char* cur_ = nullptr;
    const unsigned char* end_ = nullptr;
    bool eof_ = false;
    int last_char_ = 0;
    std::string seq_, qual_, name_;
    SubsampleRule rule_;
    uint64_t number_ = 0;
    ReadFilterRule rf_;
};

}  // namespace vgh
