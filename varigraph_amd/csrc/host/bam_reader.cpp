#include "bam_reader.hpp"

#include <cstring>
#include <fstream>
#include <stdexcept>
#include <unordered_map>

namespace vgh {

namespace {
uint32_t le32(const unsigned char* p) { return p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// a record's bytes for bam_filter_verdict: offsets from its block_size field
struct RecordBytes {
    const unsigned char* r;
    uint32_t u8(size_t p) const { return r[p]; }
    uint32_t u32(size_t p) const { return le32(r + p); }
    size_t find_nul(size_t p, size_t end) const
    {
        const void* z = memchr(r + p, 0, end - p);
        return z ? (size_t)(static_cast<const unsigned char*>(z) - r) : end;
    }
};

// bytes already taken from a source, then the rest of it
class PrefixSource final : public ByteSource {
public:
    PrefixSource(std::vector<unsigned char> head, std::unique_ptr<ByteSource> rest) : head_(std::move(head)), rest_(std::move(rest)) {}
    bool next_chunk(const unsigned char*& p, size_t& n) override
    {
        if (!head_done_) {
            head_done_ = true;
            if (!head_.empty()) {
                p = head_.data();
                n = head_.size();
                return true;
            }
        }
        return rest_->next_chunk(p, n);
    }
    const char* kind() const override { return rest_->kind(); }

private:
    std::vector<unsigned char> head_;
    bool head_done_ = false;
    std::unique_ptr<ByteSource> rest_;
};
}  // namespace

std::unique_ptr<ByteSource> open_sniffed(const std::string& path, unsigned decode_threads, bool& is_bam)
{
    is_bam = false;
    std::unique_ptr<ByteSource> src = ByteSource::open(path, decode_threads);
    if (strcmp(src->kind(), "bgzf") != 0) return src;
    std::vector<unsigned char> head;
    const unsigned char* p = nullptr;
    size_t n = 0;
    while (head.size() < 4 && src->next_chunk(p, n)) head.insert(head.end(), p, p + n);
    is_bam = head.size() >= 4 && memcmp(head.data(), "BAM\1", 4) == 0;
    return std::make_unique<PrefixSource>(std::move(head), std::move(src));
}

void BamReader::bad(uint64_t at, const char* what) const
{
    throw std::runtime_error("'" + path_ + "': not a valid BAM record at decompressed byte " + std::to_string(at) + " (" + what + ")");
}

bool BamReader::fill(size_t n)
{
    while (buf_.size() - pos_ < n) {
        if (pos_ && pos_ >= buf_.size() / 2) {
            buf_.erase(buf_.begin(), buf_.begin() + (long)pos_);
            pos_ = 0;
        }
        const unsigned char* p = nullptr;
        size_t m = 0;
        if (!src_->next_chunk(p, m)) return false;
        buf_.insert(buf_.end(), p, p + m);
    }
    return true;
}

BamReader::BamReader(std::unique_ptr<ByteSource> src, const std::string& path, bool keep_refs) : src_(std::move(src)), path_(path)
{
    // magic, l_text, text, n_ref, then per reference l_name, name, l_ref
    uint64_t need = 8;
    if (!fill(need)) bad(buf_.size(), "truncated header");
    if (memcmp(buf_.data(), "BAM\1", 4) != 0) bad(0, "no BAM magic");
    const int32_t l_text = (int32_t)le32(buf_.data() + 4);
    if (l_text < 0) bad(4, "negative l_text");
    need += (uint64_t)l_text + 4;
    if (!fill(need)) bad(buf_.size(), "truncated header");
    n_ref_ = (int32_t)le32(buf_.data() + need - 4);
    if (n_ref_ < 0) bad(need - 4, "negative n_ref");
    // the references are read a piece at a time: the header may be large, the buffer only holds what is needed
    off_ = need;
    pos_ = need;
    for (int32_t r = 0; r < n_ref_; ++r) {
        if (!fill(4)) bad(off_ + (buf_.size() - pos_), "truncated header");
        const int32_t l_name = (int32_t)le32(buf_.data() + pos_);
        if (l_name < 0) bad(off_, "negative l_name");
        if (!fill(8 + (size_t)l_name)) bad(off_ + (buf_.size() - pos_), "truncated header");
        if (keep_refs) {
            const char* nm = reinterpret_cast<const char*>(buf_.data() + pos_ + 4);
            ref_names_.emplace_back(nm, strnlen(nm, (size_t)l_name));
            ref_lengths_.push_back(le32(buf_.data() + pos_ + 4 + (size_t)l_name));
        }
        pos_ += 8 + (size_t)l_name;
        off_ += 8 + (uint64_t)l_name;
    }
    header_bytes_ = off_;
}

void BamReader::skip_to(uint64_t offset)
{
    while (off_ < offset) {
        if (pos_ == buf_.size()) {
            buf_.clear();
            pos_ = 0;
            if (!fill(1)) return;
        }
        const size_t d = (size_t)std::min<uint64_t>(offset - off_, buf_.size() - pos_);
        pos_ += d;
        off_ += d;
    }
}

long BamReader::next()
{
    static const char nt16[] = "=ACMGRSVTWYHKDBN";
    for (;;) {
        if (!fill(1)) return -1;
        const uint64_t at = off_;
        if (!fill(4)) bad(at, "block_size runs past the end of the data");
        const uint32_t bs = le32(buf_.data() + pos_);
        if (!fill(4 + (size_t)bs)) bad(at, "block_size runs past the end of the data");
        const unsigned char* r = buf_.data() + pos_;
        if (bs < 32) bad(at, "fixed fields longer than block_size");
        const int32_t ref = (int32_t)le32(r + 4), next_ref = (int32_t)le32(r + 24);
        if (ref < -1 || ref >= n_ref_) bad(at, "refID out of range");
        if (next_ref < -1 || next_ref >= n_ref_) bad(at, "next_refID out of range");
        const uint32_t l_rn = r[12], n_cig = r[16] | (uint32_t)r[17] << 8, flag = r[18] | (uint32_t)r[19] << 8, l_seq = le32(r + 20);
        if (l_rn == 0) bad(at, "l_read_name is 0");
        if (32ull + l_rn + 4ull * n_cig + (l_seq + 1ull) / 2 + l_seq > bs) bad(at, "fields longer than block_size");
        if (r[36 + l_rn - 1] != 0) bad(at, "read name not NUL-terminated");
        // the rule of vgmi_bam_filter.h (with every parameter at its default: flag & 0x900 == 0 and l_seq > 0)
        const int verdict =
            regions_.empty()
                ? bam_filter_verdict(filt_, RecordBytes{r}, (size_t)0, bs, l_rn, (uint32_t)r[13], n_cig, flag, l_seq, (double*)nullptr)
                : bam_filter_region_verdict(filt_, BamRegions{regions_.data(), (uint32_t)regions_.size(), unplaced_ ? 1u : 0u}, RecordBytes{r}, (size_t)0,
                                            bs, l_rn, (uint32_t)r[13], n_cig, flag, l_seq, ref, (int32_t)le32(r + 8), (double*)nullptr);
        if (verdict == BAM_FILTER_FAULT) bad(at, "auxiliary fields");
        pos_ += 4 + (size_t)bs;
        off_ += 4 + (uint64_t)bs;
        ++records_;
        if (verdict != BAM_FILTER_READ) continue;
        ++reads_;
        if (!rule_.keep(number_++)) continue;
        const unsigned char* s = r + 36 + l_rn + 4 * (size_t)n_cig;
        if (rf_.on()) {
            const int cls = read_filter_class(rf_.p, s + (l_seq + 1) / 2, l_seq, true);
            ++rf_.n_class[cls];
            if (cls != READ_PASS) continue;
        }
        seq_.resize(l_seq);
        for (uint32_t i = 0; i < l_seq; ++i) seq_[i] = nt16[(s[i >> 1] >> ((~i & 1) << 2)) & 15];
        qual_.assign(reinterpret_cast<const char*>(s + (l_seq + 1) / 2), l_seq);
        return (long)l_seq;
    }
}

namespace {
// plain decimal digits -> a number below 2^62; false for anything else
bool region_number(const std::string& t, int64_t& v)
{
    if (t.empty() || t.size() > 18) return false;
    v = 0;
    for (char c : t) {
        if (c < '0' || c > '9') return false;
        v = v * 10 + (c - '0');
    }
    return true;
}
}  // namespace

std::vector<BamInterval> resolve_bam_regions(const BamRegionSpec& spec, const std::vector<std::string>& ref_names, const std::string& path,
                                             uint64_t* bed_skipped)
{
    std::unordered_map<std::string, int32_t> ids;
    ids.reserve(ref_names.size());
    for (size_t i = 0; i < ref_names.size(); ++i) ids.emplace(ref_names[i], (int32_t)i);      // (a repeated name: its first id)
    std::vector<BamInterval> v;
    uint64_t skipped = 0;
    for (size_t a = 0; a < spec.list.size();) {
        size_t e = spec.list.find(',', a);
        if (e == std::string::npos) e = spec.list.size();
        const std::string item = spec.list.substr(a, e - a);
        a = e + 1;
        if (item.empty()) continue;
        auto malformed = [&]() -> void { throw std::runtime_error("region '" + item + "' is not NAME, NAME:BEG or NAME:BEG-END (1-based, BEG <= END <= 2^31)"); };
        int64_t beg = 0, end = VGH_BAM_REGION_END;
        auto it = ids.find(item);
        if (it == ids.end()) {
            const size_t colon = item.rfind(':');
            const std::string name = colon == std::string::npos ? item : item.substr(0, colon);
            it = ids.find(name);
            if (it == ids.end()) throw std::runtime_error("'" + path + "': reference '" + name + "' of region '" + item + "' is not in the header");
            const std::string range = item.substr(colon + 1);
            const size_t dash = range.find('-');
            int64_t b1 = 0, e1 = 0;
            if (!region_number(range.substr(0, dash), b1) || b1 < 1 || b1 > VGH_BAM_REGION_END) malformed();
            beg = b1 - 1;
            if (dash != std::string::npos) {
                if (!region_number(range.substr(dash + 1), e1) || e1 < b1 || e1 > VGH_BAM_REGION_END) malformed();
                end = e1;
            }
        }
        v.push_back(BamInterval{it->second, (uint32_t)beg, (uint32_t)end});
    }
    if (!spec.bed.empty()) {
        std::ifstream in(spec.bed);
        if (!in) throw std::runtime_error("'" + spec.bed + "': No such file or directory.");
        std::string line;
        for (uint64_t no = 1; std::getline(in, line); ++no) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
            std::string col[3];
            size_t p = 0;
            int n_col = 0;
            for (; n_col < 3 && p <= line.size(); ++n_col) {
                size_t q = line.find_first_of("\t ", p);
                if (q == std::string::npos) q = line.size();
                col[n_col] = line.substr(p, q - p);
                p = line.find_first_not_of("\t ", q);
                if (p == std::string::npos) p = line.size() + 1;
            }
            int64_t b0 = 0, e0 = 0;
            if (n_col < 3 || !region_number(col[1], b0) || !region_number(col[2], e0) || b0 >= e0 || e0 > VGH_BAM_REGION_END)
                throw std::runtime_error("'" + spec.bed + "': line " + std::to_string(no) + " is not NAME START END with 0 <= START < END <= 2^31");
            const auto it = ids.find(col[0]);
            if (it == ids.end()) {
                ++skipped;
                continue;
            }
            v.push_back(BamInterval{it->second, (uint32_t)b0, (uint32_t)e0});
        }
    }
    bam_regions_normalise(v);
    if (v.size() > VGH_BAM_MAX_REGIONS) throw std::runtime_error(bam_regions_invalid_text(5));
    // (an empty list would mean "no region test" to every reader: a BED file none of whose lines names a reference of this header is refused)
    if (v.empty() && spec.on()) throw std::runtime_error("'" + path + "': no line of '" + spec.bed + "' names a reference of the header");
    if (bed_skipped) *bed_skipped = skipped;
    return v;
}

uint64_t BamReader::mask_below(uint32_t q)
{
    if (q == 0 || qual_.size() != seq_.size() || qual_.empty() || (unsigned char)qual_[0] == 0xFFu) return 0;
    uint64_t n = 0;
    for (size_t i = 0; i < seq_.size(); ++i)
        if ((unsigned char)qual_[i] < q) {
            seq_[i] = 'N';
            ++n;
        }
    return n;
}

}  // namespace vgh
