// bam_filter_check.cpp -- vgh::bam_filter_verdict (csrc/vgmi_bam_filter.h) on records read from a file, for comparison with the Python
// model of tests/bam_filter_cases.py.  A stand-alone program, built with -fsanitize=address,undefined by tests/test_bam_filter_cpu.py:
// every record is copied into a heap block of exactly its size, so a walk that reads past a record's end is reported.
//   bam_filter_check FILE EXCLUDE REQUIRE MIN_MAPQ TAG|- MIN_VALUE
// FILE holds BAM records back to back (block_size first).  Per record one line: the verdict (1 read, 0 not a read, -1 walk fault) and
// the bits of the tag's value as a double, or "-" where the walk found no numeric one.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vgmi_bam_filter.h"

namespace {
struct Bytes {
    const unsigned char* r;
    uint32_t u8(size_t p) const { return r[p]; }
    uint32_t u32(size_t p) const { return r[p] | (uint32_t)r[p + 1] << 8 | (uint32_t)r[p + 2] << 16 | (uint32_t)r[p + 3] << 24; }
    size_t find_nul(size_t p, size_t end) const
    {
        while (p < end && r[p]) ++p;
        return p;
    }
};
}  // namespace

int main(int argc, char** argv)
{
    if (argc != 7) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> all;
    unsigned char buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + n);
    std::fclose(f);
    const uint32_t exclude = (uint32_t)std::strtoul(argv[2], nullptr, 0), require = (uint32_t)std::strtoul(argv[3], nullptr, 0),
                   min_mapq = (uint32_t)std::strtoul(argv[4], nullptr, 0);
    const char* tag = std::strcmp(argv[5], "-") ? argv[5] : nullptr;
    const double min_value = std::strtod(argv[6], nullptr);
    if (vgh::bam_filter_invalid(exclude, require, min_mapq, tag, min_value)) return 3;
    const vgh::BamFilterParams p = vgh::bam_filter_params(exclude, require, min_mapq, tag, min_value);
    for (size_t o = 0; o + 36 <= all.size();) {
        const uint32_t bs = Bytes{all.data()}.u32(o);
        if (bs < 32 || o + 4 + (size_t)bs > all.size()) return 4;
        unsigned char* rec = static_cast<unsigned char*>(std::malloc(4 + (size_t)bs));
        std::memcpy(rec, all.data() + o, 4 + (size_t)bs);
        const Bytes b{rec};
        double v = 0.0;
        bool have = false;
        // the value is set exactly when the walk found a numeric field: a sentinel the walk cannot produce tells
        uint64_t bits = 0x7FF8DEADBEEF0001ull;
        std::memcpy(&v, &bits, 8);
        const int r = vgh::bam_filter_verdict(p, b, (size_t)0, bs, rec[12], rec[13], (uint32_t)(rec[16] | rec[17] << 8),
                                              (uint32_t)(rec[18] | rec[19] << 8), b.u32(20), &v);
        std::memcpy(&bits, &v, 8);
        have = bits != 0x7FF8DEADBEEF0001ull;
        if (have) std::printf("%d %016llx\n", r, (unsigned long long)bits);
        else std::printf("%d -\n", r);
        std::free(rec);
        o += 4 + (size_t)bs;
    }
    return 0;
}
