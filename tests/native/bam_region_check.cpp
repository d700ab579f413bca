// bam_region_check.cpp -- the region test of csrc/vgmi_bam_filter.h (bam_regions_invalid, bam_regions_normalise, bam_region_overlap,
// bam_region_overlap_plain, bam_filter_region_verdict) on records and intervals read from files, for comparison with the Python model of
// tests/bam_region_cases.py.  A stand-alone program, built with -fsanitize=address,undefined by tests/test_bam_region_cpu.py: every
// record is copied into a heap block of exactly its size, and the normalised list into one of exactly its size, so a CIGAR walk or a
// binary search that reads past either end is reported.
//   bam_region_check FILE REGIONS N_REF UNPLACED EXCLUDE REQUIRE MIN_MAPQ TAG|- MIN_VALUE
// FILE holds BAM records back to back (block_size first); REGIONS holds "ref beg end" per line, in any order.  Output: "invalid K" and
// exit status 0 where bam_regions_invalid refuses the list (K its code); else "n M" and the M normalised intervals, one per line, then
// per record one line "V S P": the whole rule's verdict (1 read, 0 not a read, -1 walk fault), bam_region_overlap and
// bam_region_overlap_plain on the record's placement alone.
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
    if (argc != 10) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> all;
    unsigned char buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) all.insert(all.end(), buf, buf + n);
    std::fclose(f);
    std::vector<int32_t> ref;
    std::vector<int64_t> beg, end;
    f = std::fopen(argv[2], "r");
    if (!f) return 2;
    long long a, b, c;
    while (std::fscanf(f, "%lld %lld %lld", &a, &b, &c) == 3) ref.push_back((int32_t)a), beg.push_back(b), end.push_back(c);
    std::fclose(f);
    const int32_t n_ref = (int32_t)std::strtol(argv[3], nullptr, 0);
    const int unplaced = std::atoi(argv[4]);
    const uint32_t exclude = (uint32_t)std::strtoul(argv[5], nullptr, 0), require = (uint32_t)std::strtoul(argv[6], nullptr, 0),
                   min_mapq = (uint32_t)std::strtoul(argv[7], nullptr, 0);
    const char* tag = std::strcmp(argv[8], "-") ? argv[8] : nullptr;
    const double min_value = std::strtod(argv[9], nullptr);
    if (vgh::bam_filter_invalid(exclude, require, min_mapq, tag, min_value)) return 3;
    const vgh::BamFilterParams p = vgh::bam_filter_params(exclude, require, min_mapq, tag, min_value);
    uint32_t which = 0;
    if (const int bad = vgh::bam_regions_invalid((uint32_t)ref.size(), ref.data(), beg.data(), end.data(), unplaced, n_ref, &which)) {
        std::printf("invalid %d\n", bad);
        return 0;
    }
    std::vector<vgh::BamInterval> v(ref.size());
    for (size_t i = 0; i < ref.size(); ++i) v[i] = vgh::BamInterval{ref[i], (uint32_t)beg[i], (uint32_t)end[i]};
    vgh::bam_regions_normalise(v);
    std::printf("n %zu\n", v.size());
    for (const vgh::BamInterval& iv : v) std::printf("%d %u %u\n", iv.ref, iv.beg, iv.end);
    vgh::BamInterval* list = static_cast<vgh::BamInterval*>(std::malloc(v.size() * sizeof(vgh::BamInterval) + (v.empty() ? 1 : 0)));
    if (!v.empty()) std::memcpy(list, v.data(), v.size() * sizeof(vgh::BamInterval));
    const vgh::BamRegions g{list, (uint32_t)v.size(), unplaced ? 1u : 0u};
    for (size_t o = 0; o + 36 <= all.size();) {
        const uint32_t bs = Bytes{all.data()}.u32(o);
        if (bs < 32 || o + 4 + (size_t)bs > all.size()) return 4;
        unsigned char* rec = static_cast<unsigned char*>(std::malloc(4 + (size_t)bs));
        std::memcpy(rec, all.data() + o, 4 + (size_t)bs);
        const Bytes by{rec};
        const uint32_t l_rn = rec[12], n_cig = (uint32_t)(rec[16] | rec[17] << 8), flag = (uint32_t)(rec[18] | rec[19] << 8);
        const int32_t ref_id = (int32_t)by.u32(4), pos = (int32_t)by.u32(8);
        const int r = vgh::bam_filter_region_verdict(p, g, by, (size_t)0, bs, l_rn, rec[13], n_cig, flag, by.u32(20), ref_id, pos, (double*)nullptr);
        const bool fast = vgh::bam_region_overlap(g, by, (size_t)(36u + l_rn), n_cig, flag, ref_id, pos);
        const bool slow = vgh::bam_region_overlap_plain(g, by, (size_t)(36u + l_rn), n_cig, flag, ref_id, pos);
        std::printf("%d %d %d\n", r, fast ? 1 : 0, slow ? 1 : 0);
        std::free(rec);
        o += 4 + (size_t)bs;
    }
    std::free(list);
    return 0;
}
