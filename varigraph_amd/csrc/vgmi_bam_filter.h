// The read filter of a BAM stream (`genotype --bam-exclude-flags / --bam-require-flags / --bam-min-mapq / --bam-min-tag`), written
// once: the device's record kernels (vgmi_bam.hip), the host decoder (csrc/host/bam_reader.cpp) and the stand-alone check
// (tests/native/bam_filter_check.cpp) all call bam_filter_verdict.  Not the reference's behaviour (it reads FASTQ): the result is the
// reference's on the FASTQ twin of the BAM with exactly the filtered records removed.
//
// A valid record of the chain is a read iff
//   1  l_seq > 0
//   2  (flag & exclude) == 0                   exclude replaces the default 0x900, as `samtools fastq -F` does
//   3  (flag & require) == require
//   4  mapq >= min_mapq                        the byte at offset 13 as a number: 255 passes, an unmapped record's 0 fails a positive bound
//   5  with a tag bound: the FIRST auxiliary field carrying the tag is numeric (c C s S i I f, and d as 8 bytes) and its value, as a
//      double (integers exact, f promoted), is >= min_value; NaN fails; absent or of type A Z H B: not a read (`samtools view -e '[tg]>=v'`)
// With a region list (`--bam-regions`, further down) the region test stands between 4 and the tag bound, and the walk waits for it too.
// The auxiliary walk runs only with a tag bound and only for records that passed 1 to 4.  It goes from behind QUAL to the record's end
// or to the first field with the tag; what lies behind that field is not looked at.  A field's value takes 1 (A c C), 2 (s S), 4 (i I f)
// or 8 (d) bytes, up to and including the NUL (Z H), or subtype + 32-bit count + count x size (B, subtype in cCsSiIf).  A walk fault --
// one or two bytes left in front of the record's end, an unknown type or subtype, a value that runs past the record's end (the count
// arithmetic in 64 bits), a Z / H without NUL inside the record -- makes the record invalid: the device stops at its first byte, the
// host decoder names it.
//
// The record's bytes come through an accessor `B` with u8(p), u32(p) (little endian, any alignment) and find_nul(p, end) (the first
// p' in [p, end) with a zero byte, or end), p counted as the caller counts: the device reads aligned dwords, the host a byte array.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VGH_BAMF_HD __host__ __device__
#else
#define VGH_BAMF_HD
#endif

namespace vgh {

// what a chunk's kernels and a reader carry; on == 0: every member at its default, the filter of before the options existed
struct BamFilterParams {
    uint32_t on;
    uint32_t exclude, require, min_mapq;
    uint32_t tag;          // 0: no tag bound; else 0x10000 | second byte << 8 | first byte
    double min_value;
};

enum : int { BAM_FILTER_FAULT = -1, BAM_FILTER_DROP = 0, BAM_FILTER_READ = 1 };

// bytes of one element of a B array (0: not a subtype)
VGH_BAMF_HD inline uint32_t bam_aux_elem_size(uint32_t sub)
{
    switch (sub) {
    case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    default: return 0;
    }
}

// The walk over the auxiliary fields in [p, end) for the tag (t0, t1).  BAM_FILTER_READ: its first field is numeric, *value is set;
// BAM_FILTER_DROP: no such field, or not numeric; BAM_FILTER_FAULT: a walk fault in front of that field or in it.
template <class B, class Pos>
VGH_BAMF_HD inline int bam_aux_find(const B& b, Pos p, Pos end, uint32_t t0, uint32_t t1, double* value)
{
    while (p != end) {
        if (end - p < 3) return BAM_FILTER_FAULT;
        const bool hit = b.u8(p) == t0 && b.u8(p + 1) == t1;
        const uint32_t type = b.u8(p + 2);
        p += 3;
        const uint64_t left = end - p;
        uint64_t n;
        switch (type) {
        case 'A': case 'c': case 'C': n = 1; break;
        case 's': case 'S': n = 2; break;
        case 'i': case 'I': case 'f': n = 4; break;
        case 'd': n = 8; break;
        case 'Z': case 'H': {
            const Pos z = b.find_nul(p, end);
            if (z == end) return BAM_FILTER_FAULT;
            n = (uint64_t)(z - p) + 1;
            break;
        }
        case 'B': {
            if (left < 5) return BAM_FILTER_FAULT;
            const uint32_t sz = bam_aux_elem_size(b.u8(p));
            if (!sz) return BAM_FILTER_FAULT;
            n = 5 + (uint64_t)b.u32(p + 1) * sz;
            break;
        }
        default: return BAM_FILTER_FAULT;
        }
        if (n > left) return BAM_FILTER_FAULT;
        if (hit) {
            double v;
            switch (type) {
            case 'c': v = (double)(int8_t)b.u8(p); break;
            case 'C': v = (double)b.u8(p); break;
            case 's': v = (double)(int16_t)(b.u8(p) | b.u8(p + 1) << 8); break;
            case 'S': v = (double)(b.u8(p) | b.u8(p + 1) << 8); break;
            case 'i': v = (double)(int32_t)b.u32(p); break;
            case 'I': v = (double)b.u32(p); break;
            case 'f': {
                const uint32_t w = b.u32(p);
                float f;
                __builtin_memcpy(&f, &w, 4);
                v = (double)f;
                break;
            }
            case 'd': {
                const uint64_t w = b.u32(p) | (uint64_t)b.u32(p + 4) << 32;
                __builtin_memcpy(&v, &w, 8);
                break;
            }
            default: return BAM_FILTER_DROP;
            }
            *value = v;
            return BAM_FILTER_READ;
        }
        p += (Pos)n;
    }
    return BAM_FILTER_DROP;
}

// The rule on a valid record that starts at o (its block_size field; the fixed fields given as the caller has loaded them).  *value: the
// tag's value where the walk found a numeric one (else untouched).
template <class B, class Pos>
VGH_BAMF_HD inline int bam_filter_verdict(const BamFilterParams& f, const B& b, Pos o, uint32_t block_size, uint32_t l_read_name, uint32_t mapq,
                                          uint32_t n_cigar_op, uint32_t flag, uint32_t l_seq, double* value)
{
    if (l_seq == 0 || (flag & f.exclude) != 0 || (flag & f.require) != f.require || mapq < f.min_mapq) return BAM_FILTER_DROP;
    if (!f.tag) return BAM_FILTER_READ;
    const Pos aux = o + (Pos)(36u + l_read_name + 4u * n_cigar_op + (l_seq + 1u) / 2u + l_seq);      // (the validity check bounds it by block_size)
    double v = 0.0;
    const int r = bam_aux_find(b, aux, o + (Pos)4u + (Pos)block_size, f.tag & 0xFFu, (f.tag >> 8) & 0xFFu, &v);
    if (r != BAM_FILTER_READ) return r;
    if (value) *value = v;
    return v >= f.min_value ? BAM_FILTER_READ : BAM_FILTER_DROP;      // (a NaN value compares false)
}

// ---- condition 5: the region test (`genotype --bam-regions / --bam-regions-file / --bam-regions-unplaced`) --------------------------
// With a region list the rule above gains a condition between 4 and the tag bound, which becomes condition 6: the auxiliary walk runs
// only for records that passed 1 to 5, so a record the region test drops is never walked and cannot fault.
//   5  refID == -1: the record passes iff `unplaced` is set.  refID >= 0: it passes iff some interval (ref, beg, end) -- 0-based, half
//      open -- has ref == refID, pos < end and endpos > beg, in signed 64-bit arithmetic.  pos is the signed field at offset 8;
//      endpos = pos + 1 if flag & 0x4, n_cigar_op == 0 or reflen == 0, else pos + reflen; reflen = the sum of cigar >> 4 over the
//      operations whose code cigar & 15 is M(0) D(2) N(3) =(7) X(8).  I S H P and the undefined codes 9 to 15 consume nothing.
// This is bam_endpos with bed_overlap, what `samtools view -L` does on a stream.  An unmapped record without CIGAR at pos == -1 has
// endpos 0 and overlaps nothing.  The placeholder CIGAR <l_seq>S<reflen>N of a record whose CIGAR is in a CG tag gives the right end.
// The list is normalised (bam_regions_normalise): sorted by (ref, beg), overlapping or touching intervals of one reference merged, so
// that beg[i] < end[i] < beg[i + 1] inside a reference.  bam_region_overlap_plain is the definition; bam_region_overlap is what the
// kernel and the host decoder call, and the stand-alone check holds the one against the other.
struct BamInterval {
    int32_t ref;
    uint32_t beg, end;      // 0 <= beg < end <= 2^31
};

// a normalised list where the caller keeps it (device or host memory); n == 0: no region test
struct BamRegions {
    const BamInterval* iv;
    uint32_t n;
    uint32_t unplaced;
};

#define VGH_BAM_MAX_REGIONS (1u << 20)
#define VGH_BAM_REGION_END (1ll << 31)

VGH_BAMF_HD inline bool bam_cigar_consumes_ref(uint32_t op)
{
    return ((1u << (op & 15u)) & ((1u << 0) | (1u << 2) | (1u << 3) | (1u << 7) | (1u << 8))) != 0;
}

// the definition: every interval looked at, the whole CIGAR summed (cig: the position of the first CIGAR dword, as B counts)
template <class B, class Pos>
VGH_BAMF_HD inline bool bam_region_overlap_plain(const BamRegions& g, const B& b, Pos cig, uint32_t n_cigar_op, uint32_t flag, int32_t ref_id,
                                                 int32_t pos32)
{
    if (ref_id < 0) return g.unplaced != 0;
    const int64_t pos = pos32;
    int64_t reflen = 0;
    for (uint32_t i = 0; i < n_cigar_op; ++i) {
        const uint32_t c = b.u32(cig + (Pos)(4u * i));
        if (bam_cigar_consumes_ref(c)) reflen += (int64_t)(c >> 4);
    }
    const int64_t endpos = ((flag & 0x4u) || n_cigar_op == 0 || reflen == 0) ? pos + 1 : pos + reflen;
    for (uint32_t i = 0; i < g.n; ++i)
        if (g.iv[i].ref == ref_id && pos < (int64_t)g.iv[i].end && endpos > (int64_t)g.iv[i].beg) return true;
    return false;
}

// The same verdict on a normalised list by one binary search: j = the last interval with (ref, beg) <= (refID, pos).  pos inside j:
// an overlap, whatever the CIGAR says (endpos > pos >= beg).  Else the intervals up to j end at or in front of pos, and the only
// interval the record can reach first is j + 1: none of refID there, or an endpos of pos + 1: no overlap, the CIGAR unread.  Otherwise
// the CIGAR is summed until pos + reflen passes that interval's beg.
template <class B, class Pos>
VGH_BAMF_HD inline bool bam_region_overlap(const BamRegions& g, const B& b, Pos cig, uint32_t n_cigar_op, uint32_t flag, int32_t ref_id, int32_t pos32)
{
    if (ref_id < 0) return g.unplaced != 0;
    const int64_t pos = pos32;
    const int64_t key = (int64_t)ref_id * (1ll << 32) + pos;      // (beg < 2^31: a negative pos still sorts behind the reference in front)
    uint32_t lo = 0, hi = g.n;      // the first interval with (ref, beg) > (refID, pos)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        const int64_t k = (int64_t)g.iv[mid].ref * (1ll << 32) + (int64_t)g.iv[mid].beg;
        if (k <= key) lo = mid + 1u;
        else hi = mid;
    }
    if (lo > 0 && g.iv[lo - 1u].ref == ref_id && (int64_t)g.iv[lo - 1u].end > pos) return true;
    if (lo == g.n || g.iv[lo].ref != ref_id) return false;
    if ((flag & 0x4u) || n_cigar_op == 0) return false;      // endpos = pos + 1 <= beg
    const int64_t reach = (int64_t)g.iv[lo].beg - pos;       // > 0: the reference length that passes beg
    int64_t reflen = 0;
    for (uint32_t i = 0; i < n_cigar_op; ++i) {
        const uint32_t c = b.u32(cig + (Pos)(4u * i));
        if (bam_cigar_consumes_ref(c)) {
            reflen += (int64_t)(c >> 4);
            if (reflen > reach) return true;
        }
    }
    return false;      // (reflen == 0: endpos = pos + 1 <= beg as well)
}

// The rule with a region list: bam_filter_verdict with condition 5 in front of the tag bound.  f: the filter's parameters, the defaults
// of bam_filter_params() where none was configured.  ref_id, pos: the signed fields at offsets 4 and 8.
template <class B, class Pos>
VGH_BAMF_HD inline int bam_filter_region_verdict(const BamFilterParams& f, const BamRegions& g, const B& b, Pos o, uint32_t block_size,
                                                 uint32_t l_read_name, uint32_t mapq, uint32_t n_cigar_op, uint32_t flag, uint32_t l_seq, int32_t ref_id,
                                                 int32_t pos, double* value)
{
    if (l_seq == 0 || (flag & f.exclude) != 0 || (flag & f.require) != f.require || mapq < f.min_mapq) return BAM_FILTER_DROP;
    if (g.n && !bam_region_overlap(g, b, o + (Pos)(36u + l_read_name), n_cigar_op, flag, ref_id, pos)) return BAM_FILTER_DROP;
    if (!f.tag) return BAM_FILTER_READ;
    const Pos aux = o + (Pos)(36u + l_read_name + 4u * n_cigar_op + (l_seq + 1u) / 2u + l_seq);
    double v = 0.0;
    const int r = bam_aux_find(b, aux, o + (Pos)4u + (Pos)block_size, f.tag & 0xFFu, (f.tag >> 8) & 0xFFu, &v);
    if (r != BAM_FILTER_READ) return r;
    if (value) *value = v;
    return v >= f.min_value ? BAM_FILTER_READ : BAM_FILTER_DROP;
}

// ---- the host's side: parameters as the options give them ---------------------------------------------------------------------------
inline bool bam_filter_tag_valid(const char* t)
{
    auto letter = [](char c) { return (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z'); };
    return t && letter(t[0]) && (letter(t[1]) || (t[1] >= '0' && t[1] <= '9'));
}

// 0: fine; else which parameter is out of range (1 exclude, 2 require, 3 min_mapq, 4 tag, 5 a NaN bound)
inline int bam_filter_invalid(uint32_t exclude, uint32_t require, uint32_t min_mapq, const char* tag, double min_value)
{
    if (exclude > 0xFFFFu) return 1;
    if (require > 0xFFFFu) return 2;
    if (min_mapq > 255u) return 3;
    if (tag && !bam_filter_tag_valid(tag)) return 4;
    if (tag && min_value != min_value) return 5;
    return 0;
}

inline const char* bam_filter_invalid_text(int which)
{
    switch (which) {
    case 1: return "BAM exclude flags are out of range (0..65535)";
    case 2: return "BAM require flags are out of range (0..65535)";
    case 3: return "BAM minimum MAPQ is out of range (0..255)";
    case 4: return "BAM tag is not a letter followed by a letter or digit";
    case 5: return "BAM tag bound is not a number";
    default: return "";
    }
}

// valid parameters (bam_filter_invalid == 0) as the kernels take them; the all-default call gives on == 0
inline BamFilterParams bam_filter_params(uint32_t exclude = 0x900u, uint32_t require = 0, uint32_t min_mapq = 0, const char* tag = nullptr,
                                         double min_value = 0.0)
{
    BamFilterParams f{};
    f.exclude = exclude;
    f.require = require;
    f.min_mapq = min_mapq;
    f.tag = tag ? 0x10000u | (uint32_t)(unsigned char)tag[1] << 8 | (uint32_t)(unsigned char)tag[0] : 0u;
    f.min_value = tag ? min_value : 0.0;
    f.on = exclude != 0x900u || require != 0 || min_mapq != 0 || tag != nullptr;
    return f;
}

// ---- the host's side of the region list ------------------------------------------------------------------------------------------------
// 0: fine; else what is wrong with the list as given (1 a ref outside [0, n_ref), 2 a beg outside [0, 2^31), 3 an end outside
// (beg, 2^31], 4 `unplaced` without a list); *which = the offending item
inline int bam_regions_invalid(uint32_t n, const int32_t* ref, const int64_t* beg, const int64_t* end, int unplaced, int32_t n_ref, uint32_t* which)
{
    for (uint32_t i = 0; i < n; ++i) {
        if (which) *which = i;
        if (ref[i] < 0 || ref[i] >= n_ref) return 1;
        if (beg[i] < 0 || beg[i] >= VGH_BAM_REGION_END) return 2;
        if (end[i] <= beg[i] || end[i] > VGH_BAM_REGION_END) return 3;
    }
    if (n == 0 && unplaced) return 4;
    return 0;
}

inline const char* bam_regions_invalid_text(int which)
{
    switch (which) {
    case 1: return "a BAM region names a reference outside the file's header";
    case 2: return "a BAM region's begin is out of range (0 <= beg < 2^31)";
    case 3: return "a BAM region's end is out of range (beg < end <= 2^31)";
    case 4: return "unplaced BAM reads are kept only together with a region list";
    case 5: return "more than 1048576 BAM regions remain after merging";
    default: return "";
    }
}

// valid intervals, any order -> sorted by (ref, beg), overlapping or touching ones of a reference merged
inline void bam_regions_normalise(std::vector<BamInterval>& v)
{
    std::sort(v.begin(), v.end(), [](const BamInterval& a, const BamInterval& b) { return a.ref != b.ref ? a.ref < b.ref : a.beg < b.beg; });
    size_t m = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        if (m && v[m - 1].ref == v[i].ref && v[i].beg <= v[m - 1].end) {
            if (v[i].end > v[m - 1].end) v[m - 1].end = v[i].end;
        } else {
            v[m++] = v[i];
        }
    }
    v.resize(m);
}

}  // namespace vgh
