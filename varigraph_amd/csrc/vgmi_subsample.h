// The rule of `genotype --subsample F --subsample-seed S`, written once: the host readers, the device kernels (vgmi_fastq.hip,
// vgmi_fasta.hip, vgmi_bam.hip include this header) and the stand-alone check (tests/native/subsample_check.cpp) all call
// subsample_keep.  Not the reference's behaviour (it has no such option): the result is the reference's on the file with the
// dropped reads removed.  It lies beside the kernels' headers, where the build's header glob finds it; the host library includes it too.
//
// A file's reads are numbered i = 0, 1, 2, ... in file order (FASTQ / FASTA: the records; BAM: the records that pass the read filter,
// flag & 0x900 == 0 and l_seq > 0).  Read i is kept iff z(i, S) < T, all arithmetic mod 2^64:
//   T = (uint64_t)(F * 2^64)                       exact: a power-of-two scaling of the double, then truncation
//   x = (i + 1) * 0x9E3779B97F4A7C15 + S           then the splitmix64 finaliser
// so the kept set depends on the file, F and S alone -- not on chunks, containers, or which reader served a record.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VGH_SUBSAMPLE_HD __host__ __device__
#else
#define VGH_SUBSAMPLE_HD
#endif

namespace vgh {

VGH_SUBSAMPLE_HD inline uint64_t subsample_hash(uint64_t i, uint64_t seed)
{
    uint64_t x = (i + 1u) * 0x9E3779B97F4A7C15ull + seed;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// read i of a file is kept
VGH_SUBSAMPLE_HD inline bool subsample_keep(uint64_t i, uint64_t seed, uint64_t threshold) { return subsample_hash(i, seed) < threshold; }

// a fraction the option takes: in (0, 1], not NaN
inline bool subsample_fraction_valid(double f) { return f > 0.0 && f <= 1.0; }

// T of a valid fraction below 1 (1 itself is "off": every caller tests for it first, and 2^64 does not fit).  ldexp of a double is
// exact, the product is below 2^64, and the conversion truncates.
inline uint64_t subsample_threshold(double f) { return (uint64_t)(f * 18446744073709551616.0); }

// what a reader carries: off (fraction 1) keeps every read without evaluating anything
struct SubsampleRule {
    bool on = false;
    uint64_t seed = 11;
    uint64_t threshold = 0;
    double fraction = 1.0;
    SubsampleRule() = default;
    SubsampleRule(double f, uint64_t s) : on(f < 1.0), seed(s), threshold(f < 1.0 ? subsample_threshold(f) : 0), fraction(f) {}
    bool keep(uint64_t i) const { return !on || subsample_keep(i, seed, threshold); }
};

}  // namespace vgh
