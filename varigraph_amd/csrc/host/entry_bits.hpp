// entry_bits.hpp -- how the host reads one entry of a node's k-mer list when its products stay on the device: which haplotypes of a window's
// list count as carrying the k-mer (hidden_states' rules, src/genotype.cpp:690-760) and whether a drawn haplotype carries it at all (the
// prune, :673-686).  Two forms of the same reading:
//   packed   one 64-bit word per entry -- coverage | multiplicity << 8 | haplotype bits << 16 -- for graphs of up to six bytes of bits
//   bytes    coverage, multiplicity and the entry's `bl` bytes as they stand in the graph's bit vectors, for 7 to 64 bytes (up to 511
//            haplotypes); masks over haplotype ids are then W = words_of(bl) 64-bit words, word i holding haplotypes 64 i .. 64 i + 63
// In both the LAST bit of the vector (bit 8 bl - 1) is a flag, never a haplotype.  The device's kernels read the same entries the same way
// (vgmi_hmm.hip); tests/native/entry_bits_check.cpp holds the two forms against each other and against a literal model.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace vgh {

inline uint32_t words_of(uint32_t bl) { return bl <= 8 ? 1u : bl <= 16 ? 2u : bl <= 32 ? 4u : 8u; }

// 2: the entry asks for the haplotypes' sequences (under-covered, multi-copy); 1: it is checked once they are there; 0: neither
inline uint32_t entry_low_multi(uint8_t c, uint8_t f, double lower) { return (c < lower && f >= 2) ? 2u : (!(c > lower || f <= 1)) ? 1u : 0u; }

// bits over the places of `used`: the haplotypes that count as carrying the k-mer.  gt0_mask: the places whose haplotype carries the
// reference allele at this node -- they carry every k-mer with the last bit set whose coverage lies in [lower, upper]
inline uint64_t carried_packed(uint64_t w, uint32_t bl, const uint16_t* used, size_t n_used, uint64_t gt0_mask, double lower, double upper, uint32_t& low_multi)
{
    const uint8_t c = (uint8_t)w, f = (uint8_t)(w >> 8);
    const uint64_t bits = w >> 16;
    const int lb = (int)((bits >> (8 * bl - 1)) & 1u);
    const bool in_interval = lb == 1 && c >= lower && c <= upper;
    uint64_t om = 0;
    for (size_t p = 0; p < n_used; ++p) om |= (uint64_t)((in_interval && ((gt0_mask >> p) & 1u)) ? 1u : (uint32_t)((bits >> used[p]) & 1u)) << p;
    low_multi = entry_low_multi(c, f, lower);
    return om;
}

inline uint64_t carried_bytes(uint8_t c, uint8_t f, const uint8_t* bits, uint32_t bl, const uint16_t* used, size_t n_used, uint64_t gt0_mask, double lower,
                              double upper, uint32_t& low_multi)
{
    const int lb = (bits[bl - 1] >> 7) & 1;
    const bool in_interval = lb == 1 && c >= lower && c <= upper;
    uint64_t om = 0;
    for (size_t p = 0; p < n_used; ++p) {
        const uint32_t hap = used[p];      // (< 8 bl - 1: the caller's haplotypes are the panel's)
        om |= (uint64_t)((in_interval && ((gt0_mask >> p) & 1u)) ? 1u : (uint32_t)((bits[hap >> 3] >> (hap & 7u)) & 1u)) << p;
    }
    low_multi = entry_low_multi(c, f, lower);
    return om;
}

// the prune: does any haplotype of `mask` carry the entry?
inline bool meets_packed(uint64_t w, uint64_t mask) { return ((w >> 16) & mask) != 0; }

inline bool meets_bytes(const uint8_t* bits, uint32_t bl, const uint64_t* mask)
{
    uint64_t met = 0;
    for (uint32_t i = 0; 8 * i < bl; ++i) {
        uint64_t word = 0;
        const uint32_t n = bl - 8 * i < 8 ? bl - 8 * i : 8;
        std::memcpy(&word, bits + 8 * i, n);      // little-endian: byte j of the vector is byte j of the words
        met |= word & mask[i];
    }
    return met != 0;
}

}  // namespace vgh
