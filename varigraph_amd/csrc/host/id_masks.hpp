// id_masks.hpp -- masks over haplotype IDS for a polyploid sample over a panel of 48 to 254 haplotypes.  The host's sequence checks and
// reference-allele masks are 64 bits over the PLACES of a window's `used` list (sequence_fixes, SelectedPart::gt0); the device's kernels
// for such a sample (vgmi_hmm_emissions_select_ploidy_wide) take W = words_of(bit_len) 64-bit words over ids, word i holding haplotypes
// 64 i .. 64 i + 63, as entry_bits.hpp's meets_bytes reads them.  tests/native/id_masks_check.cpp holds this against a bool per haplotype.
#pragma once
#include <cstddef>
#include <cstdint>

#include "entry_bits.hpp"

namespace vgh {

// words[0 .. W) |= the haplotypes used[p] of the places p set in `places`.  A place at or beyond n_used names nothing; every used[p] is
// below 64 W (the caller's haplotypes are the panel's: below 8 bit_len - 1)
inline void places_to_ids(uint64_t places, const uint16_t* used, size_t n_used, uint64_t* words)
{
    for (size_t p = 0; p < n_used && p < 64; ++p)
        if ((places >> p) & 1u) words[used[p] >> 6] |= 1ull << (used[p] & 63u);
}

// Which polyploid samples take the device path over such a panel: 7 to 32 bytes of haplotype bits, 3 to 8 haplotypes per genotype, and no
// more PLACES than the host's 64-bit masks hold -- a window names up to -n x ploidy distinct haplotypes
inline bool wide_ploidy_sample(uint64_t bit_len, uint32_t ploidy, uint64_t n_drawn)
{
    return bit_len >= 7 && bit_len <= 32 && ploidy >= 3 && ploidy <= 8 && n_drawn >= 1 && n_drawn * ploidy <= 64;
}

}  // namespace vgh
