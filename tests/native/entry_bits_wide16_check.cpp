// entry_bits_wide16_check.cpp -- csrc/host/entry_bits.hpp beyond 32 bytes of haplotype bits (panels of 255 to 511 haplotypes, eight words per
// mask): words_of over 1 to 64 bytes, and carried_bytes / meets_bytes at 33, 40, 41, 63 and 64 bytes against a literal model -- one bool per
// haplotype, no words, no shifts of words.  Every selection can name ids 255, 256 (the first no byte holds) and 8 bl - 2 (the last haplotype);
// one entry in eight has no bit but (perhaps) the flag.  Stand-alone; meant to run under -fsanitize=address,undefined: entries and masks are
// allocated at their exact sizes, so a read past an entry's last byte or a mask's last word is a report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "entry_bits.hpp"

namespace {
struct Lit {      // an entry, literally
    std::vector<bool> carries;      // per haplotype id, 8 bl - 1 of them
    bool last = false;
    uint8_t c = 0, f = 0;
};

size_t failures = 0;
void expect(bool ok, const char* what, uint32_t bl, size_t i)
{
    if (ok) return;
    if (failures++ < 20) std::fprintf(stderr, "MISMATCH %s: bit_len %u, entry %zu\n", what, bl, i);
}

uint64_t model_carried(const Lit& e, const std::vector<uint16_t>& used, uint64_t gt0, double lower, double upper, uint32_t& lm)
{
    const bool in_interval = e.last && e.c >= lower && e.c <= upper;
    uint64_t om = 0;
    for (size_t p = 0; p < used.size(); ++p) {
        const bool one = (in_interval && ((gt0 >> p) & 1u)) ? true : (bool)e.carries[used[p]];
        if (one) om |= 1ull << p;
    }
    lm = (e.c < lower && e.f >= 2) ? 2u : (e.c <= lower && e.f > 1) ? 1u : 0u;
    return om;
}

void run(uint32_t bl, std::mt19937_64& rng, size_t n)
{
    const uint32_t n_hap = 8 * bl - 1, W = vgh::words_of(bl);
    const double lower = 14.0, upper = 33.0;
    static const uint8_t covs[] = {0, 1, 5, 13, 14, 15, 23, 33, 34, 60, 255};
    // haplotypes the selections must be able to name: the first, the last (8 bl - 2), 255 and 256, and both sides of every word boundary
    std::vector<uint16_t> edge = {0, (uint16_t)(n_hap - 1), 255, 256};
    for (uint32_t b = 63; b + 1 < n_hap; b += 64) {
        edge.push_back((uint16_t)b);
        edge.push_back((uint16_t)(b + 1));
    }
    size_t flag_only = 0, beyond_byte = 0;
    for (size_t i = 0; i < n; ++i) {
        Lit e;
        e.carries.assign(n_hap, false);
        const unsigned kind = (unsigned)(rng() % 8);
        if (kind == 0) {
            // nothing but (perhaps) the flag: never carried, never meets a mask
        } else if (kind == 1) {
            e.carries[edge[rng() % edge.size()]] = true;      // one haplotype at an edge
        } else {
            const unsigned den = 2 + (unsigned)(rng() % 40);
            for (uint32_t h = 0; h < n_hap; ++h) e.carries[h] = rng() % den == 0;
        }
        e.last = rng() % 2;
        flag_only += kind == 0 && e.last;
        e.c = covs[rng() % (sizeof covs)];
        e.f = (uint8_t)(rng() % 5);
        std::unique_ptr<uint8_t[]> bytes(new uint8_t[bl]());      // exactly bl bytes
        for (uint32_t h = 0; h < n_hap; ++h)
            if (e.carries[h]) bytes[h >> 3] |= (uint8_t)(1u << (h & 7u));
        if (e.last) bytes[bl - 1] |= 0x80u;
        // a window's list: 1 .. 16 distinct haplotypes, ascending, biased to the edges
        const size_t n_used = 1 + rng() % 16;
        std::vector<bool> in(n_hap, false);
        std::vector<uint16_t> used;
        while (used.size() < n_used) {
            const uint16_t h = rng() % 3 == 0 ? edge[rng() % edge.size()] : (uint16_t)(rng() % n_hap);
            if (in[h]) continue;
            in[h] = true;
            used.push_back(h);
        }
        std::sort(used.begin(), used.end());
        beyond_byte += used.back() > 255;
        const uint64_t gt0 = rng() & ((1ull << n_used) - 1ull);
        std::unique_ptr<uint64_t[]> mask(new uint64_t[W]());      // exactly W words
        bool model_meets = false;
        for (uint16_t h : used) {
            mask[h >> 6] |= 1ull << (h & 63u);
            model_meets = model_meets || e.carries[h];
        }
        uint32_t lm_model = 0, lm_bytes = 0;
        const uint64_t om_model = model_carried(e, used, gt0, lower, upper, lm_model);
        const uint64_t om_bytes = vgh::carried_bytes(e.c, e.f, bytes.get(), bl, used.data(), used.size(), gt0, lower, upper, lm_bytes);
        expect(om_bytes == om_model && lm_bytes == lm_model, "carried_bytes against the model", bl, i);
        expect(vgh::meets_bytes(bytes.get(), bl, mask.get()) == model_meets, "meets_bytes against the model", bl, i);
    }
    expect(flag_only > 0 && beyond_byte > n / 4, "the cases the run is for", bl, n);
}
}  // namespace

int main()
{
    for (uint32_t bl = 1; bl <= 64; ++bl) {
        const uint32_t want = bl <= 8 ? 1u : bl <= 16 ? 2u : bl <= 32 ? 4u : 8u;
        expect(vgh::words_of(bl) == want && 8 * vgh::words_of(bl) >= bl, "words_of", bl, 0);
    }
    std::mt19937_64 rng(20261020);
    size_t n = 0;
    for (uint32_t bl : {33u, 40u, 41u, 63u, 64u}) {
        run(bl, rng, 20000);
        n += 20000;
    }
    if (failures) {
        std::printf("%zu mismatches\n", failures);
        return 1;
    }
    std::printf("entry readings identical: words_of at 1 .. 64, %zu entries at bit_len 33, 40, 41, 63, 64 (bytes and model)\n", n);
    return 0;
}
