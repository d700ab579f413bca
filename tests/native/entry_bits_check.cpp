// entry_bits_check.cpp -- csrc/host/entry_bits.hpp: the host's reading of an entry from the graph's bit vectors (7 to 32 bytes of haplotype
// bits) against (a) the packed word's reading at six bytes and fewer, entry by entry, and (b) a literal model -- one bool per haplotype, no
// words, no shifts of words -- at 7, 9 and 32 bytes.  Stand-alone; meant to run under -fsanitize=address,undefined: every vector is allocated
// at its exact size, so a read past an entry's last byte or a mask's last word is a report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    // haplotypes the selections must be able to name: the first, the last, and both sides of every word boundary
    std::vector<uint16_t> edge = {0, (uint16_t)(n_hap - 1)};
    for (uint32_t b = 63; b + 1 < n_hap; b += 64) {
        edge.push_back((uint16_t)b);
        edge.push_back((uint16_t)(b + 1));
    }
    for (size_t i = 0; i < n; ++i) {
        Lit e;
        e.carries.assign(n_hap, false);
        const unsigned kind = (unsigned)(rng() % 8);
        if (kind == 0) {
            // nothing but (perhaps) the last bit: never carried, never meets a mask
        } else if (kind == 1) {
            e.carries[edge[rng() % edge.size()]] = true;      // one haplotype at an edge
        } else {
            const unsigned den = 2 + (unsigned)(rng() % 12);
            for (uint32_t h = 0; h < n_hap; ++h) e.carries[h] = rng() % den == 0;
        }
        e.last = rng() % 2;
        e.c = covs[rng() % (sizeof covs)];
        e.f = (uint8_t)(rng() % 5);
        // the entry's bytes, in an allocation of exactly bl bytes
        std::unique_ptr<uint8_t[]> bytes(new uint8_t[bl]());
        for (uint32_t h = 0; h < n_hap; ++h)
            if (e.carries[h]) bytes[h >> 3] |= (uint8_t)(1u << (h & 7u));
        if (e.last) bytes[bl - 1] |= 0x80u;
        // a window's list: 1 .. 16 distinct haplotypes, ascending, biased to the edges
        const size_t n_used = 1 + rng() % std::min<size_t>(16, n_hap);
        std::vector<bool> in(n_hap, false);
        std::vector<uint16_t> used;
        while (used.size() < n_used) {
            const uint16_t h = rng() % 3 == 0 ? edge[rng() % edge.size()] : (uint16_t)(rng() % n_hap);
            if (in[h]) continue;
            in[h] = true;
            used.push_back(h);
        }
        std::sort(used.begin(), used.end());
        const uint64_t gt0 = rng() & ((1ull << n_used) - 1ull);
        std::unique_ptr<uint64_t[]> mask(new uint64_t[W]());
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
        if (bl <= 6) {      // ... and the packed word says the same
            uint64_t bits = 0;
            std::memcpy(&bits, bytes.get(), bl);
            const uint64_t w = (uint64_t)e.c | (uint64_t)e.f << 8 | bits << 16;
            uint32_t lm_packed = 0;
            const uint64_t om_packed = vgh::carried_packed(w, bl, used.data(), used.size(), gt0, lower, upper, lm_packed);
            expect(om_packed == om_bytes && lm_packed == lm_bytes, "carried_bytes against carried_packed", bl, i);
            expect(vgh::meets_packed(w, mask[0]) == vgh::meets_bytes(bytes.get(), bl, mask.get()), "meets_bytes against meets_packed", bl, i);
        }
    }
}
}  // namespace

int main()
{
    std::mt19937_64 rng(20261019);
    size_t n = 0;
    for (uint32_t bl : {1u, 3u, 6u, 7u, 8u, 9u, 16u, 17u, 32u}) {
        run(bl, rng, 20000);
        n += 20000;
    }
    if (failures) {
        std::printf("%zu mismatches\n", failures);
        return 1;
    }
    std::printf("entry readings identical: %zu entries at bit_len 1, 3, 6 (packed and bytes), 7, 8, 9, 16, 17, 32 (bytes and model)\n", n);
    return 0;
}
