// id_masks_check.cpp -- csrc/host/id_masks.hpp: masks over the places of a window's `used` list turned into W-word masks over haplotype ids,
// against a literal model -- one bool per haplotype, no words -- at 7, 8, 9, 16, 17 and 32 bytes of haplotype bits, and the bound on the
// samples that take the device path.  Stand-alone; meant to run under -fsanitize=address,undefined: the words are allocated at their exact
// size W, so a write past the last word is a report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include "id_masks.hpp"

namespace {
size_t failures = 0;
void expect(bool ok, const char* what, uint32_t bl, size_t i)
{
    if (ok) return;
    if (failures++ < 20) std::fprintf(stderr, "MISMATCH %s: bit_len %u, case %zu\n", what, bl, i);
}

// the words against one bool per haplotype: every id of `want` set, nothing else -- the flag bit and the padding included
void same(const uint64_t* words, uint32_t W, const std::vector<bool>& want, const char* what, uint32_t bl, size_t i)
{
    bool ok = true;
    for (uint32_t b = 0; b < 64u * W; ++b) {
        const bool got = (words[b >> 6] >> (b & 63u)) & 1u;
        ok = ok && got == (b < want.size() ? (bool)want[b] : false);
    }
    expect(ok, what, bl, i);
}

void run(uint32_t bl, std::mt19937_64& rng, size_t n)
{
    const uint32_t n_ids = 8 * bl - 1, W = vgh::words_of(bl);      // ids 0 .. 8 bl - 2; the last bit is no haplotype
    std::vector<uint16_t> must = {0, 63, 64, 127, 128, (uint16_t)(n_ids - 1)};
    must.erase(std::remove_if(must.begin(), must.end(), [&](uint16_t h) { return h >= n_ids; }), must.end());
    std::sort(must.begin(), must.end());
    must.erase(std::unique(must.begin(), must.end()), must.end());
    for (size_t i = 0; i < n; ++i) {
        // a `used` list of 1 .. 64 distinct ids, ascending; every other case holds the ids around the word boundaries
        std::vector<uint16_t> ids(n_ids);
        for (uint32_t h = 0; h < n_ids; ++h) ids[h] = (uint16_t)h;
        std::shuffle(ids.begin(), ids.end(), rng);
        const size_t n_used = 1 + rng() % std::min<size_t>(64, n_ids);
        std::vector<uint16_t> used(ids.begin(), ids.begin() + (ptrdiff_t)n_used);
        if (i % 2 == 0) {
            for (size_t q = 0; q < must.size() && q < used.size(); ++q)
                if (std::find(used.begin(), used.end(), must[q]) == used.end()) used[q] = must[q];
            std::sort(used.begin(), used.end());
            used.erase(std::unique(used.begin(), used.end()), used.end());
        }
        std::sort(used.begin(), used.end());
        // every place, no place, one place, a random set -- and bits beyond the list, which name nothing
        uint64_t places = i % 5 == 0 ? ~0ull : i % 5 == 1 ? 0ull : i % 5 == 2 ? 1ull << (rng() % used.size()) : rng();
        if (i % 5 != 0 && i % 3 == 0 && used.size() < 64) places |= 1ull << used.size();
        std::vector<bool> want(n_ids, false);
        for (size_t p = 0; p < used.size(); ++p)
            if ((places >> p) & 1u) want[used[p]] = true;
        std::unique_ptr<uint64_t[]> words(new uint64_t[W]());      // exactly W words
        vgh::places_to_ids(places, used.data(), used.size(), words.get());
        same(words.get(), W, want, "places_to_ids", bl, i);
        // a second row's places or-ed into the same words, as gt0 and a fix are built
        const uint64_t more = rng();
        for (size_t p = 0; p < used.size(); ++p)
            if ((more >> p) & 1u) want[used[p]] = true;
        vgh::places_to_ids(more, used.data(), used.size(), words.get());
        same(words.get(), W, want, "places_to_ids (or-ed)", bl, i);
    }
    // the ids on both sides of the word boundaries and the last haplotype, one at a time, each at the place it has in a list of all of them
    for (size_t q = 0; q < must.size(); ++q) {
        std::unique_ptr<uint64_t[]> words(new uint64_t[W]());
        std::vector<bool> want(n_ids, false);
        want[must[q]] = true;
        vgh::places_to_ids(1ull << q, must.data(), must.size(), words.get());
        same(words.get(), W, want, "places_to_ids (one id)", bl, q);
    }
}
}  // namespace

int main()
{
    std::mt19937_64 rng(20251019);
    for (uint32_t bl : {7u, 8u, 9u, 16u, 17u, 32u}) run(bl, rng, 2000);
    // the samples that take the device path: 7 to 32 bytes, ploidy 3 to 8, at most 64 places
    struct { uint64_t bl; uint32_t p; uint64_t n; bool want; } const cases[] = {
        {7, 4, 5, true},  {7, 4, 15, true}, {7, 4, 16, true},  {7, 4, 17, false}, {7, 6, 15, false}, {7, 6, 10, true}, {7, 8, 8, true}, {7, 8, 9, false},
        {7, 3, 21, true}, {7, 3, 22, false}, {7, 2, 5, false}, {7, 9, 1, false},  {6, 4, 5, false},  {32, 4, 5, true}, {33, 4, 5, false}, {9, 4, 0, false}};
    size_t i = 0;
    for (const auto& c : cases) expect(vgh::wide_ploidy_sample(c.bl, c.p, c.n) == c.want, "wide_ploidy_sample", (uint32_t)c.bl, i++);
    if (failures) {
        std::fprintf(stderr, "%zu mismatches\n", failures);
        return 1;
    }
    std::printf("id masks identical: 6 widths x 2000 lists, %zu bounds\n", i);
    return 0;
}
