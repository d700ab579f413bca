// subsample_check.cpp -- vgh::subsample_keep and the threshold (csrc/vgmi_subsample.h) against the known answers of the option's
// definition.  A stand-alone program, built with -fsanitize=address,undefined by tests/test_subsample_cpu.py: the arithmetic is mod 2^64
// on unsigned words, so read number 2^64 - 2 must go through without a report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "vgmi_subsample.h"

static int fails = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            ++fails;                                                   \
        }                                                              \
    } while (0)

int main()
{
    const uint64_t top = std::numeric_limits<uint64_t>::max();
    const uint64_t seeds[3] = {11, 0, top};
    const uint64_t numbers[5] = {0, 1, 2, 1ull << 32, top - 1};
    const uint64_t want[5][3] = {
        {0x50f5647d2380309dull, 0xe220a8397b1dcdafull, 0xe4d971771b652c20ull},
        {0x432a5cd27a6b13a1ull, 0x6e789e6aa1b965f4ull, 0xe99ff867dbf682c9ull},
        {0xa356be306e9b126dull, 0x06c45d188009454full, 0x382ff84cb27281e9ull},
        {0x6f1848d17c7a49caull, 0x46093cf9861ec2e4ull, 0xc5aa1d1d7e827744ull},
        {0x64edd2139b64e0d6ull, 0x336503c6b835bec0ull, 0xde0a564cbcd060c4ull},
    };
    for (int i = 0; i < 5; ++i)
        for (int s = 0; s < 3; ++s) {
            const uint64_t z = vgh::subsample_hash(numbers[i], seeds[s]);
            CHECK(z == want[i][s]);
            // keep is z < T: on both sides of the value itself
            CHECK(!vgh::subsample_keep(numbers[i], seeds[s], z));
            CHECK(vgh::subsample_keep(numbers[i], seeds[s], z + 1));
            CHECK(!vgh::subsample_keep(numbers[i], seeds[s], 0));
        }

    CHECK(vgh::subsample_threshold(0.5) == 0x8000000000000000ull);
    CHECK(vgh::subsample_threshold(0.02) == 0x051eb851eb851ec0ull);
    CHECK(vgh::subsample_threshold(0.9) == 0xe666666666666800ull);
    // the edge thresholds: F = 2^-64 gives T = 1, anything smaller T = 0, which keeps nothing
    CHECK(vgh::subsample_threshold(std::ldexp(1.0, -64)) == 1);
    CHECK(vgh::subsample_threshold(std::ldexp(1.0, -65)) == 0);
    CHECK(vgh::subsample_threshold(std::ldexp(3.0, -64)) == 3);
    CHECK(vgh::subsample_threshold(std::nextafter(1.0, 0.0)) == top - 2047);      // the largest fraction below 1: 2^64 - 2^11

    // the first 4 000 reads at seed 11: kept, the first kept ones, the longest run of dropped reads
    struct Row {
        double f;
        unsigned kept, longest;
        unsigned first[6];
        unsigned n_first;
    };
    const Row rows[3] = {{0.5, 2017, 15, {0, 1, 4, 6, 8, 10}, 6}, {0.02, 70, 274, {41, 69, 123}, 3}, {0.9, 3611, 3, {}, 0}};
    for (const Row& r : rows) {
        const vgh::SubsampleRule rule(r.f, 11);
        CHECK(rule.on && rule.threshold == vgh::subsample_threshold(r.f));
        unsigned kept = 0, run = 0, longest = 0, n_first = 0;
        for (uint64_t i = 0; i < 4000; ++i) {
            const bool k = rule.keep(i);
            CHECK(k == vgh::subsample_keep(i, 11, rule.threshold));
            if (k) {
                if (n_first < r.n_first) CHECK(i == r.first[n_first++]);
                ++kept;
                run = 0;
            } else if (++run > longest) {
                longest = run;
            }
        }
        CHECK(kept == r.kept);
        CHECK(longest == r.longest);
    }

    // F = 1 is off and keeps everything, whatever the seed; T = 0 keeps nothing; T = 1 keeps a read only where z is 0
    for (int s = 0; s < 3; ++s) {
        const vgh::SubsampleRule off(1.0, seeds[s]), none(std::ldexp(1.0, -65), seeds[s]), one(std::ldexp(1.0, -64), seeds[s]);
        CHECK(!off.on && none.on && one.on && none.threshold == 0 && one.threshold == 1);
        for (uint64_t i = 0; i < 100000; ++i) {
            CHECK(off.keep(i));
            CHECK(!none.keep(i));
            CHECK(one.keep(i) == (vgh::subsample_hash(i, seeds[s]) == 0));
        }
        for (int i = 0; i < 5; ++i) {
            CHECK(off.keep(numbers[i]));
            CHECK(!none.keep(numbers[i]));
        }
        CHECK(off.keep(top) && !none.keep(top));      // (i + 1 wraps to 0: x = S)
    }

    CHECK(vgh::subsample_fraction_valid(1.0) && vgh::subsample_fraction_valid(std::ldexp(1.0, -70)) && vgh::subsample_fraction_valid(0.5));
    CHECK(!vgh::subsample_fraction_valid(0.0) && !vgh::subsample_fraction_valid(-0.5) && !vgh::subsample_fraction_valid(std::nextafter(1.0, 2.0)));
    CHECK(!vgh::subsample_fraction_valid(std::nan("")) && !vgh::subsample_fraction_valid(INFINITY));

    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("subsample rule identical to its known answers\n");
    return 0;
}
