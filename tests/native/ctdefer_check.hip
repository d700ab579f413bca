// ctdefer_check -- test driver for the two kernels behind the context-table count kernels' row loop (varigraph_amd/csrc/vgmi_ctdefer.hip).
// Compiled together with that one source file and nothing else of the library; it holds no kernel of its own.
//
//   ctdefer_check geometry <n_cu> <n_counts> <n_bytes> [<n_cu> <n_counts> <n_bytes> ...]
//       no HIP call: what ctd_scratch_bytes / ctd_layout make of every triple, one JSON object a line.
//   ctdefer_check apply <case>
//       on the GPU: seeded records into a scratch laid out by ctd_scratch_bytes / ctd_layout, launch_ctd_apply, every counter against
//       a plain 64-bit loop on the host.  A record {x, y} with m = y & 0xFFF adds one to counter x + j (bit 12 of y set) or x - j (clear)
//       for every set bit j of m; records at or beyond min(cursor, cap) do not exist.  One JSON object a launch; exit status 1 on
//       any difference (the first differing counter is printed: index, region, got, want), 2 on a HIP error or a case that did
//       not reach what it is for.
#include <hip/hip_runtime.h>
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "vgmi_kernels.h"

using namespace vgk;

#define CHECK(x)                                                                                          \
    do {                                                                                                  \
        const hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) {                                                                           \
            fprintf(stderr, "ctdefer_check: %s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);    \
            exit(2);                                                                                      \
        }                                                                                                 \
    } while (0)

static const uint32_t GUARD = 64;      // words behind the counters that no launch may touch

struct Rng {      // splitmix64
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next()
    {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint64_t below(uint64_t n) { return next() % n; }
};

static uint32_t top_bit(uint32_t m) { return 31u - (uint32_t)__builtin_clz(m); }

// a record whose LOWEST counter is `lo` (0 <= lo < n): the mask is cut to the counters the table has from there on
static uint2 record_at(uint64_t n, uint64_t lo, uint32_t m, bool up)
{
    const uint64_t avail = n - lo;
    if (avail < 12) m &= (1u << avail) - 1u;
    m |= 1u;
    if (up) return make_uint2((uint32_t)lo, m | 0x1000u);      // bit 0 set: the lowest counter is x
    return make_uint2((uint32_t)(lo + top_bit(m)), m);         // x - top_bit is the lowest, x (bit 0) the highest
}

// uniform over the table: both directions, masks uniform in 0 .. 0xFFF (1 / 4096 null), 0xFFF forced on 1 %, every touched counter inside [0, n)
static void gen_uniform(std::vector<uint2>& out, Rng& r, uint64_t n, size_t count, uint64_t first = 0, uint64_t span = 0)
{
    if (!span) span = n;
    for (size_t i = 0; i < count; ++i) {
        const uint64_t v = r.next();
        uint32_t m = (uint32_t)(v & 0xFFFu);
        const bool up = (v >> 12) & 1u;
        if ((v >> 13) % 100 == 0) m = 0xFFFu;
        const uint32_t h = m ? top_bit(m) : 0u;
        const uint64_t lo_x = up ? first : std::max<uint64_t>(first, h), hi_x = std::min<uint64_t>(first + span, n) - (up ? h : 0);      // x in [lo_x, hi_x)
        const uint64_t x = lo_x + r.below(hi_x - lo_x);
        out.push_back(make_uint2((uint32_t)x, m | (up ? 0x1000u : 0u)));
    }
}

// the boundary set: lowest counter in [b * region - 12, b * region + 1] for the given regions b (b == n_bins: the end of the table, the
// last counter included), both directions
static void gen_boundary(std::vector<uint2>& out, Rng& r, const CtDefer& d, const std::vector<uint32_t>& regions, size_t count)
{
    const uint64_t n = d.n_counts;
    for (size_t i = 0; i < count; ++i) {
        const uint32_t b = regions[i % regions.size()];
        const uint64_t v = r.next();
        const uint64_t edge = std::min<uint64_t>((uint64_t)b * d.region, n);
        int64_t lo = (int64_t)edge - 12 + (int64_t)((v >> 16) % 14);
        if (lo < 0) lo = (int64_t)((v >> 16) % 2);
        if (lo >= (int64_t)n) lo = (int64_t)n - 1;
        if (b == d.n_bins && (i / regions.size()) % 4 == 0) lo = (int64_t)n - 1;      // counter n_counts - 1 by itself
        uint32_t m = (uint32_t)(v & 0xFFFu);
        if ((v >> 40) % 8 == 0) m = 0xFFFu;
        out.push_back(record_at(n, (uint64_t)lo, m, (v >> 12) & 1u));
    }
}

static void shuffle(std::vector<uint2>& v, Rng& r)
{
    for (size_t i = v.size(); i > 1; --i) std::swap(v[i - 1], v[r.below(i)]);
}

struct Rig {
    CtDefer d{};
    uint32_t n_cu = 0;
    size_t bytes = 0;
    uint8_t* scratch = nullptr;
    uint32_t* counts = nullptr;      // n_counts + GUARD
    std::vector<uint64_t> want;      // the same on the host
    std::vector<uint32_t> got;
    int launches = 0;
};

static void rig_make(Rig& g, const char* name, uint64_t n_counts, uint64_t n_bytes, uint64_t seed)
{
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    g.n_cu = (uint32_t)prop.multiProcessorCount;
    g.bytes = ctd_scratch_bytes(n_bytes, n_counts, g.n_cu, &g.d);
    if (!g.bytes) {
        fprintf(stderr, "ctdefer_check: %s: ctd_scratch_bytes does not serve %" PRIu64 " counters on %u CUs\n", name, n_counts, g.n_cu);
        exit(2);
    }
    CHECK(hipMalloc(reinterpret_cast<void**>(&g.scratch), g.bytes));
    CHECK(hipMemset(g.scratch, 0xFF, g.bytes));      // whatever a launch reads without having written it is as wrong as it can be
    ctd_layout(g.scratch, &g.d);
    CHECK(hipMalloc(reinterpret_cast<void**>(&g.counts), (n_counts + GUARD) * 4));
    // seeded non-zero start values: a store in place of an add shows
    Rng r(seed ^ 0xC0FFEEull);
    g.want.resize(n_counts + GUARD);
    g.got.resize(n_counts + GUARD);
    for (size_t i = 0; i < g.want.size(); ++i) g.got[i] = 1u + (uint32_t)(r.next() & 0xFFFFu), g.want[i] = g.got[i];
    CHECK(hipMemcpy(g.counts, g.got.data(), g.got.size() * 4, hipMemcpyHostToDevice));
}

static void rig_free(Rig& g)
{
    CHECK(hipFree(g.scratch));
    CHECK(hipFree(g.counts));
}

// one launch: `recs` into d.rec (as many as it holds), the cursor set, launch_ctd_apply, every counter compared.  Returns the number of differences.
static uint64_t rig_apply(Rig& g, const char* name, const std::vector<uint2>& recs, uint64_t cursor, bool want_overflowing_room = false)
{
    const CtDefer& d = g.d;
    const size_t n_up = std::min<size_t>(recs.size(), d.cap);
    if (cursor > 0xFFFFFFFFull) exit(2);
    CHECK(launch_ctd_reset(d, nullptr));
    if (n_up) CHECK(hipMemcpy(d.rec, recs.data(), n_up * sizeof(uint2), hipMemcpyHostToDevice));
    const uint32_t cur = (uint32_t)cursor;
    CHECK(hipMemcpy(d.cursor, &cur, 4, hipMemcpyHostToDevice));
    XTableView xt{};
    xt.counts = g.counts;
    CHECK(launch_ctd_apply(xt, d, g.n_cu, nullptr));
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(g.got.data(), g.counts, g.got.size() * 4, hipMemcpyDeviceToHost));
    // the reference: a plain loop
    const uint64_t n_applied = std::min<uint64_t>(cursor, d.cap);
    if (n_applied > n_up) {
        fprintf(stderr, "ctdefer_check: %s: cursor %" PRIu64 " beyond the %zu records written\n", name, cursor, n_up);
        exit(2);
    }
    uint64_t increments = 0;
    for (uint64_t i = 0; i < n_applied; ++i) {
        const uint2 rc = recs[i];
        const bool up = rc.y & 0x1000u;
        for (uint32_t m = rc.y & 0xFFFu; m; m &= m - 1u) {
            const uint32_t j = (uint32_t)__builtin_ctz(m);
            const int64_t at = up ? (int64_t)rc.x + j : (int64_t)rc.x - j;
            if (at < 0 || at >= (int64_t)d.n_counts) {
                fprintf(stderr, "ctdefer_check: %s: the generator left the table (record %" PRIu64 ")\n", name, i);
                exit(2);
            }
            ++g.want[at];
            ++increments;
        }
    }
    uint64_t bad = 0, first = 0;
    for (size_t i = 0; i < g.want.size(); ++i)
        if ((uint64_t)g.got[i] != g.want[i] && !bad++) first = i;
    // the rooms: how full the fullest is
    std::vector<uint32_t> bc((size_t)d.n_bins * d.n_wg);
    CHECK(hipMemcpy(bc.data(), d.bin_cursor, bc.size() * 4, hipMemcpyDeviceToHost));
    uint64_t over = 0, in_rooms = 0;
    uint32_t fullest = 0;
    for (uint32_t v : bc) {
        over += v > d.room;
        in_rooms += v;
        fullest = std::max(fullest, v);
    }
    printf("{\"case\": \"%s\", \"launch\": %d, \"n_cu\": %u, \"n_counts\": %" PRIu64 ", \"n_bins\": %u, \"region\": %u, \"room\": %u, \"cap\": %u, \"n_wg\": %u, "
           "\"scratch_bytes\": %zu, \"records\": %zu, \"cursor\": %" PRIu64 ", \"applied\": %" PRIu64 ", \"increments\": %" PRIu64
           ", \"records_binned\": %" PRIu64 ", \"rooms_overflowed\": %" PRIu64 ", \"fullest_room\": %u, \"differences\": %" PRIu64,
           name, g.launches++, g.n_cu, d.n_counts, d.n_bins, d.region, d.room, d.cap, d.n_wg, g.bytes, recs.size(), cursor, n_applied, increments, in_rooms, over,
           fullest, bad);
    if (bad)
        printf(", \"first\": {\"index\": %" PRIu64 ", \"region\": %" PRIu64 ", \"got\": %u, \"want\": %" PRIu64 ", \"guard\": %s}", first, first / d.region, g.got[first],
               g.want[first], first >= d.n_counts ? "true" : "false");
    printf("}\n");
    fflush(stdout);
    if (!bad && want_overflowing_room && !over) {
        fprintf(stderr, "ctdefer_check: %s: no room overflowed (fullest %u of %u): the case does not reach what it is for\n", name, fullest, d.room);
        exit(2);
    }
    // (the next launch of a case goes on from what the device holds)
    if (bad) for (size_t i = 0; i < g.want.size(); ++i) g.want[i] = g.got[i];
    return bad;
}

static std::vector<uint32_t> all_regions(const CtDefer& d)
{
    std::vector<uint32_t> v;
    for (uint32_t b = 0; b <= d.n_bins; ++b) v.push_back(b);
    return v;
}

static void expect(const char* name, bool ok, const char* what)
{
    if (ok) return;
    fprintf(stderr, "ctdefer_check: %s: %s\n", name, what);
    exit(2);
}

static int run_apply(const std::string& c)
{
    const char* const name = c.c_str();
    uint64_t bad = 0;
    Rig g;
    std::vector<uint2> recs;
    if (c == "uniform-32768") {      // the offset field of a binned record full, one region a workgroup (at 256 CUs)
        Rng r(1);
        rig_make(g, name, 8388608, 16ull * 3000000, 1);
        gen_uniform(recs, r, g.d.n_counts, 3000000);
        bad += rig_apply(g, name, recs, recs.size());
    } else if (c == "two-rounds") {      // more regions than workgroups of the accumulate kernel, an odd region size, runs that straddle regions, the last region's guard
        Rng r(2);
        rig_make(g, name, 8388609, 16ull * 3000000, 2);
        gen_uniform(recs, r, g.d.n_counts, 1500000);
        gen_boundary(recs, r, g.d, all_regions(g.d), 1500000);
        shuffle(recs, r);
        bad += rig_apply(g, name, recs, recs.size());
    } else if (c == "max-table") {      // the largest table served: CTD_MAX_BINS regions of 32 768
        Rng r(3);
        rig_make(g, name, 67108864, 600000000ull, 3);
        expect(name, g.d.n_bins == CTD_MAX_BINS && g.d.region == 32768, "not 2 048 regions of 32 768");
        gen_uniform(recs, r, g.d.n_counts, 4000000);
        std::vector<uint32_t> regions;
        for (uint32_t i = 0; i < 8; ++i) regions.push_back(i), regions.push_back(g.d.n_bins / 2 - 4 + i), regions.push_back(g.d.n_bins - 7 + i);
        gen_boundary(recs, r, g.d, regions, 200000);
        shuffle(recs, r);
        bad += rig_apply(g, name, recs, recs.size());
    } else if (c == "tiny") {      // the 256-counter clamp, fewer regions than CUs
        for (uint64_t n : {300ull, 5000ull}) {
            Rng r(4 + n);
            Rig t;
            rig_make(t, name, n, 16ull * 200000, 4 + n);
            expect(name, t.d.region == 256, "region is not 256");
            recs.clear();
            gen_uniform(recs, r, n, 150000);
            gen_boundary(recs, r, t.d, all_regions(t.d), 50000);
            shuffle(recs, r);
            bad += rig_apply(t, name, recs, recs.size());
            rig_free(t);
        }
        return bad ? 1 : 0;
    } else if (c == "pile-up") {      // a sample whose reads pile onto one region: rooms overflow, the rest is counted where it is met
        Rng r(5);
        rig_make(g, name, 8388608, 16ull * 2100000, 5);
        expect(name, g.d.cap >= 2100000, "cap does not hold all records");
        const uint32_t b = g.d.n_bins / 3;
        gen_uniform(recs, r, g.d.n_counts, 2000000, (uint64_t)b * g.d.region + 11, g.d.region - 22);
        gen_uniform(recs, r, g.d.n_counts, 100000);      // elsewhere
        shuffle(recs, r);
        bad += rig_apply(g, name, recs, recs.size(), true);
    } else if (c == "rooms-of-8") {      // nearly everything through ctd_count_direct
        setenv("VGMI_CT_DEFER_ROOM", "7", 1);
        Rng r(6);
        rig_make(g, name, 1800000, 16ull * 1000000, 6);
        expect(name, g.d.room == 8, "room is not 8");
        gen_uniform(recs, r, g.d.n_counts, 900000);
        gen_boundary(recs, r, g.d, all_regions(g.d), 100000);
        shuffle(recs, r);
        bad += rig_apply(g, name, recs, recs.size(), true);
    } else if (c == "cursor") {      // min(cursor, cap), a single chunk, an empty launch
        setenv("VGMI_CT_DEFER_CAP", "40000", 1);
        Rng r(7);
        rig_make(g, name, 1800000, 16ull * 1000000, 7);
        expect(name, g.d.cap == 40448, "cap is not 40 448");
        gen_uniform(recs, r, g.d.n_counts, g.d.cap);
        for (uint64_t cur : {(uint64_t)0, (uint64_t)256, (uint64_t)g.d.cap, (uint64_t)g.d.cap + 768}) bad += rig_apply(g, name, recs, cur);
    } else if (c == "reuse") {      // a second launch on the same scratch with fewer records: what the first left in the rooms must not count
        Rng r(8);
        rig_make(g, name, 8388609, 16ull * 3000000, 8);
        gen_uniform(recs, r, g.d.n_counts, 2000000);
        gen_boundary(recs, r, g.d, all_regions(g.d), 1000000);
        shuffle(recs, r);
        bad += rig_apply(g, name, recs, recs.size());
        recs.clear();
        gen_uniform(recs, r, g.d.n_counts, 40000);
        gen_boundary(recs, r, g.d, all_regions(g.d), 10000);
        shuffle(recs, r);
        bad += rig_apply(g, name, recs, recs.size());
    } else {
        fprintf(stderr, "ctdefer_check: unknown case %s\n", name);
        return 2;
    }
    rig_free(g);
    return bad ? 1 : 0;
}

static int run_geometry(int argc, char** argv)
{
    if (argc < 3 || argc % 3) return 2;
    for (int i = 0; i + 2 < argc; i += 3) {
        const uint32_t n_cu = (uint32_t)strtoul(argv[i], nullptr, 10);
        const uint64_t n_counts = strtoull(argv[i + 1], nullptr, 10), n_bytes = strtoull(argv[i + 2], nullptr, 10);
        CtDefer d{};
        const size_t bytes = ctd_scratch_bytes(n_bytes, n_counts, n_cu, &d);
        if (!bytes) {
            printf("{\"n_cu\": %u, \"n_counts\": %" PRIu64 ", \"n_bytes\": %" PRIu64 ", \"bytes\": 0}\n", n_cu, n_counts, n_bytes);
            continue;
        }
        uint8_t* const base = reinterpret_cast<uint8_t*>((uintptr_t)1 << 32);      // (an address to lay out from: nothing is touched)
        ctd_layout(base, &d);
        const uint64_t rooms = (uint64_t)d.n_bins * d.n_wg;
        printf("{\"n_cu\": %u, \"n_counts\": %" PRIu64 ", \"n_bytes\": %" PRIu64 ", \"bytes\": %zu, \"cap\": %u, \"n_bins\": %u, \"room\": %u, \"d_n_counts\": %" PRIu64
               ", \"region\": %u, \"inv\": %u, \"n_wg\": %u, \"cursor_at\": %td, \"bin_cursor_at\": %td, \"bin_cursor_end\": %" PRIu64 ", \"rec_at\": %td, \"rec_end\": %" PRIu64
               ", \"binned_at\": %td, \"binned_end\": %" PRIu64 "}\n",
               n_cu, n_counts, n_bytes, bytes, d.cap, d.n_bins, d.room, d.n_counts, d.region, d.inv, d.n_wg, reinterpret_cast<uint8_t*>(d.cursor) - base,
               reinterpret_cast<uint8_t*>(d.bin_cursor) - base, (uint64_t)(reinterpret_cast<uint8_t*>(d.bin_cursor) - base) + rooms * 4,
               reinterpret_cast<uint8_t*>(d.rec) - base, (uint64_t)(reinterpret_cast<uint8_t*>(d.rec) - base) + (uint64_t)d.cap * 8,
               reinterpret_cast<uint8_t*>(d.binned) - base, (uint64_t)(reinterpret_cast<uint8_t*>(d.binned) - base) + rooms * d.room * 4);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc >= 3 && !strcmp(argv[1], "geometry")) return run_geometry(argc - 2, argv + 2);
    if (argc == 3 && !strcmp(argv[1], "apply")) return run_apply(argv[2]);
    fprintf(stderr, "usage: ctdefer_check geometry <n_cu> <n_counts> <n_bytes> ... | apply <case>\n");
    return 2;
}
