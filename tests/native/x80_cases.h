// x80_cases.h -- the operands csrc/vg_x80.h is held against the x87 unit on, for x80_check.cpp (host, g++) and x80_device_check.hip
// (the same header compiled for the device).  Two sets:
//
//   X80Gen            the seeded random generator: significands of all ones / single bits / short patterns / anything, exponents at the
//                     underflow boundary, among probabilities and anywhere; pair() places the second operand of a sum at every
//                     alignment distance, triple() places r of  r + s * o  around the product.
//   x80_structured_*  the cross product of edge significands with edge placements -- what a random draw reaches with a chance
//                     of 2^-64 or never: ties on an even and on an odd significand, all ones carrying into the next binade, every
//                     alignment distance 0 .. 130 in both orders, exponent fields 0 / 1 / 2 / 64, denormals of 1 / 32 / 63 significant
//                     bits, zeros, products and quotients on either side of the underflow border, and for  r + s * o  the product
//                     normal / denormal / flushed to zero with r at -66 .. +66 binades around it.
//
// Nothing here computes with vg_x80.h: only its VgX80 (significand, exponent field) carries the operands.
// Test infrastructure (tests/test_x80_cpu.py, tests/test_x80_cases_cpu.py, tests/test_gpu_x80.py).
#ifndef X80_CASES_H
#define X80_CASES_H
#include <cstdint>
#include <random>
#include <vector>

#include "vg_x80.h"

struct X80Gen {
    std::mt19937_64 rng;
    explicit X80Gen(uint64_t seed = 12345) : rng(seed) {}

    uint64_t significand()
    {
        switch (rng() % 8) {
            case 0: return ~0ULL;
            case 1: return 1ULL << 63;
            case 2: return (1ULL << 63) | 1u;
            case 3: return (1ULL << 63) | (rng() & 0xFFFF);
            case 4: return ~(rng() & 0xFFFF);
            case 5: return (1ULL << 63) | (1ULL << (rng() % 63));
            default: return rng() | (1ULL << 63);
        }
    }

    uint64_t denormal_significand()
    {
        const uint64_t m = significand();
        return m >> (1 + rng() % 63);
    }

    VgX80 value()
    {
        VgX80 v;
        const unsigned kind = (unsigned)(rng() % 16);
        if (kind == 0) {
            v.m = 0;
            v.e = 0;
        } else if (kind == 1) {                       // denormal
            v.e = 0;
            v.m = denormal_significand();
            if (v.m == 0) v.m = 1;
        } else if (kind < 5) {                        // close to the underflow boundary
            v.e = 1 + (uint32_t)(rng() % 140);
            v.m = significand();
        } else if (kind < 8) {                        // products of these land around the boundary
            v.e = 8100 + (uint32_t)(rng() % 300);
            v.m = significand();
        } else if (kind < 12) {                       // probabilities
            v.e = VG_X80_BIAS - (uint32_t)(rng() % 200);
            v.m = significand();
        } else {                                      // anything below 2^8
            v.e = 1 + (uint32_t)(rng() % (VG_X80_BIAS + 8));
            v.m = significand();
        }
        return v;
    }

    // the operands of a product, a sum and a quotient; one time in three the second lies within 70 binades of the first (every
    // alignment distance of a sum)
    void pair(VgX80& a, VgX80& b)
    {
        a = value();
        b = value();
        if (rng() % 3 == 0 && a.e > 80 && b.e) b.e = a.e - 70 + (uint32_t)(rng() % 140);
    }

    // r + s * o  with r placed around the product (every alignment distance, both orders) three times in four, anywhere otherwise;
    // false: the product could overflow, no case
    bool triple(VgX80& r, VgX80& s, VgX80& o)
    {
        s = value();
        o = value();
        if ((int)s.e + (int)o.e > 2 * VG_X80_BIAS - 100) return false;
        r = value();
        if (rng() % 4 && s.m && o.m) {
            const int pe = (int)(s.e ? s.e : 1) + (int)(o.e ? o.e : 1) - VG_X80_BIAS + (int)(rng() % 140) - 70;
            r.e = pe < 1 ? 0 : (uint32_t)pe;
            r.m = r.e ? significand() : denormal_significand();
        }
        return true;
    }
};

struct X80Pair {
    VgX80 a, b;
};
struct X80Triple {
    VgX80 r, s, o;      // r + s * o
};

// ---- the structured set ---------------------------------------------------------------------------------------------------------
// x = X * 2^32 (32 bits, the low word empty) and a 64-bit y whose 128-bit product ends in EXACTLY half an ulp of its upper 64 bits:
// the product in [2^127, 2^128) (`up`: the low 64 bits are 2^63) or in [2^126, 2^127) (the low 63 bits are 2^62), the kept half odd
// or even.  Found by a deterministic search: X odd, y's low word solves  X * L = 2^31  (mod 2^32) resp.  2^30  (mod 2^31), and every
// candidate is checked on the 128-bit product itself.
static inline void x80_tie_product(bool up, bool odd, uint64_t& x, uint64_t& y)
{
    for (uint64_t i = 1;; ++i) {
        const uint64_t X = 0x80000001ull | ((i * 0x9E3779B1ull) & 0x7FFFFFFEull);
        const uint64_t H = 0x80000000ull | ((i * 0x85EBCA6Bull) & 0x7FFFFFFFull);
        uint64_t inv = X;                                         // X^-1 mod 2^32 (Newton: three bits, then doubling)
        for (int k = 0; k < 5; ++k) inv *= 2 - X * inv;
        const uint64_t t = up ? 0x80000000ull : 0x40000000ull + ((i & 1u) << 31);
        const uint64_t L = (inv * t) & 0xFFFFFFFFull;
        x = X << 32;
        y = (H << 32) | L;
        const unsigned __int128 p = (unsigned __int128)x * y;
        const bool p_up = (uint64_t)(p >> 127) != 0;
        const uint64_t low = (uint64_t)p;
        const bool half = p_up ? low == (1ULL << 63) : (low & ~(1ULL << 63)) == (1ULL << 62);
        const bool p_odd = p_up ? ((uint64_t)(p >> 64) & 1u) != 0 : (low >> 63) != 0;
        if (p_up == up && half && p_odd == odd) return;
    }
}

static inline std::vector<uint64_t> x80_edge_significands()
{
    std::vector<uint64_t> s = {1ULL << 63, (1ULL << 63) | 1u, ~0ULL, ~0ULL - 1u};
    for (unsigned k : {1u, 2u, 31u, 32u, 33u, 61u, 62u}) s.push_back((1ULL << 63) | (1ULL << k));     // single low bits
    for (int up = 0; up < 2; ++up)
        for (int odd = 0; odd < 2; ++odd) {
            uint64_t x, y;
            x80_tie_product(up != 0, odd != 0, x, y);
            s.push_back(x);
            s.push_back(y);
        }
    return s;
}

// the fewer significands o and r of  r + s * o  take (the cross product is cubic): o keeps the second factor of every tie
static inline std::vector<uint64_t> x80_edge_significands_o()
{
    std::vector<uint64_t> s = {1ULL << 63, (1ULL << 63) | 1u, ~0ULL, ~0ULL - 1u};
    for (int up = 0; up < 2; ++up)
        for (int odd = 0; odd < 2; ++odd) {
            uint64_t x, y;
            x80_tie_product(up != 0, odd != 0, x, y);
            s.push_back(y);
        }
    return s;
}
static inline std::vector<uint64_t> x80_edge_significands_r() { return {1ULL << 63, (1ULL << 63) | 1u, ~0ULL, (1ULL << 63) | (1ULL << 62)}; }

// significand m (bit 63 set) at exponent e of its leading bit, which may lie below 1: the stored value then is a denormal that keeps
// what fits (and zero when nothing does)
static inline VgX80 x80_at(uint64_t m, int e)
{
    VgX80 v;
    if (e >= 1) {
        v.m = m;
        v.e = (uint32_t)e;
    } else {
        v.e = 0;
        v.m = 1 - e >= 64 ? 0 : m >> (1 - e);
    }
    return v;
}

static inline void x80_structured_pairs(std::vector<X80Pair>& out)
{
    const std::vector<uint64_t> sig = x80_edge_significands();
    const int B = VG_X80_BIAS;
    std::vector<std::pair<int, int>> place;                       // exponents of the two leading bits
    for (int d = 0; d <= 130; ++d) {                              // every alignment distance of a sum, both orders
        place.push_back({B, B - d});
        place.push_back({B - d, B});
    }
    for (int d : {0, 1, 2, 62, 63, 64, 65, 66, 127, 128, 129}) {  // ... and with the smaller operand a denormal, the larger near it
        place.push_back({1 + d, 0});
        place.push_back({0, 1 + d});
        place.push_back({1 + d, -31});
        place.push_back({-62, 1 + d});
    }
    for (int ea : {-62, -31, 0, 1, 2, 64})                        // fields 0 (1, 32 and 63 significant bits), 1, 2, 64 on either side
        for (int eb : {-62, -31, 0, 1, 2, 64}) place.push_back({ea, eb});
    for (int t = -70; t <= 4; ++t) {                              // products on either side of the underflow border
        place.push_back({8191, 8192 + t});
        place.push_back({B + t, -10});                            // ... of a denormal and a normal operand
    }
    for (int t = -70; t <= 4; ++t) {                              // quotients on either side of it
        place.push_back({100, B + 100 - t});
        place.push_back({-20, B - 20 - t});
    }
    for (int ea : {0, 1, 2, 64})                                  // quotients of operands at the border themselves
        for (int eb : {-62, 0, 1, 2, 64}) place.push_back({ea + 30, eb + 30});
    for (uint64_t ma : sig)
        for (uint64_t mb : sig)
            for (const auto& p : place) out.push_back({x80_at(ma, p.first), x80_at(mb, p.second)});
    const VgX80 zero = {0, 0};
    out.push_back({zero, zero});
    for (uint64_t m : sig)
        for (int e : {-62, -31, 0, 1, 2, 64, B}) {
            out.push_back({x80_at(m, e), zero});
            out.push_back({zero, x80_at(m, e)});
        }
}

static inline void x80_structured_triples(std::vector<X80Triple>& out)
{
    const std::vector<uint64_t> sig = x80_edge_significands(), sig_o = x80_edge_significands_o(), sig_r = x80_edge_significands_r();
    const int B = VG_X80_BIAS;
    // (exponent of s, exponent of o): the product a normal number, a denormal with 31 / 2 / 1 bits, on the rounding border of the
    // smallest denormal (-63: up to it, -64: a tie with zero or just above one), flushed to zero
    const std::pair<int, int> products[] = {{B, B - 100}, {8191, 8192 - 33}, {8191, 8192 - 62}, {8191, 8192 - 63}, {8191, 8192 - 64},
                                            {8191, 8192 - 80}, {B - 40, -10}};
    for (uint64_t ms : sig)
        for (uint64_t mo : sig_o)
            for (const auto& p : products) {
                const int pe = p.first + p.second - B;      // the product's exponent, or one above
                for (uint64_t mr : sig_r)
                    for (int d = -66; d <= 66; ++d) out.push_back({x80_at(mr, pe + d), x80_at(ms, p.first), x80_at(mo, p.second)});
            }
    const VgX80 zero = {0, 0};
    for (uint64_t ms : sig)
        for (uint64_t mo : sig)
            for (int e : {-62, 0, 1, 64, B}) {
                out.push_back({zero, x80_at(ms, e), x80_at(mo, B - 1)});
                out.push_back({x80_at(mo, e), zero, x80_at(ms, B)});
                out.push_back({x80_at(mo, e), x80_at(ms, B), zero});
                out.push_back({zero, zero, x80_at(ms, e)});
            }
    out.push_back({zero, zero, zero});
}

// ---- named cases: operands that once exposed a fault stay here, by name ------------------------------------------------------------
// (none so far: no class of tests/native/x80_device_check.hip has found a difference between vg_x80.h and the x87 unit)

#endif
