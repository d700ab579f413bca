// x80_device_check -- csrc/vg_x80.h AS THE DEVICE RUNS IT against the x87 unit of the host.  The header takes other branches under
// __HIP_DEVICE_COMPILE__ (__umul64hi, __clzll) and goes through another back end there (selects, variable 64-bit shifts, masked shift
// counts; on wavefront-uniform operands the scalar unit's forms of them), so the host check (x80_check.cpp) says nothing about it.
//
//   x80_device_check [--host] [--divergent] [--uniform] [--chains] [<random cases per function>]
//
//   --host       no HIP call at all: the cases go through the host pass's compile of vg_x80.h (what tests/test_x80_cases_cpu.py drives)
//   --divergent  one case per lane: a wavefront holds fast-path and fallback lanes side by side
//   --uniform    one case per wavefront, its index made uniform with readfirstlane; all 64 lanes write the result and all 64 must be
//                the x87 value
//   --chains     r += s * o over 120 terms, one chain per lane, in the three forms the recursion has used (x80_add / x80_mul,
//                n80_add / n80_mul, n80_muladd)
//
// The cases are x80_cases.h's: the structured cross product, then seeded random ones.  Expected values are the x87 unit's (volatile
// long double).  Per function and mode one JSON line: cases, skipped (a division by zero or a quotient that overflows -- nothing else is),
// redrawn (random triples of  r + s * o  whose product could overflow, which the generator refuses: another is drawn in its place),
// mismatches, the first ten mismatching operand triples, and how many cases fell into each class.  The classes are counted on the host from
// the operands and the x87 results alone -- the unit's directed rounding modes bracket the exact value, unsigned __int128 arithmetic finds
// its lowest set bit, which decides a tie -- never with vg_x80.h, the code under test.  Exit status 1 on any mismatch, 2 on a HIP error.
// Test infrastructure (tests/x80_harness.py).
#include <hip/hip_runtime.h>
#include <fenv.h>
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "vg_x80.h"
#include "x80_cases.h"

#define CHECK(x)                                                                                              \
    do {                                                                                                      \
        const hipError_t e_ = (x);                                                                            \
        if (e_ != hipSuccess) {                                                                               \
            fprintf(stderr, "x80_device_check: %s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);     \
            exit(2);                                                                                          \
        }                                                                                                     \
    } while (0)

enum Op { X80_MUL, X80_ADD, X80_DIV, N80_MUL, N80_ADD, N80_SUM, N80_DIV, N80_MULADD, N80_ROUNDTRIP, N_OPS };
static const char* const OP_NAME[N_OPS] = {"x80_mul", "x80_add", "x80_div", "n80_mul", "n80_add", "n80_sum", "n80_div", "n80_muladd", "n80_from_to"};

struct Case {       // a (op) b;  r + a * b for n80_muladd;  a alone for the round trip
    VgX80 a, b, r;
};
struct Res {
    uint64_t m;
    uint32_t e, pad;
};

template <int OP>
__host__ __device__ inline Res apply(const Case& c)
{
    VgX80 v = {0, 0};
    if (OP == X80_MUL) v = x80_mul(c.a, c.b);
    if (OP == X80_ADD) v = x80_add(c.a, c.b);
    if (OP == X80_DIV) v = x80_div(c.a, c.b);
    if (OP == N80_MUL) v = n80_to(n80_mul(n80_from(c.a), n80_from(c.b)));
    if (OP == N80_ADD) v = n80_to(n80_add(n80_from(c.a), n80_from(c.b)));
    if (OP == N80_SUM) v = n80_to(n80_sum(n80_from(c.a), n80_from(c.b)));
    if (OP == N80_DIV) v = n80_to(n80_div(n80_from(c.a), n80_from(c.b)));
    if (OP == N80_MULADD) v = n80_to(n80_muladd(n80_from(c.r), n80_from(c.a), n80_from(c.b)));
    if (OP == N80_ROUNDTRIP) v = n80_to(n80_from(c.a));
    Res r;
    r.m = v.m;
    r.e = v.e;
    r.pad = 0;
    return r;
}

template <int OP>
__global__ __launch_bounds__(256) void divergent_kernel(const Case* __restrict__ in, Res* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    out[i] = apply<OP>(in[i]);
}

// wavefront w of the launch takes case first + w; the index is uniform, so the operands are and the function runs in its uniform form
template <int OP>
__global__ __launch_bounds__(256) void uniform_kernel(const Case* __restrict__ in, Res* __restrict__ out, uint32_t first, uint32_t n)
{
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    if (w >= n) return;
    const Res r = apply<OP>(in[first + w]);
    out[(size_t)w * 64u + (threadIdx.x & 63u)] = r;
}

static const int CHAIN_TERMS = 120;
struct ChainOut {
    Res x80, n80, fused;
    uint32_t fused_differs, pad;      // terms at which n80_muladd and n80_add(n80_mul) disagreed
};

// chain i: o = v[i * 121], s_t = v[i * 121 + 1 + t]
__host__ __device__ inline ChainOut run_chain(const VgX80* v)
{
    const VgX80 o = v[0];
    VgX80 r = {0, 0};
    VgN80 rn = {0, 0}, rf = {0, 0};
    ChainOut out;
    out.fused_differs = 0;
    out.pad = 0;
    for (int t = 0; t < CHAIN_TERMS; ++t) {
        const VgX80 s = v[1 + t];
        r = x80_add(r, x80_mul(s, o));
        rn = n80_add(rn, n80_mul(n80_from(s), n80_from(o)));
        rf = n80_muladd(rf, n80_from(s), n80_from(o));
        if (rf.m != rn.m || rf.e != rn.e) {
            ++out.fused_differs;
            rf = rn;
        }
    }
    const VgX80 a = n80_to(rn), b = n80_to(rf);
    out.x80 = Res{r.m, r.e, 0};
    out.n80 = Res{a.m, a.e, 0};
    out.fused = Res{b.m, b.e, 0};
    return out;
}

__global__ __launch_bounds__(64) void chains_kernel(const VgX80* __restrict__ v, ChainOut* __restrict__ out, uint32_t n)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    out[i] = run_chain(v + (size_t)i * (CHAIN_TERMS + 1));
}

// ---- the x87 unit ------------------------------------------------------------------------------------------------------------------
static long double to_ld(VgX80 v)
{
    unsigned char b[16] = {0};
    const uint16_t se = (uint16_t)v.e;
    memcpy(b, &v.m, 8);
    memcpy(b + 8, &se, 2);
    long double x;
    memcpy(&x, b, sizeof x);
    return x;
}

static VgX80 from_ld(long double x)
{
    VgX80 v;
    uint16_t se;
    memcpy(&v.m, &x, 8);
    memcpy(&se, (const char*)&x + 8, 2);
    v.e = se & 0x7FFFu;
    return v;
}

static bool same(VgX80 a, VgX80 b) { return a.m == b.m && a.e == b.e; }

enum Kind { K_MUL, K_ADD, K_DIV, K_MULADD, K_ROUNDTRIP };
static Kind kind_of(int op)
{
    switch (op) {
        case X80_MUL: case N80_MUL: return K_MUL;
        case X80_ADD: case N80_ADD: case N80_SUM: return K_ADD;
        case X80_DIV: case N80_DIV: return K_DIV;
        case N80_MULADD: return K_MULADD;
        default: return K_ROUNDTRIP;
    }
}

// the operation in the rounding mode that is set; for r + a * b the product is always rounded to nearest first (`prod`), so that the
// directed modes bracket the SECOND rounding, the one whose class is counted
static VgX80 x87(Kind k, const Case& c, VgX80 prod)
{
    volatile long double x = to_ld(c.a), y = to_ld(c.b), z = to_ld(c.r), p = to_ld(prod);
    volatile long double w = 0;
    switch (k) {
        case K_MUL: w = x * y; break;
        case K_ADD: w = x + y; break;
        case K_DIV: w = x / y; break;
        case K_MULADD: w = z + p; break;
        case K_ROUNDTRIP: w = x; break;
    }
    return from_ld(w);
}

struct Expect {
    VgX80 rn, lo, hi, prod;     // to nearest, downward, upward; prod: the rounded product of r + a * b
};

// ---- classes -----------------------------------------------------------------------------------------------------------------------
enum Class {
    C_EXACT, C_DOWN, C_UP, C_TIE_EVEN, C_TIE_ODD, C_CARRIED, C_RES_DENORMAL, C_DENORMAL_TO_NORMAL, C_NONZERO_TO_ZERO, C_ONE_DENORMAL,
    C_MORE_DENORMAL, C_ONE_ZERO, C_MORE_ZERO, C_D0_CARRY, C_D0_PLAIN, C_D1_CARRY, C_D1_PLAIN, C_D63_CARRY, C_D63_PLAIN, C_D64_CARRY, C_D64_PLAIN,
    C_D65_PLAIN, C_D128_PLAIN, C_MA_PROD_DENORMAL_R_NORMAL, C_MA_SUM_DENORMAL, C_MA_PROD_UNDERFLOW_ZERO, C_MA_R_ZERO, C_MA_R_ABOVE, C_MA_R_BELOW,
    C_MA_D63, C_MA_D64, C_MA_D65, N_CLASSES
};
static const char* const CLASS_NAME[N_CLASSES] = {
    "exact", "inexact_rounded_down", "inexact_rounded_up", "tie_kept_even", "tie_rounded_up_odd", "round_up_carried_into_next_binade",
    "result_denormal", "denormal_rounded_up_to_smallest_normal", "nonzero_operands_giving_zero", "one_operand_denormal",
    "more_operands_denormal", "one_operand_zero", "more_operands_zero", "distance_0_carry", "distance_0_no_carry", "distance_1_carry",
    "distance_1_no_carry", "distance_63_carry", "distance_63_no_carry", "distance_64_carry", "distance_64_no_carry", "distance_65_no_carry",
    "distance_128_up_no_carry", "product_denormal_r_normal", "sum_denormal", "product_zero_by_underflow", "r_zero", "r_above_product",
    "r_below_product", "distance_r_product_63", "distance_r_product_64", "distance_r_product_65"};

// Which classes a function can reach at all.  A sum of denormals is exact (so no sum rounds a denormal up to the smallest normal, and
// none of non-zero operands is zero); an operand 65 binades down or further is below half an ulp and cannot carry; a quotient of
// normal significands is never a tie nor carries, but one rounded at a denormal's precision is and does; 0 / 0 is no case.
static uint64_t applicable(Kind k)
{
    auto range = [](int a, int b) { uint64_t m = 0; for (int i = a; i <= b; ++i) m |= 1ull << i; return m; };
    switch (k) {
        case K_MUL: return range(C_EXACT, C_MORE_ZERO);
        case K_ADD: return (range(C_EXACT, C_RES_DENORMAL) | range(C_ONE_DENORMAL, C_D128_PLAIN));
        case K_DIV: return range(C_EXACT, C_ONE_ZERO);
        case K_MULADD: return (range(C_EXACT, C_RES_DENORMAL) | range(C_ONE_DENORMAL, C_MA_D65));
        default: return (1ull << C_EXACT) | (1ull << C_ONE_DENORMAL) | (1ull << C_ONE_ZERO);
    }
}

static int eff(VgX80 v) { return v.e ? (int)v.e : 1; }      // the exponent a stored value's bit 63 has
static int ctz64(uint64_t x) { return __builtin_ctzll(x); }
static bool denormal(VgX80 v) { return v.e == 0 && v.m != 0; }

// position of the lowest set bit of the exact sum a + b (both non-zero); bit j of v lies at eff(v) + j
static int lowest_bit_of_sum(VgX80 a, VgX80 b)
{
    const int pa = eff(a) + ctz64(a.m), pb = eff(b) + ctz64(b.m);
    if (pa != pb) return pa < pb ? pa : pb;
    if (eff(a) < eff(b)) { const VgX80 t = a; a = b; b = t; }
    const int d = eff(a) - eff(b);      // < 64: the lowest bits coincide
    const unsigned __int128 s = ((unsigned __int128)a.m << d) + b.m;
    const uint64_t lo = (uint64_t)s, hi = (uint64_t)(s >> 64);
    return eff(b) + (lo ? ctz64(lo) : 64 + ctz64(hi));
}

// is a / b exactly halfway between lo and its successor?  T = 2 lo + 1 in units of half an ulp:  a = T * 2^(eff(lo) - 1) * b.
// Only a result at a denormal's precision can be (T then fits 64 bits); odd parts and exponents are compared.
static bool quotient_is_tie(VgX80 a, VgX80 b, VgX80 lo)
{
    if (lo.e != 0) return false;
    const unsigned __int128 tb = (unsigned __int128)(2 * lo.m + 1) * b.m;
    uint64_t t_lo = (uint64_t)tb, t_hi = (uint64_t)(tb >> 64);
    int shift = 0;
    unsigned __int128 odd = tb;
    if (t_lo == 0) { shift = 64 + ctz64(t_hi); } else { shift = ctz64(t_lo); }
    odd >>= shift;
    if ((uint64_t)(odd >> 64) != 0) return false;
    const int za = ctz64(a.m);
    if ((a.m >> za) != (uint64_t)odd) return false;
    // a.m 2^(eff(a) - C) = T b.m 2^(eff(lo) - 1 - C + eff(b) - C),  C = BIAS + 63
    return eff(a) + za == eff(lo) - 1 + eff(b) - (VG_X80_BIAS + 63) + shift;
}

static uint64_t classify(Kind k, const Case& c, const Expect& x)
{
    uint64_t m = 0;
    auto set = [&](int cl) { m |= 1ull << cl; };
    // the operands of the rounding that is classified
    VgX80 a = c.a, b = c.b;
    if (k == K_MULADD) { a = c.r; b = x.prod; }
    const bool exact = same(x.lo, x.hi);
    if (exact) {
        set(C_EXACT);
    } else {
        bool tie = false;
        if (k == K_MUL) tie = eff(a) + ctz64(a.m) + eff(b) + ctz64(b.m) - (VG_X80_BIAS + 63) == eff(x.lo) - 1;
        if (k == K_ADD || k == K_MULADD) tie = lowest_bit_of_sum(a, b) == eff(x.lo) - 1;
        if (k == K_DIV) tie = quotient_is_tie(a, b, x.lo);
        const bool up = same(x.rn, x.hi);
        set(tie ? (up ? C_TIE_ODD : C_TIE_EVEN) : (up ? C_UP : C_DOWN));
        if (up && __builtin_popcountll(x.hi.m) == 1) set(C_CARRIED);
        if (up && x.hi.e == 1 && x.hi.m == 1ull << 63) set(C_DENORMAL_TO_NORMAL);
    }
    if (denormal(x.rn)) set(C_RES_DENORMAL);
    const int n_ops = k == K_ROUNDTRIP ? 1 : (k == K_MULADD ? 3 : 2);
    const VgX80 ops[3] = {c.a, c.b, c.r};
    int n_den = 0, n_zero = 0;
    for (int i = 0; i < n_ops; ++i) {
        n_den += denormal(ops[i]);
        n_zero += ops[i].m == 0;
    }
    if (n_den == 1) set(C_ONE_DENORMAL);
    if (n_den > 1) set(C_MORE_DENORMAL);
    if (n_zero == 1) set(C_ONE_ZERO);
    if (n_zero > 1) set(C_MORE_ZERO);
    if ((k == K_MUL || k == K_DIV) && n_zero == 0 && x.rn.m == 0) set(C_NONZERO_TO_ZERO);
    if ((k == K_ADD || k == K_MULADD) && a.m != 0 && b.m != 0) {
        const int d = eff(a) > eff(b) ? eff(a) - eff(b) : eff(b) - eff(a);
        const bool carry = eff(x.rn) > (eff(a) > eff(b) ? eff(a) : eff(b));
        if (d == 0) set(carry ? C_D0_CARRY : C_D0_PLAIN);
        if (d == 1) set(carry ? C_D1_CARRY : C_D1_PLAIN);
        if (d == 63) set(carry ? C_D63_CARRY : C_D63_PLAIN);
        if (d == 64) set(carry ? C_D64_CARRY : C_D64_PLAIN);
        if (d == 65) set(C_D65_PLAIN);
        if (d >= 128) set(C_D128_PLAIN);
        if (k == K_MULADD) {
            if (d == 63) set(C_MA_D63);
            if (d == 64) set(C_MA_D64);
            if (d == 65) set(C_MA_D65);
            const long double r = to_ld(a), p = to_ld(b);
            if (r > p) set(C_MA_R_ABOVE);
            if (r < p) set(C_MA_R_BELOW);
        }
    }
    if (k == K_MULADD) {
        if (denormal(x.prod) && c.r.e >= 1) set(C_MA_PROD_DENORMAL_R_NORMAL);
        if (denormal(x.rn)) set(C_MA_SUM_DENORMAL);
        if (c.a.m != 0 && c.b.m != 0 && x.prod.m == 0) set(C_MA_PROD_UNDERFLOW_ZERO);
        if (c.r.m == 0) set(C_MA_R_ZERO);
    }
    return m & applicable(k);
}

// ---- the cases of a function ---------------------------------------------------------------------------------------------------------
struct CaseSet {
    std::vector<Case> cases;
    std::vector<Expect> expect;
    std::vector<uint64_t> classes;
    long skipped = 0, redrawn = 0;
};

static int norm_exp(VgX80 v) { return eff(v) - (v.m ? __builtin_clzll(v.m) : 0); }

static void make_cases(Kind k, long n_random, CaseSet& s)
{
    const VgX80 zero = {0, 0};
    std::vector<Case>& out = s.cases;
    if (k == K_MULADD) {
        std::vector<X80Triple> t;
        x80_structured_triples(t);
        for (const auto& q : t) out.push_back({q.s, q.o, q.r});
        X80Gen gen(2024);
        for (long i = 0; i < n_random; ++i) {
            X80Triple q;
            while (!gen.triple(q.r, q.s, q.o)) ++s.redrawn;      // the product could overflow (outside vg_x80.h's domain): drawn again
            out.push_back({q.s, q.o, q.r});
        }
    } else {
        std::vector<X80Pair> p;
        x80_structured_pairs(p);
        X80Gen gen(12345);
        for (long i = 0; i < n_random; ++i) {
            X80Pair q;
            gen.pair(q.a, q.b);
            p.push_back(q);
        }
        for (const auto& q : p) {
            // no case: a division by zero, a quotient that overflows (the exponent of a quotient is at most one below this)
            if (k == K_DIV && (q.b.m == 0 || (q.a.m != 0 && norm_exp(q.a) - norm_exp(q.b) + VG_X80_BIAS >= 32766))) {
                ++s.skipped;
                continue;
            }
            out.push_back({q.a, k == K_ROUNDTRIP ? zero : q.b, zero});
        }
    }
    const size_t n = out.size();
    s.expect.resize(n);
    fesetround(FE_TONEAREST);
    for (size_t i = 0; i < n; ++i) {
        if (k == K_MULADD) s.expect[i].prod = x87(K_MUL, out[i], zero);
        s.expect[i].rn = x87(k, out[i], s.expect[i].prod);
    }
    fesetround(FE_DOWNWARD);
    for (size_t i = 0; i < n; ++i) s.expect[i].lo = x87(k, out[i], s.expect[i].prod);
    fesetround(FE_UPWARD);
    for (size_t i = 0; i < n; ++i) s.expect[i].hi = x87(k, out[i], s.expect[i].prod);
    fesetround(FE_TONEAREST);
    s.classes.resize(n);
    for (size_t i = 0; i < n; ++i) s.classes[i] = classify(k, out[i], s.expect[i]);
}

struct Report {
    long mismatches = 0;
    std::string first;
    void miss(const Case& c)
    {
        if (mismatches++ < 10) {
            char buf[256];
            snprintf(buf, sizeof buf, "%s[\"%016" PRIx64 ":%u\", \"%016" PRIx64 ":%u\", \"%016" PRIx64 ":%u\"]", first.empty() ? "" : ", ", c.a.m, c.a.e,
                     c.b.m, c.b.e, c.r.m, c.r.e);
            first += buf;
        }
    }
};

static void print_line(int op, const char* mode, const CaseSet& s, const Report& r)
{
    printf("{\"function\": \"%s\", \"mode\": \"%s\", \"cases\": %zu, \"skipped\": %ld, \"redrawn\": %ld, \"mismatches\": %ld, \"first\": [%s], \"classes\": {", OP_NAME[op],
           mode, s.cases.size(), s.skipped, s.redrawn, r.mismatches, r.first.c_str());
    const uint64_t app = applicable(kind_of(op));
    bool sep = false;
    for (int cl = 0; cl < N_CLASSES; ++cl) {
        if (!((app >> cl) & 1u)) continue;
        long count = 0;
        for (uint64_t m : s.classes) count += (m >> cl) & 1u;
        printf("%s\"%s\": %ld", sep ? ", " : "", CLASS_NAME[cl], count);
        sep = true;
    }
    printf("}}\n");
    fflush(stdout);
}

template <int OP>
static long run_op(const CaseSet& s, bool host, bool divergent, bool uniform)
{
    const size_t n = s.cases.size();
    long bad = 0;
    auto differs = [&](const Res& r, size_t i) { return r.m != s.expect[i].rn.m || r.e != s.expect[i].rn.e; };
    if (host) {
        Report rep;
        for (size_t i = 0; i < n; ++i)
            if (differs(apply<OP>(s.cases[i]), i)) rep.miss(s.cases[i]);
        print_line(OP, "host", s, rep);
        bad += rep.mismatches;
    }
    if (!divergent && !uniform) return bad;
    Case* d_in = nullptr;
    CHECK(hipMalloc(&d_in, n * sizeof(Case)));
    CHECK(hipMemcpy(d_in, s.cases.data(), n * sizeof(Case), hipMemcpyHostToDevice));
    if (divergent) {
        Res* d_out = nullptr;
        std::vector<Res> out(n);
        CHECK(hipMalloc(&d_out, n * sizeof(Res)));
        CHECK(hipMemset(d_out, 0xFF, n * sizeof(Res)));
        hipLaunchKernelGGL(divergent_kernel<OP>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, 0, d_in, d_out, (uint32_t)n);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(out.data(), d_out, n * sizeof(Res), hipMemcpyDeviceToHost));
        CHECK(hipFree(d_out));
        Report rep;
        for (size_t i = 0; i < n; ++i)
            if (differs(out[i], i)) rep.miss(s.cases[i]);
        print_line(OP, "divergent", s, rep);
        bad += rep.mismatches;
    }
    if (uniform) {
        const size_t chunk = 32768;     // cases a launch: 64 results each
        Res* d_out = nullptr;
        Res* out = nullptr;
        CHECK(hipHostMalloc(&out, chunk * 64 * sizeof(Res)));
        CHECK(hipMalloc(&d_out, chunk * 64 * sizeof(Res)));
        Report rep;
        for (size_t first = 0; first < n; first += chunk) {
            const size_t count = n - first < chunk ? n - first : chunk;
            CHECK(hipMemsetAsync(d_out, 0xFF, count * 64 * sizeof(Res), 0));
            hipLaunchKernelGGL(uniform_kernel<OP>, dim3((uint32_t)((count + 3) / 4)), dim3(256), 0, 0, d_in, d_out, (uint32_t)first, (uint32_t)count);
            CHECK(hipGetLastError());
            CHECK(hipMemcpy(out, d_out, count * 64 * sizeof(Res), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < count; ++i) {
                bool miss = false;
                for (size_t l = 0; l < 64; ++l) miss = miss || differs(out[i * 64 + l], first + i);
                if (miss) rep.miss(s.cases[first + i]);
            }
        }
        CHECK(hipFree(d_out));
        CHECK(hipHostFree(out));
        print_line(OP, "uniform", s, rep);
        bad += rep.mismatches;
    }
    CHECK(hipFree(d_in));
    return bad;
}

static long run_chains(long n_chains, bool host, bool device)
{
    std::vector<VgX80> v;
    std::vector<VgX80> want;
    X80Gen gen(777);
    const VgX80 zero = {0, 0};
    fesetround(FE_TONEAREST);
    for (long i = 0; i < n_chains; ++i) {
        const VgX80 o = gen.value();
        v.push_back(o);
        volatile long double oo = to_ld(o), rr = 0.0L;
        for (int t = 0; t < CHAIN_TERMS; ++t) {
            VgX80 s = gen.value();
            if ((int)s.e + (int)o.e > 2 * VG_X80_BIAS - 100) s = zero;      // the product could overflow: the term is left out
            volatile long double ss = to_ld(s);
            rr = rr + ss * oo;
            v.push_back(s);
        }
        want.push_back(from_ld(rr));
    }
    long bad = 0;
    auto judge = [&](const std::vector<ChainOut>& out, const char* mode) {
        long miss = 0;
        std::string first;
        for (long i = 0; i < n_chains; ++i) {
            const ChainOut& c = out[i];
            const VgX80 w = want[i];
            if (c.x80.m != w.m || c.x80.e != w.e || c.n80.m != w.m || c.n80.e != w.e || c.fused.m != w.m || c.fused.e != w.e || c.fused_differs) {
                if (miss++ < 10) first += (first.empty() ? "" : ", ") + std::to_string(i);
            }
        }
        printf("{\"function\": \"chains\", \"mode\": \"%s\", \"cases\": %ld, \"skipped\": 0, \"mismatches\": %ld, \"first\": [%s], \"classes\": {}}\n", mode,
               n_chains, miss, first.c_str());
        fflush(stdout);
        bad += miss;
    };
    std::vector<ChainOut> out(n_chains);
    if (host) {
        for (long i = 0; i < n_chains; ++i) out[i] = run_chain(v.data() + (size_t)i * (CHAIN_TERMS + 1));
        judge(out, "host");
    }
    if (device) {
        VgX80* d_v = nullptr;
        ChainOut* d_out = nullptr;
        CHECK(hipMalloc(&d_v, v.size() * sizeof(VgX80)));
        CHECK(hipMalloc(&d_out, n_chains * sizeof(ChainOut)));
        CHECK(hipMemcpy(d_v, v.data(), v.size() * sizeof(VgX80), hipMemcpyHostToDevice));
        CHECK(hipMemset(d_out, 0xFF, n_chains * sizeof(ChainOut)));
        hipLaunchKernelGGL(chains_kernel, dim3((uint32_t)((n_chains + 63) / 64)), dim3(64), 0, 0, d_v, d_out, (uint32_t)n_chains);
        CHECK(hipGetLastError());
        CHECK(hipMemcpy(out.data(), d_out, n_chains * sizeof(ChainOut), hipMemcpyDeviceToHost));
        CHECK(hipFree(d_v));
        CHECK(hipFree(d_out));
        judge(out, "chains");
    }
    return bad;
}

int main(int argc, char** argv)
{
    bool host = false, divergent = false, uniform = false, chains = false;
    long n_random = 1L << 19;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--host")) host = true;
        else if (!strcmp(argv[i], "--divergent")) divergent = true;
        else if (!strcmp(argv[i], "--uniform")) uniform = true;
        else if (!strcmp(argv[i], "--chains")) chains = true;
        else if (argv[i][0] >= '0' && argv[i][0] <= '9') n_random = atol(argv[i]);
        else {
            fprintf(stderr, "usage: x80_device_check [--host] [--divergent] [--uniform] [--chains] [<random cases per function>]\n");
            return 2;
        }
    }
    long bad = 0;
    if (host || divergent || uniform) {
        for (Kind k : {K_MUL, K_ADD, K_DIV, K_MULADD, K_ROUNDTRIP}) {
            CaseSet s;
            make_cases(k, n_random, s);
            switch (k) {
                case K_MUL:
                    bad += run_op<X80_MUL>(s, host, divergent, uniform);
                    bad += run_op<N80_MUL>(s, host, divergent, uniform);
                    break;
                case K_ADD:
                    bad += run_op<X80_ADD>(s, host, divergent, uniform);
                    bad += run_op<N80_ADD>(s, host, divergent, uniform);
                    bad += run_op<N80_SUM>(s, host, divergent, uniform);
                    break;
                case K_DIV:
                    bad += run_op<X80_DIV>(s, host, divergent, uniform);
                    bad += run_op<N80_DIV>(s, host, divergent, uniform);
                    break;
                case K_MULADD: bad += run_op<N80_MULADD>(s, host, divergent, uniform); break;
                case K_ROUNDTRIP: bad += run_op<N80_ROUNDTRIP>(s, host, divergent, uniform); break;
            }
        }
    }
    if (chains || host) bad += run_chains(n_random / 64 < 256 ? 256 : n_random / 64, host, chains);
    return bad != 0;
}
