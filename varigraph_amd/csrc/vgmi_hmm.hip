// vgmi_hmm.hip -- the forward / backward recursion of the genotyping HMM on the device, in the reference's arithmetic.
//
// replaces (inner loops of): GenotypeNameSpace::forward / backward (src/genotype.cpp:1170-1380): for every genotype g of the
// window,  r_g = sum over the previous node's entries p, IN THEIR ORDER, of  ((prev_p * no_recomb^keep) * recomb^change) * obs_g,
// keep = haplotypes g and p share, change = ploidy - keep;  then  total = sum of r_g in genotype order,  out_g = r_g / total
// (1 / n when total is zero).  The first node of a chain has  r_g = obs_g.  All of it is `long double` on the host; here it is
// vg_x80.h: the x87 unit's results bit for bit (one rounding per operation, gradual underflow), in integer instructions.
//
// One workgroup per chain (a window in one direction), one lane per genotype (<= 128).  The chain is serial node by node and
// term by term -- that is the reference's order of additions -- so the parallelism is genotypes x chains: 120 lanes x 2 x
// the windows of a sample.  The libm values (exp, pow) stay on the host and arrive as tables per step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "vg_x80.h"
#include "vgmi_kernels.h"

namespace vgk {

// what a step reads from memory, fetched one step ahead of its use (a chain is latency from end to end: a load that is
// waited for is time nothing else fills)
template <uint32_t STRIDE>
struct HmmStepIn {
    VgX80 keep_pow[STRIDE], change_pow[STRIDE];     // no_recomb^k, recomb^(ploidy - k)
    VgX80 obs;
    uint32_t restart;
};

// WAVES wavefronts share the genotypes evenly (2: a throughput launch; 4: a launch of few chains that has a CU per workgroup
// anyway -- the fewer genotypes a wavefront holds, the more often all of them agree that a term is negligible, and the idle
// SIMDs cost nothing: 392 instead of 405 ms on a chr20-scale sample; 8, two per SIMD, 455 ms)
template <uint32_t STRIDE, uint32_t WAVES>
__global__ __launch_bounds__(64 * WAVES) void hmm_recursion_kernel(HmmParams P)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t hmm_smem[];
    constexpr uint32_t stride = STRIDE;
    const uint32_t n = P.n_gt, per_wave = (n + WAVES - 1) / WAVES, lane = threadIdx.x & 63u;
    const bool active = lane < per_wave && (threadIdx.x >> 6) * per_wave + lane < n;
    const uint32_t g = active ? (threadIdx.x >> 6) * per_wave + lane : 0u;      // an idle lane reads genotype 0's inputs and writes nothing
    uint8_t* const s_keep = hmm_smem;                                              // n * n
    uint64_t* const s_step_m = reinterpret_cast<uint64_t*>(hmm_smem + ((n * n + 15u) & ~15u));   // 128 * stride
    int32_t* const s_step_e = reinterpret_cast<int32_t*>(s_step_m + 128u * stride);
    uint64_t* const s_r_m = reinterpret_cast<uint64_t*>(s_step_e + 128u * stride);      // 512 * stride bytes on: 8-byte aligned
    int32_t* const s_r_e = reinterpret_cast<int32_t*>(s_r_m + 128);

    const HmmChain ch = P.chains[blockIdx.x];
    const uint8_t* keep_g = P.keep + (size_t)ch.keep_index * n * n;
    for (uint32_t i = threadIdx.x; i < n * n; i += blockDim.x) s_keep[i] = keep_g[i];
    __syncthreads();
    const uint8_t* const my_keep = s_keep + (size_t)g * n;
    const VgX80 uniform = x80_load(P.uniform);
    if (ch.n_steps == 0) return;

    // a zero the compiler cannot see through: the per-step loads go through the vector memory path, whose counter the
    // waits on LDS do not share (a scalar load in flight would make every LDS wait a wait for memory)
    uint32_t lane_zero = 0;
    asm volatile("" : "+v"(lane_zero));
    auto fetch = [&](uint64_t s, uint32_t row_s, HmmStepIn<STRIDE>& in) {
        const uint8_t* pw = P.pow + s * (size_t)(2 * stride) * 16 + lane_zero;
#pragma unroll      // (the tables stay in registers at every stride: left to itself the compiler stops unrolling at stride 9 and indexes them in scratch)
        for (uint32_t k = 0; k < stride; ++k) {
            in.keep_pow[k] = x80_load(pw + (size_t)k * 16);
            in.change_pow[k] = x80_load(pw + (size_t)(stride + (stride - 1 - k)) * 16);
        }
        in.obs = x80_load(P.obs + ((size_t)row_s * n + g) * 16);
        in.restart = P.restart[s + lane_zero];
    };
    const uint64_t s_end = ch.first_step + ch.n_steps;
    HmmStepIn<STRIDE> cur;
    fetch(ch.first_step, P.row[ch.first_step], cur);
    uint32_t row_next = ch.n_steps > 1 ? P.row[ch.first_step + 1] : 0u;

    // values stay normalised (vg_x80.h: VgN80) from the load of a score to the store of a row: the hundred products and sums
    // of a node then take the one-rounding path, and only a result that is not a normal number takes the general one
    VgN80 prev = {0, 0};
    for (uint64_t s = ch.first_step; s < s_end; ++s) {
        HmmStepIn<STRIDE> nx = cur;
        uint32_t row_after = 0;
        if (s + 1 < s_end) fetch(s + 1, row_next, nx);
        if (s + 2 < s_end) row_after = P.row[s + 2 + lane_zero];

        const bool restart = __builtin_amdgcn_readfirstlane(cur.restart) != 0;
        VgN80 o = {0, 0};
        if (active) o = n80_from(cur.obs);
        if (!restart) {
            // (prev * no_recomb^keep) * recomb^change for this lane's previous entry and every keep
#pragma unroll
            for (uint32_t k = 0; k < stride; ++k) {
                const VgN80 st = n80_mul(n80_mul(prev, n80_from(cur.keep_pow[k])), n80_from(cur.change_pow[k]));
                if (active) {
                    s_step_m[g * stride + k] = st.m;
                    s_step_e[g * stride + k] = st.e;
                }
            }
        }
        __syncthreads();
        VgN80 r = {0, 0};
        if (active) {
            if (restart || (VG_DBG(P.dbg) & 2u)) {
                r = o;
            } else {
                // the table entry of term p + 1 and the keep byte of term p + 2 are fetched while term p is computed: the
                // chain r -> r is the only dependency the loop has to wait for (one wavefront per SIMD: nothing else hides LDS)
                uint32_t at = my_keep[0];
                VgN80 nxt;
                nxt.m = s_step_m[at];
                nxt.e = s_step_e[at];
                uint32_t k2 = n > 1 ? my_keep[1] : 0;
                for (uint32_t p = 0; p < n; ++p) {
                    const VgN80 st = nxt;
                    if (p + 1 < n) {
                        at = (p + 1) * stride + k2;
                        nxt.m = s_step_m[at];
                        nxt.e = s_step_e[at];
                        k2 = my_keep[p + 2 < n ? p + 2 : p + 1];
                    }
                    // a term more than 64 binades below the sum so far leaves it as it is (its exponent is at most the
                    // operands' sum + 2); when that holds for every genotype of the wavefront -- past the entries that carry
                    // the previous node's weight it mostly does -- the term is not computed
                    const bool nothing = st.m == 0 || o.m == 0 || (r.m != 0 && r.e - (st.e + o.e - VG_X80_BIAS + 2) > 64);
                    if (__builtin_amdgcn_ballot_w64(!nothing) == 0 && !(VG_DBG(P.dbg) & 8u)) continue;
                    r = n80_muladd(r, st, o);
                }
            }
        }
        if (active) {
            s_r_m[g] = r.m;
            s_r_e[g] = r.e;
        }
        __syncthreads();
        VgN80 total = {0, 0};
        VgN80 tn;
        // every lane adds the same values in the same order; the addresses carry lane_zero so that this runs on the vector
        // unit, branch-free (as scalar code it is a jump per case and twice the time)
        tn.m = s_r_m[lane_zero];
        tn.e = s_r_e[lane_zero];
        for (uint32_t p = 0; p < ((VG_DBG(P.dbg) & 1u) ? 1u : n); ++p) {
            const VgN80 t = tn;
            if (p + 1 < n) {
                tn.m = s_r_m[p + 1 + lane_zero];
                tn.e = s_r_e[p + 1 + lane_zero];
            }
            // an entry more than 64 binades below the running sum (or zero) leaves it as it is: every lane sees the same two
            // values, so the jump is taken by the whole wavefront (most entries of an informative node are that small)
            if (t.m == 0 || (total.m != 0 && total.e - t.e > 64)) continue;
            total = n80_sum(total, t);
        }
        VgX80 out = uniform;
        if (total.m != 0) {
            prev = (VG_DBG(P.dbg) & 4u) ? r : n80_div(r, total);
            out = n80_to(prev);
        } else {
            prev = n80_from(uniform);
        }
        if (active) x80_store(P.out + (s * n + g) * 16, out);
        __syncthreads();
        cur = nx;
        row_next = row_after;
    }
}

// ---- the recursion under `-m fre`: transitions by haplotype frequency (src/genotype.cpp:1196-1215, 1297-1316) ---------------------
// Both transition probabilities are zero there and a term is  (prev_p * obs_g) * score[hap_g[0]] * ... * score[hap_g[ploidy - 1]],
// the window's normalised gamma draws (doubles, widened exactly) multiplied on in the genotype's haplotype order.  obs_g comes first, so
// a term depends on p and g before any factor that is the lane's alone: no step table, 1 + PLOIDY products per term.  What does not
// change is the layout (a workgroup per chain, a lane per genotype, WAVES wavefronts), the sum over the previous entries in their order,
// the total, the divide and the uniform fallback.  A chain's keep_index names its table of factors: n_gt x PLOIDY long doubles.
// The previous row is published to LDS after the divide, one value per entry; every lane walks it in entry order.  Only  r + t  is a
// dependency from term to term: term p + 1 is multiplied out before term p is added, so its products overlap the addition.
template <uint32_t PLOIDY, uint32_t WAVES>
__global__ __launch_bounds__(64 * WAVES) void hmm_recursion_fre_kernel(HmmFreParams P)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t hmm_smem[];
    const uint32_t n = P.n_gt, per_wave = (n + WAVES - 1) / WAVES, lane = threadIdx.x & 63u;
    const bool active = lane < per_wave && (threadIdx.x >> 6) * per_wave + lane < n;
    const uint32_t g = active ? (threadIdx.x >> 6) * per_wave + lane : 0u;      // an idle lane reads genotype 0's inputs and writes nothing
    uint64_t* const s_r_m = reinterpret_cast<uint64_t*>(hmm_smem);             // this node's sums, for the total
    uint64_t* const s_p_m = s_r_m + 128;                                        // the previous node's row
    int32_t* const s_r_e = reinterpret_cast<int32_t*>(s_p_m + 128);
    int32_t* const s_p_e = s_r_e + 128;

    const HmmChain ch = P.chains[blockIdx.x];
    const VgX80 uniform = x80_load(P.uniform);
    if (ch.n_steps == 0) return;
    // the lane's factors: the window's, the same at every step.  ef: what they add to the bound on a term's exponent
    VgN80 f[PLOIDY];
    bool dead = false;
    int32_t ef = 0;
#pragma unroll
    for (uint32_t q = 0; q < PLOIDY; ++q) {
        f[q] = n80_from(x80_load(P.freq + (((size_t)ch.keep_index * n + g) * PLOIDY + q) * 16));
        dead = dead || f[q].m == 0;
        ef += f[q].e - VG_X80_BIAS + 1;
    }

    if (active) {      // a chain that does not begin with a restart begins from zeros, as the other kernel's does
        s_p_m[g] = 0;
        s_p_e[g] = 0;
    }
    __syncthreads();

    uint32_t lane_zero = 0;      // (see hmm_recursion_kernel: the per-step loads stay on the vector memory path)
    asm volatile("" : "+v"(lane_zero));
    const uint64_t s_end = ch.first_step + ch.n_steps;
    VgX80 obs_cur = x80_load(P.obs + ((size_t)P.row[ch.first_step] * n + g) * 16);
    uint32_t restart_cur = P.restart[ch.first_step + lane_zero];
    uint32_t row_next = ch.n_steps > 1 ? P.row[ch.first_step + 1] : 0u;

    for (uint64_t s = ch.first_step; s < s_end; ++s) {
        VgX80 obs_nx = obs_cur;
        uint32_t restart_nx = 0, row_after = 0;
        if (s + 1 < s_end) {      // the next step's inputs, fetched a step ahead
            obs_nx = x80_load(P.obs + ((size_t)row_next * n + g) * 16);
            restart_nx = P.restart[s + 1 + lane_zero];
        }
        if (s + 2 < s_end) row_after = P.row[s + 2 + lane_zero];

        const bool restart = __builtin_amdgcn_readfirstlane(restart_cur) != 0;
        VgN80 o = {0, 0};
        if (active) o = n80_from(obs_cur);
        VgN80 r = {0, 0};
        if (active) {
            if (restart) {
                r = o;
            } else {
                // a term's exponent is at most its operands' summed, plus one per multiply (and one to spare, as the other kernel has it)
                const bool lane_dead = dead || o.m == 0;
                const int32_t eo = o.e - VG_X80_BIAS + 1 + ef + 1;
                auto term = [&](uint32_t p, const VgN80& sum) {
                    VgN80 pv;
                    pv.m = s_p_m[p + lane_zero];
                    pv.e = s_p_e[p + lane_zero];
                    // nothing to add: a zero operand, or a term more than 64 binades below the sum so far (which only grows, so the sum
                    // of a term earlier decides no differently than the exact one would allow).  Skipped when the wavefront agrees.
                    const bool nothing = pv.m == 0 || lane_dead || (sum.m != 0 && sum.e - (pv.e + eo) > 64);
                    VgN80 t = {0, 0};
                    if (__builtin_amdgcn_ballot_w64(!nothing) != 0) {
                        t = n80_mul(pv, o);
#pragma unroll
                        for (uint32_t q = 0; q < PLOIDY; ++q) t = n80_mul(t, f[q]);
                    }
                    return t;
                };
                VgN80 t = term(0, r);
                for (uint32_t p = 0; p < n; ++p) {
                    VgN80 tn = {0, 0};
                    if (p + 1 < n) tn = term(p + 1, r);
                    if (__builtin_amdgcn_ballot_w64(t.m != 0) != 0) r = n80_sum(r, t);
                    t = tn;
                }
            }
            s_r_m[g] = r.m;
            s_r_e[g] = r.e;
        }
        __syncthreads();
        VgN80 total = {0, 0};
        VgN80 tn;
        tn.m = s_r_m[lane_zero];
        tn.e = s_r_e[lane_zero];
        for (uint32_t p = 0; p < n; ++p) {      // every lane adds the same values in the same order (hmm_recursion_kernel)
            const VgN80 t = tn;
            if (p + 1 < n) {
                tn.m = s_r_m[p + 1 + lane_zero];
                tn.e = s_r_e[p + 1 + lane_zero];
            }
            if (t.m == 0 || (total.m != 0 && total.e - t.e > 64)) continue;
            total = n80_sum(total, t);
        }
        VgX80 out = uniform;
        VgN80 prev = n80_from(uniform);
        if (total.m != 0) {
            prev = n80_div(r, total);
            out = n80_to(prev);
        }
        if (active) {
            x80_store(P.out + (s * n + g) * 16, out);
            s_p_m[g] = prev.m;
            s_p_e[g] = prev.e;
        }
        __syncthreads();
        obs_cur = obs_nx;
        restart_cur = restart_nx;
        row_next = row_after;
    }
}

// ---- posterior of a node (src/genotype.cpp:1387-1522) from the alpha / beta rows the recursion left on the device --------
//   denominator = sum of a_g * b_g in entry order;  post_g = (a_g * b_g) / denominator;  per genotype STRING (gid, made by the
//   host: alleles as decimal strings, sorted as strings) the sum of its entries' posts in entry order;  the first maximum in
//   string order (order[]) wins, its sum is the call's probability;  the call's genotype is the first entry of that string
//   with the largest post.  A zero denominator makes every post NaN on the host, which no comparison accepts: no call.
__device__ __forceinline__ bool x80_gt(VgX80 a, VgX80 b) { return a.e > b.e || (a.e == b.e && a.m > b.m); }

// what one lane does last, on the posts (s_m, s_e), the strings' sums (s_sum_m, s_sum_e) and the entries' strings (s_gid) in LDS: the
// first maximum in string order (ord) is the call's probability, the first entry of that string with the largest post its genotype
__device__ __forceinline__ void hmm_posterior_pick(const HmmPostParams& P, uint64_t rowi, const uint64_t* s_m, const uint32_t* s_e, const uint64_t* s_sum_m,
                                                   const uint32_t* s_sum_e, const uint8_t* s_gid, const uint8_t* ord)
{
    const uint32_t n = P.n_gt;
    VgX80 best = {0, 0};
    uint32_t best_id = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < n && ord[k] != 0xFF; ++k) {
        VgX80 sk;
        sk.m = s_sum_m[ord[k]];
        sk.e = s_sum_e[ord[k]];
        if (best_id == 0xFFFFFFFFu || x80_gt(sk, best)) {     // the host starts from -1: the first string always enters
            best = sk;
            best_id = ord[k];
        }
    }
    VgX80 max_post = {0, 0};
    uint32_t win = 0xFFFFFFFFu;
    for (uint32_t q = 0; q < n; ++q) {
        if (s_gid[q] != best_id) continue;
        VgX80 t;
        t.m = s_m[q];
        t.e = s_e[q];
        if (x80_gt(t, max_post)) {
            max_post = t;
            win = q;
        }
    }
    x80_store(P.prob + rowi * 16, best);
    P.winner[rowi] = best_id == 0xFFFFFFFFu ? 0xFFFFFFFEu : win;   // 0xFFFFFFFE: no string at all
}

__global__ __launch_bounds__(128) void hmm_posterior_kernel(HmmPostParams P)
{
    __shared__ uint64_t s_m[128];
    __shared__ uint32_t s_e[128];
    __shared__ uint64_t s_sum_m[128];
    __shared__ uint32_t s_sum_e[128];
    __shared__ uint8_t s_gid[128];
    const uint32_t n = P.n_gt, g = threadIdx.x;
    const uint64_t rowi = P.row0 + blockIdx.x;
    const bool active = g < n;
    VgX80 p = {0, 0};
    if (active) {
        const VgX80 a = x80_load(P.ab + (P.fwd_step[rowi] * n + g) * 16), b = x80_load(P.ab + (P.bwd_step[rowi] * n + g) * 16);
        p = x80_mul(a, b);
        s_gid[g] = P.gid[rowi * n + g];
    }
    s_m[g] = p.m;
    s_e[g] = p.e;
    __syncthreads();
    VgX80 den = {0, 0};
    for (uint32_t q = 0; q < n; ++q) {
        VgX80 t;
        t.m = s_m[q];
        t.e = s_e[q];
        den = x80_add(den, t);
    }
    if (den.m == 0) {
        if (g == 0) P.winner[rowi] = 0xFFFFFFFFu;
        return;
    }
    __syncthreads();
    const VgX80 post = x80_div(p, den);
    s_m[g] = post.m;
    s_e[g] = post.e;
    __syncthreads();
    // lane k sums string k's entries in entry order
    VgX80 sum = {0, 0};
    for (uint32_t q = 0; q < n; ++q)
        if (s_gid[q] == g) {
            VgX80 t;
            t.m = s_m[q];
            t.e = s_e[q];
            sum = x80_add(sum, t);
        }
    s_sum_m[g] = sum.m;
    s_sum_e[g] = sum.e;
    __syncthreads();
    if (g == 0) hmm_posterior_pick(P, rowi, s_m, s_e, s_sum_m, s_sum_e, s_gid, P.order + rowi * n);
}

// ---- more than 128 genotypes per window (`-n` > 15 on a diploid sample: n (n + 1) / 2 pairs; any list the C ABI is given) -------
// The same recursion, the same order of additions: 256 lanes per chain, lane t holds genotypes t, t + 256, ... (GPL of them, in
// registers), the step table of ALL previous entries lives in LDS (12 bytes x n x (ploidy + 1)), and the keep matrix -- n x n
// bytes, too large for LDS from 363 genotypes on -- is read from global memory ROW p for term p: keep is symmetric (what two
// genotypes share does not depend on who asks), so keep[p][g] = keep[g][p] and the 256 lanes read consecutive bytes; the
// matrix of a window is L2-resident (n = 2 048: 4 MiB).  Time per node is n x GPL dependent terms per lane: the reference's
// O(n^2) per node, 256 genotypes at a time.
template <uint32_t STRIDE, uint32_t GPL>
__global__ __launch_bounds__(256) void hmm_recursion_big_kernel(HmmParams P)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t hmm_smem[];
    constexpr uint32_t stride = STRIDE, T = 256;
    const uint32_t n = P.n_gt, tid = threadIdx.x;
    uint64_t* const s_step_m = reinterpret_cast<uint64_t*>(hmm_smem);                 // n * stride
    uint64_t* const s_r_m = s_step_m + (size_t)n * stride;                             // n
    int32_t* const s_step_e = reinterpret_cast<int32_t*>(s_r_m + n);                   // n * stride
    int32_t* const s_r_e = s_step_e + (size_t)n * stride;                              // n
    const HmmChain ch = P.chains[blockIdx.x];
    const uint8_t* const keep_g = P.keep + (size_t)ch.keep_index * n * n;
    const VgX80 uniform = x80_load(P.uniform);
    if (ch.n_steps == 0) return;
    uint32_t lane_zero = 0;
    asm volatile("" : "+v"(lane_zero));
    bool act[GPL];
    uint32_t gi[GPL];
#pragma unroll
    for (uint32_t j = 0; j < GPL; ++j) {
        act[j] = tid + j * T < n;
        gi[j] = act[j] ? tid + j * T : 0u;     // an idle slot reads genotype 0's inputs and writes nothing
    }
    VgN80 prev[GPL];
#pragma unroll
    for (uint32_t j = 0; j < GPL; ++j) prev[j] = VgN80{0, 0};
    const uint64_t s_end = ch.first_step + ch.n_steps;
    for (uint64_t s = ch.first_step; s < s_end; ++s) {
        const uint32_t row_s = P.row[s];
        const bool restart = P.restart[s] != 0;
        const uint8_t* pw = P.pow + s * (size_t)(2 * stride) * 16;
        VgN80 o[GPL], r[GPL];
#pragma unroll
        for (uint32_t j = 0; j < GPL; ++j) {
            o[j] = VgN80{0, 0};
            if (act[j]) o[j] = n80_from(x80_load(P.obs + ((size_t)row_s * n + gi[j]) * 16));
            r[j] = VgN80{0, 0};
        }
        if (!restart) {
            for (uint32_t k = 0; k < stride; ++k) {
                const VgN80 kp = n80_from(x80_load(pw + (size_t)k * 16 + lane_zero));
                const VgN80 cp = n80_from(x80_load(pw + (size_t)(stride + (stride - 1 - k)) * 16 + lane_zero));
#pragma unroll
                for (uint32_t j = 0; j < GPL; ++j) {
                    const VgN80 st = n80_mul(n80_mul(prev[j], kp), cp);
                    if (act[j]) {
                        s_step_m[(size_t)gi[j] * stride + k] = st.m;
                        s_step_e[(size_t)gi[j] * stride + k] = st.e;
                    }
                }
            }
        }
        __syncthreads();
        if (restart) {
#pragma unroll
            for (uint32_t j = 0; j < GPL; ++j) r[j] = o[j];
        } else {
            uint8_t kb[GPL], kb_next[GPL];
#pragma unroll
            for (uint32_t j = 0; j < GPL; ++j) kb_next[j] = keep_g[gi[j]];
            for (uint32_t p = 0; p < n; ++p) {
#pragma unroll
                for (uint32_t j = 0; j < GPL; ++j) kb[j] = kb_next[j];
                if (p + 1 < n) {
#pragma unroll
                    for (uint32_t j = 0; j < GPL; ++j) kb_next[j] = keep_g[(size_t)(p + 1) * n + gi[j]];
                }
#pragma unroll
                for (uint32_t j = 0; j < GPL; ++j) {
                    VgN80 st;
                    st.m = s_step_m[(size_t)p * stride + kb[j]];
                    st.e = s_step_e[(size_t)p * stride + kb[j]];
                    // a term more than 64 binades below the sum so far leaves it as it is (vgmi_hmm.hip, the small kernel)
                    const bool nothing = !act[j] || st.m == 0 || o[j].m == 0 || (r[j].m != 0 && r[j].e - (st.e + o[j].e - VG_X80_BIAS + 2) > 64);
                    if (__builtin_amdgcn_ballot_w64(!nothing) == 0) continue;
                    r[j] = n80_muladd(r[j], st, o[j]);
                }
            }
        }
#pragma unroll
        for (uint32_t j = 0; j < GPL; ++j)
            if (act[j]) {
                s_r_m[gi[j]] = r[j].m;
                s_r_e[gi[j]] = r[j].e;
            }
        __syncthreads();
        VgN80 total = {0, 0};
        for (uint32_t p = 0; p < n; ++p) {
            VgN80 t;
            t.m = s_r_m[p + lane_zero];
            t.e = s_r_e[p + lane_zero];
            if (t.m == 0 || (total.m != 0 && total.e - t.e > 64)) continue;
            total = n80_sum(total, t);
        }
#pragma unroll
        for (uint32_t j = 0; j < GPL; ++j) {
            VgX80 out = uniform;
            if (total.m != 0) {
                prev[j] = n80_div(r[j], total);
                out = n80_to(prev[j]);
            } else {
                prev[j] = n80_from(uniform);
            }
            if (act[j]) x80_store(P.out + (s * n + gi[j]) * 16, out);
        }
        __syncthreads();
    }
}

// the posterior for any number of genotypes: 256 lanes, lane t takes entries t, t + 256, ...; at most 255 distinct genotype
// strings per node (gid is a byte; the host keeps a node with more on its own path)
__global__ __launch_bounds__(256) void hmm_posterior_big_kernel(HmmPostParams P)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t post_smem[];
    const uint32_t n = P.n_gt, tid = threadIdx.x;
    uint64_t* const s_m = reinterpret_cast<uint64_t*>(post_smem);       // n
    uint64_t* const s_sum_m = s_m + n;                                  // 256
    uint32_t* const s_e = reinterpret_cast<uint32_t*>(s_sum_m + 256);   // n
    uint32_t* const s_sum_e = s_e + n;                                  // 256
    uint8_t* const s_gid = reinterpret_cast<uint8_t*>(s_sum_e + 256);   // n
    const uint64_t rowi = P.row0 + blockIdx.x;
    const uint64_t fs = P.fwd_step[rowi], bs = P.bwd_step[rowi];
    for (uint32_t g = tid; g < n; g += 256) {
        const VgX80 a = x80_load(P.ab + (fs * n + g) * 16), b = x80_load(P.ab + (bs * n + g) * 16);
        const VgX80 p = x80_mul(a, b);
        s_m[g] = p.m;
        s_e[g] = p.e;
        s_gid[g] = P.gid[rowi * n + g];
    }
    __syncthreads();
    VgX80 den = {0, 0};
    for (uint32_t q = 0; q < n; ++q) {
        VgX80 t;
        t.m = s_m[q];
        t.e = s_e[q];
        den = x80_add(den, t);
    }
    if (den.m == 0) {
        if (tid == 0) P.winner[rowi] = 0xFFFFFFFFu;
        return;
    }
    __syncthreads();
    for (uint32_t g = tid; g < n; g += 256) {
        VgX80 p;
        p.m = s_m[g];
        p.e = s_e[g];
        const VgX80 post = x80_div(p, den);
        s_m[g] = post.m;
        s_e[g] = post.e;
    }
    __syncthreads();
    VgX80 sum = {0, 0};      // lane k sums string k's entries in entry order
    for (uint32_t q = 0; q < n; ++q)
        if (s_gid[q] == tid) {
            VgX80 t;
            t.m = s_m[q];
            t.e = s_e[q];
            sum = x80_add(sum, t);
        }
    s_sum_m[tid] = sum.m;
    s_sum_e[tid] = sum.e;
    __syncthreads();
    if (tid == 0) hmm_posterior_pick(P, rowi, s_m, s_e, s_sum_m, s_sum_e, s_gid, P.order + rowi * n);
}

// ---- emission scores of a node: hidden states (src/genotype.cpp:640-830) and observable states (:960-1000) --------------------
// One workgroup of 128 lanes per node, lane g = genotype g = a PAIR of haplotypes (used[pos_a[g]], used[pos_b[g]]) -- or three or four
// of them (a polyploid sample's genotypes are blocks of `ploidy` consecutive haplotypes, src/genotype.cpp:846-873; round 5).  Per k-mer of
// the node, in list order: coverage c, multiplicity f and the haplotype bits decide, the same for every lane, which of the
// <= 16 haplotypes count as carrying the k-mer; the lane's copy number h is the sum over its two; (h, c, f) go through
// most_likely_depth (:1118-1145, float and double arithmetic as the host's SSE code does it) and select the term -- geometric for
// h = 0, Poisson(ave * h) otherwise, libm values tabulated by the host per sample -- and the lane multiplies it onto its product
// in the reference's long double (vg_x80.h).  A k-mer that is under-covered, multi-copy and carried makes the reference check
// the haplotype's SEQUENCE (:760-800): such a node is flagged and scored by the host.  Every k-mer list must be whole (no
// selected-haplotype pruning: all haplotypes are selected), which the caller guarantees and bit 1 of the flags verifies -- unless the
// haplotypes are selected per window (SELECT below): then the kernel prunes, as the reference's forward pass does.
__device__ __forceinline__ uint32_t hmm_most_likely_depth(uint32_t h, uint32_t c, uint32_t f, float ave, double upper)
{
    if (f == 1u) return c;
    if (h > 0u && (float)c > ave * (float)h) return (uint32_t)(int32_t)(ave * (float)h) & 0xFFu;
    if (h == 0u && (float)c > ave) return ((double)f > (double)((float)c) / upper) ? 0u : (uint32_t)(int32_t)((float)c / (float)f) & 0xFFu;
    if (h == 0u) return (uint32_t)(int32_t)((float)c / (float)f) & 0xFFu;
    return c;
}

// the sample's term tables, (ploidy + 1) x 256 long doubles, into LDS as 12-byte terms, by a workgroup of BLOCK lanes
template <uint32_t BLOCK>
__device__ __forceinline__ void hmm_stage_tables(const uint8_t* tables, uint32_t ploidy, uint64_t* s_tm, int32_t* s_te)
{
    for (uint32_t i = threadIdx.x; i < (ploidy + 1u) * 256u; i += BLOCK) {
        const VgN80 t = n80_from(x80_load(tables + (size_t)i * 16));
        s_tm[i] = t.m;
        s_te[i] = t.e;
    }
    __syncthreads();
}

// ---- how a node-list entry is read: two storage forms, one kernel body per family -----------------------------------------------------
// packed (vgmi_hmm_entries_upload): one 64-bit word per entry, multiplicity << 8 | haplotype bits << 16 -- up to six bytes of bits.
// wide (vgmi_hmm_entries_upload_wide, panels of 48 to 254 haplotypes; _wide16, up to 511): the multiplicity byte f[e] and the bit vector as it
// stands in the graph, little-endian in W = 1, 2, 4 or 8 64-bit words, zero-padded, entry-major: bits[e * W + i] -- one contiguous 8, 16, 32
// or 64-byte load.
// The last bit of the vector (bit bl8 - 1) is the flag it is everywhere, never a haplotype.
// A reader E states, for entry e:
//   E::W            words of haplotype bits per entry, and per mask over haplotype ids (a window's, a row's gt0, a fix's)
//   E::kMaxHap      the most haplotypes a panel has in this form (the support kernel's counters in LDS)
//   E::Id           what a window's list of drawn haplotypes (win_used) holds: a byte, or 16 bits where ids go beyond 255 (W = 8)
//   E::kDiploidOnly the place form of the emissions is launched for pairs of selected haplotypes only (no pos_more, no whole lists)
//   head(e)         what ONE load of the entry gives before anything is known about it: packed the word, wide nothing
//   mult(h, e)      the multiplicity: out of the head, or f[e]
//   word(h, e, i)   word i of the haplotype bits: out of the head, or bits[e * W + i]
//   carries(h, e, hap)  one haplotype's bit when only that is wanted (the tallies): out of the head, or the one word that holds it
//   hap_mask(n, i)  word i of the mask of the first n haplotypes
// So a packed kernel loads an entry once, wherever the body asks for its parts, and a wide one loads each part where it is asked for.
// A register array of W words is only ever indexed by an unrolled loop's counter; the word of haplotype `hap` is picked by a chain
// over W (hmm_pick_word) or loaded on its own (the tallies).  (The polyploid tally is not read through a reader: see there.)  Row, window and every haplotype id are wavefront-uniform where the
// kernels say so, in either form: the words of an entry, the window's mask and the choice of a word stay on the scalar side.
struct HmmPackedEntries {
    static constexpr uint32_t W = 1, kMaxHap = 48;
    static constexpr bool kDiploidOnly = false;
    using Id = uint8_t;
    const unsigned long long* __restrict__ words;
    struct Head {
        unsigned long long word;
    };
    static __device__ __forceinline__ HmmPackedEntries of(const uint8_t*, const unsigned long long* words) { return HmmPackedEntries{words}; }
    __device__ __forceinline__ Head head(uint64_t e) const { return Head{words[e]}; }
    __device__ __forceinline__ uint32_t mult(const Head& h, uint64_t) const { return (uint32_t)(h.word >> 8) & 0xFFu; }
    __device__ __forceinline__ unsigned long long word(const Head& h, uint64_t, uint32_t) const { return h.word >> 16; }
    __device__ __forceinline__ bool carries(const Head& h, uint64_t, uint32_t hap) const { return ((h.word >> 16) >> hap) & 1ull; }
    static __device__ __forceinline__ unsigned long long hap_mask(uint32_t n, uint32_t) { return (1ull << n) - 1ull; }      // n <= 48
};

template <uint32_t WORDS>
struct HmmWideEntries {
    static constexpr uint32_t W = WORDS, kMaxHap = WORDS > 4u ? 512 : 256;
    static constexpr bool kDiploidOnly = true;
    using Id = typename std::conditional<(WORDS > 4u), uint16_t, uint8_t>::type;
    const uint8_t* __restrict__ f;
    const unsigned long long* __restrict__ bits;
    struct Head {};
    static __device__ __forceinline__ HmmWideEntries of(const uint8_t* f, const unsigned long long* words) { return HmmWideEntries{f, words}; }
    __device__ __forceinline__ Head head(uint64_t) const { return Head{}; }
    __device__ __forceinline__ uint32_t mult(const Head&, uint64_t e) const { return f[e]; }
    __device__ __forceinline__ unsigned long long word(const Head&, uint64_t e, uint32_t i) const { return bits[e * W + i]; }
    __device__ __forceinline__ bool carries(const Head&, uint64_t e, uint32_t hap) const { return (bits[e * W + (W > 1u ? hap >> 6 : 0u)] >> (hap & 63u)) & 1ull; }
    static __device__ __forceinline__ unsigned long long hap_mask(uint32_t n, uint32_t i)      // n <= 64 W - 1
    {
        return n >= 64u * (i + 1u) ? ~0ull : n <= 64u * i ? 0ull : (1ull << (n - 64u * i)) - 1ull;
    }
};

template <uint32_t W>
__device__ __forceinline__ unsigned long long hmm_pick_word(const unsigned long long (&b)[W], uint32_t wi)
{
    if (W == 1u) return b[0];
    unsigned long long w = 0;      // (masks, not selects: a chain of selects over an array is what the compiler turns back into an index)
#pragma unroll
    for (uint32_t i = 0; i < W; ++i) w |= b[i] & (0ull - (unsigned long long)(wi == i));
    return w;
}

// bit `id` of W words
template <uint32_t W>
__device__ __forceinline__ uint32_t hmm_bit_of(const unsigned long long (&b)[W], uint32_t id)
{
    if (W == 1u) return (uint32_t)(b[0] >> id) & 1u;      // (id < 64: no word to choose, no bits to mask off the shift)
    return (uint32_t)(hmm_pick_word<W>(b, id >> 6) >> (id & 63u)) & 1u;
}

// SELECT (vgmi_hmm_emissions_select, _wide): -n picks fewer haplotypes than the panel has, so every window has drawn its own.  The row names
// its window, the window supplies `used` and the W-word mask; an entry that is no longer in its node's list is passed over, and an entry no
// selected haplotype carries -- no word of it meets the mask -- LEAVES the list here, for good (src/genotype.cpp:673-686, 815-818: the next
// window, the next sample score what is left).  Every lane takes the same decisions; lane 0 writes them down.  From `om` -- at most 16 bits
// over the places of the list -- on nothing depends on the entries' form.
// MAXP: the most haplotypes a genotype may have.  The tables are sized by it -- 4: 1 280 terms, 15 360 bytes of LDS, what a diploid, tri- or
// tetraploid launch has always asked for; 8: 2 304 terms, 27 648 bytes, for ploidy 5 .. 8 only (a workgroup per row: a larger table for
// everyone would cost every diploid launch workgroups per CU).
template <class E, bool SELECT, uint32_t MAXP>
__global__ __launch_bounds__(128) void hmm_emissions_kernel(HmmEmitParams P)
{
    constexpr uint32_t W = E::W;
    static_assert(SELECT || W == 1u, "one mask for every row is one word");
    __shared__ uint64_t s_tm[(MAXP + 1u) * 256u];      // (ploidy + 1) x 256 terms: up to MAXP haplotypes per genotype
    __shared__ int32_t s_te[(MAXP + 1u) * 256u];
    const uint32_t ploidy = E::kDiploidOnly ? 2u : P.ploidy;
    const uint32_t g = threadIdx.x;
    hmm_stage_tables<128>(P.tables, ploidy, s_tm, s_te);
    const uint64_t rowi = P.fix_rows ? P.fix_rows[blockIdx.x] : P.row_lo + blockIdx.x;
    uint32_t fp = P.fix_rows ? P.fix_off[blockIdx.x] : 0u;
    const uint32_t fe = P.fix_rows ? P.fix_off[blockIdx.x + 1] : 0u;
    const uint64_t e0 = P.entry_begin[rowi];
    const uint32_t cnt = P.entry_count[rowi], gt0 = P.gt0[rowi];
    const bool active = g < P.n_gt;
    unsigned long long top_mask[W];
    const typename E::Id* wused = nullptr;
    if (SELECT) {
        const uint32_t w = P.row_win[rowi];
#pragma unroll
        for (uint32_t i = 0; i < W; ++i) top_mask[i] = P.win_top_mask[(size_t)w * W + i];
        wused = reinterpret_cast<const typename E::Id*>(P.win_used) + (size_t)w * 16u;
    } else {
        top_mask[0] = P.top_mask;
    }
    const uint32_t pa = P.pos_a[active ? g : 0u], pb = P.pos_b[active ? g : 0u];
    const uint32_t pc = ploidy > 2u ? P.pos_more[0][active ? g : 0u] : 0u, pd = ploidy > 3u ? P.pos_more[1][active ? g : 0u] : 0u;
    uint32_t pe[MAXP > 4u ? MAXP - 4u : 1u] = {0};      // the fifth to the eighth haplotype's places (unrolled: the array stays in registers)
    if (MAXP > 4u) {
#pragma unroll
        for (uint32_t q = 4; q < MAXP; ++q)
            if (q < ploidy) pe[q - 4u] = P.pos_more[q - 2u][active ? g : 0u];
    }
    VgN80 prod;
    prod.m = 1ULL << 63;      // 1.0L
    prod.e = VG_X80_BIAS;
    uint32_t kept = 0, flag = 0;
    const E ent = E::of(P.ent.f, P.ent.words);
    for (uint32_t j = 0; j < cnt; ++j) {
        const uint64_t e = e0 + j;
        if (SELECT && P.alive[e] == 0) continue;      // pruned by an earlier window's or sample's selection
        const typename E::Head hd = ent.head(e);
        unsigned long long b[W], met = 0;
#pragma unroll
        for (uint32_t i = 0; i < W; ++i) {
            b[i] = ent.word(hd, e, i);
            met |= b[i] & top_mask[i];
        }
        const uint32_t c = P.cov[e], f = ent.mult(hd, e);
        if (met == 0) {
            if (SELECT) {
                if (g == 0 && !P.fix_rows) P.alive[e] = 0;      // the prune
            } else {
                flag |= 2u;      // the host would drop it from the list: this path does not prune
            }
            continue;
        }
        ++kept;
        const uint32_t lb = hmm_bit_of<W>(b, P.bl8 - 1u);
        const bool in_interval = lb == 1u && (double)c >= P.lower && (double)c <= P.upper;
        uint32_t om = 0;
        for (uint32_t p = 0; p < P.n_used; ++p) {
            const uint32_t hap = SELECT ? (uint32_t)wused[p] : (uint32_t)P.used[p];
            const uint32_t one = (in_interval && ((gt0 >> p) & 1u)) ? 1u : hmm_bit_of<W>(b, hap);
            om |= one << p;
        }
        if ((double)c < P.lower && f >= 2u && om != 0) flag |= 1u;
        if (fp < fe && P.fix_j[fp] == j) {      // (the second launch: haplotypes whose sequence does not hold this k-mer do not carry it)
            om &= ~(uint32_t)P.fix_mask[fp];
            ++fp;
        }
        const uint32_t fj = (lb == 1u && f == 1u) ? 2u : f;
        uint32_t h = ((om >> pa) & 1u) + ((om >> pb) & 1u);
        if (ploidy > 2u) h += (om >> pc) & 1u;
        if (ploidy > 3u) h += (om >> pd) & 1u;
        if (MAXP > 4u) {
#pragma unroll
            for (uint32_t q = 4; q < MAXP; ++q)
                if (q < ploidy) h += (om >> pe[q - 4u]) & 1u;
        }
        const uint32_t cc = hmm_most_likely_depth(h, c, fj, P.ave, P.upper);
        const uint32_t ti = h * 256u + cc;
        VgN80 t;
        t.m = s_tm[ti];
        t.e = s_te[ti];
        prod = n80_mul(prod, t);
    }
    if (active) x80_store(P.obs + (rowi * P.n_gt + g) * 16, n80_to(prod));
    if (g == 0 && !P.fix_rows) {
        P.n_kept[rowi] = kept;
        P.flags[rowi] = (uint8_t)flag;
    }
}

// ---- ... with a genotype LIST per window (vgmi_hmm_emissions_select_ploidy, _wide): a polyploid sample under -n ------------------------
// The genotypes of a window are the blocks of `ploidy` consecutive haplotypes that hold a drawn haplotype (src/genotype.cpp:846-873): 1 ..
// -n of them, another number in every window, over up to -n x ploidy haplotypes of which only the drawn ones decide the prune.  So
// nothing is a place in a 16-entry `used` list here: genotype g of window w names its haplotypes by id (win_haps), and every mask -- the
// drawn haplotypes (the prune), the blocks' haplotypes (who counts as carrying), the row's reference-allele bits, a fix -- is W words over
// haplotype ids, and so is `om`, the haplotypes that count as carrying an entry.  That is a few mask operations for the whole wavefront
// instead of a loop over places, and a lane's copy number is the sum over its `ploidy` ids with repeats (haplotype 0 stands several times
// in a truncated or all-zero block and counts each time, as the host's flat list does).  Only a lane's ids differ: it picks the word of
// each id out of `om` by hmm_pick_word's masks (an indexed read of `om` is what becomes scratch).
// A wavefront takes a row: the lists are 1 .. 16 genotypes long, a second wavefront per row would idle entirely; lanes beyond the window's
// count idle through the entry loop (and write a zero score: the part's rows are n_gt wide).  Every decision about an entry -- dead,
// pruned, flagged, fixed -- is the same for the whole wavefront: the row is made wavefront-uniform (readfirstlane), so the entry's words,
// coverage and alive byte are scalar loads and the branches are uniform.  The term tables, (ploidy + 1) x 256 entries of 12 bytes, are
// staged in LDS once per workgroup of four wavefronts, which takes kWinRows rows: a workgroup per row (the kernel above) would spend more
// on staging 15 KB than on a list of some fifty entries.
// MAXP as in hmm_emissions_kernel: 15 360 bytes of tables for ploidy 2 .. 4, 27 648 for ploidy 5 .. 8.
constexpr uint32_t kWinRows = 16;
template <class E, uint32_t MAXP>
__global__ __launch_bounds__(256) void hmm_emissions_win_kernel(HmmEmitWinParams P)
{
    constexpr uint32_t W = E::W;
    __shared__ uint64_t s_tm[(MAXP + 1u) * 256u];
    __shared__ int32_t s_te[(MAXP + 1u) * 256u];
    hmm_stage_tables<256>(P.tables, P.ploidy, s_tm, s_te);      // (its barrier is the only one: from here on the wavefronts go their own ways)
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), g = threadIdx.x & 63u;
    for (uint32_t k = wave; k < kWinRows; k += 4u) {
        const uint64_t item = (uint64_t)blockIdx.x * kWinRows + k;
        if (item >= P.n_items) break;
        const uint64_t rowi = P.fix_rows ? P.fix_rows[item] : item;
        uint32_t fp = P.fix_rows ? P.fix_off[item] : 0u;
        const uint32_t fe = P.fix_rows ? P.fix_off[item + 1] : 0u;
        const uint64_t e0 = P.entry_begin[rowi];
        const uint32_t cnt = P.entry_count[rowi];
        unsigned long long gt0[W], top_mask[W], used_mask[W];
#pragma unroll
        for (uint32_t i = 0; i < W; ++i) gt0[i] = P.gt0[rowi * W + i];
        const uint32_t w = P.row_win[rowi];
#pragma unroll
        for (uint32_t i = 0; i < W; ++i) {
            top_mask[i] = P.win_top_mask[(size_t)w * W + i];
            used_mask[i] = P.win_used_mask[(size_t)w * W + i];
        }
        const uint32_t n_here = P.win_n_gt[w];
        const bool active = g < n_here;
        uint32_t hap[MAXP] = {0};
        if (active) {
            if (MAXP > 4u || W > 1u) {
#pragma unroll
                for (uint32_t q = 0; q < MAXP; ++q)      // (unrolled with the places beyond `ploidy` left out: the array stays in registers)
                    if (q < P.ploidy) hap[q] = P.win_haps[((size_t)w * P.n_gt + g) * P.ploidy + q];
            } else {
                for (uint32_t q = 0; q < P.ploidy; ++q) hap[q] = P.win_haps[((size_t)w * P.n_gt + g) * P.ploidy + q];
            }
        }
        VgN80 prod;
        prod.m = 1ULL << 63;      // 1.0L
        prod.e = VG_X80_BIAS;
        uint32_t kept = 0, flag = 0;
        const E ent = E::of(P.ent.f, P.ent.words);
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t e = e0 + j;
            if (P.alive[e] == 0) continue;      // pruned by an earlier window's or sample's selection
            const typename E::Head hd = ent.head(e);
            unsigned long long b[W], met = 0;
#pragma unroll
            for (uint32_t i = 0; i < W; ++i) {
                b[i] = ent.word(hd, e, i);
                met |= b[i] & top_mask[i];
            }
            const uint32_t c = P.cov[e], f = ent.mult(hd, e);
            if (met == 0) {
                if (g == 0 && !P.fix_rows) P.alive[e] = 0;      // the prune: by the DRAWN haplotypes
                continue;
            }
            ++kept;
            const uint32_t lb = hmm_bit_of<W>(b, P.bl8 - 1u);
            const bool in_interval = lb == 1u && (double)c >= P.lower && (double)c <= P.upper;
            unsigned long long om[W], any = 0;      // the score: over the BLOCKS' haplotypes
#pragma unroll
            for (uint32_t i = 0; i < W; ++i) {
                om[i] = (b[i] | (in_interval ? gt0[i] : 0ull)) & used_mask[i];
                any |= om[i];
            }
            if ((double)c < P.lower && f >= 2u && any != 0) flag |= 1u;
            if (fp < fe && P.fix_j[fp] == j) {      // (the second launch: haplotypes whose sequence does not hold this k-mer do not carry it)
#pragma unroll
                for (uint32_t i = 0; i < W; ++i) om[i] &= ~P.fix_mask[(size_t)fp * W + i];
                ++fp;
            }
            if (!active) continue;
            const uint32_t fj = (lb == 1u && f == 1u) ? 2u : f;
            uint32_t h = hmm_bit_of<W>(om, hap[0]) + hmm_bit_of<W>(om, hap[1]);
            if (P.ploidy > 2u) h += hmm_bit_of<W>(om, hap[2]);
            if (P.ploidy > 3u) h += hmm_bit_of<W>(om, hap[3]);
            if (MAXP > 4u) {
#pragma unroll
                for (uint32_t q = 4; q < MAXP; ++q)      // (a repeated id counts at every place it stands)
                    if (q < P.ploidy) h += hmm_bit_of<W>(om, hap[q]);
            }
            const uint32_t cc = hmm_most_likely_depth(h, c, fj, P.ave, P.upper);
            const uint32_t ti = h * 256u + cc;
            VgN80 t;
            t.m = s_tm[ti];
            t.e = s_te[ti];
            prod = n80_mul(prod, t);
        }
        if (active) x80_store(P.obs + (rowi * P.n_gt + g) * 16, n80_to(prod));
        else if (g < P.n_gt) *reinterpret_cast<uint4*>(P.obs + (rowi * P.n_gt + g) * 16) = make_uint4(0, 0, 0, 0);
        if (g == 0 && !P.fix_rows) {
            P.n_kept[rowi] = kept;
            P.flags[rowi] = (uint8_t)flag;
        }
    }
}

// rows the host scored itself, handed in as one block: row[i] of the part <- src[i]
__global__ __launch_bounds__(128) void hmm_scatter_rows_kernel(uint8_t* obs, const uint64_t* rows, const uint8_t* src, uint32_t n_gt)
{
    const uint32_t g = threadIdx.x;
    if (g < n_gt)
        *reinterpret_cast<uint4*>(obs + (rows[blockIdx.x] * n_gt + g) * 16) = *reinterpret_cast<const uint4*>(src + ((size_t)blockIdx.x * n_gt + g) * 16);
}

// ---- a call's k-mer tallies (src/genotype.cpp:1387-1414 as posterior() reads them for the called haplotypes) -------------------
// Per row (node) with a called genotype g = (hap_a[g], hap_b[g]): over the node's entries, how many k-mers each called haplotype
// carries and the sum of their coverages (the caller divides), and how many k-mers have multiplicity <= 1 (clamped at 255).  A
// haplotype outside the panel or the selection reads as (0, 0), as on the host.  One lane per row: the entries of a node are ~50
// consecutive words, or per entry the two words that hold the called haplotypes.
// SELECT (vgmi_hmm_tallies_select, _wide), haplotypes selected per window: hap_ab holds places in the row's window's list (win_used), and
// only the entries still in the node's list count -- the unique-k-mer count as well (posterior() walks the pruned list)
template <class E, bool SELECT>
__global__ __launch_bounds__(256) void hmm_tally_kernel(const unsigned long long* __restrict__ words, const uint8_t* __restrict__ cov, const uint8_t* __restrict__ alive,
                                                        const uint64_t* __restrict__ entry_begin, const uint32_t* __restrict__ entry_count,
                                                        const uint32_t* __restrict__ row_win, const uint32_t* __restrict__ winner,
                                                        const uint8_t* __restrict__ hap_ab, const uint8_t* __restrict__ win_used, uint32_t n_gt, uint32_t n_hap,
                                                        unsigned long long sel_mask, uint64_t n_rows, uint32_t* __restrict__ out, uint8_t* __restrict__ uniq,
                                                        const uint8_t* __restrict__ f)
{
    const E ent = E::of(f, words);
    const uint64_t r = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rows) return;
    uint32_t num_a = 0, sum_a = 0, num_b = 0, sum_b = 0, u = 0;
    const uint32_t g = winner[r];
    if (g < n_gt) {
        uint32_t ha = hap_ab[2u * g], hb = hap_ab[2u * g + 1u];
        bool ok_a = true, ok_b = true;
        if (SELECT) {
            const typename E::Id* used = reinterpret_cast<const typename E::Id*>(win_used) + (size_t)row_win[r] * 16u;
            ha = used[ha];
            hb = used[hb];
        } else {
            ok_a = ha < n_hap && ((sel_mask >> ha) & 1ull);
            ok_b = hb < n_hap && ((sel_mask >> hb) & 1ull);
        }
        const uint64_t e0 = entry_begin[r];
        const uint32_t cnt = entry_count[r];
        for (uint32_t j = 0; j < cnt; ++j) {
            const uint64_t e = e0 + j;
            if (SELECT && alive[e] == 0) continue;
            const typename E::Head hd = ent.head(e);
            const uint32_t c = cov[e];
            if (ent.mult(hd, e) <= 1u && u < 255u) ++u;
            if (ok_a && ent.carries(hd, e, ha)) { ++num_a; sum_a += c; }
            if (ok_b && ent.carries(hd, e, hb)) { ++num_b; sum_b += c; }
        }
    }
    out[4 * r] = num_a;
    out[4 * r + 1] = sum_a;
    out[4 * r + 2] = num_b;
    out[4 * r + 3] = sum_b;
    uniq[r] = (uint8_t)u;
}

// (This family alone stays a PAIR of kernels: written once over the reader, the body was 5 to 7 % slower on the device in both forms
// -- DESIGN_INGEST_HMM.md 4.19.  The two differ in what an entry's load is and in which ids count: packed any id below 64 that the mask
// holds, wide the ids below bl8 - 1.  One launcher and one implementation of the C ABI serve both.)
// ---- ... of a POLYPLOID call (vgmi_hmm_tallies_ploidy): the called genotype is `ploidy` haplotype ids of the row's window's list ---------
// win_haps as the emission launch of such a sample takes them; an id that stands several times (haplotype 0 in a truncated or all-zero
// block) is tallied at every place it stands, an id outside win_sel_mask[w] -- not drawn, not in the panel -- or beyond 63 reads (0, 0), a
// winner at or beyond the window's count is no call: zeros.  alive == nullptr: the lists are whole, every entry counts.
// A wavefront takes a row and a lane an entry, 64 entries a turn, so the loads of a turn are consecutive words / bytes; the row is made
// wavefront-uniform (readfirstlane), the turns are the same for every lane, and what is counted is a ballot's population: the k-mers a
// called haplotype carries and the single-copy k-mers never leave the scalar side.  The coverage sums are kept per lane and added up
// across the wavefront once per row; lane 0 writes the row.  32-bit integer sums: any order of additions gives the host's numbers.
constexpr uint32_t kTallyRows = 16;
__global__ __launch_bounds__(256) void hmm_tally_ploidy_kernel(const unsigned long long* __restrict__ packed, const uint8_t* __restrict__ cov,
                                                               const uint8_t* __restrict__ alive, const uint64_t* __restrict__ entry_begin,
                                                               const uint32_t* __restrict__ entry_count, const uint32_t* __restrict__ row_win,
                                                               const uint32_t* __restrict__ winner, const uint32_t* __restrict__ win_n_gt,
                                                               const uint8_t* __restrict__ win_haps, const unsigned long long* __restrict__ win_sel_mask,
                                                               uint32_t n_gt, uint32_t ploidy, uint64_t n_rows, uint32_t* __restrict__ out,
                                                               uint8_t* __restrict__ uniq)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    for (uint32_t k = wave; k < kTallyRows; k += 4u) {
        const uint64_t r = (uint64_t)blockIdx.x * kTallyRows + k;
        if (r >= n_rows) break;
        const uint32_t w = row_win ? row_win[r] : 0u;
        const uint32_t g = winner[r];
        uint32_t num[4] = {0, 0, 0, 0}, sum[4] = {0, 0, 0, 0}, u = 0;
        if (g < (win_n_gt ? win_n_gt[w] : n_gt)) {
            const unsigned long long sel = win_sel_mask[w];
            uint32_t id[4] = {0, 0, 0, 0};
            bool ok[4] = {false, false, false, false};
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)      // (unrolled with the places beyond `ploidy` left out: the arrays stay in registers)
                if (q < ploidy) {
                    const uint32_t h = win_haps[((size_t)w * n_gt + g) * ploidy + q];
                    ok[q] = h < 64u && ((sel >> (h & 63u)) & 1ull);
                    id[q] = ok[q] ? h : 0u;
                }
            const uint64_t e0 = entry_begin[r];
            const uint32_t cnt = entry_count[r];
            for (uint32_t base = 0; base < cnt; base += 64u) {      // (every lane takes every turn: the ballots are the wavefront's)
                const uint32_t j = base + lane;
                const bool in = j < cnt && (!alive || alive[e0 + j] != 0);
                const unsigned long long word = in ? packed[e0 + j] : 0ull;
                const uint32_t c = in ? cov[e0 + j] : 0u;
                u += (uint32_t)__popcll(__ballot(in && ((uint32_t)(word >> 8) & 0xFFu) <= 1u));
                const unsigned long long bits = word >> 16;
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const bool hit = in && ok[q] && ((bits >> id[q]) & 1ull);
                    num[q] += (uint32_t)__popcll(__ballot(hit));
                    sum[q] += hit ? c : 0u;
                }
            }
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                for (uint32_t d = 32; d; d >>= 1) sum[q] += (uint32_t)__shfl_xor((int)sum[q], (int)d);
            if (u > 255u) u = 255u;
        }
        if (lane == 0) {
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                if (q < ploidy) {
                    out[(r * ploidy + q) * 2] = num[q];
                    out[(r * ploidy + q) * 2 + 1] = sum[q];
                }
            uniq[r] = (uint8_t)u;
        }
    }
}

// hmm_tally_ploidy_kernel over such a panel: a wavefront per row, a lane per entry, 64 entries a turn; a place counts if its id is a
// haplotype (below bl8 - 1) that the window's W-word mask holds, and every lane loads the one word of its entry that holds the id
template <uint32_t W>
__global__ __launch_bounds__(256) void hmm_tally_ploidy_wide_kernel(const uint8_t* __restrict__ f, const unsigned long long* __restrict__ bits,
                                                                    const uint8_t* __restrict__ cov, const uint8_t* __restrict__ alive,
                                                                    const uint64_t* __restrict__ entry_begin, const uint32_t* __restrict__ entry_count,
                                                                    const uint32_t* __restrict__ row_win, const uint32_t* __restrict__ winner,
                                                                    const uint32_t* __restrict__ win_n_gt, const uint8_t* __restrict__ win_haps,
                                                                    const unsigned long long* __restrict__ win_sel_mask, uint32_t n_gt, uint32_t ploidy,
                                                                    uint32_t bl8, uint64_t n_rows, uint32_t* __restrict__ out, uint8_t* __restrict__ uniq)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    for (uint32_t k = wave; k < kTallyRows; k += 4u) {
        const uint64_t r = (uint64_t)blockIdx.x * kTallyRows + k;
        if (r >= n_rows) break;
        const uint32_t w = row_win ? row_win[r] : 0u;
        const uint32_t g = winner[r];
        uint32_t num[4] = {0, 0, 0, 0}, sum[4] = {0, 0, 0, 0}, u = 0;
        if (g < (win_n_gt ? win_n_gt[w] : n_gt)) {
            uint32_t id_word[4] = {0, 0, 0, 0}, id_bit[4] = {0, 0, 0, 0};
            bool ok[4] = {false, false, false, false};
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)      // (unrolled with the places beyond `ploidy` left out: the arrays stay in registers)
                if (q < ploidy) {
                    const uint32_t h = win_haps[((size_t)w * n_gt + g) * ploidy + q];
                    const bool is_hap = h < bl8 - 1u;      // (then h >> 6 < W)
                    const uint32_t hw = is_hap && W > 1u ? h >> 6 : 0u;
                    ok[q] = is_hap && ((win_sel_mask[(size_t)w * W + hw] >> (h & 63u)) & 1ull);
                    id_word[q] = ok[q] ? hw : 0u;
                    id_bit[q] = ok[q] ? h & 63u : 0u;
                }
            const uint64_t e0 = entry_begin[r];
            const uint32_t cnt = entry_count[r];
            for (uint32_t base = 0; base < cnt; base += 64u) {      // (every lane takes every turn: the ballots are the wavefront's)
                const uint32_t j = base + lane;
                const uint64_t e = e0 + j;
                const bool in = j < cnt && (!alive || alive[e] != 0);
                const uint32_t c = in ? cov[e] : 0u;
                const uint32_t fm = in ? f[e] : 2u;
                u += (uint32_t)__popcll(__ballot(fm <= 1u));
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const unsigned long long word = in && ok[q] ? bits[e * W + id_word[q]] : 0ull;
                    const bool hit = (word >> id_bit[q]) & 1ull;
                    num[q] += (uint32_t)__popcll(__ballot(hit));
                    sum[q] += hit ? c : 0u;
                }
            }
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                for (uint32_t d = 32; d; d >>= 1) sum[q] += (uint32_t)__shfl_xor((int)sum[q], (int)d);
            if (u > 255u) u = 255u;
        }
        if (lane == 0) {
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                if (q < ploidy) {
                    out[(r * ploidy + q) * 2] = num[q];
                    out[(r * ploidy + q) * 2 + 1] = sum[q];
                }
            uniq[r] = (uint8_t)u;
        }
    }
}

// ---- selection support of the windows (src/genotype.cpp:500-560: what haplotype_selection sums before the gamma draws) ---------------
// support[w][hap] = sum of c over the alive entries of window w's rows with c > 1 and multiplicity <= 1 that haplotype `hap` carries.
// 32-bit integer sums: any order of additions gives the host's number.  A workgroup takes kSupportRows consecutive rows, a wavefront a
// row at a time, a lane an entry, the set bits walked word by word; the sums of a workgroup are gathered in LDS (E::kMaxHap counters) and
// leave it as one atomic per haplotype and window (rows come window after window, so a workgroup nearly always sees one window).
constexpr uint32_t kSupportRows = 64;
template <class E>
__global__ __launch_bounds__(256) void hmm_support_kernel(const unsigned long long* __restrict__ words, const uint8_t* __restrict__ cov, const uint8_t* __restrict__ alive,
                                                          const uint64_t* __restrict__ entry_begin, const uint32_t* __restrict__ entry_count,
                                                          const uint32_t* __restrict__ row_win, uint64_t n_rows, uint32_t n_hap, uint32_t* __restrict__ support,
                                                          const uint8_t* __restrict__ f)
{
    constexpr uint32_t W = E::W;
    const E ent = E::of(f, words);
    __shared__ uint32_t s_sup[E::kMaxHap];
    const uint64_t r0 = (uint64_t)blockIdx.x * kSupportRows;
    const uint64_t r1 = r0 + kSupportRows < n_rows ? r0 + kSupportRows : n_rows;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    unsigned long long hap_mask[W];      // the first n_hap bits
#pragma unroll
    for (uint32_t i = 0; i < W; ++i) hap_mask[i] = E::hap_mask(n_hap, i);
    uint64_t ra = r0;
    while (ra < r1) {      // the rows [ra, rb) of one window
        const uint32_t w = row_win[ra];
        uint64_t rb = ra + 1;
        while (rb < r1 && row_win[rb] == w) ++rb;
        if (E::kMaxHap <= 256u) {
            if (threadIdx.x < E::kMaxHap) s_sup[threadIdx.x] = 0;
        } else {      // (more counters than lanes)
            for (uint32_t h = threadIdx.x; h < E::kMaxHap; h += 256u) s_sup[h] = 0;
        }
        __syncthreads();
        for (uint64_t r = ra + wave; r < rb; r += 4) {
            const uint64_t e0 = entry_begin[r];
            const uint32_t cnt = entry_count[r];
            for (uint32_t j = lane; j < cnt; j += 64u) {
                const uint64_t e = e0 + j;
                if (alive[e] == 0) continue;
                const typename E::Head hd = ent.head(e);
                const uint32_t c = cov[e];
                if (c <= 1u || ent.mult(hd, e) > 1u) continue;
#pragma unroll
                for (uint32_t i = 0; i < W; ++i) {
                    unsigned long long word = ent.word(hd, e, i) & hap_mask[i];
                    while (word) {
                        const uint32_t hap = 64u * i + (uint32_t)__ffsll((long long)word) - 1u;
                        word &= word - 1ull;
                        atomicAdd(&s_sup[hap], c);
                    }
                }
            }
        }
        __syncthreads();
        if (E::kMaxHap <= 256u) {
            if (threadIdx.x < n_hap && s_sup[threadIdx.x] != 0) atomicAdd(&support[(size_t)w * n_hap + threadIdx.x], s_sup[threadIdx.x]);
        } else {
            for (uint32_t h = threadIdx.x; h < n_hap; h += 256u)
                if (s_sup[h] != 0) atomicAdd(&support[(size_t)w * n_hap + h], s_sup[h]);
        }
        __syncthreads();
        ra = rb;
    }
}

namespace {
// the run-time form and word count of the entries as the compile-time reader: launch(reader) for one of the five.  W = 8 is taken by the
// launchers that say so (WITH8: a diploid sample's support, emissions by places with their fixes, tallies); a genotype list per window is not
template <bool WITH8 = false, class Launch>
hipError_t hmm_with_entries(const HmmEntries& ent, Launch&& launch)
{
    if constexpr (WITH8)
        if (ent.W == 8) return launch(HmmWideEntries<8>{});
    switch (ent.W) {
        case 0: return launch(HmmPackedEntries{});
        case 1: return launch(HmmWideEntries<1>{});
        case 2: return launch(HmmWideEntries<2>{});
        case 4: return launch(HmmWideEntries<4>{});
        default: return hipErrorInvalidValue;
    }
}

// wide entries come with both arrays and a bit length their W words hold; the packed calls have never been asked
bool hmm_entries_fit(const HmmEntries& ent, uint32_t bl8) { return ent.W == 0 || (ent.f && ent.words && bl8 >= 8 && bl8 <= 64u * ent.W); }
}  // namespace

hipError_t launch_hmm_tally(const unsigned long long* packed, const uint8_t* cov, const uint64_t* entry_begin, const uint32_t* entry_count, const uint32_t* winner,
                            const uint8_t* hap_ab, uint32_t n_gt, uint32_t n_hap, unsigned long long sel_mask, uint64_t n_rows, uint32_t* out, uint8_t* uniq,
                            hipStream_t st)
{
    if (n_rows == 0) return hipSuccess;
    hipLaunchKernelGGL((hmm_tally_kernel<HmmPackedEntries, false>), dim3((uint32_t)((n_rows + 255) / 256)), dim3(256), 0, st, packed, cov, nullptr, entry_begin,
                       entry_count, nullptr, winner, hap_ab, nullptr, n_gt, n_hap, sel_mask, n_rows, out, uniq, nullptr);
    return hipGetLastError();
}

hipError_t launch_hmm_scatter_rows(uint8_t* obs, const uint64_t* rows, const uint8_t* src, uint32_t n_gt, uint64_t n, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(hmm_scatter_rows_kernel, dim3((uint32_t)n), dim3(128), 0, st, obs, rows, src, n_gt);
    return hipGetLastError();
}

hipError_t launch_hmm_emissions(const HmmEmitParams& P, uint64_t n_rows, hipStream_t st)
{
    if (n_rows == 0) return hipSuccess;
    if (P.ploidy < 2 || P.ploidy > 8 || !hmm_entries_fit(P.ent, P.bl8)) return hipErrorInvalidValue;
    if (P.row_win && (!P.win_used || !P.win_top_mask || !P.alive)) return hipErrorInvalidValue;
    return hmm_with_entries<true>(P.ent, [&](auto ent) {
        using E = decltype(ent);
        const dim3 grid((uint32_t)n_rows), block(128);
        if constexpr (E::kDiploidOnly) {
            if (P.ploidy != 2 || !P.row_win) return hipErrorInvalidValue;
            hipLaunchKernelGGL((hmm_emissions_kernel<E, true, 4>), grid, block, 0, st, P);
        } else if (P.row_win) {
            if (P.ploidy > 4) return hipErrorInvalidValue;      // (selection per window by places: a diploid sample's)
            hipLaunchKernelGGL((hmm_emissions_kernel<E, true, 4>), grid, block, 0, st, P);
        } else if (P.ploidy > 4) {
            hipLaunchKernelGGL((hmm_emissions_kernel<E, false, 8>), grid, block, 0, st, P);
        } else {
            hipLaunchKernelGGL((hmm_emissions_kernel<E, false, 4>), grid, block, 0, st, P);
        }
        return hipGetLastError();
    });
}

hipError_t launch_hmm_emissions_win(const HmmEmitWinParams& P, hipStream_t st)
{
    if (P.n_items == 0) return hipSuccess;
    if (P.n_gt < 1 || P.n_gt > 64 || P.ploidy < 2 || P.ploidy > 8 || !P.alive || !P.row_win || !P.win_n_gt || !P.win_haps || !P.win_top_mask || !P.win_used_mask ||
        (P.ent.W && !P.gt0) || !hmm_entries_fit(P.ent, P.bl8))
        return hipErrorInvalidValue;
    return hmm_with_entries(P.ent, [&](auto ent) {
        using E = decltype(ent);
        const dim3 grid((uint32_t)((P.n_items + kWinRows - 1) / kWinRows));
        if (P.ploidy > 4) hipLaunchKernelGGL((hmm_emissions_win_kernel<E, 8>), grid, dim3(256), 0, st, P);
        else hipLaunchKernelGGL((hmm_emissions_win_kernel<E, 4>), grid, dim3(256), 0, st, P);
        return hipGetLastError();
    });
}

hipError_t launch_hmm_support(const HmmEntries& ent, const uint8_t* cov, const uint8_t* alive, const uint64_t* entry_begin, const uint32_t* entry_count,
                              const uint32_t* row_win, uint64_t n_rows, uint32_t n_hap, uint32_t* support, hipStream_t st)
{
    if (n_rows == 0) return hipSuccess;
    if (n_hap < 1 || n_hap > (ent.W ? 64u * ent.W - 1u : 48u) || (ent.W <= 4 && n_hap > 255u)) return hipErrorInvalidValue;
    return hmm_with_entries<true>(ent, [&](auto e) {
        hipLaunchKernelGGL(hmm_support_kernel<decltype(e)>, dim3((uint32_t)((n_rows + kSupportRows - 1) / kSupportRows)), dim3(256), 0, st, ent.words, cov, alive,
                           entry_begin, entry_count, row_win, n_rows, n_hap, support, ent.f);
        return hipGetLastError();
    });
}

hipError_t launch_hmm_tally_select(const HmmEntries& ent, const uint8_t* cov, const uint8_t* alive, const uint64_t* entry_begin, const uint32_t* entry_count,
                                   const uint32_t* row_win, const uint32_t* winner, const uint8_t* pos_ab, const uint8_t* win_used, uint32_t n_gt, uint64_t n_rows,
                                   uint32_t* out, uint8_t* uniq, hipStream_t st)
{
    if (n_rows == 0) return hipSuccess;
    return hmm_with_entries<true>(ent, [&](auto e) {
        hipLaunchKernelGGL((hmm_tally_kernel<decltype(e), true>), dim3((uint32_t)((n_rows + 255) / 256)), dim3(256), 0, st, ent.words, cov, alive, entry_begin,
                           entry_count, row_win, winner, pos_ab, win_used, n_gt, 0u, 0ull, n_rows, out, uniq, ent.f);
        return hipGetLastError();
    });
}

hipError_t launch_hmm_tally_ploidy(const HmmEntries& ent, const uint8_t* cov, const uint8_t* alive, const uint64_t* entry_begin, const uint32_t* entry_count,
                                   const uint32_t* row_win, const uint32_t* winner, const uint32_t* win_n_gt, const uint8_t* win_haps,
                                   const unsigned long long* win_sel_mask, uint32_t n_gt, uint32_t ploidy, uint32_t bl8, uint64_t n_rows, uint32_t* out, uint8_t* uniq,
                                   hipStream_t st)
{
    if (n_rows == 0) return hipSuccess;
    if (ploidy < 2 || ploidy > 4 || n_gt < 1 || !win_haps || !win_sel_mask || !hmm_entries_fit(ent, bl8)) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((n_rows + kTallyRows - 1) / kTallyRows));
    auto wide = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, ent.f, ent.words, cov, alive, entry_begin, entry_count, row_win, winner, win_n_gt, win_haps, win_sel_mask, n_gt,
                           ploidy, bl8, n_rows, out, uniq);
    };
    switch (ent.W) {      // (the one family that is a pair of kernels: no reader to turn the form into)
        case 0:
            hipLaunchKernelGGL(hmm_tally_ploidy_kernel, grid, dim3(256), 0, st, ent.words, cov, alive, entry_begin, entry_count, row_win, winner, win_n_gt, win_haps,
                               win_sel_mask, n_gt, ploidy, n_rows, out, uniq);
            break;
        case 1: wide(hmm_tally_ploidy_wide_kernel<1>); break;
        case 2: wide(hmm_tally_ploidy_wide_kernel<2>); break;
        case 4: wide(hmm_tally_ploidy_wide_kernel<4>); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_hmm_posterior(const HmmPostParams& P, uint64_t n_rows, hipStream_t st)
{
    if (n_rows == 0) return hipSuccess;
    if (P.n_gt > 128) {
        const size_t lds = (size_t)P.n_gt * 13 + 256 * 12 + 64;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(hmm_posterior_big_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(hmm_posterior_big_kernel, dim3((uint32_t)n_rows), dim3(256), lds, st, P);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(hmm_posterior_kernel, dim3((uint32_t)n_rows), dim3(128), 0, st, P);
    return hipGetLastError();
}

size_t hmm_lds_bytes(uint32_t n_gt, uint32_t ploidy)
{
    const uint32_t stride = ploidy + 1;
    return (((size_t)n_gt * n_gt + 15u) & ~(size_t)15u) + (size_t)128 * stride * 12 + (size_t)128 * 12 + 64;
}

namespace {
// how many wavefronts a chain gets and how much LDS its workgroup asks for, for both recursion launchers
uint32_t hmm_waves_and_lds(uint32_t n_chains, size_t plain_lds, size_t& lds)
{
    // A small launch asks for more than half a CU's LDS: its workgroups then have a CU each.  The parts of a sample are
    // launches of a few dozen chains on streams of their own; the dispatcher starts each at the same CUs, and chains that
    // share a SIMD wait for each other's instructions (measured: 450 instead of 400 ms for the later parts).
    const size_t alone = 84 * 1024;
    const bool spread = n_chains <= 64 && plain_lds < alone;
    lds = spread ? alone : plain_lds;
    uint32_t waves = spread ? 4u : 2u;
    if (const char* w = getenv("VGMI_HMM_WAVES")) waves = atoi(w) == 4 ? 4u : 2u;     // A/B
    // (Several callers on one device -- the samples of a run side by side -- need nothing special: a SIMD runs two of these
    // wavefronts at little more than one's pace, a chain is latency; tools/gpu_hmm_pack.sh, 1 000 steps of 120 genotypes: 60 chains in
    // one launch 33.5 ms, 480 chains 39.6 ms, 960 chains 39.5 ms in the dense layout -- and 78.7 ms packed two workgroups to a CU.)
    return waves;
}

template <uint32_t STRIDE, uint32_t WAVES>
hipError_t launch_recursion_as(const HmmParams& Q, uint32_t n_chains, size_t lds, size_t plain_lds, hipStream_t st)
{
    if (lds > plain_lds &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(hmm_recursion_kernel<STRIDE, WAVES>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess) {
        (void)hipGetLastError();    // not granted: the plain launch
        lds = plain_lds;
    }
    hipLaunchKernelGGL((hmm_recursion_kernel<STRIDE, WAVES>), dim3(n_chains), dim3(64 * WAVES), lds, st, Q);
    return hipGetLastError();
}
template <uint32_t STRIDE>
hipError_t launch_recursion_waves(uint32_t waves, const HmmParams& Q, uint32_t n_chains, size_t lds, size_t plain_lds, hipStream_t st)
{
    switch (waves) {
        case 4: return launch_recursion_as<STRIDE, 4>(Q, n_chains, lds, plain_lds, st);
        default: return launch_recursion_as<STRIDE, 2>(Q, n_chains, lds, plain_lds, st);
    }
}
}  // namespace

namespace {
template <uint32_t STRIDE, uint32_t GPL>
hipError_t launch_recursion_big_as(const HmmParams& Q, uint32_t n_chains, hipStream_t st)
{
    const size_t lds = (size_t)Q.n_gt * (STRIDE + 1) * 12 + 64;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(hmm_recursion_big_kernel<STRIDE, GPL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((hmm_recursion_big_kernel<STRIDE, GPL>), dim3(n_chains), dim3(256), lds, st, Q);
    return hipGetLastError();
}
template <uint32_t STRIDE>
hipError_t launch_recursion_big(const HmmParams& Q, uint32_t n_chains, hipStream_t st)
{
    if (Q.n_gt <= 512) return launch_recursion_big_as<STRIDE, 2>(Q, n_chains, st);
    if (Q.n_gt <= 1024) return launch_recursion_big_as<STRIDE, 4>(Q, n_chains, st);
    return launch_recursion_big_as<STRIDE, 8>(Q, n_chains, st);
}
}  // namespace

hipError_t launch_hmm_recursion(const HmmParams& P, uint32_t n_chains, hipStream_t st)
{
    if (n_chains == 0) return hipSuccess;
    if (P.n_gt > 128) {
        if (P.n_gt > VGMI_HMM_MAX_GT) return hipErrorInvalidValue;
        HmmParams Q = P;
        Q.dbg = 0;
        switch (P.ploidy) {
            case 1: return launch_recursion_big<2>(Q, n_chains, st);
            case 2: return launch_recursion_big<3>(Q, n_chains, st);
            case 3: return launch_recursion_big<4>(Q, n_chains, st);
            case 4: return launch_recursion_big<5>(Q, n_chains, st);
            case 5: return launch_recursion_big<6>(Q, n_chains, st);
            case 6: return launch_recursion_big<7>(Q, n_chains, st);
            case 7: return launch_recursion_big<8>(Q, n_chains, st);
            case 8: return launch_recursion_big<9>(Q, n_chains, st);
            default: return hipErrorInvalidValue;
        }
    }
    const size_t plain_lds = hmm_lds_bytes(P.n_gt, P.ploidy);
    size_t lds = 0;
    const uint32_t waves = hmm_waves_and_lds(n_chains, plain_lds, lds);
    HmmParams Q = P;
    Q.dbg = vgmi_dbg_env();
    switch (P.ploidy) {
        case 1: return launch_recursion_waves<2>(waves, Q, n_chains, lds, plain_lds, st);
        case 2: return launch_recursion_waves<3>(waves, Q, n_chains, lds, plain_lds, st);
        case 3: return launch_recursion_waves<4>(waves, Q, n_chains, lds, plain_lds, st);
        case 4: return launch_recursion_waves<5>(waves, Q, n_chains, lds, plain_lds, st);
        case 5: return launch_recursion_waves<6>(waves, Q, n_chains, lds, plain_lds, st);
        case 6: return launch_recursion_waves<7>(waves, Q, n_chains, lds, plain_lds, st);
        case 7: return launch_recursion_waves<8>(waves, Q, n_chains, lds, plain_lds, st);
        case 8: return launch_recursion_waves<9>(waves, Q, n_chains, lds, plain_lds, st);
        default: return hipErrorInvalidValue;
    }
}

namespace {
template <uint32_t PLOIDY, uint32_t WAVES>
hipError_t launch_recursion_fre_as(const HmmFreParams& P, uint32_t n_chains, size_t lds, size_t plain_lds, hipStream_t st)
{
    if (lds > plain_lds &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(hmm_recursion_fre_kernel<PLOIDY, WAVES>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
            hipSuccess) {
        (void)hipGetLastError();    // not granted: the plain launch
        lds = plain_lds;
    }
    hipLaunchKernelGGL((hmm_recursion_fre_kernel<PLOIDY, WAVES>), dim3(n_chains), dim3(64 * WAVES), lds, st, P);
    return hipGetLastError();
}
template <uint32_t PLOIDY>
hipError_t launch_recursion_fre_waves(uint32_t waves, const HmmFreParams& P, uint32_t n_chains, size_t lds, size_t plain_lds, hipStream_t st)
{
    switch (waves) {
        case 4: return launch_recursion_fre_as<PLOIDY, 4>(P, n_chains, lds, plain_lds, st);
        default: return launch_recursion_fre_as<PLOIDY, 2>(P, n_chains, lds, plain_lds, st);
    }
}
}  // namespace

hipError_t launch_hmm_recursion_fre(const HmmFreParams& P, uint32_t n_chains, hipStream_t st)
{
    if (n_chains == 0) return hipSuccess;
    if (P.n_gt < 1 || P.n_gt > 128 || !P.freq) return hipErrorInvalidValue;
    const size_t plain_lds = (size_t)2 * 128 * 12 + 64;      // two rows of 128 values
    size_t lds = 0;
    const uint32_t waves = hmm_waves_and_lds(n_chains, plain_lds, lds);
    switch (P.ploidy) {
        case 2: return launch_recursion_fre_waves<2>(waves, P, n_chains, lds, plain_lds, st);
        case 3: return launch_recursion_fre_waves<3>(waves, P, n_chains, lds, plain_lds, st);
        case 4: return launch_recursion_fre_waves<4>(waves, P, n_chains, lds, plain_lds, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace vgk
