// genotyper.cpp -- see genotyper.hpp.  Floating-point note: every score is an x87 `long double`; the order of the
// operations and the std:: overload each one resolves to (double vs long double) are part of the contract, because
// the VCF prints GPP with one decimal and GQ from log10(1 - p).
#include "genotyper.hpp"

#include <immintrin.h>
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <iomanip>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <queue>
#include <random>
#include <set>
#include <sstream>
#include <stdexcept>
#include <thread>
#include <unordered_map>
#include <unordered_set>

#include "../vgmi_device.h"
#include "entry_bits.hpp"
#include "id_masks.hpp"
#include "fixed1.hpp"
#include "mem_advice.hpp"
#include "node_flanks.hpp"

namespace vgh {

namespace {
std::mutex g_cpu_mu;
std::condition_variable g_cpu_cv;
unsigned g_cpu_limit = 0, g_cpu_used = 0;
std::atomic<long long> g_cpu_wait_ns{0};        // VGH_TIMING: how long helpers stood in line for a token
const bool g_cpu_timing = getenv("VGH_TIMING") != nullptr;
}  // namespace

void CpuBudget::set(unsigned tokens)
{
    std::lock_guard<std::mutex> lk(g_cpu_mu);
    g_cpu_limit = tokens;
    g_cpu_cv.notify_all();
}

CpuBudget::Hold::Hold()
{
    std::unique_lock<std::mutex> lk(g_cpu_mu);
    if (g_cpu_timing && g_cpu_limit != 0 && g_cpu_used >= g_cpu_limit) {
        const auto t0 = std::chrono::steady_clock::now();
        g_cpu_cv.wait(lk, [] { return g_cpu_limit == 0 || g_cpu_used < g_cpu_limit; });
        g_cpu_wait_ns += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
    } else {
        g_cpu_cv.wait(lk, [] { return g_cpu_limit == 0 || g_cpu_used < g_cpu_limit; });
    }
    ++g_cpu_used;
}

CpuBudget::Hold::~Hold()
{
    {
        std::lock_guard<std::mutex> lk(g_cpu_mu);
        --g_cpu_used;
    }
    g_cpu_cv.notify_one();
}

namespace {

// ---------------------------------------------------------------- small numeric pieces (src/genotype.cpp:930-1150)
void poisson_interval(const double& lambda, double& lower, double& upper)
{
    const double sd = std::sqrt(lambda);
    upper = lambda + 1.96 * sd;
    lower = lambda - 1.96 * sd;
}

// recombination / no-recombination probabilities for a gap of `distance_bp` (Li-Stephens style, :940-950)
std::pair<long double, long double> transition_probabilities(uint32_t distance_bp, uint16_t population)
{
    const double effective_population_size = 1e-05;
    const double recomb_rate = 1.26;
    const long double d = distance_bp * 0.000004L * ((long double)recomb_rate) * effective_population_size;
    const long double recomb = (1.0L - std::exp(-d / (long double)population)) * (1.0L / (long double)population);
    const long double no_recomb = std::exp(-d / (long double)population) + recomb;
    return {recomb, no_recomb};
}

long double poisson_pmf(long double mean, uint8_t value)
{
    long double sum = 0.0L;
    const int v = (int)value;
    for (size_t i = 1; i <= value; ++i) sum += std::log(i);   // double log of an integer, accumulated in long double
    const long double log_val = -mean + v * std::log(mean) - sum;
    return std::exp(log_val);
}

double error_param(double ave_cov)
{
    if (ave_cov < 10.0) return 0.99;
    if (ave_cov < 20) return 0.95;
    if (ave_cov < 40) return 0.9;
    return 0.8;
}

long double geometric_prior(long double p)
{
    const long double mean = 0.5;
    const long double variance = 0.05;
    return (1 / (std::sqrt(2 * M_PI * variance))) * std::exp(-std::pow(p - mean, 2) / (2 * variance));
}

long double geometric_likelihood(long double p, uint8_t value)
{
    const long double q = 1.0 - p;
    return (std::pow(q, value)) * (std::pow(p, (1 - value)));
}

long double geometric(long double p, uint8_t value) { return geometric_likelihood(p, value) * geometric_prior(p); }

// h/c/f adjustment before scoring (:1118-1145)
void most_likely_depth(uint8_t h, uint8_t& c, uint8_t f, float ave_cov, double upper)
{
    if (f == 1) return;
    if (h > 0 && c > (ave_cov * h)) {
        c = ave_cov * h;
    } else if (h == 0 && c > ave_cov) {
        c = (f > ((float)c / upper)) ? 0 : c / (float)f;
    } else if (h == 0 && c <= ave_cov) {
        c /= (float)f;
    }
}

double phred_scaled(long double value) { return (value >= 1.0) ? 99 : (-10 * std::log10(1.0 - value)); }

// every k-mer key of a sequence (kmerBit::kmer_sketch_genotype, src/kmer.cpp:150-190)
std::unordered_set<uint64_t> sequence_keys(const std::string& s, uint32_t k)
{
    std::unordered_set<uint64_t> out;
    out.reserve(s.size());
    const uint64_t shift1 = 2 * (uint64_t)(k - 1), mask = (1ULL << 2 * k) - 1;
    uint64_t fwd = 0, rev = 0;
    int l = 0, span = 0;
    const unsigned int len = (unsigned int)s.size();
    for (unsigned int i = 0; i < len; ++i) {
        const uint32_t c = vg_nt4((uint8_t)s[i]);
        if (c < 4) {
            span = l + 1 < (int)k ? l + 1 : (int)k;
            fwd = (fwd << 2 | c) & mask;
            rev = (rev >> 2) | (3ULL ^ c) << shift1;
            if (fwd == rev) continue;
            const uint64_t canon = fwd < rev ? fwd : rev;
            ++l;
            if (l >= (int)k && span < 256) out.insert(vg_hash64(canon, mask) << 8 | (uint64_t)span);
        } else {
            l = 0;
            span = 0;
        }
    }
    return out;
}

// seed source of the haplotype sampler: std::random_device like the reference, or a fixed value for reproducible
// runs (VGH_RANDOM_DEVICE_VALUE; the reference's deterministic test build pins random_device the same way)
uint32_t random_device_value()
{
    if (const char* e = std::getenv("VGH_RANDOM_DEVICE_VALUE")) return (uint32_t)std::strtoul(e, nullptr, 10);
    std::random_device rd;
    return rd();
}

// Dirichlet-style haplotype sampling (src/haplotype_select.cpp): gamma draws weighted by the k-mer support of each
// haplotype, then the `n` largest
struct HaplotypeSampler {
    std::vector<uint16_t> top;                      // ascending draw (order the reference's min-heap pops them)
    std::unordered_map<uint16_t, double> score;     // normalised over the selected ones

    HaplotypeSampler(const std::vector<uint32_t>& support, int n)
    {
        std::mt19937 prng(random_device_value());
        const size_t hap_num = support.size();
        std::vector<double> freq(hap_num, 0.0);
        double total = 0;
        for (size_t i = 0; i < hap_num; ++i) {
            if (support[i] == 0) continue;
            freq[i] = std::gamma_distribution<double>(support[i] + 1.0, 1)(prng);
            total += freq[i];
        }
        if (total > 0)
            for (auto& f : freq) f /= total;
        struct Greater {
            bool operator()(const std::pair<double, uint16_t>& a, const std::pair<double, uint16_t>& b) { return a.first > b.first; }
        };
        std::priority_queue<std::pair<double, uint16_t>, std::vector<std::pair<double, uint16_t>>, Greater> pq;
        double sum = 0.0;
        for (uint16_t i = 0; i < freq.size(); i++) {
            pq.push(std::make_pair(freq[i], i));
            sum += freq[i];
            if (pq.size() > (size_t)n) {
                sum -= pq.top().first;
                pq.pop();
            }
        }
        while (!pq.empty()) {
            top.push_back(pq.top().second);
            score[pq.top().second] = pq.top().first / sum;
            pq.pop();
        }
    }
};

// every genotype the HMM considers: multisets of `ploidy` selected haplotypes (diploid), or the blocks of `ploidy`
// consecutive haplotype indices that make one polyploid VCF sample (src/genotype.cpp:835-915)
std::vector<std::vector<uint16_t>> haplotype_combinations(const std::vector<uint16_t>& haps, const std::string& sample_type,
                                                          uint32_t ploidy, uint16_t max_hap_idx)
{
    std::vector<std::vector<uint16_t>> out;
    if (ploidy > 2) {
        for (const auto& hap : haps) {
            std::vector<uint16_t> v(ploidy);
            if (hap == 0) {
                v.assign(ploidy, 0);
            } else {
                const int32_t quotient = std::ceil(hap / (float)ploidy);
                const uint16_t first = (quotient - 1) * ploidy + 1;
                std::iota(v.begin(), v.end(), first);
                for (auto& x : v)
                    if (x > max_hap_idx) x = 0;
            }
            out.push_back(std::move(v));
        }
        std::set<std::vector<uint16_t>> uniq(out.begin(), out.end());
        out.assign(uniq.begin(), uniq.end());
        return out;
    }
    const uint32_t last = (uint32_t)haps.size() - 1;
    std::vector<std::vector<uint32_t>> idx;
    for (uint32_t i = 0; i < haps.size(); i++) {
        std::vector<uint32_t> v(ploidy, i);
        idx.push_back(v);
        if (sample_type == "hom" || ploidy < 2) continue;
        auto mn = std::min_element(v.begin() + 1, v.end());
        while (*mn < last) {
            uint32_t j = (uint32_t)v.size() - 1;
            while (v[j] == last) {
                v[j] = *mn + 1;
                j--;
            }
            v[j]++;
            idx.push_back(v);
            mn = std::min_element(v.begin() + 1, v.end());
        }
    }
    out.reserve(idx.size());
    for (const auto& v : idx) {
        std::vector<uint16_t> h;
        h.reserve(v.size());
        for (uint32_t i : v) h.push_back(haps[i]);
        out.push_back(std::move(h));
    }
    return out;
}

template <typename T>
std::string join_numbers(const std::vector<T>& v, const char* delim)
{
    std::string s;
    for (size_t i = 0; i < v.size(); ++i) {
        s += std::to_string(v[i]);
        if (i + 1 != v.size()) s += delim;
    }
    return s;
}

std::string strip_newlines(const std::string& s)   // strip(str, '\n') of src/strip_split_join.cpp
{
    size_t i = 0, j = s.size();
    while (i < j && s[i] == '\n') ++i;
    while (j > i && s[j - 1] == '\n') --j;
    return s.substr(i, j - i);
}

}  // namespace

struct Genotyper::Run {
    // Everything per sample is in NODE ORDER: entry j belongs to place j of the graph2node lists (GraphIndex::node_key_index[j] is
    // its key) -- the order the device's per-node gather (K5, vgmi_counts_finish's cov_node) delivers and the order the windows
    // walk, so a node's k-mers are neighbours in memory instead of gathers over the key arrays.
    const uint8_t* cov;      // cov_node
    // coverage | multiplicity << 8 | haplotype bits << 16 of every entry in one word, when the bits fit; else nullptr
    const uint64_t* packed = nullptr;
    // ... and when they do not (7 to 32 bytes, a diploid sample): the entries are read from the graph's bit vectors, and the device holds them
    // as bytes (hmm_selected; VGH_HMM_WIDE_DEVICE=0: no such path)
    bool wide = false;
    float hap_cov;
    const GenotypeConfig* cfg;
    uint32_t haploid_num;   // min(-n, #haplotypes)
};

// A window prepared for the device recursion: its genotypes, the emission scores of its nodes and the tables of powers of
// both directions; window_finish() turns the device's alpha / beta into the nodes' calls.
struct Genotyper::WindowWork {
    Chrom* chr = nullptr;
    bool on_device = false;
    std::vector<uint16_t> top;
    std::vector<std::vector<uint16_t>> genotypes;
    std::vector<uint8_t> keep_mat;
    size_t n_gt = 0;
    uint32_t ploidy = 0;
    std::vector<uint32_t> nodes;                  // nodes with emission scores, in position order
    // where this window's rows and steps go in the run's arrays (room for every node the HMM works on; the tail stays unused)
    size_t row0 = 0, step0 = 0, room = 0;
    long double* obs = nullptr;                   // row0 on: nodes.size() x n_gt emission scores
    long double* pw = nullptr;                    // step0 on: per step no_recomb^0..ploidy, recomb^0..ploidy
    uint32_t* row = nullptr;                      // step0 on: forward chain (the nodes in order), then backward chain (from the last)
    uint8_t* restart = nullptr;
    uint8_t *gid = nullptr, *order = nullptr;     // row0 on: per node the genotype string of every entry / the strings in string order
    uint64_t *fwd_step = nullptr, *bwd_step = nullptr;   // row0 on: the steps that hold the node's alpha / beta
};

Genotyper::Genotyper(const GraphIndex& g, unsigned threads) : g_(g)
{
    n_hap_ = (uint32_t)g.hap_names.size();
    for (const auto& kv : g.hap_names) hap_ids_.push_back(kv.first);
    // variant nodes in mGraphMap order carry the graph2node k-mer lists (CSR over key indices).  The maps are walked once for
    // the nodes' places; the half million small k-mer lists are then copied by `threads` workers.
    struct Place { uint32_t start; const GraphNode* gn; size_t v; };
    size_t v = 0;
    const auto t_ctor = std::chrono::steady_clock::now();
    kmer_pool_.reset(new uint32_t[g.node_off.empty() || g.node_off.back() == 0 ? 1 : g.node_off.back()]);
    double s_walk = 0, s_alloc = 0, s_fill = 0;
    auto since = [](std::chrono::steady_clock::time_point a) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count(); };
    for (const auto& [chr, nodes] : g.graph_seq) {
        auto t_a = std::chrono::steady_clock::now();
        Chrom c;
        c.name = chr;
        auto it = g.chr_len.find(chr);
        c.len = it == g.chr_len.end() ? 0 : it->second;
        std::vector<Place> places;
        places.reserve(nodes.size());
        for (const GraphNode* gn : nodes) {
            size_t mine = SIZE_MAX;
            if (gn->hap_gt.size() != 1) {
                if (v + 1 >= g.node_off.size()) throw std::runtime_error("graph index: node list shorter than the graph");
                mine = v++;
            }
            places.push_back({gn->start, gn, mine});
        }
        s_walk += since(t_a);
        t_a = std::chrono::steady_clock::now();
        c.nodes.resize(places.size());
        s_alloc += since(t_a);
        t_a = std::chrono::steady_clock::now();
        auto fill = [&](size_t lo, size_t hi) {
            CpuBudget::Hold cpu;
            for (size_t i = lo; i < hi; ++i) {
                Node& n = c.nodes[i];
                n.start = places[i].start;
                n.gn = places[i].gn;
                if (places[i].v != SIZE_MAX) {      // places of the node's k-mers in the node-ordered arrays (not key indices)
                    n.kmers.p = kmer_pool_.get() + g.node_off[places[i].v];
                    n.kmers.n = (uint32_t)(g.node_off[places[i].v + 1] - g.node_off[places[i].v]);
                    std::iota(n.kmers.p, n.kmers.p + n.kmers.n, (uint32_t)g.node_off[places[i].v]);
                }
            }
        };
        const size_t nt = std::max<size_t>(1, std::min<size_t>(threads, places.size() / 4096 + 1));
        std::vector<std::thread> pool;
        for (size_t t = 1; t < nt; ++t) pool.emplace_back(fill, places.size() * t / nt, places.size() * (t + 1) / nt);
        fill(0, places.size() / nt);
        for (auto& th : pool) th.join();
        s_fill += since(t_a);
        chroms_.push_back(std::move(c));
    }
    if (getenv("VGH_TIMING"))
        std::fprintf(stderr, "[varigraph-mi] genotyper set-up %.3f s: nodes walked %.3f, allocated %.3f, k-mer lists %.3f\n", since(t_ctor), s_walk, s_alloc, s_fill);
}

// flanking sequence of a haplotype around a node: node_flanks.hpp (shared with `construct`)
std::pair<std::string, std::string> Genotyper::flanks(const Chrom& chr, uint32_t node_i, uint16_t hap, uint16_t alt_gt,
                                                      std::string& alt_seq, uint32_t want) const
{
    return node_flanks(chr.nodes, node_i, hap, alt_gt, alt_seq, want);
}

// ---------------------------------------------------------------- hidden states of one node (src/genotype.cpp:640-830)
// `genotypes` = the window's haplotype combinations (the same for every node of a window), `used` = the haplotypes
// occurring in them.  The per-haplotype term of a k-mer does not depend on the genotype, so it is evaluated once
// per (k-mer, haplotype) and summed per genotype.
// phase times summed over the pool's threads (VGH_TIMING): where the windows spend their time
namespace {
struct HmmPhases {
    std::atomic<long long> select{0}, states{0}, emit{0}, fwd{0}, bwd{0}, post{0};
    std::atomic<long long> list{0}, pass_a{0}, pass_b{0}, pass_c{0}, fill{0}, text{0};     // the device-emission path's host work, thread-seconds
};
HmmPhases g_phase;
const bool g_phase_on = getenv("VGH_TIMING") != nullptr;
struct PhaseTimer {
    std::atomic<long long>& acc;
    std::chrono::steady_clock::time_point t0;
    explicit PhaseTimer(std::atomic<long long>& a) : acc(a) { if (g_phase_on) t0 = std::chrono::steady_clock::now(); }
    ~PhaseTimer() { if (g_phase_on) acc += std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
};
}  // namespace

namespace {
// h[g] = one16[pos_a[g]] + one16[pos_b[g]] for 16 genotypes per step (the copy count of every genotype of a window for one
// k-mer: the same byte sums as the scalar loop)
__attribute__((target("ssse3"))) void hrow_pairs_ssse3(const uint8_t* one16, const uint8_t* pos_a, const uint8_t* pos_b, uint8_t* out, size_t n16)
{
    const __m128i tab = _mm_loadu_si128(reinterpret_cast<const __m128i*>(one16));
    for (size_t g = 0; g < n16; g += 16) {
        const __m128i a = _mm_shuffle_epi8(tab, _mm_loadu_si128(reinterpret_cast<const __m128i*>(pos_a + g)));
        const __m128i b = _mm_shuffle_epi8(tab, _mm_loadu_si128(reinterpret_cast<const __m128i*>(pos_b + g)));
        _mm_storeu_si128(reinterpret_cast<__m128i*>(out + g), _mm_add_epi8(a, b));
    }
}
const bool g_have_ssse3 = [] {
    __builtin_cpu_init();
    return __builtin_cpu_supports("ssse3") != 0;
}();
}  // namespace

Genotyper::NodeStates Genotyper::hidden_states(Chrom& chr, uint32_t node_i, const std::vector<uint16_t>& top,
                                               const std::vector<std::vector<uint16_t>>& genotypes,
                                               const std::vector<uint16_t>& used, const GenotypeList& gl, double lower,
                                               double upper, bool filter, const Run& r, NodeStates&& recycled, const Node* ahead)
{
    Node& node = chr.nodes[node_i];
    const std::vector<uint16_t>& hap_gt = node.gn->hap_gt;
    const uint64_t bl = g_.bitlen;
    const uint32_t* const key_of = g_.node_key_index.data();      // place in the node-ordered arrays -> key
    auto hap_bit = [&](uint32_t key, uint16_t hap) -> uint8_t { return ((uint8_t)g_.bitvec[(size_t)key * bl + (hap >> 3)] >> (hap & 7)) & 1u; };
    auto last_bit = [&](uint32_t key) -> int { return ((uint8_t)g_.bitvec[(size_t)key * bl + bl - 1] >> 7) & 1; };

    const size_t n_gt = genotypes.size();
    NodeStates ns = std::move(recycled);   // the previous node's buffers
    ns.n_genotypes = n_gt;
    ns.c.clear();
    ns.f.clear();
    ns.h.clear();
    ns.c.reserve(node.kmers.size());
    ns.f.reserve(node.kmers.size());
    ns.h.resize(node.kmers.size() * n_gt);
    const std::vector<uint16_t>& flat = gl.flat;
    const std::vector<uint32_t>& flat_off = gl.off;
    const bool pairs = gl.pairs;
    const bool shuffle = pairs && !gl.pos_a.empty() && g_have_ssse3;
    size_t n_kept = 0;

    std::vector<uint32_t>& kept = ns.kept;        // the node's k-mers that take part (all of them unless `filter`)
    kept.clear();
    kept.reserve(node.kmers.size());
    std::map<uint16_t, uint32_t> need_sequence;   // haplotypes with multi-copy, under-covered k-mers: check their sequence
    std::vector<uint8_t>& one = ns.one;
    one.assign(n_hap_, 0);
    // the per-key arrays are indexed at random: the keys of the node ahead are asked for one per k-mer of this node (all at
    // once they would overrun the core's miss buffers and most of the requests would be dropped)
    const uint32_t* pf = ahead ? ahead->kmers.data() : nullptr;
    const uint32_t* const pf_end = ahead ? pf + ahead->kmers.size() : nullptr;
    auto prefetch_one = [&]() {
        if (pf != pf_end) {
            const uint32_t k2 = *pf++;
            if (r.packed) {
                __builtin_prefetch(&r.packed[k2]);
                return;
            }
            __builtin_prefetch(&r.cov[k2]);
            __builtin_prefetch(&g_.f[key_of[k2]]);
            __builtin_prefetch(&g_.bitvec[(size_t)key_of[k2] * bl]);
        }
    };
    // Fast path (haplotype bits of a k-mer fit one 64-bit word, genotypes are pairs over <= 16 haplotypes): the word is
    // read once per k-mer and every test is a mask or a shift of it
    const bool fast = shuffle && r.packed != nullptr;
    ns.cls.clear();
    ns.rep.clear();
    // haplotypes (positions in `used`) that carried the same k-mers so far: a partition refined k-mer by k-mer
    uint16_t part[16];
    uint32_t n_part = 1;
    part[0] = (uint16_t)((1u << used.size()) - 1u);
    uint64_t top_mask = 0;
    uint8_t gt0[16] = {0};      // haplotype used[p] carries the reference allele at this node
    if (fast) {
        for (uint16_t hap : top) top_mask |= 1ULL << hap;
        for (size_t p = 0; p < used.size(); ++p) gt0[p] = hap_gt[used[p]] == 0;
    }
    for (uint32_t pos : node.kmers) {
        prefetch_one();
        uint8_t* hrow = &ns.h[n_kept * n_gt];
        if (fast) {
            const uint64_t w = r.packed[pos];
            const uint8_t c = (uint8_t)w, f = (uint8_t)(w >> 8);
            const uint64_t bits = w >> 16;
            const int lb = (int)((bits >> (8 * bl - 1)) & 1u);
            if (filter && (bits & top_mask) == 0) continue;
            kept.push_back(pos);
            const bool in_interval = lb == 1 && c >= lower && c <= upper;
            uint8_t one16[16] = {0};
            uint32_t carried_mask = 0;
            for (size_t p = 0; p < used.size(); ++p) {
                one16[p] = (in_interval && gt0[p]) ? 1 : (uint8_t)((bits >> used[p]) & 1u);
                carried_mask |= (uint32_t)one16[p] << p;
            }
            for (uint32_t q = 0, nq = n_part; q < nq; ++q) {
                const uint16_t in = (uint16_t)(part[q] & carried_mask);
                if (in && in != part[q]) {
                    part[n_part++] = (uint16_t)(part[q] & ~carried_mask);
                    part[q] = in;
                }
            }
            if (c < lower && f >= 2)
                for (size_t p = 0; p < used.size(); ++p)
                    if (one16[p]) need_sequence.emplace(used[p], 0);
            ns.c.push_back(c);
            ns.f.push_back((lb == 1 && f == 1) ? (uint8_t)(f + 1) : f);
            const size_t g16 = n_gt & ~(size_t)15;
            hrow_pairs_ssse3(one16, gl.pos_a.data(), gl.pos_b.data(), hrow, g16);
            for (size_t gi = g16; gi < n_gt; ++gi) hrow[gi] = (uint8_t)(one16[gl.pos_a[gi]] + one16[gl.pos_b[gi]]);
            ++n_kept;
            continue;
        }
        const uint32_t key = key_of[pos];
        const uint8_t c = r.cov[pos];
        const uint8_t f = g_.f[key];
        const int lb = last_bit(key);
        if (filter) {
            uint64_t carried = 0;
            for (uint16_t hap : top) carried += hap_bit(key, hap);
            if (carried == 0) continue;
        }
        kept.push_back(pos);
        const bool in_interval = lb == 1 && c >= lower && c <= upper;
        for (uint16_t hap : used) {
            one[hap] = (in_interval && hap_gt[hap] == 0) ? 1 : hap_bit(key, hap);
            if (one[hap] > 0 && c < lower && f >= 2) need_sequence.emplace(hap, 0);
        }
        ns.c.push_back(c);
        ns.f.push_back((lb == 1 && f == 1) ? (uint8_t)(f + 1) : f);
        if (pairs) {
            for (size_t gi = 0; gi < n_gt; ++gi) hrow[gi] = (uint8_t)(one[flat[2 * gi]] + one[flat[2 * gi + 1]]);
        } else {
            for (size_t gi = 0; gi < n_gt; ++gi) {
                uint8_t h = 0;
                for (uint32_t t = flat_off[gi]; t < flat_off[gi + 1]; ++t) h += one[flat[t]];
                hrow[gi] = h;
            }
        }
        ++n_kept;
    }
    ns.h.resize(n_kept * n_gt);
    while (pf != pf_end) prefetch_one();

    if (fast && need_sequence.empty() && n_kept) {
        uint8_t group[16] = {0};
        for (uint32_t q = 0; q < n_part; ++q)
            for (size_t p = 0; p < used.size(); ++p)
                if ((part[q] >> p) & 1u) group[p] = (uint8_t)q;
        int16_t id_of[256];
        std::memset(id_of, 0xFF, sizeof id_of);
        ns.cls.resize(n_gt);
        for (size_t gi = 0; gi < n_gt; ++gi) {
            const uint8_t a = group[gl.pos_a[gi]], b = group[gl.pos_b[gi]];
            int16_t& id = id_of[a < b ? a * 16 + b : b * 16 + a];
            if (id < 0) {
                id = (int16_t)ns.rep.size();
                ns.rep.push_back((uint16_t)gi);
            }
            ns.cls[gi] = (uint16_t)id;
        }
    }
    if (!need_sequence.empty()) {
        std::unordered_map<uint16_t, std::unordered_set<uint64_t>> hap_keys;
        for (const auto& [hap, unused] : need_sequence) {
            (void)unused;
            const uint16_t gt = hap_gt[hap];
            if (gt >= node.gn->seqs.size())
                throw std::runtime_error("Node '" + chr.name + "-" + std::to_string(node.start) +
                                         "' does not contain sequence information for haplotype " + std::to_string(gt) + ".");
            std::string seq = node.gn->seqs[gt];
            const auto fl = flanks(chr, node_i, hap, gt, seq, g_.k - 1);
            seq = fl.first + seq + fl.second;
            hap_keys[hap] = sequence_keys(seq, g_.k);
        }
        uint32_t si = 0;
        for (uint32_t pos : kept) {
            const uint32_t key = key_of[pos];
            const uint8_t c = r.cov[pos];
            const uint8_t f = g_.f[key];
            if (c > lower || f <= 1) {
                si++;
                continue;
            }
            const int lb = last_bit(key);
            const uint64_t key_hash = g_.keys[key];
            for (size_t gi = 0; gi < n_gt; ++gi) {
                uint8_t& h = ns.h[(size_t)si * n_gt + gi];
                for (uint16_t hap : genotypes[gi]) {
                    const uint8_t o1 = (lb == 1 && hap_gt[hap] == 0 && c >= lower && c <= upper) ? 1 : hap_bit(key, hap);
                    auto it = hap_keys.find(hap);
                    if (it == hap_keys.end() || o1 == 0) continue;
                    if (o1 == 1 && it->second.find(key_hash) == it->second.end()) {
                        if (h >= 1) h--;
                    }
                }
            }
            si++;
        }
    }
    if (filter) {
        if (kept.size() != node.kmers.size()) {
            lists_whole_.store(false, std::memory_order_relaxed);     // the device's whole-list emission path needs whole lists
            alive_stale_.store(true, std::memory_order_relaxed);      // ... and the per-window one the lists as they are now
        }
        node.kmers.keep(kept);
    }
    return ns;
}

Genotyper::EmitPartPlan::~EmitPartPlan() { vgmi_hmm_plan_free(plan); }

// The sequence check of hidden_states() on its own (same conditions, same sets, same strings), for a node whose products stay on the
// device: which entries of the node's list lose which haplotypes.  The fast path's reading of an entry (one 64-bit word: coverage,
// multiplicity, haplotype bits) -- the device's emission kernel reads the same word the same way.
void Genotyper::sequence_fixes(const Chrom& chr, uint32_t node_i, const std::vector<uint16_t>& used, uint64_t gt0_mask, double lower, double upper,
                               const Run& r, std::vector<uint32_t>& fix_j, std::vector<uint64_t>& fix_mask) const
{
    const Node& node = chr.nodes[node_i];
    const std::vector<uint16_t>& hap_gt = node.gn->hap_gt;
    const uint64_t bl = g_.bitlen;
    const uint32_t* const key_of = g_.node_key_index.data();
    // (masks over the places of `used`: 16 for a diploid sample's pairs, up to -n x ploidy <= 64 for a polyploid sample's blocks)
    // bits over `used`: the haplotypes that count as carrying the k-mer (entry_bits.hpp: the packed word, or -- a graph of 7 to 32 bytes of
    // haplotype bits -- the entry's bytes in the graph's bit vectors and the sample's coverage)
    auto carried = [&](uint32_t pos, uint32_t& low_multi) -> uint64_t {
        if (r.packed) return vgh::carried_packed(r.packed[pos], (uint32_t)bl, used.data(), used.size(), gt0_mask, lower, upper, low_multi);
        const uint32_t key = key_of[pos];
        return vgh::carried_bytes(r.cov[pos], (uint8_t)g_.f[key], reinterpret_cast<const uint8_t*>(&g_.bitvec[(size_t)key * bl]), (uint32_t)bl, used.data(),
                                  used.size(), gt0_mask, lower, upper, low_multi);
    };
    uint64_t need = 0;
    for (uint32_t pos : node.kmers) {
        uint32_t lm;
        const uint64_t om = carried(pos, lm);
        if (lm == 2u) need |= om;
    }
    if (!need) return;
    // the needed haplotypes' sequences; haplotypes with the same allele and the same flanks share one (two sequences at most nodes)
    std::vector<std::pair<std::string, std::unordered_set<uint64_t>>> seqs;
    uint8_t which[64] = {0};
    for (size_t p = 0; p < used.size(); ++p) {
        if (!((need >> p) & 1u)) continue;
        const uint16_t hap = used[p], gt = hap_gt[hap];
        if (gt >= node.gn->seqs.size())
            throw std::runtime_error("Node '" + chr.name + "-" + std::to_string(node.start) + "' does not contain sequence information for haplotype " +
                                     std::to_string(gt) + ".");
        std::string seq = node.gn->seqs[gt];
        const auto fl = flanks(chr, node_i, hap, gt, seq, g_.k - 1);
        seq = fl.first + seq + fl.second;
        size_t at = 0;
        while (at < seqs.size() && seqs[at].first != seq) ++at;
        if (at == seqs.size()) {
            std::unordered_set<uint64_t> keys = sequence_keys(seq, g_.k);
            seqs.emplace_back(std::move(seq), std::move(keys));
        }
        which[p] = (uint8_t)at;
    }
    uint32_t j = 0;      // (an entry's index: 32 bits end to end, like entry_count -- graph2node keeps 128 k-mers a node, src/construct_index.cpp:1592-1596, but nothing here relies on it)
    for (uint32_t pos : node.kmers) {
        uint32_t lm;
        const uint64_t om = carried(pos, lm) & need;
        if (lm != 0u && om != 0u) {
            const uint64_t key_hash = g_.keys[key_of[pos]];
            uint64_t drop = 0;
            for (size_t p = 0; p < used.size(); ++p)
                if (((om >> p) & 1u) && seqs[which[p]].second.find(key_hash) == seqs[which[p]].second.end()) drop |= 1ull << p;
            if (drop) {
                fix_j.push_back(j);
                fix_mask.push_back(drop);
            }
        }
        ++j;
    }
}

// ---------------------------------------------------------------- posterior of one node (src/genotype.cpp:1387-1522)
void Genotyper::posterior(Node& n, const std::vector<uint16_t>& top, const Run& r) const
{
    const uint64_t bl = g_.bitlen;
    const uint32_t* const key_of = g_.node_key_index.data();
    uint8_t unique_kmers = 0;
    for (uint32_t pos : n.kmers) {
        if (g_.f[key_of[pos]] > 1) continue;
        if (unique_kmers < UINT8_MAX) unique_kmers++;
    }
    const auto& hap_gt = n.gn->hap_gt;

    // selected haplotype -> (#k-mers it carries, sum of their coverage); any other haplotype reads as (0, 0)
    std::vector<uint64_t> hap_num(n_hap_, 0), hap_sum(n_hap_, 0);
    for (uint32_t pos : n.kmers) {
        if (r.packed) {
            const uint64_t w = r.packed[pos];
            const uint8_t c = (uint8_t)w;
            const uint64_t bits = w >> 16;
            for (uint16_t hap : top) {
                if ((bits >> hap) & 1u) {
                    ++hap_num[hap];
                    hap_sum[hap] += c;
                }
            }
            continue;
        }
        const uint8_t c = r.cov[pos];
        const uint32_t key = key_of[pos];
        for (uint16_t hap : top) {
            if (((uint8_t)g_.bitvec[(size_t)key * bl + (hap >> 3)] >> (hap & 7)) & 1u) {
                ++hap_num[hap];
                hap_sum[hap] += c;
            }
        }
    }

    long double denominator = 0.0L;
    for (const auto& s : n.hmm) denominator += s.a * s.b;

    // The reference sums the posteriors per genotype STRING (alleles as decimal strings, sorted as strings, joined by
    // '/') in a std::map and takes the first maximum in key order.  Few distinct strings occur per node: every entry
    // gets the index of its string, the sums run in entry order exactly as the map's do, and the strings themselves
    // are only built once each.
    struct Distinct { std::string text; long double sum = 0.0L; };
    std::vector<Distinct> distinct;
    std::vector<int32_t> gid(n.hmm.size(), -1);
    uint16_t max_allele = 0;
    for (uint16_t a : hap_gt) max_allele = a > max_allele ? a : max_allele;
    std::vector<std::string> allele_text((size_t)max_allele + 1);   // decimal string per allele number, filled on demand
    std::vector<std::vector<uint16_t>> distinct_alleles;  // sorted (as strings) allele tuple of every distinct string
    std::vector<uint16_t> tuple;
    auto text_of = [&](uint16_t a) -> const std::string& {
        if (allele_text[a].empty()) allele_text[a] = std::to_string(a);
        return allele_text[a];
    };
    // the string of an entry depends on its alleles only: pairs of small allele numbers (the usual case) remember theirs
    const size_t na = (size_t)max_allele + 1;
    std::vector<int32_t> pair_id;
    if (na <= 64) pair_id.assign(na * na, -2);
    for (size_t i = 0; i < n.hmm.size(); ++i) {
        if (!n.hmm[i].haps || n.hmm[i].haps->empty()) continue;
        const auto& haps = *n.hmm[i].haps;
        int32_t* memo = nullptr;
        if (haps.size() == 2 && !pair_id.empty()) {
            memo = &pair_id[(size_t)hap_gt[haps[0]] * na + hap_gt[haps[1]]];
            if (*memo != -2) {
                gid[i] = *memo;
                continue;
            }
        }
        tuple.clear();
        for (uint16_t hap : haps) tuple.push_back(hap_gt[hap]);
        std::sort(tuple.begin(), tuple.end(), [&](uint16_t x, uint16_t y) { return text_of(x) < text_of(y); });
        int32_t id = -1;
        for (size_t d = 0; d < distinct_alleles.size(); ++d)
            if (distinct_alleles[d] == tuple) { id = (int32_t)d; break; }
        if (id < 0) {
            id = (int32_t)distinct.size();
            distinct_alleles.push_back(tuple);
            Distinct e;
            for (size_t t = 0; t < tuple.size(); ++t) {
                e.text += text_of(tuple[t]);
                if (t + 1 != tuple.size()) e.text += "/";
            }
            distinct.push_back(std::move(e));
        }
        gid[i] = id;
        if (memo) *memo = id;
    }
    // (a * b) / denominator of every entry: the same expression in both passes of the reference, evaluated once
    std::vector<long double> post(n.hmm.size());
    for (size_t i = 0; i < n.hmm.size(); ++i) {
        const auto& s = n.hmm[i];
        post[i] = (s.a * s.b) / (long double)denominator;
        if (gid[i] < 0) continue;
        distinct[(size_t)gid[i]].sum += post[i];
    }
    std::vector<size_t> order(distinct.size());
    for (size_t d = 0; d < order.size(); ++d) order[d] = d;
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return distinct[x].text < distinct[y].text; });
    int32_t best_id = -1;
    long double best = -1.0;
    for (size_t d : order) {
        if (distinct[d].sum > best) {
            best = distinct[d].sum;
            best_id = (int32_t)d;
        }
    }

    // the entry with the largest posterior among those of the winning string (the first one on ties) makes the call
    long double max_post = 0.0L;
    size_t winner = n.hmm.size();
    for (size_t i = 0; i < n.hmm.size(); ++i) {
        if (gid[i] < 0 || gid[i] != best_id) continue;
        n.call.probability = best;
        if (max_post < post[i]) {
            max_post = post[i];
            winner = i;
        }
    }
    if (winner != n.hmm.size()) {
        n.call.haps = *n.hmm[winner].haps;
        n.call.kmer_num.clear();
        n.call.kmer_ave_cov.clear();
        for (uint16_t hap : n.call.haps) {
            const uint64_t num = hap < n_hap_ ? hap_num[hap] : 0;
            const uint64_t sum = hap < n_hap_ ? hap_sum[hap] : 0;
            const float ave = (num != 0) ? static_cast<float>(sum) / (float)num : 0.0;
            n.call.kmer_num.push_back(num);
            n.call.kmer_ave_cov.push_back(ave);
        }
        n.call.unique_kmers = unique_kmers;
    }
    std::vector<HmmScore>().swap(n.hmm);
}

// The per-key arrays (coverage, multiplicity, haplotype bits) are indexed by key number, i.e. at random: a node's keys are
// asked for one node ahead of their use
void Genotyper::prefetch_keys(const Node& n, const Run& r) const
{
    if (n.kmers.empty()) return;
    if (r.packed) {      // a node's entries are neighbours (unless an earlier sample pruned the list): one line per 8
        for (size_t j = 0; j < n.kmers.size(); j += 8) __builtin_prefetch(&r.packed[n.kmers[j]]);
        return;
    }
    const uint64_t bl = g_.bitlen;
    __builtin_prefetch(&r.cov[n.kmers[0]]);
    for (uint32_t pos : n.kmers) {
        const uint32_t key = g_.node_key_index[pos];
        __builtin_prefetch(&g_.f[key]);
        __builtin_prefetch(&g_.bitvec[(size_t)key * bl]);
    }
}


// ---------------------------------------------------------------- emission scores of one node (observable_states, :960-1000)
// Scratch and the sample's memoised libm values, one per thread that scores nodes.
struct Genotyper::ScoreCtx {
    float ave = 0;
    double score_up = 0;
    std::vector<long double> pois_tab = std::vector<long double>(256 * 256);
    std::vector<uint8_t> pois_have = std::vector<uint8_t>(256 * 256, 0);
    long double geo_tab[256];
    bool geo_have[256] = {false};
    std::vector<long double> term_buf, class_prod;
    std::vector<uint8_t> term_have;
};

std::vector<long double> Genotyper::score_states(const NodeStates& ns, ScoreCtx& sc) const
{
    const float ave = sc.ave;
    const double score_up = sc.score_up;
    std::vector<long double>& pois_tab = sc.pois_tab;
    std::vector<uint8_t>& pois_have = sc.pois_have;
    long double* const geo_tab = sc.geo_tab;
    bool* const geo_have = sc.geo_have;
    std::vector<long double>& term_buf = sc.term_buf;
    std::vector<long double>& class_prod = sc.class_prod;
    std::vector<uint8_t>& term_have = sc.term_have;
    std::vector<long double> obs;
    const size_t nk = ns.c.size(), ng = ns.n_genotypes;
    if (ng == 0 || nk == 0) return obs;
    // with classes of equivalent genotypes (hidden_states) every column of h equals its class's first member's:
    // those columns alone say which copy numbers occur
    const bool by_class = !ns.rep.empty();
    uint8_t max_h = 0;
    if (by_class) {
        for (size_t j = 0; j < nk; ++j)
            for (uint16_t g : ns.rep) max_h = std::max(max_h, ns.h[j * ng + g]);
    } else {
        for (uint8_t h : ns.h) max_h = h > max_h ? h : max_h;
    }
    const size_t hs = (size_t)max_h + 1;
    // the term of k-mer j under h copies, for the (j, h) that occur
    term_buf.resize(nk * hs);
    // which copy numbers occur for k-mer j: one pass over its row (a term is only evaluated for those, as the
    // reference evaluates it)
    term_have.assign(nk * hs, 0);
    for (size_t j = 0; j < nk; ++j) {
        const uint8_t* hj = &ns.h[j * ng];
        uint8_t* have = &term_have[j * hs];
        if (by_class) {
            for (uint16_t g : ns.rep) have[hj[g]] = 1;
        } else {
            for (size_t gi = 0; gi < ng; ++gi) have[hj[gi]] = 1;
        }
    }
    for (size_t j = 0; j < nk; ++j) {
        for (size_t hh = 0; hh < hs; ++hh) {
            if (!term_have[j * hs + hh]) continue;
            const uint8_t h = (uint8_t)hh;
            uint8_t c = ns.c[j];
            most_likely_depth(h, c, ns.f[j], ave, score_up);
            if (h == 0) {
                if (!geo_have[c]) {
                    geo_tab[c] = geometric(error_param(ave), c);
                    geo_have[c] = true;
                }
                term_buf[j * hs + h] = geo_tab[c];
            } else {
                const size_t slot = (size_t)h * 256 + c;
                if (!pois_have[slot]) {
                    pois_tab[slot] = poisson_pmf(ave * h, c);
                    pois_have[slot] = 1;
                }
                term_buf[j * hs + h] = pois_tab[slot];
            }
        }
    }
    obs.resize(ng);
    if (!ns.rep.empty()) {
        // one product per class of genotypes with the same column of h (the same factors in the same order give the
        // same bits), four classes in x87 registers at a time
        const size_t nc = ns.rep.size();
        std::vector<long double>& prod = class_prod;
        prod.resize(nc);
        size_t ci = 0;
        for (; ci + 4 <= nc; ci += 4) {
            const size_t g0 = ns.rep[ci], g1 = ns.rep[ci + 1], g2 = ns.rep[ci + 2], g3 = ns.rep[ci + 3];
            long double r0 = 1.0L, r1 = 1.0L, r2 = 1.0L, r3 = 1.0L;
            const uint8_t* hj = ns.h.data();
            const long double* t = term_buf.data();
            for (size_t j = 0; j < nk; ++j, hj += ng, t += hs) {
                r0 *= t[hj[g0]];
                r1 *= t[hj[g1]];
                r2 *= t[hj[g2]];
                r3 *= t[hj[g3]];
            }
            prod[ci] = r0;
            prod[ci + 1] = r1;
            prod[ci + 2] = r2;
            prod[ci + 3] = r3;
        }
        for (; ci < nc; ++ci) {
            long double res = 1.0L;
            const size_t g = ns.rep[ci];
            for (size_t j = 0; j < nk; ++j) res *= term_buf[j * hs + ns.h[j * ng + g]];
            prod[ci] = res;
        }
        for (size_t g = 0; g < ng; ++g) obs[g] = prod[ns.cls[g]];
        return obs;
    }
    size_t gi = 0;
    for (; gi + 4 <= ng; gi += 4) {   // four products in x87 registers, each in k-mer order
        long double r0 = 1.0L, r1 = 1.0L, r2 = 1.0L, r3 = 1.0L;
        const uint8_t* hj = &ns.h[gi];
        const long double* t = term_buf.data();
        for (size_t j = 0; j < nk; ++j, hj += ng, t += hs) {
            r0 *= t[hj[0]];
            r1 *= t[hj[1]];
            r2 *= t[hj[2]];
            r3 *= t[hj[3]];
        }
        obs[gi] = r0;
        obs[gi + 1] = r1;
        obs[gi + 2] = r2;
        obs[gi + 3] = r3;
    }
    for (; gi < ng; ++gi) {
        long double res = 1.0L;
        for (size_t j = 0; j < nk; ++j) res *= term_buf[j * hs + ns.h[j * ng + gi]];
        obs[gi] = res;
    }
    return obs;
}

// ---------------------------------------------------------------- what the three paths through the HMM share
namespace {
// every switch of the device paths is on unless its variable starts with '0'
bool knob_off(const char* name)
{
    const char* e = getenv(name);
    return e && e[0] == '0';
}

// ... but for the ones that are asked for: on only if the variable starts with '1'
bool knob_on(const char* name)
{
    const char* e = getenv(name);
    return e && e[0] == '1';
}

void device_check(vgmi_ctx* dev, int rc, const char* what)
{
    if (rc != VGMI_OK) throw std::runtime_error(std::string(what) + vgmi_last_error(dev));
}

struct PartHandle {
    vgmi_hmm_part* p = nullptr;
    ~PartHandle() { vgmi_hmm_part_free(p); }
};

// fn(0) .. fn(n - 1) on `threads` threads, the caller's among them: a thread token and `spent` per item; the first error is thrown
// once every thread has ended
void over_windows(size_t n, size_t threads, std::atomic<long long>& spent, const std::function<void(size_t)>& fn)
{
    std::atomic<size_t> next{0};
    std::string err;
    std::mutex mu;
    auto body = [&]() {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= n) return;
            try {
                CpuBudget::Hold cpu;
                PhaseTimer tt(spent);
                fn(i);
            } catch (const std::exception& e) {
                std::lock_guard<std::mutex> lock(mu);
                if (err.empty()) err = e.what();
            }
        }
    };
    std::vector<std::thread> helpers;
    for (size_t h = 1; h < threads; ++h) helpers.emplace_back(body);
    body();
    for (auto& th : helpers) th.join();
    if (!err.empty()) throw std::runtime_error(err);
}

// how many haplotypes two sorted genotypes share (the size of their std::set_intersection)
int32_t shared_haplotypes(const std::vector<uint16_t>& a, const std::vector<uint16_t>& b)
{
    int32_t n = 0;
    for (size_t x = 0, y = 0; x < a.size() && y < b.size();) {
        if (a[x] < b[y]) ++x;
        else if (b[y] < a[x]) ++y;
        else { ++n; ++x; ++y; }
    }
    return n;
}

std::vector<uint8_t> keep_matrix(const std::vector<std::vector<uint16_t>>& genotypes)
{
    const size_t n_gt = genotypes.size();
    std::vector<uint8_t> keep_mat(n_gt * n_gt);
    for (size_t i = 0; i < n_gt; ++i)
        for (size_t j = 0; j < n_gt; ++j) keep_mat[i * n_gt + j] = (uint8_t)shared_haplotypes(genotypes[i], genotypes[j]);
    return keep_mat;
}

// the sample's libm values for the emission kernel: geometric(error_param(ave), c) for h = 0, poisson(ave * h, c) for h = 1 .. ploidy
// `-m fre`: a window's table of factors for the device recursion (vgmi_hmm_recursion_fre) -- per genotype its haplotypes' scores, the
// window's normalised gamma draws (HaplotypeSampler::score: hapIdxScoreMap), in the genotype's order, widened (exact).  A haplotype the
// window did not draw has no score: where the host's recursion would have stopped (src/genotype.cpp:1203-1207), this stops.
std::vector<long double> frequency_table(const std::vector<std::vector<uint16_t>>& genotypes, const std::unordered_map<uint16_t, double>& score)
{
    std::vector<long double> table;
    for (const auto& haps : genotypes)
        for (uint16_t hap : haps) {
            auto it = score.find(hap);
            if (it == score.end()) throw std::runtime_error("'" + std::to_string(hap) + "' does not exist in 'hapIdxScoreMap'.");
            table.push_back((long double)it->second);
        }
    return table;
}

std::vector<long double> emission_table(float ave, uint32_t ploidy)
{
    std::vector<long double> tab((size_t)(ploidy + 1) * 256);
    for (int c = 0; c < 256; ++c) {
        tab[c] = geometric(error_param(ave), (uint8_t)c);
        for (uint8_t h = 1; h <= ploidy; ++h) tab[(size_t)h * 256 + c] = poisson_pmf(ave * h, (uint8_t)c);
    }
    return tab;
}

// ---- a site's VCF line (src/genotype.cpp:1628-1690)
using SiteMap = std::map<uint32_t, std::vector<std::string>>;

// CHROM .. INFO with FILTER forced PASS, FORMAT and the tab behind it; false (nothing appended): the VCF has no such site
bool append_site_head(std::string& out, const std::vector<std::string>* fields)
{
    if (!fields) return false;
    for (size_t i = 0; i < 9; i++) {
        if (i == 0) out += (*fields)[i];
        else if (i == 6) out += "\tPASS";
        else if (i < 8) { out += '\t'; out += (*fields)[i]; }
        else out += "\tGT:GQ:GPP:NAK:CAK:UK";
    }
    out += '\t';
    return true;
}

void append_sample_field(std::string& out, const uint64_t* gt, size_t n_alleles, bool no_call, float gq, long double probability, const uint64_t* kmer_num,
                         const float* kmer_ave_cov, size_t n_counts, uint8_t unique_kmers)
{
    for (size_t i = 0; i < n_alleles; ++i) {
        if (i) out += '/';
        if (no_call) out += '.';
        else append_uint(out, gt[i]);
    }
    out += ':';
    append_fixed1(out, gq);
    out += ':';
    append_fixed1(out, probability);
    out += ':';
    for (size_t i = 0; i < n_counts; ++i) {
        if (i) out += ',';
        append_uint(out, kmer_num[i]);
    }
    out += ':';
    for (size_t i = 0; i < n_counts; i++) {
        if (i) out += ',';
        append_fixed1(out, kmer_ave_cov[i]);
    }
    out += ':';
    append_uint(out, unique_kmers);
    out += '\n';
}

// A call's line straight from what the device sent back -- the alleles of the `ploidy` (2 .. kTallyPloidyMax) called haplotypes, the posterior, the
// tallies (k-mers, coverage sum per called haplotype: tl[2 q], tl[2 q + 1]) -- without the detour through the node's call record
// (window_finish writes it, write_piece reads it back: two walks over half a million scattered nodes per sample).  An all-reference call
// has no line.  head(out) as append_site_head.
// (The device tallies calls of up to kTallyPloidyMax haplotypes, vgmi_hmm_tallies_ploidy; a call of more keeps the host's walk over the
// called nodes' lists -- finish_rows, window_finish -- and never comes here: device_tally_ploidy() is what both callers ask.)
constexpr uint32_t kTallyPloidyMax = 4;
inline bool device_tally_ploidy(uint32_t ploidy) { return ploidy >= 3 && ploidy <= kTallyPloidyMax; }
template <class HapGt, class Head>
void append_tally_line(std::string& out, const HapGt& hap_gt, const uint16_t* called, uint32_t ploidy, long double probability, const uint32_t* tl,
                       uint8_t unique_kmers, float min_gq, Head&& head)
{
    if (ploidy > kTallyPloidyMax) throw std::runtime_error("internal: a tally line for a call of more haplotypes than the device tallies");
    uint64_t gt[kTallyPloidyMax], num[kTallyPloidyMax];
    float cov[kTallyPloidyMax];
    bool all_ref = true;
    for (uint32_t q = 0; q < ploidy; ++q) {
        gt[q] = (uint64_t)hap_gt[called[q]];
        all_ref = all_ref && gt[q] == 0;
        num[q] = tl[2 * q];
        cov[q] = tl[2 * q] ? static_cast<float>((uint64_t)tl[2 * q + 1]) / (float)(uint64_t)tl[2 * q] : 0.0f;
    }
    if (all_ref || !head(out)) return;
    const float gq = phred_scaled(probability);
    append_sample_field(out, gt, ploidy, gq < min_gq, gq, probability, num, cov, ploidy, unique_kmers);
}

// A window's nodes come in the order of their start, as the sites of the map do: one walk along the map instead of a search from its
// root per node (0.4 thread-seconds per chr20-scale sample were these searches)
struct SiteWalk {
    const SiteMap& sites;
    SiteMap::const_iterator site;
    uint32_t prev_start = UINT32_MAX;      // (the first node is searched for; a node in front of the last one, too -- never, with node lists as graph.bin holds them)
    explicit SiteWalk(const SiteMap& s) : sites(s), site(s.end()) {}
    const std::vector<std::string>* at(uint32_t start)      // nullptr: no site at `start`
    {
        if (start < prev_start) site = sites.lower_bound(start);
        prev_start = start;
        while (site != sites.end() && site->first < start) ++site;
        return site == sites.end() || site->first != start ? nullptr : &site->second;
    }
};
}  // namespace

// the line of a node's call, if it has one with a non-reference allele; gt: scratch; head(out) as append_site_head
template <class Head>
void Genotyper::append_call_line(std::string& out, const Node& node, float min_gq, std::vector<uint64_t>& gt, Head&& head)
{
    const SiteCall& call = node.call;
    if (call.haps.empty()) return;
    gt.clear();
    bool all_ref = true;
    for (uint16_t hap : call.haps) {
        gt.push_back((uint64_t)node.gn->hap_gt[hap]);
        all_ref = all_ref && gt.back() == 0;
    }
    if (all_ref || !head(out)) return;
    const float gq = phred_scaled(call.probability);
    append_sample_field(out, gt.data(), gt.size(), gq < min_gq, gq, call.probability, call.kmer_num.data(), call.kmer_ave_cov.data(), call.kmer_num.size(),
                        call.unique_kmers);
}

const Genotyper::SiteMap& Genotyper::vcf_sites(const Chrom& chr) const
{
    auto vcf_chr = g_.vcf_info.find(chr.name);
    if (vcf_chr == g_.vcf_info.end()) throw std::runtime_error("'" + chr.name + "' does not exist in the VCF file.");
    return vcf_chr->second;
}

// which nodes the HMM passes over: those with one allele and, under --sv, those whose alleles are all shorter than 50 bases
bool Genotyper::skipped(const Chrom& chr, const SiteMap& sites, const Node& n, bool sv_only)
{
    if (n.gn->hap_gt.size() <= 1) return true;
    if (sv_only) {
        auto site = sites.find(n.start);
        if (site == sites.end()) throw std::runtime_error("'" + chr.name + ":" + std::to_string(n.start) + "' does not exist in the VCF file.");
        if (site->second[3].size() < 50 && site->second[4].size() < 50) return true;
    }
    return false;
}

// used: the haplotypes occurring in `genotypes`, ascending
Genotyper::GenotypeList Genotyper::genotype_list(const std::vector<std::vector<uint16_t>>& genotypes, const std::vector<uint16_t>& used)
{
    const size_t n_gt = genotypes.size();
    GenotypeList glist;
    glist.off.assign(n_gt + 1, 0);
    for (size_t gi = 0; gi < n_gt; ++gi) {
        glist.flat.insert(glist.flat.end(), genotypes[gi].begin(), genotypes[gi].end());
        glist.off[gi + 1] = (uint32_t)glist.flat.size();
        glist.pairs = glist.pairs && genotypes[gi].size() == 2;
    }
    if (glist.pairs && used.size() <= 16) {
        std::unordered_map<uint16_t, uint8_t> where;
        for (size_t p = 0; p < used.size(); ++p) where[used[p]] = (uint8_t)p;
        glist.pos_a.resize(n_gt);
        glist.pos_b.resize(n_gt);
        for (size_t gi = 0; gi < n_gt; ++gi) {
            glist.pos_a[gi] = where[glist.flat[2 * gi]];
            glist.pos_b[gi] = where[glist.flat[2 * gi + 1]];
        }
    }
    return glist;
}

// The step tables of a window's two chains, forward (the nodes in order) and backward (from the last): per step the powers
// no_recomb^0..ploidy, recomb^0..ploidy of the gap to the node before it in the chain, whether the chain restarts there, and its row;
// per scored node the steps that hold its alpha and its beta.  pw / row / restart point at the window's first step, which is step
// `step0` of the arrays the device gets; a node's row is row_base + at, fwd / bwd are indexed by `at`.
void Genotyper::step_tables(const std::vector<Seen>& seen, uint32_t stride, uint16_t population, size_t step0, size_t row_base, long double* pw,
                            uint32_t* row, uint8_t* restart, uint64_t* fwd, uint64_t* bwd)
{
    size_t m = 0;
    for (const Seen& sn : seen) m += sn.at >= 0;
    if (!m) return;
    // the tables of powers are a function of the distance alone: neighbouring nodes are tens to hundreds of bases apart, so a window's
    // few thousand steps share a few hundred distinct tables (same libm calls, each made once)
    constexpr uint32_t kMemo = 4096;
    std::vector<long double> memo(pw ? (size_t)kMemo * 2 * stride : 0);
    std::vector<uint8_t> memo_have(kMemo, 0);
    auto powers = [&](long double* dst, uint32_t distance) {
        if (!pw) return;      // transitions by haplotype frequency: no powers
        if (distance < kMemo && memo_have[distance]) {
            std::memcpy(dst, &memo[(size_t)distance * 2 * stride], 2 * stride * sizeof(long double));
            return;
        }
        long double recomb, no_recomb;
        std::tie(recomb, no_recomb) = transition_probabilities(distance, population);
        for (uint32_t k = 0; k < stride; ++k) {
            dst[k] = std::pow(no_recomb, (int32_t)k);
            dst[stride + k] = std::pow(recomb, (int32_t)k);
        }
        if (distance < kMemo) {
            std::memcpy(&memo[(size_t)distance * 2 * stride], dst, 2 * stride * sizeof(long double));
            memo_have[distance] = 1;
        }
    };
    size_t j = 0;
    for (size_t q = 0; q < seen.size(); ++q) {
        if (seen[q].at < 0) continue;
        const size_t fs = j, bs = m + (m - 1 - j);     // its forward and its backward step
        // forward: the node in front (prev_end = 0 in front of the first); the chain restarts behind a node without scores
        powers(pw ? pw + fs * 2 * stride : nullptr, seen[q].start - (q ? seen[q - 1].end : 0u));
        restart[fs] = (q == 0 || seen[q - 1].at < 0) ? 1 : 0;
        row[fs] = (uint32_t)(row_base + seen[q].at);
        // backward: the node behind (prev_start = 0 behind the last)
        powers(pw ? pw + bs * 2 * stride : nullptr, (q + 1 < seen.size() ? seen[q + 1].start : 0u) - seen[q].end);
        restart[bs] = (q + 1 == seen.size() || seen[q + 1].at < 0) ? 1 : 0;
        row[bs] = (uint32_t)(row_base + seen[q].at);
        fwd[seen[q].at] = step0 + fs;
        bwd[seen[q].at] = step0 + bs;
        ++j;
    }
}

// ---------------------------------------------------------------- one window: selection, forward, backward, posterior
void Genotyper::window(Chrom& chr, uint32_t first, uint32_t last, const Run& r, WindowWork* work, const std::vector<uint16_t>* forced_top)
{
    const GenotypeConfig& cfg = *r.cfg;
    const SiteMap& sites = vcf_sites(chr);
    if (first >= chr.nodes.size()) return;

    // ---- haplotype selection (src/genotype.cpp:500-610)
    std::unique_ptr<PhaseTimer> t_select(new PhaseTimer(g_phase.select));
    std::vector<uint16_t> top;
    if (n_hap_ <= r.haploid_num)
        for (const auto& kv : g_.hap_names) top.push_back(kv.first);
    std::vector<uint32_t> support(n_hap_, 0);
    const uint64_t bl = g_.bitlen;
    for (uint32_t i = first; i < last; ++i) {
        const Node& n = chr.nodes[i];
        if (n.gn->hap_gt.size() == 1) continue;
        {
            uint32_t nx = i + 1;
            while (nx < last && chr.nodes[nx].gn->hap_gt.size() == 1) ++nx;
            if (nx < last) prefetch_keys(chr.nodes[nx], r);
        }
        if (r.packed) {
            for (uint32_t pos : n.kmers) {
                const uint64_t w = r.packed[pos];
                const uint8_t c = (uint8_t)w;
                if (c <= 1 || (uint8_t)(w >> 8) > 1) continue;
                const uint64_t bits = w >> 16;
                for (const uint16_t hap : hap_ids_)
                    if ((bits >> hap) & 1u) support[hap] += c;
            }
            continue;
        }
        for (uint32_t pos : n.kmers) {
            const uint32_t key = g_.node_key_index[pos];
            const uint8_t c = r.cov[pos];
            if (c <= 1 || g_.f[key] > 1) continue;
            const uint8_t* bits = reinterpret_cast<const uint8_t*>(g_.bitvec.data()) + (size_t)key * bl;
            for (const uint16_t hap : hap_ids_)
                if ((bits[hap >> 3] >> (hap & 7)) & 1u) support[hap] += c;
        }
    }
    HaplotypeSampler sampler(support, (int)r.haploid_num);
    if (top.empty()) top = sampler.top;
    if (forced_top) top = *forced_top;
    std::sort(top.begin(), top.end());
    const std::unordered_map<uint16_t, double>& hap_score = sampler.score;
    t_select.reset();

    double lower = 256.0f, upper = -0.1f;
    poisson_interval(r.hap_cov, lower, upper);

    auto skipped = [&](const Node& n) { return Genotyper::skipped(chr, sites, n, cfg.sv_only); };
    // emission score of every genotype of a node (observable_states, :960-1000).  poisson(ave * h, c) and
    // geometric(p, c) are pure functions of (h, c) within a sample: evaluated once each (the values, and therefore
    // the products, are the reference's bit for bit)
    const float ave = r.hap_cov;
    double score_lo = 256.0f, score_up = -0.1f;
    poisson_interval(ave, score_lo, score_up);
    // genotypes of this window, the haplotypes they use, and how many haplotypes two genotypes share (the size of
    // std::set_intersection of the two sorted vectors)
    const std::vector<std::vector<uint16_t>> genotypes =
        haplotype_combinations(top, cfg.sample_type, cfg.sample_ploidy, (uint16_t)(n_hap_ - 1));
    const size_t n_gt = genotypes.size();
    std::vector<uint16_t> used;
    for (const auto& gtv : genotypes) used.insert(used.end(), gtv.begin(), gtv.end());
    std::sort(used.begin(), used.end());
    used.erase(std::unique(used.begin(), used.end()), used.end());
    const GenotypeList glist = genotype_list(genotypes, used);
    bool all_full = true;   // every genotype has `ploidy` haplotypes
    for (const auto& gtv : genotypes) all_full = all_full && gtv.size() == (size_t)cfg.sample_ploidy;
    const std::vector<uint8_t> keep_mat = keep_matrix(genotypes);

    // emission score of every genotype of a node; empty when the node has no k-mer left (every genotype is skipped).
    // Every genotype's score is the product of its k-mers' terms in k-mer order (observable_states); walking the
    // k-mers in the outer loop keeps that order per genotype and turns one long dependent multiply chain per
    // genotype into n_genotypes independent ones.  A k-mer's term depends on the genotype only through h.
    ScoreCtx sctx;
    sctx.ave = ave;
    sctx.score_up = score_up;
    auto score_states = [&](const NodeStates& ns) -> std::vector<long double> { return this->score_states(ns, sctx); };
    // one step of the forward (alpha) or backward (beta) recursion (:1170-1380); obs[i] = emission of genotype i
    auto recursion = [&](const std::vector<HmmScore>& prev, bool use_alpha, long double recomb, long double no_recomb,
                         const std::vector<long double>& obs) -> std::vector<long double> {
        // pow(no_recomb, keep) and pow(recomb, change) take ploidy + 1 distinct values each per node
        const int32_t max_n = (int32_t)cfg.sample_ploidy;
        std::vector<long double> pow_keep(max_n + 1), pow_change(max_n + 1);
        const bool by_score = recomb == 0.0L && no_recomb == 0.0L;
        if (!by_score)
            for (int32_t i = 0; i <= max_n; ++i) {
                pow_keep[i] = std::pow(no_recomb, i);
                pow_change[i] = std::pow(recomb, i);
            }
        const bool aligned = prev.size() == n_gt;   // the previous node's entries are this window's genotypes, in order
        // (prev * pow(no_recomb, keep)) * pow(recomb, change) does not depend on the genotype being scored: one value
        // per previous entry and number of shared haplotypes -- the same two roundings, taken out of the inner loop
        std::vector<long double> step;
        if (!by_score && aligned) {
            step.resize(prev.size() * (size_t)(max_n + 1));
            for (size_t pi = 0; pi < prev.size(); ++pi) {
                const long double pv = use_alpha ? prev[pi].a : prev[pi].b;
                for (int32_t keep = 0; keep <= max_n; ++keep) {
                    const int32_t change = max_n - keep;   // every genotype has `ploidy` haplotypes
                    step[pi * (size_t)(max_n + 1) + keep] = pv * pow_keep[keep] * pow_change[change];
                }
            }
        }
        std::vector<long double> out;
        out.reserve(obs.size());
        long double total = 0.0L;
        size_t gi0 = 0;
        if (!prev.empty() && !by_score && aligned && all_full) {
            // three genotypes at a time: each sum still adds its terms in the order of the previous entries, but three
            // independent x87 add chains are in flight instead of one (three accumulators and their three emission
            // factors fill the register stack; a fourth chain would spill the factors to 80-bit memory operands)
            const size_t stride = (size_t)(max_n + 1);
            for (; gi0 + 3 <= obs.size(); gi0 += 3) {
                const uint8_t* k0 = &keep_mat[gi0 * n_gt];
                const uint8_t* k1 = k0 + n_gt;
                const uint8_t* k2 = k1 + n_gt;
                const long double o0 = obs[gi0], o1 = obs[gi0 + 1], o2 = obs[gi0 + 2];
                long double r0 = 0.0L, r1 = 0.0L, r2 = 0.0L;
                const long double* sp = step.data();
                for (size_t pi = 0; pi < prev.size(); ++pi, sp += stride) {
                    r0 += sp[k0[pi]] * o0;
                    r1 += sp[k1[pi]] * o1;
                    r2 += sp[k2[pi]] * o2;
                }
                out.push_back(r0);
                total += r0;
                out.push_back(r1);
                total += r1;
                out.push_back(r2);
                total += r2;
            }
        }
        for (size_t gi = gi0; gi < obs.size(); ++gi) {
            const std::vector<uint16_t>& haps = genotypes[gi];
            const int32_t hap_num = (int32_t)haps.size();
            long double res = 0.0L;
            if (prev.empty()) {
                res += obs[gi];
            } else if (!by_score && aligned && hap_num == max_n) {
                const uint8_t* km = &keep_mat[gi * n_gt];
                const long double o = obs[gi];
                const size_t stride = (size_t)(max_n + 1);
                for (size_t pi = 0; pi < prev.size(); ++pi) res += step[pi * stride + km[pi]] * o;
            } else {
                for (size_t pi = 0; pi < prev.size(); ++pi) {
                    const HmmScore& p = prev[pi];
                    const long double pv = use_alpha ? p.a : p.b;
                    if (by_score) {
                        long double t = pv * obs[gi];
                        for (uint16_t hap : haps) {
                            auto it = hap_score.find(hap);
                            if (it == hap_score.end())
                                throw std::runtime_error("'" + std::to_string(hap) + "' does not exist in 'hapIdxScoreMap'.");
                            t *= it->second;
                        }
                        res += t;
                    } else {
                        const int32_t keep = aligned ? (int32_t)keep_mat[gi * n_gt + pi] : shared_haplotypes(haps, *p.haps);
                        const int32_t change = hap_num - keep;
                        const long double pk = keep <= max_n ? pow_keep[keep] : std::pow(no_recomb, keep);
                        const long double pc = (change >= 0 && change <= max_n) ? pow_change[change] : std::pow(recomb, change);
                        res += pv * pk * pc * obs[gi];
                    }
                }
            }
            out.push_back(res);
            total += res;
        }
        if (total > 0.0L) {
            for (auto& x : out) x = x / total;
        } else {
            const long double uniform = 1.0L / (long double)out.size();
            for (auto& x : out) x = uniform;
        }
        return out;
    };

    // ---- forward.  The emissions are kept for the backward pass: it would recompute exactly the same hidden states
    // (it runs on the k-mer lists this pass has just pruned, with the same coverage and the same genotypes).
    // Device recursion: this pass fills hidden states, emission scores and the libm tables of every node; the recursion
    // itself and the posterior follow in window_finish() (the pruning of a node's k-mer list depends on the window's
    // haplotypes, not on alpha, so nothing here waits for the recursion)
    const bool to_device = work != nullptr && work->obs != nullptr && n_gt == work->n_gt && cfg.transition == "rec" && all_full && n_gt <= 2048 &&
                           cfg.sample_ploidy >= 1 && cfg.sample_ploidy <= 8;    // 2048: VGMI_HMM_MAX_GT (csrc/vgmi_kernels.h)
    if (to_device) {
        std::vector<Seen> seen;      // at: the node's place in work->nodes
        NodeStates st;
        for (uint32_t i = first; i < last; ++i) {
            Node& n = chr.nodes[i];
            if (skipped(n)) continue;
            const uint32_t n_start = n.start;
            const uint32_t n_end = (uint32_t)(n_start + n.gn->seqs[0].size() - 1);
            {
                PhaseTimer t(g_phase.states);
                uint32_t nx = i + 1;
                while (nx < last && skipped(chr.nodes[nx])) ++nx;
                st = hidden_states(chr, i, top, genotypes, used, glist, lower, upper, true, r, std::move(st), nx < last ? &chr.nodes[nx] : nullptr);
            }
            std::vector<long double> obs;
            {
                PhaseTimer t(g_phase.emit);
                obs = score_states(st);
            }
            if (obs.empty()) {
                seen.push_back(Seen{n_start, n_end, -1});
                continue;
            }
            seen.push_back(Seen{n_start, n_end, (int64_t)work->nodes.size()});
            if (work->nodes.size() >= work->room || obs.size() != n_gt) throw std::runtime_error("internal: device HMM window larger than announced");
            std::memcpy(work->obs + work->nodes.size() * n_gt, obs.data(), n_gt * sizeof(long double));
            if (!genotype_strings(n, genotypes, work->gid + work->nodes.size() * n_gt, work->order + work->nodes.size() * n_gt)) {
                // more distinct genotype strings at this node than the device's byte-sized ids hold (> 255: dozens of alleles
                // under hundreds of genotypes): the host takes the window, with the haplotypes already drawn
                work->nodes.clear();
                work->on_device = false;
                window(chr, first, last, r, nullptr, &top);
                return;
            }
            work->nodes.push_back(i);
        }
        step_tables(seen, cfg.sample_ploidy + 1, (uint16_t)n_hap_, work->step0, work->row0, work->pw, work->row, work->restart, work->fwd_step, work->bwd_step);
        work->chr = &chr;
        work->on_device = true;
        work->n_gt = n_gt;
        work->ploidy = cfg.sample_ploidy;
        work->top = top;
        work->keep_mat = keep_mat;
        work->genotypes = genotypes;
        return;
    }
    std::vector<std::vector<long double>> emissions(last - first);
    const std::vector<HmmScore> no_prev;
    const std::vector<HmmScore>* prev = &no_prev;   // the entries of the node scored before this one
    uint32_t prev_start = 0, prev_end = 0;
    NodeStates states;
    for (uint32_t i = first; i < last; ++i) {
        Node& n = chr.nodes[i];
        if (skipped(n)) continue;
        const uint32_t n_start = n.start;
        const uint32_t n_end = (uint32_t)(n_start + n.gn->seqs[0].size() - 1);
        {
            PhaseTimer t(g_phase.states);
            uint32_t nx = i + 1;        // the node that is worked on next (nodes with one allele are passed over)
            while (nx < last && skipped(chr.nodes[nx])) ++nx;
            states = hidden_states(chr, i, top, genotypes, used, glist, lower, upper, true, r, std::move(states),
                                   nx < last ? &chr.nodes[nx] : nullptr);
        }
        long double recomb = 0.0L, no_recomb = 0.0L;
        if (cfg.transition == "rec") std::tie(recomb, no_recomb) = transition_probabilities(n_start - prev_end, (uint16_t)n_hap_);
        std::vector<long double>& obs = emissions[i - first];
        {
            PhaseTimer t(g_phase.emit);
            obs = score_states(states);
        }
        std::unique_ptr<PhaseTimer> t_fwd(new PhaseTimer(g_phase.fwd));
        const std::vector<long double> alpha = recursion(*prev, true, recomb, no_recomb, obs);
        t_fwd.reset();
        n.hmm.resize(alpha.size());
        for (size_t j = 0; j < alpha.size(); ++j) {
            n.hmm[j].a = alpha[j];
            n.hmm[j].haps = &genotypes[j];
        }
        prev_start = n_start;
        prev_end = n_end;
        prev = &n.hmm;
    }
    // ---- backward, and the posterior of a node as soon as the node in front of it has used its beta (its alpha / beta
    // entries are still in the cache then; the posterior of one node does not depend on any other's)
    prev = &no_prev;
    prev_start = 0;
    prev_end = 0;
    Node* due = nullptr;
    for (uint32_t i = last; i-- > first;) {
        Node& n = chr.nodes[i];
        if (skipped(n)) continue;
        prefetch_keys(n, r);
        const uint32_t n_start = n.start;
        const uint32_t n_end = (uint32_t)(n_start + n.gn->seqs[0].size() - 1);
        long double recomb = 0.0L, no_recomb = 0.0L;
        if (cfg.transition == "rec") std::tie(recomb, no_recomb) = transition_probabilities(prev_start - n_end, (uint16_t)n_hap_);
        std::unique_ptr<PhaseTimer> t_bwd(new PhaseTimer(g_phase.bwd));
        const std::vector<long double> beta = recursion(*prev, false, recomb, no_recomb, emissions[i - first]);
        t_bwd.reset();
        for (size_t j = 0; j < beta.size(); ++j) n.hmm[j].b = beta[j];
        std::vector<long double>().swap(emissions[i - first]);
        if (due) {
            PhaseTimer t(g_phase.post);
            posterior(*due, top, r);
        }
        due = &n;
        prev_start = n_start;
        prev_end = n_end;
        prev = &n.hmm;
    }
    (void)prev_end;
    if (due) {
        PhaseTimer t(g_phase.post);
        posterior(*due, top, r);
    }
}

// The genotype STRING of every entry of a node (posterior(): alleles as decimal strings, sorted as strings, joined by '/'),
// as small numbers in order of first appearance, and those numbers in string order (0xFF behind the last): what the
// device's posterior groups and ranks by.
bool Genotyper::genotype_strings(const Node& n, const std::vector<std::vector<uint16_t>>& genotypes, uint8_t* gid, uint8_t* order) const
{
    const auto& hap_gt = n.gn->hap_gt;
    uint16_t max_allele = 0;
    for (uint16_t a : hap_gt) max_allele = a > max_allele ? a : max_allele;
    std::vector<std::string> allele_text((size_t)max_allele + 1);
    auto text_of = [&](uint16_t a) -> const std::string& {
        if (allele_text[a].empty()) allele_text[a] = std::to_string(a);
        return allele_text[a];
    };
    std::vector<std::string> texts;
    std::vector<std::vector<uint16_t>> tuples;
    const size_t na = (size_t)max_allele + 1;
    std::vector<int32_t> pair_id;
    if (na <= 64) pair_id.assign(na * na, -2);
    std::vector<uint16_t> tuple;
    for (size_t i = 0; i < genotypes.size(); ++i) {
        const auto& haps = genotypes[i];
        int32_t* memo = nullptr;
        if (haps.size() == 2 && !pair_id.empty()) {
            memo = &pair_id[(size_t)hap_gt[haps[0]] * na + hap_gt[haps[1]]];
            if (*memo != -2) {
                gid[i] = (uint8_t)*memo;
                continue;
            }
        }
        tuple.clear();
        for (uint16_t hap : haps) tuple.push_back(hap_gt[hap]);
        std::sort(tuple.begin(), tuple.end(), [&](uint16_t x, uint16_t y) { return text_of(x) < text_of(y); });
        int32_t id = -1;
        for (size_t d = 0; d < tuples.size(); ++d)
            if (tuples[d] == tuple) { id = (int32_t)d; break; }
        if (id < 0) {
            id = (int32_t)tuples.size();
            if (id >= 255) return false;      // 0xFF ends the order list
            tuples.push_back(tuple);
            std::string t;
            for (size_t q = 0; q < tuple.size(); ++q) {
                t += text_of(tuple[q]);
                if (q + 1 != tuple.size()) t += "/";
            }
            texts.push_back(std::move(t));
        }
        gid[i] = (uint8_t)id;
        if (memo) *memo = id;
    }
    std::vector<size_t> by_text(texts.size());
    for (size_t d = 0; d < by_text.size(); ++d) by_text[d] = d;
    std::sort(by_text.begin(), by_text.end(), [&](size_t x, size_t y) { return texts[x] < texts[y]; });
    for (size_t q = 0; q < genotypes.size(); ++q) order[q] = q < by_text.size() ? (uint8_t)by_text[q] : 0xFF;
    return true;
}

// the device's verdict on the nodes of a window prepared by window(): probability of the winning genotype string and the
// entry that makes the call, per node; the rest of the call (k-mer counts of its haplotypes) as posterior() fills it
// tally / uniq (optional, diploid calls): per node of the window the device's tallies (vgmi_hmm_tallies) -- (k-mers, coverage sum) of
// the two called haplotypes and the count of single-copy k-mers -- instead of the walk over the node's k-mer list
void Genotyper::window_finish(WindowWork& w, const long double* prob, const uint32_t* winner, const Run& r, const uint32_t* tally, const uint8_t* uniq)
{
    const uint64_t bl = g_.bitlen;
    // posterior() tallies the SELECTED haplotypes (w.top); a called haplotype outside the selection -- the reference haplotype,
    // which every genotype list may hold, when -n picked fewer haplotypes than the panel has -- reads as (0, 0) there and here
    std::vector<uint8_t> selected(n_hap_, 0);
    for (uint16_t hap : w.top)
        if (hap < n_hap_) selected[hap] = 1;
    for (size_t j = 0; j < w.nodes.size(); ++j) {
        if (winner[j] >= w.n_gt) continue;            // no entry with a positive posterior: no call
        PhaseTimer t(g_phase.post);
        Node& n = w.chr->nodes[w.nodes[j]];
        // k-mer count and coverage sum of the CALLED haplotypes only (posterior() tallies every selected haplotype and then reads
        // the called ones: the same numbers for a seventh of the work at 15 haplotypes)
        const std::vector<uint16_t>& called = w.genotypes[winner[j]];
        uint64_t num[8] = {0}, sum[8] = {0};
        const size_t nc = std::min<size_t>(called.size(), 8);
        uint8_t unique_kmers = 0;
        const bool from_device = tally && called.size() == 2;
        if (from_device) {
            num[0] = tally[4 * j];
            sum[0] = tally[4 * j + 1];
            num[1] = tally[4 * j + 2];
            sum[1] = tally[4 * j + 3];
            unique_kmers = uniq[j];
        } else if (j + 1 < w.nodes.size()) prefetch_keys(w.chr->nodes[w.nodes[j + 1]], r);
        if (!from_device)
        for (uint32_t pos : n.kmers) {
            if (r.packed) {
                const uint64_t word = r.packed[pos];
                if ((uint8_t)(word >> 8) <= 1 && unique_kmers < UINT8_MAX) unique_kmers++;
                const uint8_t c = (uint8_t)word;
                const uint64_t bits = word >> 16;
                for (size_t q = 0; q < nc; ++q)
                    if (called[q] < n_hap_ && selected[called[q]] && ((bits >> called[q]) & 1u)) {
                        ++num[q];
                        sum[q] += c;
                    }
                continue;
            }
            const uint32_t key = g_.node_key_index[pos];
            if (g_.f[key] <= 1 && unique_kmers < UINT8_MAX) unique_kmers++;
            const uint8_t c = r.cov[pos];
            for (size_t q = 0; q < nc; ++q)
                if (called[q] < n_hap_ && selected[called[q]] && (((uint8_t)g_.bitvec[(size_t)key * bl + (called[q] >> 3)] >> (called[q] & 7)) & 1u)) {
                    ++num[q];
                    sum[q] += c;
                }
        }
        n.call.probability = prob[j];
        n.call.haps = called;
        n.call.kmer_num.clear();
        n.call.kmer_ave_cov.clear();
        for (size_t q = 0; q < called.size(); ++q) {
            const uint64_t nq = q < nc ? num[q] : 0, sq = q < nc ? sum[q] : 0;
            const float ave = (nq != 0) ? static_cast<float>(sq) / (float)nq : 0.0;
            n.call.kmer_num.push_back(nq);
            n.call.kmer_ave_cov.push_back(ave);
        }
        n.call.unique_kmers = unique_kmers;
    }
}

// ---------------------------------------------------------------- driver + VCF text
struct Genotyper::RunShared {
    const Run& r;
    std::chrono::steady_clock::time_point t_begin;
    std::vector<Task> tasks;
    uint32_t n_threads = 1;
    // A window's VCF lines are written as soon as its calls are known -- for most windows while the last chains are still on the
    // device -- and joined in task order at the end
    std::vector<std::string> pieces;
    std::vector<uint8_t> piece_done;
    std::atomic<int64_t> dev_first{INT64_MAX}, dev_last{0};      // from the first device call's start to the last one's end
    std::atomic<size_t> emit_windows_done{0};                    // windows with rows whose emissions the device scored

    explicit RunShared(const Run& run) : r(run) {}
    int64_t since_begin() const { return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t_begin).count(); }
    void note_device_span(int64_t ta, int64_t tb)
    {
        for (int64_t v = dev_first.load(); ta < v && !dev_first.compare_exchange_weak(v, ta);) {}
        for (int64_t v = dev_last.load(); tb > v && !dev_last.compare_exchange_weak(v, tb);) {}
    }
};

struct Genotyper::DevicePaths {
    bool pool_device = false;      // windows on the pool, their recursion and posterior on the device
    bool emit = false;             // emissions on the device, whole panel
    bool select = false;           // emissions on the device, haplotypes selected per window
    size_t n_gt = 0, total_room = 0;
};

// The windows on the pool write their emission scores and step tables straight into the run's arrays: room for every node with more
// than one allele is set aside per window (a node without k-mers leaves its row unused).
struct Genotyper::WindowBuffers {
    long double *obs = nullptr, *pw = nullptr, *prob = nullptr;
    uint32_t *row = nullptr, *win = nullptr;
    uint8_t *restart = nullptr, *gid = nullptr, *order = nullptr;
    uint64_t *fs = nullptr, *bs = nullptr;
    size_t n_gt = 0;
    uint32_t stride = 0;

    WindowBuffers() = default;
    WindowBuffers(const WindowBuffers&) = delete;
    WindowBuffers& operator=(const WindowBuffers&) = delete;
    ~WindowBuffers()
    {
        for (void* p : {(void*)obs, (void*)pw, (void*)prob, (void*)row, (void*)win, (void*)restart, (void*)gid, (void*)order, (void*)fs, (void*)bs}) std::free(p);
    }
    bool ready() const { return obs != nullptr; }
    void allocate(size_t total_room, size_t n_genotypes, uint32_t ploidy)
    {
        n_gt = n_genotypes;
        stride = ploidy + 1;
        obs = static_cast<long double*>(std::malloc(total_room * n_gt * sizeof(long double)));
        pw = static_cast<long double*>(std::malloc(2 * total_room * 2 * stride * sizeof(long double)));
        row = static_cast<uint32_t*>(std::calloc(2 * total_room, sizeof(uint32_t)));
        restart = static_cast<uint8_t*>(std::calloc(2 * total_room, 1));
        gid = static_cast<uint8_t*>(std::calloc(total_room * n_gt, 1));
        order = static_cast<uint8_t*>(std::calloc(total_room * n_gt, 1));
        fs = static_cast<uint64_t*>(std::calloc(total_room, sizeof(uint64_t)));
        bs = static_cast<uint64_t*>(std::calloc(total_room, sizeof(uint64_t)));
        prob = static_cast<long double*>(std::malloc(total_room * sizeof(long double)));
        win = static_cast<uint32_t*>(std::malloc(total_room * sizeof(uint32_t)));
        if (!obs || !pw || !row || !restart || !gid || !order || !fs || !bs || !prob || !win) throw std::runtime_error("out of memory (HMM tables)");
        advise_huge_pages(obs, total_room * n_gt * sizeof(long double));       // gigabytes, first touched here and by the copies
    }
    void bind(WindowWork& w) const
    {
        w.n_gt = n_gt;      // a window whose genotype list has another length takes the host path
        w.obs = obs + w.row0 * n_gt;
        w.pw = pw + w.step0 * 2 * stride;
        w.row = row + w.step0;
        w.restart = restart + w.step0;
        w.gid = gid + w.row0 * n_gt;
        w.order = order + w.row0 * n_gt;
        w.fwd_step = fs + w.row0;
        w.bwd_step = bs + w.row0;
        // rows and steps a window leaves unused (nodes without k-mers) still point into its own part of the arrays
        std::fill(w.row, w.row + 2 * w.room, (uint32_t)w.row0);
        std::fill(w.fwd_step, w.fwd_step + w.room, (uint64_t)w.step0);
        std::fill(w.bwd_step, w.bwd_step + w.room, (uint64_t)w.step0);
    }
};

// One word per entry of the node lists: multiplicity and haplotype bits are the graph's (filled once, a gather over the key arrays),
// the low byte is this sample's coverage -- a sequential pass over the device's cov_node
void Genotyper::fill_packed(Run& r, uint32_t threads)
{
    const size_t n_entries = g_.node_key_index.size();
    const uint8_t* const cov_node = r.cov;
    const size_t bl = g_.bitlen;
    const bool first = packed_.size() != n_entries;
    if (first) {
        packed_.reserve(n_entries);
        advise_huge_pages(packed_.data(), n_entries * sizeof(uint64_t));
        packed_.resize(n_entries);
    }
    const uint32_t nt = std::max(1u, threads);
    std::vector<std::thread> fill;
    auto part = [&](size_t a, size_t b) {
        CpuBudget::Hold cpu;
        PhaseTimer tt(g_phase.fill);
        if (first && g_.entry_words.size() == n_entries) {      // the graph's half was gathered once for every Genotyper
            for (size_t j = a; j < b; ++j) packed_[j] = g_.entry_words[j] | cov_node[j];
        } else if (first) {
            for (size_t j = a; j < b; ++j) {
                const size_t key = g_.node_key_index[j];
                uint64_t bits = 0;
                std::memcpy(&bits, &g_.bitvec[key * bl], bl);
                packed_[j] = (uint64_t)cov_node[j] | (uint64_t)(uint8_t)g_.f[key] << 8 | bits << 16;
            }
        } else {
            for (size_t j = a; j < b; ++j) packed_[j] = (packed_[j] & ~(uint64_t)0xFF) | cov_node[j];
        }
    };
    for (uint32_t t = 1; t < nt; ++t) fill.emplace_back(part, n_entries * t / nt, n_entries * (t + 1) / nt);
    part(0, n_entries / nt);
    for (auto& th : fill) th.join();
    r.packed = packed_.data();
}

// The graph's half of every entry for a panel of 48 to 511 haplotypes -- multiplicity and the 7 to 64 bytes of haplotype bits -- to the
// device, once per graph and context: gathered through node_key_index chunk by chunk into a staging buffer (threaded like fill_packed)
// and handed over (vgmi_hmm_entries_fill_wide, above 32 bytes _wide16); no second copy of n_entries x bitlen bytes is kept on the host.
void Genotyper::upload_entries_wide(uint32_t threads)
{
    const size_t n_entries = g_.node_key_index.size(), bl = g_.bitlen;
    const auto t0 = std::chrono::steady_clock::now();
    const bool ids16 = bl > 32;
    device_check(dev_, ids16 ? vgmi_hmm_entries_reserve_wide16(dev_, n_entries, (uint32_t)bl) : vgmi_hmm_entries_reserve_wide(dev_, n_entries, (uint32_t)bl),
                 "device HMM emissions: ");
    const size_t kChunk = (size_t)1 << (ids16 ? 21 : 22);      // entries per hand-over: at most 128 MiB of bits
    const size_t chunk = std::min(kChunk, std::max<size_t>(n_entries, 1));
    std::vector<uint8_t> f(chunk), bits(chunk * bl);
    const uint32_t nt = std::max(1u, threads);
    for (size_t lo = 0; lo < n_entries; lo += chunk) {
        const size_t m = std::min(chunk, n_entries - lo);
        auto part = [&](size_t a, size_t b) {
            CpuBudget::Hold cpu;
            PhaseTimer tt(g_phase.fill);
            for (size_t j = a; j < b; ++j) {
                const size_t key = g_.node_key_index[lo + j];
                f[j] = (uint8_t)g_.f[key];
                std::memcpy(&bits[j * bl], &g_.bitvec[key * bl], bl);
            }
        };
        std::vector<std::thread> fill;
        for (uint32_t t = 1; t < nt; ++t) fill.emplace_back(part, m * t / nt, m * (t + 1) / nt);
        part(0, m / nt);
        for (auto& th : fill) th.join();
        device_check(dev_, ids16 ? vgmi_hmm_entries_fill_wide16(dev_, lo, m, f.data(), bits.data()) : vgmi_hmm_entries_fill_wide(dev_, lo, m, f.data(), bits.data()),
                     "device HMM emissions: ");
    }
    if (g_phase_on)
        std::fprintf(stderr, "[varigraph-mi] HMM haplotype bits on the device: %zu bytes per entry (%zu entries, %.3f s)\n", bl, n_entries,
                     std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

void Genotyper::reset_calls()
{
    for (auto& c : chroms_)
        for (auto& n : c.nodes) {
            if (n.hmm.capacity()) std::vector<HmmScore>().swap(n.hmm);
            // (cleared, not replaced: the three small vectors of a call keep their storage from sample to sample)
            n.call.probability = 0;
            n.call.haps.clear();
            n.call.kmer_num.clear();
            n.call.kmer_ave_cov.clear();
            n.call.unique_kmers = 0;
        }
}

// windows of `chr_len_thread` bp over the node list of every chromosome (src/genotype.cpp:76-140)
std::vector<Genotyper::Task> Genotyper::windows(const GenotypeConfig& cfg)
{
    std::vector<Task> tasks;
    for (auto& chr : chroms_) {
        const uint64_t n_nodes = chr.nodes.size();
        if (g_.chr_len.find(chr.name) == g_.chr_len.end())
            throw std::runtime_error("'" + chr.name + "' does not exist in the reference genome.");
        const uint32_t chr_len = chr.len;
        const uint32_t step = std::min(cfg.chr_len_thread, chr_len);
        const uint32_t steps = (uint32_t)std::ceil(double(chr_len) / step);
        uint32_t end = 0;
        for (uint32_t i = 0; i < steps; i++) {
            const uint32_t step_end = (i + 1) * step;
            const uint32_t first = end;
            if (first >= n_nodes) break;
            for (uint32_t j = first; j < n_nodes; ++j) {
                if (chr.nodes[j].start > step_end) break;
                end++;
            }
            tasks.push_back({&chr, first, end});
        }
    }
    return tasks;
}

// Which path a sample takes.  With a device context (set_device; VGH_HMM_DEVICE=0 keeps the host): recursion and posterior of the
// eligible windows on the device (window(), window_finish()); `works` gets a window's room in the run's arrays.
Genotyper::DevicePaths Genotyper::device_paths(const Run& r, const std::vector<Task>& tasks, std::vector<WindowWork>& works, bool refuse_select) const
{
    const GenotypeConfig& cfg = *r.cfg;
    DevicePaths dp;
    // `-m fre` (transitions by haplotype frequency) has a recursion kernel of its own, fed by the two paths that score the emissions on the
    // device: 2 .. 4 haplotypes per genotype, at most 128 genotypes, never the pool.  VGH_HMM_FRE_DEVICE=0: such a sample stays on the host.
    const bool fre = cfg.transition == "fre";
    // (`-m rec` takes genotypes of up to 8 haplotypes; the `-m fre` kernel stops at 4: such a sample of ploidy 5 .. 8 stays on the host)
    const bool transition_ok = cfg.transition == "rec" || (fre && cfg.sample_ploidy >= 2 && cfg.sample_ploidy <= 4 && !knob_off("VGH_HMM_FRE_DEVICE"));
    const bool use_device = dev_ != nullptr && !knob_off("VGH_HMM_DEVICE") && transition_ok && cfg.sample_ploidy >= 1 && cfg.sample_ploidy <= 8;
    if (!use_device) return dp;
    works.resize(tasks.size());
    std::vector<uint16_t> some(std::min<size_t>(r.haploid_num, n_hap_));
    for (size_t i = 0; i < some.size(); ++i) some[i] = (uint16_t)i;
    dp.n_gt = haplotype_combinations(some, cfg.sample_type, cfg.sample_ploidy, (uint16_t)(n_hap_ - 1)).size();
    for (size_t t = 0; t < tasks.size(); ++t) {
        size_t room = 0;
        for (uint32_t i = tasks[t].first; i < tasks[t].last; ++i) room += tasks[t].chr->nodes[i].gn->hap_gt.size() > 1;
        works[t].room = room;
        works[t].row0 = dp.total_room;
        works[t].step0 = 2 * dp.total_room;
        dp.total_room += room;
    }
    const size_t dev_n_gt = dp.n_gt, total_room = dp.total_room;
    // (the emission scores of all windows are held at once, on the host and -- with alpha and beta, three times that -- on
    // the device: beyond 16 GiB, a genome's worth of sites at 120 genotypes, the host runs the recursion as before;
    // VGH_HMM_DEVICE_GIB moves the bound)
    size_t score_gib = 16;
    if (const char* e = getenv("VGH_HMM_DEVICE_GIB")) score_gib = (size_t)std::max(0L, atol(e));
    // ... and what the device has free right now: a part holds its scores, alpha and beta (3 x its scores) until its calls are
    // back, all parts of a sample may be in flight at once, and 4 / dev_parts_ samples share the device (set_device)
    bool fits_device = true;
    {
        size_t free_b = 0, total_b = 0;
        const size_t need = 3 * total_room * dev_n_gt * sizeof(long double) * ((4 + dev_parts_ - 1) / dev_parts_) + (size_t(1) << 30);
        if (vgmi_device_memory(dev_, &free_b, &total_b) == VGMI_OK) fits_device = need <= free_b - free_b / 10;
        if (!fits_device && g_phase_on)
            std::fprintf(stderr, "[varigraph-mi] HMM on the host: %.1f GiB of device memory wanted, %.1f free\n", need / 1073741824.0, free_b / 1073741824.0);
    }
    const bool device_ok = fits_device && dev_n_gt >= 1 && dev_n_gt <= 2048 && total_room && total_room * dev_n_gt * sizeof(long double) <= (score_gib << 30);
    // the emission scores can be computed on the device as well (hmm_whole_panel): a diploid sample, every haplotype selected, whole lists
    // (polyploid samples too -- their genotypes are blocks of `ploidy` consecutive haplotypes, :846-873, a handful per window).
    // VGH_HMM_EMIT_DEVICE=0: the host prepares the scores as before.
    dp.emit = device_ok && !emit_device_off_ && r.packed != nullptr && cfg.sample_ploidy >= 2 && cfg.sample_ploidy <= 8 && n_hap_ <= r.haploid_num && n_hap_ <= 16 &&
              dev_n_gt <= 128 && lists_whole_.load() && !knob_off("VGH_HMM_EMIT_DEVICE");
    // ... and when -n selects fewer haplotypes than the graph has, for a diploid sample (hmm_selected: every window draws its own haplotypes,
    // the genotype list keeps its shape, the k-mer lists are pruned on the device and here alike).  VGH_HMM_SELECT_DEVICE=0: the host
    // prepares such a sample as before.
    bool plain_ids = true;      // haplotype h is bit h of an entry's word
    for (size_t i = 0; i < hap_ids_.size(); ++i) plain_ids = plain_ids && hap_ids_[i] == i;
    // A polyploid sample (3 .. 8 haplotypes per genotype: use_device bounds it) takes that path too: its windows have lists of 1 .. -n blocks of haplotypes, so the
    // room on the device is reckoned for -n genotypes, not for the handful dp.n_gt counts over the first -n haplotypes.
    const bool blocks = cfg.sample_ploidy >= 3;
    const size_t sel_n_gt = blocks ? std::max<size_t>(dev_n_gt, r.haploid_num) : dev_n_gt;
    const bool select_fits = !blocks || (total_room * sel_n_gt * sizeof(long double) <= (score_gib << 30) && [&] {
        size_t free_b = 0, total_b = 0;
        const size_t need = 3 * total_room * sel_n_gt * sizeof(long double) * ((4 + dev_parts_ - 1) / dev_parts_) + (size_t(1) << 30);
        return vgmi_device_memory(dev_, &free_b, &total_b) != VGMI_OK || need <= free_b - free_b / 10;
    }());
    // A graph of 7 to 64 bytes of haplotype bits (48 to 511 haplotypes) has no packed words: a diploid sample's entries go to the device as
    // bytes (r.wide), once per graph and context -- W words and a multiplicity byte per entry that have to fit as well
    bool wide_fits = true;
    if (r.wide && !entries_uploaded_) {
        size_t free_b = 0, total_b = 0;
        const size_t n_entries = g_.node_key_index.size();
        const size_t need = n_entries * (8 * (size_t)vgh::words_of((uint32_t)g_.bitlen) + 3) + 3 * total_room * sel_n_gt * sizeof(long double) * ((4 + dev_parts_ - 1) / dev_parts_) +
                            (size_t(1) << 30);
        if (vgmi_device_memory(dev_, &free_b, &total_b) == VGMI_OK) wide_fits = need <= free_b - free_b / 10;
        if (!wide_fits && g_phase_on)
            std::fprintf(stderr, "[varigraph-mi] HMM on the host: %.1f GiB of device memory wanted, %.1f free\n", need / 1073741824.0, free_b / 1073741824.0);
    }
    const bool entries_ok = r.packed != nullptr || (r.wide && wide_fits);
    dp.select = device_ok && select_fits && !refuse_select && !dp.emit && entries_ok && (cfg.sample_ploidy == 2 || blocks) && n_hap_ > r.haploid_num &&
                r.haploid_num >= 1 && r.haploid_num <= 16 && dev_n_gt <= 128 && plain_ids && n_hap_ < 8 * g_.bitlen && !knob_off("VGH_HMM_EMIT_DEVICE") &&
                !knob_off("VGH_HMM_SELECT_DEVICE");
    if (fre) {
        // the whole panel's windows draw too under `-m fre` (their scores are the factors): the support sums come from the device, which
        // reads haplotype h as bit h.  With selection only a diploid sample: a polyploid one's blocks name haplotypes that were not drawn
        // and have no score -- the reference stops there ("does not exist in 'hapIdxScoreMap'"), and so does the host path
        dp.emit = dp.emit && plain_ids;
        dp.select = dp.select && cfg.sample_ploidy == 2;
    }
    dp.pool_device = device_ok && !dp.emit && !dp.select && !fre;
    return dp;
}

// ---- VCF (src/genotype.cpp:1579-1696): sites in vcf_info order, only those with a non-reference call.  The
// reference walks mVcfInfoMap (chromosome, then position) and looks every site up in the graph; the windows are the
// same nodes in the same order, so every task writes the lines of its own nodes and the pieces are joined in task
// order (chromosomes of the graph that the VCF lacks have thrown in window() already).
void Genotyper::write_piece(RunShared& s, size_t t)
{
    s.piece_done[t] = 1;
    const Task& task = s.tasks[t];
    const Chrom& chr = *task.chr;
    auto vc = g_.vcf_info.find(chr.name);
    if (vc == g_.vcf_info.end()) return;
    SiteWalk walk(vc->second);
    std::string out;
    std::vector<uint64_t> gt;
    for (uint32_t ni = task.first; ni < task.last; ++ni) {
        const Node& node = chr.nodes[ni];
        const std::vector<std::string>* fields = walk.at(node.start);
        append_call_line(out, node, s.r.cfg->min_gq, gt, [&](std::string& o) { return append_site_head(o, fields); });
    }
    s.pieces[t] = std::move(out);
}

// ---- Windows on the pool.  Three kinds of work on one pool: a window is prepared (window()), the recursion and posterior of a PART of the
// windows run on the device (one call per part, on a thread of its own that mostly waits), the calls of a part's windows
// are written back (window_finish()).  A chain is serial from its first node to its last, so the device takes as long
// for ten windows as for all of them: the parts go to the device as soon as their windows are prepared, side by side
// (vgmi_hmm_calls_part: own stream and buffers per call), while the pool prepares the next and finishes the last.
// At most four parts, over all the samples genotyped at the same time (set_device): a process has four hardware queues by
// default and a stream beyond them shares one, waiting behind the other stream's kernel for its whole length.
void Genotyper::hmm_on_pool(RunShared& s, std::vector<WindowWork>& works, const WindowBuffers& bufs, size_t n_gt)
{
    const Run& r = s.r;
    const GenotypeConfig& cfg = *r.cfg;
    const std::vector<Task>& tasks = s.tasks;
    const bool device_ready = bufs.ready();
    const size_t max_parts = std::min<size_t>(4, dev_parts_);
    const size_t part_windows = std::max<size_t>(s.n_threads, (tasks.size() + max_parts - 1) / max_parts);
    const size_t n_parts = device_ready ? (tasks.size() + part_windows - 1) / part_windows : 0;
    std::vector<std::atomic<size_t>> part_done(n_parts);
    for (auto& d : part_done) d.store(0);
    std::vector<std::thread> part_threads(n_parts);
    std::mutex q_mu;
    std::condition_variable q_cv;
    std::deque<size_t> finish_q;          // windows whose calls are back from the device
    size_t parts_open = n_parts;          // under q_mu
    std::atomic<size_t> next{0};
    std::string error;
    std::atomic<bool> failed{false};
    auto fail_with = [&](const char* what) {
        if (!failed.exchange(true)) error = what;
        std::lock_guard<std::mutex> lock(q_mu);
        q_cv.notify_all();
    };
    auto run_part = [&](size_t part) {
        try {
            const size_t t0 = part * part_windows, t1 = std::min(tasks.size(), t0 + part_windows);
            std::vector<size_t> dw;
            for (size_t t = t0; t < t1; ++t)
                if (works[t].on_device && !works[t].nodes.empty()) dw.push_back(t);
            if (!dw.empty() && !failed.load()) {
                const size_t n = n_gt;
                std::vector<uint8_t> keep(dw.size() * n * n);
                std::vector<vgmi_hmm_chain> chains;
                for (size_t wi = 0; wi < dw.size(); ++wi) {
                    const WindowWork& w = works[dw[wi]];
                    if (w.n_gt != n || w.ploidy != cfg.sample_ploidy) throw std::runtime_error("internal: a window with another genotype list");
                    std::memcpy(&keep[wi * n * n], w.keep_mat.data(), n * n);
                    const uint64_t m = w.nodes.size();
                    chains.push_back(vgmi_hmm_chain{w.step0, m, (uint32_t)wi, 0});
                    chains.push_back(vgmi_hmm_chain{w.step0 + m, m, (uint32_t)wi, 0});
                }
                const uint64_t row_lo = works[t0].row0, row_hi = works[t1 - 1].row0 + works[t1 - 1].room;
                const long double uniform = 1.0L / (long double)n;
                const int64_t ta = s.since_begin();
                const int rc = vgmi_hmm_calls_part(dev_, (uint32_t)n, cfg.sample_ploidy, keep.data(), (uint32_t)dw.size(), bufs.obs, row_lo, row_hi, bufs.row,
                                                   bufs.restart, bufs.pw, 2 * row_lo, 2 * row_hi, &uniform, chains.data(), (uint32_t)chains.size(), bufs.gid,
                                                   bufs.order, bufs.fs, bufs.bs, bufs.prob, bufs.win);
                if (rc == VGMI_E_NOMEM || (rc == VGMI_OK && getenv("VGH_HMM_FAKE_NOMEM") && part % 2 == 1)) {
                    // the device had no room for this part after all (other samples' parts, the table, the read buffers): the
                    // host runs these windows' recursion instead, with the haplotypes the first pass drew -- the sample is
                    // not lost, only slower
                    if (g_phase_on) std::fprintf(stderr, "[varigraph-mi] HMM part %zu: no device memory, %zu windows back on the host\n", part, dw.size());
                    for (size_t t : dw) {
                        CpuBudget::Hold cpu;
                        WindowWork& w = works[t];
                        w.on_device = false;
                        window(*tasks[t].chr, tasks[t].first, tasks[t].last, r, nullptr, &w.top);
                    }
                    dw.clear();
                } else if (rc != VGMI_OK)
                    throw std::runtime_error(std::string("device HMM recursion: ") + vgmi_last_error(dev_));
                const int64_t tb = s.since_begin();
                if (g_phase_on)
                    std::fprintf(stderr, "[varigraph-mi] HMM part %zu (windows %zu-%zu): on the device from %.3f to %.3f s\n", part, t0, t1 - 1, ta * 1e-9, tb * 1e-9);
                s.note_device_span(ta, tb);
            }
            std::lock_guard<std::mutex> lock(q_mu);
            for (size_t t : dw) finish_q.push_back(t);
            --parts_open;
            q_cv.notify_all();
        } catch (const std::exception& e) {
            fail_with(e.what());
        }
    };
    auto worker = [&]() {
        for (;;) {
            const size_t t = next.fetch_add(1);
            if (t >= tasks.size() || failed.load()) break;
            try {
                {
                    CpuBudget::Hold cpu;
                    window(*tasks[t].chr, tasks[t].first, tasks[t].last, r, device_ready ? &works[t] : nullptr);
                }
                if (device_ready) {
                    const size_t part = t / part_windows;
                    const size_t in_part = std::min(tasks.size(), (part + 1) * part_windows) - part * part_windows;
                    if (part_done[part].fetch_add(1) + 1 == in_part) part_threads[part] = std::thread(run_part, part);
                }
            } catch (const std::exception& e) {
                fail_with(e.what());
                return;
            }
        }
        for (;;) {      // nothing left to prepare: the calls that are back
            size_t t;
            {
                std::unique_lock<std::mutex> lock(q_mu);
                q_cv.wait(lock, [&] { return !finish_q.empty() || parts_open == 0 || failed.load(); });
                if (failed.load() || finish_q.empty()) return;
                t = finish_q.front();
                finish_q.pop_front();
            }
            try {
                CpuBudget::Hold cpu;
                WindowWork& w = works[t];
                window_finish(w, bufs.prob + w.row0, bufs.win + w.row0, r);
                write_piece(s, t);
            } catch (const std::exception& e) {
                fail_with(e.what());
                return;
            }
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < s.n_threads; ++t) pool.emplace_back(worker);
    worker();
    for (auto& th : pool) th.join();
    for (auto& th : part_threads)
        if (th.joinable()) th.join();
    if (failed.load()) throw std::runtime_error(error);
}

// ---------------------------------------------------------------- emissions on the device: what both paths do per row and per window
struct Genotyper::WindowHaps {
    const std::vector<uint16_t>& top;       // the selected haplotypes, ascending
    const std::vector<uint16_t>& used;      // those occurring in the genotypes, ascending
    const std::vector<std::vector<uint16_t>>& genotypes;
    const GenotypeList& glist;
};

// Rows the emission kernel flagged hold a multi-copy, under-covered, carried k-mer: the reference consults the haplotype's sequence
// (:760-800).  The strings are the host's; the row's products stay on the device, scored again (vgmi_hmm_part_fix_rows) with the
// haplotypes the sequences rule out taken off the entries concerned.  VGH_HMM_FIX_DEVICE=0: such a row is scored by the host (hidden
// states, products in x87 arithmetic) and handed in (vgmi_hmm_part_set_rows).  Collected per window, by the window's thread.
struct Genotyper::FlaggedRows {
    std::vector<std::vector<uint64_t>> host_rows, fix_rows;
    std::vector<std::vector<long double>> host_obs;
    std::vector<std::vector<uint32_t>> fix_cnt, fix_j;      // fix_j: the entries, counted along the node's list
    std::vector<std::vector<uint64_t>> fix_mask;            // over the places of `used`, until the caller says otherwise
    size_t n_host = 0, n_fixed = 0;      // rows handed over by upload_flagged
    explicit FlaggedRows(size_t nw) : host_rows(nw), fix_rows(nw), host_obs(nw), fix_cnt(nw), fix_j(nw), fix_mask(nw) {}
};

struct Genotyper::FlaggedScratch {      // of one window's thread
    ScoreCtx sctx;
    NodeStates st;
    double lower, upper;
    FlaggedScratch(float ave, double lo, double up) : lower(lo), upper(up)
    {
        sctx.ave = ave;
        sctx.score_up = up;
    }
};

void Genotyper::flagged_row(FlaggedRows& fl, size_t wi, size_t rr, Chrom& chr, uint32_t node_i, const WindowHaps& h, uint64_t gt0, const Run& r,
                            FlaggedScratch& sc, uint32_t& n_kept)
{
    static const bool fix_on_device = !knob_off("VGH_HMM_FIX_DEVICE");
    if (fix_on_device) {
        PhaseTimer tt(g_phase.states);
        const size_t before = fl.fix_j[wi].size();
        sequence_fixes(chr, node_i, h.used, gt0, sc.lower, sc.upper, r, fl.fix_j[wi], fl.fix_mask[wi]);
        if (fl.fix_j[wi].size() != before) {
            fl.fix_rows[wi].push_back(rr);
            fl.fix_cnt[wi].push_back((uint32_t)(fl.fix_j[wi].size() - before));
        }
        return;
    }
    {
        PhaseTimer tt(g_phase.states);
        sc.st = hidden_states(chr, node_i, h.top, h.genotypes, h.used, h.glist, sc.lower, sc.upper, true, r, std::move(sc.st), nullptr);
    }
    PhaseTimer tt(g_phase.emit);
    const std::vector<long double> obs = score_states(sc.st, sc.sctx);
    n_kept = (uint32_t)(obs.empty() ? 0 : sc.st.c.size());
    if (!obs.empty()) {
        fl.host_rows[wi].push_back(rr);
        fl.host_obs[wi].insert(fl.host_obs[wi].end(), obs.begin(), obs.end());
    }
}

void Genotyper::upload_flagged(FlaggedRows& fl, vgmi_hmm_part* part, bool by_hap_id, bool wide_ids)
{
    std::vector<uint64_t> all_rows, f_rows;
    std::vector<long double> all_obs;
    std::vector<uint32_t> f_off(1, 0), f_j;
    std::vector<uint64_t> f_m;
    for (size_t wi = 0; wi < fl.host_rows.size(); ++wi) {
        all_rows.insert(all_rows.end(), fl.host_rows[wi].begin(), fl.host_rows[wi].end());
        all_obs.insert(all_obs.end(), fl.host_obs[wi].begin(), fl.host_obs[wi].end());
        std::vector<long double>().swap(fl.host_obs[wi]);
        f_rows.insert(f_rows.end(), fl.fix_rows[wi].begin(), fl.fix_rows[wi].end());
        for (uint32_t cnt : fl.fix_cnt[wi]) f_off.push_back(f_off.back() + cnt);
        f_j.insert(f_j.end(), fl.fix_j[wi].begin(), fl.fix_j[wi].end());
        f_m.insert(f_m.end(), fl.fix_mask[wi].begin(), fl.fix_mask[wi].end());
    }
    fl.n_host = all_rows.size();
    fl.n_fixed = f_rows.size();
    if (!all_rows.empty()) device_check(dev_, vgmi_hmm_part_set_rows(part, all_rows.size(), all_rows.data(), all_obs.data()), "device HMM emissions: ");
    if (f_rows.empty()) return;
    if (wide_ids) {      // ... over a panel of 48 to 254 haplotypes: W words of haplotype ids per fix
        device_check(dev_, vgmi_hmm_part_fix_rows_ploidy_wide(part, f_rows.size(), f_rows.data(), f_off.data(), f_j.data(), f_m.data()), "device HMM emissions: ");
        return;
    }
    if (by_hap_id) {      // a part with a genotype list per window: the masks are over haplotype ids already
        device_check(dev_, vgmi_hmm_part_fix_rows_wide(part, f_rows.size(), f_rows.data(), f_off.data(), f_j.data(), f_m.data()), "device HMM emissions: ");
        return;
    }
    const std::vector<uint16_t> f_m16(f_m.begin(), f_m.end());      // (<= 16 places)
    device_check(dev_, vgmi_hmm_part_fix_rows(part, f_rows.size(), f_rows.data(), f_off.data(), f_j.data(), f_m16.data()), "device HMM emissions: ");
}

// The rows [row_lo, row_hi) of a window: every node as the chains see it (`seen`), and for the rows that have a score (n_kept) the
// genotype strings of their entries (gid / order: n_gt bytes per row).  The genotype strings of a node with two alleles depend on which
// haplotypes carry the reference allele only: one evaluation per distinct mask (the strings themselves as genotype_strings builds them).
template <class Mask>
void Genotyper::row_strings(const Chrom& chr, size_t row_lo, size_t row_hi, const uint32_t* row_node, const Mask* gt0, const uint32_t* n_kept,
                            const WindowHaps& h, uint8_t* gid, uint8_t* order, std::vector<Seen>& seen, std::vector<uint32_t>& scored_rows) const
{
    const size_t n_gt = h.genotypes.size();
    std::unordered_map<uint64_t, uint32_t> gs_memo;      // mask -> a row that holds the pattern
    for (size_t rr = row_lo; rr < row_hi; ++rr) {
        const Node& n = chr.nodes[row_node[rr]];
        const uint32_t n_start = n.start, n_end = (uint32_t)(n_start + n.gn->seqs[0].size() - 1);
        if (n_kept[rr] == 0) {
            seen.push_back(Seen{n_start, n_end, -1});
            continue;
        }
        seen.push_back(Seen{n_start, n_end, (int64_t)rr});
        bool biallelic = true;
        for (uint16_t hap : h.used) biallelic = biallelic && n.gn->hap_gt[hap] <= 1;
        auto it = biallelic ? gs_memo.find(gt0[rr]) : gs_memo.end();
        if (it != gs_memo.end()) {
            std::memcpy(gid + rr * n_gt, gid + (size_t)it->second * n_gt, n_gt);
            std::memcpy(order + rr * n_gt, order + (size_t)it->second * n_gt, n_gt);
        } else {
            (void)genotype_strings(n, h.genotypes, gid + rr * n_gt, order + rr * n_gt);     // <= 128 strings: always fits
            if (biallelic) gs_memo.emplace(gt0[rr], (uint32_t)rr);
        }
        scored_rows.push_back((uint32_t)rr);
    }
}

// The step tables of a part's windows end to end (two chains per window with a scored row), as the device call takes them
struct Genotyper::StepArrays {
    std::vector<size_t> win_step0;
    size_t n_steps = 0;
    uint32_t stride;
    bool has_pow;
    std::vector<long double> pw;
    std::vector<uint32_t> row;
    std::vector<uint8_t> restart;
    std::vector<uint64_t> fwd, bwd;
    std::vector<vgmi_hmm_chain> chains;

    // keep_per_window: window wi's chains use keep matrix wi (a genotype list per window) or table wi (`-m fre`); else one matrix serves
    // all.  with_pow false (`-m fre`): no tables of powers are made
    StepArrays(const std::vector<std::vector<uint32_t>>& win_rows, size_t n_rows, uint32_t ploidy, bool keep_per_window = false, bool with_pow = true)
        : win_step0(win_rows.size() + 1, 0), stride(ploidy + 1), has_pow(with_pow)
    {
        for (size_t wi = 0; wi < win_rows.size(); ++wi) win_step0[wi + 1] = win_step0[wi] + 2 * win_rows[wi].size();
        n_steps = win_step0.back();
        if (!n_steps) return;
        if (has_pow) pw.resize(n_steps * 2 * stride);
        row.assign(n_steps, 0);
        restart.assign(n_steps, 0);
        fwd.assign(n_rows, 0);
        bwd.assign(n_rows, 0);
        for (size_t wi = 0; wi < win_rows.size(); ++wi) {
            const size_t m = win_rows[wi].size();
            if (!m) continue;
            const uint32_t keep_index = keep_per_window ? (uint32_t)wi : 0u;
            chains.push_back(vgmi_hmm_chain{win_step0[wi], m, keep_index, 0});
            chains.push_back(vgmi_hmm_chain{win_step0[wi] + m, m, keep_index, 0});
        }
    }
    void fill(size_t wi, const std::vector<Seen>& seen, uint16_t population)      // (libm: a window per thread)
    {
        const size_t s0 = win_step0[wi];
        step_tables(seen, stride, population, s0, 0, has_pow ? pw.data() + s0 * 2 * stride : nullptr, row.data() + s0, restart.data() + s0, fwd.data(), bwd.data());
    }
};

// the calls of a window's scored rows into its nodes' records, for the lines that are written from those (no tallies from the device)
void Genotyper::finish_rows(Chrom* chr, const std::vector<uint32_t>& rows, const uint32_t* row_node, const WindowHaps& h, const long double* prob,
                            const uint32_t* winner, const Run& r)
{
    WindowWork w;
    w.chr = chr;
    w.n_gt = h.genotypes.size();
    w.genotypes = h.genotypes;
    w.top = h.top;
    std::vector<long double> pr(rows.size());
    std::vector<uint32_t> wn(rows.size());
    for (size_t q = 0; q < rows.size(); ++q) {
        w.nodes.push_back(row_node[rows[q]]);
        pr[q] = prob[rows[q]];
        wn[q] = winner[rows[q]];
    }
    window_finish(w, pr.data(), wn.data(), r);
}

// ---------------------------------------------------------------- emissions on the device, whole panel
// Emission scores on the device too (vgmi_hmm_emissions): a sample over a graph all of whose haplotypes are selected (-n >= haplotypes:
// one genotype list for every window, no k-mer list is ever pruned).  Per part of the windows: the host lists the nodes' entry ranges,
// the device scores them from the node-ordered coverage it was handed, the host sees to the few nodes whose haplotype sequences must
// be consulted, builds the step tables (libm) and the genotype strings, the device runs recursion and posterior on the scores where
// they lie.
struct Genotyper::PanelSample {
    float ave = 0;
    double lower = 256.0f, upper = -0.1f;
    std::vector<uint16_t> top, used;      // one genotype list for the whole sample
    std::vector<std::vector<uint16_t>> genotypes;
    GenotypeList glist;
    std::vector<uint8_t> used8, pos_all;      // pos_all: per genotype its haplotypes' places in `used`
    std::vector<uint8_t> keep_mat;
    uint64_t top_mask = 0;
    std::vector<long double> tab;
    size_t per_part = 1, n_parts = 0;
    std::string cache_key;
    std::atomic<bool> broken{false};      // a pruned list after all: the host path
    std::atomic<size_t> ploidy_tally_rows{0};      // rows of a polyploid sample whose calls the device tallied, over the parts
    // `-m fre`: the scores of every window's draw are the recursion's factors -- per window of the run the table of the genotypes' haplotypes'
    // scores; the recursion's other inputs go up per sample (vgmi_hmm_part_calls_fre) instead of lying in a plan
    bool by_freq = false;
    std::vector<std::vector<long double>> win_freq;
    WindowHaps haps() const { return WindowHaps{top, used, genotypes, glist}; }
};

Genotyper::Emitted Genotyper::hmm_whole_panel(RunShared& s)
{
    const Run& r = s.r;
    const GenotypeConfig& cfg = *r.cfg;
    const double tb0 = s.since_begin() * 1e-9;
    PanelSample ps;
    ps.ave = r.hap_cov;
    poisson_interval(ps.ave, ps.lower, ps.upper);
    for (const auto& kv : g_.hap_names) ps.top.push_back(kv.first);
    std::sort(ps.top.begin(), ps.top.end());
    ps.genotypes = haplotype_combinations(ps.top, cfg.sample_type, cfg.sample_ploidy, (uint16_t)(n_hap_ - 1));
    const size_t n_gt = ps.genotypes.size();
    for (const auto& gtv : ps.genotypes) ps.used.insert(ps.used.end(), gtv.begin(), gtv.end());
    std::sort(ps.used.begin(), ps.used.end());
    ps.used.erase(std::unique(ps.used.begin(), ps.used.end()), ps.used.end());
    bool full = true;      // (every genotype holds `ploidy` haplotypes: pairs for a diploid sample)
    for (const auto& gtv : ps.genotypes) full = full && gtv.size() == cfg.sample_ploidy;
    if (!(full && n_gt >= 1 && n_gt <= 128 && ps.used.size() <= 16)) return Emitted::no;
    ps.glist = genotype_list(ps.genotypes, ps.used);
    std::vector<uint8_t> where(n_hap_ + 1, 0);
    ps.used8.resize(ps.used.size());
    for (size_t p = 0; p < ps.used.size(); ++p) {
        where[ps.used[p]] = (uint8_t)p;
        ps.used8[p] = (uint8_t)ps.used[p];
    }
    ps.pos_all.resize(n_gt * cfg.sample_ploidy);
    for (size_t gi = 0; gi < n_gt; ++gi)
        for (uint32_t q = 0; q < cfg.sample_ploidy; ++q) ps.pos_all[gi * cfg.sample_ploidy + q] = where[ps.genotypes[gi][q]];
    ps.by_freq = cfg.transition == "fre";
    if (!ps.by_freq) ps.keep_mat = keep_matrix(ps.genotypes);
    for (uint16_t hap : ps.top) ps.top_mask |= 1ULL << hap;
    ps.tab = emission_table(ps.ave, cfg.sample_ploidy);
    if (!entries_uploaded_) {
        device_check(dev_, vgmi_hmm_entries_upload(dev_, packed_.data(), packed_.size()), "device HMM emissions: ");
        entries_uploaded_ = true;
    }
    device_check(dev_, vgmi_hmm_sample_upload(dev_, r.cov, g_.node_key_index.size()), "device HMM emissions: ");
    if (ps.by_freq && !panel_draws(s, ps)) return Emitted::lists_pruned;
    const size_t max_parts = std::min<size_t>(4, dev_parts_);
    ps.per_part = std::max<size_t>(1, (s.tasks.size() + max_parts - 1) / max_parts);
    ps.n_parts = (s.tasks.size() + ps.per_part - 1) / ps.per_part;
    ps.cache_key = std::to_string(s.tasks.size()) + "/" + std::to_string(ps.per_part) + "/" + std::to_string(cfg.sv_only) + "/" +
                   std::to_string(cfg.sample_ploidy) + "/" + cfg.sample_type + "/" + std::to_string(n_gt) + "/" + std::to_string(r.haploid_num) + "/" +
                   std::to_string(cfg.chr_len_thread) + "/" + cfg.transition;
    // What a part's device calls need beyond a sample's coverage is a function of the graph and the options: the rows (entry
    // ranges, reference-allele masks), and the PLAN -- genotype strings, which rows have a score, the step tables (libm), chains,
    // all of it resident on the device (vgmi_hmm_plan).  Made by the first sample that gets there, kept with the graph, shared
    // by every Genotyper of the run (eight consumers of one device would otherwise build eight of everything).
    int dev_id = 0;
    (void)vgmi_device_of(dev_, &dev_id);
    if (emit_cache_.size() != ps.n_parts) {
        emit_cache_.clear();
        emit_cache_.resize(ps.n_parts);
    }
    for (size_t part = 0; part < ps.n_parts; ++part) {
        const std::string slot = "emit/" + std::to_string(dev_id) + "/" + std::to_string(ps.n_parts) + "/" + std::to_string(part) + "/" + ps.cache_key;
        std::lock_guard<std::mutex> lock(g_.shared_mu);
        auto it = g_.shared_slots.find(slot);
        if (it == g_.shared_slots.end()) it = g_.shared_slots.emplace(slot, std::static_pointer_cast<void>(std::make_shared<EmitPartCache>())).first;
        emit_cache_[part] = std::static_pointer_cast<EmitPartCache>(it->second);
    }
    std::mutex err_mu;
    std::string err_text;
    auto part_fn = [&](size_t part) {
        try {
            panel_part(s, ps, part);
        } catch (const std::exception& e) {
            std::lock_guard<std::mutex> lock(err_mu);
            if (err_text.empty()) err_text = e.what();
        }
    };
    std::vector<std::thread> pthreads;
    for (size_t p = 1; p < ps.n_parts; ++p) pthreads.emplace_back(part_fn, p);
    if (ps.n_parts) part_fn(0);
    for (auto& th : pthreads) th.join();
    if (!err_text.empty()) throw std::runtime_error(err_text);
    if (ps.broken.load()) return Emitted::lists_pruned;
    if (g_phase_on) std::fprintf(stderr, "[varigraph-mi] HMM emissions on the device: %zu parts, %.2f s\n", ps.n_parts, s.since_begin() * 1e-9 - tb0);
    if (g_phase_on && ps.ploidy_tally_rows.load())
        std::fprintf(stderr, "[varigraph-mi] HMM tallies on the device: %zu rows, ploidy %u\n", ps.ploidy_tally_rows.load(), cfg.sample_ploidy);
    if (g_phase_on && ps.by_freq)
        std::fprintf(stderr, "[varigraph-mi] HMM transitions by haplotype frequency on the device: %zu windows\n", s.emit_windows_done.load());
    return Emitted::yes;
}

// `-m fre` with the whole panel: the windows draw all the same, because the scores of the draw are the recursion's factors.  The support
// sums over every node with more than one allele come from the device (vgmi_hmm_support; the lists are whole, so a node's list is a
// range), the draws are made here as hmm_selected makes them, and every window gets its table.  false: a node's list is not whole
bool Genotyper::panel_draws(RunShared& s, PanelSample& ps)
{
    const Run& r = s.r;
    const size_t nw = s.tasks.size();
    std::vector<uint64_t> sup_begin;
    std::vector<uint32_t> sup_count, sup_win;
    {
        CpuBudget::Hold cpu;
        PhaseTimer t_list(g_phase.list);
        for (size_t t = 0; t < nw; ++t) {
            const Chrom& chr = *s.tasks[t].chr;
            for (uint32_t i = s.tasks[t].first; i < s.tasks[t].last; ++i) {
                const Node& n = chr.nodes[i];
                if (n.gn->hap_gt.size() <= 1) continue;
                if (!n.kmers.empty() && (size_t)(n.kmers.back() - n.kmers.front()) + 1 != n.kmers.size()) return false;
                sup_begin.push_back(n.kmers.empty() ? 0 : n.kmers.front());
                sup_count.push_back((uint32_t)n.kmers.size());
                sup_win.push_back((uint32_t)t);
            }
        }
    }
    std::vector<uint32_t> support(nw * n_hap_, 0);
    device_check(dev_, vgmi_hmm_support(dev_, n_hap_, (uint32_t)nw, sup_begin.size(), sup_begin.data(), sup_count.data(), sup_win.data(), support.data()),
                 "device HMM support: ");
    ps.win_freq.resize(nw);
    over_windows(nw, s.n_threads, g_phase.select, [&](size_t wi) {
        HaplotypeSampler sampler(std::vector<uint32_t>(support.begin() + wi * n_hap_, support.begin() + (wi + 1) * n_hap_), (int)r.haploid_num);
        ps.win_freq[wi] = frequency_table(ps.genotypes, sampler.score);
    });
    return true;
}

// the rows of a part: every node the HMM works on, window after window (the same for every sample and every Genotyper: listed once).
// false: a node's list is not whole
bool Genotyper::panel_rows(RunShared& s, const PanelSample& ps, EmitPartCache& pc, size_t t0, size_t t1)
{
    std::lock_guard<std::mutex> lock(pc.mu);
    if (pc.key == ps.cache_key) return true;
    CpuBudget::Hold cpu;
    PhaseTimer t_list(g_phase.list);
    pc.e_begin.clear(); pc.e_count.clear(); pc.row_node.clear(); pc.gt0.clear();
    pc.plan.reset();
    pc.win_row0.assign(t1 - t0 + 1, 0);
    for (size_t t = t0; t < t1; ++t) {
        const Chrom& chr = *s.tasks[t].chr;
        const SiteMap& sites = vcf_sites(chr);
        for (uint32_t i = s.tasks[t].first; i < s.tasks[t].last; ++i) {
            const Node& n = chr.nodes[i];
            if (skipped(chr, sites, n, s.r.cfg->sv_only)) continue;
            if (!n.kmers.empty() && (size_t)(n.kmers.back() - n.kmers.front()) + 1 != n.kmers.size()) return false;
            pc.e_begin.push_back(n.kmers.empty() ? 0 : n.kmers.front());
            pc.e_count.push_back((uint32_t)n.kmers.size());
            uint16_t m = 0;
            for (size_t p = 0; p < ps.used.size(); ++p) m |= (uint16_t)((n.gn->hap_gt[ps.used[p]] == 0) << p);
            pc.gt0.push_back(m);
            pc.row_node.push_back(i);
        }
        pc.win_row0[t - t0 + 1] = pc.e_begin.size();
    }
    pc.key = ps.cache_key;
    return true;
}

// The plan of a part, for the rows that have a score -- the same for every sample of this path (a row's kept k-mers are those some
// haplotype carries, and every haplotype is selected); held against the pattern all the same.  Made under the part's lock.
std::shared_ptr<Genotyper::EmitPartPlan> Genotyper::panel_plan(RunShared& s, const PanelSample& ps, EmitPartCache& pc, size_t t0, size_t nw, size_t helpers,
                                                               const std::vector<uint32_t>& n_kept)
{
    const size_t n_rows = pc.e_begin.size(), n_gt = ps.genotypes.size();
    const std::vector<size_t>& win_row0 = pc.win_row0;
    std::vector<uint8_t> scored(n_rows);
    for (size_t rr = 0; rr < n_rows; ++rr) scored[rr] = n_kept[rr] != 0;
    std::lock_guard<std::mutex> lock(pc.mu);
    if (pc.plan && pc.plan->scored == scored) return pc.plan;
    auto np = std::make_shared<EmitPartPlan>();
    np->scored = scored;
    np->win_rows.resize(nw);
    std::vector<std::vector<Seen>> seen(nw);
    std::vector<uint8_t> gid(n_rows * n_gt, 0), order(n_rows * n_gt, 0);
    const WindowHaps haps = ps.haps();
    over_windows(nw, helpers, g_phase.pass_a, [&](size_t wi) {
        row_strings(*s.tasks[t0 + wi].chr, win_row0[wi], win_row0[wi + 1], pc.row_node.data(), pc.gt0.data(), n_kept.data(), haps, gid.data(), order.data(), seen[wi],
                    np->win_rows[wi]);
    });
    // the lines' shared heads, window by window
    std::vector<std::string> heads(nw);
    std::vector<std::vector<uint32_t>> head_len(nw);
    over_windows(nw, helpers, g_phase.pass_a, [&](size_t wi) {
        const Chrom& chr = *s.tasks[t0 + wi].chr;
        auto vc = g_.vcf_info.find(chr.name);
        head_len[wi].assign(win_row0[wi + 1] - win_row0[wi], 0);
        if (vc == g_.vcf_info.end()) return;
        SiteWalk walk(vc->second);
        for (size_t rr = win_row0[wi]; rr < win_row0[wi + 1]; ++rr) {
            const size_t before = heads[wi].size();
            if (append_site_head(heads[wi], walk.at(chr.nodes[pc.row_node[rr]].start))) head_len[wi][rr - win_row0[wi]] = (uint32_t)(heads[wi].size() - before);
        }
    });
    np->line_head_off.assign(n_rows + 1, 0);
    size_t total = 0;
    for (size_t wi = 0; wi < nw; ++wi) total += heads[wi].size();
    np->line_head.reserve(total);
    for (size_t wi = 0; wi < nw; ++wi) {
        for (size_t rr = win_row0[wi]; rr < win_row0[wi + 1]; ++rr) np->line_head_off[rr + 1] = np->line_head_off[rr] + head_len[wi][rr - win_row0[wi]];
        np->line_head += heads[wi];
        std::string().swap(heads[wi]);
    }
    StepArrays steps(np->win_rows, n_rows, s.r.cfg->sample_ploidy, ps.by_freq, !ps.by_freq);
    np->n_steps = steps.n_steps;
    if (steps.n_steps && ps.by_freq) {
        // no device plan: the tables of factors are the sample's.  What is the graph's -- rows, restarts, chains, strings -- is kept here and
        // goes up with every sample's tables (vgmi_hmm_part_calls_fre)
        over_windows(nw, helpers, g_phase.pass_b, [&](size_t wi) { steps.fill(wi, seen[wi], (uint16_t)n_hap_); });
        np->gid = std::move(gid);
        np->order = std::move(order);
        np->row = std::move(steps.row);
        np->restart = std::move(steps.restart);
        np->fwd = std::move(steps.fwd);
        np->bwd = std::move(steps.bwd);
        np->chains = std::move(steps.chains);
    } else if (steps.n_steps) {
        over_windows(nw, helpers, g_phase.pass_b, [&](size_t wi) { steps.fill(wi, seen[wi], (uint16_t)n_hap_); });
        const long double uniform = 1.0L / (long double)n_gt;
        device_check(dev_, vgmi_hmm_plan_create(dev_, (uint32_t)n_gt, s.r.cfg->sample_ploidy, ps.keep_mat.data(), 1, n_rows, steps.row.data(), steps.restart.data(),
                                                steps.pw.data(), steps.n_steps, &uniform, steps.chains.data(), (uint32_t)steps.chains.size(), gid.data(),
                                                order.data(), steps.fwd.data(), steps.bwd.data(), &np->plan),
                     "device HMM plan: ");
    }
    pc.plan = np;
    return np;
}

void Genotyper::panel_part(RunShared& s, PanelSample& ps, size_t part)
{
    const Run& r = s.r;
    const GenotypeConfig& cfg = *r.cfg;
    const size_t t0 = part * ps.per_part, t1 = std::min(s.tasks.size(), t0 + ps.per_part), nw = t1 - t0;
    const size_t n_gt = ps.genotypes.size();
    EmitPartCache& pc = *emit_cache_[part];
    if (!panel_rows(s, ps, pc, t0, t1)) {
        ps.broken = true;
        return;
    }
    const std::vector<size_t>& win_row0 = pc.win_row0;
    const size_t n_rows = pc.e_begin.size();
    if (n_rows == 0) return;      // no node of this part is the HMM's business (--sv over a part without long alleles): no calls, no lines
    std::vector<uint32_t> n_kept(n_rows);
    std::vector<uint8_t> flags(n_rows);
    PartHandle ph;
    const int64_t ta = s.since_begin();
    device_check(dev_, vgmi_hmm_emissions_ploidy(dev_, (uint32_t)n_gt, cfg.sample_ploidy, (uint32_t)ps.used.size(), ps.used8.data(), ps.pos_all.data(), ps.top_mask,
                                                 (uint32_t)g_.bitlen, ps.ave, ps.lower, ps.upper, ps.tab.data(), n_rows, pc.e_begin.data(), pc.e_count.data(),
                                                 pc.gt0.data(), n_kept.data(), flags.data(), &ph.p),
                 "device HMM emissions: ");
    const int64_t t_emit = s.since_begin();
    for (size_t rr = 0; rr < n_rows; ++rr)
        if (flags[rr] & 2u) {
            ps.broken = true;          // a k-mer no haplotype carries: the host path prunes it
            return;
        }
    // The part's windows on `helpers` threads.  A: the flagged rows.  (Once per graph, under the part's lock: the plan.)  Then recursion
    // and posterior on the device.  C: the calls and the VCF lines.
    const size_t helpers = std::max<size_t>(1, std::min<size_t>(nw, s.n_threads / ps.n_parts));
    const WindowHaps haps = ps.haps();
    FlaggedRows fl(nw);
    over_windows(nw, helpers, g_phase.pass_a, [&](size_t wi) {
        FlaggedScratch sc(ps.ave, ps.lower, ps.upper);
        for (size_t rr = win_row0[wi]; rr < win_row0[wi + 1]; ++rr)
            if (flags[rr] & 1u) flagged_row(fl, wi, rr, *s.tasks[t0 + wi].chr, pc.row_node[rr], haps, pc.gt0[rr], r, sc, n_kept[rr]);
    });
    const int64_t t_a = s.since_begin();
    upload_flagged(fl, ph.p);
    const int64_t t_rows = s.since_begin();
    const std::shared_ptr<EmitPartPlan> plan = panel_plan(s, ps, pc, t0, nw, helpers, n_kept);
    const int64_t t_b = s.since_begin();
    std::vector<long double> prob(n_rows);
    std::vector<uint32_t> winner(n_rows, 0xFFFFFFFFu);
    if (plan->n_steps && ps.by_freq) {
        const uint32_t ploidy_f = cfg.sample_ploidy;
        const long double uniform = 1.0L / (long double)n_gt;
        std::vector<long double> freq_all;
        freq_all.reserve(nw * n_gt * ploidy_f);
        for (size_t wi = 0; wi < nw; ++wi) freq_all.insert(freq_all.end(), ps.win_freq[t0 + wi].begin(), ps.win_freq[t0 + wi].end());
        if (freq_all.size() != nw * n_gt * ploidy_f) throw std::runtime_error("internal: a window's table of haplotype scores has another length");
        device_check(dev_, vgmi_hmm_part_calls_fre(ph.p, ploidy_f, freq_all.data(), (uint32_t)nw, plan->row.data(), plan->restart.data(), plan->n_steps, &uniform,
                                                   plan->chains.data(), (uint32_t)plan->chains.size(), plan->gid.data(), plan->order.data(), plan->fwd.data(),
                                                   plan->bwd.data(), prob.data(), winner.data()),
                     "device HMM recursion: ");
    } else if (plan->n_steps)
        device_check(dev_, vgmi_hmm_part_calls_plan(ph.p, plan->plan, prob.data(), winner.data()), "device HMM recursion: ");
    const int64_t t_calls = s.since_begin();
    if (g_phase_on)
        std::fprintf(stderr, "[varigraph-mi] HMM part %zu (windows %zu-%zu): emissions, recursion and posterior on the device from %.3f to %.3f s (%zu of %zu nodes scored by the host, %zu scored again on the device): "
                     "emission kernel %.3f, sequence checks (host) %.3f, rows fixed on the device %.3f, plan (strings + step tables: once per graph) %.3f, recursion + posterior %.3f\n",
                     part, t0, t1 - 1, ta * 1e-9, t_calls * 1e-9, fl.n_host, n_rows, fl.n_fixed, (t_emit - ta) * 1e-9, (t_a - t_emit) * 1e-9, (t_rows - t_a) * 1e-9,
                     (t_b - t_rows) * 1e-9, (t_calls - t_b) * 1e-9);
    s.note_device_span(ta, t_calls);
    // the calls' k-mer tallies on the device too (the node lists and the sample's coverage are there for the emissions):
    // per sample, the walk over every called node's k-mer list was 0.8 of 1.7 host thread-seconds (VGH_DEVICE_TALLIES=0: the walk).
    // A tri- or tetraploid sample's through vgmi_hmm_tallies_ploidy: one window, the sample's one list by haplotype id, whole lists
    // (ploidy 5 .. 8: the walk, finish_rows).
    const uint32_t ploidy = cfg.sample_ploidy;
    std::vector<uint32_t> tally;      // per row 2 x ploidy numbers
    std::vector<uint8_t> tally_uniq;
    static const bool device_tallies = !knob_off("VGH_DEVICE_TALLIES");
    if (device_tallies && plan->n_steps && device_tally_ploidy(ploidy) && n_hap_ <= 64 && n_gt <= 128) {
        std::vector<uint8_t> haps_all(n_gt * ploidy);
        bool ids = true;
        for (size_t g2 = 0; g2 < n_gt && ids; ++g2)
            for (uint32_t q = 0; q < ploidy; ++q) {
                if (ps.genotypes[g2][q] > 254) { ids = false; break; }
                haps_all[g2 * ploidy + q] = (uint8_t)ps.genotypes[g2][q];
            }
        uint64_t sel = 0;
        for (uint16_t hap : ps.top)
            if (hap < n_hap_ && hap < 64) sel |= 1ull << hap;
        if (ids) {
            tally.resize(2 * (size_t)ploidy * n_rows);
            tally_uniq.resize(n_rows);
            device_check(dev_, vgmi_hmm_tallies_ploidy(dev_, ploidy, (uint32_t)n_gt, 1, nullptr, haps_all.data(), &sel, n_rows, pc.e_begin.data(), pc.e_count.data(),
                                                       nullptr, winner.data(), 0, tally.data(), tally_uniq.data()),
                         "device tallies: ");
            ps.ploidy_tally_rows += n_rows;
        }
    }
    if (device_tallies && plan->n_steps && cfg.sample_ploidy == 2 && n_hap_ <= 64 && n_gt <= 128) {
        std::vector<uint8_t> hap_ab(2 * n_gt, 0xFF);
        bool pairs = true;
        for (size_t g2 = 0; g2 < n_gt; ++g2) {
            if (ps.genotypes[g2].size() != 2 || ps.genotypes[g2][0] > 254 || ps.genotypes[g2][1] > 254) { pairs = false; break; }
            hap_ab[2 * g2] = (uint8_t)ps.genotypes[g2][0];
            hap_ab[2 * g2 + 1] = (uint8_t)ps.genotypes[g2][1];
        }
        uint64_t sel = 0;
        for (uint16_t hap : ps.top)
            if (hap < n_hap_ && hap < 64) sel |= 1ull << hap;
        if (pairs) {
            tally.resize(4 * n_rows);
            tally_uniq.resize(n_rows);
            device_check(dev_, vgmi_hmm_tallies(dev_, n_rows, pc.e_begin.data(), pc.e_count.data(), winner.data(), (uint32_t)n_gt, hap_ab.data(), n_hap_, sel,
                                                tally.data(), tally_uniq.data()),
                         "device tallies: ");
        }
    }
    over_windows(nw, helpers, g_phase.pass_c, [&](size_t wi) {
        const size_t t = t0 + wi;
        const Chrom& chr = *s.tasks[t].chr;
        const std::vector<uint32_t>& rows_w = plan->win_rows[wi];
        if (tally.empty()) finish_rows(s.tasks[t].chr, rows_w, pc.row_node.data(), haps, prob.data(), winner.data(), r);
        // the lines of the scored rows -- no other node has a call -- with the head of every line taken from the plan instead of the site map
        s.piece_done[t] = 1;
        std::string out;
        size_t room = 0;
        for (const uint32_t rw : rows_w) room += (size_t)(plan->line_head_off[rw + 1] - plan->line_head_off[rw]) + 48;
        out.reserve(room);
        std::vector<uint64_t> gt;
        for (const uint32_t rw : rows_w) {
            auto head = [&](std::string& o) {
                const uint64_t h0 = plan->line_head_off[rw], h1 = plan->line_head_off[rw + 1];
                if (h0 != h1) o.append(plan->line_head, h0, h1 - h0);
                return h0 != h1;      // false: no such site in the VCF
            };
            const Node& node = chr.nodes[pc.row_node[rw]];
            if (tally.empty()) append_call_line(out, node, cfg.min_gq, gt, head);
            else if (winner[rw] < n_gt) {      // (else no entry with a positive posterior: no call)
                const std::vector<uint16_t>& called = ps.genotypes[winner[rw]];
                append_tally_line(out, node.gn->hap_gt, called.data(), ploidy, prob[rw], &tally[2 * (size_t)ploidy * rw], tally_uniq[rw], cfg.min_gq, head);
            }
        }
        s.pieces[t] = std::move(out);
        s.emit_windows_done += !rows_w.empty();
    });
}

// ---------------------------------------------------------------- emissions on the device, haplotypes selected per window
// -n below the graph's haplotypes, a diploid sample: DESIGN_INGEST_HMM.md 4.13.
// The reference draws every window's haplotypes from their k-mer support, drops from a node's list every k-mer no drawn haplotype
// carries -- for good -- and scores what is left (src/genotype.cpp:500-610, 673-686, 815-818).  haplotype_combinations over the sorted
// draw yields pairs over -n places whatever was drawn: positions, keep matrix and the shape of every step are the sample's, the
// haplotype at each place is the window's.  Support sums, emissions (with the prune), recursion, posterior and tallies run on the
// device; the draws (std::mt19937, libm), the sequence checks (strings), the step tables (libm) and the genotype strings stay here.
// A row is the range [front, back] of what is left of its node's list plus the device's alive bytes; node.kmers is pruned by the same
// rule right after the emission launch, so that the host's lists and the device's bytes agree after every sample.
// A polyploid sample (ploidy 3 .. 8) takes the same steps with another genotype list: haplotype_combinations turns every drawn haplotype into
// the block of `ploidy` consecutive haplotypes that holds it (:846-873), so a window has 1 .. -n genotypes over up to -n x ploidy
// haplotypes -- `used`, which the scores, the sequence checks and the strings go by -- while the prune still goes by the drawn ones.  The
// device's recursion takes one list length per part: the windows are dealt into parts by the length of their lists (SelectedPart), each
// with its own emission launch, keep matrix per window and 1 / n_gt, and its own tally launch (vgmi_hmm_tallies_ploidy) over the same lists:
// the lines of a polyploid sample are written from the device's numbers as a diploid sample's are.
// Over a graph of 7 to 64 bytes of haplotype bits (Run::wide) the entries are on the device as bytes and every mask over haplotype ids is
// mask_words words: a diploid sample always (4.16; above 32 bytes the _wide16 calls with 16-bit ids, 4.21), a polyploid one up to 32 bytes when VGH_HMM_WIDE_PLOIDY_DEVICE=1 asks for it and its windows name at
// most 64 haplotypes, the width of the masks over places that the sequence checks and gt0 work on (4.18; id_masks.hpp).
struct Genotyper::SelectedSample {
    float ave = 0;
    double lower = 256.0f, upper = -0.1f;
    uint32_t ploidy = 2, n_drawn = 0;
    bool blocks = false;                     // polyploid: a genotype list per window
    std::vector<long double> tab;
    std::vector<uint8_t> pos_a, pos_b, keep_mat;      // diploid: the one shape of every window's list
    // per window of the run
    std::vector<std::vector<uint16_t>> win_top, win_used;      // drawn, ascending / occurring in the genotypes, ascending (diploid: the drawn ones)
    std::vector<std::vector<std::vector<uint16_t>>> win_gts;
    std::vector<GenotypeList> win_glist;
    std::vector<uint8_t> win_used8;          // diploid: the drawn haplotypes as the device takes them
    std::vector<uint16_t> win_used16;        // ... above 32 bytes of haplotype bits, where an id does not fit a byte (ids16)
    bool ids16 = false;
    std::vector<uint64_t> win_mask;          // the drawn haplotypes: mask_words words per window (one unless the entries are bytes)
    uint32_t mask_words = 1;
    bool wide = false;                       // the entries are on the device as bytes (7 to 64 of them): the _wide calls, _wide16 above 32
    bool by_freq = false;                    // `-m fre`: no keep matrix, no powers; per window the table of its genotypes' haplotypes' scores
    std::vector<std::vector<long double>> win_freq;
    // what the VGH_TIMING line sums over the parts
    size_t n_fixed_rows = 0, n_host_rows = 0, n_pruned = 0, n_parts = 0, n_ploidy_tally_rows = 0;
    int64_t ns_emit = 0, ns_a = 0, ns_rows = 0, ns_b = 0, ns_calls = 0, t_last = 0;
    const std::vector<uint16_t>& used(size_t wi) const { return blocks ? win_used[wi] : win_top[wi]; }
    WindowHaps haps(size_t wi) const { return WindowHaps{win_top[wi], used(wi), win_gts[wi], win_glist[wi]}; }
};

// The windows of a sample whose genotype lists have `n_gt` entries, and their rows end to end (a diploid sample: every window)
struct Genotyper::SelectedPart {
    size_t n_gt = 0;
    std::vector<uint32_t> wins;              // the run's windows, ascending
    std::vector<size_t> win_row0;            // wins.size() + 1
    std::vector<uint64_t> e_begin;
    std::vector<uint32_t> e_count, row_win, row_node;      // row_win: a place in `wins`
    std::vector<uint64_t> gt0;               // per row: the places of the window's `used` whose haplotype carries the reference allele
};

Genotyper::Emitted Genotyper::hmm_selected(RunShared& s)
{
    const Run& r = s.r;
    const GenotypeConfig& cfg = *r.cfg;
    const std::vector<Task>& tasks = s.tasks;
    const size_t n_entries = g_.node_key_index.size();
    const double tb0 = s.since_begin() * 1e-9;
    SelectedSample ss;
    ss.ave = r.hap_cov;
    poisson_interval(ss.ave, ss.lower, ss.upper);
    ss.ploidy = cfg.sample_ploidy;
    ss.blocks = cfg.sample_ploidy > 2;
    ss.n_drawn = r.haploid_num;
    ss.by_freq = cfg.transition == "fre";
    const uint32_t n_used = ss.n_drawn;
    size_t n_gt = 0;      // diploid: of every window
    if (!ss.blocks) {
        std::vector<uint16_t> places(n_used);
        std::iota(places.begin(), places.end(), (uint16_t)0);
        const std::vector<std::vector<uint16_t>> shape = haplotype_combinations(places, cfg.sample_type, 2, (uint16_t)(n_hap_ - 1));
        n_gt = shape.size();
        bool pairs = n_gt >= 1 && n_gt <= 128;
        for (const auto& gtv : shape) pairs = pairs && gtv.size() == 2;
        if (!pairs) return Emitted::no;
        ss.pos_a.resize(n_gt);
        ss.pos_b.resize(n_gt);
        for (size_t gi = 0; gi < n_gt; ++gi) {
            ss.pos_a[gi] = (uint8_t)shape[gi][0];
            ss.pos_b[gi] = (uint8_t)shape[gi][1];
        }
        if (!ss.by_freq) ss.keep_mat = keep_matrix(shape);      // (places keep the haplotypes' order)
    }
    ss.tab = emission_table(ss.ave, ss.ploidy);
    ss.wide = r.packed == nullptr;
    if (ss.wide && !r.wide) throw std::runtime_error("internal: a sample without packed entries on the selected path");
    ss.mask_words = ss.wide ? vgh::words_of((uint32_t)g_.bitlen) : 1u;
    const uint32_t bit_len = (uint32_t)g_.bitlen;
    ss.ids16 = ss.wide && bit_len > 32;
    if (!entries_uploaded_) {
        if (ss.wide) upload_entries_wide(s.n_threads);
        else device_check(dev_, vgmi_hmm_entries_upload(dev_, packed_.data(), packed_.size()), "device HMM emissions: ");
        entries_uploaded_ = true;
        if (!lists_whole_.load()) alive_stale_.store(true);
    }
    device_check(dev_, vgmi_hmm_sample_upload(dev_, r.cov, n_entries), "device HMM emissions: ");
    if (alive_stale_.load()) {      // a sample of this run took a host path: the lists as the host left them
        std::vector<uint8_t> alive(n_entries, 0);
        for (const auto& c : chroms_)
            for (const auto& n : c.nodes)
                for (uint32_t pos : n.kmers) alive[pos] = 1;
        device_check(dev_, vgmi_hmm_alive_upload(dev_, alive.data(), n_entries), "device HMM emissions: ");
        alive_stale_.store(false);
    }
    const size_t nw = tasks.size();
    // rows, window after window.  Support reads every node with more than one allele; the HMM works on those --sv leaves.
    std::vector<uint64_t> sup_begin, e_begin_sv;
    std::vector<uint32_t> sup_count, sup_win, sup_node, e_count_sv, e_win_sv, e_node_sv;
    std::vector<size_t> win_row0(nw + 1, 0);
    {
        CpuBudget::Hold cpu;
        PhaseTimer t_list(g_phase.list);
        for (size_t t = 0; t < nw; ++t) {
            const Chrom& chr = *tasks[t].chr;
            const SiteMap& sites = vcf_sites(chr);
            for (uint32_t i = tasks[t].first; i < tasks[t].last; ++i) {
                const Node& n = chr.nodes[i];
                if (n.gn->hap_gt.size() <= 1) continue;
                const uint64_t b = n.kmers.empty() ? 0 : n.kmers.front();
                const uint32_t cnt = n.kmers.empty() ? 0 : n.kmers.back() - n.kmers.front() + 1;
                sup_begin.push_back(b);
                sup_count.push_back(cnt);
                sup_win.push_back((uint32_t)t);
                sup_node.push_back(i);
                if (cfg.sv_only && !skipped(chr, sites, n, true)) {
                    e_begin_sv.push_back(b);
                    e_count_sv.push_back(cnt);
                    e_win_sv.push_back((uint32_t)t);
                    e_node_sv.push_back(i);
                }
            }
            win_row0[t + 1] = cfg.sv_only ? e_begin_sv.size() : sup_begin.size();
        }
    }
    const std::vector<uint64_t>& e_begin = cfg.sv_only ? e_begin_sv : sup_begin;
    const std::vector<uint32_t>&e_count = cfg.sv_only ? e_count_sv : sup_count, &row_node = cfg.sv_only ? e_node_sv : sup_node;
    const size_t n_rows = e_begin.size();
    const int64_t ta = s.since_begin();
    // 1. the support the draw is weighted by, on the device
    std::vector<uint32_t> support(nw * n_hap_, 0);
    if (ss.ids16)
        device_check(dev_, vgmi_hmm_support_wide16(dev_, bit_len, n_hap_, (uint32_t)nw, sup_begin.size(), sup_begin.data(), sup_count.data(), sup_win.data(), support.data()),
                     "device HMM support: ");
    else if (ss.wide)
        device_check(dev_, vgmi_hmm_support_wide(dev_, bit_len, n_hap_, (uint32_t)nw, sup_begin.size(), sup_begin.data(), sup_count.data(), sup_win.data(), support.data()),
                     "device HMM support: ");
    else
        device_check(dev_, vgmi_hmm_support(dev_, n_hap_, (uint32_t)nw, sup_begin.size(), sup_begin.data(), sup_count.data(), sup_win.data(), support.data()),
                     "device HMM support: ");
    const int64_t t_sup = s.since_begin();
    // 2. the draws; 3. what follows from them: the window's haplotypes and mask, its genotypes, the rows' reference-allele masks
    ss.win_top.resize(nw);
    ss.win_used.resize(ss.blocks ? nw : 0);
    ss.win_gts.resize(nw);
    ss.win_glist.resize(nw);
    ss.win_used8.assign(ss.blocks || ss.ids16 ? 0 : nw * n_used, 0);
    ss.win_used16.assign(ss.ids16 ? nw * n_used : 0, 0);
    ss.win_mask.assign(nw * ss.mask_words, 0);
    ss.win_freq.resize(ss.by_freq ? nw : 0);
    std::vector<uint64_t> gt0(n_rows ? n_rows : 1, 0);
    over_windows(nw, s.n_threads, g_phase.select, [&](size_t wi) {
        HaplotypeSampler sampler(std::vector<uint32_t>(support.begin() + wi * n_hap_, support.begin() + (wi + 1) * n_hap_), (int)r.haploid_num);
        std::vector<uint16_t>& top = ss.win_top[wi];
        top = sampler.top;
        std::sort(top.begin(), top.end());
        if (top.size() != n_used) throw std::runtime_error("internal: a window drew another number of haplotypes");
        for (size_t p = 0; p < n_used; ++p) ss.win_mask[wi * ss.mask_words + (top[p] >> 6)] |= 1ULL << (top[p] & 63u);      // (packed entries: ids below 47, one word)
        if (ss.blocks) {
            ss.win_gts[wi] = haplotype_combinations(top, cfg.sample_type, ss.ploidy, (uint16_t)(n_hap_ - 1));
            std::vector<uint16_t>& used = ss.win_used[wi];
            for (const auto& gtv : ss.win_gts[wi]) used.insert(used.end(), gtv.begin(), gtv.end());
            std::sort(used.begin(), used.end());
            used.erase(std::unique(used.begin(), used.end()), used.end());
        } else {
            if (ss.ids16) std::copy(top.begin(), top.end(), ss.win_used16.begin() + wi * n_used);
            else for (size_t p = 0; p < n_used; ++p) ss.win_used8[wi * n_used + p] = (uint8_t)top[p];
            ss.win_gts[wi].resize(n_gt);
            for (size_t gi = 0; gi < n_gt; ++gi) ss.win_gts[wi][gi] = {top[ss.pos_a[gi]], top[ss.pos_b[gi]]};
        }
        const std::vector<uint16_t>& used = ss.used(wi);
        ss.win_glist[wi] = genotype_list(ss.win_gts[wi], used);
        if (ss.by_freq) ss.win_freq[wi] = frequency_table(ss.win_gts[wi], sampler.score);
        const Chrom& chr = *tasks[wi].chr;
        for (size_t rr = win_row0[wi]; rr < win_row0[wi + 1]; ++rr) {
            const auto& hap_gt = chr.nodes[row_node[rr]].gn->hap_gt;
            uint64_t m = 0;
            for (size_t p = 0; p < used.size(); ++p) m |= (uint64_t)(hap_gt[used[p]] == 0) << p;
            gt0[rr] = m;
        }
    });
    const int64_t t_draw = s.since_begin();
    ss.t_last = t_draw;
    // the parts: the windows by the length of their genotype lists (a diploid sample: one part)
    std::vector<SelectedPart> parts;
    {
        CpuBudget::Hold cpu;
        PhaseTimer t_list(g_phase.list);
        std::map<size_t, size_t> part_of;      // list length -> part
        for (size_t wi = 0; wi < nw; ++wi) {
            const size_t len = ss.win_gts[wi].size();
            if (len < 1 || (ss.blocks && (len > 64 || ss.used(wi).size() > 64))) throw std::runtime_error("internal: a window's genotype list the device cannot take");
            auto it = part_of.find(len);
            if (it == part_of.end()) {
                it = part_of.emplace(len, parts.size()).first;
                parts.emplace_back();
                parts.back().n_gt = len;
                parts.back().win_row0.push_back(0);
            }
            SelectedPart& pt = parts[it->second];
            const uint32_t place = (uint32_t)pt.wins.size();
            pt.wins.push_back((uint32_t)wi);
            const size_t lo = win_row0[wi], hi = win_row0[wi + 1];
            pt.e_begin.insert(pt.e_begin.end(), e_begin.begin() + lo, e_begin.begin() + hi);
            pt.e_count.insert(pt.e_count.end(), e_count.begin() + lo, e_count.begin() + hi);
            pt.row_node.insert(pt.row_node.end(), row_node.begin() + lo, row_node.begin() + hi);
            pt.gt0.insert(pt.gt0.end(), gt0.begin() + lo, gt0.begin() + hi);
            pt.row_win.insert(pt.row_win.end(), hi - lo, place);
            pt.win_row0.push_back(pt.e_begin.size());
        }
    }
    size_t n_steps = 0;
    for (const SelectedPart& pt : parts) n_steps += selected_part(s, ss, pt);
    s.note_device_span(ta, ss.t_last);
    (void)n_steps;
    if (g_phase_on) {
        std::fprintf(stderr, "[varigraph-mi] HMM with haplotypes selected per window (%zu windows, %zu rows, %zu nodes pruned, %zu nodes scored by the host, %zu scored "
                     "again on the device): support %.3f, draws (host) %.3f, emission kernel %.3f, prune + sequence checks (host) %.3f, rows fixed on the device %.3f, "
                     "strings + step tables (host) %.3f, recursion + posterior %.3f\n",
                     nw, n_rows, ss.n_pruned, ss.n_host_rows, ss.n_fixed_rows, (t_sup - ta) * 1e-9, (t_draw - t_sup) * 1e-9, ss.ns_emit * 1e-9, ss.ns_a * 1e-9,
                     ss.ns_rows * 1e-9, ss.ns_b * 1e-9, ss.ns_calls * 1e-9);
        std::fprintf(stderr, "[varigraph-mi] HMM emissions on the device: %zu parts, %.2f s; haplotypes selected per window for %zu of %zu windows\n",
                     std::max<size_t>(1, parts.size()), s.since_begin() * 1e-9 - tb0, nw, tasks.size());
        if (ss.n_ploidy_tally_rows) std::fprintf(stderr, "[varigraph-mi] HMM tallies on the device: %zu rows, ploidy %u\n", ss.n_ploidy_tally_rows, ss.ploidy);
        if (ss.by_freq) std::fprintf(stderr, "[varigraph-mi] HMM transitions by haplotype frequency on the device: %zu windows\n", s.emit_windows_done.load());
    }
    return Emitted::yes;
}

// Steps 4 to 9 for one part; returns its steps
size_t Genotyper::selected_part(RunShared& s, SelectedSample& ss, const SelectedPart& pt)
{
    const Run& r = s.r;
    const GenotypeConfig& cfg = *r.cfg;
    const std::vector<Task>& tasks = s.tasks;
    const size_t n_gt = pt.n_gt, nwp = pt.wins.size(), n_rows = pt.e_begin.size();
    const float ave = ss.ave;
    const double lower = ss.lower, upper = ss.upper;
    const std::vector<size_t>& win_row0 = pt.win_row0;
    const std::vector<uint32_t>& row_node = pt.row_node;
    const int64_t t_begin = s.since_begin();
    int64_t t_emit = t_begin, t_a = t_begin, t_rows = t_begin, t_b = t_begin, t_calls = t_begin;
    std::vector<long double> prob(n_rows ? n_rows : 1);
    std::vector<uint32_t> winner(n_rows ? n_rows : 1, 0xFFFFFFFFu);
    std::vector<std::vector<uint32_t>> win_rows(nwp);      // per window: the rows that have a score
    size_t n_steps = 0;
    // a list per window: the lists by haplotype id and the drawn haplotypes, for the emission launch and the tallies
    std::vector<uint32_t> w_n;
    std::vector<uint8_t> w_haps;
    std::vector<uint64_t> w_mask;
    if (n_rows) {
        // 4. emission scores on the device, the prune included
        std::vector<uint32_t> n_kept(n_rows);
        std::vector<uint8_t> flags(n_rows);
        PartHandle ph;
        if (ss.blocks) {
            // ... and the rows' reference-allele masks over haplotype ids
            w_n.assign(nwp, (uint32_t)n_gt);
            w_haps.resize(nwp * n_gt * ss.ploidy);
            const size_t W = ss.mask_words;      // (packed entries: one word per window, row and fix)
            w_mask.resize(nwp * W);
            std::vector<uint64_t> gt0_ids(n_rows * W, 0);
            for (size_t lw = 0; lw < nwp; ++lw) {
                const size_t wi = pt.wins[lw];
                std::copy_n(&ss.win_mask[wi * W], W, &w_mask[lw * W]);
                for (size_t gi = 0; gi < n_gt; ++gi)
                    for (uint32_t q = 0; q < ss.ploidy; ++q) w_haps[(lw * n_gt + gi) * ss.ploidy + q] = (uint8_t)ss.win_gts[wi][gi][q];
                const std::vector<uint16_t>& used = ss.win_used[wi];
                for (size_t rr = win_row0[lw]; rr < win_row0[lw + 1]; ++rr) vgh::places_to_ids(pt.gt0[rr], used.data(), used.size(), &gt0_ids[rr * W]);
            }
            if (ss.wide)
                device_check(dev_, vgmi_hmm_emissions_select_ploidy_wide(dev_, (uint32_t)n_gt, ss.ploidy, (uint32_t)nwp, w_n.data(), w_haps.data(), w_mask.data(),
                                                                         (uint32_t)g_.bitlen, ave, lower, upper, ss.tab.data(), n_rows, pt.e_begin.data(),
                                                                         pt.e_count.data(), pt.row_win.data(), gt0_ids.data(), n_kept.data(), flags.data(), &ph.p),
                             "device HMM emissions: ");
            else
                device_check(dev_, vgmi_hmm_emissions_select_ploidy(dev_, (uint32_t)n_gt, ss.ploidy, (uint32_t)nwp, w_n.data(), w_haps.data(), w_mask.data(),
                                                                    (uint32_t)g_.bitlen, ave, lower, upper, ss.tab.data(), n_rows, pt.e_begin.data(), pt.e_count.data(),
                                                                    pt.row_win.data(), gt0_ids.data(), n_kept.data(), flags.data(), &ph.p),
                             "device HMM emissions: ");
        } else {
            const std::vector<uint16_t> gt0_16(pt.gt0.begin(), pt.gt0.end());      // (<= 16 places)
            if (ss.ids16)
                device_check(dev_, vgmi_hmm_emissions_select_wide16(dev_, (uint32_t)n_gt, ss.n_drawn, ss.pos_a.data(), ss.pos_b.data(), (uint32_t)nwp, ss.win_used16.data(),
                                                                    ss.win_mask.data(), (uint32_t)g_.bitlen, ave, lower, upper, ss.tab.data(), n_rows, pt.e_begin.data(),
                                                                    pt.e_count.data(), pt.row_win.data(), gt0_16.data(), n_kept.data(), flags.data(), &ph.p),
                             "device HMM emissions: ");
            else if (ss.wide)      // (a diploid sample has one part: its windows are the run's, in order, and so are the masks)
                device_check(dev_, vgmi_hmm_emissions_select_wide(dev_, (uint32_t)n_gt, ss.n_drawn, ss.pos_a.data(), ss.pos_b.data(), (uint32_t)nwp, ss.win_used8.data(),
                                                                  ss.win_mask.data(), (uint32_t)g_.bitlen, ave, lower, upper, ss.tab.data(), n_rows, pt.e_begin.data(),
                                                                  pt.e_count.data(), pt.row_win.data(), gt0_16.data(), n_kept.data(), flags.data(), &ph.p),
                             "device HMM emissions: ");
            else
                device_check(dev_, vgmi_hmm_emissions_select(dev_, (uint32_t)n_gt, ss.n_drawn, ss.pos_a.data(), ss.pos_b.data(), (uint32_t)nwp, ss.win_used8.data(),
                                                             ss.win_mask.data(), (uint32_t)g_.bitlen, ave, lower, upper, ss.tab.data(), n_rows, pt.e_begin.data(),
                                                             pt.e_count.data(), pt.row_win.data(), gt0_16.data(), n_kept.data(), flags.data(), &ph.p),
                             "device HMM emissions: ");
        }
        t_emit = s.since_begin();
        // 5. the same prune on the host's lists, for exactly the nodes that lost k-mers; 6. the flagged rows
        FlaggedRows fl(nwp);
        std::atomic<size_t> pruned_nodes{0};
        over_windows(nwp, s.n_threads, g_phase.pass_a, [&](size_t lw) {
            const size_t wi = pt.wins[lw];
            Chrom& chr = *tasks[wi].chr;
            const WindowHaps haps = ss.haps(wi);
            std::vector<uint32_t> kept;
            FlaggedScratch sc(ave, lower, upper);
            for (size_t rr = win_row0[lw]; rr < win_row0[lw + 1]; ++rr) {
                Node& node = chr.nodes[row_node[rr]];
                if (n_kept[rr] != node.kmers.size()) {
                    kept.clear();
                    if (ss.wide) {      // the entry's bytes in the graph's bit vectors against the window's words
                        const size_t bl = g_.bitlen;
                        const uint64_t* const mask = &ss.win_mask[wi * ss.mask_words];
                        for (uint32_t pos : node.kmers)
                            if (vgh::meets_bytes(reinterpret_cast<const uint8_t*>(&g_.bitvec[(size_t)g_.node_key_index[pos] * bl]), (uint32_t)bl, mask)) kept.push_back(pos);
                    } else {
                        for (uint32_t pos : node.kmers)
                            if (vgh::meets_packed(r.packed[pos], ss.win_mask[wi])) kept.push_back(pos);
                    }
                    if (kept.size() != n_kept[rr]) throw std::runtime_error("internal: the device's k-mer lists differ from the host's");
                    node.kmers.keep(kept);
                    ++pruned_nodes;
                }
                if (!(flags[rr] & 1u)) continue;
                const size_t before = fl.fix_j[lw].size(), before_m = fl.fix_mask[lw].size();
                flagged_row(fl, lw, rr, chr, row_node[rr], haps, pt.gt0[rr], r, sc, n_kept[rr]);
                // (sequence_fixes counts along the list and over the places of `used`; the device along the row's range -- and, with a list
                // per window, over haplotype ids: mask_words words per fix)
                for (size_t q = before; q < fl.fix_j[lw].size(); ++q) fl.fix_j[lw][q] = node.kmers[fl.fix_j[lw][q]] - (uint32_t)pt.e_begin[rr];
                if (ss.blocks) {
                    const size_t W = ss.mask_words;
                    const std::vector<uint64_t> places(fl.fix_mask[lw].begin() + (ptrdiff_t)before_m, fl.fix_mask[lw].end());
                    fl.fix_mask[lw].resize(before_m);
                    fl.fix_mask[lw].resize(before_m + places.size() * W, 0);
                    for (size_t q = 0; q < places.size(); ++q) vgh::places_to_ids(places[q], haps.used.data(), haps.used.size(), &fl.fix_mask[lw][before_m + q * W]);
                }
            }
        });
        ss.n_pruned += pruned_nodes.load();
        if (pruned_nodes.load()) lists_whole_.store(false, std::memory_order_relaxed);
        alive_stale_.store(false);      // (hidden_states above walked lists that were pruned already: nothing left them)
        t_a = s.since_begin();
        upload_flagged(fl, ph.p, ss.blocks, ss.blocks && ss.wide);
        ss.n_host_rows += fl.n_host;
        ss.n_fixed_rows += fl.n_fixed;
        t_rows = s.since_begin();
        // 7. the recursion's inputs: genotype strings (the window's haplotypes decide them), step tables (libm), chains
        std::vector<std::vector<Seen>> seen(nwp);
        std::vector<uint8_t> gid(n_rows * n_gt, 0), order(n_rows * n_gt, 0);
        over_windows(nwp, s.n_threads, g_phase.pass_a, [&](size_t lw) {
            row_strings(*tasks[pt.wins[lw]].chr, win_row0[lw], win_row0[lw + 1], row_node.data(), pt.gt0.data(), n_kept.data(), ss.haps(pt.wins[lw]), gid.data(),
                        order.data(), seen[lw], win_rows[lw]);
        });
        StepArrays steps(win_rows, n_rows, ss.ploidy, ss.blocks || ss.by_freq, !ss.by_freq);
        n_steps = steps.n_steps;
        if (n_steps) over_windows(nwp, s.n_threads, g_phase.pass_b, [&](size_t lw) { steps.fill(lw, seen[lw], (uint16_t)n_hap_); });
        t_b = s.since_begin();
        if (n_steps && ss.by_freq) {      // a table of factors per window in place of keep matrix and powers
            const long double uniform = 1.0L / (long double)n_gt;
            std::vector<long double> freq_all;
            freq_all.reserve(nwp * n_gt * ss.ploidy);
            for (size_t lw = 0; lw < nwp; ++lw) freq_all.insert(freq_all.end(), ss.win_freq[pt.wins[lw]].begin(), ss.win_freq[pt.wins[lw]].end());
            if (freq_all.size() != nwp * n_gt * ss.ploidy) throw std::runtime_error("internal: a window's table of haplotype scores has another length");
            device_check(dev_, vgmi_hmm_part_calls_fre(ph.p, ss.ploidy, freq_all.data(), (uint32_t)nwp, steps.row.data(), steps.restart.data(), n_steps, &uniform,
                                                       steps.chains.data(), (uint32_t)steps.chains.size(), gid.data(), order.data(), steps.fwd.data(),
                                                       steps.bwd.data(), prob.data(), winner.data()),
                         "device HMM recursion: ");
        } else if (n_steps) {
            const long double uniform = 1.0L / (long double)n_gt;
            std::vector<uint8_t> keep_all;      // a list per window: a keep matrix per window
            if (ss.blocks) {
                keep_all.reserve(nwp * n_gt * n_gt);
                for (size_t lw = 0; lw < nwp; ++lw) {
                    const std::vector<uint8_t> km = keep_matrix(ss.win_gts[pt.wins[lw]]);
                    keep_all.insert(keep_all.end(), km.begin(), km.end());
                }
            }
            device_check(dev_, vgmi_hmm_part_calls(ph.p, ss.ploidy, ss.blocks ? keep_all.data() : ss.keep_mat.data(), ss.blocks ? (uint32_t)nwp : 1u, steps.row.data(),
                                                   steps.restart.data(), steps.pw.data(), n_steps, &uniform, steps.chains.data(), (uint32_t)steps.chains.size(),
                                                   gid.data(), order.data(), steps.fwd.data(), steps.bwd.data(), prob.data(), winner.data()),
                         "device HMM recursion: ");
        }
        t_calls = s.since_begin();
    }
    ss.ns_emit += t_emit - t_begin;
    ss.ns_a += t_a - t_emit;
    ss.ns_rows += t_rows - t_a;
    ss.ns_b += t_b - t_rows;
    ss.ns_calls += t_calls - t_b;
    ss.t_last = t_calls;
    // 8. the calls' tallies on the device (VGH_DEVICE_TALLIES=0: the walk over the called nodes' lists); a polyploid sample's over the lists
    // of the emission launch, the drawn haplotypes being the ones that count
    std::vector<uint32_t> tally;      // per row 2 x ploidy numbers
    std::vector<uint8_t> tally_uniq;
    static const bool device_tallies = !knob_off("VGH_DEVICE_TALLIES");
    if (device_tallies && n_steps && ss.blocks && device_tally_ploidy(ss.ploidy)) {
        tally.resize(2 * (size_t)ss.ploidy * n_rows);
        tally_uniq.resize(n_rows);
        if (ss.wide)
            device_check(dev_, vgmi_hmm_tallies_ploidy_wide(dev_, (uint32_t)g_.bitlen, ss.ploidy, (uint32_t)n_gt, (uint32_t)nwp, w_n.data(), w_haps.data(), w_mask.data(),
                                                            n_rows, pt.e_begin.data(), pt.e_count.data(), pt.row_win.data(), winner.data(), 1, tally.data(),
                                                            tally_uniq.data()),
                         "device tallies: ");
        else
            device_check(dev_, vgmi_hmm_tallies_ploidy(dev_, ss.ploidy, (uint32_t)n_gt, (uint32_t)nwp, w_n.data(), w_haps.data(), w_mask.data(), n_rows, pt.e_begin.data(),
                                                       pt.e_count.data(), pt.row_win.data(), winner.data(), 1, tally.data(), tally_uniq.data()),
                         "device tallies: ");
        ss.n_ploidy_tally_rows += n_rows;
    }
    if (device_tallies && n_steps && !ss.blocks) {
        tally.resize(4 * n_rows);
        tally_uniq.resize(n_rows);
        if (ss.ids16)
            device_check(dev_, vgmi_hmm_tallies_select_wide16(dev_, (uint32_t)g_.bitlen, n_rows, pt.e_begin.data(), pt.e_count.data(), pt.row_win.data(), winner.data(),
                                                              (uint32_t)n_gt, ss.pos_a.data(), ss.pos_b.data(), ss.n_drawn, (uint32_t)nwp, ss.win_used16.data(), tally.data(),
                                                              tally_uniq.data()),
                         "device tallies: ");
        else if (ss.wide)
            device_check(dev_, vgmi_hmm_tallies_select_wide(dev_, (uint32_t)g_.bitlen, n_rows, pt.e_begin.data(), pt.e_count.data(), pt.row_win.data(), winner.data(),
                                                            (uint32_t)n_gt, ss.pos_a.data(), ss.pos_b.data(), ss.n_drawn, (uint32_t)nwp, ss.win_used8.data(), tally.data(),
                                                            tally_uniq.data()),
                         "device tallies: ");
        else
            device_check(dev_, vgmi_hmm_tallies_select(dev_, n_rows, pt.e_begin.data(), pt.e_count.data(), pt.row_win.data(), winner.data(), (uint32_t)n_gt, ss.pos_a.data(),
                                                       ss.pos_b.data(), ss.n_drawn, (uint32_t)nwp, ss.win_used8.data(), tally.data(), tally_uniq.data()),
                         "device tallies: ");
    }
    // 9. the lines
    over_windows(nwp, s.n_threads, g_phase.pass_c, [&](size_t lw) {
        const size_t wi = pt.wins[lw];
        s.emit_windows_done += !win_rows[lw].empty();
        const Chrom& chr = *tasks[wi].chr;
        if (tally.empty()) {
            finish_rows(tasks[wi].chr, win_rows[lw], row_node.data(), ss.haps(wi), prob.data(), winner.data(), r);
            write_piece(s, wi);
            return;
        }
        s.piece_done[wi] = 1;
        auto vc = g_.vcf_info.find(chr.name);
        if (vc == g_.vcf_info.end()) return;
        SiteWalk walk(vc->second);
        std::string out;
        for (const uint32_t rw : win_rows[lw]) {
            const Node& node = chr.nodes[row_node[rw]];
            const std::vector<std::string>* fields = walk.at(node.start);
            if (winner[rw] >= n_gt) continue;            // no entry with a positive posterior: no call
            const std::vector<uint16_t>& called = ss.win_gts[wi][winner[rw]];
            append_tally_line(out, node.gn->hap_gt, called.data(), ss.ploidy, prob[rw], &tally[2 * (size_t)ss.ploidy * rw], tally_uniq[rw], cfg.min_gq,
                              [&](std::string& o) { return append_site_head(o, fields); });
        }
        s.pieces[wi] = std::move(out);
    });
    return n_steps;
}

std::string Genotyper::run(const uint8_t* cov, float hap_kmer_coverage, const std::string& sample_name,
                           const GenotypeConfig& cfg, const uint8_t* cov_node)
{
    const auto t_begin = std::chrono::steady_clock::now();
    std::vector<uint8_t> gathered;
    if (!cov_node) {      // a caller with per-key counters only (tests, the C API): the per-node gather on the host
        const size_t n_entries = g_.node_key_index.size();
        gathered.resize(n_entries);
        for (size_t j = 0; j < n_entries; ++j) gathered[j] = cov[g_.node_key_index[j]];
        cov_node = gathered.data();
    }
    Run r;
    r.cov = cov_node;
    r.hap_cov = hap_kmer_coverage;
    r.cfg = &cfg;
    r.haploid_num = std::min(cfg.haploid_num, n_hap_);
    if (g_.bitlen <= 6) fill_packed(r, cfg.threads);
    else      // (a polyploid sample over such a graph only when asked and up to 32 bytes: VGH_HMM_WIDE_PLOIDY_DEVICE=1, DESIGN_INGEST_HMM.md 4.18; a diploid one
              // up to 64 bytes, 4.21)
        r.wide = !knob_off("VGH_HMM_WIDE_DEVICE") &&
                 ((cfg.sample_ploidy == 2 && g_.bitlen <= 64) ||
                  (knob_on("VGH_HMM_WIDE_PLOIDY_DEVICE") && vgh::wide_ploidy_sample(g_.bitlen, cfg.sample_ploidy, r.haploid_num)));
    reset_calls();

    RunShared s(r);
    s.t_begin = t_begin;
    s.tasks = windows(cfg);
    s.n_threads = std::max(1u, std::min<uint32_t>(cfg.threads, (uint32_t)s.tasks.size()));
    s.pieces.resize(s.tasks.size());
    s.piece_done.assign(s.tasks.size(), 0);

    std::vector<WindowWork> works;
    // (VGH_HMM_FAKE_NOMEM: as if the device had no room for the first sample of a run whose haplotypes are selected per window -- it takes
    // the pool, the host prunes its lists, and the next sample has to start from those)
    const bool refuse_select = getenv("VGH_HMM_FAKE_NOMEM") != nullptr && samples_run_ == 0;
    ++samples_run_;
    const DevicePaths paths = device_paths(r, s.tasks, works, refuse_select);
    WindowBuffers bufs;
    if (paths.pool_device) {
        bufs.allocate(paths.total_room, paths.n_gt, cfg.sample_ploidy);
        for (WindowWork& w : works) bufs.bind(w);
    }
    const Emitted emitted = paths.emit ? hmm_whole_panel(s) : paths.select ? hmm_selected(s) : Emitted::no;
    if (emitted == Emitted::lists_pruned) {
        // a list was pruned after all (or would be): this graph takes the host's preparation from now on
        emit_device_off_ = true;
        return run(cov, hap_kmer_coverage, sample_name, cfg, cov_node);
    }
    if (emitted == Emitted::no) hmm_on_pool(s, works, bufs, paths.n_gt);

    const bool emitted_on_device = emitted == Emitted::yes;
    last_device_seconds = s.dev_last.load() > 0 ? (double)(s.dev_last.load() - s.dev_first.load()) * 1e-9 : 0;
    last_windows = s.tasks.size();
    last_device_windows = emitted_on_device ? s.emit_windows_done.load() : 0;
    for (const auto& w : works) last_device_windows += w.on_device && !w.nodes.empty();
    const auto t_hmm = std::chrono::steady_clock::now();
    last_hmm_seconds = std::chrono::duration<double>(t_hmm - t_begin).count();
    if (g_phase_on) {
        std::fprintf(stderr, "[varigraph-mi] HMM thread-seconds: selection %.2f, hidden states %.2f, emissions %.2f, forward %.2f, backward %.2f, posterior %.2f (wall %.2f on %u threads)\n",
                     g_phase.select.exchange(0) * 1e-9, g_phase.states.exchange(0) * 1e-9, g_phase.emit.exchange(0) * 1e-9, g_phase.fwd.exchange(0) * 1e-9,
                     g_phase.bwd.exchange(0) * 1e-9, g_phase.post.exchange(0) * 1e-9, last_hmm_seconds, s.n_threads);
        if (last_device_seconds > 0) std::fprintf(stderr, "[varigraph-mi] HMM recursion on the device: %.2f s\n", last_device_seconds);
        if (emitted_on_device)
            std::fprintf(stderr, "[varigraph-mi] host thread-seconds around the device (all samples in flight since the last line of this kind): node lists %.2f, "
                         "host-scored nodes + genotype strings %.2f, step tables %.2f, calls + VCF lines %.2f, coverage words %.2f, text joined %.2f, in line for a thread %.2f\n",
                         g_phase.list.exchange(0) * 1e-9, g_phase.pass_a.exchange(0) * 1e-9, g_phase.pass_b.exchange(0) * 1e-9, g_phase.pass_c.exchange(0) * 1e-9,
                         g_phase.fill.exchange(0) * 1e-9, g_phase.text.exchange(0) * 1e-9, g_cpu_wait_ns.exchange(0) * 1e-9);
    }

    // ---- the pieces that are not written yet (windows without a device call), then the whole text
    {
        std::atomic<size_t> next_text{0};
        auto text_worker = [&]() {
            for (;;) {
                const size_t t = next_text.fetch_add(1);
                if (t >= s.tasks.size()) return;
                if (!s.piece_done[t]) {
                    CpuBudget::Hold cpu;
                    write_piece(s, t);
                }
            }
        };
        std::vector<std::thread> tpool;
        for (uint32_t t = 1; t < s.n_threads; ++t) tpool.emplace_back(text_worker);
        text_worker();
        for (auto& th : tpool) th.join();
    }
    // the graph's chromosomes are a std::map like mVcfInfoMap: the tasks are already in the reference's output order
    CpuBudget::Hold cpu;
    PhaseTimer t_text(g_phase.text);
    std::ostringstream oss;
    oss << g_.vcf_head + "\t" + sample_name + "\n";
    for (const auto& piece : s.pieces) oss << piece;
    // SAVE::save strips the newlines around each 10 MB chunk and adds one back (src/save.cpp:16-24); on the whole
    // text that is: no leading newline, exactly one trailing
    std::string text = strip_newlines(oss.str());
    if (!text.empty()) text += "\n";
    last_text_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_hmm).count();
    return text;
}

// SAVE writes the text through gzwrite (src/save.cpp:11-30); the bytes of a .gz depend on the zlib build anyway, what
// has to be identical is the content.  Here the text goes out as block gzip (BGZF: gzip members of <= 64 KiB with the
// 'BC' extra field, the form bgzip / tabix expect for VCFs) and the blocks are deflated by `threads` workers.
void Genotyper::write_gz(const std::string& path, const std::string& text, unsigned threads)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) throw std::runtime_error("'" + path + "': No such file or directory or possibly reached the maximum open file limit.");
    constexpr size_t kBlock = 0xff00;
    const size_t n_blocks = (text.size() + kBlock - 1) / kBlock;
    std::vector<std::string> out(n_blocks);
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    auto worker = [&]() {
        std::vector<unsigned char> buf(compressBound(kBlock) + 64);
        for (;;) {
            const size_t b = next.fetch_add(1);
            if (b >= n_blocks) return;
            CpuBudget::Hold cpu;
            const size_t off = b * kBlock, len = std::min(kBlock, text.size() - off);
            z_stream zs;
            std::memset(&zs, 0, sizeof zs);
            if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) { failed = true; return; }
            zs.next_in = reinterpret_cast<Bytef*>(const_cast<char*>(text.data() + off));
            zs.avail_in = (uInt)len;
            zs.next_out = buf.data();
            zs.avail_out = (uInt)buf.size();
            const int rc = deflate(&zs, Z_FINISH);
            const size_t clen = buf.size() - zs.avail_out;
            deflateEnd(&zs);
            if (rc != Z_STREAM_END || clen + 26 > 65536) { failed = true; return; }
            const uint32_t crc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), reinterpret_cast<const Bytef*>(text.data() + off), (uInt)len);
            const uint16_t bsize = (uint16_t)(clen + 25);
            std::string& o = out[b];
            o.reserve(clen + 26);
            static const unsigned char head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
            o.append(reinterpret_cast<const char*>(head), 16);
            o.push_back((char)(bsize & 0xFF));
            o.push_back((char)(bsize >> 8));
            o.append(reinterpret_cast<const char*>(buf.data()), clen);
            for (uint32_t v : {crc, (uint32_t)len})
                for (int sh = 0; sh < 32; sh += 8) o.push_back((char)((v >> sh) & 0xFF));
        }
    };
    const unsigned n_threads = (unsigned)std::max<size_t>(1, std::min<size_t>(threads ? threads : 1, n_blocks));
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < n_threads; ++t) pool.emplace_back(worker);
    worker();
    for (auto& th : pool) th.join();
    bool ok = !failed.load();
    for (size_t b = 0; ok && b < n_blocks; ++b) ok = fwrite(out[b].data(), 1, out[b].size(), f) == out[b].size();
    static const unsigned char eof_block[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    ok = ok && fwrite(eof_block, 1, sizeof eof_block, f) == sizeof eof_block;
    ok = (fclose(f) == 0) && ok;
    if (!ok) throw std::runtime_error("'" + path + "': write error");
}

}  // namespace vgh
