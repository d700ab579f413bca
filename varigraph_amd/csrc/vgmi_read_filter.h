// The rule of `genotype --min-read-length / --max-read-length / --min-read-quality / --max-low-quality`, written once: the host readers,
// the device kernels (vgmi_fastq.hip, vgmi_bam.hip include this header) and the stand-alone check (tests/native/read_filter_check.cpp)
// all call the functions below.  Not the reference's behaviour (it has no such options): the result is the reference's on the file with
// the failing reads removed.  It lies beside the kernels' headers, where the build's header glob finds it.
//
// Everything is integer arithmetic: no pow, no floating point in any verdict -- a float sum's order would differ between a wavefront
// and the host reader.
//
// Parameters (all off by default):
//   min_len        0 = off            max_len        0 = none
//   min_mean_q     tenths of a Phred unit, 0 .. 930, 0 = off
//   lowq_below     0 .. 93, 0 = off   lowq_max_pct   0 .. 100
// Per-base quality q: FASTQ clamp(byte - 33, 0, 93) on the unsigned byte; BAM min(QUAL[i], 93).  A BAM record whose QUAL[0] is 0xff and
// a FASTA record have no qualities: only the length tests apply, both quality tests pass.
// Error table: E10[t] = round_half_even(10^(-t/100) * 2^30), t = 0 .. 930 (tools/gen_read_filter_table.py; E10[0] = 2^30); a base of
// quality q weighs E[q] = E10[10 q].
// Tests, in this order -- the first that fails is the read's class (len: the sequence length):
//   1 short         len < min_len
//   2 long          max_len && len > max_len
//   3 low fraction  lowq_below && cnt(q < lowq_below) * 100 > lowq_max_pct * len            (fastp -q / -u: strictly more than PCT percent)
//   4 low mean      min_mean_q && sum E[q_i] > E10[min_mean_q] * len                        (chopper / NanoFilt: the mean error probability,
//                                                                                            not the mean Phred; equality passes)
// All sums and products are unsigned 64-bit, exact for len < 2^31 (E <= 2^30).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VGH_READ_FILTER_HD __host__ __device__
#else
#define VGH_READ_FILTER_HD
#endif

namespace vgh {

enum : int { READ_PASS = 0, READ_SHORT = 1, READ_LONG = 2, READ_LOW_FRACTION = 3, READ_LOW_MEAN = 4 };

#define VGH_READ_FILTER_MAX_TENTHS 930u
#define VGH_READ_FILTER_MAX_Q 93u
#define VGH_READ_FILTER_MAX_LEN 0x7FFFFFFFull      // the sums are exact below 2^31 bases

// E10[t], t <= 930
VGH_READ_FILTER_HD inline uint32_t read_filter_e10(uint32_t t)
{
    static constexpr uint32_t E10[931] = {
        // VGH_E10_BEGIN
        1073741824u, 1049300476u, 1025415481u, 1002074175u, 979264182u, 956973408u, 935190034u, 913902510u, 893099549u, 872770121u,      // 0
        852903448u, 833488995u, 814516469u, 795975811u, 777857189u, 760150998u, 742847849u, 725938567u, 709414188u, 693265950u,      // 10
        677485290u, 662063842u, 646993429u, 632266061u, 617873928u, 603809400u, 590065020u, 576633501u, 563507720u, 550680718u,      // 20
        538145694u, 525896003u, 513925148u, 502226784u, 490794706u, 479622855u, 468705306u, 458036271u, 447610092u, 437421243u,      // 30
        427464319u, 417734044u, 408225256u, 398932915u, 389852093u, 380977976u, 372305858u, 363831142u, 355549334u, 347456043u,      // 40
        339546978u, 331817945u, 324264847u, 316883678u, 309670525u, 302621563u, 295733055u, 289001349u, 282422875u, 275994146u,      // 50
        269711752u, 263572363u, 257572723u, 251709652u, 245980041u, 240380852u, 234909116u, 229561931u, 224336464u, 219229942u,      // 60
        214239660u, 209362970u, 204597287u, 199940084u, 195388892u, 190941298u, 186594943u, 182347524u, 178196787u, 174140533u,      // 70
        170176611u, 166302918u, 162517402u, 158818054u, 155202914u, 151670064u, 148217632u, 144843787u, 141546739u, 138324742u,      // 80
        135176087u, 132099103u, 129092161u, 126153664u, 123282056u, 120475814u, 117733450u, 115053509u, 112434572u, 109875248u,      // 90
        107374182u, 104930048u, 102541548u, 100207418u, 97926418u, 95697341u, 93519003u, 91390251u, 89309955u, 87277012u,      // 100
        85290345u, 83348899u, 81451647u, 79597581u, 77785719u, 76015100u, 74284785u, 72593857u, 70941419u, 69326595u,      // 110
        67748529u, 66206384u, 64699343u, 63226606u, 61787393u, 60380940u, 59006502u, 57663350u, 56350772u, 55068072u,      // 120
        53814569u, 52589600u, 51392515u, 50222678u, 49079471u, 47962285u, 46870531u, 45803627u, 44761009u, 43742124u,      // 130
        42746432u, 41773404u, 40822526u, 39893291u, 38985209u, 38097798u, 37230586u, 36383114u, 35554933u, 34745604u,      // 140
        33954698u, 33181795u, 32426485u, 31688368u, 30967052u, 30262156u, 29573306u, 28900135u, 28242288u, 27599415u,      // 150
        26971175u, 26357236u, 25757272u, 25170965u, 24598004u, 24038085u, 23490912u, 22956193u, 22433646u, 21922994u,      // 160
        21423966u, 20936297u, 20459729u, 19994008u, 19538889u, 19094130u, 18659494u, 18234752u, 17819679u, 17414053u,      // 170
        17017661u, 16630292u, 16251740u, 15881805u, 15520291u, 15167006u, 14821763u, 14484379u, 14154674u, 13832474u,      // 180
        13517609u, 13209910u, 12909216u, 12615366u, 12328206u, 12047581u, 11773345u, 11505351u, 11243457u, 10987525u,      // 190
        10737418u, 10493005u, 10254155u, 10020742u, 9792642u, 9569734u, 9351900u, 9139025u, 8930995u, 8727701u,      // 200
        8529034u, 8334890u, 8145165u, 7959758u, 7778572u, 7601510u, 7428478u, 7259386u, 7094142u, 6932659u,      // 210
        6774853u, 6620638u, 6469934u, 6322661u, 6178739u, 6038094u, 5900650u, 5766335u, 5635077u, 5506807u,      // 220
        5381457u, 5258960u, 5139251u, 5022268u, 4907947u, 4796229u, 4687053u, 4580363u, 4476101u, 4374212u,      // 230
        4274643u, 4177340u, 4082253u, 3989329u, 3898521u, 3809780u, 3723059u, 3638311u, 3555493u, 3474560u,      // 240
        3395470u, 3318179u, 3242648u, 3168837u, 3096705u, 3026216u, 2957331u, 2890013u, 2824229u, 2759941u,      // 250
        2697118u, 2635724u, 2575727u, 2517097u, 2459800u, 2403809u, 2349091u, 2295619u, 2243365u, 2192299u,      // 260
        2142397u, 2093630u, 2045973u, 1999401u, 1953889u, 1909413u, 1865949u, 1823475u, 1781968u, 1741405u,      // 270
        1701766u, 1663029u, 1625174u, 1588181u, 1552029u, 1516701u, 1482176u, 1448438u, 1415467u, 1383247u,      // 280
        1351761u, 1320991u, 1290922u, 1261537u, 1232821u, 1204758u, 1177334u, 1150535u, 1124346u, 1098752u,      // 290
        1073742u, 1049300u, 1025415u, 1002074u, 979264u, 956973u, 935190u, 913903u, 893100u, 872770u,      // 300
        852903u, 833489u, 814516u, 795976u, 777857u, 760151u, 742848u, 725939u, 709414u, 693266u,      // 310
        677485u, 662064u, 646993u, 632266u, 617874u, 603809u, 590065u, 576634u, 563508u, 550681u,      // 320
        538146u, 525896u, 513925u, 502227u, 490795u, 479623u, 468705u, 458036u, 447610u, 437421u,      // 330
        427464u, 417734u, 408225u, 398933u, 389852u, 380978u, 372306u, 363831u, 355549u, 347456u,      // 340
        339547u, 331818u, 324265u, 316884u, 309671u, 302622u, 295733u, 289001u, 282423u, 275994u,      // 350
        269712u, 263572u, 257573u, 251710u, 245980u, 240381u, 234909u, 229562u, 224336u, 219230u,      // 360
        214240u, 209363u, 204597u, 199940u, 195389u, 190941u, 186595u, 182348u, 178197u, 174141u,      // 370
        170177u, 166303u, 162517u, 158818u, 155203u, 151670u, 148218u, 144844u, 141547u, 138325u,      // 380
        135176u, 132099u, 129092u, 126154u, 123282u, 120476u, 117733u, 115054u, 112435u, 109875u,      // 390
        107374u, 104930u, 102542u, 100207u, 97926u, 95697u, 93519u, 91390u, 89310u, 87277u,      // 400
        85290u, 83349u, 81452u, 79598u, 77786u, 76015u, 74285u, 72594u, 70941u, 69327u,      // 410
        67749u, 66206u, 64699u, 63227u, 61787u, 60381u, 59007u, 57663u, 56351u, 55068u,      // 420
        53815u, 52590u, 51393u, 50223u, 49079u, 47962u, 46871u, 45804u, 44761u, 43742u,      // 430
        42746u, 41773u, 40823u, 39893u, 38985u, 38098u, 37231u, 36383u, 35555u, 34746u,      // 440
        33955u, 33182u, 32426u, 31688u, 30967u, 30262u, 29573u, 28900u, 28242u, 27599u,      // 450
        26971u, 26357u, 25757u, 25171u, 24598u, 24038u, 23491u, 22956u, 22434u, 21923u,      // 460
        21424u, 20936u, 20460u, 19994u, 19539u, 19094u, 18659u, 18235u, 17820u, 17414u,      // 470
        17018u, 16630u, 16252u, 15882u, 15520u, 15167u, 14822u, 14484u, 14155u, 13832u,      // 480
        13518u, 13210u, 12909u, 12615u, 12328u, 12048u, 11773u, 11505u, 11243u, 10988u,      // 490
        10737u, 10493u, 10254u, 10021u, 9793u, 9570u, 9352u, 9139u, 8931u, 8728u,      // 500
        8529u, 8335u, 8145u, 7960u, 7779u, 7602u, 7428u, 7259u, 7094u, 6933u,      // 510
        6775u, 6621u, 6470u, 6323u, 6179u, 6038u, 5901u, 5766u, 5635u, 5507u,      // 520
        5381u, 5259u, 5139u, 5022u, 4908u, 4796u, 4687u, 4580u, 4476u, 4374u,      // 530
        4275u, 4177u, 4082u, 3989u, 3899u, 3810u, 3723u, 3638u, 3555u, 3475u,      // 540
        3395u, 3318u, 3243u, 3169u, 3097u, 3026u, 2957u, 2890u, 2824u, 2760u,      // 550
        2697u, 2636u, 2576u, 2517u, 2460u, 2404u, 2349u, 2296u, 2243u, 2192u,      // 560
        2142u, 2094u, 2046u, 1999u, 1954u, 1909u, 1866u, 1823u, 1782u, 1741u,      // 570
        1702u, 1663u, 1625u, 1588u, 1552u, 1517u, 1482u, 1448u, 1415u, 1383u,      // 580
        1352u, 1321u, 1291u, 1262u, 1233u, 1205u, 1177u, 1151u, 1124u, 1099u,      // 590
        1074u, 1049u, 1025u, 1002u, 979u, 957u, 935u, 914u, 893u, 873u,      // 600
        853u, 833u, 815u, 796u, 778u, 760u, 743u, 726u, 709u, 693u,      // 610
        677u, 662u, 647u, 632u, 618u, 604u, 590u, 577u, 564u, 551u,      // 620
        538u, 526u, 514u, 502u, 491u, 480u, 469u, 458u, 448u, 437u,      // 630
        427u, 418u, 408u, 399u, 390u, 381u, 372u, 364u, 356u, 347u,      // 640
        340u, 332u, 324u, 317u, 310u, 303u, 296u, 289u, 282u, 276u,      // 650
        270u, 264u, 258u, 252u, 246u, 240u, 235u, 230u, 224u, 219u,      // 660
        214u, 209u, 205u, 200u, 195u, 191u, 187u, 182u, 178u, 174u,      // 670
        170u, 166u, 163u, 159u, 155u, 152u, 148u, 145u, 142u, 138u,      // 680
        135u, 132u, 129u, 126u, 123u, 120u, 118u, 115u, 112u, 110u,      // 690
        107u, 105u, 103u, 100u, 98u, 96u, 94u, 91u, 89u, 87u,      // 700
        85u, 83u, 81u, 80u, 78u, 76u, 74u, 73u, 71u, 69u,      // 710
        68u, 66u, 65u, 63u, 62u, 60u, 59u, 58u, 56u, 55u,      // 720
        54u, 53u, 51u, 50u, 49u, 48u, 47u, 46u, 45u, 44u,      // 730
        43u, 42u, 41u, 40u, 39u, 38u, 37u, 36u, 36u, 35u,      // 740
        34u, 33u, 32u, 32u, 31u, 30u, 30u, 29u, 28u, 28u,      // 750
        27u, 26u, 26u, 25u, 25u, 24u, 23u, 23u, 22u, 22u,      // 760
        21u, 21u, 20u, 20u, 20u, 19u, 19u, 18u, 18u, 17u,      // 770
        17u, 17u, 16u, 16u, 16u, 15u, 15u, 14u, 14u, 14u,      // 780
        14u, 13u, 13u, 13u, 12u, 12u, 12u, 12u, 11u, 11u,      // 790
        11u, 10u, 10u, 10u, 10u, 10u, 9u, 9u, 9u, 9u,      // 800
        9u, 8u, 8u, 8u, 8u, 8u, 7u, 7u, 7u, 7u,      // 810
        7u, 7u, 6u, 6u, 6u, 6u, 6u, 6u, 6u, 6u,      // 820
        5u, 5u, 5u, 5u, 5u, 5u, 5u, 5u, 4u, 4u,      // 830
        4u, 4u, 4u, 4u, 4u, 4u, 4u, 4u, 4u, 3u,      // 840
        3u, 3u, 3u, 3u, 3u, 3u, 3u, 3u, 3u, 3u,      // 850
        3u, 3u, 3u, 3u, 2u, 2u, 2u, 2u, 2u, 2u,      // 860
        2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u, 2u,      // 870
        2u, 2u, 2u, 2u, 2u, 2u, 1u, 1u, 1u, 1u,      // 880
        1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u,      // 890
        1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u,      // 900
        1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u,      // 910
        1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u, 1u,      // 920
        1u,      // 930
        // VGH_E10_END
    };
    return E10[t];
}

// the quality of a FASTQ quality byte / a BAM QUAL byte
VGH_READ_FILTER_HD inline uint32_t read_filter_q_fastq(uint32_t byte) { return byte < 33u ? 0u : byte - 33u > 93u ? 93u : byte - 33u; }
VGH_READ_FILTER_HD inline uint32_t read_filter_q_bam(uint32_t byte) { return byte > 93u ? 93u : byte; }
// E of a base of quality q <= 93
VGH_READ_FILTER_HD inline uint32_t read_filter_e(uint32_t q) { return read_filter_e10(10u * q); }

// what the kernels take (FqBuffers::rf, BamBuffers::rf) and the readers carry.  on == 0: nothing is evaluated, every read passes.
struct ReadFilterParams {
    uint32_t on;              // any test set
    uint32_t min_len, max_len;
    uint32_t min_mean_q;      // tenths
    uint32_t lowq_below, lowq_max_pct;
    uint32_t mean_bound;      // E10[min_mean_q] (0 with the test off)
    uint32_t pad;
    VGH_READ_FILTER_HD bool quality() const { return min_mean_q || lowq_below; }      // a test that reads quality bytes
    VGH_READ_FILTER_HD bool lengths() const { return min_len || max_len; }
};

// 0: valid; else the first field out of range (1 max_len below min_len, 2 min_mean_q, 3 lowq_below, 4 lowq_max_pct, 5 a percentage without a bound)
inline int read_filter_invalid(uint32_t min_len, uint32_t max_len, uint32_t min_mean_q, uint32_t lowq_below, uint32_t lowq_max_pct)
{
    if (max_len && max_len < min_len) return 1;
    if (min_mean_q > VGH_READ_FILTER_MAX_TENTHS) return 2;
    if (lowq_below > VGH_READ_FILTER_MAX_Q) return 3;
    if (lowq_max_pct > 100u) return 4;
    if (!lowq_below && lowq_max_pct) return 5;
    return 0;
}
inline const char* read_filter_invalid_text(int field)
{
    switch (field) {
    case 1: return "maximum read length is below the minimum read length";
    case 2: return "minimum read quality is out of range (0..93, in tenths: 0..930)";
    case 3: return "low-quality bound is out of range (0..93, Phred)";
    case 4: return "low-quality percentage is out of range (0..100)";
    case 5: return "a low-quality percentage needs a low-quality bound (1..93)";
    default: return "";
    }
}

inline ReadFilterParams read_filter_params(uint32_t min_len = 0, uint32_t max_len = 0, uint32_t min_mean_q = 0, uint32_t lowq_below = 0,
                                           uint32_t lowq_max_pct = 0)
{
    ReadFilterParams p{};
    p.min_len = min_len;
    p.max_len = max_len;
    p.min_mean_q = min_mean_q;
    p.lowq_below = lowq_below;
    p.lowq_max_pct = lowq_below ? lowq_max_pct : 0u;
    p.mean_bound = min_mean_q ? read_filter_e10(min_mean_q) : 0u;
    p.on = (min_len || max_len || min_mean_q || lowq_below) ? 1u : 0u;
    return p;
}

// tests 1 and 2
VGH_READ_FILTER_HD inline int read_filter_length_class(const ReadFilterParams& p, uint64_t len)
{
    if (len < p.min_len) return READ_SHORT;
    if (p.max_len && len > p.max_len) return READ_LONG;
    return READ_PASS;
}
// tests 3 and 4 from a read's two sums: n_low = cnt(q < lowq_below), sum_e = sum E[q_i]
VGH_READ_FILTER_HD inline int read_filter_quality_class(const ReadFilterParams& p, uint64_t len, uint64_t n_low, uint64_t sum_e)
{
    if (p.lowq_below && n_low * 100u > (uint64_t)p.lowq_max_pct * len) return READ_LOW_FRACTION;
    if (p.min_mean_q && sum_e > (uint64_t)p.mean_bound * len) return READ_LOW_MEAN;
    return READ_PASS;
}

// A read's class on the host: qual = its len quality bytes as stored (null: none -- FASTA), bam: QUAL bytes (QUAL[0] == 0xff: none) in
// place of Phred+33 characters.  n_low / sum_e (may be null) get the two sums where a quality test evaluated them, else 0.
inline int read_filter_class(const ReadFilterParams& p, const unsigned char* qual, uint64_t len, bool bam, uint64_t* n_low = nullptr,
                             uint64_t* sum_e = nullptr)
{
    if (n_low) *n_low = 0;
    if (sum_e) *sum_e = 0;
    const int lc = read_filter_length_class(p, len);
    if (lc || !p.quality() || !qual || !len || (bam && qual[0] == 0xFFu)) return lc;
    uint64_t low = 0, sum = 0;
    for (uint64_t i = 0; i < len; ++i) {
        const uint32_t q = bam ? read_filter_q_bam(qual[i]) : read_filter_q_fastq(qual[i]);
        low += q < p.lowq_below;
        sum += read_filter_e(q);
    }
    if (n_low) *n_low = low;
    if (sum_e) *sum_e = sum;
    return read_filter_quality_class(p, len, low, sum);
}

// "Q" with at most one fractional digit -> tenths, by its characters alone: digits, at most one '.', one digit behind it, no sign, no
// leading zero in front of another digit, at most 93.0.  false for anything else.
inline bool read_filter_parse_tenths(const char* s, uint32_t* tenths)
{
    if (!s || !*s) return false;
    uint32_t whole = 0, n = 0;
    const char* p = s;
    for (; *p >= '0' && *p <= '9'; ++p, ++n) {
        if (n >= 2) return false;
        whole = whole * 10u + (uint32_t)(*p - '0');
    }
    if (!n || (n > 1 && s[0] == '0')) return false;
    uint32_t frac = 0;
    if (*p == '.') {
        ++p;
        if (!(*p >= '0' && *p <= '9')) return false;
        frac = (uint32_t)(*p - '0');
        ++p;
    }
    if (*p) return false;
    const uint32_t t = whole * 10u + frac;
    if (t > VGH_READ_FILTER_MAX_TENTHS) return false;
    *tenths = t;
    return true;
}

// what a reader carries: the parameters and the class counts of the reads it evaluated
struct ReadFilterRule {
    ReadFilterParams p = read_filter_params();
    uint64_t n_class[5] = {0, 0, 0, 0, 0};      // [READ_PASS] = kept
    ReadFilterRule() = default;
    explicit ReadFilterRule(const ReadFilterParams& q) : p(q) {}
    bool on() const { return p.on != 0; }
    uint64_t evaluated() const { return n_class[0] + n_class[1] + n_class[2] + n_class[3] + n_class[4]; }
};

}  // namespace vgh
