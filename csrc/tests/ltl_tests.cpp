// gol-mi355x: host-side tests of Larger than Life rules (no GPU needed).  Run: build/gol_ltl_unit
//
// Covers: the rule strings (accepted forms, the alias, the canonical string, ltl(), every rejection), the folding of the
// middle flag into the four thresholds on the box sum that includes the centre (M0 and M1, the clamps), and
// cpu::superstep under such rules on both boundaries against a per-cell count written here.
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "gol/bits.hpp"
#include "gol/cpu.hpp"
#include "gol/geometry.hpp"
#include "gol/rule.hpp"

using namespace gol;

static int g_fail = 0, g_pass = 0;
#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            if (g_fail < 20) fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                                                     \
        } else {                                                                          \
            ++g_pass;                                                                     \
        }                                                                                 \
    } while (0)

// the string must be refused as an invalid rule, with an error that names it (and holds `word` when one is given)
static void check_rejected(const std::string& s, const std::string& word = "") {
    bool threw = false, named = false, worded = word.empty();
    try {
        Rule::parse(s);
    } catch (const Error& e) {
        const std::string what = e.what();
        threw = true;
        named = what.find("invalid rule '" + s + "'") != std::string::npos;
        worded = worded || what.find(word) != std::string::npos;
        if (!worded) fprintf(stderr, "'%s': no '%s' in: %s\n", s.c_str(), word.c_str(), e.what());
    }
    if (!threw) fprintf(stderr, "accepted: '%s'\n", s.c_str());
    CHECK(threw);
    CHECK(named);
    CHECK(worded);
}

static void test_strings() {
    const std::string bosco = "R5,C0,M1,S34..58,B34..45,NM";
    const Rule b = Rule::parse(bosco);
    CHECK(b.ltl() && b.range == 5 && b.middle == 1 && b.smin == 34 && b.smax == 58 && b.bmin == 34 && b.bmax == 45);
    CHECK(b.states == 2 && !b.generations() && !b.is_conway() && b.nbhd == Nbhd::Moore && b.box() == 121);
    CHECK(b.str() == bosco);
    for (const char* s : {"bosco", "Bosco", "BOSCO", "r5,c0,m1,s34..58,b34..45,nm", "R5,C0,M1,S34..58,B34..45", "R5,C2,M1,S34..58,B34..45,NM",
                          "r5,C2,m1,S34..58,b34..45"})
        CHECK(Rule::parse(s) == b && Rule::parse(s).str() == bosco);
    CHECK(Rule::parse("R1,C0,M0,S2..3,B3..3,NM").str() == "R1,C0,M0,S2..3,B3..3,NM");
    CHECK(Rule::parse("R7,C0,M1,S63..108,B63..84,NM").range == 7);
    CHECK(Rule::parse("R7,C0,M0,S0..225,B1..225,NM").smax == 225);
    CHECK(Rule::parse("R1,C0,M0,S0..0,B9..9").str() == "R1,C0,M0,S0..0,B9..9,NM");
    CHECK(Rule::from_ltl(5, 1, 34, 58, 34, 45) == b);
    // every existing rule is what it was: not LtL, its masks, string and code
    for (const char* s : {"B3/S23", "B36/S23", "B2/S345/C4", "B13/S13V", "replicator", "conway"}) CHECK(!Rule::parse(s).ltl());
    CHECK(Rule::parse("replicator").str() == "B1357/S1357");
    CHECK(Rule().range == 0 && Rule().is_conway() && Rule::from_code(Rule().code()) == Rule());
    CHECK(Rule::parse("B3/S23") != Rule::parse("R1,C0,M0,S2..3,B3..3"));

    check_rejected("R0,C0,M1,S1..1,B1..1,NM", "R1 to R7");
    check_rejected("R8,C0,M1,S34..58,B34..45,NM", "R1 to R7");
    check_rejected("R10,C0,M1,S34..58,B34..45,NM", "R1 to R7");
    check_rejected("R5,C3,M1,S34..58,B34..45,NM", "not built");
    check_rejected("R5,C255,M1,S34..58,B34..45,NM", "history states");
    check_rejected("R5,C1,M1,S34..58,B34..45,NM");
    check_rejected("R5,C0,M2,S34..58,B34..45,NM", "M0");
    check_rejected("R5,C0,M1,S34..58,B34..45,NN", "NN");
    check_rejected("R5,C0,M1,S34..58,B34..45,NC", "NC");
    check_rejected("R5,C0,M1,S34..58,B34..45,NX");
    check_rejected("R5,C0,M1,S34..58,B34..45,N");
    check_rejected("R5,C0,M1,S58..34,B34..45,NM", "min <= max");
    check_rejected("R5,C0,M1,S34..122,B34..45,NM", "121");
    check_rejected("R5,C0,M1,S34..58,B45..34,NM", "min <= max");
    check_rejected("R5,C0,M1,S34..58,B34..122,NM", "121");
    check_rejected("R1,C0,M0,S2..3,B3..10,NM", "9");
    check_rejected("R5,C0,M1,S34..58,B0..45,NM", "B0 rules are out of scope");
    check_rejected("R5,C0,M1,S34..58,B0..0,NM", "B0 rules are out of scope");
    check_rejected("R5,R5,C0,M1,S34..58,B34..45,NM", "twice");
    check_rejected("R5,C0,M1,S34..58,S34..58,B34..45,NM", "twice");
    check_rejected("R5,C0,M1,S34..58,B34..45,NM,NM", "twice");
    check_rejected("R5,M1,S34..58,B34..45,NM", "missing");
    check_rejected("R5,C0,S34..58,B34..45,NM", "missing");
    check_rejected("R5,C0,M1,B34..45,NM", "missing");
    check_rejected("R5,C0,M1,S34..58,NM", "missing");
    check_rejected("R5,C0,M1,S34..58,B34..45,NM,", "trailing comma");
    check_rejected("R5,C0,M1,S34..58,B34..45,", "trailing comma");
    check_rejected("R5, C0,M1,S34..58,B34..45,NM", "spaces");
    check_rejected("R5,C0,M1,S34..58,B34..45,NM ", "spaces");
    check_rejected("R05,C0,M1,S34..58,B34..45,NM", "leading zero");
    check_rejected("R5,C00,M1,S34..58,B34..45,NM", "leading zero");
    check_rejected("R5,C0,M1,S034..58,B34..45,NM", "leading zero");
    check_rejected("R5,C0,M1,S34..058,B34..45,NM", "leading zero");
    check_rejected("R5,C0,M1,S34-58,B34..45,NM");
    check_rejected("R5,C0,M1,S34..,B34..45,NM");
    check_rejected("R5,C0,M1,S..58,B34..45,NM");
    check_rejected("R5,C0,M1,S34...58,B34..45,NM");
    check_rejected("R,C0,M1,S34..58,B34..45,NM");
    check_rejected("R5,,C0,M1,S34..58,B34..45,NM");
    check_rejected("R5,C0,M1,B34..45,S34..58,NM", "order");
    check_rejected("R5,C0,M1,S34..58,B34..45,NM,X1");
    check_rejected("R5,C0,M1,S34..58,B34..45,NM/C3");
    check_rejected("R5");
    check_rejected("R99999,C0,M1,S1..1,B1..1");
    bool threw = false;
    try {
        Rule::from_ltl(5, 1, 34, 58, 0, 45);
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
}

static void test_thresholds() {
    // M1: the count is T itself
    Rule::LtlThresholds t = Rule::parse("bosco").ltl_thresholds();
    CHECK(t.blo == 34 && t.bhi == 45 && t.slo == 34 && t.shi == 58);
    // M0: a live centre adds one to T
    t = Rule::parse("R5,C0,M0,S33..57,B34..45,NM").ltl_thresholds();
    CHECK(t.blo == 34 && t.bhi == 45 && t.slo == 34 && t.shi == 58);
    t = Rule::parse("R1,C0,M0,S2..3,B3..3").ltl_thresholds();
    CHECK(t.blo == 3 && t.bhi == 3 && t.slo == 3 && t.shi == 4);
    t = Rule::parse("R1,C0,M0,S0..0,B1..1").ltl_thresholds();  // a lone live cell: T = 1
    CHECK(t.slo == 1 && t.shi == 1);
    // the clamps: smax + 1 above the box is the box; smin + 1 above the box is an empty interval
    t = Rule::parse("R1,C0,M0,S2..9,B3..9").ltl_thresholds();
    CHECK(t.slo == 3 && t.shi == 9 && t.bhi == 9);
    t = Rule::parse("R1,C0,M0,S9..9,B3..3").ltl_thresholds();  // nine neighbours without the centre: never
    CHECK(t.slo > t.shi && t.slo <= 9);
    t = Rule::parse("R7,C0,M0,S225..225,B1..225").ltl_thresholds();
    CHECK(t.slo > t.shi && t.bhi == 225 && t.blo == 1);
    t = Rule::parse("R1,C0,M1,S9..9,B3..3").ltl_thresholds();  // with the centre: a full box
    CHECK(t.slo == 9 && t.shi == 9);
    // against the definition, every T and both centre states, for a handful of rules
    for (const char* s : {"R1,C0,M0,S2..3,B3..3", "R1,C0,M1,S3..4,B3..3", "R2,C0,M0,S0..25,B1..25", "R2,C0,M1,S0..0,B25..25",
                          "R3,C0,M0,S49..49,B49..49", "R7,C0,M0,S224..225,B225..225", "R7,C0,M1,S225..225,B1..1"}) {
        const Rule r = Rule::parse(s);
        const Rule::LtlThresholds th = r.ltl_thresholds();
        for (int alive = 0; alive < 2; ++alive)
            for (int T = alive; T <= r.box() - (1 - alive); ++T) {  // (T counts the centre)
                const int n = r.middle ? T : T - alive;
                const bool want = alive ? (n >= r.smin && n <= r.smax) : (n >= r.bmin && n <= r.bmax);
                const bool got = alive ? (T >= th.slo && T <= th.shi) : (T >= th.blo && T <= th.bhi);
                CHECK(want == got);
            }
        CHECK(th.blo <= r.box() && th.bhi <= r.box() && th.slo <= r.box() && th.shi <= r.box());
    }
}

// cpu::superstep against a per-cell count on a hand-made board: a gradient of density, so that low and high counts occur
static void test_superstep() {
    struct Case {
        const char* rule;
        i64 h, w;
    };
    const Case cases[] = {{"R1,C0,M0,S2..3,B3..3,NM", 20, 70},   {"R1,C0,M1,S3..4,B3..3,NM", 3, 3},
                          {"R2,C0,M1,S7..12,B7..9,NM", 5, 130},  {"bosco", 40, 67},
                          {"R5,C0,M0,S33..57,B34..45,NM", 11, 64}, {"R7,C0,M1,S63..108,B63..84,NM", 33, 65},
                          {"R7,C0,M0,S61..106,B63..84,NM", 15, 15}};
    std::mt19937_64 rng(7);
    for (const Case& c : cases)
        for (Boundary bd : {Boundary::Torus, Boundary::Dead}) {
            const Rule rule = Rule::parse(c.rule);
            const int R = rule.range;
            Decomposition dec = make_decomposition(c.h, 1, true, "1d", "", c.w);
            Geometry g = make_geometry(dec, 0);
            Layout L(c.h, c.w, R);
            std::vector<u64> a((size_t)L.words(), 0), b((size_t)L.words(), 0);
            std::vector<u8> cells((size_t)(c.h * c.w));
            for (i64 r = 0; r < c.h; ++r)
                for (i64 col = 0; col < c.w; ++col) {
                    const double p = (double)((r + col) % std::max(c.h, c.w)) / (double)(std::max(c.h, c.w) - 1);
                    const u8 v = std::uniform_real_distribution<double>(0, 1)(rng) < p;
                    cells[(size_t)(r * c.w + col)] = v;
                    if (v) a[(size_t)L.index(r, col >> 6)] |= 1ull << storage_bit(col);
                }
            const cpu::Edges edges(bd, g);
            u64* cur = a.data();
            u64* oth = b.data();
            for (int gen = 0; gen < 3; ++gen) {
                std::vector<u8> next(cells.size());
                for (i64 r = 0; r < c.h; ++r)
                    for (i64 col = 0; col < c.w; ++col) {
                        int n = 0;
                        for (i64 dy = -R; dy <= R; ++dy)
                            for (i64 dx = -R; dx <= R; ++dx) {
                                if (dy == 0 && dx == 0 && !rule.middle) continue;
                                i64 rr = r + dy, cc = col + dx;
                                if (bd == Boundary::Dead) {
                                    if (rr < 0 || rr >= c.h || cc < 0 || cc >= c.w) continue;
                                } else {
                                    rr = pmod(rr, c.h);
                                    cc = pmod(cc, c.w);
                                }
                                n += cells[(size_t)(rr * c.w + cc)];
                            }
                        const bool alive = cells[(size_t)(r * c.w + col)] != 0;
                        next[(size_t)(r * c.w + col)] = alive ? (n >= rule.smin && n <= rule.smax) : (n >= rule.bmin && n <= rule.bmax);
                    }
                u64* res = cpu::superstep(cur, oth, L, 1, rule, edges);
                if (res != cur) std::swap(cur, oth);
                cells = next;
                bool same = true;
                u64 pop = 0;
                for (i64 r = 0; r < c.h; ++r)
                    for (i64 col = 0; col < c.w; ++col) {
                        const u8 got = (u8)((cur[(size_t)L.index(r, col >> 6)] >> storage_bit(col)) & 1ull);
                        same = same && got == cells[(size_t)(r * c.w + col)];
                        pop += cells[(size_t)(r * c.w + col)];
                    }
                if (!same) fprintf(stderr, "superstep differs: %s %lldx%lld boundary %d gen %d\n", c.rule, (long long)c.h, (long long)c.w, (int)bd, gen);
                CHECK(same);
                CHECK(cpu::population(cur, L) == pop);
            }
        }
    // what the stepper refuses: a board smaller than the box, a record
    bool threw = false;
    try {
        Layout L(10, 64, 5);
        std::vector<u64> a((size_t)L.words(), 0), b((size_t)L.words(), 0);
        cpu::superstep(a.data(), b.data(), L, 1, Rule::parse("bosco"));
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
        Layout L(20, 64, 5);
        std::vector<u64> a((size_t)L.words(), 0), b((size_t)L.words(), 0);
        u64 counts[1] = {0};
        cpu::superstep(a.data(), b.data(), L, 1, Rule::parse("bosco"), cpu::Edges(), counts);
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
}

int main() {
    test_strings();
    test_thresholds();
    test_superstep();
    printf("gol_ltl_unit: %d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
