// gol-mi355x: host-side tests of the life-like rules (no GPU needed).  Run: build/gol_rule_unit
//
// Covers: rule strings (parse / canonical form round trips, aliases, every rejection) and the CPU stepper's
// generic bit-sliced path, cpu::superstep under a rule, against a byte-per-cell loop written here.
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

static const char* kRules[] = {"B36/S23", "B3678/S34678", "B2/S", "B1357/S1357", "B3/S012345678", "B35678/S5678"};

static unsigned mask_of(const char* digits) {
    unsigned m = 0;
    for (; *digits; ++digits) m |= 1u << (*digits - '0');
    return m;
}

// the string must be refused, with an error that names it
static void check_rejected(const std::string& s) {
    bool threw = false, named = false;
    try {
        Rule::parse(s);
    } catch (const Error& e) {
        threw = true;
        named = std::string(e.what()).find("'" + s + "'") != std::string::npos;
    }
    if (!threw) fprintf(stderr, "accepted: '%s'\n", s.c_str());
    CHECK(threw);
    CHECK(named);
}

static void test_strings() {
    for (const char* s : kRules) {
        const Rule r = Rule::parse(s);
        CHECK(r.str() == s);
        CHECK(Rule::parse(r.str()) == r);
        CHECK(!r.is_conway());
    }
    CHECK(Rule::parse("B36/S23").birth == mask_of("36") && Rule::parse("B36/S23").survive == mask_of("23"));
    CHECK(Rule::parse("B2/S").birth == mask_of("2") && Rule::parse("B2/S").survive == 0);
    CHECK(Rule::parse("B/S0").birth == 0 && Rule::parse("B/S0").survive == 1);
    CHECK(Rule().is_conway() && Rule().str() == "B3/S23");
    CHECK(Rule::parse("b3/s23").is_conway());
    CHECK(Rule::parse("s32/B3").is_conway());  // either order, any digit order
    CHECK(Rule::parse("S23/b3").str() == "B3/S23");
    CHECK(Rule::parse("B8765/S8").str() == "B5678/S8");
    CHECK(Rule::parse("conway").is_conway() && Rule::parse("Life").is_conway());
    CHECK(Rule::parse("highlife").str() == "B36/S23");
    CHECK(Rule::parse("DayNight").str() == "B3678/S34678");
    CHECK(Rule::parse("seeds").str() == "B2/S");
    CHECK(Rule::parse("replicator").str() == "B1357/S1357");
    CHECK(Rule::parse("B36/S23").code() == (mask_of("36") | (mask_of("23") << 16)));
    CHECK(Rule::from_masks(mask_of("36"), mask_of("23")) == Rule::parse("highlife"));
    // rejections: digits > 8, repeated digits, a missing part, trailing text, B0
    for (const char* s : {"B39/S23", "B3/S29", "B33/S23", "B3/S232", "B3", "S23", "B3/", "/S23", "B3S23", "B3/B2", "S2/S3",
                          "B3/S23 ", "B3/S23x", "B3/S23/", " B3/S23", "B3/S2 3", "", "lifelike", "3/23", "B0/S", "B03/S23",
                          "B012345678/S012345678", "s23/b0"})
        check_rejected(s);
    try {
        Rule::parse("B0/S");
    } catch (const Error& e) {
        CHECK(std::string(e.what()).find("out of scope") != std::string::npos);
    }
    bool threw = false;
    try {
        Rule::from_masks(1, 0);
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
        Rule::from_masks(2, 1u << 9);
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
}

// ---------- byte-per-cell oracle on a torus ----------
static std::vector<u8> byte_step(const std::vector<u8>& b, i64 H, i64 W, const Rule& r) {
    std::vector<u8> o(b.size());
    for (i64 y = 0; y < H; ++y)
        for (i64 x = 0; x < W; ++x) {
            int n = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    if (dy || dx) n += b[(size_t)(pmod(y + dy, H) * W + pmod(x + dx, W))];
            const u8 c = b[(size_t)(y * W + x)];
            o[(size_t)(y * W + x)] = (u8)(((c ? r.survive : r.birth) >> n) & 1u);
        }
    return o;
}

static std::vector<u64> pack(const std::vector<u8>& b, i64 H, i64 W) {
    const i64 nw = ceil_div(W, 64);
    std::vector<u64> w((size_t)(H * nw), 0);
    for (i64 y = 0; y < H; ++y)
        for (i64 x = 0; x < W; ++x)
            if (b[(size_t)(y * W + x)]) w[(size_t)(y * nw + x / 64)] |= 1ull << (x % 64);
    return w;
}

static void check_superstep(const Rule& rule, i64 H, i64 W, int k, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<u8> ref((size_t)(H * W));
    for (auto& v : ref) v = (u8)(rng() & 1);
    const Layout L(H, W, k);
    std::vector<u64> a((size_t)L.words(), 0), c((size_t)L.words(), 0);
    const std::vector<u64> pw = pack(ref, H, W);
    cpu::insert_words(a.data(), L, pw.data());
    u64* cur = a.data();
    u64* oth = c.data();
    for (int ss = 0; ss < 2; ++ss) {  // two supersteps of k generations
        cpu::fill_ghost_cols_wrap(cur, L, 0, H);
        cpu::fill_ghost_rows_wrap(cur, L);
        u64* res = cpu::superstep(cur, oth, L, k, rule);
        if (res != cur) std::swap(cur, oth);
        for (int g = 0; g < k; ++g) ref = byte_step(ref, H, W, rule);
    }
    std::vector<u64> out((size_t)(H * L.nw));
    cpu::extract_words(cur, L, out.data());
    const bool same = out == pack(ref, H, W);
    if (!same) fprintf(stderr, "mismatch: rule %s, %lldx%lld, k = %d\n", rule.str().c_str(), (long long)H, (long long)W, k);
    CHECK(same);
}

static void test_superstep() {
    unsigned seed = 1;
    for (const char* s : kRules)
        for (int k : {1, 3, 8}) {
            check_superstep(Rule::parse(s), 65, 137, k, seed++);
            check_superstep(Rule::parse(s), 3, 3, k, seed++);
        }
    // B3/S23 through both paths: the specialised gates (default) agree with the byte loop too
    for (int k : {1, 3, 8}) check_superstep(Rule(), 65, 137, k, seed++);
    // every single-bit rule: each (state, count) entry of the generic finish on its own
    for (int c = 1; c <= 8; ++c) check_superstep(Rule::from_masks(1u << c, 0), 33, 70, 1, seed++);
    for (int c = 0; c <= 8; ++c) check_superstep(Rule::from_masks(0, 1u << c), 33, 70, 1, seed++);
}

int main() {
    test_strings();
    test_superstep();
    printf("gol_rule_unit: %d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
