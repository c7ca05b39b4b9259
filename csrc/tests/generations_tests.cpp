// gol-mi355x: host-side tests of Generations rules (no GPU needed).  Run: build/gol_generations_unit
//
// Covers: the rule strings (accepted forms and their canonical strings, the code() / from_code round trip, C2 as the
// plain rule, every rejection) and the CPU stepper's planes, cpu::superstep and cpu::state_counts under a Generations
// rule on both boundaries, against a byte-per-cell loop of states written here.
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
    const Rule sw = Rule::parse("B2/S345/C4");
    CHECK(sw.states == 4 && sw.birth == (1u << 2) && sw.survive == ((1u << 3) | (1u << 4) | (1u << 5)) && sw.nbhd == Nbhd::Moore);
    CHECK(sw.generations() && sw.decay_planes() == 2 && !sw.is_conway());
    CHECK(sw.str() == "B2/S345/C4");
    for (const char* s : {"b2/s345/c4", "S345/B2/C4", "s543/b2/C4", "345/2/4", "B2/S345/c4"}) CHECK(Rule::parse(s) == sw);
    CHECK(Rule::parse("B2/S/C3").str() == "B2/S/C3" && Rule::parse("/2/3") == Rule::parse("B2/S/C3"));
    CHECK(Rule::parse("B34/S12/C3").str() == "B34/S12/C3" && Rule::parse("12/34/3").str() == "B34/S12/C3");
    CHECK(Rule::parse("B2/S345/C9").states == 9 && Rule::parse("B2/S345/C9").decay_planes() == 3);
    const int planes[10] = {0, 0, 0, 1, 2, 2, 3, 3, 3, 3};
    for (unsigned c = 2; c <= 9; ++c) {
        const Rule r = Rule::from_masks(1u << 2, 1u << 3, Nbhd::Moore, c);
        CHECK(r.states == c && r.decay_planes() == planes[c] && r.generations() == (c > 2));
        CHECK(Rule::from_code(r.code()) == r);
        CHECK(Rule::parse(r.str()) == r);
        CHECK((r.code() & 0x0FFFFFFFu) == Rule::from_masks(1u << 2, 1u << 3).code());  // the two-state code's bits are free
    }
    // C2 is the two-state rule: the same rule, the same string, the same code
    CHECK(Rule::parse("B3/S23/C2") == Rule() && Rule::parse("B3/S23/C2").is_conway() && Rule::parse("B3/S23/C2").str() == "B3/S23");
    CHECK(Rule::parse("23/3/2") == Rule());
    CHECK(Rule::parse("B36/S23/C2").code() == Rule::parse("B36/S23").code());
    // every accepted two-state string keeps its masks, str() and code()
    CHECK(Rule::parse("B36/S23").states == 2 && Rule::parse("B36/S23").code() == ((1u << 3) | (1u << 6) | (((1u << 2) | (1u << 3)) << 16)));
    CHECK(Rule::parse("B2/S34H").states == 2 && Rule::parse("B2/S34H").str() == "B2/S34H");
    CHECK(Rule::from_code(Rule::parse("B13/S13V").code()) == Rule::parse("B13/S13V"));
    // rejections: the state count out of range, leading zeros, an empty count, a suffix with /C, B0, and what was
    // refused before and is not of the new form
    for (const char* s : {"B2/S345/C0", "B2/S345/C1", "B2/S345/C10", "B2/S345/C11", "B2/S345/C99", "B2/S345/C04", "B2/S345/C00",
                          "B2/S345/C", "B2/S345/C4V", "B2/S345/C4H", "B2/S34V/C4", "B2/S34H/C3", "B0/S/C3", "B02/S345/C4", "/0/3",
                          "345/2/", "345/2/0", "345/2/1", "345/2/10", "345/2/04", "345/2/4/", "345/2/c4", "B2/S345/4", "B2/S345/C4 ",
                          "B2/S345/C4x", "B2/S345//C4", "B2/S345/C-3", "B3/S23/", "B3/B3", "3/23", "B3/S23/C", "B9/S/C3", "349/2/4",
                          "B22/S/C3", "33/2/4", "B2/S345/D4", "B2/C4", "C4"})
        check_rejected(s);
    for (unsigned c : {0u, 1u, 10u, 64u}) {
        bool threw = false;
        try {
            Rule::from_masks(1u << 2, 0, Nbhd::Moore, c);
        } catch (const Error&) {
            threw = true;
        }
        CHECK(threw);
    }
    bool threw = false;
    try {
        Rule::from_masks(1u << 2, 0, Nbhd::VonNeumann, 3);
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
        Rule::from_code(0x80000000u | Rule().code());
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
}

// ---------- byte-per-cell oracle of the states ----------
static std::vector<u8> byte_step(const std::vector<u8>& b, i64 H, i64 W, const Rule& r, bool torus) {
    std::vector<u8> o(b.size());
    for (i64 y = 0; y < H; ++y)
        for (i64 x = 0; x < W; ++x) {
            int n = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!dy && !dx) continue;
                    i64 yy = y + dy, xx = x + dx;
                    if (torus)
                        yy = pmod(yy, H), xx = pmod(xx, W);
                    else if (yy < 0 || yy >= H || xx < 0 || xx >= W)
                        continue;
                    n += b[(size_t)(yy * W + xx)] == 1;
                }
            const u8 c = b[(size_t)(y * W + x)];
            u8 v;
            if (c == 0)
                v = (u8)((r.birth >> n) & 1u);
            else if (c == 1)
                v = (u8)(((r.survive >> n) & 1u) ? 1 : 2);
            else
                v = (u8)(c + 1 < r.states ? c + 1 : 0);
            o[(size_t)(y * W + x)] = v;
        }
    return o;
}

// the planes of a state board, dense natural-order words
static std::vector<std::vector<u64>> planes_of(const std::vector<u8>& b, i64 H, i64 W, int M) {
    const i64 nw = ceil_div(W, 64);
    std::vector<std::vector<u64>> p((size_t)(M + 1), std::vector<u64>((size_t)(H * nw), 0));
    for (i64 y = 0; y < H; ++y)
        for (i64 x = 0; x < W; ++x) {
            const unsigned s = b[(size_t)(y * W + x)];
            const size_t at = (size_t)(y * nw + x / 64);
            if (s == 1) p[0][at] |= 1ull << (x % 64);
            for (int m = 0; s >= 2 && m < M; ++m)
                if (((s - 1) >> m) & 1u) p[(size_t)(m + 1)][at] |= 1ull << (x % 64);
        }
    return p;
}

static void check_superstep(const Rule& rule, i64 H, i64 W, int k, bool torus, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<u8> ref((size_t)(H * W));
    for (auto& v : ref) v = (u8)(rng() % rule.states);  // every state, dying ones included
    const int M = rule.decay_planes();
    const Layout L(H, W, k);
    const i64 stride = L.words() + 7;  // (a stride of its own: the planes need not be packed)
    std::vector<u64> a((size_t)((M + 1) * stride), 0), c((size_t)((M + 1) * stride), 0);
    const auto pw = planes_of(ref, H, W, M);
    for (int m = 0; m <= M; ++m) cpu::insert_words(a.data() + m * stride, L, pw[(size_t)m].data());
    Geometry g = make_geometry(make_decomposition(H, 1, true, "1d", "", W), 0);
    const cpu::Edges edges(torus ? Boundary::Torus : Boundary::Dead, g);
    u64* cur = a.data();
    u64* oth = c.data();
    for (int ss = 0; ss < 2; ++ss) {  // two supersteps of k generations
        for (int m = 0; m <= M; ++m) {
            cpu::fill_ghost_cols_wrap(cur + m * stride, L, 0, H);
            cpu::fill_ghost_rows_wrap(cur + m * stride, L);
        }
        u64* res = cpu::superstep(cur, oth, L, k, rule, edges, nullptr, nullptr, cpu::FilmOut(), cpu::DensityOut(), nullptr, stride);
        if (res != cur) std::swap(cur, oth);
        for (int gen = 0; gen < k; ++gen) ref = byte_step(ref, H, W, rule, torus);
    }
    const auto want = planes_of(ref, H, W, M);
    bool same = true;
    for (int m = 0; m <= M; ++m) {
        std::vector<u64> out((size_t)(H * L.nw));
        cpu::extract_words(cur + m * stride, L, out.data());
        same = same && out == want[(size_t)m];
    }
    std::vector<u64> counts(rule.states, 0), refc(rule.states, 0);
    cpu::state_counts(cur, L, stride, rule, counts.data());
    for (u8 v : ref) refc[v] += 1;
    same = same && counts == refc;
    if (!same)
        fprintf(stderr, "mismatch: rule %s, %lldx%lld, k = %d, %s\n", rule.str().c_str(), (long long)H, (long long)W, k,
                torus ? "torus" : "dead");
    CHECK(same);
}

static void test_superstep() {
    unsigned seed = 1;
    for (const char* s : {"B2/S/C3", "B2/S345/C4", "B34/S12/C5", "B2/S345/C6", "B3/S23/C8", "B2/S345/C9"})
        for (int k : {1, 3, 8})
            for (bool torus : {true, false}) {
                check_superstep(Rule::parse(s), 65, 137, k, torus, seed++);
                check_superstep(Rule::parse(s), 3, 100, k, torus, seed++);
            }
    // a recording under a Generations rule and a plane stride below a board are refused
    const Rule r = Rule::parse("B2/S/C3");
    const Layout L(8, 64, 1);
    std::vector<u64> a((size_t)(2 * L.words()), 0), b((size_t)(2 * L.words()), 0);
    u64 count = 0;
    bool threw = false;
    try {
        cpu::superstep(a.data(), b.data(), L, 1, r, cpu::Edges(), &count, nullptr, cpu::FilmOut(), cpu::DensityOut(), nullptr, L.words());
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
    threw = false;
    try {
        cpu::superstep(a.data(), b.data(), L, 1, r, cpu::Edges(), nullptr, nullptr, cpu::FilmOut(), cpu::DensityOut(), nullptr, L.words() - 1);
    } catch (const Error&) {
        threw = true;
    }
    CHECK(threw);
}

int main() {
    test_strings();
    test_superstep();
    printf("gol_generations_unit: %d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
