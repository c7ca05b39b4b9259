// gol-mi355x: host-side tests of soup batches (no GPU needed).  Run: build/gol_soup_unit
//
// Covers: the CPU backend of SoupBatch (soups.hpp) against a byte-per-cell torus written here that follows the same
// search (saved copy, window doubling, two-copy transient): random rules at S = 64 and S = 128, plain stepping bit for
// bit, the records of settle() with and without the transient, independence of the chunk and of how max_gens is
// reached, soups given as words, and the refusals.
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "gol/bits.hpp"
#include "gol/soups.hpp"

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

using Bytes = std::vector<u8>;

static Bytes byte_step(const Bytes& b, i64 S, const Rule& r) {
    Bytes o(b.size());
    for (i64 y = 0; y < S; ++y)
        for (i64 x = 0; x < S; ++x) {
            int n = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    if (dy || dx) n += b[(size_t)(pmod(y + dy, S) * S + pmod(x + dx, S))];
            const u8 c = b[(size_t)(y * S + x)];
            o[(size_t)(y * S + x)] = (u8)(((c ? r.survive : r.birth) >> n) & 1u);
        }
    return o;
}

static Bytes byte_soup(i64 S, u64 seed) {
    Bytes b((size_t)(S * S));
    const i64 M = S / 64;
    for (i64 y = 0; y < S; ++y)
        for (i64 x = 0; x < S; ++x) b[(size_t)(y * S + x)] = (u8)((random_word(seed, y, x / 64, M) >> (x % 64)) & 1u);
    return b;
}

struct Naive {
    u32 period = 0, generation = 0, population = 0;
    i64 transient = -1;
    Bytes board;
};

static Naive naive_settle(const Bytes& init, i64 S, const Rule& r, u64 max_gens, bool transient) {
    Naive out;
    Bytes b = init, saved = init;
    u64 g = 0, s = 0, w = 1;
    while (g < max_gens) {
        b = byte_step(b, S, r);
        ++g;
        if (b == saved) {
            out.period = (u32)(g - s);
            break;
        }
        if (g - s == w) {
            saved = b;
            s = g;
            w *= 2;
        }
    }
    out.generation = (u32)g;
    for (u8 c : b) out.population += c;
    out.board = b;
    if (transient && out.period) {
        Bytes x = init, y = init;
        for (u32 k = 0; k < out.period; ++k) y = byte_step(y, S, r);
        i64 t = 0;
        while (x != y) {
            x = byte_step(x, S, r);
            y = byte_step(y, S, r);
            ++t;
        }
        out.transient = t;
    }
    return out;
}

static std::unique_ptr<SoupBatch> batch(i64 n, i64 S, const Rule& r) {
    SoupConfig c;
    c.n = n;
    c.size = S;
    c.rule = r;
    c.backend = "cpu";
    return SoupBatch::create(c);
}

static Bytes one_board(SoupBatch& sb, i64 i) { return sb.boards({i}); }

static bool same_records(const std::vector<SoupRecord>& a, const std::vector<SoupRecord>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].period != b[i].period || a[i].transient != b[i].transient || a[i].generation != b[i].generation ||
            a[i].population != b[i].population)
            return false;
    return true;
}

template <typename F>
static bool throws_with(F f, const char* what) {
    try {
        f();
    } catch (const Error& e) {
        return std::string(e.what()).find(what) != std::string::npos;
    }
    return false;
}

int main() {
    std::mt19937_64 rng(20240611);
    // ---- plain stepping and settling under random rules ----
    for (i64 S : {64, 128}) {
        const int rules = S == 64 ? 6 : 3;
        for (int t = 0; t < rules; ++t) {
            Rule r;
            if (t > 0) r = Rule::from_masks((unsigned)(rng() & 0x1FEu), (unsigned)(rng() & 0x1FFu));
            const i64 n = 3;
            const u64 seed = 500 + 10 * (u64)t;
            auto sb = batch(n, S, r);
            sb->init_seed(seed);
            std::vector<Bytes> ref;
            for (i64 i = 0; i < n; ++i) {
                ref.push_back(byte_soup(S, seed + (u64)i));
                CHECK(one_board(*sb, i) == ref.back());
            }
            u32 pop0 = 0;
            for (u8 c : ref[0]) pop0 += c;
            CHECK(sb->records()[0].population == pop0 && sb->records()[0].generation == 0);
            for (int g : {1, 2, 5}) {
                sb->step((u64)g);
                for (i64 i = 0; i < n; ++i) {
                    for (int k = 0; k < g; ++k) ref[(size_t)i] = byte_step(ref[(size_t)i], S, r);
                    CHECK(one_board(*sb, i) == ref[(size_t)i]);
                }
            }
            CHECK(sb->records()[1].generation == 8);
            // a fresh batch for the search: its origin is generation 0
            const u64 max_gens = S == 64 ? 150 : 60;
            auto sa = batch(n, S, r);
            sa->init_seed(seed);
            sa->settle(max_gens, true, 16);
            auto sc = batch(n, S, r);
            sc->init_seed(seed);
            sc->settle(max_gens / 3, false, 1);
            sc->settle(max_gens, true, 7);
            const auto ra = sa->records();
            CHECK(same_records(ra, sc->records()));
            for (i64 i = 0; i < n; ++i) {
                const Naive nv = naive_settle(byte_soup(S, seed + (u64)i), S, r, max_gens, true);
                CHECK(ra[(size_t)i].period == nv.period);
                CHECK(ra[(size_t)i].generation == nv.generation);
                CHECK(ra[(size_t)i].population == nv.population);
                CHECK(ra[(size_t)i].transient == nv.transient);
                CHECK(one_board(*sa, i) == nv.board);
                CHECK(one_board(*sc, i) == nv.board);
            }
        }
    }
    // ---- B3/S23 long enough to settle: a glider from words, and random soups ----
    {
        const i64 S = 64;
        std::vector<u64> words((size_t)(2 * S), 0);  // soup 0: a glider; soup 1: empty
        words[1] = 1ull << 2;
        words[2] = 1ull << 3;
        words[3] = (1ull << 1) | (1ull << 2) | (1ull << 3);
        auto sb = batch(2, S, Rule());
        sb->init_words(words.data());
        sb->settle(2000, true, 100);
        const auto r = sb->records();
        CHECK(r[0].period == 256 && r[0].generation == 511 && r[0].transient == 0 && r[0].population == 5);
        CHECK(r[1].period == 1 && r[1].generation == 1 && r[1].transient == 0 && r[1].population == 0);
        CHECK(sb->stats().settled == 2 && sb->stats().kernel == "soups@64");
        CHECK(throws_with([&] { sb->step(1); }, "after settle()"));
        CHECK(throws_with([&] { sb->settle(100); }, "max_gens = 100"));
        CHECK(throws_with([&] { sb->settle(3000, false, 0); }, "chunk = 0"));
        CHECK(throws_with([&] { sb->boards({2}); }, "index 2"));
    }
    // ---- refusals ----
    {
        SoupConfig c;
        c.backend = "cpu";
        c.size = 96;
        CHECK(throws_with([&] { SoupBatch::create(c); }, "size 96"));
        c.size = 64;
        c.n = 0;
        CHECK(throws_with([&] { SoupBatch::create(c); }, "n = 0"));
        c.n = ((i64)1 << 20) + 1;
        CHECK(throws_with([&] { SoupBatch::create(c); }, "n = 1048577"));
        c.n = 1;
        c.rule = Rule::parse("B2/S34H");
        CHECK(throws_with([&] { SoupBatch::create(c); }, "B2/S34H"));
        c.rule = Rule::parse("B13/S13V");
        CHECK(throws_with([&] { SoupBatch::create(c); }, "B13/S13V"));
        c.rule = Rule();
        c.boundary = "dead";
        CHECK(throws_with([&] { SoupBatch::create(c); }, "dead"));
        c.boundary = "torus";
        c.compat = true;
        CHECK(throws_with([&] { SoupBatch::create(c); }, "compat"));
        c.compat = false;
        c.backend = "cuda";
        CHECK(throws_with([&] { SoupBatch::create(c); }, "cuda"));
        CHECK(batch(1, 256, Rule::parse("B36/S23"))->stats().kernel == "soups@256:rule");
    }
    printf("soup tests: %d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
