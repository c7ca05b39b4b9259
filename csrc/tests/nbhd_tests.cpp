// gol-mi355x: host-side tests of the von Neumann and hexagonal neighbourhoods (no GPU needed).  Run: build/gol_nbhd_unit
//
// Covers: rule strings with the V / H suffix (round trips, rejections, code()), and cpu::superstep under V and H rules
// against a byte-per-cell loop written here from the neighbourhoods' 3 x 3 masks: random rules, tiles at every position
// of a 3 x 3 rank grid, unaligned widths, every depth k up to R, both boundaries, noise in the ghost cells nothing
// may read (dead edges: beyond the board; torus: beyond depth k), one rank through the torus ghost fills, and the
// per-generation counts and signatures.
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "gol/bits.hpp"
#include "gol/cpu.hpp"
#include "gol/geometry.hpp"
#include "gol/rle.hpp"
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

// The neighbourhoods as literals (rows downward, columns rightward), by Nbhd's value.
static const int kMask[3][3][3] = {{{1, 1, 1}, {1, 0, 1}, {1, 1, 1}}, {{0, 1, 0}, {1, 0, 1}, {0, 1, 0}}, {{1, 1, 0}, {1, 0, 1}, {0, 1, 1}}};

static std::vector<u8> byte_step(const std::vector<u8>& b, i64 H, i64 W, const Rule& r, bool dead) {
    std::vector<u8> o(b.size());
    for (i64 y = 0; y < H; ++y)
        for (i64 x = 0; x < W; ++x) {
            int n = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!kMask[(int)r.nbhd][dy + 1][dx + 1]) continue;
                    const i64 yy = y + dy, xx = x + dx;
                    if (dead) {
                        if (yy >= 0 && yy < H && xx >= 0 && xx < W) n += b[(size_t)(yy * W + xx)];
                    } else {
                        n += b[(size_t)(pmod(yy, H) * W + pmod(xx, W))];
                    }
                }
            const u8 c = b[(size_t)(y * W + x)];
            o[(size_t)(y * W + x)] = (u8)(((c ? r.survive : r.birth) >> n) & 1u);
        }
    return o;
}

static Rule random_rule(std::mt19937& rng, Nbhd n) {
    const unsigned all = (2u << nbhd_max_count(n)) - 1u;
    return Rule::from_masks(rng() & all & ~1u, rng() & all, n);  // (B0 is refused)
}

// ---------- rule strings ----------
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
    for (const char* s : {"B2/S34H", "B13/S13V", "B1/SH", "B1/SV", "B/S0V", "B123456/S0123456H", "B1234/S01234V"}) {
        const Rule r = Rule::parse(s);
        CHECK(r.str() == s);
        CHECK(Rule::parse(r.str()) == r);
        CHECK(Rule::from_code(r.code()) == r);
        CHECK(!r.is_conway());
    }
    CHECK(Rule::parse("s43/b2h").str() == "B2/S34H");
    CHECK(Rule::parse("S31/B31v").str() == "B13/S13V");
    CHECK(Rule::parse("b2/s34h") == Rule::parse("B2/S34H"));
    CHECK(Rule::parse("B2/S34H").nbhd == Nbhd::Hex && Rule::parse("B13/S13V").nbhd == Nbhd::VonNeumann);
    CHECK(Rule::parse("B2/S34").nbhd == Nbhd::Moore && Rule().nbhd == Nbhd::Moore);
    CHECK(Rule::parse("B2/S34H") != Rule::parse("B2/S34") && Rule::parse("B2/S34H") != Rule::parse("B2/S34V"));
    CHECK(!Rule::parse("B3/S23V").is_conway() && !Rule::parse("B3/S23H").is_conway() && Rule::parse("B3/S23").is_conway());
    for (const char* s : {"B5/S2V", "B2/S5V", "B7/S2H", "B2/S7H", "B0/SV", "B0/SH", "B3/S23VH", "B3/S23 V", "B3V/S23", "B3/S23HV",
                          "B3/S23X", "V", "B3/VS23", "lifeH"})
        check_rejected(s);
    // the range is named
    bool ranged = false;
    try {
        Rule::parse("B5/S2V");
    } catch (const Error& e) {
        ranged = std::string(e.what()).find("von Neumann") != std::string::npos && std::string(e.what()).find("0 to 4") != std::string::npos;
    }
    CHECK(ranged);
    // a Moore rule's code is what it was before there were neighbourhoods
    CHECK(Rule().code() == 0x000C0008u);
    CHECK(Rule::parse("B36/S23").code() == 0x000C0048u);
    CHECK(Rule::from_code(0x000C0008u).is_conway());
    CHECK(Rule::parse("B3/S23V").code() != Rule().code() && Rule::parse("B3/S23H").code() != Rule::parse("B3/S23V").code());
    CHECK(Rule::from_masks(1u << 2, (1u << 3) | (1u << 4), Nbhd::Hex) == Rule::parse("B2/S34H"));
    CHECK(Rule::from_masks(1u << 3, 3u << 2) == Rule());
    for (int which = 0; which < 3; ++which) {
        bool threw = false;
        try {
            if (which == 0) Rule::from_masks(1u << 5, 0, Nbhd::VonNeumann);
            if (which == 1) Rule::from_masks(2, 1u << 7, Nbhd::Hex);
            if (which == 2) Rule::from_code(0x000C0008u | (3u << 12));
        } catch (const Error&) {
            threw = true;
        }
        CHECK(threw);
    }
    // the RLE header: the suffix before the topology, either form of the lists
    RlePattern p = parse_rle("x = 1, y = 1, rule = B2/S34H\no!");
    CHECK(p.rule == "B2/S34H" && p.topology.empty());
    p = parse_rle("x = 1, y = 1, rule = 34/2H\no!");
    CHECK(p.rule == "B2/S34H");
    p = parse_rle("x = 1, y = 1, rule = 13/13v\no!");
    CHECK(p.rule == "B13/S13V");
    p = parse_rle("x = 1, y = 1, rule = B2/S34H:T64,64\no!");
    CHECK(p.rule == "B2/S34H" && p.topology == "T" && p.bound_cols == 64 && p.bound_rows == 64);
    CHECK(write_rle(p).find("rule = B2/S34H:T64,64\n") != std::string::npos);
    CHECK(parse_rle(write_rle(p)).rule == "B2/S34H");
    p = parse_rle("x = 1, y = 1, rule = b13/s13v:P30,20\no!");
    CHECK(p.rule == "B13/S13V" && p.topology == "P" && p.bound_cols == 30 && p.bound_rows == 20);
    CHECK(write_rle(p).find("rule = B13/S13V:P30,20\n") != std::string::npos);
    bool threw = false;
    try {
        parse_rle("x = 1, y = 1, rule = B7/S2H\no!");
    } catch (const Error& e) {
        threw = std::string(e.what()).find("B7/S2H") != std::string::npos;
    }
    CHECK(threw);
}

// ---------- one live cell under B1/S: the neighbourhood's mask itself (both are point-symmetric) ----------
static void test_literal_masks() {
    for (Nbhd n : {Nbhd::VonNeumann, Nbhd::Hex}) {
        const Rule rule = Rule::from_masks(2, 0, n);
        const i64 N = 5;
        const Layout L(N, N, 1);
        std::vector<u64> a((size_t)L.words(), 0), b((size_t)L.words(), 0), pw((size_t)N, 0);
        pw[2] = 1ull << 2;
        cpu::insert_words(a.data(), L, pw.data());
        cpu::fill_ghost_cols_wrap(a.data(), L, 0, N);
        cpu::fill_ghost_rows_wrap(a.data(), L);
        u64* res = cpu::superstep(a.data(), b.data(), L, 1, rule);
        std::vector<u64> out((size_t)N);
        cpu::extract_words(res, L, out.data());
        for (i64 y = 0; y < N; ++y)
            for (i64 x = 0; x < N; ++x) {
                const bool in = y >= 1 && y <= 3 && x >= 1 && x <= 3;
                const int want = in ? kMask[(int)n][y - 1][x - 1] : 0;
                CHECK((int)((out[(size_t)y] >> x) & 1ull) == want);
            }
    }
}

// ---------- tiles of a rank grid ----------
// The tile's cells and ghost area from the global board.  Dead edges: noise (or torus cells) wherever a ghost cell or
// tail bit lies beyond the board.  Torus: the wrapped cells in the ghost area a depth-k superstep may read (k rows,
// one word), noise in the ghost rows beyond.
static void check_tile(const Geometry& g, const std::vector<u8>& board, const std::vector<std::vector<u8>>& want, const Rule& rule,
                       int k, int R, bool dead, std::mt19937& rng) {
    const i64 H = g.dec.H, W = g.dec.W;
    const Layout L(g.h, g.w, R);
    std::vector<u64> a((size_t)L.words()), b((size_t)L.words());
    for (auto& v : a) v = ((u64)rng() << 32) | rng();
    for (auto& v : b) v = ((u64)rng() << 32) | rng();
    for (i64 r = -(dead ? R : k); r < L.h + (dead ? R : k); ++r)
        for (i64 c = -1; c <= L.nw; ++c) {
            u64 nat = ((u64)rng() << 32) | rng();
            const i64 gr = g.row0 + r;
            for (int bit = 0; bit < 64; ++bit) {
                const i64 gc = 64 * (g.word0() + c) + bit;
                const bool inside = gr >= 0 && gr < H && gc >= 0 && gc < W;
                if (inside || !dead || (rng() & 1)) {
                    nat &= ~(1ull << bit);
                    nat |= (u64)board[(size_t)(pmod(gr, H) * W + pmod(gc, W))] << bit;
                }
            }
            a[(size_t)L.index(r, c)] = split_word(nat);
        }
    std::vector<u64> counts((size_t)k, 0), sigs((size_t)k, 0);
    u64* res = cpu::superstep(a.data(), b.data(), L, k, rule, dead ? cpu::Edges(Boundary::Dead, g) : cpu::Edges(), counts.data(),
                              sigs.data());
    std::vector<u64> out((size_t)(L.h * L.nw));
    cpu::extract_words(res, L, out.data());
    bool same = true;
    for (i64 r = 0; r < L.h && same; ++r)
        for (i64 c = 0; c < L.w; ++c) {
            const u8 got = (u8)((out[(size_t)(r * L.nw + (c >> 6))] >> (c & 63)) & 1ull);
            if (got != want[(size_t)k - 1][(size_t)((g.row0 + r) * W + g.col0 + c)]) {
                fprintf(stderr, "mismatch: rule %s, %s, rank %d (tile %lldx%lld at %lld,%lld), k = %d, R = %d, cell (%lld, %lld)\n",
                        rule.str().c_str(), dead ? "dead" : "torus", g.rank, (long long)g.h, (long long)g.w, (long long)g.row0,
                        (long long)g.col0, k, R, (long long)r, (long long)c);
                same = false;
                break;
            }
        }
    CHECK(same);
    // the tile's own cells of every generation, counted
    bool counted = true;
    for (int gen = 0; gen < k; ++gen) {
        u64 n = 0;
        for (i64 r = 0; r < L.h; ++r)
            for (i64 c = 0; c < L.w; ++c) n += want[(size_t)gen][(size_t)((g.row0 + r) * W + g.col0 + c)];
        counted = counted && counts[(size_t)gen] == n;
    }
    CHECK(counted);
}

static void test_grid(i64 H, i64 W, const std::vector<i64>& row_starts, const std::vector<i64>& col_starts, int R, bool dead,
                      unsigned seed) {
    std::mt19937 rng(seed);
    const int Py = (int)row_starts.size() - 1, Px = (int)col_starts.size() - 1, P = Px * Py;
    std::vector<Geometry> tiles;
    for (int cy = 0; cy < Py; ++cy)
        for (int cx = 0; cx < Px; ++cx) {
            Geometry g;
            g.dec.H = H;
            g.dec.W = W;
            g.dec.P = P;
            g.dec.Px = Px;
            g.dec.Py = Py;
            g.rank = cy * Px + cx;
            g.cx = cx;
            g.cy = cy;
            g.row0 = row_starts[(size_t)cy];
            g.col0 = col_starts[(size_t)cx];
            g.h = row_starts[(size_t)cy + 1] - g.row0;
            g.w = col_starts[(size_t)cx + 1] - g.col0;
            CHECK(g.col0 % 64 == 0 && g.h >= R && g.w >= 1);
            tiles.push_back(g);
        }
    CHECK(row_starts.back() == H && col_starts.back() == W && (dead || W % 64 == 0));
    for (Nbhd n : {Nbhd::VonNeumann, Nbhd::Hex})
        for (int trial = 0; trial < 3; ++trial) {
            const Rule rule = trial == 0 ? Rule::from_masks(2, 0, n) : random_rule(rng, n);
            std::vector<u8> board((size_t)(H * W));
            for (auto& v : board) v = (u8)(rng() & 1);
            std::vector<std::vector<u8>> want, moore;
            Rule as_moore = rule;
            as_moore.nbhd = Nbhd::Moore;
            for (int gen = 0; gen < R; ++gen) {
                want.push_back(byte_step(gen ? want.back() : board, H, W, rule, dead));
                moore.push_back(byte_step(gen ? moore.back() : board, H, W, as_moore, dead));
            }
            CHECK(want[0] != moore[0]);  // (ignoring the neighbourhood would not pass)
            for (int k = 1; k <= R; ++k)
                for (const Geometry& g : tiles) check_tile(g, board, want, rule, k, R, dead, rng);
        }
}

// One rank, its ghosts filled by the torus self-wrap as the engine does: several supersteps, unaligned widths.
static void test_one_rank(i64 H, i64 W, int k, bool dead, unsigned seed) {
    std::mt19937 rng(seed);
    const Decomposition dec = make_decomposition(H, 1, true, "1d", "", W);
    const Geometry g = make_geometry(dec, 0);
    for (Nbhd n : {Nbhd::VonNeumann, Nbhd::Hex})
        for (int trial = 0; trial < 3; ++trial) {
            const Rule rule = trial == 0 ? Rule::from_masks(2, 0, n) : random_rule(rng, n);
            std::vector<u8> ref((size_t)(H * W));
            for (auto& v : ref) v = (u8)(rng() & 1);
            const Layout L(H, W, k);
            std::vector<u64> a((size_t)L.words(), 0), c((size_t)L.words(), 0);
            const i64 nw = L.nw;
            std::vector<u64> pw((size_t)(H * nw), 0);
            for (i64 y = 0; y < H; ++y)
                for (i64 x = 0; x < W; ++x)
                    if (ref[(size_t)(y * W + x)]) pw[(size_t)(y * nw + x / 64)] |= 1ull << (x % 64);
            cpu::insert_words(a.data(), L, pw.data());
            u64* cur = a.data();
            u64* oth = c.data();
            bool sig_ok = true;
            for (int ss = 0; ss < 3; ++ss) {
                cpu::fill_ghost_cols_wrap(cur, L, 0, H);
                cpu::fill_ghost_rows_wrap(cur, L);
                std::vector<u64> sigs((size_t)k, 0);
                u64* res = cpu::superstep(cur, oth, L, k, rule, dead ? cpu::Edges(Boundary::Dead, g) : cpu::Edges(), nullptr, sigs.data());
                if (res != cur) std::swap(cur, oth);
                for (int gen = 0; gen < k; ++gen) ref = byte_step(ref, H, W, rule, dead);
                sig_ok = sig_ok && sigs[(size_t)k - 1] == cpu::signature(cur, L, 0, 0);
            }
            CHECK(sig_ok);
            std::vector<u64> out((size_t)(H * nw));
            cpu::extract_words(cur, L, out.data());
            bool same = true;
            for (i64 y = 0; y < H; ++y)
                for (i64 x = 0; x < W; ++x)
                    same = same && (((out[(size_t)(y * nw + x / 64)] >> (x % 64)) & 1ull) == ref[(size_t)(y * W + x)]);
            if (!same)
                fprintf(stderr, "one rank mismatch: rule %s, %s, %lldx%lld, k = %d\n", rule.str().c_str(), dead ? "dead" : "torus",
                        (long long)H, (long long)W, k);
            CHECK(same);
        }
}

int main() {
    test_strings();
    test_literal_masks();
    test_grid(30, 200, {0, 10, 20, 30}, {0, 64, 128, 200}, 8, true, 11);   // 3 x 3, the last word 8 cells wide
    test_grid(13, 129, {0, 5, 9, 13}, {0, 64, 128, 129}, 4, true, 12);     // 3 x 3, a last column of tiles one cell wide
    test_grid(24, 330, {0, 8, 16, 24}, {0, 128, 256, 330}, 8, true, 13);   // 3 x 3, two-word tiles
    test_grid(12, 192, {0, 4, 8, 12}, {0, 64, 128, 192}, 4, false, 14);    // 3 x 3 on the torus
    test_grid(24, 384, {0, 8, 16, 24}, {0, 128, 256, 384}, 8, false, 15);  // 3 x 3 on the torus, two-word tiles
    test_grid(21, 64, {0, 7, 14, 21}, {0, 64}, 7, false, 16);              // row strips on the torus
    test_grid(21, 70, {0, 7, 14, 21}, {0, 70}, 7, true, 17);               // row strips, dead edges
    for (bool dead : {false, true})
        for (int k : {1, 3, 8}) {
            test_one_rank(65, 137, k, dead, 20 + (unsigned)k);
            test_one_rank(64, 128, k, dead, 30 + (unsigned)k);
            test_one_rank(3, 3, k, dead, 40 + (unsigned)k);
            test_one_rank(1, 1, k, dead, 50 + (unsigned)k);
            test_one_rank(2, 65, k, dead, 60 + (unsigned)k);
            test_one_rank(7, 130, k, dead, 70 + (unsigned)k);
        }
    printf("gol_nbhd_unit: %d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
