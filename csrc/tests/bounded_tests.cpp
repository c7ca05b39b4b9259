// gol-mi355x: host-side tests of bounded boards (Boundary::Dead; no GPU needed).  Run: build/gol_bounded_unit
//
// Covers: cpu::superstep on a bounded board against a byte-per-cell loop written here (random rules, tiles at
// every position of a 3 x 3 rank grid, unaligned widths, every depth k up to R, ghost cells beyond the board
// filled with noise), the one-rank case through the torus ghost fills, and the RLE topology suffix parser.
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

// ---------- byte-per-cell oracles: dead edges, and the torus (the results must differ) ----------
static std::vector<u8> byte_step(const std::vector<u8>& b, i64 H, i64 W, const Rule& r, bool dead) {
    std::vector<u8> o(b.size());
    for (i64 y = 0; y < H; ++y)
        for (i64 x = 0; x < W; ++x) {
            int n = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!dy && !dx) continue;
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

static Rule random_rule(std::mt19937& rng) {
    return Rule::from_masks((rng() & 0x1FEu), (rng() & 0x1FFu));  // (B0 is refused)
}

// One tile of a decomposed bounded board: its cells and its ghost area from the global board as the torus
// machinery would deliver them, with noise wherever a ghost cell (or a tail bit) lies beyond the board.
static void check_tile(const Geometry& g, const std::vector<u8>& board, const std::vector<u8>& want, const Rule& rule, int k,
                       int R, std::mt19937& rng) {
    const i64 H = g.dec.H, W = g.dec.W;
    const Layout L(g.h, g.w, R);
    std::vector<u64> a((size_t)L.words()), b((size_t)L.words());
    for (auto& v : a) v = ((u64)rng() << 32) | rng();  // noise everywhere first, the unused ghost rows included
    for (auto& v : b) v = ((u64)rng() << 32) | rng();
    for (i64 r = -R; r < L.h + R; ++r)
        for (i64 c = -1; c <= L.nw; ++c) {
            u64 nat = ((u64)rng() << 32) | rng();
            const i64 gr = g.row0 + r;
            for (int bit = 0; bit < 64; ++bit) {
                const i64 gc = 64 * (g.word0() + c) + bit;
                // inside the board: the cell; beyond it: what a torus exchange might have delivered, or noise
                if (gr >= 0 && gr < H && gc >= 0 && gc < W) {
                    nat &= ~(1ull << bit);
                    nat |= (u64)board[(size_t)(gr * W + gc)] << bit;
                } else if (rng() & 1) {
                    nat &= ~(1ull << bit);
                    nat |= (u64)board[(size_t)(pmod(gr, H) * W + pmod(gc, W))] << bit;
                }
            }
            a[(size_t)L.index(r, c)] = split_word(nat);
        }
    u64* res = cpu::superstep(a.data(), b.data(), L, k, rule, cpu::Edges(Boundary::Dead, g));
    std::vector<u64> out((size_t)(L.h * L.nw));
    cpu::extract_words(res, L, out.data());
    bool same = true;
    for (i64 r = 0; r < L.h && same; ++r)
        for (i64 c = 0; c < L.w; ++c) {
            const u8 got = (u8)((out[(size_t)(r * L.nw + (c >> 6))] >> (c & 63)) & 1ull);
            if (got != want[(size_t)((g.row0 + r) * W + g.col0 + c)]) {
                fprintf(stderr, "mismatch: rule %s, rank %d (tile %lldx%lld at %lld,%lld), k = %d, R = %d, cell (%lld, %lld)\n",
                        rule.str().c_str(), g.rank, (long long)g.h, (long long)g.w, (long long)g.row0, (long long)g.col0, k, R,
                        (long long)r, (long long)c);
                same = false;
                break;
            }
        }
    CHECK(same);
}

// A rank grid cut by hand (rows anywhere, columns at multiples of 64: the last column of tiles may end in a
// partial word, which make_decomposition's 2-D grids do not offer): the stepper needs only the tile's place.
static void test_grid(i64 H, i64 W, const std::vector<i64>& row_starts, const std::vector<i64>& col_starts, int R,
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
    CHECK(row_starts.back() == H && col_starts.back() == W);
    for (int trial = 0; trial < 3; ++trial) {
        const Rule rule = trial == 0 ? Rule() : (trial == 1 ? Rule::parse("B1/S012345678") : random_rule(rng));
        std::vector<u8> board((size_t)(H * W));
        for (auto& v : board) v = (u8)(rng() & 1);
        for (int k = 1; k <= R; ++k) {
            std::vector<u8> want = board, torus = board;
            for (int gen = 0; gen < k; ++gen) {
                want = byte_step(want, H, W, rule, true);
                torus = byte_step(torus, H, W, rule, false);
            }
            CHECK(want != torus);  // (running the torus would not pass)
            for (const Geometry& g : tiles) check_tile(g, board, want, rule, k, R, rng);
        }
    }
}

// One rank, its ghosts filled by the torus self-wrap as the engine does: several supersteps.
static void test_one_rank(i64 H, i64 W, int k, unsigned seed) {
    std::mt19937 rng(seed);
    const Decomposition dec = make_decomposition(H, 1, true, "1d", "", W);
    const Geometry g = make_geometry(dec, 0);
    for (int trial = 0; trial < 3; ++trial) {
        const Rule rule = trial == 0 ? Rule() : (trial == 1 ? Rule::parse("B1357/S1357") : random_rule(rng));
        std::vector<u8> ref((size_t)(H * W));
        for (auto& v : ref) v = 1;  // a full board: every edge cell differs between the two boundaries
        if (trial == 2)
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
        for (int ss = 0; ss < 3; ++ss) {
            cpu::fill_ghost_cols_wrap(cur, L, 0, H);
            cpu::fill_ghost_rows_wrap(cur, L);
            u64* res = cpu::superstep(cur, oth, L, k, rule, cpu::Edges(Boundary::Dead, g));
            if (res != cur) std::swap(cur, oth);
            for (int gen = 0; gen < k; ++gen) ref = byte_step(ref, H, W, rule, true);
        }
        std::vector<u64> out((size_t)(H * nw));
        cpu::extract_words(cur, L, out.data());
        bool same = true;
        for (i64 y = 0; y < H; ++y)
            for (i64 x = 0; x < W; ++x)
                same = same && (((out[(size_t)(y * nw + x / 64)] >> (x % 64)) & 1ull) == ref[(size_t)(y * W + x)]);
        if (!same) fprintf(stderr, "one rank mismatch: rule %s, %lldx%lld, k = %d\n", rule.str().c_str(), (long long)H, (long long)W, k);
        CHECK(same);
    }
}

// The default arguments are the torus: existing callers are unchanged.
static void test_default_is_torus() {
    std::mt19937 rng(7);
    const i64 H = 9, W = 70;
    const Layout L(H, W, 2);
    std::vector<u64> a((size_t)L.words(), 0), b1((size_t)L.words(), 0), b2((size_t)L.words(), 0);
    for (i64 r = 0; r < H; ++r)
        for (i64 c = 0; c < L.nw; ++c) a[(size_t)L.index(r, c)] = split_word((((u64)rng() << 32) | rng()) & L.mask(c));
    cpu::fill_ghost_cols_wrap(a.data(), L, 0, H);
    cpu::fill_ghost_rows_wrap(a.data(), L);
    std::vector<u64> a2 = a;
    u64* r1 = cpu::superstep(a.data(), b1.data(), L, 2);
    u64* r2 = cpu::superstep(a2.data(), b2.data(), L, 2, Rule(), cpu::Edges());
    std::vector<u64> o1((size_t)(H * L.nw)), o2((size_t)(H * L.nw));
    cpu::extract_words(r1, L, o1.data());
    cpu::extract_words(r2, L, o2.data());
    CHECK(o1 == o2);
    CHECK(!cpu::Edges().dead());
}

// ---------- the topology suffix ----------
static void check_suffix_rejected(const std::string& field) {
    bool threw = false, named = false;
    const std::string sfx = field.substr(field.find(':'));
    try {
        split_rule_topology(field);
    } catch (const Error& e) {
        threw = true;
        named = std::string(e.what()).find("'" + sfx + "'") != std::string::npos;
    }
    if (!threw) fprintf(stderr, "accepted: '%s'\n", field.c_str());
    CHECK(threw);
    CHECK(named);
}

static void test_suffix() {
    RleTopology t = split_rule_topology("B3/S23");
    CHECK(t.rule == "B3/S23" && t.topology.empty() && t.cols == 0 && t.rows == 0);
    t = split_rule_topology("B3/S23:P200,100");
    CHECK(t.rule == "B3/S23" && t.topology == "P" && t.cols == 200 && t.rows == 100);
    t = split_rule_topology("B36/S23:T30,20");
    CHECK(t.rule == "B36/S23" && t.topology == "T" && t.cols == 30 && t.rows == 20);
    t = split_rule_topology("23/3:p64");  // lower case, square shorthand
    CHECK(t.rule == "23/3" && t.topology == "P" && t.cols == 64 && t.rows == 64);
    t = split_rule_topology("B3/S23:t7");
    CHECK(t.topology == "T" && t.cols == 7 && t.rows == 7);
    for (const char* s : {"B3/S23:P0,100", "B3/S23:P100,0", "B3/S23:T0", "B3/S23:T30+5,20", "B3/S23:T30,20-2", "B3/S23:T30*,20",
                          "B3/S23:K30,20", "B3/S23:C30,20", "B3/S23:S30", "B3/S23:X30,20", "B3/S23:", "B3/S23:P", "B3/S23:P,5",
                          "B3/S23:P30,", "B3/S23:P30,20,10", "B3/S23:P30 ,20", "B3/S23:P30x20"})
        check_suffix_rejected(s);

    // through the reader and the writer
    RlePattern p = parse_rle("x = 3, y = 3, rule = B3/S23:P200,100\nbob$2bo$3o!\n");
    CHECK(p.rule == "B3/S23" && p.topology == "P" && p.bound_cols == 200 && p.bound_rows == 100);
    CHECK(p.rows == 3 && p.cols == 3 && p.cell(0, 1) && p.cell(2, 0) && !p.cell(0, 0));
    const std::string text = write_rle(p);
    CHECK(text.find("rule = B3/S23:P200,100\n") != std::string::npos);
    const RlePattern q = parse_rle(text);
    CHECK(q.topology == "P" && q.bound_cols == 200 && q.bound_rows == 100 && q.words == p.words && q.rule == p.rule);
    p = parse_rle("x = 1, y = 1, rule = 23/3:T16\no!");
    CHECK(p.rule == "B3/S23" && p.topology == "T" && p.bound_cols == 16 && p.bound_rows == 16);
    CHECK(write_rle(p).find("rule = B3/S23:T16,16\n") != std::string::npos);
    p = parse_rle("x = 1, y = 1, rule = B36/S23\no!");
    CHECK(p.topology.empty() && p.bound_cols == 0 && write_rle(p).find(':') == std::string::npos);
    bool threw = false;
    try {
        parse_rle("x = 1, y = 1, rule = B3/S23:K8,8\no!");
    } catch (const Error& e) {
        threw = std::string(e.what()).find("':K8,8'") != std::string::npos;
    }
    CHECK(threw);
}

static void test_boundary_names() {
    CHECK(parse_boundary("torus") == Boundary::Torus && parse_boundary("dead") == Boundary::Dead);
    CHECK(std::string(boundary_name(Boundary::Dead)) == "dead" && std::string(boundary_name(Boundary::Torus)) == "torus");
    bool named = false;
    try {
        parse_boundary("banana");
    } catch (const Error& e) {
        named = std::string(e.what()).find("'banana'") != std::string::npos;
    }
    CHECK(named);
}

int main() {
    test_boundary_names();
    test_default_is_torus();
    test_grid(30, 200, {0, 10, 20, 30}, {0, 64, 128, 200}, 8, 11);  // 3 x 3, the last word 8 cells wide
    test_grid(13, 129, {0, 5, 9, 13}, {0, 64, 128, 129}, 4, 12);    // 3 x 3, a last column of tiles one cell wide
    test_grid(12, 192, {0, 4, 8, 12}, {0, 64, 128, 192}, 4, 13);    // 3 x 3, aligned width
    test_grid(24, 330, {0, 8, 16, 24}, {0, 128, 256, 330}, 8, 15);  // 3 x 3, two-word tiles, k up to the 8-row tiles
    test_grid(21, 70, {0, 7, 14, 21}, {0, 70}, 7, 14);              // row strips
    for (int k : {1, 3, 8}) {
        test_one_rank(65, 137, k, 20 + (unsigned)k);
        test_one_rank(64, 128, k, 30 + (unsigned)k);
        test_one_rank(3, 3, k, 40 + (unsigned)k);
        test_one_rank(1, 1, k, 50 + (unsigned)k);
        test_one_rank(2, 65, k, 60 + (unsigned)k);
    }
    test_suffix();
    printf("gol_bounded_unit: %d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
