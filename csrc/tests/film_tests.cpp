// gol-mi355x: host-side tests of film mode (no GPU needed).  Run: build/gol_film_unit
//
// Covers: cpu::superstep with a FilmOut against a byte-per-cell loop written here.  The packed frames of the tiles
// of a rank grid, added up as Engine::film() adds them, must unpack to the window of the global board after every
// generation, whatever the ghost rows and words hold: 3 x 3 rank grids, unaligned widths, every depth k up to the
// halo depth R, random rules, both boundaries (on a bounded board the ghost cells beyond the board are noise),
// windows that cross the seams and the rank boundaries, lie inside one rank, or are single cells; and FilmGeo's
// word count against a count made here.
#include <cstring>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "gol/bits.hpp"
#include "gol/cpu.hpp"
#include "gol/film.hpp"
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

static std::vector<u8> byte_window(const std::vector<u8>& b, i64 H, i64 W, const FilmRect& f) {
    std::vector<u8> o((size_t)(f.rows * f.cols));
    for (i64 i = 0; i < f.rows; ++i)
        for (i64 j = 0; j < f.cols; ++j) o[(size_t)(i * f.cols + j)] = b[(size_t)(pmod(f.r0 + i, H) * W + pmod(f.c0 + j, W))];
    return o;
}

static Rule random_rule(std::mt19937& rng) {
    return Rule::from_masks((rng() & 0x1FEu), (rng() & 0x1FFu));  // (B0 is refused)
}

// One tile of a decomposed board, its ghost area from the global board as the torus machinery delivers it; on a
// bounded board noise wherever a ghost cell (or a tail bit) lies beyond the board.  The tile's words of the k frames
// are added into `sum` (k * slot words), as the ranks' frames are added.
static void film_tile(const Geometry& g, const std::vector<u8>& board, const Rule& rule, int k, int R, bool dead,
                      const FilmGeo& geo, std::vector<u64>& sum, std::mt19937& rng) {
    const i64 H = g.dec.H, W = g.dec.W;
    const Layout L(g.h, g.w, R);
    std::vector<u64> a((size_t)L.words()), b((size_t)L.words());
    for (auto& v : a) v = ((u64)rng() << 32) | rng();
    for (auto& v : b) v = ((u64)rng() << 32) | rng();
    for (i64 r = -R; r < L.h + R; ++r)
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
    std::vector<u64> mine((size_t)(k * geo.slot_words()), 0);
    cpu::superstep(a.data(), b.data(), L, k, rule, cpu::Edges(dead ? Boundary::Dead : Boundary::Torus, g), nullptr, nullptr,
                   cpu::FilmOut{&geo, mine.data()});
    for (size_t i = 0; i < mine.size(); ++i) {
        CHECK((sum[i] & mine[i]) == 0);  // (every word has one owner)
        sum[i] += mine[i];
    }
}

// A rank grid cut by hand (rows anywhere, columns at multiples of 64; on the torus the board's width is a multiple
// of 64 too, as the engine's 2-D grids require).
static void test_grid(i64 H, i64 W, const std::vector<i64>& row_starts, const std::vector<i64>& col_starts, int R, bool dead,
                      const std::vector<FilmRect>& windows, unsigned seed) {
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
    CHECK(row_starts.back() == H && col_starts.back() == W && (dead || W % 64 == 0 || Px == 1));
    for (int trial = 0; trial < 3; ++trial) {
        const Rule rule = trial == 0 ? Rule() : (trial == 1 ? Rule::parse("B36/S23") : random_rule(rng));
        std::vector<u8> board((size_t)(H * W));
        for (auto& v : board) v = (u8)(rng() & 1);
        std::vector<std::vector<u8>> series;
        for (int gen = 0; gen < R; ++gen) series.push_back(byte_step(gen ? series.back() : board, H, W, rule, dead));
        for (const FilmRect& f : windows) {
            const FilmGeo geo(f, H, W);
            for (int k = 1; k <= R; ++k) {
                std::vector<u64> sum((size_t)(k * geo.slot_words()), 0);
                for (const Geometry& g : tiles) film_tile(g, board, rule, k, R, dead, geo, sum, rng);
                std::vector<u8> got((size_t)(f.rows * f.cols));
                for (int j = 0; j < k; ++j) {
                    geo.unpack(&sum[(size_t)(j * geo.slot_words())], got.data());
                    const bool same = got == byte_window(series[(size_t)j], H, W, f);
                    if (!same)
                        fprintf(stderr, "frame mismatch: rule %s, %s, %lld x %lld board, window %lld x %lld at (%lld, %lld), k = %d, generation %d\n",
                                rule.str().c_str(), dead ? "dead" : "torus", (long long)H, (long long)W, (long long)f.rows,
                                (long long)f.cols, (long long)f.r0, (long long)f.c0, k, j + 1);
                    CHECK(same);
                }
            }
        }
    }
}

// FilmGeo's words against the set of words the window's columns touch, and every column found where unpack looks.
static void test_geo() {
    for (i64 W : {1, 3, 63, 64, 65, 130, 200, 256})
        for (i64 c0 = -W - 3; c0 <= 2 * W; c0 += (W > 70 ? 7 : 1))
            for (i64 cols : {(i64)1, (i64)5, W / 2 + 1, W - 1, W}) {
                if (cols < 1) continue;
                const FilmGeo geo(FilmRect{true, -2, c0, 3, cols}, 5, W);
                std::set<i64> words;
                for (i64 j = 0; j < cols; ++j) words.insert(pmod(c0 + j, W) / 64);
                CHECK(geo.fw >= (i64)words.size() && geo.fw <= geo.gwords);
                CHECK(geo.fw == (i64)words.size() || geo.fw == geo.gwords);
                for (i64 w : words) CHECK(geo.frame_word(w) < geo.fw);
                CHECK(geo.r0 == 3 && geo.frame_row(3) == 0 && geo.frame_row(0) == 2 && geo.frame_row(1) >= 3);
            }
}

int main() {
    test_geo();
    for (int dead = 0; dead < 2; ++dead) {
        const bool d = dead != 0;
        // 3 x 3 ranks, uneven rows.  Windows: over all nine ranks and both seams (torus), inside one rank, one cell,
        // one full row, one full column, where four tiles meet
        std::vector<FilmRect> w1 = {{true, 8, 60, 3, 10}, {true, 10, 70, 5, 20}, {true, 3, 5, 1, 1}, {true, 12, 0, 1, 192},
                                    {true, 0, 100, 30, 1}, {true, 0, 0, 30, 192}};
        if (!d) {
            w1.push_back({true, 25, 180, 12, 30});
            w1.push_back({true, -40, -500, 30, 192});
        }
        test_grid(30, 192, {0, 9, 20, 30}, {0, 64, 128, 192}, 4, d, w1, 11u + (unsigned)dead);
        std::vector<FilmRect> w2 = {{true, 7, 60, 9, 140}, {true, 0, 0, 23, 256}};
        if (!d) w2.push_back({true, 20, 250, 8, 70});
        test_grid(23, 256, {0, 8, 15, 23}, {0, 64, 192, 256}, 3, d, w2, 21u + (unsigned)dead);
        // strips of unaligned width (one column of ranks); on the torus the x seam runs through the masked tail word
        for (i64 W : {1, 3, 63, 65, 130, 200}) {
            std::vector<FilmRect> ws = {{true, 0, 0, 24, W}, {true, 5, W / 2, 10, (W + 1) / 2}};
            if (!d) ws.push_back({true, 20, W - 1, 9, W});
            test_grid(24, W, {0, 8, 16, 24}, {0, W}, 5, d, ws, 31u + (unsigned)dead + (unsigned)W);
        }
    }
    // bounded, unaligned: 22 cells in the last tiles
    test_grid(31, 150, {0, 10, 20, 31}, {0, 64, 128, 150}, 4, true, {{true, 0, 0, 31, 150}, {true, 9, 120, 12, 30}}, 51u);
    test_grid(12, 70, {0, 4, 8, 12}, {0, 64, 70}, 4, true, {{true, 0, 0, 12, 70}, {true, 3, 60, 6, 10}}, 52u);
    printf("film unit tests: %d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
