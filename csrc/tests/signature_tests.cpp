// gol-mi355x: host-side tests of the board signature (no GPU needed).  Run: build/gol_signature_unit
//
// Covers: cpu::superstep with `sigs` and cpu::signature against a byte-per-cell loop written here, which applies
// the definition cell by cell: a live cell at global (r, x) adds  2^((x mod 64) / 2) * (rho(r) * gam(2 (x / 64) +
// (x mod 2)) mod 2^32)  mod 2^64.  sigs[g] must be that sum over the tile's own rectangle of the global board after
// generation g + 1, whatever the ghost rows and words hold: tiles at every position of a 3 x 3 rank grid, unaligned
// widths, every depth k up to the halo depth R, random rules, both boundaries (noise in the ghost cells beyond a
// bounded board; live neighbours' cells on the torus), and one rank through the torus ghost fills over several
// supersteps.  Also the seven published vectors, and that the tiles' shares add up to the board's signature.
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

// The definition, written out again (not shared with gol/signature.hpp).
static u32 mix32(u32 x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
static u64 cell_term(i64 r, i64 x) {
    const u32 rho = mix32((u32)r ^ 0x9E3779B9u) | 1u;
    const u32 gam = mix32((u32)(2 * (x / 64) + (x & 1)) + 0x7F4A7C15u) | 1u;
    return (u64)(u32)(rho * gam) << ((x % 64) / 2);
}
static u64 byte_signature(const std::vector<u8>& b, i64 W, i64 r0, i64 c0, i64 h, i64 w) {
    u64 s = 0;
    for (i64 y = r0; y < r0 + h; ++y)
        for (i64 x = c0; x < c0 + w; ++x)
            if (b[(size_t)(y * W + x)]) s += cell_term(y, x);
    return s;
}

static Rule random_rule(std::mt19937& rng) {
    return Rule::from_masks((rng() & 0x1FEu), (rng() & 0x1FFu));  // (B0 is refused)
}

static void check_tile(const Geometry& g, const std::vector<u8>& board, const std::vector<std::vector<u8>>& series,
                       const Rule& rule, int k, int R, bool dead, std::mt19937& rng) {
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
    // the board in memory first (its tail bits hold noise or the torus neighbour's cells: they are masked)
    CHECK(cpu::signature(a.data(), L, g.row0, g.word0()) == byte_signature(board, W, g.row0, g.col0, g.h, g.w));
    std::vector<u64> sigs((size_t)k, 0), counts((size_t)k, 0);
    sigs[0] = 0xFEDCBA9876543210ull;  // (the stepper adds, wrapping: what a slot held stays)
    u64* res = cpu::superstep(a.data(), b.data(), L, k, rule, cpu::Edges(dead ? Boundary::Dead : Boundary::Torus, g),
                              counts.data(), sigs.data());
    sigs[0] -= 0xFEDCBA9876543210ull;
    for (int j = 0; j < k; ++j) {
        const u64 want = byte_signature(series[(size_t)j], W, g.row0, g.col0, g.h, g.w);
        if (sigs[(size_t)j] != want)
            fprintf(stderr, "signature mismatch: rule %s, %s, rank %d (tile %lldx%lld at %lld,%lld), k = %d, generation %d: %016llx, want %016llx\n",
                    rule.str().c_str(), dead ? "dead" : "torus", g.rank, (long long)g.h, (long long)g.w, (long long)g.row0,
                    (long long)g.col0, k, j + 1, (unsigned long long)sigs[(size_t)j], (unsigned long long)want);
        CHECK(sigs[(size_t)j] == want);
    }
    CHECK(sigs[(size_t)k - 1] == cpu::signature(res, L, g.row0, g.word0()));
    CHECK(counts[(size_t)k - 1] == cpu::population(res, L));
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
    for (int trial = 0; trial < 3; ++trial) {
        const Rule rule = trial == 0 ? Rule() : (trial == 1 ? Rule::parse("B1/S012345678") : random_rule(rng));
        std::vector<u8> board((size_t)(H * W));
        for (auto& v : board) v = (u8)(rng() & 1);
        std::vector<std::vector<u8>> series;
        for (int gen = 0; gen < R; ++gen) series.push_back(byte_step(gen ? series.back() : board, H, W, rule, dead));
        for (int k = 1; k <= R; ++k) {
            u64 total = 0;
            for (const Geometry& g : tiles) {
                check_tile(g, board, series, rule, k, R, dead, rng);
                total += byte_signature(series[(size_t)k - 1], W, g.row0, g.col0, g.h, g.w);
            }
            CHECK(total == byte_signature(series[(size_t)k - 1], W, 0, 0, H, W));  // (the tiles partition the board)
        }
    }
}

// One rank, its ghosts filled by the torus self-wrap as the engine does: several supersteps, one running series.
static void test_one_rank(i64 H, i64 W, int k, bool dead, unsigned seed) {
    std::mt19937 rng(seed);
    const Decomposition dec = make_decomposition(H, 1, true, "1d", "", W);
    const Geometry g = make_geometry(dec, 0);
    for (int trial = 0; trial < 3; ++trial) {
        const Rule rule = trial == 0 ? Rule() : (trial == 1 ? Rule::parse("B1357/S1357") : random_rule(rng));
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
        std::vector<u64> got, want;
        for (int ss = 0; ss < 3; ++ss) {
            cpu::fill_ghost_cols_wrap(cur, L, 0, H);
            cpu::fill_ghost_rows_wrap(cur, L);
            got.resize(got.size() + (size_t)k, 0);
            u64* res = cpu::superstep(cur, oth, L, k, rule, cpu::Edges(dead ? Boundary::Dead : Boundary::Torus, g), nullptr,
                                      got.data() + got.size() - (size_t)k);
            if (res != cur) std::swap(cur, oth);
            for (int gen = 0; gen < k; ++gen) {
                ref = byte_step(ref, H, W, rule, dead);
                want.push_back(byte_signature(ref, W, 0, 0, H, W));
            }
        }
        CHECK(got == want);
        CHECK(got.back() == cpu::signature(cur, L, 0, 0));
    }
}

// The published vectors, from cells.
static void test_vectors() {
    auto one = [](i64 H, i64 W, i64 r, i64 x) {
        std::vector<u8> b((size_t)(H * W), 0);
        b[(size_t)(r * W + x)] = 1;
        return byte_signature(b, W, 0, 0, H, W);
    };
    CHECK(byte_signature(std::vector<u8>(100, 0), 10, 0, 0, 10, 10) == 0);
    CHECK(one(8, 128, 0, 0) == 0x0000000093257869ull);
    CHECK(one(8, 128, 0, 1) == 0x00000000aafb63cfull);
    CHECK(one(8, 128, 1, 0) == 0x0000000010c50fd7ull);
    CHECK(one(8, 128, 5, 63) == 0x7956f7c180000000ull);
    CHECK(one(8, 128, 5, 64) == 0x00000000ec8a0243ull);
    std::vector<u8> b(200 * 200, 0);  // glider bob$2bo$3o, first cell at (100, 62)
    for (auto rc : {std::pair<int, int>{0, 1}, {1, 2}, {2, 0}, {2, 1}, {2, 2}}) b[(size_t)((100 + rc.first) * 200 + 62 + rc.second)] = 1;
    CHECK(byte_signature(b, 200, 0, 0, 200, 200) == 0xe6fd2de10676268aull);
    // ... and through the packed path
    const Layout L(200, 200, 1);
    std::vector<u64> buf((size_t)L.words(), 0), pw((size_t)(200 * L.nw), 0);
    for (i64 y = 0; y < 200; ++y)
        for (i64 x = 0; x < 200; ++x)
            if (b[(size_t)(y * 200 + x)]) pw[(size_t)(y * L.nw + x / 64)] |= 1ull << (x % 64);
    cpu::insert_words(buf.data(), L, pw.data());
    CHECK(cpu::signature(buf.data(), L, 0, 0) == 0xe6fd2de10676268aull);
}

int main() {
    test_vectors();
    for (int dead = 0; dead < 2; ++dead) {
        // 3 x 3 ranks, uneven rows; bounded: the last column of tiles ends in a partial word
        test_grid(30, 192, {0, 9, 20, 30}, {0, 64, 128, 192}, 4, dead != 0, 11u + (unsigned)dead);
        test_grid(23, 256, {0, 8, 15, 23}, {0, 64, 192, 256}, 3, dead != 0, 21u + (unsigned)dead);
        test_grid(24, 64, {0, 8, 16, 24}, {0, 64}, 5, dead != 0, 31u + (unsigned)dead);
        for (i64 W : {1, 3, 63, 64, 65, 130, 200})
            for (int k : {1, 2, 5}) test_one_rank(k > 3 ? 7 : 5, W, k, dead != 0, 41u + (unsigned)W + (unsigned)k);
    }
    test_grid(31, 150, {0, 10, 20, 31}, {0, 64, 128, 150}, 4, true, 51u);  // bounded, unaligned: 22 cells in the last tiles
    test_grid(12, 70, {0, 4, 8, 12}, {0, 64, 70}, 4, true, 52u);
    printf("signature unit tests: %d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
