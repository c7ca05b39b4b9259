// gol-mi355x: host-side tests of density-film mode (no GPU needed).  Run: build/gol_density_film_unit
//
// Covers: the CPU stepper's per-generation density maps (cpu::superstep with a DensityOut, through CPU engines on 1
// to 4 thread ranks whose maps Engine::density_film() sums) against a byte-per-cell loop and block count written
// here: random rules on the Moore, von Neumann and hexagonal neighbourhoods, both boundaries, unaligned widths, block
// shapes that divide nothing, a block taller than the board, one block (the census); the start and clear rules; and
// the parsing of GOL_DENSITY_FILM.
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "gol/density_film.hpp"
#include "gol/engine.hpp"
#include "gol/geometry.hpp"
#include "gol/rule.hpp"
#include "gol/transport.hpp"

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

// the neighbours a neighbourhood counts (rule.hpp): Moore all eight, von Neumann the four edge neighbours, hexagonal
// all but NE and SW
static bool counted(Nbhd n, int dy, int dx) {
    if (!dy && !dx) return false;
    if (n == Nbhd::VonNeumann) return !dy || !dx;
    if (n == Nbhd::Hex) return !((dy == -1 && dx == 1) || (dy == 1 && dx == -1));
    return true;
}

static std::vector<u8> byte_step(const std::vector<u8>& b, i64 H, i64 W, const Rule& r, bool dead) {
    std::vector<u8> o(b.size());
    for (i64 y = 0; y < H; ++y)
        for (i64 x = 0; x < W; ++x) {
            int n = 0;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!counted(r.nbhd, dy, dx)) continue;
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

static std::vector<u32> byte_map(const std::vector<u8>& b, i64 H, i64 W, i64 br, i64 bc) {
    const i64 gr = ceil_div(H, br), gc = ceil_div(W, bc);
    std::vector<u32> m((size_t)(gr * gc), 0);
    for (i64 y = 0; y < H; ++y)
        for (i64 x = 0; x < W; ++x) m[(size_t)((y / br) * gc + x / bc)] += b[(size_t)(y * W + x)];
    return m;
}

static Rule random_rule(std::mt19937& rng, Nbhd n) {
    const unsigned all = (2u << nbhd_max_count(n)) - 1u;
    return Rule::from_masks((rng() & 0x1FEu) & all, (rng() & 0x1FFu) & all, n);  // (B0 is refused)
}

// P thread ranks (strips) step an H x W board: a superstep of R generations, a remainder, a clear and two more
// generations; every rank's maps must be the byte loop's, and the starts the census's.
static void test_ranks(int P, i64 H, i64 W, int R, const Rule& rule, bool dead, i64 br, i64 bc, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<u8> board((size_t)(H * W));
    for (auto& v : board) v = (u8)(rng() & 1);
    const int gens1 = R + 2, gens2 = 2;
    std::vector<std::vector<u32>> ref;
    std::vector<u8> cur = board;
    for (int g = 0; g < gens1 + gens2; ++g) {
        cur = byte_step(cur, H, W, rule, dead);
        ref.push_back(byte_map(cur, H, W, br, bc));
    }
    const Decomposition dec = make_decomposition(H, P, true, "1d", "", W);
    const size_t blocks = ref[0].size();
    std::vector<int> ok((size_t)P, 0);
    std::shared_ptr<ThreadGroup> group = P > 1 ? make_thread_group(P) : nullptr;
    auto rank_main = [&](int r) {
        try {
            const Geometry g = make_geometry(dec, r);
            std::shared_ptr<Transport> t;
            if (P > 1)
                t = std::make_shared<ThreadTransport>(group, r);
            else
                t = std::make_shared<SelfTransport>();
            EngineConfig cfg;
            cfg.backend = "cpu";
            cfg.rule = rule;
            cfg.boundary = dead ? Boundary::Dead : Boundary::Torus;
            cfg.halo_depth = R;
            cfg.density_film = DensityBlocks{true, br, bc};
            std::unique_ptr<Engine> e = Engine::create(g, cfg, t);
            e->init(PatternSpec{});
            const i64 nw = ceil_div(g.w, 64);
            std::vector<u64> dense((size_t)(g.h * nw), 0);
            for (i64 y = 0; y < g.h; ++y)
                for (i64 x = 0; x < g.w; ++x)
                    dense[(size_t)(y * nw + x / 64)] |= (u64)board[(size_t)((g.row0 + y) * W + g.col0 + x)] << (x & 63);
            e->set_tile_words(dense);
            bool good = e->density_geo().blocks() == (i64)blocks && e->stats().density_film == cfg.density_film;
            e->run((u64)gens1);
            Engine::DensityFilm f = e->density_film();
            good = good && f.start == 0 && f.n == (size_t)gens1 && f.maps.size() == f.n * blocks;
            for (int j = 0; good && j < gens1; ++j)
                good = std::equal(ref[(size_t)j].begin(), ref[(size_t)j].end(), f.maps.begin() + (size_t)j * blocks);
            e->density_film_clear();
            e->run((u64)gens2);
            f = e->density_film();
            good = good && f.start == (u64)gens1 && f.n == (size_t)gens2 && f.maps.size() == f.n * blocks;
            for (int j = 0; good && j < gens2; ++j)
                good = std::equal(ref[(size_t)(gens1 + j)].begin(), ref[(size_t)(gens1 + j)].end(), f.maps.begin() + (size_t)j * blocks);
            ok[(size_t)r] = good;
        } catch (const std::exception& ex) {
            fprintf(stderr, "rank %d: %s\n", r, ex.what());
        }
    };
    std::vector<std::thread> th;
    for (int r = 1; r < P; ++r) th.emplace_back(rank_main, r);
    rank_main(0);
    for (auto& t : th) t.join();
    for (int r = 0; r < P; ++r) {
        if (!ok[(size_t)r])
            fprintf(stderr, "maps mismatch: rank %d of %d, rule %s, %s, %lld x %lld board, blocks %lld x %lld, R = %d\n", r, P,
                    rule.str().c_str(), dead ? "dead" : "torus", (long long)H, (long long)W, (long long)br, (long long)bc, R);
        CHECK(ok[(size_t)r]);
    }
}

static bool refused(const char* s) {
    try {
        (void)parse_density_film(s);
    } catch (const Error& e) {
        return std::string(e.what()).find("GOL_DENSITY_FILM") != std::string::npos && std::string(e.what()).find(s) != std::string::npos;
    }
    return false;
}

static void test_parse() {
    CHECK((parse_density_film("512") == DensityBlocks{true, 512, 512}));
    CHECK((parse_density_film("7,64") == DensityBlocks{true, 7, 64}));
    CHECK((parse_density_film(" 8 , 128 ") == DensityBlocks{true, 8, 128}));
    CHECK((parse_density_film("-3,64") == DensityBlocks{true, -3, 64}));  // (the engine names the value it refuses)
    for (const char* s : {"", "x", "7,", "7,64,1", "7x64", "7,64x", ",64", "7 64"}) CHECK(refused(s));
    // the grid and the slot
    const DensityGeo g(DensityBlocks{true, 7, 128}, 137, 200);
    CHECK(g.block_words == 2 && g.grid_rows == 20 && g.grid_cols == 2 && g.blocks() == 40 && g.slot_words() == 20);
    const DensityGeo one(DensityBlocks{true, 200, 256}, 137, 200);
    CHECK(one.blocks() == 1 && one.slot_words() == 1);
    const DensityGeo odd(DensityBlocks{true, 50, 64}, 137, 137);
    CHECK(odd.grid_rows == 3 && odd.grid_cols == 3 && odd.slot_words() == 5);
}

int main() {
    test_parse();
    std::mt19937 rng(2026);
    const i64 shapes[][2] = {{1, 64}, {7, 64}, {8, 128}, {5, 192}, {1000, 256}};
    unsigned seed = 100;
    for (int dead = 0; dead < 2; ++dead)
        for (Nbhd n : {Nbhd::Moore, Nbhd::VonNeumann, Nbhd::Hex})
            for (int P = 1; P <= 4; ++P) {
                const i64 W = (P & 1) ? 137 : 200;  // (strips: any width)
                for (int trial = 0; trial < 2; ++trial) {
                    const Rule rule = random_rule(rng, n);
                    const i64* s = shapes[(seed + (unsigned)trial) % 5];
                    test_ranks(P, 12 * P + (trial ? 5 : 0), W, trial ? 5 : 3, rule, dead != 0, s[0], s[1], seed);
                    ++seed;
                }
            }
    test_ranks(1, 3, 65, 3, Rule::parse("B36/S23"), false, 2, 64, 7u);
    test_ranks(2, 40, 130, 8, Rule::parse("B1/S012345678"), true, 7, 64, 8u);
    printf("density film unit tests: %d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
