// gol-mi355x: host-side tests of connected components (gol/components.hpp; no GPU needed).  Run: build/gol_components_unit
//
// Covers: components_host, the CPU backends' labeller, against a byte-per-cell flood fill written here, on random boards of
// three densities and on adversarial ones (empty, full, one cell, a full row, a comb, the serpentine snake, the
// checkerboard), on the torus and on the bounded board, under all three neighbourhoods, on shapes of one word, word
// seams and tail words of 36 and of 2 cells, alone and as a batch; the box rule against extents measured from the cell
// lists; the hash against arrays turned cell by cell, and its equality over the eight turns; truncation; the refusals.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "gol/components.hpp"

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

template <typename F>
static bool throws(F f) {
    try {
        f();
    } catch (const Error&) {
        return true;
    }
    return false;
}

struct Cells {
    i64 h, w;
    std::vector<u8> c;
    Cells(i64 h_, i64 w_) : h(h_), w(w_), c((size_t)(h_ * w_), 0) {}
    u8& at(i64 r, i64 col) { return c[(size_t)(r * w + col)]; }
    u8 at(i64 r, i64 col) const { return c[(size_t)(r * w + col)]; }
    std::vector<u64> words() const {
        const i64 nw = ceil_div(w, 64);
        std::vector<u64> out((size_t)(h * nw), 0);
        for (i64 r = 0; r < h; ++r)
            for (i64 col = 0; col < w; ++col)
                if (at(r, col)) out[(size_t)(r * nw + (col >> 6))] |= 1ull << (col & 63);
        return out;
    }
};

static bool joined(int dr, int dc, CcNeighbourhood nb) {
    const int a = dr < 0 ? -dr : dr, b = dc < 0 ? -dc : dc;
    if (a == 0 && b == 0) return false;
    if (nb == CcNeighbourhood::VonNeumann) return a + b == 1;
    return std::max(a, b) <= (nb == CcNeighbourhood::Moore ? 1 : 2);
}

// the flood fill: labels 1 + the first cell of the component in row-major order
static std::vector<i32> flood(const Cells& b, bool torus, CcNeighbourhood nb) {
    std::vector<i32> lab((size_t)(b.h * b.w), 0);
    std::vector<i64> stack;
    for (i64 s = 0; s < b.h * b.w; ++s) {
        if (!b.c[(size_t)s] || lab[(size_t)s]) continue;
        lab[(size_t)s] = (i32)(1 + s);
        stack.push_back(s);
        while (!stack.empty()) {
            const i64 x = stack.back();
            stack.pop_back();
            for (int dr = -2; dr <= 2; ++dr)
                for (int dc = -2; dc <= 2; ++dc) {
                    if (!joined(dr, dc, nb)) continue;
                    i64 r = x / b.w + dr, c = x % b.w + dc;
                    if (torus)
                        r = pmod(r, b.h), c = pmod(c, b.w);
                    else if (r < 0 || r >= b.h || c < 0 || c >= b.w)
                        continue;
                    if (b.at(r, c) && !lab[(size_t)(r * b.w + c)]) {
                        lab[(size_t)(r * b.w + c)] = (i32)(1 + s);
                        stack.push_back(r * b.w + c);
                    }
                }
        }
    }
    return lab;
}

// the box rule on one axis from a list of coordinates
static void axis_box(const std::vector<i64>& xs, i64 L, bool torus, i64& x0, i64& len) {
    i64 mn = L, mx = -1, mn2 = L, mx2 = -1;
    for (i64 x : xs) {
        mn = std::min(mn, x), mx = std::max(mx, x);
        const i64 y = (x + L / 2) % L;
        mn2 = std::min(mn2, y), mx2 = std::max(mx2, y);
    }
    if (!torus || mx - mn <= mx2 - mn2)
        x0 = mn, len = mx - mn + 1;
    else
        x0 = pmod(mn2 - L / 2, L), len = mx2 - mn2 + 1;
}

// orientation k of a rows x cols array, turned cell by cell: a left-right mirror image for k >= 4, then k & 3 clockwise
// quarter turns (new (i, j) = old (rows - 1 - j, i))
static std::vector<u8> turned(std::vector<u8> a, i64& rows, i64& cols, int k) {
    if (k >= 4) {
        std::vector<u8> m(a.size());
        for (i64 i = 0; i < rows; ++i)
            for (i64 j = 0; j < cols; ++j) m[(size_t)(i * cols + j)] = a[(size_t)(i * cols + cols - 1 - j)];
        a = m;
    }
    for (int t = 0; t < (k & 3); ++t) {
        std::vector<u8> n(a.size());
        const i64 nr = cols, nc = rows;
        for (i64 i = 0; i < nr; ++i)
            for (i64 j = 0; j < nc; ++j) n[(size_t)(i * nc + j)] = a[(size_t)((rows - 1 - j) * cols + i)];
        a = n, rows = nr, cols = nc;
    }
    return a;
}

static u64 plain_sum(const std::vector<u8>& a, i64 rows, i64 cols) {
    u64 s = 0;
    for (i64 i = 0; i < rows; ++i)
        for (i64 j = 0; j < cols; ++j)
            if (a[(size_t)(i * cols + j)]) s += (u64)sig_rho((u32)i) * (u64)sig_gam((u32)j);
    return s;
}

static u64 hash_by_turning(const std::vector<u8>& a, i64 rows, i64 cols) {
    u64 best = ~0ull;
    for (int k = 0; k < 8; ++k) {
        i64 r = rows, c = cols;
        const std::vector<u8> t = turned(a, r, c, k);
        best = std::min(best, plain_sum(t, r, c));
    }
    return best;
}

static void check_board(const Cells& b, bool torus, CcNeighbourhood nb) {
    const std::vector<u64> words = b.words();
    const std::vector<i32> want = flood(b, torus, nb);
    std::vector<i32> lab((size_t)(b.h * b.w), -7);
    const ComponentsResult res = components_host(words.data(), b.h, b.w, 1, torus, nb, 1 << 20, true, true, lab.data());
    CHECK(lab == want);
    // the objects from the flood fill's labels
    std::vector<i32> roots;
    for (i64 s = 0; s < b.h * b.w; ++s)
        if (want[(size_t)s] == 1 + s) roots.push_back((i32)s);
    CHECK(res.count == roots.size() && !res.truncated && res.population.size() == roots.size());
    CHECK(res.per_board.size() == 1 && res.per_board[0] == roots.size());
    if (res.population.size() != roots.size()) return;
    bool ok = true;
    const size_t step = roots.size() > 400 ? roots.size() / 200 : 1;  // (every object of a small census, a sample of a large one)
    for (size_t k = 0; k < roots.size(); ++k) {
        ok = ok && res.anchor[2 * k] == roots[k] / b.w && res.anchor[2 * k + 1] == roots[k] % b.w && res.board[k] == 0;
        if (k % step) continue;
        std::vector<i64> rs, cs;
        for (i64 s = 0; s < b.h * b.w; ++s)
            if (want[(size_t)s] == 1 + roots[k]) rs.push_back(s / b.w), cs.push_back(s % b.w);
        i64 r0, rows, c0, cols;
        axis_box(rs, b.h, torus, r0, rows);
        axis_box(cs, b.w, torus, c0, cols);
        ok = ok && res.population[k] == rs.size();
        ok = ok && res.bbox[4 * k] == r0 && res.bbox[4 * k + 1] == c0 && res.bbox[4 * k + 2] == rows && res.bbox[4 * k + 3] == cols;
        std::vector<u8> a((size_t)(rows * cols), 0);
        for (size_t i = 0; i < rs.size(); ++i) a[(size_t)(pmod(rs[i] - r0, b.h) * cols + pmod(cs[i] - c0, b.w))] = 1;
        if (rows * cols <= 1 << 16) ok = ok && res.hash[k] == hash_by_turning(a, rows, cols);
        ok = ok && res.hash[k] == object_hash_host(a.data(), rows, cols);
    }
    CHECK(ok);
    // the count alone; no hashes
    const ComponentsResult cnt = components_host(words.data(), b.h, b.w, 1, torus, nb, 1, false, false, nullptr);
    CHECK(cnt.count == roots.size() && cnt.population.empty() && !cnt.truncated);
    const ComponentsResult nohash = components_host(words.data(), b.h, b.w, 1, torus, nb, 1 << 20, false, true, nullptr);
    CHECK(nohash.hash.empty() && nohash.bbox == res.bbox && nohash.population == res.population);
}

static Cells random_cells(i64 h, i64 w, u64 seed, int per_mille) {
    Cells b(h, w);
    for (i64 s = 0; s < h * w; ++s) b.c[(size_t)s] = (mix64(seed * 1000003ull + (u64)s) >> 11) % 1000 < (u64)per_mille;
    return b;
}

static std::vector<Cells> adversarial(i64 h, i64 w) {
    std::vector<Cells> out;
    out.emplace_back(h, w);  // empty
    Cells full(h, w);
    std::fill(full.c.begin(), full.c.end(), 1);
    out.push_back(full);
    Cells one(h, w);
    one.at(h - 1, w - 1) = 1;
    out.push_back(one);
    Cells row(h, w);
    for (i64 c = 0; c < w; ++c) row.at(5, c) = 1;
    out.push_back(row);
    Cells comb(h, w);  // a spine along row 0 with a tooth in every second column
    for (i64 c = 0; c < w; ++c) comb.at(0, c) = 1;
    for (i64 r = 1; r < h - 2; ++r)
        for (i64 c = 0; c < w; c += 2) comb.at(r, c) = 1;
    out.push_back(comb);
    Cells snake(h, w);  // every second row full, joined alternately at the right and left ends
    for (i64 r = 0; r < h - 2; r += 2) {
        for (i64 c = 1; c < w - 1; ++c) snake.at(r, c) = 1;
        if (r + 2 < h - 2) snake.at(r + 1, (r / 2) % 2 ? 1 : w - 2) = 1;
    }
    out.push_back(snake);
    Cells checker(h, w);
    for (i64 r = 0; r < h; ++r)
        for (i64 c = 0; c < w; ++c) checker.at(r, c) = (r + c) % 2 == 0;
    out.push_back(checker);
    return out;
}

int main() {
    const CcNeighbourhood nbs[3] = {CcNeighbourhood::VonNeumann, CcNeighbourhood::Moore, CcNeighbourhood::Moore2};
    u64 seed = 1;
    for (auto hw : {std::pair<i64, i64>{64, 64}, {40, 192}, {33, 100}, {35, 130}, {34, 40}})
        for (bool torus : {true, false})
            for (CcNeighbourhood nb : nbs) {
                for (int per_mille : {100, 300, 500}) check_board(random_cells(hw.first, hw.second, seed++, per_mille), torus, nb);
                for (const Cells& b : adversarial(hw.first, hw.second)) check_board(b, torus, nb);
            }
    // the neighbourhoods by hand: two cells at Chebyshev distance 1 (diagonal), 2 and 3
    {
        Cells b(16, 16);
        b.at(2, 2) = b.at(3, 3) = 1;   // diagonal
        b.at(8, 2) = b.at(8, 4) = 1;   // distance 2
        b.at(12, 2) = b.at(12, 5) = 1; // distance 3
        const std::vector<u64> w = b.words();
        CHECK(components_host(w.data(), 16, 16, 1, true, CcNeighbourhood::VonNeumann, 100, false, false, nullptr).count == 6);
        CHECK(components_host(w.data(), 16, 16, 1, true, CcNeighbourhood::Moore, 100, false, false, nullptr).count == 5);
        CHECK(components_host(w.data(), 16, 16, 1, true, CcNeighbourhood::Moore2, 100, false, false, nullptr).count == 4);
    }
    // the box rule by hand: a block on the torus corner, and a row that takes more than half of the axis
    {
        Cells b(16, 20);
        b.at(0, 0) = b.at(0, 19) = b.at(15, 0) = b.at(15, 19) = 1;
        const std::vector<u64> w = b.words();
        const ComponentsResult t = components_host(w.data(), 16, 20, 1, true, CcNeighbourhood::Moore, 100, true, true, nullptr);
        CHECK(t.count == 1 && t.anchor[0] == 0 && t.anchor[1] == 0 && t.population[0] == 4);
        CHECK(t.bbox == (std::vector<i64>{15, 19, 2, 2}));
        const u8 block[4] = {1, 1, 1, 1};
        CHECK(t.hash[0] == object_hash_host(block, 2, 2));
        const ComponentsResult d = components_host(w.data(), 16, 20, 1, false, CcNeighbourhood::Moore, 100, true, true, nullptr);
        CHECK(d.count == 4 && d.bbox[0] == 0 && d.bbox[1] == 0 && d.bbox[2] == 1 && d.bbox[3] == 1);
        Cells r(16, 20);
        for (i64 c = 15; c < 20 + 8; ++c) r.at(3, c % 20) = 1;  // 13 cells across the seam: columns 15 .. 19, 0 .. 7
        const std::vector<u64> rw = r.words();
        const ComponentsResult q = components_host(rw.data(), 16, 20, 1, true, CcNeighbourhood::Moore, 100, false, true, nullptr);
        CHECK(q.count == 1 && q.bbox == (std::vector<i64>{3, 15, 1, 13}));
    }
    // the hash: the same under the eight turns and under translation, different for different objects
    {
        const std::vector<u8> glider = {0, 1, 0, 0, 0, 1, 1, 1, 1};
        const u64 h0 = object_hash_host(glider.data(), 3, 3);
        CHECK(h0 == hash_by_turning(glider, 3, 3));
        for (int k = 0; k < 8; ++k) {
            i64 r = 3, c = 3;
            const std::vector<u8> t = turned(glider, r, c, k);
            CHECK(object_hash_host(t.data(), r, c) == h0);
            Cells b(64, 100);
            for (i64 i = 0; i < r; ++i)
                for (i64 j = 0; j < c; ++j) b.at((62 + i) % 64, (98 + j) % 100) = t[(size_t)(i * c + j)];  // on the torus corner
            const std::vector<u64> w = b.words();
            const ComponentsResult res = components_host(w.data(), 64, 100, 1, true, CcNeighbourhood::Moore, 10, true, true, nullptr);
            CHECK(res.count == 1 && res.hash[0] == h0 && res.bbox == (std::vector<i64>{62, 98, 3, 3}));
        }
        const std::vector<u8> lshape = {1, 0, 1, 0, 1, 1}, ishape = {1, 1, 1, 1};
        i64 r = 3, c = 2;
        const std::vector<u8> lturned = turned(lshape, r, c, 5);
        CHECK(r == 2 && c == 3 && object_hash_host(lshape.data(), 3, 2) == object_hash_host(lturned.data(), r, c));
        CHECK(object_hash_host(lshape.data(), 3, 2) != object_hash_host(ishape.data(), 4, 1));
        CHECK(object_hash_host(ishape.data(), 4, 1) == object_hash_host(ishape.data(), 1, 4));
        CHECK(object_hash_host(ishape.data(), 2, 2) != object_hash_host(ishape.data(), 1, 4));
    }
    // a batch: every board its own torus; truncation
    {
        const i64 S = 64, n = 5;
        std::vector<u64> words;
        std::vector<ComponentsResult> each;
        for (i64 i = 0; i < n; ++i) {
            Cells b = random_cells(S, S, 77 + (u64)i, 150);
            b.at(S - 1, S - 1) = b.at(S - 1, 0) = b.at(0, S - 1) = 1;  // across the corner, into its own board
            const std::vector<u64> w = b.words();
            words.insert(words.end(), w.begin(), w.end());
            each.push_back(components_host(w.data(), S, S, 1, true, CcNeighbourhood::Moore, 1 << 20, true, true, nullptr));
        }
        const ComponentsResult all = components_host(words.data(), S, S, n, true, CcNeighbourhood::Moore, 1 << 20, true, true, nullptr);
        size_t at = 0;
        bool ok = all.per_board.size() == (size_t)n;
        for (i64 i = 0; i < n && ok; ++i) {
            ok = ok && all.per_board[(size_t)i] == each[(size_t)i].count;
            for (size_t k = 0; k < each[(size_t)i].population.size() && ok; ++k, ++at)
                ok = all.board[at] == i && all.anchor[2 * at] == each[(size_t)i].anchor[2 * k] &&
                     all.anchor[2 * at + 1] == each[(size_t)i].anchor[2 * k + 1] && all.hash[at] == each[(size_t)i].hash[k] &&
                     all.population[at] == each[(size_t)i].population[k] &&
                     std::equal(all.bbox.begin() + 4 * (i64)at, all.bbox.begin() + 4 * (i64)at + 4, each[(size_t)i].bbox.begin() + 4 * (i64)k);
        }
        CHECK(ok && at == all.population.size() && all.count == at);
        const ComponentsResult cut = components_host(words.data(), S, S, n, true, CcNeighbourhood::Moore, 3, true, true, nullptr);
        CHECK(cut.count == all.count && cut.truncated && cut.population.size() == 3 && cut.hash.size() == 3);
        CHECK(std::equal(cut.hash.begin(), cut.hash.end(), all.hash.begin()) && std::equal(cut.bbox.begin(), cut.bbox.end(), all.bbox.begin()));
    }
    // refusals
    {
        const std::vector<u64> w(64, 0);
        CHECK(throws([&] { components_host(w.data(), 64, 64, 1, true, CcNeighbourhood::Moore, 0, true, true, nullptr); }));
        CHECK(throws([&] { cc_check(65536, 32768, 1, 10, "t"); }));      // 2^31 cells
        CHECK(throws([&] { cc_check(64, 64, 1 << 19, 10, "t"); }));      // 2^31 cells in a batch
        CHECK(!throws([&] { cc_check(32768, 32768, 1, 10, "t"); }));     // 2^30
        CHECK(throws([&] { cc_neighbourhood("hex"); }));
        CHECK(cc_neighbourhood("moore2") == CcNeighbourhood::Moore2 && cc_neighbourhood("von_neumann") == CcNeighbourhood::VonNeumann);
        CHECK(std::string(cc_neighbourhood_name(CcNeighbourhood::Moore)) == "moore");
    }
    printf("gol_components_unit: %d checks passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
