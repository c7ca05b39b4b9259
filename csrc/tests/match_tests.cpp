// gol-mi355x: host-side tests of pattern matching (gol/match.hpp; no GPU needed).  Run: build/gol_match_unit
//
// Covers: match_host, the CPU backends' matcher, against a byte-per-cell loop written here, on random boards (one word,
// word seams, tail words of 36 and of 2 cells, a board narrower than a word) and random templates (care masks of every
// density, negative offsets through the ring) on the torus and on the bounded board; the bitmap, the OR into it and
// match_positions_host; the orientations (a block has 1, a blinker 2, a glider 8; ids and shapes); the builders; and
// the refusals.
#include <cstring>
#include <string>
#include <vector>

#include "gol/bits.hpp"
#include "gol/match.hpp"

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

struct Board {
    i64 h, w;
    std::vector<u8> cells;
    std::vector<u64> words;
    Board(i64 h_, i64 w_, u64 seed, int density_shift) : h(h_), w(w_), cells((size_t)(h_ * w_)), words((size_t)(h_ * ceil_div(w_, 64))) {
        const i64 nw = ceil_div(w, 64);
        for (i64 r = 0; r < h; ++r)
            for (i64 c = 0; c < w; ++c) {
                const bool on = (mix64(seed * 1000003ull + (u64)(r * w + c)) >> 7) % (1u << density_shift) == 0;
                cells[(size_t)(r * w + c)] = on;
                if (on) words[(size_t)(r * nw + (c >> 6))] |= 1ull << (c & 63);
            }
    }
    int at(i64 r, i64 c, bool torus) const {
        if (torus) return cells[(size_t)(pmod(r, h) * w + pmod(c, w))];
        return (r < 0 || r >= h || c < 0 || c >= w) ? 0 : cells[(size_t)(r * w + c)];
    }
};

static bool matches_at(const Board& b, const MatchTemplate& t, i64 r, i64 c, bool torus) {
    for (int i = 0; i < t.th; ++i)
        for (int j = 0; j < t.tw; ++j)
            if (t.cell_care(i, j) && b.at(r - t.ring + i, c - t.ring + j, torus) != (int)t.cell_value(i, j)) return false;
    return true;
}

// a random template whose values are copied from the board at (r0, c0), so that it matches there
static MatchTemplate random_template(const Board& b, int th, int tw, int ring, u64 seed, int care_shift, i64 r0, i64 c0, bool torus) {
    std::vector<u8> value((size_t)(th * tw)), care((size_t)(th * tw));
    for (int i = 0; i < th; ++i)
        for (int j = 0; j < tw; ++j) {
            const bool on = (mix64(seed + (u64)(i * 37 + j)) >> 9) % (1u << care_shift) == 0 || (i == 0 && j == 0) ||
                            (i == th - 1 && j == tw - 1);
            care[(size_t)(i * tw + j)] = on;
            value[(size_t)(i * tw + j)] = on && b.at(r0 - ring + i, c0 - ring + j, torus);
        }
    return MatchTemplate::from_cells(value.data(), care.data(), th, tw, ring);
}

static void test_matcher(i64 h, i64 w, bool torus, int density_shift, int th, int tw, int ring, int care_shift, u64 seed) {
    const Board b(h, w, seed, density_shift);
    const i64 nw = ceil_div(w, 64), r0 = h - 1, c0 = w - 1;  // (the box crosses both seams)
    const MatchTemplate t = random_template(b, th, tw, ring, seed * 7 + 1, care_shift, r0, c0, torus);
    t.validate(h, w);
    std::vector<u64> bits((size_t)(h * nw), ~0ull);
    const u64 n = match_host(b.words.data(), h, w, torus, t, bits.data());
    u64 want = 0;
    bool same = true;
    for (i64 r = 0; r < h; ++r)
        for (i64 c = 0; c < 64 * nw; ++c) {
            const bool m = c < w && matches_at(b, t, r, c, torus);
            want += m;
            same = same && (((bits[(size_t)(r * nw + (c >> 6))] >> (c & 63)) & 1ull) == (u64)m);
        }
    CHECK(same);
    CHECK(n == want);
    CHECK(want >= 1);  // (it matches where it was copied from)
    CHECK(match_host(b.words.data(), h, w, torus, t, nullptr) == want);
    // positions: row-major, capped
    std::vector<i32> pos;
    match_positions_host(bits.data(), h, w, (i64)want + 5, &pos);
    CHECK(pos.size() == 2 * want);
    bool ordered = true, real = true;
    for (size_t k = 0; k < pos.size() / 2; ++k) {
        real = real && matches_at(b, t, pos[2 * k], pos[2 * k + 1], torus);
        if (k) ordered = ordered && (pos[2 * k - 2] < pos[2 * k] || (pos[2 * k - 2] == pos[2 * k] && pos[2 * k - 1] < pos[2 * k + 1]));
    }
    CHECK(ordered && real);
    std::vector<i32> few;
    match_positions_host(bits.data(), h, w, 1, &few);
    CHECK(few.size() == 2 && few[0] == pos[0] && few[1] == pos[1]);
    // or_into: a second template's matches join the first's
    const MatchTemplate t2 = random_template(b, 2, 2, 0, seed + 99, 0, 1, 1, torus);
    std::vector<u64> both = bits, second((size_t)(h * nw));
    const u64 n2 = match_host(b.words.data(), h, w, torus, t2, both.data(), true);
    CHECK(n2 == match_host(b.words.data(), h, w, torus, t2, second.data()));
    bool ored = true;
    for (size_t k = 0; k < both.size(); ++k) ored = ored && both[k] == (bits[k] | second[k]);
    CHECK(ored);
}

static RlePattern pattern_of(const std::vector<std::string>& rows) {
    RlePattern p;
    p.rows = (i64)rows.size(), p.cols = (i64)rows[0].size();
    p.words.assign((size_t)(p.rows * p.nw()), 0);
    for (i64 r = 0; r < p.rows; ++r)
        for (i64 c = 0; c < p.cols; ++c)
            if (rows[(size_t)r][(size_t)c] == 'o') p.set(r, c);
    return p;
}

int main() {
    // the matcher against the per-cell loop
    u64 seed = 1;
    for (bool torus : {true, false})
        for (auto hw : {std::pair<i64, i64>{64, 64}, {40, 192}, {33, 100}, {35, 130}, {34, 40}, {32, 32}}) {
            test_matcher(hw.first, hw.second, torus, 1, 3, 3, 1, 0, seed++);    // every cell constrained
            test_matcher(hw.first, hw.second, torus, 1, 1, 32, 0, 1, seed++);   // one row, 32 wide
            test_matcher(hw.first, hw.second, torus, 1, 32, 1, 0, 1, seed++);   // one column
            test_matcher(hw.first, hw.second, torus, 1, 32, 32, 0, 5, seed++);  // sparse care, offsets 0 .. 31
            test_matcher(hw.first, hw.second, torus, 1, 32, 32, 15, 5, seed++); // offsets -15 .. 16
            test_matcher(hw.first, hw.second, torus, 3, 5, 7, 2, 2, seed++);    // a sparse board
            test_matcher(hw.first, hw.second, torus, 1, 2, 2, 0, 0, seed++);
        }
    // the builders
    {
        const RlePattern glider = pattern_of({"bob", "bbo", "ooo"});
        const MatchTemplate t = MatchTemplate::from_pattern(glider, 1);
        CHECK(t.th == 5 && t.tw == 5 && t.ring == 1);
        bool ok = true;
        for (int i = 0; i < 5; ++i)
            for (int j = 0; j < 5; ++j) {
                const bool in = i >= 1 && i <= 3 && j >= 1 && j <= 3;
                ok = ok && t.cell_care(i, j) && t.cell_value(i, j) == (in && glider.cell(i - 1, j - 1));
            }
        CHECK(ok);
        const MatchTemplate t0 = MatchTemplate::from_pattern(glider, 0);
        CHECK(t0.th == 3 && t0.tw == 3 && t0.ring == 0 && t0.value[0] == 2u && t0.value[1] == 4u && t0.value[2] == 7u);
    }
    // orientations: ids, shapes, dedup
    {
        const MatchTemplate block = MatchTemplate::from_pattern(pattern_of({"oo", "oo"}), 1);
        const MatchTemplate blinker = MatchTemplate::from_pattern(pattern_of({"ooo"}), 1);
        const MatchTemplate glider = MatchTemplate::from_pattern(pattern_of({"bob", "bbo", "ooo"}), 1);
        CHECK(block.orientations(true).size() == 1);
        CHECK(blinker.orientations(true).size() == 2);
        CHECK(glider.orientations(true).size() == 8);
        CHECK(glider.orientations(false).size() == 1 && glider.orientations(false)[0].first == 0);
        const auto bl = blinker.orientations(true);
        CHECK(bl[0].first == 0 && bl[1].first == 1 && bl[1].second.th == 5 && bl[1].second.tw == 3 && bl[1].second.ring == 1);
        CHECK(bl[1].second.value[1] == 2u && bl[1].second.value[2] == 2u && bl[1].second.value[3] == 2u);
        for (int k = 0; k < 8; ++k) CHECK(glider.orientations(true)[(size_t)k].first == k);
        // a quarter turn clockwise: the first row becomes the last column
        const MatchTemplate g0 = MatchTemplate::from_pattern(pattern_of({"bob", "bbo", "ooo"}), 0);
        const MatchTemplate g1 = g0.oriented(1);  // ob. / o.o / oo.  read as rows: "obb", "obo", "oob"
        CHECK(g1.value[0] == 1u && g1.value[1] == 5u && g1.value[2] == 3u);
        CHECK(g0.oriented(2).value[0] == 7u && g0.oriented(2).value[1] == 1u && g0.oriented(2).value[2] == 2u);
        CHECK(g0.oriented(4).value[0] == 2u && g0.oriented(4).value[1] == 1u && g0.oriented(4).value[2] == 7u);
        CHECK(g0.oriented(1).oriented(1) == g0.oriented(2) && g0.oriented(3).oriented(1) == g0);
        CHECK(g0.oriented(5) == g0.oriented(4).oriented(1));
    }
    // refusals
    {
        const RlePattern big = [] {
            RlePattern p;
            p.rows = 31, p.cols = 4;
            p.words.assign(31, 1);
            return p;
        }();
        CHECK(throws([&] { MatchTemplate::from_pattern(big, 1); }));   // 33 rows
        CHECK(!throws([&] { MatchTemplate::from_pattern(big, 0); }));
        CHECK(throws([&] { MatchTemplate::from_pattern(big, -1); }));  // a negative margin
        std::vector<u8> ones(33 * 33, 1), zeros(33 * 33, 0);
        CHECK(throws([&] { MatchTemplate::from_cells(ones.data(), ones.data(), 33, 2, 0); }));
        CHECK(throws([&] { MatchTemplate::from_cells(ones.data(), ones.data(), 2, 0, 0); }));
        CHECK(throws([&] { MatchTemplate::from_cells(zeros.data(), zeros.data(), 3, 3, 0).validate(); }));  // no care cell
        CHECK(throws([&] { MatchTemplate::from_cells(ones.data(), zeros.data(), 3, 3, 0).validate(); }));   // value outside care
        CHECK(throws([&] { MatchTemplate::from_cells(ones.data(), ones.data(), 4, 6, 2).validate(); }));    // 2 ring = min
        CHECK(throws([&] { MatchTemplate::from_cells(ones.data(), ones.data(), 4, 6, -1).validate(); }));
        CHECK(!throws([&] { MatchTemplate::from_cells(ones.data(), ones.data(), 5, 6, 2).validate(); }));
        const MatchTemplate t = MatchTemplate::from_cells(ones.data(), ones.data(), 5, 6, 2);
        CHECK(throws([&] { t.validate(4, 64); }));  // th > H
        CHECK(throws([&] { t.validate(64, 5); }));  // tw > W
        CHECK(!throws([&] { t.validate(5, 6); }));
        CHECK(throws([&] { t.oriented(8); }));
    }
    printf("gol_match_unit: %d checks passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
