// gol-mi355x: host-side tests of the dense-cell conversions (gol/cells.hpp; no GPU needed).  Run: build/gol_tensor_unit
//
// Covers: unpack_cells_host and pack_cells_host, the CPU backends' conversions and the description the device kernels
// share, against a per-cell loop written here on storage_bit(): all four element types; the three layouts (a board
// buffer with halo rows and ghost words read through a wrapping rectangle, film frames across the x seam and the
// board's tail word, a soup store); tail words of 1 and of 63 cells; the odd values of packing (2, -1, 0.5, -0.0,
// NaN); ghost cells of a tile's last word kept out of the output; and the refusals (numel one too small, a rectangle
// that reaches outside its words, a misaligned pointer).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gol/bits.hpp"
#include "gol/cells.hpp"
#include "gol/film.hpp"
#include "gol/geometry.hpp"

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

static const CellType kTypes[] = {CellType::U8, CellType::F16, CellType::BF16, CellType::F32};

// cell c of a row of split words, straight from the storage bit
static int cell_of(const u64* row, i64 c) { return (int)((row[c >> 6] >> storage_bit(c)) & 1ull); }

static u32 element(const std::vector<u8>& buf, CellType t, i64 i) {
    u32 v = 0;
    std::memcpy(&v, buf.data() + i * cell_size(t), (size_t)cell_size(t));
    return v;
}

template <typename F>
static bool throws(F f) {
    try {
        f();
    } catch (const Error&) {
        return true;
    }
    return false;
}

// a board buffer in layout L, every word random (ghost rows, ghost words and the ghost cells of the last word too)
static std::vector<u64> random_buffer(const Layout& L, u64 seed) {
    std::vector<u64> b((size_t)L.words());
    for (size_t i = 0; i < b.size(); ++i) b[i] = mix64(seed + i);
    return b;
}

static CellSource board_source(const std::vector<u64>& buf, const Layout& L, i64 r0, i64 c0, i64 rows, i64 cols) {
    CellSource s;
    s.base = buf.data() + L.index(0, 0);
    s.words = L.words() - L.index(0, 0);
    s.frame_stride = 0, s.row_stride = L.pitch;
    s.n = 1, s.rows = rows, s.cols = cols;
    s.r0 = r0, s.H = L.h, s.c0 = c0, s.W = L.w;
    s.w0 = 0, s.gwords = L.nw, s.fw = L.nw;
    return s;
}

static void test_board(i64 h, i64 w, i64 r0, i64 c0, i64 rows, i64 cols) {
    const Layout L(h, w, 3);
    const std::vector<u64> buf = random_buffer(L, (u64)(h * 1000 + w));
    const CellSource s = board_source(buf, L, r0, c0, rows, cols);
    for (CellType t : kTypes) {
        const size_t guard = 16;
        std::vector<u8> out((size_t)(rows * cols * cell_size(t)) + 2 * guard, 0xA5);
        unpack_cells_host(s, CellBuffer{out.data() + guard, t, rows * cols});
        bool ok = true;
        for (i64 i = 0; i < rows && ok; ++i)
            for (i64 j = 0; j < cols; ++j) {
                const u64* row = buf.data() + L.index((r0 + i) % h, 0);
                const u32 want = cell_of(row, (c0 + j) % w) ? cell_one(t) : 0u;
                u32 got = 0;
                std::memcpy(&got, out.data() + guard + (size_t)((i * cols + j) * cell_size(t)), (size_t)cell_size(t));
                if (got != want) {
                    ok = false;
                    break;
                }
            }
        CHECK(ok);
        for (size_t g = 0; g < guard; ++g) CHECK(out[g] == 0xA5 && out[out.size() - 1 - g] == 0xA5);
        // one element too few, one too many: refused
        CHECK(throws([&] { unpack_cells_host(s, CellBuffer{out.data() + guard, t, rows * cols - 1}); }));
        CHECK(throws([&] { unpack_cells_host(s, CellBuffer{out.data() + guard, t, rows * cols + 1}); }));
    }
}

// film frames as film.hpp packs them, against FilmGeo::unpack_row
static void test_film(i64 H, i64 W, FilmRect rect, i64 n) {
    const FilmGeo g(rect, H, W);
    std::vector<u64> frames((size_t)(n * g.slot_words()));
    for (size_t i = 0; i < frames.size(); ++i) frames[i] = mix64(77 + i);
    CellSource s;
    s.base = frames.data(), s.words = (i64)frames.size();
    s.frame_stride = g.slot_words(), s.row_stride = g.fw;
    s.n = n, s.rows = g.rows, s.cols = g.cols;
    s.r0 = 0, s.H = g.rows, s.c0 = g.c0, s.W = g.W;
    s.w0 = g.w0, s.gwords = g.gwords, s.fw = g.fw;
    std::vector<u8> ref((size_t)(n * g.rows * g.cols));
    for (i64 r = 0; r < n * g.rows; ++r) g.unpack_row(frames.data() + r * g.fw, ref.data() + r * g.cols);
    for (CellType t : kTypes) {
        std::vector<u8> out(ref.size() * (size_t)cell_size(t));
        unpack_cells_host(s, CellBuffer{out.data(), t, (i64)ref.size()});
        bool ok = true;
        for (size_t i = 0; i < ref.size() && ok; ++i) ok = element(out, t, (i64)i) == (ref[i] ? cell_one(t) : 0u);
        CHECK(ok);
    }
    CellSource bad = s;
    bad.words -= 1;
    std::vector<u8> out(ref.size());
    CHECK(throws([&] { unpack_cells_host(bad, CellBuffer{out.data(), CellType::U8, (i64)ref.size()}); }));
}

static void test_soups(i64 S, i64 n, i64 first, i64 count) {
    const i64 M = S / 64, wps = S * M;
    std::vector<u64> store((size_t)(n * wps));
    for (size_t i = 0; i < store.size(); ++i) store[i] = mix64(5 + i);
    CellSource s;
    s.base = store.data() + first * wps, s.words = count * wps;
    s.frame_stride = wps, s.row_stride = M;
    s.n = count, s.rows = S, s.cols = S;
    s.r0 = 0, s.H = S, s.c0 = 0, s.W = S;
    s.w0 = 0, s.gwords = M, s.fw = M;
    for (CellType t : kTypes) {
        std::vector<u8> out((size_t)(count * S * S * cell_size(t)));
        unpack_cells_host(s, CellBuffer{out.data(), t, count * S * S});
        bool ok = true;
        for (i64 q = 0; q < count * S && ok; ++q)
            for (i64 j = 0; j < S; ++j)
                if (element(out, t, q * S + j) != (cell_of(store.data() + (first * S + q) * M, j) ? cell_one(t) : 0u)) ok = false;
        CHECK(ok);
        // and back: packing the elements gives the store's words
        std::vector<u64> back((size_t)(count * wps), ~0ull);
        CellTarget tg;
        tg.base = back.data(), tg.words = (i64)back.size(), tg.row_stride = M, tg.rows = count * S, tg.cols = S;
        pack_cells_host(CellBuffer{out.data(), t, count * S * S}, tg);
        CHECK(std::memcmp(back.data(), store.data() + first * wps, back.size() * sizeof(u64)) == 0);
    }
}

static uint16_t half_bits(float f) {  // the few values used here: exact in f16
    if (f == 0.0f) return std::signbit(f) ? 0x8000u : 0u;
    if (f == 2.0f) return 0x4000u;
    if (f == -1.0f) return 0xBC00u;
    if (f == 0.5f) return 0x3800u;
    if (f == 1.0f) return 0x3C00u;
    return 0x7E00u;  // NaN
}
static uint16_t bf16_bits(float f) {
    u32 v;
    std::memcpy(&v, &f, 4);
    return (uint16_t)(v >> 16);
}

// packing into a board buffer: rows of `w` cells with odd values; the words of rows 0 .. h - 1 alone change
static void test_pack(i64 h, i64 w) {
    const Layout L(h, w, 2);
    const float odd[] = {0.0f, 1.0f, 2.0f, -1.0f, 0.5f, -0.0f, NAN};
    const int alive[] = {0, 1, 1, 1, 1, 0, 1};
    for (CellType t : kTypes) {
        std::vector<u8> in((size_t)(h * w * cell_size(t)));
        std::vector<int> want((size_t)(h * w));
        for (i64 i = 0; i < h * w; ++i) {
            const int k = (int)(mix64((u64)i * 3 + (u64)w) % (t == CellType::U8 ? 3 : 7));
            want[(size_t)i] = alive[k];
            if (t == CellType::U8) {
                in[(size_t)i] = (u8)(k == 2 ? 2 : k);  // 0, 1, 2
            } else if (t == CellType::F32) {
                std::memcpy(in.data() + 4 * i, &odd[k], 4);
            } else {
                const uint16_t v = t == CellType::F16 ? half_bits(odd[k]) : bf16_bits(odd[k]);
                std::memcpy(in.data() + 2 * i, &v, 2);
            }
        }
        std::vector<u64> buf = random_buffer(L, 9), before = buf;
        CellTarget tg;
        tg.base = buf.data() + L.index(0, 0), tg.words = L.words() - L.index(0, 0);
        tg.row_stride = L.pitch, tg.rows = h, tg.cols = w;
        pack_cells_host(CellBuffer{in.data(), t, h * w}, tg);
        bool ok = true, rest = true;
        for (i64 r = -L.R; r < h + L.R; ++r)
            for (i64 c = -1; c <= L.nw; ++c) {
                const size_t at = (size_t)L.index(r, c);
                if (r < 0 || r >= h || c < 0 || c >= L.nw) {
                    rest = rest && buf[at] == before[at];
                    continue;
                }
                u64 nat = 0;
                for (i64 x = 0; x < 64 && 64 * c + x < w; ++x) nat |= (u64)want[(size_t)(r * w + 64 * c + x)] << x;
                ok = ok && buf[at] == split_word(nat);  // (the last word: masked to the row's cells)
            }
        CHECK(ok);
        CHECK(rest);
        CHECK(throws([&] { pack_cells_host(CellBuffer{in.data(), t, h * w - 1}, tg); }));
        CellTarget small = tg;
        small.words -= L.R * L.pitch + L.pitch - L.nw;  // one word short of the last row's last word
        CHECK(throws([&] { pack_cells_host(CellBuffer{in.data(), t, h * w}, small); }));
    }
}

int main() {
    // boards: whole tiles (tail words of 1 and of 63 cells among them), and rectangles across both seams
    const i64 sides[] = {1, 2, 3, 63, 64, 65, 127, 137, 200};
    for (i64 n : sides) test_board(n, n, 0, 0, n, n);
    test_board(137, 200, 0, 0, 137, 200);
    test_board(7, 65, 0, 0, 7, 65);    // a tail word of 1 cell
    test_board(5, 127, 0, 0, 5, 127);  // of 63
    test_board(137, 200, 130, 190, 15, 21);  // rows and columns wrap, through the 8-cell tail word
    test_board(137, 200, 70, 131, 1, 1);
    test_board(50, 3969, 45, 3900, 10, 140);
    test_board(3, 3, 2, 2, 3, 3);
    // film frames: inside a word, across the x seam through the tail word, the whole board from the middle
    test_film(137, 200, FilmRect{true, 30, 70, 9, 5}, 3);
    test_film(137, 200, FilmRect{true, 5, 190, 30, 21}, 2);
    test_film(137, 200, FilmRect{true, 45, 101, 137, 200}, 2);
    test_film(50, 3969, FilmRect{true, 45, 3900, 10, 140}, 2);
    test_film(3, 3, FilmRect{true, 1, 2, 3, 3}, 4);
    test_film(65, 65, FilmRect{true, 0, 64, 65, 65}, 2);
    // soup stores
    test_soups(64, 5, 1, 3);
    test_soups(128, 3, 0, 3);
    test_soups(256, 2, 1, 1);
    // packing
    for (i64 w : {(i64)1, (i64)63, (i64)64, (i64)65, (i64)127, (i64)200}) test_pack(5, w);
    // a misaligned pointer, an unknown type code
    {
        const Layout L(4, 64, 1);
        const std::vector<u64> buf = random_buffer(L, 1);
        std::vector<u8> out(4 * 64 * 4 + 8);
        const CellSource s = board_source(buf, L, 0, 0, 4, 64);
        u8* odd = out.data() + (((uintptr_t)out.data() & 1u) ? 0 : 1);
        CHECK(throws([&] { unpack_cells_host(s, CellBuffer{odd, CellType::F32, 4 * 64}); }));
        CHECK(throws([&] { unpack_cells_host(s, CellBuffer{odd, CellType::F16, 4 * 64}); }));
        unpack_cells_host(s, CellBuffer{odd, CellType::U8, 4 * 64});
        CHECK(throws([] { cell_type_from_code(4); }));
        CHECK(cell_type_from_code(2) == CellType::BF16);
    }
    printf("gol_tensor_unit: %d checks passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
