// gol-mi355x: dense cells <-> packed words on the host (gol/cells.hpp): the checks both backends run before a
// conversion, and the CPU backends' conversions.
#include "gol/cells.hpp"

#include <algorithm>
#include <cstring>

#include "gol/bits.hpp"

namespace gol {

CellType cell_type_from_code(int code) {
    if (code < 0 || code > 3) throw Error(strprintf("cells: element type code %d is not 0 (u8), 1 (f16), 2 (bf16) or 3 (f32)", code));
    return (CellType)code;
}

namespace {

void check_buffer(const CellBuffer& b, i64 cells, const char* what) {
    if (!b.ptr) throw Error(std::string(what) + ": the cell buffer is a null pointer");
    if ((int)b.type < 0 || (int)b.type > 3) throw Error(strprintf("%s: element type %d is unknown", what, (int)b.type));
    if (b.numel != cells)
        throw Error(strprintf("%s: the buffer holds %lld elements, the cells are %lld", what, (long long)b.numel, (long long)cells));
    if ((uintptr_t)b.ptr % (uintptr_t)cell_size(b.type))
        throw Error(strprintf("%s: the buffer at %p is not aligned to its %lld-byte elements", what, b.ptr, (long long)cell_size(b.type)));
}

}  // namespace

void check_cells(const CellSource& s, const CellBuffer& b, const char* what) {
    if (!s.base || s.n < 1 || s.rows < 1 || s.cols < 1 || s.H < 1 || s.W < 1 || s.rows > s.H || s.cols > s.W || s.r0 < 0 ||
        s.r0 >= s.H || s.c0 < 0 || s.c0 >= s.W || s.frame_stride < 0 || s.row_stride < 1 || s.fw < 1 || s.w0 < 0)
        throw Error(strprintf("%s: %lld x %lld x %lld cells at (%lld, %lld) of %lld x %lld is no rectangle of the source", what,
                              (long long)s.n, (long long)s.rows, (long long)s.cols, (long long)s.r0, (long long)s.c0,
                              (long long)s.H, (long long)s.W));
    // the source words the columns reach, as FilmGeo counts them: w0 .. the last column's word, or round the seam
    const i64 gwords = ceil_div(s.W, 64), last = s.c0 + s.cols - 1;
    if (s.gwords != gwords || (s.w0 != 0 && s.w0 != (s.c0 >> 6)))
        throw Error(strprintf("%s: word %lld of %lld does not start the columns from %lld on (rows of %lld words)", what,
                              (long long)s.w0, (long long)s.gwords, (long long)s.c0, (long long)gwords));
    const i64 need = last < s.W ? (last >> 6) - s.w0 + 1 : std::min(gwords, gwords - s.w0 + ((last - s.W) >> 6) + 1);
    if (need > s.fw || s.fw > s.row_stride)
        throw Error(strprintf("%s: the columns reach %lld words of a row, the source has %lld (stride %lld)", what,
                              (long long)need, (long long)s.fw, (long long)s.row_stride));
    if ((s.n - 1) * s.frame_stride + (s.H - 1) * s.row_stride + s.fw > s.words)
        throw Error(strprintf("%s: the rectangle reaches word %lld of a source of %lld words", what,
                              (long long)((s.n - 1) * s.frame_stride + (s.H - 1) * s.row_stride + s.fw), (long long)s.words));
    check_buffer(b, s.cells(), what);
}

void check_cells(const CellTarget& t, const CellBuffer& b, const char* what) {
    if (!t.base || t.rows < 1 || t.cols < 1 || t.row_stride < ceil_div(t.cols, 64))
        throw Error(strprintf("%s: %lld x %lld cells in rows of %lld words is no target", what, (long long)t.rows,
                              (long long)t.cols, (long long)t.row_stride));
    if ((t.rows - 1) * t.row_stride + ceil_div(t.cols, 64) > t.words)
        throw Error(strprintf("%s: the rows reach word %lld of a target of %lld words", what,
                              (long long)((t.rows - 1) * t.row_stride + ceil_div(t.cols, 64)), (long long)t.words));
    check_buffer(b, t.cells(), what);
}

namespace {

template <typename E>
void unpack_rows(const CellSource& s, E* out, E one) {
    const i64 total = s.n * s.rows;
#pragma omp parallel for schedule(static) if (total * s.cols > 65536)
    for (i64 q = 0; q < total; ++q) {
        const i64 k = q / s.rows, i = q - k * s.rows;
        const u64* row = s.base + k * s.frame_stride + ((s.r0 + i) % s.H) * s.row_stride;
        E* o = out + q * s.cols;
        for (i64 j = 0; j < s.cols;) {  // the run of columns one source word holds: to its end, the seam or the last column
            const i64 c = (s.c0 + j) % s.W;
            const int b = (int)(c & 63);
            const i64 run = std::min(std::min((i64)64 - b, s.W - c), s.cols - j);
            const u64 nat = merge_word(row[pmod((c >> 6) - s.w0, s.gwords)]) >> b;
            for (i64 x = 0; x < run; ++x) o[j + x] = ((nat >> x) & 1ull) ? one : (E)0;
            j += run;
        }
    }
}

template <typename E>
void pack_rows(const E* in, const CellTarget& t, E sign) {
    const i64 nw = ceil_div(t.cols, 64);
#pragma omp parallel for schedule(static) if (t.rows * t.cols > 65536)
    for (i64 r = 0; r < t.rows; ++r) {
        const E* row = in + r * t.cols;
        for (i64 cw = 0; cw < nw; ++cw) {
            const i64 run = std::min<i64>(64, t.cols - 64 * cw);
            u64 nat = 0;
            for (i64 x = 0; x < run; ++x) nat |= (u64)((E)(row[64 * cw + x] & (E)~sign) != 0) << x;
            t.base[r * t.row_stride + cw] = split_word(nat);
        }
    }
}

}  // namespace

void unpack_cells_host(const CellSource& s, const CellBuffer& dst) {
    check_cells(s, dst, "unpack_cells");
    switch (dst.type) {
        case CellType::U8: return unpack_rows<u8>(s, (u8*)dst.ptr, (u8)1);
        case CellType::F32: return unpack_rows<u32>(s, (u32*)dst.ptr, cell_one(dst.type));
        default: return unpack_rows<uint16_t>(s, (uint16_t*)dst.ptr, (uint16_t)cell_one(dst.type));
    }
}

// (a float element is compared through its bits: everything but the sign bit clear is +0.0 or -0.0, dead)
void pack_cells_host(const CellBuffer& src, const CellTarget& t) {
    check_cells(t, src, "pack_cells");
    switch (src.type) {
        case CellType::U8: return pack_rows<u8>((const u8*)src.ptr, t, (u8)0);
        case CellType::F32: return pack_rows<u32>((const u32*)src.ptr, t, 0x80000000u);
        default: return pack_rows<uint16_t>((const uint16_t*)src.ptr, t, (uint16_t)0x8000u);
    }
}

}  // namespace gol
