// gol-mi355x: dense cells <-> packed words -- what the tensor readers and writers share (engine.hpp, soups.hpp).
//
// A CellBuffer is a caller's dense buffer of numel elements, one per cell, in one of four element types (torch.bool
// and torch.uint8 are both U8).  Unpacking writes the exact values 0 and 1 of the type (f16 0x3C00, bf16 0x3F80,
// f32 0x3F800000); packing takes a cell as alive iff its element != 0, so -0.0 is dead and NaN is alive.
//
// One source description, CellSource, covers the three packed layouts in the split word format (bits.hpp):
//   the board or envelope buffer   base = word 0 of tile row 0, row_stride = the pitch; a rectangle may wrap (r0, c0);
//   the film slot buffer           n packed frames of rows x fw words, word f of a frame row = board word
//                                  (w0 + f) mod gwords (gol/film.hpp: what FilmGeo::unpack_row reads on the host);
//   the soup store                 n x S rows of S / 64 words, dense.
// Output element (k, i, j) of the (n, rows, cols) result is cell (c0 + j) mod W of source row (r0 + i) mod H of frame k.
// Only cells below W are read, so the ghost cells of a tile's last word never reach the output.
//
// The HIP backends run these conversions on the device (src/hip/tensor_kernels.hip) from the same descriptions; the
// host loops here are the CPU backends' and the oracle of build/gol_tensor_unit.
#pragma once

#include "gol/common.hpp"

namespace gol {

enum class CellType : int { U8 = 0, F16 = 1, BF16 = 2, F32 = 3 };

struct CellBuffer {
    void* ptr = nullptr;
    CellType type = CellType::U8;
    i64 numel = 0;
};

inline i64 cell_size(CellType t) { return t == CellType::U8 ? 1 : (t == CellType::F32 ? 4 : 2); }
inline const char* cell_type_name(CellType t) {
    switch (t) {
        case CellType::U8: return "u8";
        case CellType::F16: return "f16";
        case CellType::BF16: return "bf16";
        default: return "f32";
    }
}
// the element that stands for a live cell, in the low bits
inline u32 cell_one(CellType t) {
    switch (t) {
        case CellType::U8: return 1u;
        case CellType::F16: return 0x3C00u;
        case CellType::BF16: return 0x3F80u;
        default: return 0x3F800000u;
    }
}
CellType cell_type_from_code(int code);  // throws Error naming a code outside 0 .. 3

struct CellSource {
    const u64* base = nullptr;  // source word 0 of source row 0 of frame 0
    i64 words = 0;              // words the caller owns from base on (the checks below keep every read inside)
    i64 frame_stride = 0, row_stride = 0;  // words from frame to frame, row to row
    i64 n = 1, rows = 0, cols = 0;         // the output: (n, rows, cols) cells
    i64 r0 = 0, H = 0;                     // output row i is source row (r0 + i) mod H
    i64 c0 = 0, W = 0;                     // output column j is cell (c0 + j) mod W of the row
    i64 w0 = 0, gwords = 0, fw = 0;        // cell c lies in source word ((c >> 6) - w0) mod gwords, which is < fw
    i64 cells() const { return n * rows * cols; }
};

struct CellTarget {
    u64* base = nullptr;  // word 0 of row 0
    i64 words = 0;        // words the caller owns from base on
    i64 row_stride = 0;   // words from row to row
    i64 rows = 0, cols = 0;  // the input: (rows, cols) cells; ceil(cols / 64) words of every row are written, the last
                             // one masked to the row's cells
    i64 cells() const { return rows * cols; }
};

// Throw Error (naming `what` and the offending value) unless the description is consistent, every word it reaches lies
// inside [base, base + words), the buffer holds exactly cells() elements and its pointer is aligned to its element.
void check_cells(const CellSource& s, const CellBuffer& b, const char* what);
void check_cells(const CellTarget& t, const CellBuffer& b, const char* what);

// The host conversions (both pointers host memory): word by word, a run of cells at a time.
void unpack_cells_host(const CellSource& s, const CellBuffer& dst);
void pack_cells_host(const CellBuffer& src, const CellTarget& t);

}  // namespace gol
