// gol-mi355x: connected components of the live board -- labels, per-object records and the orientation-free hash.
//
// Neighbourhoods: von_neumann (|dr| + |dc| = 1), moore (Chebyshev distance 1), moore2 (Chebyshev distance <= 2: two
// live cells this close share a neighbour, the pseudo-object notion).  Two live cells are joined when one lies in the
// other's neighbourhood; a component is a class of the transitive closure.  On the torus the coordinates wrap (every
// board of a batch is its own torus), on a bounded board nothing lies outside.
//
// Per component:
//   anchor      its first cell in row-major order; the label of its cells is 1 + row * W + col of the anchor (dead: 0);
//   population  its cells;
//   bbox        (r0, c0, rows, cols).  Bounded board: the plain extents.  Torus, per axis of length L: the extents of the
//               coordinate x and of (x + L / 2) mod L are taken, the frame with the smaller extent is kept (the plain
//               one on a tie), and r0 / c0 is reported in board coordinates, so r0 + rows may exceed H.  A component
//               whose cyclic extent is at most L / 2 gets its true box (such an interval cannot cross both seams);
//   hash        with A the component's cells inside its box (rows x cols), A_k its orientation k (0..3 clockwise quarter
//               turns, 4..7 the same turns of the left-right mirror image, as gol/match.hpp turns a template) and
//               h_k = sum over the live (i, j) of A_k of (u64) sig_rho(i) * (u64) sig_gam(j) mod 2^64
//               (gol/signature.hpp): hash = min over k of h_k.  It is the same for all eight orientations and under
//               translation.
// Objects are sorted by (board, anchor row, anchor col).
//
// The raw record (CcRecord, 8 extents and 8 orientation sums) is what both implementations produce -- the host one below
// (the CPU backends, and the oracle of build/gol_components_unit's device-shaped checks) and the kernels of
// src/hip/components_kernel.hip -- and cc_finish() turns raw records into the result.
#pragma once

#include <string>
#include <vector>

#include "gol/bits.hpp"
#include "gol/common.hpp"
#include "gol/signature.hpp"

namespace gol {

enum class CcNeighbourhood : int { VonNeumann = 0, Moore = 1, Moore2 = 2 };
// "von_neumann" | "moore" | "moore2"; throws Error naming anything else.
CcNeighbourhood cc_neighbourhood(const std::string& name);
const char* cc_neighbourhood_name(CcNeighbourhood nb);

// One object as both implementations accumulate it: the anchor's cell index inside the batch (board * H * W +
// row * W + col), the population, and the minima and maxima of row, column, (row + H / 2) mod H, (col + W / 2) mod W.
struct CcRecord {
    i32 root;
    u32 pop;
    i32 ext[8];  // rmin, rmax, cmin, cmax, then the same four of the shifted frame
};
static_assert(sizeof(CcRecord) == 40, "the kernels address a record as ten 32-bit words");

// One axis of the box rule: (first coordinate, extent) from the extents of the plain and of the shifted frame.
BITS_HD void cc_box_axis(i32 mn, i32 mx, i32 mn2, i32 mx2, i64 L, bool torus, i64& x0, i64& len) {
    const i64 e1 = (i64)mx - mn + 1, e2 = (i64)mx2 - mn2 + 1;
    if (!torus || e1 <= e2) {
        x0 = mn, len = e1;
    } else {
        x0 = ((i64)mn2 + L - L / 2) % L, len = e2;
    }
}

// The eight orientation sums' keys of box cell (i, j) of a rows x cols box: orientation k adds
// sig_rho(row_k) * sig_gam(col_k), where with a = i, a' = rows - 1 - i, b = j, b' = cols - 1 - j
//   (row_k, col_k) = (a, b), (b, a'), (a', b'), (b', a), (a, b'), (b', a'), (a', b), (b, a)   for k = 0 .. 7.
BITS_HD void cc_hash_add(u64 h[8], i64 i, i64 j, i64 rows, i64 cols) {
    const u32 a = (u32)i, a2 = (u32)(rows - 1 - i), b = (u32)j, b2 = (u32)(cols - 1 - j);
    const u64 ra = sig_rho(a), ra2 = sig_rho(a2), rb = sig_rho(b), rb2 = sig_rho(b2);
    const u64 ga = sig_gam(a), ga2 = sig_gam(a2), gb = sig_gam(b), gb2 = sig_gam(b2);
    h[0] += ra * gb, h[1] += rb * ga2, h[2] += ra2 * gb2, h[3] += rb2 * ga;
    h[4] += ra * gb2, h[5] += rb2 * ga2, h[6] += ra2 * gb, h[7] += rb * ga;
}

struct ComponentsResult {
    u64 count = 0;                // objects over all boards; always exact
    std::vector<i64> board;       // k: the object's board (0 with one board)
    std::vector<i64> anchor;      // k x 2 (row, col) in the board's own coordinates
    std::vector<u32> population;  // k
    std::vector<i64> bbox;        // k x 4 (r0, c0, rows, cols)
    std::vector<u64> hash;        // k, or empty without hashes
    bool truncated = false;       // count > max_objects: the k = max_objects records are some of the objects
    std::vector<u32> per_board;   // objects of every board (batch counts)
};

// Raw records (k of them, in any order; sums: k x 8 orientation sums or nullptr) into the sorted result.
ComponentsResult cc_finish(const CcRecord* rec, const u64* sums, i64 k, u64 count, i64 h, i64 w, bool torus);

// Throws Error naming the offending value: max_objects < 1, h * w * batch >= 2^31 (labels are 32-bit).
void cc_check(i64 h, i64 w, i64 batch, i64 max_objects, const char* what);

// Host implementation.  words: batch boards of h rows of nw = ceil(w / 64) natural-order words (bit b of word c =
// column 64 c + b), cells at columns >= w clear.  labels (h * w * batch i32, may be nullptr): 1 + row * W + col of the
// anchor of every live cell's component, 0 for a dead cell.  want_records = false fills count and per_board alone.
ComponentsResult components_host(const u64* words, i64 h, i64 w, i64 batch, bool torus, CcNeighbourhood nb, i64 max_objects,
                                 bool hashes, bool want_records, i32* labels);

// The hash of a rows x cols 0/1 array (bytes, != 0 is set) as it stands: its eight orientation sums' minimum.
u64 object_hash_host(const u8* cells, i64 rows, i64 cols);

}  // namespace gol
