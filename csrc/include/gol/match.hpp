// gol-mi355x: pattern matching on the packed board -- templates, their orientations and the host matcher.
//
// A template is two equal-shape 0/1 arrays, `value` and `care`, of th x tw cells (1 <= th, tw <= 32), and a ring
// width `ring` >= 0 with 2 ring < min(th, tw); value <= care cell by cell, and at least one care cell is set.  Its
// origin is the template cell (ring, ring).  It matches at board cell (r, c) when, for every template cell (i, j) with
// care[i][j] = 1, board cell (r - ring + i, c - ring + j) equals value[i][j]: on the torus the coordinates wrap, on a
// bounded board the cells outside it are dead.  Only board cells are candidate positions.
//
// A template built from a pattern with margin m is the pattern padded by m dead cells on every side, care all ones,
// ring = m: a match means the pattern sits there with m dead cells around it, and the reported position is the board
// cell under the pattern's first cell.
//
// Orientations 0..3 are the template turned clockwise by 0, 90, 180, 270 degrees, 4..7 the same four turns of its
// left-right mirror image; value and care turn together and ring stays.
//
// The host matcher below is the CPU backends' implementation (engine and soup batches) and the oracle of
// build/gol_match_unit; the HIP backends run k_match (src/hip/match_kernel.hip) from the same MatchTemplate.
#pragma once

#include <utility>
#include <vector>

#include "gol/common.hpp"
#include "gol/rle.hpp"

namespace gol {

constexpr int kMatchMaxSide = 32;

struct MatchTemplate {
    i32 th = 0, tw = 0, ring = 0;
    u32 care[kMatchMaxSide] = {};   // per template row: bit j = column j is constrained
    u32 value[kMatchMaxSide] = {};  // per template row: bit j = column j must be alive (a subset of care)

    // The pattern padded by `margin` dead cells on every side, care all ones, ring = margin.  Throws Error naming the
    // offending value on a negative margin and on a padded shape over 32 x 32.
    static MatchTemplate from_pattern(const RlePattern& p, i64 margin);
    // From th x tw bytes each (row after row, != 0 is set).  Throws on a shape outside 1..32; validate() does the rest.
    static MatchTemplate from_cells(const u8* value, const u8* care, i64 th, i64 tw, i64 ring);

    bool cell_care(int i, int j) const { return (care[i] >> j) & 1u; }
    bool cell_value(int i, int j) const { return (value[i] >> j) & 1u; }
    bool operator==(const MatchTemplate& o) const;

    // Orientation k (0..7) of this template.
    MatchTemplate oriented(int k) const;
    // (id, template) of orientation 0 alone, or of all eight without those equal to one of a lower id.
    std::vector<std::pair<int, MatchTemplate>> orientations(bool all) const;

    // Throws Error naming the offending value: a shape outside 1..32, no care cell, a value cell outside care,
    // ring < 0 or 2 ring >= min(th, tw), and (H, W > 0) th > H or tw > W.
    void validate(i64 H = 0, i64 W = 0) const;
};

// Host matcher.  words: h rows of nw = ceil(w / 64) natural-order words (bit b of word c = column 64 c + b), cells at
// columns >= w clear.  out (h * nw words, may be nullptr): bit b of word c of row r set iff the template matches at
// (r, 64 c + b); with or_into the matches are ORed into what out holds.  Returns the number of matches.
u64 match_host(const u64* words, i64 h, i64 w, bool torus, const MatchTemplate& t, u64* out, bool or_into = false);
// The set bits of a match_host bitmap as (row, col) pairs in row-major order, at most max_hits of them.
void match_positions_host(const u64* bitmap, i64 h, i64 w, i64 max_hits, std::vector<i32>* out);

}  // namespace gol
