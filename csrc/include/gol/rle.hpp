// gol-mi355x: run-length-encoded pattern files (the RLE format of Golly and LifeWiki).
//
//   #C a comment
//   x = 3, y = 3, rule = B3/S23
//   bob$2bo$3o!
//
// The body is a list of runs <count><tag>: b = dead cells, o = live cells, $ = end of row (a counted $
// skips rows), ! = end of pattern; a missing count is 1.  Line breaks and blanks may fall anywhere between
// the runs, rows shorter than x are dead-padded, rows missing at the end are dead, and whatever follows
// the ! is ignored.
//
// The rule field may end in a topology suffix, as Golly writes it for a bounded grid:
//   rule = B3/S23:P200,100     a plane of 200 columns x 100 rows: cells beyond its edges are dead
//   rule = B3/S23:T200,100     a torus of the same size;  one number (:P64) means a square board
// Infinite dimensions (a 0), shifted or twisted edges (+n, -n, *) and the topologies K, C and S (Klein
// bottle, cross-surface, sphere) are refused, naming the suffix.
#pragma once

#include <string>
#include <vector>

#include "gol/common.hpp"

namespace gol {

struct RlePattern {
    i64 rows = 0, cols = 0;
    std::string rule;        // canonical (B3/S23), without the topology suffix; "" when the header has none
    std::string topology;    // "" (the header has no suffix), "T" torus or "P" plane (dead edges)
    i64 bound_cols = 0, bound_rows = 0;  // the suffix's board (0 without one)
    std::vector<u64> words;  // rows x ceil(cols/64) natural-order words (bit b of word c = column 64c+b)

    i64 nw() const { return ceil_div(cols, 64); }
    bool cell(i64 r, i64 c) const { return (words[(size_t)(r * nw() + (c >> 6))] >> (c & 63)) & 1ull; }
    void set(i64 r, i64 c) { words[(size_t)(r * nw() + (c >> 6))] |= 1ull << (c & 63); }
};

// Largest pattern the reader accepts (cells); a header beyond it is refused before anything is allocated.
constexpr i64 kRleMaxCells = (i64)1 << 34;

// Throws gol::Error naming the offending character and its offset on: a missing header, a run that passes
// x or y, an unknown tag, a count overflow, a missing '!'.  The header's rule goes through Rule::parse; the
// S/B form Golly writes for it (23/3) is accepted here as well.
RlePattern parse_rle(const std::string& text);
// The topology suffix of a header's rule field: "B3/S23:P200,100" -> rule "B3/S23", topology "P", 200 x 100.
// A field without ':' comes back whole, with no topology.  Throws gol::Error naming the suffix on anything
// but :T<w>[,<h>] and :P<w>[,<h>] with w, h >= 1.
struct RleTopology {
    std::string rule;      // the field before the ':' (not parsed here)
    std::string topology;  // "", "T" or "P"
    i64 cols = 0, rows = 0;
};
RleTopology split_rule_topology(const std::string& field);
// Canonical header (with the rule when the pattern has one, and its topology suffix when that is set), no trailing dead cells in a row, no trailing
// dead rows, lines of at most 70 characters, a final '!'.
std::string write_rle(const RlePattern& p);

RlePattern read_rle_file(const std::string& path);
void write_rle_file(const std::string& path, const RlePattern& p);

}  // namespace gol
