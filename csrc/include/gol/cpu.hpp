// gol-mi355x: CPU backend — bit-packed stepper, halo helpers, init and I/O on host memory.
//
// This is both the GPU-less plumbing backend (BASELINE config 1: 256^2 x 100 gens on the CPU) and
// the C++ oracle for the HIP kernels.  It implements exactly the same temporal-blocking semantics
// as the GPU kernel: a superstep of k generations reads k ghost rows above and below the tile and
// the ghost words beside it, and the ghost area is evolved redundantly (shrinking by one row per
// generation) so no exchange is needed inside the superstep.
#pragma once

#include "gol/density_film.hpp"
#include "gol/film.hpp"
#include "gol/geometry.hpp"
#include "gol/pattern.hpp"
#include "gol/rule.hpp"

namespace gol {
namespace cpu {

// The board's boundary and the tile's place on the global board (what a bounded step needs to know which of
// the cells it sees lie outside the board).  The default is the torus, where the place is not used.
struct Edges {
    Boundary boundary = Boundary::Torus;
    i64 row0 = 0;   // global row of tile row 0
    i64 rows = 0;   // rows of the global board (H)
    i64 word0 = 0;  // global word index of tile word 0
    i64 cols = 0;   // columns of the global board (W)

    Edges() = default;
    Edges(Boundary b, const Geometry& g) : boundary(b), row0(g.row0), rows(g.dec.H), word0(g.word0()), cols(g.dec.W) {}
    bool dead() const { return boundary == Boundary::Dead; }
};

// Boundary::Dead: clear every cell of rows [r_lo, r_hi) (words -1 .. nw) that lies outside the global board:
// whole rows whose global row is outside [0, H), words whose global index is outside [0, ceil(W / 64)), and the
// bits past column W of the board's last word.  (No-op on the torus.)
void mask_rows(u64* buf, const Layout& L, i64 r_lo, i64 r_hi, const Edges& edges);

// One generation for rows [r_lo, r_hi) (all words -1 .. nw) of `dst` from `src`.  B3/S23 runs the
// specialised gates (bits.hpp rule64); any other rule a generic bit-sliced path (4-plane count, then
// next = x ? S[count] : B[count] from the rule's masks), chosen once per call.  On a bounded board the
// output rows are masked (mask_rows); the caller masks the input.
void step_rows(const u64* src, u64* dst, const Layout& L, i64 r_lo, i64 r_hi, const Rule& rule = Rule(),
               const Edges& edges = Edges());

// k generations (k <= L.R).  Ping-pongs between a and b; returns the buffer with the result.  On a bounded
// board the input rows [-k, h + k) of `a` are masked in place first (the ghost rows and words hold what the
// torus machinery delivered across the board's edges), then every generation's output.
// counts (census; k slots, or null): counts[g] += the live cells of the tile itself after generation g + 1: rows
// [0, h), words [0, nw) under the storage mask, no ghost row or word.
// sigs (signature mode; k slots, or null): sigs[g] += the tile's share of the board signature (gol/signature.hpp)
// after generation g + 1, over the same cells, keyed by edges.row0 and edges.word0 (the tile's place; needed on the
// torus too).
// film (film mode; frames == nullptr: none): frames + g * geo->slot_words() is the packed frame (gol/film.hpp) after
// generation g + 1: the tile's own words (the same cells) that are words of the window are OR-ed into their place,
// found from edges.row0 and edges.word0; the words of other tiles are left as they are.
struct FilmOut {
    const FilmGeo* geo = nullptr;
    u64* frames = nullptr;  // k frames
};
// density (density-film mode; maps == nullptr: none): maps + g * geo->slot_words() is the slot (gol/density_film.hpp)
// after generation g + 1: the live cells of the tile's own words (the same cells) are added to the counts of their
// blocks of the global board, found from edges.row0 and edges.word0.
struct DensityOut {
    const DensityGeo* geo = nullptr;
    u64* maps = nullptr;  // k slots
};
u64* superstep(u64* a, u64* b, const Layout& L, int k, const Rule& rule = Rule(), const Edges& edges = Edges(),
               u64* counts = nullptr, u64* sigs = nullptr, const FilmOut& film = FilmOut(),
               const DensityOut& density = DensityOut(), u64* envelope = nullptr, i64 plane_stride = 0);
// Generations rules (rule.states > 2, gol/rule.hpp): a and b hold 1 + M planes in layout L, plane_stride >= L.words()
// words apart: plane 0 the live cells (state 1), planes 1 .. M the bits of the decay counter d = state - 1 of the dying
// cells, M = rule.decay_planes().  Every plane is masked, stepped and extended like the live plane (the decay counter of a
// ghost row is needed: a dying cell there cannot be born); no cell is alive and dying.  counts, sigs, film, density and
// envelope must be off.  state_counts: counts[s] += the tile's own cells in state s, s = 0 .. rule.states - 1.
void state_counts(const u64* buf, const Layout& L, i64 plane_stride, const Rule& rule, u64* counts);
// Larger than Life rules (rule.range > 0, gol/rule.hpp): superstep steps one generation at a time, any k >= 1, on a tile
// that is the whole board (one rank: edges.row0 and word0 are 0, a bounded board's size is the tile's) of at least
// 2 range + 1 cells either way.  It reads the tile's own cells only (the torus by indexing, a bounded board by zeros
// around it) and writes rows [0, h) whole, ghost words zero.  Row-wise sums over unpacked cells: an oracle, not fast.
// counts, sigs, film, density and envelope must be off.
// envelope (envelope mode; nullptr: none): a buffer in layout L; after every generation the tile's own cells (rows
// [0, h), words [0, nw), storage mask on the last word) are ORed into it.  envelope_or does that for one board.
void envelope_or(u64* envelope, const u64* board, const Layout& L);

// x-periodic ghost words (and tail ghost bits) for rows [r_lo, r_hi).
void fill_ghost_cols_wrap(u64* buf, const Layout& L, i64 r_lo, i64 r_hi);
// y-periodic ghost rows of a tile that is its own vertical neighbour (any h, even h < R).
void fill_ghost_rows_wrap(u64* buf, const Layout& L);

// Initialise the tile from a pattern (ghost area zeroed; caller refreshes halos).
void init_tile(u64* buf, const Layout& L, const Geometry& g, const PatternSpec& p);

// Dense, masked copy of the tile words (h * nw), and the reverse.
void extract_words(const u64* buf, const Layout& L, u64* dense);
void insert_words(u64* buf, const Layout& L, const u64* dense);

// Live-cell count and decomposition-invariant fingerprint of the tile.
u64 population(const u64* buf, const Layout& L);
u64 fingerprint(const u64* buf, const Layout& L, i64 grow0, i64 gword0, i64 gwords);
// The tile's share of the board signature (gol/signature.hpp): rows [0, h), words [0, nw) under the storage mask.
u64 signature(const u64* buf, const Layout& L, i64 grow0, i64 gword0);

}  // namespace cpu
}  // namespace gol
