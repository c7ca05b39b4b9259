// gol-mi355x: life-like rules (outer-totalistic, radius 1, two states) on the Moore, von Neumann or hexagonal
// neighbourhood.
//
// A rule is two 9-bit masks and a neighbourhood: bit c (0..8) of `birth` / `survive` says that a dead / live
// cell with c live neighbours is alive in the next generation.  Conway's Life is B3/S23 = {0x008, 0x00C}.
// The neighbours counted, as 3 x 3 masks around the centre (rows downward, columns rightward):
//   Moore (no suffix)   von Neumann (V)   hexagonal (H: the square-grid emulation without NE and SW)
//       1 1 1               0 1 0             1 1 0
//       1 . 1               1 . 1             1 . 1
//       1 1 1               0 1 0             0 1 1
//
// Generations rules (B/S/C) add dying states: `states` = C in 3..9 (2: the life-like rule).  State 0 is dead, state 1
// alive and states 2 .. C-1 dying: a live cell that does not survive becomes 2, a dying cell s becomes s + 1 whatever
// its neighbours do, C-1 becomes 0; only state 1 counts as a neighbour and only state 0 can be born.  Moore only.
//
// B0 rules are refused: with B0 the infinite dead background comes alive, and the engine's zeroed slack
// rows, trash lanes and masked tail bits all assume that dead stays dead where nothing is stored.
#pragma once

#include <string>

#include "gol/common.hpp"

namespace gol {

using u16 = uint16_t;

enum class Nbhd : u16 { Moore = 0, VonNeumann = 1, Hex = 2 };

// The largest neighbour count of a neighbourhood: 8, 4, 6.
constexpr int nbhd_max_count(Nbhd n) { return n == Nbhd::VonNeumann ? 4 : (n == Nbhd::Hex ? 6 : 8); }
// The rule-string suffix: "", "V", "H".
constexpr const char* nbhd_suffix(Nbhd n) { return n == Nbhd::VonNeumann ? "V" : (n == Nbhd::Hex ? "H" : ""); }
const char* nbhd_name(Nbhd n);  // "Moore", "von Neumann", "hexagonal"

struct Rule {
    u16 birth = 1u << 3;
    u16 survive = (1u << 2) | (1u << 3);
    Nbhd nbhd = Nbhd::Moore;
    u16 states = 2;  // C of a Generations rule (3..9); 2: two states, the life-like rule

    static constexpr int kMaxStates = 9;
    bool generations() const { return states > 2; }
    // The planes of the decay counter d = state - 1 of a dying cell (0 otherwise), 0 .. C-2: bit_width(C-2); 0 for C = 2.
    int decay_planes() const { return states <= 2 ? 0 : (states == 3 ? 1 : (states <= 5 ? 2 : 3)); }

    // "B<digits>/S<digits>[V|H]" or "S<digits>/B<digits>[V|H]" (letters in either case, digits without repeats
    // from 0 to the neighbourhood's largest count -- 8, V: 4, H: 6 --, either list may be empty), or an alias:
    // conway, life, highlife, daynight, seeds, replicator.  A Generations rule adds a third field: "B<digits>/S<digits>/C<n>",
    // "S<digits>/B<digits>/C<n>" or the bare "<survive digits>/<birth digits>/<n>" (the S/B/C order of the bare form is the
    // common one for these rules: Star Wars is 345/2/4), n from 2 to 9 without leading zeros, C2 being the two-state
    // rule; no V or H suffix.  Throws gol::Error naming the string on anything else, and on every rule with B0.
    static Rule parse(const std::string& s);
    // Masks -> rule, with the same range and B0 checks as parse (bindings, checkpoints).  Two arguments: Moore.
    static Rule from_masks(unsigned birth, unsigned survive);
    static Rule from_masks(unsigned birth, unsigned survive, Nbhd nbhd);
    static Rule from_masks(unsigned birth, unsigned survive, Nbhd nbhd, unsigned states);  // states 2..9; above 2 Moore only
    // code() -> rule, checked as from_masks.
    static Rule from_code(u32 code);
    // Canonical form: B<digits>/S<digits>, digits ascending, then V or H (nothing for Moore), or /C<n> for n > 2.
    std::string str() const;
    bool is_conway() const {
        return birth == (1u << 3) && survive == ((1u << 2) | (1u << 3)) && nbhd == Nbhd::Moore && states == 2;
    }
    // birth | neighbourhood << 12 | survive << 16 (checkpoint header, rank agreement).  The neighbourhood lies in
    // bits no Moore code has set: a code written before there were neighbourhoods reads as Moore.  states - 2 lies in
    // bits 28..30, which no two-state code has set (and which a reader from before refuses as a survive mask).
    u32 code() const { return (u32)birth | ((u32)nbhd << 12) | ((u32)survive << 16) | ((u32)(states - 2) << 28); }
    bool operator==(const Rule& o) const {
        return birth == o.birth && survive == o.survive && nbhd == o.nbhd && states == o.states;
    }
    bool operator!=(const Rule& o) const { return !(*this == o); }
};

}  // namespace gol
