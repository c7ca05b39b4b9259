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
// Larger than Life rules (LtL) are a family of their own: two states, the box of range R (the (2R+1)^2 cells around a
// cell), birth and survival by count intervals.  Golly writes R5,C0,M1,S34..58,B34..45,NM (Bosco's rule): n is the
// number of live cells in the box, the cell itself counted iff M is 1; a dead cell is born iff bmin <= n <= bmax, a
// live cell survives iff smin <= n <= smax.  R runs from 1 to 7, so that a count fits 8 bit planes ((2*7+1)^2 = 225);
// C is 0 or 2 (history states, C >= 3, are not built), N is M, the box (NN and NC are not built).  `range` > 0 marks
// such a rule: its masks are unused (zero), and it has no code().
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

    // Larger than Life: range R (0: not an LtL rule), the middle flag M and the four interval bounds
    u16 range = 0;
    u16 middle = 0;
    u16 smin = 0, smax = 0, bmin = 0, bmax = 0;

    static constexpr int kMaxStates = 9;
    static constexpr int kMaxRange = 7;
    bool ltl() const { return range > 0; }
    // cells of the box, (2R+1)^2: the largest count
    int box() const { return (2 * (int)range + 1) * (2 * (int)range + 1); }
    bool generations() const { return states > 2; }
    // The planes of the decay counter d = state - 1 of a dying cell (0 otherwise), 0 .. C-2: bit_width(C-2); 0 for C = 2.
    int decay_planes() const { return states <= 2 ? 0 : (states == 3 ? 1 : (states <= 5 ? 2 : 3)); }

    // "B<digits>/S<digits>[V|H]" or "S<digits>/B<digits>[V|H]" (letters in either case, digits without repeats
    // from 0 to the neighbourhood's largest count -- 8, V: 4, H: 6 --, either list may be empty), or an alias:
    // conway, life, highlife, daynight, seeds, replicator.  A Generations rule adds a third field: "B<digits>/S<digits>/C<n>",
    // "S<digits>/B<digits>/C<n>" or the bare "<survive digits>/<birth digits>/<n>" (the S/B/C order of the bare form is the
    // common one for these rules: Star Wars is 345/2/4), n from 2 to 9 without leading zeros, C2 being the two-state
    // rule; no V or H suffix.  A Larger than Life rule is "R<r>,C<c>,M<m>,S<smin>..<smax>,B<bmin>..<bmax>[,N<n>]"
    // (letters in either case, the fields in this order, numbers without leading zeros; r in 1..7, c 0 or 2, m 0 or 1,
    // min <= max <= (2r+1)^2, bmin >= 1, n M or missing) or the alias bosco.  Throws gol::Error naming the string on
    // anything else, and on every rule with B0.
    static Rule parse(const std::string& s);
    // The four bounds -> an LtL rule, with parse's checks (bindings, tests).
    static Rule from_ltl(unsigned range, unsigned middle, unsigned smin, unsigned smax, unsigned bmin, unsigned bmax);
    // Masks -> rule, with the same range and B0 checks as parse (bindings, checkpoints).  Two arguments: Moore.
    static Rule from_masks(unsigned birth, unsigned survive);
    static Rule from_masks(unsigned birth, unsigned survive, Nbhd nbhd);
    static Rule from_masks(unsigned birth, unsigned survive, Nbhd nbhd, unsigned states);  // states 2..9; above 2 Moore only
    // code() -> rule, checked as from_masks.
    static Rule from_code(u32 code);
    // Canonical form: B<digits>/S<digits>, digits ascending, then V or H (nothing for Moore), or /C<n> for n > 2.
    // An LtL rule: all six fields with C0, R5,C0,M1,S34..58,B34..45,NM.
    std::string str() const;
    // LtL: the rule as four thresholds on T, the box sum INCLUDING the centre cell (what the steppers count): a dead
    // cell is born iff blo <= T <= bhi, a live cell survives iff slo <= T <= shi, with slo = smin + 1 - M and
    // shi = smax + 1 - M (a live centre adds one to T, which M = 1 counts anyway), clamped to 0 .. (2R+1)^2.  An
    // interval the clamp would empty (smin + 1 - M above the box) is given as lo = 1, hi = 0, which no T satisfies.
    struct LtlThresholds {
        u16 blo, bhi, slo, shi;
    };
    LtlThresholds ltl_thresholds() const;
    bool is_conway() const {
        return birth == (1u << 3) && survive == ((1u << 2) | (1u << 3)) && nbhd == Nbhd::Moore && states == 2 && range == 0;
    }
    // birth | neighbourhood << 12 | survive << 16 (checkpoint header, rank agreement).  The neighbourhood lies in
    // bits no Moore code has set: a code written before there were neighbourhoods reads as Moore.  states - 2 lies in
    // bits 28..30, which no two-state code has set (and which a reader from before refuses as a survive mask).
    // (An LtL rule has no code: whatever needs one refuses the rule first.)
    u32 code() const { return (u32)birth | ((u32)nbhd << 12) | ((u32)survive << 16) | ((u32)(states - 2) << 28); }
    bool operator==(const Rule& o) const {
        return birth == o.birth && survive == o.survive && nbhd == o.nbhd && states == o.states && range == o.range &&
               middle == o.middle && smin == o.smin && smax == o.smax && bmin == o.bmin && bmax == o.bmax;
    }
    bool operator!=(const Rule& o) const { return !(*this == o); }
};

}  // namespace gol
