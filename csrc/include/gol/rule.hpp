// gol-mi355x: life-like rules (outer-totalistic, radius-1 Moore neighbourhood, two states).
//
// A rule is two 9-bit masks: bit c (0..8) of `birth` / `survive` says that a dead / live cell with c
// live neighbours is alive in the next generation.  Conway's Life is B3/S23 = {0x008, 0x00C}.
//
// B0 rules are refused: with B0 the infinite dead background comes alive, and the engine's zeroed slack
// rows, trash lanes and masked tail bits all assume that dead stays dead where nothing is stored.
#pragma once

#include <string>

#include "gol/common.hpp"

namespace gol {

using u16 = uint16_t;

struct Rule {
    u16 birth = 1u << 3;
    u16 survive = (1u << 2) | (1u << 3);

    // "B<digits>/S<digits>" or "S<digits>/B<digits>" (letters in either case, digits 0..8 without
    // repeats, either list may be empty), or an alias: conway, life, highlife, daynight, seeds,
    // replicator.  Throws gol::Error naming the string on anything else, and on every rule with B0.
    static Rule parse(const std::string& s);
    // Masks -> rule, with the same range and B0 checks as parse (bindings, checkpoints).
    static Rule from_masks(unsigned birth, unsigned survive);
    // Canonical form: B<digits>/S<digits>, digits ascending.
    std::string str() const;
    bool is_conway() const { return birth == (1u << 3) && survive == ((1u << 2) | (1u << 3)); }
    // birth | survive << 16 (checkpoint header, rank agreement)
    u32 code() const { return (u32)birth | ((u32)survive << 16); }
    bool operator==(const Rule& o) const { return birth == o.birth && survive == o.survive; }
    bool operator!=(const Rule& o) const { return !(*this == o); }
};

}  // namespace gol
