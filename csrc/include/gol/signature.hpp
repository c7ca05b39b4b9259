// gol-mi355x: the board signature, a cheap, linear, position-keyed 64-bit hash of the global board.
//
// For a board of H x W cells and G = ceil(W / 64) words per row, with E / O the even / odd 32-bit halves of the
// split storage word (bits.hpp) of global row r and global word c, masked to columns < W:
//     rho(r) = mix32((u32)r ^ 0x9E3779B9) | 1            gam(j) = mix32((u32)j + 0x7F4A7C15) | 1
//     signature = sum over r, c of  E * (rho(r) * gam(2c) mod 2^32) + O * (rho(r) * gam(2c + 1) mod 2^32)   mod 2^64
// each product 32 x 32 -> 64 bits.  A wrapping sum keyed by global coordinates: independent of ranks, grids, plans
// and segment cuts, and cheap enough for the stepping kernel (two 32-bit multiplies and two 64-bit multiply-adds per
// word with the row key wave-uniform and the column keys fixed per lane; signature_kernel.hip).  The key is a
// product of a row key and a column key, not a sum: with a sum, swapping equal bits between the corners of a
// rectangle of words would cancel identically.
#pragma once

#include "gol/bits.hpp"

namespace gol {

BITS_HD u32 sig_mix32(u32 x) {
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}
BITS_HD u32 sig_rho(u32 grow) { return sig_mix32(grow ^ 0x9E3779B9u) | 1u; }  // key of a global row
BITS_HD u32 sig_gam(u32 j) { return sig_mix32(j + 0x7F4A7C15u) | 1u; }        // key of a half word: 2c even, 2c + 1 odd

// Contribution of one (masked) split-storage word at global row `grow`, global word `gword`.
BITS_HD u64 signature_word(i64 grow, i64 gword, u64 split) {
    const u32 rho = sig_rho((u32)grow);
    const u32 ka = rho * sig_gam(2u * (u32)gword), kb = rho * sig_gam(2u * (u32)gword + 1u);
    return (u64)(u32)split * (u64)ka + (u64)(u32)(split >> 32) * (u64)kb;
}

}  // namespace gol
