// gol-mi355x: host API of step_soups (soup_kernel.hip), the soup-batch kernel for gfx950.
#pragma once

#include <hip/hip_runtime.h>

#include "gol/rule.hpp"
#include "gol/soups.hpp"

namespace gol {
namespace hipk {

enum SoupMode : int { SOUP_PLAIN = 0, SOUP_SETTLE = 1, SOUP_TRANSIENT = 2 };

// Boards: n soups x S rows x m words of split storage; lane l of soup i's wave owns the m * m words from
// (i * 64 + l) * m * m on (rows m l .. m l + m - 1).
struct SoupArgs {
    u64* board;        // every mode
    u64* saved;        // SETTLE: the search's copy; TRANSIENT: the first of the two copies
    const u64* init;   // TRANSIENT: the initial boards
    u64* tmp;          // TRANSIENT: the second copy
    SoupState* state;
    u32* counters;     // [0]: soups settled (SETTLE adds), [1]: settled soups without a transient (TRANSIENT adds)
    u32 n;
    u32 gens;          // generations (TRANSIENT: loop passes) of this launch, per soup
    u32 max_gens;      // SETTLE: no soup passes this generation
};

// One launch: ceil(n / (workgroup / 64)) workgroups of `workgroup` threads (64, 128 or 256), one wave per soup.
void launch_step_soups(int m, SoupMode mode, const Rule& rule, const SoupArgs& a, int workgroup, hipStream_t stream);
// Soup i = pattern 5 of seed + i; states reset (population is set by the next SOUP_PLAIN launch, gens = 0 included).
void launch_init_soups(int m, u64* board, SoupState* state, u32 n, u64 seed, hipStream_t stream);
void launch_reset_soup_states(SoupState* state, u32 n, hipStream_t stream);
// s = g, w = 1 for every soup (the search begins where step() left the boards).
void launch_begin_soup_search(SoupState* state, u32 n, hipStream_t stream);

}  // namespace hipk
}  // namespace gol
