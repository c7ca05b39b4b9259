// gol-mi355x: step_gen<K, M, ROWS, BOUNDED> -- Generations rules (B/S/C, gol/rule.hpp) on the generic streaming wave,
// for gfx950 (CDNA4).
//
// A cell of a Generations rule is dead (0), alive (1) or dying (2 .. C - 1).  The board is 1 + M planes in one layout,
// plane_stride words apart: the live plane, which is the two-state board of the other kernels, and the M = bit_width(C - 2)
// planes of the decay counter d = state - 1 of the dying cells (0 elsewhere).  Only live cells count as neighbours, so
// the runner's ring, horizontal sums and rule gates run on the live plane as they are; what a level adds is per cell:
//     R   the gates' output (birth and survival as if every cell that is not alive were dead)
//     A   the row's live cells at the previous level, d its counter there
//     A' = R & ~any(d)                                          a dying cell is not born
//     d' = (A & ~R) ? 1 : (any(d) & d != C - 2 ? d + 1 : 0)       decay starts, goes on, or ends
// C is a kernel argument: d is compared with uniform all-ones / all-zeros words for the bits of C - 2, the increment is a
// ripple over the M planes, all in v_bitop3_b32 (generations_policy.hpp: half()).
//
// The chain.  Level l outputs in row iteration i the row whose previous-level value level l - 1 output one iteration
// earlier, so A and d travel from level to level with the envelope chains' delay (envelope_kernel.hip): level l - 1
// hands (A', d') on as nxt[l], level 0 moves nxt to cur at the start of every iteration, level l reads cur[l]:
// 2 + 2 M values per level live across the iterations.  (A is the value the ring holds as the level's centre row; it
// is carried here because a policy does not see the ring, and the compiler merges the two.)  A level is first called
// in iteration 2 l + 2 and finds what level l - 1 made in iteration 2 l + 1, which was called (2 l + 1 >= 2 l), as in
// step_envelope.  Level 0's row is the runner's loaded row of the iteration before, with its counter.
//
// The counter's load stream is the policy's own: M loads per row at the runner's addresses in the decay planes (start
// row row0 - K, the ROWS_WRAP select, the lane's col + 1, halo lanes included: a level's births depend on the dying
// cells of the whole footprint), three rows ahead at every depth: the runner's rows and words at a plane's offset, and
// past a segment's last input row at most three rows, within the slack the runner's prefetch requires (INVARIANT
// below).  On a bounded board the loaded counter gets the edge mask like the loaded row, and so do A' and d'.
//
// The last level stores d' into the decay planes of dst where the runner stores the row: every stored row of every
// LANE_STORE lane (a later pass of the superstep reads the extension rows).  Lanes without LANE_STORE store no counter.
//
// INVARIANT, beside the runner's: in planes 1 .. M step_gen writes exactly the rows and words it writes in the live
// plane, and reads the rows and words it reads there, except past a segment's last input row, where it reads at most
// three rows (the runner: three at K >= 5, up to six at K <= 4, and at K <= 4 its tail may stop a row or two short of
// the counter's stream).  Three rows past the last input row lie within the slack rows every plane carries for the
// runner's prefetch, so a plan that validate_plan accepts for a board is safe for its planes, which are allocated like
// the board (the launcher checks that plane_stride covers a board).
//
// Depths: K = 1 .. kGenMaxDepth[M], the deepest at which every instantiation of that M uses neither scratch nor AGPRs
// (docs/PERFORMANCE.md, "Generations rules", has the table).  MASK_UNI / MASK_LANE by one_row0, both row modes.
#include "generations_policy.hpp"
#include "rule_launch.hpp"

namespace gol {
namespace hipk {

namespace {

// By M.  Beyond these the register allocator spills into AGPRs and the kernel drops to one wave per SIMD: M = 2 from
// K = 6 on (step_gen<6, 2, ROWS_GHOST, false>: 256 VGPRs + 8 AGPRs), M = 3 from K = 3 on (<3, 3, ROWS_GHOST, false>: 256 + 10).
// GOL_GEN_KMAX<M> overrides one, for the stand-alone compile of this unit that gives the resource table of every depth
// (tools/README.md) and for nothing else: in a build of the library it would change max_generations_depth() and
// instantiate kernels that need AGPRs and run at one wave per SIMD.
#ifndef GOL_GEN_KMAX1
#define GOL_GEN_KMAX1 8
#endif
#ifndef GOL_GEN_KMAX2
#define GOL_GEN_KMAX2 5
#endif
#ifndef GOL_GEN_KMAX3
#define GOL_GEN_KMAX3 2
#endif
constexpr int kGenMaxDepth[4] = {0, GOL_GEN_KMAX1, GOL_GEN_KMAX2, GOL_GEN_KMAX3};

template <int K, int M, int ROWS, bool BOUNDED>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_gen(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                 const LaneDesc* __restrict__ plan, StepParams p, RuleMasks rm,
                                                                 TileArgs ta, GenArgs ga) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    if (one_row0(d)) {
        RuleRunner<K, ROWS, GenPolicy<K, M, MASK_UNI, BOUNDED, ROWS>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta, src, dst, ga);
        w.run();
    } else {
        RuleRunner<K, ROWS, GenPolicy<K, M, MASK_LANE, BOUNDED, ROWS>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta, src, dst, ga);
        w.run();
    }
}

template <int M>
const void* gen_kernel_of(int k, u32 flags, bool bounded) {
    if (k > kGenMaxDepth[M]) return nullptr;
    return kernel_of(k, flags, [bounded](auto K, auto ROWS) -> const void* {
        if constexpr (K() <= kGenMaxDepth[M])
            return bounded ? (const void*)step_gen<K(), M, ROWS(), true> : (const void*)step_gen<K(), M, ROWS(), false>;
        else
            return nullptr;
    });
}

const void* gen_kernel_of(int planes, int k, u32 flags, bool bounded) {
    return planes == 1 ? gen_kernel_of<1>(k, flags, bounded) : planes == 2 ? gen_kernel_of<2>(k, flags, bounded) : gen_kernel_of<3>(k, flags, bounded);
}

int planes_of(int states) {
    if (states < 3 || states > Rule::kMaxStates)
        throw Error(strprintf("step_gen: %d states; a Generations rule has 3 to %d", states, Rule::kMaxStates));
    return states == 3 ? 1 : (states <= 5 ? 2 : 3);
}

}  // namespace

int max_generations_depth(int states) { return kGenMaxDepth[planes_of(states)]; }

int generations_blocks_per_cu(int k, u32 flags, bool bounded, int states) {
    return blocks_per_cu(gen_kernel_of(planes_of(states), k, flags, bounded));
}

void launch_step_gen(int k, const Rule& rule, const BoardEdges& place, bool bounded, i64 tile_cols, const u64* src, u64* dst,
                     i64 plane_stride, i64 board_words, const LaneDesc* plan, i64 n_waves, const StepParams& p, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_gen has no seam-reading variant (sub-tiles do not run Generations rules)");
    check_rule_masks("step_gen", rule);
    if (rule.nbhd != Nbhd::Moore) throw Error("step_gen: Generations rules count the Moore neighbourhood only");
    const int planes = planes_of((int)rule.states);
    check_place("step_gen", place);
    check_tile_cols("step_gen", tile_cols, p);
    if (board_words < 1 || plane_stride < board_words)
        throw Error(strprintf("step_gen: a plane stride of %lld words does not cover a board allocation of %lld words",
                              (long long)plane_stride, (long long)board_words));
    const void* f = gen_kernel_of(planes, k, p.flags, bounded);
    if (!f)
        throw Error(strprintf("no Generations kernel instantiated for depth %d with %d states (1..%d)", k, (int)rule.states,
                              kGenMaxDepth[planes]));
    const GenArgs ga{plane_stride, (u32)rule.states};
    launch_generic("generations", f, rule, src, dst, plan, n_waves, p, s, tile_args(&place, tile_cols, p), ga);
}

}  // namespace hipk
}  // namespace gol
