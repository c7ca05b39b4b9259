// gol-mi355x: step_envelope<K, ROWS, BOUNDED> -- step_rule / step_rule_bounded that also records every cell that
// was alive in any generation of the pass, for gfx950 (CDNA4).
//
// A temporal-blocked pass keeps generations 1 .. K - 1 in registers only, so the OR over the generations can be
// formed nowhere but here.  The envelope is a third device buffer in the board's own layout (same pitch, halo rows
// and slack rows): the word the runner stores at *st has its envelope word at the same offset.
//
// The chain.  In row iteration i, level l outputs row counter t = i - (l + 1): the K outputs of one row appear in K
// consecutive iterations, one level later each time, so the row's OR travels with it.  Level l computes
//     e = cur[l] | out        cur[l]: what level l - 1 made of the same row one iteration earlier (level 0: e = out)
// and hands e on as nxt[l + 1]; level 0, the first call of every iteration, moves nxt to cur.  (advance() runs the
// levels in ascending order, so level l - 1 overwrites its hand-over before level l has read the old one: hence two
// names per level.  In the unrolled loop the move is renaming: 2 (K - 1) values live across the iterations, and one
// v_or_b32 per word half and level.  The move is made by level 0 and not by the reading level because a level is
// not called while the pipeline fills: level l is first called in iteration 2l + 2 and must then find what level
// l - 1 made in iteration 2l + 1, when nobody read it.)
//
// The last level masks e to the cells the lane owns (OwnMask: owned word, owned row, exactly the census's partition,
// census_kernel.hip) and ORs it into the envelope word: one 64-bit read-modify-write per owned word and row per
// pass.  Lanes that own nothing (halo lanes, trash-slot lanes) and rows that are not owned (a segment's 2K extra
// rows, extension rows, ghost words) touch no envelope memory, and an owning lane whose masked chain is zero sends
// nothing either.  Ownership partitions the tile, the interior and the bands of a split pass own disjoint words, so
// every envelope word has one writer per pass.
//
// The owned rows' chains are complete.  The first owned row has t = Ao >= K.  Level l outputs it in iteration
// t + l + 1 >= K + l + 1 >= 2l + 2 (l <= K - 1), the first iteration in which level l is called at all; so every level
// has put the row's output into the chain, and the hand-over it reads was made one iteration earlier, in iteration
// t + l >= 2 (l - 1) + 2, by a level l - 1 that was called.  Rows before Ao may carry incomplete chains (zeros from
// the tally's start); they are not owned.
//
// Kept: a vector atomic OR without return (global_atomic_or_x2), not a load / OR / store.  The atomic needs no
// wait for the old word in the loop, whose vmcnt waits are the row prefetch's; the read-modify-write is made in L2.
// The load / OR / store form, built and measured beside it on HighLife at K = 8, was slower: 5.49 against 5.31 us/gen
// at 8192^2, 33.76 against 29.57 at 32768^2 (docs/PERFORMANCE.md section 28).
//
// envelope == nullptr skips the memory access (uniformly): the engine's init-time timing launches, schedule timing
// and the hinted run's prediction.
//
// BOUNDED: the edge mask on the input and on every level, as in the other policies.  Depths K = 1 .. 8, both row
// modes, MASK_UNI / MASK_LANE by one_row0; registers: docs/PERFORMANCE.md section 28.
#include "rule_launch.hpp"
#include "rule_policies.hpp"

namespace gol {
namespace hipk {

namespace {

template <int K, int ROWS, bool BOUNDED>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_envelope(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                      const LaneDesc* __restrict__ plan, StepParams p,
                                                                      RuleMasks rm, TileArgs ta, EnvelopeArgs ea) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    if (one_row0(d)) {
        RuleRunner<K, ROWS, EnvelopePolicy<K, MASK_UNI, BOUNDED>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta, ea);
        w.run();
    } else {
        RuleRunner<K, ROWS, EnvelopePolicy<K, MASK_LANE, BOUNDED>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta, ea);
        w.run();
    }
}

const void* envelope_kernel_of(Nbhd nbhd, int k, u32 flags, bool bounded) {
    if (nbhd != Nbhd::Moore) return nbhd_envelope_kernel(nbhd, k, flags, bounded);
    return kernel_of(k, flags, [bounded](auto K, auto ROWS) {
        return bounded ? (const void*)step_envelope<K(), ROWS(), true> : (const void*)step_envelope<K(), ROWS(), false>;
    });
}

}  // namespace

int max_envelope_depth(Nbhd) { return kMaxRuleDepth; }

int envelope_blocks_per_cu(int k, u32 flags, bool bounded, Nbhd nbhd) {
    return blocks_per_cu(envelope_kernel_of(nbhd, k, flags, bounded));
}

void launch_step_envelope(int k, const Rule& rule, const BoardEdges& place, bool bounded, i64 tile_cols, const u64* src, u64* dst,
                          u64* env, const LaneDesc* plan, i64 n_waves, const StepParams& p, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_envelope has no seam-reading variant (sub-tiles do not run envelope mode)");
    check_rule_masks("step_envelope", rule);
    check_place("step_envelope", place);
    check_tile_cols("step_envelope", tile_cols, p);
    const void* f = envelope_kernel_of(rule.nbhd, k, p.flags, bounded);
    if (!f) throw Error(strprintf("no envelope kernel instantiated for depth %d (1..%d)", k, kMaxRuleDepth));
    const EnvelopeArgs ea{env};
    launch_generic("envelope", f, rule, src, dst, plan, n_waves, p, s, tile_args(&place, tile_cols, p), ea);
}

}  // namespace hipk
}  // namespace gol
