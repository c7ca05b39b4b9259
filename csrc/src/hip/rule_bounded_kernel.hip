// gol-mi355x: step_rule_bounded<K> -- step_rule (rule_kernel.hip) on a bounded board for gfx950 (CDNA4).
//
// A bounded board (Boundary::Dead) has no neighbours beyond its edges: every cell outside [0, H) x [0, W) of
// the GLOBAL board is dead in every generation.  A temporal-blocked pass runs K generations inside registers,
// so clearing the halos before the pass is not enough: a cell just outside the edge is born from inside cells
// at level 1 and feeds back at level 2.  This kernel masks the loaded row ("level 0") and the output of every
// level with the in-board cells of the word the lane streams: the streaming wave of rule_runner.hpp with the edge
// mask as its policy (EdgeMask there: the column and row masks, one and3 per word half and level, and the choice
// between scalar and per-lane row masks per wave).  Plans, StepParams, loads and stores are step_rule's.
//
// Depths K = 1 .. 8, both row modes, as step_rule.
#include "rule_launch.hpp"
#include "rule_policies.hpp"

namespace gol {
namespace hipk {

namespace {

template <int K, int ROWS>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_rule_bounded(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                          const LaneDesc* __restrict__ plan, StepParams p,
                                                                          RuleMasks rm, TileArgs ta) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    if (one_row0(d)) {
        RuleRunner<K, ROWS, EdgePolicy<K, MASK_UNI>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta);
        w.run();
    } else {
        RuleRunner<K, ROWS, EdgePolicy<K, MASK_LANE>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta);
        w.run();
    }
}

const void* bounded_kernel_of(Nbhd nbhd, int k, u32 flags) {
    if (nbhd != Nbhd::Moore) return nbhd_bounded_kernel(nbhd, k, flags);
    return kernel_of(k, flags, [](auto K, auto ROWS) { return (const void*)step_rule_bounded<K(), ROWS()>; });
}

}  // namespace

int rule_bounded_blocks_per_cu(int k, u32 flags, Nbhd nbhd) { return blocks_per_cu(bounded_kernel_of(nbhd, k, flags)); }

void launch_step_rule_bounded(int k, const Rule& rule, const BoardEdges& edges, const u64* src, u64* dst,
                              const LaneDesc* plan, i64 n_waves, const StepParams& p, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_rule_bounded has no seam-reading variant (sub-tiles run the torus only)");
    check_rule_masks("step_rule_bounded", rule);
    check_place("step_rule_bounded", edges);
    const void* f = bounded_kernel_of(rule.nbhd, k, p.flags);
    if (!f) throw Error(strprintf("no bounded rule kernel instantiated for depth %d", k));
    launch_generic("bounded rule", f, rule, src, dst, plan, n_waves, p, s, tile_args(&edges, 0, p));
}

}  // namespace hipk
}  // namespace gol
