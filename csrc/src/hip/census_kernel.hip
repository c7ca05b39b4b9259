// gol-mi355x: step_census<K, ROWS, BOUNDED> -- step_rule / step_rule_bounded that also counts the live cells of
// every generation it computes, for gfx950 (CDNA4).
//
// A temporal-blocked pass keeps generations 1 .. K - 1 in registers only, so the population of each generation can
// be counted nowhere but here.  Each level's output is already in two VGPRs (the word's even and odd cells); the
// count is a masked v_bcnt_u32_b32 of each into one accumulator per level:
//     acc[l] = bcnt(lo & own_lo & own_row, bcnt(hi & own_hi & own_row, acc[l]))      (2 v_bitop3 + 2 v_bcnt)
// and at the end of the wave each acc[l] is summed over the lanes and one lane adds it to the slot of level l with
// one 64-bit atomic: K atomics per wave, no other memory traffic.  A generation's slot is kCensusStripes partial
// sums, each on a 128-byte line of its own (the host adds them up); a wave adds into stripe  wave id mod
// kCensusStripes.  Atomics on one cache line complete one after the other, about 12-16 ns each, and the waves of a
// one-round plan all end together: with the K slots of a pass packed into one line the 8600 atomics of an 8192^2
// pass took longer than the pass computes (17.2 us/gen against step_rule's 4.5), with one line per generation 6.6
// (docs/PERFORMANCE.md section 21).
//
// The kernel is the streaming wave of rule_runner.hpp (the gates, the level loop, the runner, the edge masks, the
// ownership masks and the choice between scalar and per-lane row tests) with the count as its policy.  Plans,
// StepParams, loads and stores are step_rule's.
//
// BOUNDED is a template parameter: on the torus the edge masks (two and3 per level, the column masks' two VGPRs
// and the loaded row's mask) are compiled out, so the torus census keeps step_rule's values in every word it
// stores (the tail bits of an unaligned last word included) and a few registers more free than a kernel handed
// "everything is inside" masks would.
//
// Ownership (OwnMask of rule_runner.hpp).  A pass computes many cells more than once: the halo lanes, the 2K extra
// rows of every segment, the extension rows -e .. h + e of the earlier passes of a multi-pass superstep, the ghost
// words those passes store in the 2-D layout.  A cell of the level-j output (j = 1 .. K) of row iteration i, the
// unwrapped tile row
//     t = row0 - K + i - j                       (the row counter of the bounded kernel's row mask)
// is counted iff the lane stores (LANE_STORE), its word is a word of the tile (0 <= col < nw), the bit is a cell
// of the tile (the tile's storage mask on word nw - 1) and  max(row0, 0) <= t < min(row0 + nrows, h).  The store
// lanes of the segments partition a pass's output region and the regions of a pass (full, or interior and bands)
// partition the tile plus its extension, so every cell of the tile is counted once per level.  A level output
// skipped while the pipeline fills is never an owned row (i >= K + j there, and K + j >= 2 j).
//
// counts (the slot of the pass's first generation) == nullptr skips the atomics (uniformly): the engine's init-time
// timing launches.
//
// Depths K = 1 .. 8, both row modes, both boundaries; registers: docs/PERFORMANCE.md section 21.
#include "rule_launch.hpp"
#include "rule_policies.hpp"

namespace gol {
namespace hipk {

namespace {

template <int K, int ROWS, bool BOUNDED>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_census(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                    const LaneDesc* __restrict__ plan, StepParams p,
                                                                    RuleMasks rm, TileArgs ta, u64* __restrict__ counts) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    if (one_row0(d)) {
        RuleRunner<K, ROWS, CensusPolicy<K, MASK_UNI, BOUNDED>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta);
        w.run();
        w.policy.finish(w.tally, wave, counts);
    } else {
        RuleRunner<K, ROWS, CensusPolicy<K, MASK_LANE, BOUNDED>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta);
        w.run();
        w.policy.finish(w.tally, wave, counts);
    }
}

const void* census_kernel_of(Nbhd nbhd, int k, u32 flags, bool bounded) {
    if (nbhd != Nbhd::Moore) return nbhd_census_kernel(nbhd, k, flags, bounded);
    return kernel_of(k, flags, [bounded](auto K, auto ROWS) {
        return bounded ? (const void*)step_census<K(), ROWS(), true> : (const void*)step_census<K(), ROWS(), false>;
    });
}

}  // namespace

int max_census_depth(Nbhd) { return kMaxRuleDepth; }

int census_blocks_per_cu(int k, u32 flags, bool bounded, Nbhd nbhd) {
    return blocks_per_cu(census_kernel_of(nbhd, k, flags, bounded));
}

void launch_step_census(int k, const Rule& rule, const BoardEdges* edges, i64 tile_cols, const u64* src, u64* dst,
                        const LaneDesc* plan, i64 n_waves, const StepParams& p, u64* counts, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_census has no seam-reading variant (sub-tiles do not run the census)");
    check_rule_masks("step_census", rule);
    if (edges) check_place("step_census", *edges);
    check_tile_cols("step_census", tile_cols, p);
    const void* f = census_kernel_of(rule.nbhd, k, p.flags, edges != nullptr);
    if (!f) throw Error(strprintf("no census kernel instantiated for depth %d (1..%d)", k, kMaxRuleDepth));
    launch_generic("census", f, rule, src, dst, plan, n_waves, p, s, tile_args(edges, tile_cols, p), counts);
}

}  // namespace hipk
}  // namespace gol
