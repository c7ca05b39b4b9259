// gol-mi355x: step_density<K, ROWS, BOUNDED> -- step_rule / step_rule_bounded that also counts the live cells of every
// block of the board after every generation it computes (density-film mode), for gfx950 (CDNA4).
//
// A temporal-blocked pass keeps generations 1 .. K - 1 in registers only, so the density map of each generation can
// be counted nowhere but here.  The count is the census's (census_kernel.hip): a masked v_bcnt_u32_b32 of each half
// of a level's output into one u32 accumulator per level and lane.  The census keeps that accumulator to the end of
// the wave; here it is flushed whenever the wave leaves a block of the map:
//     maps[l * slot + block_row * grid_cols + block_col] += acc[l];  acc[l] = 0        (one u32 atomic, if acc[l] != 0)
// A map (gol/density_film.hpp) is density()'s grid of u32 counts; the slot of a generation is zeroed by the engine,
// and waves, the two streams of a split pass and the ranks of a job add into it in any order.
//
// Addressing.  block_cols is a multiple of 64, so a lane's word lies in one block column, (gword0 + col) /
// block_words, formed once.  An owned row (OwnMask) is a row of the tile, hence of the board: its global row is
// gb + t with gb = grow0 + row0 - K and t the unwrapped row counter, without a wrap.  Divisions are a multiply-high
// by a reciprocal the host computes and one correction (div_recip: exact for every u32, so any block_rows >= 1
// works), and the loop holds none: the place of level 0's row in its block row is a counter that starts again at
// every block end, and level m meets the row that level 0 met m iterations before, so "this level's row ends a
// block row" is one bit per level in a register that moves up by one per row (DensityPolicy::row_phase).  A row
// iteration costs the counter's step and one test of that register; when a bit is set, the level's count is flushed
// at the start of the next iteration, and only there is the block row (gb + t) / block_rows taken.  In a MASK_UNI
// wave the counter, the register, the test and its branch are scalar; in a MASK_LANE wave they are per lane.  (A
// first version divided once per level and row and branched on each remainder: 24 branches per row triple cut the
// K = 8 loop into as many blocks; docs/PERFORMANCE.md section 26 has both measurements.)
//
// Why a flushed count lands in the right block.  acc[l] holds owned cells only, and owned rows are consecutive.  A
// count that is not zero at the end row of a block was gathered since the last block end, so in that same block:
// either the end row is owned, or it is the first block end after the last owned row, the end of the block that row
// lies in (gb + t runs on linearly past the tile and past the board's last row: the block row of a partial last
// block is still its own).  On rows before the first owned row, where gb + t may be negative and the counter has
// not yet reached the phase it is started for, the count is zero and nothing is added.  Every level meets the last
// owned row before the wave ends, so what is left then (a block end met in the last iteration included) lies in the
// block of that row, and finish() adds it there.  So an atomic's index is that of a block holding an owned cell:
// below grid_rows * grid_cols, and the launcher checks that the pass's K slots lie inside the caller's buffer.
//
// Contention.  Atomics on one cache line complete one after the other (census_kernel.hip), and the waves of a pass
// end together.  Where a block is several words wide, the lanes of one block column therefore add their counts up
// over the lanes first (run_sum: six ds_bpermute steps along a run of lanes with one block) and the run's first lane
// adds the sum: at the wave's end always, at a block end inside the loop in a MASK_UNI wave, where every lane flushes
// at once into one block row.  With one atomic per lane, 512 x 512 blocks cost 18.8 us a generation at 8192^2
// against the census's 5.5; with the sums 6.8.  Several copies of a map per slot, a wave adding into copy  wave id
// mod 16  as the census's stripes do, measured no faster (6.75 against 6.78) and are not here.
// docs/PERFORMANCE.md section 26.
//
// Uncounted cells are the census's: halo lanes, a segment's 2K extra rows, extension rows and ghost words are
// computed and never counted; the ownership argument of census_kernel.hip carries over unchanged.
//
// maps == nullptr skips the flushes (uniformly): the engine's init-time timing launches.
//
// Depths K = 1 .. 8, both row modes, both boundaries; registers: docs/PERFORMANCE.md section 26.
#include "rule_launch.hpp"
#include "rule_policies.hpp"

namespace gol {
namespace hipk {

namespace {

template <int K, int ROWS, bool BOUNDED>
__global__ __launch_bounds__(64 * kWavesPerBlock) void step_density(const u64* __restrict__ src, u64* __restrict__ dst,
                                                                     const LaneDesc* __restrict__ plan, StepParams p,
                                                                     RuleMasks rm, TileArgs ta, DensityArgs da) {
    const int wv = threadIdx.x >> 6;
    const i64 wave = (i64)blockIdx.x * kWavesPerBlock + wv;
    const int lane = threadIdx.x & 63;
    const LaneDesc d = plan[wave * kWaveLanes + lane];
    const int nrows = __builtin_amdgcn_readfirstlane(d.nrows);
    if (nrows <= 0) return;  // padding wave (uniform)
    if (one_row0(d)) {
        RuleRunner<K, ROWS, DensityPolicy<K, MASK_UNI, BOUNDED>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta, da);
        w.run();
        w.policy.finish(w.tally);
    } else {
        RuleRunner<K, ROWS, DensityPolicy<K, MASK_LANE, BOUNDED>> w(src, dst, d, nrows, p, wave, RuleGates(rm), ta, da);
        w.run();
        w.policy.finish(w.tally);
    }
}

const void* density_kernel_of(Nbhd nbhd, int k, u32 flags, bool bounded) {
    if (nbhd != Nbhd::Moore) return nbhd_density_kernel(nbhd, k, flags, bounded);
    return kernel_of(k, flags, [bounded](auto K, auto ROWS) {
        return bounded ? (const void*)step_density<K(), ROWS(), true> : (const void*)step_density<K(), ROWS(), false>;
    });
}

}  // namespace

int max_density_depth(Nbhd) { return kMaxRuleDepth; }

int density_blocks_per_cu(int k, u32 flags, bool bounded, Nbhd nbhd) {
    return blocks_per_cu(density_kernel_of(nbhd, k, flags, bounded));
}

void launch_step_density(int k, const Rule& rule, const BoardEdges& place, bool bounded, i64 tile_cols, const u64* src, u64* dst,
                         const LaneDesc* plan, i64 n_waves, const StepParams& p, const DensityGeo& grid, u64* maps,
                         i64 maps_words, hipStream_t s) {
    if (p.flags & STEP_SEAM) throw Error("step_density has no seam-reading variant (sub-tiles do not run density-film mode)");
    check_rule_masks("step_density", rule);
    check_place("step_density", place);
    check_tile_cols("step_density", tile_cols, p);
    // the maps: the grid is the board's under these blocks, and the pass's k slots lie inside what the caller owns
    const i64 gwords = ceil_div(place.cols, 64);
    if (place.rows >= ((i64)1 << 30) || gwords >= ((i64)1 << 30) || grid.block_rows < 1 || grid.block_rows > place.rows ||
        grid.block_words < 1 || grid.block_words > gwords || grid.grid_rows != ceil_div(place.rows, grid.block_rows) ||
        grid.grid_cols != ceil_div(gwords, grid.block_words) || grid.grid_rows > ((i64)1 << 20) / grid.grid_cols)
        throw Error(strprintf("step_density: blocks of %lld rows x %lld words in a grid of %lld x %lld do not fit the %lld x %lld board "
                              "(at most 2^20 blocks, blocks no larger than the board)",
                              (long long)grid.block_rows, (long long)grid.block_words, (long long)grid.grid_rows,
                              (long long)grid.grid_cols, (long long)place.rows, (long long)place.cols));
    const i64 slot = grid.slot_words();
    if (k < 1 || k > kMaxRuleDepth) throw Error(strprintf("no density kernel instantiated for depth %d (1..%d)", k, kMaxRuleDepth));
    if (maps && maps_words < (i64)k * slot)
        throw Error(strprintf("step_density: %d maps of %lld words do not fit the %lld words left in the map buffer", k,
                              (long long)slot, (long long)maps_words));
    const void* f = density_kernel_of(rule.nbhd, k, p.flags, bounded);
    if (!f) throw Error(strprintf("no density kernel instantiated for depth %d (1..%d)", k, kMaxRuleDepth));
    const DensityArgs da{reinterpret_cast<u32*>(maps), (u32)(2 * slot),          (u32)grid.block_rows, recip_of((u32)grid.block_rows),
                         (u32)grid.block_words,         recip_of((u32)grid.block_words), (u32)grid.grid_cols};
    launch_generic("density", f, rule, src, dst, plan, n_waves, p, s, tile_args(&place, tile_cols, p), da);
}

}  // namespace hipk
}  // namespace gol
